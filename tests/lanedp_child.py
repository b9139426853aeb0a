"""Child process of tests/test_lanedp_stages_gpu.py (test infrastructure, not a test): LAMSA_HP_LANE_STAGES is read once per process, so the lane
DP in two stages and in one each get a fresh one.

    python lanedp_child.py sets PRESET OUT.npz      every job set of tests/lanedp_jobs.py for the preset through lamsa_hp_dp_batch, kinds 12 / 13
    python lanedp_child.py reads NAME OUT.npz       the reads of the golden scenario NAME through align_batch

OUT.npz receives, per set, the CIGAR words and their lengths, the status, cells and hard-queue flag of every job -- or the result streams and the
status words of the reads -- and the seconds the GPU calls took."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def flat(lists):
    ln = np.array([len(s) for s in lists], np.int64)
    return np.array([w for s in lists for w in s], np.int32), ln


def unflat(words, ln):
    off = np.concatenate([[0], np.cumsum(ln)])
    return [words[off[i]:off[i + 1]].tolist() for i in range(len(ln))]


def set_key(size, mix):
    return "s%d_%s" % (size, mix.replace("-", "_"))


def run_sets(preset, dst):
    import lanedp_jobs as LJ
    from lamsa_amd import hp
    out, secs = {}, 0.0
    h = hp.LamsaHp(hp.make_para(preset))
    try:
        for size in LJ.SIZES:
            for mix in LJ.MIXES:
                jobs, types, _ = LJ.job_set(preset, size, mix)
                t0 = time.time()
                got = h.dp_batch(jobs, types + 11, 0, 100)
                secs += time.time() - t0
                k = set_key(size, mix)
                out[k + "_words"], out[k + "_len"] = flat(got["cigars"])
                out[k + "_status"] = np.asarray(got["status"], np.int32); out[k + "_cells"] = np.asarray(got["qle"], np.int32); out[k + "_hard"] = np.asarray(got["tle"], np.int32)
    finally:
        h.close()
    out["seconds"] = np.array([secs], np.float64)
    np.savez(dst, **out)


def run_reads(name, dst):
    import goldenlib
    import reflib
    from lamsa_amd import hp
    with tempfile.TemporaryDirectory() as tmp:
        ref, reads, args, _ = goldenlib.stage_scenario(name, tmp)
        rt, over = goldenlib.para_from_args(args)
        B = reflib.Batch(ref, reads, reflib.lo_para(rt, **over))
        h = hp.LamsaHp(hp.make_para(rt, **over), ref=(B.pac, B.l_pac, B.seq_off, B.seq_len))
        try:
            t0 = time.time()
            got, st = h.align_batch(B)
            secs = time.time() - t0
        finally:
            h.close()
    out = {"seconds": np.array([secs], np.float64), "status": np.asarray(st, np.int32)}
    out["words"], out["len"] = flat(got)
    np.savez(dst, **out)


if __name__ == "__main__":
    (run_sets if sys.argv[1] == "sets" else run_reads)(sys.argv[2], sys.argv[3])
