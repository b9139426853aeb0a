"""Child process of tests/test_capacity_gpu.py (test infrastructure, not a test): LAMSA_HP_CHAIN_SHAPE is read once per process, so every
shape of the chaining kernels gets a fresh one.

    python capacity_child.py IN.npz OUT.npz

IN.npz holds groups of reads -- one batch per (read type, parameters, reference) -- written by the parent (pack_groups); OUT.npz receives, per
group, the result streams and status words of align_batch and of a second run over the resident batch (upload_batch + run_uploaded), and the
seconds both took."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH_FIELDS = ("read_off", "read_seq", "seed_all", "last_len", "seed_off", "seed_id", "hit_off", "h_pos", "h_chr", "h_strand", "h_nm", "h_len_dif",
                "h_cig_off", "h_cig_n", "cig")
REF_FIELDS = ("pac", "seq_off", "seq_len")


def pack_groups(groups):
    """groups: list of (read_type, over, ref, batch) -> dict of arrays for np.savez."""
    out = {}
    meta = []
    for i, (read_type, over, ref, batch) in enumerate(groups):
        meta.append(dict(read_type=read_type, over=dict(over), n_reads=int(batch.n_reads), l_pac=int(ref.l_pac)))
        for f in BATCH_FIELDS:
            out["g%d_%s" % (i, f)] = np.ascontiguousarray(getattr(batch, f))
        for f in REF_FIELDS:
            out["g%d_ref_%s" % (i, f)] = np.ascontiguousarray(getattr(ref, f))
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    return out


def flat(streams):
    ln = np.array([len(s) for s in streams], np.int64)
    return np.array([w for s in streams for w in s], np.int32), ln


def unflat(words, ln):
    off = np.concatenate([[0], np.cumsum(ln)])
    return [words[off[i]:off[i + 1]].tolist() for i in range(len(ln))]


def main(src, dst):
    from lamsa_amd import hp

    class _B:
        pass
    z = np.load(src)
    meta = json.loads(bytes(z["meta"]).decode())
    out = {}
    secs = []
    for i, m in enumerate(meta):
        b = _B()
        b.n_reads = m["n_reads"]
        for f in BATCH_FIELDS:
            setattr(b, f, z["g%d_%s" % (i, f)])
        ref = (z["g%d_ref_pac" % i], m["l_pac"], z["g%d_ref_seq_off" % i], z["g%d_ref_seq_len" % i])
        h = hp.LamsaHp(hp.make_para(m["read_type"], **m["over"]), ref=ref)
        try:
            t0 = time.time()
            got, st = h.align_batch(b)
            h.upload_batch(b)
            again, st2 = h.run_uploaded()
            secs.append(time.time() - t0)
        finally:
            h.close()
        out["g%d_words" % i], out["g%d_len" % i] = flat(got)
        out["g%d_words2" % i], out["g%d_len2" % i] = flat(again)
        out["g%d_status" % i] = np.asarray(st, np.int32); out["g%d_status2" % i] = np.asarray(st2, np.int32)
    out["seconds"] = np.array(secs, np.float64)
    np.savez(dst, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
