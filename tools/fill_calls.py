#!/usr/bin/env python3
"""Dynamic calls per line of the non-inlined routines of the gap fill, counted on the CPU lane emulation (no GPU): the HP_STAT slots
26-31 of the device sources (merge_cigar_full, frag_extend_multi, split_sv, split_mismatch, split_indel_map, ksw_bi_extend) over a
simulated batch shaped like a bench.py workload.  ksw_bi_extend is counted in every launch (the wave-per-job launch calls it too).
usage: tools/fill_calls.py [workload] [reads]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import bench            # noqa: E402
import reflib           # noqa: E402
import simbatch         # noqa: E402
from lamsa_amd import hp   # noqa: E402

NAMES = {26: "merge_cigar_full", 27: "frag_extend_multi", 28: "split_sv", 29: "split_mismatch", 30: "split_indel_map", 31: "ksw_bi_extend (all launches)"}


def main():
    w = sys.argv[1] if len(sys.argv) > 1 else "ont10k"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    wl = bench.WORKLOADS[w]
    ref = simbatch.SimRef(8_000_000, n_contigs=2, seed=3, threads=4)
    B = simbatch.SimBatch(ref, n, wl["length"], wl["profile"], seed=11, threads=4)
    stats = []
    got, st = reflib.emu_streams(B, hp.make_para(wl["read_type"], **wl["over"]), stats=stats)
    lines = sum(g[1] + g[2] for g in got if len(g) > 3)
    print("%s: %d reads, %d not ok, %d lines" % (w, n, int((st != 0).sum()), lines))
    for k in sorted(NAMES):
        print("  %-30s %8d calls  %7.2f per line" % (NAMES[k], stats[k], stats[k] / max(lines, 1)))


if __name__ == "__main__":
    main()
