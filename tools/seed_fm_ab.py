#!/usr/bin/env python3
"""Seeding through the host FmIndex on the host threads against lamsa_hp_fm_seed on the GPU (run on the GPU box): builds the stand-in of
tools/default_run.py and its FM index with `lamsa index --from-pac`, then runs tools/seed_fm_ab.cpp (both in one process, the hit records
compared at 1 % error; the shares of seeded seeds and reads at 1 %, 5 % and 12 %) and prints what profiles/seed_fm_ab.txt records.
usage: tools/seed_fm_ab.py [reference bases = 300000000] [reads = 65536] [read length = 5000] [threads = 16]"""
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import simbatch   # noqa: E402
import simfiles   # noqa: E402

bp = int(sys.argv[1]) if len(sys.argv) > 1 else 300_000_000
n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
rlen = int(sys.argv[3]) if len(sys.argv) > 3 else 5000
threads = int(sys.argv[4]) if len(sys.argv) > 4 else 16


def build_tool():
    """lamsa_amd/bin/seed_fm_ab from tools/seed_fm_ab.cpp, the host's index readers and the product library."""
    host = os.path.join(ROOT, "lamsa_amd", "host")
    out = os.path.join(ROOT, "lamsa_amd", "bin", "seed_fm_ab")
    srcs = [os.path.join(ROOT, "tools", "seed_fm_ab.cpp"), os.path.join(host, "rescue.cpp"), os.path.join(host, "lamsa_host.cpp")]
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs):
        subprocess.run(["g++", "-O3", "-g", "-std=c++17", "-I", host, "-o", out] + srcs + ["-L" + os.path.join(ROOT, "lamsa_amd", "lib"), "-llamsa_hp", "-Wl,-rpath,$ORIGIN/../lib", "-lz", "-lpthread"], check=True)
    return out


if __name__ == "__main__":
    tool = build_tool()
    if bp <= 0:                     # build only
        sys.exit(0)
    simbatch.build()
    d = tempfile.mkdtemp(prefix="lamsa_seedab_", dir=os.environ.get("TMPDIR", "/tmp"))
    try:
        ref = simbatch.SimRef(bp, n_contigs=12, seed=17, threads=threads)
        simfiles.write_index(d + "/ref.fa", ref)
        t = time.time()
        q = subprocess.run([os.path.join(ROOT, "lamsa_amd", "bin", "lamsa"), "index", "--from-pac", d + "/ref.fa"], capture_output=True, text=True, env=dict(os.environ, LAMSA_INDEX_THREADS=str(threads)))
        assert q.returncode == 0, q.stderr[-2000:]
        print("# stand-in of %d bp, FM index by `lamsa index --from-pac` on %d threads in %.1f s" % (int(ref.l_pac), threads, time.time() - t), flush=True)
        p = subprocess.run(["timeout", "-k", "10", "420", tool, d + "/ref.fa", str(n_reads), str(rlen), str(threads)], capture_output=True, text=True)
        print(p.stdout, end="")
        assert p.returncode == 0, p.stderr[-2000:]
        ru = os.path.join(ROOT, "lamsa_amd", "lib", "asm", "resource_usage.txt")      # `make -C lamsa_amd/csrc asm`
        if os.path.exists(ru):
            txt = open(ru).read()
            for kname in ("k_seed_search", "k_seed_locate", "k_seed_hits", "k_seed_slot", "k_seed_emit"):
                m = re.search(r"Function Name: \S*%s\S*.*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)" % kname, txt, re.S)
                if m:
                    print("%s: %s VGPRs, %s bytes of scratch per lane, %s waves per SIMD (kernel-resource-usage remarks of hipcc)" % ((kname,) + m.groups()))
    finally:
        shutil.rmtree(d, ignore_errors=True)
