"""The main chaining pass on diagonal keys (lamsa_amd/csrc/hp_cluster.h: dp_cluster_lds / cl_targets, cluster_lane; hp_gaps.h: gap_dp_core) on the
device: the hand-made reads of tests/edge_cases.py (the same batches as tests/test_edge_cpu.py, whose path counters show which routine each read
takes) through LamsaHp.align_batch, once per shape of k_chain1 / k_chain2 (2432 / 3392 / 5120 LDS words per wave), against the oracle word for
word; a second run over the resident batch must give the same.  LAMSA_HP_CHAIN_SHAPE is read once per process, so every shape runs in a fresh
child (tests/capacity_child.py), one after the other; all reads of a shape that share parameters and reference go as one batch.  A child that
dies by a signal, aborts or runs into its time limit ends the session: nothing more is started on the GPU."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import capacity_child
import crafted
import edge_cases
import reflib

pytestmark = pytest.mark.gpu

CHILD = os.path.join(reflib.ROOT, "tests", "capacity_child.py")
# seconds a child may take.  Measured on an MI355X (profiles/edge_diag_ab.txt): 0.8 / 0.6 / 4.9 s for shapes 0 / 1 / 2, library load and
# three batches included; the limit is three times the slowest, rounded up to the next ten.
CHILD_TIMEOUT = 20


@pytest.mark.parametrize("shape", [0, 1, 2])
def test_hand_made_reads_on_the_device(shape, tmp_path):
    W = edge_cases.SHAPES[shape]
    reflib.build_oracle()
    groups = sorted(crafted.groups(edge_cases.cases(W)).items())
    packed, want = [], []
    for (read_type, over, ref_key), cs in groups:
        batch = crafted.concat([c.batch for c in cs])
        w = reflib.oracle_streams(batch, reflib.lo_para(read_type), 4)
        for c, s in zip(cs, w):
            assert s[0] == 0 and s[1] >= 1, "the oracle does not align this read: %s" % c.aim
        packed.append((read_type, over, crafted.sim_ref(ref_key), batch)); want.append(w)
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **capacity_child.pack_groups(packed))
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, CHILD, src, dst], env=dict(os.environ, LAMSA_HP_CHAIN_SHAPE=str(shape)), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        pytest.exit("the child of chaining shape %d did not finish within %d s: nothing more is run on the GPU" % (shape, CHILD_TIMEOUT), returncode=1)
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.exit("the child of chaining shape %d died (exit status %d): nothing more is run on the GPU\n%s" % (shape, p.returncode, p.stderr[-2000:]), returncode=1)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(dst)
    print("shape %d (%d words): child %.1f s, batches %s s" % (shape, W, time.time() - t0, np.round(z["seconds"], 2).tolist()))
    bad = []
    for i, ((read_type, over, ref_key), cs) in enumerate(groups):
        got = capacity_child.unflat(z["g%d_words" % i], z["g%d_len" % i]); again = capacity_child.unflat(z["g%d_words2" % i], z["g%d_len2" % i])
        st, st2 = z["g%d_status" % i], z["g%d_status2" % i]
        for k, c in enumerate(cs):
            if int(st[k]) != 0 or int(st2[k]) != 0:
                bad.append((c.key, "status", int(st[k]), int(st2[k])))
            elif got[k] != want[i][k]:
                bad.append((c.key, "differs from the oracle"))
            elif again[k] != got[k]:
                bad.append((c.key, "second run differs"))
    assert bad == []
