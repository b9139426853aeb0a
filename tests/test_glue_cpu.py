"""INTEGRATION.md, compiled: the binding (lamsa_amd/glue/lamsa_hp_glue.c) and the edits of tools/apply_glue.py applied to a
scratch copy of the reference, built with -DLAMSA_HP (oracle/_ref/lamsa_glued, `make -C oracle glued`) and run on the CPU
emulation of the C-ABI instead of liblamsa_hp.so.  The reference binary -- its own file IO, GEM parsing, stage (4), ranking and
SAM writer, with stages (2),(3),(2'),(3') coming through include/lamsa_hp.h -- must write the SAM it wrote before.

Needs oracle/_ref/lamsa_glued, which build() makes only where the reference's sources are: skipped elsewhere."""
import os
import subprocess

import pytest

import goldenlib as G
import reflib

ROOT = reflib.ROOT
GLUED = os.path.join(ROOT, "oracle", "_ref", "lamsa_glued")

pytestmark = pytest.mark.skipif(not os.path.exists(GLUED), reason="oracle/_ref/lamsa_glued was not built (needs the reference's sources)")


@pytest.fixture(scope="module")
def glued(tmp_path_factory):
    """(binary, environment): the glued reference with liblamsa_hp.so resolved to the emulated C-ABI.  The binary finds its
    library through a RUNPATH, which LD_LIBRARY_PATH precedes."""
    d = tmp_path_factory.mktemp("glue")
    os.symlink(reflib.emu_capi_lib(), str(d / "liblamsa_hp.so"))
    env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join([str(d)] + [p for p in os.environ.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p]))
    return GLUED, env


@pytest.mark.parametrize("name", ("c3_ont", "c5_sv", "c6_edge", "c7_rescue"))
def test_reference_with_the_binding_writes_the_same_sam(glued, name, tmp_path):
    ref, reads, args, gold_r0 = G.stage_scenario(name, str(tmp_path))
    gold = G.golden_full(name) if name in G.RESCUE_SCENARIOS else gold_r0          # default run: stage (4) on
    out = str(tmp_path / "out.sam")
    exe, env = glued
    p = subprocess.run([exe, "aln"] + args + ["-t", "3", "-N", ref, reads, "-o", out], capture_output=True, text=True, timeout=1500, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    assert G.strip_pg(open(out).read()) == G.strip_pg(gold)
