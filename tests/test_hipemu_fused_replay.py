"""The valence replay as a row of workgroups of the traversal launch (k_traverse_wave_f16, UVOL_REPLAY=fused: the default wherever the join
is late and the traversers run in the wave form) against the same replay on the auxiliary stream (UVOL_REPLAY=aux), through the host
emulation of the kernels (tests/hipemu, no GPU).

The emulation runs the blocks of a grid in order, one after the other: the traverser rows have run to their end before the first block of
the replay row starts.  So this proves the data flow and the indexing of the new row - which block takes which frame, that blocks past
their row's count leave, that the second half of a replay block reads what the first wrote - and NOT the concurrency: a replay block that
shared bytes with a traverser, or a lifetime that ended too early, would not show here.  That shows only on the GPU
(tests/test_gpu_fused_replay.py)."""
import os
import re
import subprocess
import sys
import pytest
from conftest import ROOT

SIMT = dict(UVOL_LATE_JOIN="1", UVOL_ENTROPY_W="8", UVOL_TIMING="1")      # UVOL_TIMING: one line per group on stderr that names the replay's form
PATHS = (os.path.join(ROOT, "tests"), os.path.join(ROOT, "universal-volumetric_amd"), os.path.join(ROOT, "oracle"))
BATCH = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
         "import uvol, oracle as O, seams_beside_walk_cases as SC\n"
         "O.lib(); cd = uvol.Codec(lib_path=%r)\n"
         "SC.run_batch(O, cd); cd.close(); print('ok')\n")
ONE = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
       "import uvol, oracle as O, seams_beside_walk_cases as SC\n"
       "O.lib(); cd = uvol.Codec(lib_path=%r)\n"
       "for f in (SC.frames()[0], SC.frames()[-1]):\n"
       "    assert cd.encode_mesh(**f) == SC.oracle_bytes(O, f)\n"
       "cd.close(); print('ok')\n")


def run(code, lib, env):
    r = subprocess.run([sys.executable, "-c", code % (PATHS + (lib,))], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])
    return re.findall(r"geo group n=(\d+) .*? join, (\w+) replay, traversal records (\d)", r.stderr)


@pytest.mark.parametrize("replay", ["fused", "aux"])
@pytest.mark.parametrize("w", ["5", "64"])
def test_hipemu_fused_replay_batch_of_19(hipemu_lib, replay, w):
    """The 19 frames of seams_beside_walk_cases (the refused frame, the positions-only frame and the open meshes among them) with the
    replay in both forms.  5 walkers per wave: four traverser blocks per table against 19 replay blocks, neither count divides; 64 per
    wave: ONE traverser block per table (fewer frames than lanes) against 19 replay blocks.  Every good frame equals oracle.drc_encode
    byte for byte, and every group ran the form that was asked for, on per-face records (the wave form's)."""
    groups = run(BATCH, hipemu_lib, dict(SIMT, UVOL_SIMT_W=w, UVOL_REPLAY=replay))
    assert groups and sum(int(g[0]) for g in groups) >= 19, groups
    assert all(g[1] == replay and g[2] == "2" for g in groups), groups


def test_hipemu_fused_replay_one_frame(hipemu_lib):
    """One-frame calls (a seamed sphere, an open grid): one traverser block per table and one replay block."""
    groups = run(ONE, hipemu_lib, dict(SIMT, UVOL_SIMT_W="5", UVOL_REPLAY="fused"))
    assert len(groups) == 2 and all(g == ("1", "fused", "2") for g in groups), groups


def test_hipemu_fused_replay_is_the_default_and_keeps_the_stream_elsewhere(hipemu_lib):
    """Without UVOL_REPLAY the wave form with the late join fuses; the early join and the LDS walkers of a small call (no UVOL_SIMT_W)
    keep the auxiliary stream whatever the switch says."""
    assert all(g[1] == "fused" for g in run(ONE, hipemu_lib, dict(SIMT, UVOL_SIMT_W="5")))
    assert all(g[1] == "aux" for g in run(ONE, hipemu_lib, dict(SIMT, UVOL_SIMT_W="5", UVOL_LATE_JOIN="0", UVOL_REPLAY="fused")))
    assert all(g[1] == "aux" and g[2] != "2" for g in run(ONE, hipemu_lib, dict(SIMT, UVOL_REPLAY="fused")))
