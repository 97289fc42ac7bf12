"""The valence replay as a row of workgroups of the traversal launch (k_traverse_wave_f16) on the MI355X.  Here the replay blocks and the
traverser blocks of one launch really run side by side, so this is where a replay array that shared bytes with something a traverser
reads or writes, or a lifetime that ended before the launch did, would show (tests/test_hipemu_fused_replay.py checks the data flow and
the indexing without a GPU).  The frames are small, so the lane-per-walker kernels are forced (UVOL_SIMT_W; large calls choose them by
themselves) and with them the per-face records of the wave form; UVOL_TIMING's line per group says which form of the replay ran and on
which records.  The switches are read once per process, hence the fresh interpreters."""
import json
import os
import re
import subprocess
import sys
import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu

PATHS = (os.path.join(ROOT, "tests"), os.path.join(ROOT, "universal-volumetric_amd"), os.path.join(ROOT, "oracle"))
HEAD = ("import sys; sys.path[:0] = [%r, %r, %r]\n" % PATHS +
        "import hashlib, json, synth, uvol, oracle as O, material_cases as MC, seams_beside_walk_cases as SC\n"
        "O.lib(); cd = uvol.Codec(device=0)\n")
BATCH = HEAD + "SC.run_batch(O, cd); cd.close(); print('ok')\n"
# 70 frames of ~2500 vertices, each its own tessellation (8 base spheres, every frame its own flipped quads and jitter)
DISTINCT = HEAD + ("fs = synth.distinct_meshes(70, 64, 41, bases=8, charts=(6, 4))\n"
                   "got = cd.encode_mesh_batch(fs); cd.close()\n"
                   "if %d:\n"
                   "    for i, f in enumerate(fs): assert got[i] == SC.oracle_bytes(O, f), i\n"
                   "print(json.dumps([hashlib.sha256(g).hexdigest() for g in got])); print('ok')\n")
# small frames on per-face records (fused) and one frame of 263,200 faces - past the 8-byte records' fields, so 16-byte corner records and
# the lane form of the traversers (auxiliary stream) - in turn on ONE context
ALTERNATE = HEAD + ("small = [MC.plain(f) for f in SC.frames()]; big = synth.sphere_mesh(400, 330)\n"
                    "want = [SC.oracle_bytes(O, f) for f in small]; want_big = SC.oracle_bytes(O, big)\n"
                    "for k in range(5):\n"
                    "    if k % 2 == 0: assert cd.encode_mesh_batch(small) == want, k\n"
                    "    else: assert cd.encode_mesh_batch([big]) == [want_big], k\n"
                    "cd.close(); print('ok')\n")


def run(code, **env):
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, UVOL_TIMING="1", **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])
    return r.stdout, re.findall(r"geo group n=(\d+) .*? join, (\w+) replay, traversal records (\d)", r.stderr)


@pytest.mark.parametrize("replay", ["fused", "aux"])
def test_gpu_fused_replay_batch_of_19(replay):
    """The 19 frames of seams_beside_walk_cases, 5 walkers per wave (four traverser blocks per table beside 19 replay blocks), in both
    forms of the replay: every good frame equals oracle.drc_encode byte for byte, the refused frame keeps its status."""
    _, groups = run(BATCH, UVOL_LATE_JOIN="1", UVOL_SIMT_W="5", UVOL_ENTROPY_W="8", UVOL_REPLAY=replay)
    assert groups and all(g[1] == replay and g[2] == "2" for g in groups), groups


def test_gpu_fused_replay_70_distinct_frames_equal_in_both_forms():
    """One call of 70 distinct frames, four walkers per wave as in the bench: 18 traverser blocks per table beside 70 replay blocks, all of
    them resident at once, so the two kinds of block overlap for the whole length of the replay.  The fused form gives the
    oracle's bytes, and the auxiliary-stream form the same bytes frame for frame."""
    out = {}
    for replay in ("fused", "aux"):
        stdout, groups = run(DISTINCT % (replay == "fused"), UVOL_SIMT_W="4", UVOL_REPLAY=replay)
        assert sum(int(g[0]) for g in groups) == 70 and all(g[1] == replay and g[2] == "2" for g in groups), groups
        out[replay] = json.loads(stdout.splitlines()[-2])
    assert len(out["fused"]) == 70 and out["fused"] == out["aux"]


def test_gpu_fused_replay_alternates_with_the_auxiliary_stream_on_one_context():
    """Fused groups first, then a group that needs the auxiliary stream, and so on: the stream is created by the first group that needs
    it, after fused groups have run on the context, and a fused group follows each use of it.  All five calls give the oracle's bytes."""
    _, groups = run(ALTERNATE, UVOL_SIMT_W="4")
    assert [g[1] for g in groups] == ["fused", "aux", "fused", "aux", "fused"], groups
    assert [g[2] for g in groups] == ["2", "0", "2", "0", "2"], groups
