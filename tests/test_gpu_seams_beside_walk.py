"""The early and the late join of a lane's auxiliary stream (valence replay) on the MI355X: here the two streams really run side by side,
and with the late join the replay's inputs must stay clear of the record tables the traversals read meanwhile
(tests/test_hipemu_seams_beside_walk.py checks the data flow without a GPU).  The 19 frames are small: they run the LDS walkers on
per-corner records, not the bench's compact layout with per-face records, and the join is forced by UVOL_LATE_JOIN - the memory rule that
chooses it for large calls is checked on the host (tests/test_host_late_join_rule.py) and reached by large calls only."""
import os
import subprocess
import sys
import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu

CODE = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
        "import torch, uvol, oracle as O, material_cases as MC, seams_beside_walk_cases as SC\n"
        "O.lib()\n"
        "fs = [MC.plain(f) for f in SC.frames()]\n"
        "want = [SC.oracle_bytes(O, f) for f in fs]\n"
        "keep, ms = [], []\n"
        "for f in fs:\n"
        "    m, arrs = uvol.Codec._mesh_host(**f)\n"
        "    dev = [None if a is None else torch.from_numpy(a).cuda() for a in arrs]; keep.append(dev)\n"
        "    pos, uv, nrm, ip, iu, inr = dev\n"
        "    m.pos = pos.data_ptr(); m.idx_pos = ip.data_ptr()\n"
        "    if uv is not None: m.uv = uv.data_ptr(); m.idx_uv = iu.data_ptr()\n"
        "    if nrm is not None: m.nrm = nrm.data_ptr(); m.idx_nrm = inr.data_ptr()\n"
        "    ms.append(m)\n"
        "torch.cuda.synchronize()\n"
        "arr = (uvol.Mesh * len(ms))(*ms)\n"
        "cd = uvol.Codec(device=0)\n"
        "cd.start_mesh_batch_dev(arr, slot=0); cd.start_mesh_batch_dev(arr, slot=1)\n"
        "res = cd.finish(); cd.close()\n"
        "assert len(res) == 2\n"
        "for rr in res:\n"
        "    assert len(rr) == len(want)\n"
        "    for i, r in enumerate(rr): assert r is not None and bytes(r) == want[i], i\n"
        "print('ok')\n")


@pytest.mark.parametrize("late", ["0", "1"])
def test_gpu_seams_beside_walk_two_passes_on_one_context(late):
    """The 19-frame batch of seams_beside_walk_cases, resident in HBM, through start_mesh_batch_dev twice on one context (output slots 0
    and 1), then finish(): both passes are byte-equal to the oracle, with the join of the auxiliary stream forced early and late (read
    once per process, hence the fresh interpreter).  A call is cut into four groups (UVOL_GEO_MIN_GROUP=4) on the ring of six lanes, so
    the second pass starts on the two lanes the first left free and then takes lanes - and their auxiliary streams - whose first-pass
    outputs have not been fetched by the caller yet.  The device entry point has no material argument:
    the frame that carries ids in the emulation test goes in as the plain torus it is."""
    code = CODE % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "universal-volumetric_amd"), os.path.join(ROOT, "oracle"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, UVOL_LATE_JOIN=late, UVOL_GEO_MIN_GROUP="4"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])
