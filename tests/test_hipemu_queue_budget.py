"""The geometry ring shaped for a budget of hardware queues (geom_encode.hip: geo_ring; uvol_ws.hpp: uvol_ring_shape) through the host
emulation of the kernels (tests/hipemu, no GPU): budgets of 2, 4 and 24 queues give rings of 1, 3 and 6 lanes, the ring of 4 queues
with every lane's valence replay on ONE auxiliary stream of the context, and the results are the oracle's bytes in all of them (tests/queue_budget_cases.py: the
six frames around the refused one of the 19-frame batch - one enqueued call, two back to back, then calls of 6 / 3 / 6 / 5 frames on one context).  The emulation runs the streams one
after the other in the order of the enqueue, so this checks the data flow and the host side - lanes, events, workspaces and their cached
placements, the shared stream's creation and destruction -, not the concurrency: that is tests/test_gpu_queue_budget.py."""
import os
import subprocess
import sys
import pytest
from conftest import ROOT
import queue_budget_cases as QC


@pytest.mark.parametrize("late", QC.JOINS)
@pytest.mark.parametrize("queues", QC.QUEUES)
def test_hipemu_queue_budget_enqueued_calls(hipemu_lib, queues, late):
    """UVOL_HW_QUEUES = 2 / 4 / 24 with the join of the auxiliary stream forced early and late; the switches are read once per process,
    hence the fresh interpreter.  UVOL_DEBUG=1 makes the library say which ring it chose."""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import uvol, oracle as O, queue_budget_cases as QC\n"
            "O.lib(); cd = uvol.Codec(lib_path=%r)\n"
            "QC.run_all(O, cd, **QC.EMU); cd.close(); print('ok')\n") % (
                os.path.join(ROOT, "tests"), os.path.join(ROOT, "universal-volumetric_amd"), os.path.join(ROOT, "oracle"), hipemu_lib)
    r = subprocess.run([sys.executable, "-c", code], env=dict(QC.env_for(queues, late, QC.EMU["min_group"]), UVOL_DEBUG="1"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])
    ring = [l for l in r.stderr.splitlines() if "geometry ring:" in l]
    assert ring and QC.RING[queues] in ring[0], ring[:1]
