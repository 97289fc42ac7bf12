"""The geometry ring shaped for a budget of hardware queues on the MI355X: rings of 1, 3 and 6 lanes for 2, 4 and 24 queues, the
ring of 4 queues with every lane's valence replay on ONE auxiliary stream of the context, beside the main streams of all lanes, so a replay of one call's group may still be queued there when a
lane takes its next group - the joins (early: before the record tables, late: behind the traversals) wait on the lane's own event, and
the workspace lifetimes are what they were.  tests/queue_budget_cases.py: one enqueued call of 19 frames cut into groups of at least
three, two such calls back to back (the ring wraps), then calls of 19 / 3 / 19 / 7 frames on one context; every good frame equals the
oracle byte for byte and the refused frame keeps its status.  UVOL_HW_QUEUES changes the library's plan only, never the runtime's queues."""
import os
import subprocess
import sys
import pytest
from conftest import ROOT
import queue_budget_cases as QC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("late", QC.JOINS)
@pytest.mark.parametrize("queues", QC.QUEUES)
def test_gpu_queue_budget_enqueued_calls(queues, late):
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import uvol, oracle as O, queue_budget_cases as QC\n"
            "O.lib(); cd = uvol.Codec(device=0)\n"
            "QC.run_all(O, cd, **QC.GPU); cd.close(); print('ok')\n") % (
                os.path.join(ROOT, "tests"), os.path.join(ROOT, "universal-volumetric_amd"), os.path.join(ROOT, "oracle"))
    r = subprocess.run([sys.executable, "-c", code], env=QC.env_for(queues, late), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])
