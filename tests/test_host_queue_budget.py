"""The geometry ring's shape for a hardware-queue budget (uvol_ws.hpp: uvol_hw_queues_from, uvol_ring_shape) is a pure function of the
environment's two variables and the forced values, so it is checked here without a device, in the style of test_host_late_join_rule.py:
a small host program includes the header and prints its answers.  What is pinned: the budget is READ as the runtime reads it (unset or
no digits: 4; 1..32), a budget with a queue per stream gives exactly round 5's ring (6 lanes x 4 groups, an auxiliary stream per lane),
and a shorter one never gets more streams than queues."""
import os
import subprocess
import pytest
from conftest import ROOT

PROG = r"""
#include "uvol_ws.hpp"
#include <cstdio>
#include <cstring>
int main(int argc, char **argv) {
  if (argc >= 2 && strcmp(argv[1], "env") == 0) { printf("%d\n", uvol_hw_queues()); return 0; }       // what a process reads from its environment
  if (argc >= 4 && strcmp(argv[1], "parse") == 0) { printf("%d\n", uvol_hw_queues_from(strcmp(argv[2], "-") ? argv[2] : nullptr, strcmp(argv[3], "-") ? argv[3] : nullptr)); return 0; }
  // shape queues lanes_forced groups_forced aux_forced
  const UvolRingShape s = uvol_ring_shape(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
  printf("%d %d %d\n", s.lanes, s.groups, (int)s.shared_aux);
  return 0;
}
"""
BUDGETS = [1, 2, 3, 4, 8, 13, 14, 24, 32]


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    d = tmp_path_factory.mktemp("queue_budget"); src = d / "rule.cpp"; exe = d / "rule"
    src.write_text(PROG)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "universal-volumetric_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


def shape(rule, q, lanes=0, groups=0, aux=-1):
    l, g, a = subprocess.check_output([rule, "shape", str(q), str(lanes), str(groups), str(aux)], text=True).split()
    return int(l), int(g), a == "1"


def test_queue_budget_is_read_like_the_runtime_reads_it(rule):
    def env(**kv):
        e = {k: v for k, v in os.environ.items() if k not in ("UVOL_HW_QUEUES", "GPU_MAX_HW_QUEUES")}; e.update(kv)
        return int(subprocess.check_output([rule, "env"], env=e, text=True))
    assert env() == 4                                                       # unset: the runtime's own default
    for junk in ("", "abc", "-3", " x7", "x"):
        assert env(GPU_MAX_HW_QUEUES=junk) == 4, junk                       # no digit to read: the default again
    assert [env(GPU_MAX_HW_QUEUES=str(q)) for q in BUDGETS] == BUDGETS
    assert env(GPU_MAX_HW_QUEUES="24") == 24 and env(GPU_MAX_HW_QUEUES="8 ") == 8 and env(GPU_MAX_HW_QUEUES="12abc") == 12
    assert env(GPU_MAX_HW_QUEUES="0") == 1 and env(GPU_MAX_HW_QUEUES="32") == 32
    # values past the clamp go to the parser as arguments: no process here gets the runtime's variable set above 32
    parse = lambda own, rt: int(subprocess.check_output([rule, "parse", own, rt], text=True))
    assert parse("-", "33") == 32 and parse("-", "99999999999999999999") == 32 and parse("40", "8") == 32 and parse("-", "0") == 1
    # the library's own variable goes first and changes nothing else; garbage in it falls through to the runtime's
    assert env(UVOL_HW_QUEUES="2", GPU_MAX_HW_QUEUES="24") == 2 and env(UVOL_HW_QUEUES="24") == 24 and env(UVOL_HW_QUEUES="zz", GPU_MAX_HW_QUEUES="8") == 8
    assert subprocess.check_output([rule, "parse", "-", "-"], text=True).strip() == "4"


def test_roomy_budgets_keep_the_ring_of_six_lanes_and_four_groups(rule):
    for q in (13, 14, 24, 32):                                              # 2 x 6 streams and one queue for the rest of the process
        assert shape(rule, q) == (6, 4, False), q
    # forced values where the queues are plentiful: taken as they are, the auxiliary stream per lane unless that is forced too
    assert shape(rule, 24, lanes=3) == (3, 4, False) and shape(rule, 24, groups=2) == (6, 2, False) and shape(rule, 24, lanes=8, groups=5) == (8, 5, False)
    assert shape(rule, 24, aux=1) == (6, 4, True) and shape(rule, 24, aux=0) == (6, 4, False)


def test_short_budgets_never_get_more_streams_than_queues(rule):
    """No shape the rule returns by itself has more main streams plus auxiliary streams than the budget allows, except at a budget of
    1 (where one lane's two streams share the one queue whatever the library does): every budget of 1 to 32 is asked, not the listed
    ones only.  A short budget gets the shared auxiliary stream and at most three lanes, the one ring that was measured
    (profiles/r10_queue_budget.json)."""
    got = {q: shape(rule, q) for q in range(1, 33)}
    for q, (lanes, groups, shared) in got.items():
        streams = lanes + (1 if shared else lanes)
        assert 1 <= groups <= lanes <= 6, (q, got[q])
        if q > 1:
            assert streams <= q, (q, got[q])
        if 1 < q < 13:
            assert shared and lanes <= 3, (q, got[q])
            # 1.5 calls' worth of frames in flight at the most, one call's worth at the least
            assert 2 * lanes <= 3 * groups and groups <= lanes, (q, got[q])
    assert got[1] == (1, 1, False) and got[2] == (1, 1, True) and got[3] == (2, 2, True)
    assert all(got[q] == (3, 2, True) for q in range(4, 13)) and all(got[q] == (6, 4, False) for q in range(13, 33))
    # either auxiliary form forced on a short budget: the lanes stay
    for q in (2, 3, 4, 8):
        assert shape(rule, q, aux=0) == got[q][:2] + (False,) and shape(rule, q, aux=1) == got[q][:2] + (True,), q
    # forced lanes and groups hold on any budget; their auxiliary stream is the shared one where the ring then fits the budget
    for q in (1, 2, 4, 8):
        assert shape(rule, q, lanes=6, groups=4) == (6, 4, q == 8) and shape(rule, q, lanes=3, groups=2) == (3, 2, q == 4)      # (3 x 2 streams fit beside one queue of 8)
        assert shape(rule, q, lanes=3, groups=2, aux=1) == (3, 2, True) and shape(rule, q, lanes=3, groups=2, aux=0) == (3, 2, False)
    assert shape(rule, 8, lanes=3) == (3, 4, False) and shape(rule, 4, lanes=1) == (1, 4, False) and shape(rule, 4, lanes=2) == (2, 4, True)
    assert shape(rule, 4, groups=1) == (3, 1, True) and shape(rule, 4, lanes=99) == (16, 4, False)
