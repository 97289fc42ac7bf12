"""The rule that lets a call of more than 1200 frames join its valence replay late (geom_encode.hip, geo_submit_impl): the arithmetic is
a pure function of the workspace size, what the ring's lanes hold, and the device's free / total memory (uvol_ws.hpp), so it is checked
here without a device: a small host program includes the header and prints its answers, the expected ones are worked out in Python from
the rule as documented (a lane that is too small is re-allocated with uvol_ensure's slack; a sixteenth of the device stays free)."""
import subprocess
import os
from conftest import ROOT

PROG = r"""
#include "uvol_ws.hpp"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv) {
  // argv: ws free total cap...
  const size_t ws = strtoull(argv[1], 0, 10), fr = strtoull(argv[2], 0, 10), tot = strtoull(argv[3], 0, 10);
  std::vector<size_t> caps; for (int i = 4; i < argc; i++) caps.push_back(strtoull(argv[i], 0, 10));
  printf("%zu %d\n", uvol_ws_alloc_size(ws), (int)uvol_ws_ring_fits(ws, caps, fr, tot));
  return 0;
}
"""


def alloc_size(b):
    return b + min(b // 8, 256 << 20) + 4096


def test_late_join_rule_on_the_host(tmp_path):
    src = tmp_path / "rule.cpp"; exe = tmp_path / "rule"
    src.write_text(PROG)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "universal-volumetric_amd", "csrc"), str(src), "-o", str(exe)])

    def ask(ws, free, total, caps):
        a, f = subprocess.check_output([str(exe), str(ws), str(free), str(total)] + [str(c) for c in caps], text=True).split()
        assert int(a) == alloc_size(ws)
        return f == "1"

    total = 288 * 10 ** 9; spare = total // 16
    ws = 22 * 10 ** 9                                       # 640 frames of 34 MB
    # a ring of six lanes that hold nothing: six allocations with their slack, and exactly the spare sixteenth on top
    grow = 6 * alloc_size(ws)
    assert ask(ws, grow + spare, total, [0] * 6) and not ask(ws, grow + spare - 1, total, [0] * 6)
    # lanes sized for the early layout (19 GB each, with slack) give their buffers back first: the ring grows by the differences
    early = alloc_size(19 * 10 ** 9); grow = 6 * (alloc_size(ws) - early)
    assert ask(ws, grow + spare, total, [early] * 6) and not ask(ws, grow + spare - 1, total, [early] * 6)
    # a ring that is large enough already: nothing is allocated, the answer is 'late' whatever is free
    assert ask(ws, 0, total, [alloc_size(ws)] * 6) and ask(ws, 0, total, [ws] * 6)
    # one lane short by one byte, the others large enough: only that lane counts
    assert ask(ws, alloc_size(ws) - (ws - 1) + spare, total, [ws] * 5 + [ws - 1]) and not ask(ws, alloc_size(ws) - (ws - 1) + spare - 1, total, [ws] * 5 + [ws - 1])
    # the slack: an eighth for small buffers, 256 MiB at most
    assert ask(8000, 2 * 10 ** 9, 16 * 10 ** 9, [0]) and alloc_size(8000) == 8000 + 1000 + 4096 and alloc_size(ws) == ws + (256 << 20) + 4096
