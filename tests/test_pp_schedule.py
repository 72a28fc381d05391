"""The workgroup order of the sixteen-query MaxSim pass (raglite_amd/csrc/pp_schedule.h, RL_OPT_PP_SCHEDULE), checked on the host: the
header is plain C++, compiled here with the host compiler, so the code under test is the code the kernel runs.

Both grid shapes must map the launch's workgroups one to one onto (row range, pass); the co-scheduled shape must put the passes of a row
range on ids equal mod 8 (one XCD) next to each other."""

import shutil
import subprocess
from pathlib import Path

import pytest

HEADER_DIR = Path(__file__).resolve().parent.parent / "raglite_amd" / "csrc"

_DRIVER = r"""
#include <cstdio>
#include "pp_schedule.h"
int main() {
    const int gxs[] = {1, 2, 7, 8, 9, 15, 16, 17, 64, 255, 256, 304};
    for (int gx : gxs)
        for (int P = 1; P <= 9; ++P) {
            for (int x = 0; x < gx * P; ++x) {  // co-scheduled: a 1-D grid of gx * P
                const rl::PpSlot m = rl::pp_schedule(x, 0, gx * P, 1, P);
                std::printf("c %d %d %d %d %d %d\n", gx, P, x, m.ranges, m.range, m.pass);
            }
            for (int y = 0; y < P; ++y)  // pass-major: grid (gx, P)
                for (int x = 0; x < gx; ++x) {
                    const rl::PpSlot m = rl::pp_schedule(x, y, gx, P, P);
                    std::printf("p %d %d %d %d %d %d\n", gx, P, y * gx + x, m.ranges, m.range, m.pass);
                }
        }
    return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("pp_schedule")
    (d / "drv.cpp").write_text(_DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", f"-I{HEADER_DIR}", str(d / "drv.cpp"), "-o", str(d / "drv")], check=True)
    out = subprocess.run([str(d / "drv")], check=True, capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        kind, gx, P, lin, ranges, rng, pas = line.split()
        rows.setdefault((kind, int(gx), int(P)), []).append((int(lin), int(ranges), int(rng), int(pas)))
    return rows


@pytest.mark.parametrize("kind", ["c", "p"])
@pytest.mark.parametrize("gx", [1, 2, 7, 8, 9, 15, 16, 17, 64, 255, 256, 304])
@pytest.mark.parametrize("P", range(1, 10))
def test_schedule_is_a_bijection(table, kind, gx, P):
    rows = table[(kind, gx, P)]
    assert len(rows) == gx * P
    assert all(ranges == gx for _, ranges, _, _ in rows)
    slots = [(rng, pas) for _, _, rng, pas in rows]
    assert all(0 <= rng < gx and 0 <= pas < P for rng, pas in slots)
    assert sorted(slots) == [(r, p) for r in range(gx) for p in range(P)]


@pytest.mark.parametrize("gx", [8, 9, 15, 16, 17, 64, 255, 256, 304])
@pytest.mark.parametrize("P", range(2, 10))
def test_coscheduled_passes_share_an_xcd_and_a_dispatch_window(table, gx, P):
    """Every range in a whole block of eight: its P ids are equal mod 8 and lie in one window of 8 P consecutive ids."""
    whole = gx & ~7
    ids = {}
    for lin, _, rng, pas in table[("c", gx, P)]:
        ids.setdefault(rng, []).append(lin)
    for rng in range(whole):
        lins = sorted(ids[rng])
        assert len({lin % 8 for lin in lins}) == 1, (rng, lins)
        assert lins[-1] - lins[0] == 8 * (P - 1), (rng, lins)
    # the ranges past the last block of eight keep the pass-major order among themselves
    rest = gx - whole
    for lin, _, rng, pas in table[("c", gx, P)]:
        if rng >= whole:
            assert lin == whole * P + pas * rest + (rng - whole)


def test_one_pass_is_the_same_grid_in_both_shapes(table):
    for gx in (1, 7, 8, 9, 255, 256):
        assert table[("c", gx, 1)] == table[("p", gx, 1)]
        assert [(lin, rng) for lin, _, rng, _ in table[("c", gx, 1)]] == [(x, x) for x in range(gx)]
