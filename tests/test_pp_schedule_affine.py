"""The XCD-affine workgroup order of the sixteen-query MaxSim pass (raglite_amd/csrc/pp_schedule.h: pp_schedule_affine,
RL_OPT_PP_XCD_PASSES), checked on the host: the header is plain C++, compiled here with the host compiler, so the code under test is the
code the kernel runs.

For every width w the 1-D grid must map one to one onto (row range, pass).  Where the header says the affine order applies
(pp_affine_blocks() > 0: w in {1, 2, 4}, ranges % w == 0, at least eight passes) every id class mod 8 (one XCD under round-robin
dealing) must see exactly w passes of a block of eight passes, and the w ids that work on one range within such a pass-set must lie less
than 8 w apart.  w = 8 is the co-scheduled order of pp_schedule() id for id, and so is every case the header says falls back."""

import shutil
import subprocess
from pathlib import Path

import pytest

HEADER_DIR = Path(__file__).resolve().parent.parent / "raglite_amd" / "csrc"
GXS = [1, 2, 7, 8, 9, 15, 16, 17, 64, 255, 256, 304]
PASSES = list(range(1, 18))
WIDTHS = [1, 2, 4, 8]

_DRIVER = r"""
#include <cstdio>
#include "pp_schedule.h"
int main() {
    const int gxs[] = {1, 2, 7, 8, 9, 15, 16, 17, 64, 255, 256, 304};
    const int ws[] = {1, 2, 4, 8};
    for (int gx : gxs)
        for (int P = 1; P <= 17; ++P) {
            for (int w : ws) {
                std::printf("b %d %d %d %d\n", gx, P, w, rl::pp_affine_blocks(gx, P, w));
                for (int x = 0; x < gx * P; ++x) {
                    const rl::PpSlot m = rl::pp_schedule_affine(x, gx * P, P, w);
                    std::printf("a %d %d %d %d %d %d %d\n", gx, P, w, x, m.ranges, m.range, m.pass);
                }
            }
            for (int x = 0; x < gx * P; ++x) {  // the co-scheduled map
                const rl::PpSlot m = rl::pp_schedule(x, 0, gx * P, 1, P);
                std::printf("a %d %d 0 %d %d %d %d\n", gx, P, x, m.ranges, m.range, m.pass);
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
    d = tmp_path_factory.mktemp("pp_schedule_affine")
    (d / "drv.cpp").write_text(_DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", f"-I{HEADER_DIR}", str(d / "drv.cpp"), "-o", str(d / "drv")], check=True)
    out = subprocess.run([str(d / "drv")], check=True, capture_output=True, text=True).stdout
    maps, blocks = {}, {}
    for line in out.splitlines():
        f = line.split()
        if f[0] == "b":
            blocks[(int(f[1]), int(f[2]), int(f[3]))] = int(f[4])
        else:  # (w = 0: the co-scheduled map of pp_schedule())
            maps.setdefault((int(f[1]), int(f[2]), int(f[3])), []).append((int(f[5]), int(f[6]), int(f[7])))
    return maps, blocks


def _coscheduled(maps, gx, P):
    return maps[(gx, P, 0)]


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("gx", GXS)
def test_affine_schedule_is_a_bijection(table, gx, w):
    maps, _ = table
    for P in PASSES:
        rows = maps[(gx, P, w)]
        assert len(rows) == gx * P
        assert all(ranges == gx for ranges, _, _ in rows), (gx, P, w)
        slots = [(rng, pas) for _, rng, pas in rows]
        assert sorted(slots) == [(r, p) for r in range(gx) for p in range(P)], (gx, P, w)


def test_header_covers_what_it_says(table):
    """w in {1, 2, 4}, ranges % w == 0 and at least eight passes: every whole block of eight passes; nothing else."""
    _, blocks = table
    for (gx, P, w), n in blocks.items():
        assert n == (P // 8 if w in (1, 2, 4) and gx % w == 0 else 0), (gx, P, w)
    # the launches this order is for are covered: the headline's 256 ranges x 8 passes, and a 304-CU part's
    assert all(blocks[(gx, 8, w)] == 1 and blocks[(gx, 16, w)] == 2 for gx in (8, 16, 64, 256, 304) for w in (1, 2, 4))


@pytest.mark.parametrize("w", [1, 2, 4])
@pytest.mark.parametrize("gx", GXS)
def test_an_xcd_serves_w_passes_and_a_range_stays_in_one_window(table, gx, w):
    maps, blocks = table
    for P in PASSES:
        nblk = blocks[(gx, P, w)]
        rows = maps[(gx, P, w)]
        for blk in range(nblk):
            ids = range(8 * gx * blk, 8 * gx * (blk + 1))
            seen = {}    # id class mod 8 -> passes
            where = {}   # (pass-set, range) -> ids
            for i in ids:
                _, rng, pas = rows[i]
                assert 8 * blk <= pas < 8 * blk + 8
                seen.setdefault(i % 8, set()).add(pas)
                where.setdefault((pas // w, rng), []).append(i)
            assert sorted(seen) == list(range(8))
            for cls, passes in seen.items():
                assert len(passes) == w, (gx, P, w, blk, cls, passes)
                assert max(passes) - min(passes) == w - 1 and min(passes) % w == 0  # one aligned pass-set
            for key, lins in where.items():
                assert len(lins) == w and len({i % 8 for i in lins}) == 1, (gx, P, w, key, lins)  # one XCD
                assert max(lins) - min(lins) < 8 * w, (gx, P, w, key, lins)
            # the XCDs stay in step: the n-th workgroups of the eight classes work on the same w ranges
            for n in range(gx):
                rngs = {rows[8 * gx * blk + 8 * n + x][1] for x in range(8)}
                assert rngs == set(range(w * (n // w), w * (n // w) + w)), (gx, P, w, blk, n)


@pytest.mark.parametrize("gx", GXS)
def test_width_eight_is_the_coscheduled_order(table, gx):
    maps, _ = table
    for P in PASSES:
        assert maps[(gx, P, 8)] == _coscheduled(maps, gx, P), (gx, P)


@pytest.mark.parametrize("w", [1, 2, 4])
@pytest.mark.parametrize("gx", GXS)
def test_fallbacks_equal_the_coscheduled_map(table, gx, w):
    maps, blocks = table
    for P in PASSES:
        nblk = blocks[(gx, P, w)]
        rows = maps[(gx, P, w)]
        if nblk == 0:  # the whole launch
            assert rows == _coscheduled(maps, gx, P), (gx, P, w)
            continue
        rest = P - 8 * nblk
        tail = rows[8 * gx * nblk:]
        assert len(tail) == gx * rest
        if rest:  # the trailing passes: the co-scheduled map of a launch of those passes alone
            assert tail == [(ranges, rng, 8 * nblk + pas) for ranges, rng, pas in _coscheduled(maps, gx, rest)], (gx, P, w)
