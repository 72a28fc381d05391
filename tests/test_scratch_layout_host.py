"""The device scratch layouts of the search routes (raglite_amd/csrc/scratch_layout.h), checked on the host: the header is plain C++, so
the driver below compiles the code the library runs with the host compiler under AddressSanitizer and UBSan.

For every layout and every size of the sweep the driver does the sizing walk, mallocs exactly that many bytes, does the pointer walk over
the block, fills every byte of every sub-buffer with a tag of its own and reads all of them back: ASan proves the sub-buffers in bounds,
the tags prove them disjoint.  It prints offsets and sizes; the tests below assert on what it printed: 16-byte alignment of every take,
the adjacencies that kernels and memsets rely on, no more than padding on top of the parts, sizes that only grow with their arguments
(the pools only grow), and -- for the two layouts a launcher owns -- the size formulas the library had before the layouts were stated
once.  The last test shows that the check has teeth: the same walk of search_rows_hi at 4-byte alignment, which is the layout whose
gather buffer was misaligned for odd nb * k."""

import shutil
import subprocess
from pathlib import Path

import pytest

HEADER_DIR = Path(__file__).resolve().parent.parent / "raglite_amd" / "csrc"

_DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "scratch_layout.h"
using namespace rl;

struct Buf { const char* name; void* p; size_t bytes; };  // a take, or a named part of one (name "a.b": part b of take a)

// Tags every byte of every buffer, reads all back, prints the record:  layout|args|size|name:offset:bytes ...|bad tags
static void check(const char* layout, const char* args, size_t size, char* block, std::initializer_list<Buf> bufs) {
    unsigned char tag = 1;
    for (const Buf& b : bufs) std::memset(b.p, tag++, b.bytes);
    std::printf("%s|%s|%zu|", layout, args, size);
    for (const Buf& b : bufs) std::printf("%s:%td:%zu ", b.name, static_cast<char*>(b.p) - block, b.bytes);
    std::printf("|");
    tag = 1;
    for (const Buf& b : bufs) {
        const unsigned char* q = static_cast<const unsigned char*>(b.p);
        const bool ok = b.bytes == 0 || (q[0] == tag && std::memcmp(q, q + 1, b.bytes - 1) == 0);
        if (!ok) std::printf("%s ", b.name);
        ++tag;
    }
    std::printf("\n");
}

// size walk, malloc of exactly that, pointer walk: LAY is `L.lay(c, sizes...)` over a Carver c
#define WALK(L, LAY, ALIGN)                              \
    size_t size;                                         \
    { Carver c(nullptr, ALIGN); size = LAY; }            \
    char* block = static_cast<char*>(std::malloc(size)); \
    if (!block) return 2;                                \
    { Carver c(block, ALIGN); if (LAY != size) return 3; }
#define W(n) ((size_t)(n) * 4)

static const size_t NS[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 31, 32, 33, 96, 97, 128};
static const size_t KS[] = {1, 2, 5, 7, 33, 100, 101, 512};
static const size_t DIMS[] = {32, 256, 1024, 3072};
static char args[160];

static int hi_rows(size_t nb, size_t k, size_t dim, size_t cap, size_t align) {
    HiRows L;
    const size_t nc = nb * cap, n_bmax = nb * 2048;
    WALK(L, L.lay(c, nb, k, dim, cap, n_bmax), align)
    std::snprintf(args, sizeof args, "nb=%zu k=%zu dim=%zu cap=%zu", nb, k, dim, cap);
    check(align == 16 ? "HiRows" : "HiRowsAt4", args, size, block,
          {{"ts", L.ts, W(nb * k)}, {"ti", L.ti, W(nb * k)}, {"thr", L.thr, W(16)}, {"mb", L.mb, W(16)}, {"cnt", L.cnt, W(16)},
           {"cnt.flag", L.flag, W(16)}, {"ci", L.ci, W(nc)}, {"gn", L.gn, W(nc)}, {"G", L.G, W(nc * dim)}, {"xs", L.xs, W(nb * nc)},
           {"es", L.es, W(nc)}, {"bmax", L.bmax, n_bmax * 8}});
    std::free(block);
    return 0;
}

int main() {
#define RUN(call) do { const int st_ = call; if (st_) return st_; } while (0)
    for (size_t nb : NS)
        for (size_t dim : DIMS) {
            ScoreQueries L;
            WALK(L, L.lay(c, nb, dim), 16)
            const size_t groups = (nb + 31) / 32;
            std::snprintf(args, sizeof args, "nb=%zu dim=%zu", nb, dim);
            check("ScoreQueries", args, size, block, {{"frag", L.frag, W(groups * 32 * dim)}, {"unscale", L.unscale, W(nb)}, {"anylo", L.anylo, W(groups)},
                                                      {"q_sumsq", L.q_sumsq, W(nb)}, {"slack", block + size - 256, 256}});
            std::free(block);
        }
    for (size_t n : NS)
        for (size_t dim : DIMS) {
            QueryPlanes L;
            WALK(L, L.lay(c, n, dim), 16)
            std::snprintf(args, sizeof args, "n=%zu dim=%zu", n, dim);
            check("QueryPlanes", args, size, block, {{"frag", L.frag, n * dim * 128}, {"meta", L.meta, W(2 * n)}, {"qsum", L.qsum, W(2 * n)},
                                                     {"slack", block + size - 64, 64}});
            std::free(block);
        }
    for (size_t cap : {(size_t)8192, (size_t)1})          // MERGE_CAP, and RL_OPT_FUSED_TOPK_CAP = 1
        for (size_t ld_s : {(size_t)512, (size_t)768})
            for (size_t B : NS)
                for (size_t k : KS) {
                    if (cap != 1 && ld_s != 512) continue;  // (ld_s is a multiple of 256: one value at the big cap keeps the run short)
                    {
                        FusedRows L;
                        WALK(L, L.lay(c, B, ld_s, k, cap), 16)
                        std::snprintf(args, sizeof args, "B=%zu ld_s=%zu k=%zu cap=%zu", B, ld_s, k, cap);
                        check("FusedRows", args, size, block, {{"S_s", L.S_s, W(B * ld_s)}, {"top_s", L.top_s, W(B * k)}, {"top_i", L.top_i, W(B * k)},
                                                               {"c_s", L.c_s, W(B * cap)}, {"c_i", L.c_i, W(B * cap)}, {"cnt", L.cnt, W(B)}, {"cnt.flag", L.flag, W(16)}});
                        std::free(block);
                    }
                    for (size_t cap2 : {(size_t)1024, (size_t)1}) {
                        if (cap != 1 && cap2 == 1) continue;
                        FusedHiRows L;
                        WALK(L, L.lay(c, B, ld_s, k, cap, cap2), 16)
                        std::snprintf(args, sizeof args, "B=%zu ld_s=%zu k=%zu cap=%zu cap2=%zu", B, ld_s, k, cap, cap2);
                        check("FusedHiRows", args, size, block,
                              {{"S_s", L.S_s, W(B * ld_s)}, {"top_s", L.top_s, W(B * k)}, {"top_i", L.top_i, W(B * k)}, {"c_s", L.c_s, W(B * cap)},
                               {"c_i", L.c_i, W(B * cap)}, {"cnt", L.cnt, W(B)}, {"cnt.flag", L.flag, W(16)}, {"r_i", L.r_i, W(B * cap2)},
                               {"r_s", L.r_s, W(B * cap2)}, {"thr", L.thr, W(B)}, {"window", L.window, W(B)}, {"thr1", L.thr1, W(B)}, {"cnt2", L.cnt2, W(B)}});
                        std::free(block);
                    }
                }
    // search_rows_hi.  One candidate per query: the whole sweep.  The built-in 1024, where the gathered rows alone are nb x 1024 x dim
    // floats: the batches the route takes (up to 16 queries) at an odd, an even and the largest k over the narrowest rows, and k = 5 at
    // the other widths for 1, 2, 3 and the most queries the route takes there (4 on an index wider than 1024).
    for (size_t nb : NS)
        for (size_t k : KS)
            for (size_t dim : DIMS) {
                RUN(hi_rows(nb, k, dim, 1, 16));
                const size_t most = dim > 1024 ? 4 : 16;
                const bool big = dim == 32 ? nb <= most && (k == 2 || k == 5 || k == 512) : k == 5 && (nb <= 3 || nb == most);
                if (big) RUN(hi_rows(nb, k, dim, 1024, 16));
            }
    // ... and as it was before its gather buffer was aligned: the same walk, every take at 4-byte alignment
    RUN(hi_rows(1, 5, 32, 1024, 4));
    RUN(hi_rows(3, 33, 32, 1024, 4));
    RUN(hi_rows(2, 7, 32, 1024, 4));
    for (size_t nb : NS)
        for (size_t k : KS) {
            L2Rescore L;
            const size_t items = nb * k;
            WALK(L, L.lay(c, items), 16)
            std::snprintf(args, sizeof args, "nb=%zu k=%zu", nb, k);
            check("L2Rescore", args, size, block, {{"re", L.re, W(items)}, {"pos", L.pos, W(items)}, {"tmp_rows", L.tmp_rows, W(items)}});
            std::free(block);
        }
    for (size_t most : {(size_t)0, (size_t)1, (size_t)3})
        for (size_t rw : {(size_t)1, (size_t)7, (size_t)9376})
            for (size_t batch : NS) {
                RowMasks L;
                WALK(L, L.lay(c, most, rw, batch), 16)
                std::snprintf(args, sizeof args, "most=%zu rw=%zu batch=%zu", most, rw, batch);
                check("RowMasks", args, size, block, {{"row_sets", L.row_sets, W(most * rw)}, {"d_map", L.d_map, W(most + 2 * batch)}});
                std::free(block);
            }
    for (size_t cap : {(size_t)2048, (size_t)1})
        for (size_t n : NS)
            for (size_t k : KS) {
                HiBatchScratch L;
                const size_t n_bmax = (n < 2 ? n : 2) * 2048;
                WALK(L, L.lay(c, n, k, cap, n_bmax), 16)
                std::snprintf(args, sizeof args, "n=%zu k=%zu cap=%zu", n, k, cap);
                check("HiBatchScratch", args, size, block,
                      {{"ts", L.ts, W(n * k)}, {"ti", L.ti, W(n * k)}, {"thr", L.thr, W(n)}, {"cnt", L.cnt, W(n)}, {"cnt.flag", L.flag, W(16)},
                       {"ci", L.ci, W(n * cap)}, {"es", L.es, W(n * cap)}, {"m", L.m, W(n)}, {"es_top", L.es_top, W(n * k)}, {"bmax", L.bmax, n_bmax * 8}});
                std::free(block);
            }
    for (size_t n : NS) {
        ApproxBound L;
        WALK(L, L.lay(c, n), 16)
        std::snprintf(args, sizeof args, "n=%zu", n);
        check("ApproxBound", args, size, block, {{"top", L.top, W(n)}, {"thr", L.thr, W(n)}, {"cnt", L.cnt, W(n)}, {"flag", L.flag, W(16)}});
        std::free(block);
    }
    for (size_t R : {(size_t)1, (size_t)2})
        for (size_t B : NS)
            for (size_t n_each : {(size_t)1, (size_t)3, (size_t)64}) {
                HybridLists L;
                WALK(L, L.lay(c, R, B, n_each), 16)
                std::snprintf(args, sizeof args, "R=%zu B=%zu n_each=%zu", R, B, n_each);
                check("HybridLists", args, size, block, {{"lists", L.lists, W(R * B * n_each)}, {"scores", L.scores, W(R * B * n_each)}, {"counts", L.counts, W(R * B)}});
                std::free(block);
            }
    for (int keep : {0, 1})  // 1: the caller passes no d_s, the scores stay in the scratch
        for (size_t B : NS)
            for (size_t n_cand : {(size_t)1, (size_t)3, (size_t)64})
                for (size_t k : KS) {
                    if (k > n_cand) continue;
                    RerankScratch L;
                    WALK(L, L.lay(c, B, n_cand, k, keep != 0), 16)
                    if ((L.own_scores != nullptr) != (keep != 0)) return 4;
                    std::snprintf(args, sizeof args, "keep=%d B=%zu n_cand=%zu k=%zu", keep, B, n_cand, k);
                    check("RerankScratch", args, size, block,
                          {{"fused_scores", L.fused_scores, B * n_cand * 8}, {"fused", L.fused, W(B * n_cand)}, {"maxsim", L.maxsim, W(B * n_cand)},
                           {"fused_counts", L.fused_counts, W(B)}, {"pos", L.pos, W(B * k)}, {"own_scores", keep ? (void*)L.own_scores : (void*)block, keep ? W(B * k) : 0}});
                    std::free(block);
                }
    return 0;
}
"""

LAYOUTS = ["ScoreQueries", "QueryPlanes", "FusedRows", "FusedHiRows", "HiRows", "L2Rescore", "RowMasks", "HiBatchScratch", "ApproxBound",
           "HybridLists", "RerankScratch"]


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    """{layout: {args (a tuple of (name, value)): (size, [(buffer, offset, bytes)], [buffers whose tags were overwritten])}}"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("scratch_layout")
    (d / "drv.cpp").write_text(_DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    f"-I{HEADER_DIR}", str(d / "drv.cpp"), "-o", str(d / "drv")], check=True)
    run = subprocess.run([str(d / "drv")], capture_output=True, text=True)  # (an ordinary child, the environment as it is)
    assert run.returncode == 0, run.stderr[-4000:]
    out = {}
    for line in run.stdout.splitlines():
        layout, args, size, bufs, bad = line.split("|")
        key = tuple((a.split("=")[0], int(a.split("=")[1])) for a in args.split())
        parts = [(b.split(":")[0], int(b.split(":")[1]), int(b.split(":")[2])) for b in bufs.split()]
        parts = [p for p in parts if p[0] != "own_scores" or p[2]]  # (not taken where the caller keeps the scores)
        assert key not in out.setdefault(layout, {})
        out[layout][key] = (int(size), parts, bad.split())
    return out


def takes_of(parts):
    """The takes of a record: a buffer "a.b" is a named part of take "a", directly behind what came before it in that take."""
    takes = []
    for name, off, nbytes in parts:
        if "." in name:
            assert name.split(".")[0] == takes[-1][0] and off == takes[-1][1] + takes[-1][2], name
            takes[-1] = (takes[-1][0], takes[-1][1], takes[-1][2] + nbytes)
        else:
            takes.append((name, off, nbytes))
    return takes


def problems(size, parts, bad, need16=None):
    """What is wrong with one laid-out block, as a list of words; empty: sound.  need16: the takes that must start on a 16-byte boundary
    (default: every take, the rule of scratch_layout.h)."""
    found = [f"{name} overwritten" for name in bad]
    for name, off, nbytes in takes_of(parts):
        if off % 16 and (need16 is None or name in need16):
            found.append(f"{name} misaligned")
        if name == "bmax" and off % 8:
            found.append("bmax misaligned for uint64_t")
    spans = sorted((off, off + nbytes, name) for name, off, nbytes in parts if nbytes)
    for (lo, hi, name), (lo2, _, name2) in zip(spans, spans[1:]):
        if hi > lo2:
            found.append(f"{name} overlaps {name2}")
    found += [f"{name} out of bounds" for lo, hi, name in spans if lo < 0 or hi > size]
    return found


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_take_is_aligned_in_bounds_and_disjoint(records, layout):
    assert len(records[layout]) >= 23
    for key, (size, parts, bad) in records[layout].items():
        assert problems(size, parts, bad) == [], (layout, key)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_size_is_the_parts_plus_padding_only(records, layout):
    for key, (size, parts, _) in records[layout].items():
        takes = takes_of(parts)
        total = sum(nbytes for _, _, nbytes in takes)
        assert total <= size <= total + 16 * len(takes), (layout, key)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_size_never_shrinks_when_an_argument_grows(records, layout):
    """The pools only grow: a bigger call must never be handed a smaller block.  Every pair of sweep points that differ in one argument."""
    lines = {}  # the sweep points that agree in all arguments but one: (value of that one, size)
    for key, (size, _, _) in records[layout].items():
        for i, (name, value) in enumerate(key):
            lines.setdefault((name, key[:i] + key[i + 1:]), []).append((value, size))
    compared = 0
    for (name, rest), line in lines.items():
        line.sort()
        assert [size for _, size in line] == sorted(size for _, size in line), (layout, name, rest, line)
        compared += len(line) - 1
    assert compared > 0


@pytest.mark.parametrize("layout,flag_at", [("FusedRows", "B"), ("FusedHiRows", "B"), ("HiRows", 16), ("HiBatchScratch", "n")])
def test_the_flag_words_lie_directly_behind_the_counters(records, layout, flag_at):
    """One memset (search_rows_fused), launch_transform_hist / launch_pivot_route (search_rows_hi: cnt[0 .. 32), the MaxSim batch:
    n + 16 words from cnt) clear counters and flag words in one go; launch_scale_f32, gemm_prepare and a memset clear 16 words from flag."""
    for key, (size, parts, _) in records[layout].items():
        at = {name: (off, nbytes) for name, off, nbytes in parts}
        n = flag_at if isinstance(flag_at, int) else dict(key)[flag_at]
        assert at["cnt.flag"][0] == at["cnt"][0] + 4 * n, (layout, key)
        assert at["cnt.flag"][1] == 64 and at["cnt.flag"][0] + 64 <= size


def test_rows_hi_thresholds_and_bounds_are_sixteen_words_each(records):
    for key, (_, parts, _) in records["HiRows"].items():
        at = {name: (off, nbytes) for name, off, nbytes in parts}
        assert at["thr"][1] == 64 and at["mb"][1] == 64 and at["cnt"][1] + at["cnt.flag"][1] == 128, key


def test_launcher_owned_sizes_do_not_fall_below_their_old_formulas(records):
    """score_planes_scratch_floats and query_planes_bytes as they were before the layouts were stated once: padding on top at most."""
    for key, (size, parts, _) in records["ScoreQueries"].items():
        nb, dim = dict(key)["nb"], dict(key)["dim"]
        groups = (nb + 31) // 32
        old = 4 * (groups * 32 * dim + 2 * nb + groups + 64)
        assert old <= size <= old + 16 * len(parts), key
    for key, (size, parts, _) in records["QueryPlanes"].items():
        n, dim = dict(key)["n"], dict(key)["dim"]
        old = n * (dim * 128 + 16) + 64
        assert old <= size <= old + 16 * len(parts), key
        at = {name: off for name, off, _ in parts}
        assert at["frag"] == 0 and at["meta"] == n * dim * 128  # (the kernels index the fragments from the block's start)


def test_the_check_has_teeth_the_gather_buffer_at_four_byte_alignment(records):
    """search_rows_hi's walk as it was before its gather buffer was aligned: G sits behind 2 nb k + 64 + 2 nb 1024 words, 16-byte aligned
    only for an even nb * k.  That layout promised 16 bytes for G alone (the kernels that score the gathered rows take 16-byte loads) and 8
    for the group maxima, so that is what it is held to here; under today's rule -- every take -- its [nb x k] ids are off as well."""
    old = {(dict(key)["nb"], dict(key)["k"]): rec for key, rec in records["HiRowsAt4"].items()}
    assert problems(*old[(1, 5)], need16={"G"}) == ["G misaligned"]
    assert problems(*old[(3, 33)], need16={"G"}) == ["G misaligned"]
    assert problems(*old[(2, 7)], need16={"G"}) == []
    assert problems(*old[(2, 7)]) == ["ti misaligned"]
    for key, (size, parts, bad) in records["HiRows"].items():  # (today's walk at the same shapes and every other)
        assert "G misaligned" not in problems(size, parts, bad)
