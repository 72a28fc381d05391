"""The scratch layout of the native encoder forward (`EncoderScratch`, raglite_amd/csrc/scratch_layout.h), checked on the host the way
tests/test_scratch_layout_host.py checks the search routes' layouts: the header is plain C++, so a small program of its own compiles the
walk the library runs with the host compiler under AddressSanitizer and UBSan, mallocs exactly the size the sizing walk gives, tags every
byte of every sub-buffer and reads the tags back (ASan: in bounds; the tags: disjoint).  On top of that, what `rl_encoder_forward` relies
on: the block is reserved once for the cap and every call walks it with its own row count, so the walk of n rows must end inside the
walk of the cap -- a call writes a prefix of the block -- and every sub-buffer must start on a 16-byte boundary (the kernels take 16-byte
loads and stores on all of them)."""

import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER_DIR = ROOT / "raglite_amd" / "csrc"
CAP = int(re.search(r"#define RL_ENCODER_MAX_TOKENS (\d+)", (ROOT / "include" / "raglite_hip.h").read_text()).group(1))

_DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "scratch_layout.h"
using namespace rl;

int main() {
    static const size_t ROWS[] = {1, 2, 3, 31, 32, 33, 64, 65, 127, 128, 255, 256};
    static const size_t SHAPES[][3] = {{32, 32, 1}, {64, 128, 1}, {64, 512, 2}, {192, 320, 1}, {128, 96, 1}, {1024, 4096, 8}, {8192, 32768, 8}};
    for (const auto& sh : SHAPES)
        for (size_t rows : ROWS) {
            const size_t H = sh[0], F = sh[1], ks = sh[2];
            EncoderScratch L;
            const size_t size = L.lay(Carver(), rows, H, F, ks);
            char* block = static_cast<char*>(std::malloc(size));
            if (!block) return 2;
            if (L.lay(Carver(block), rows, H, F, ks) != size) return 3;
            struct { const char* name; void* p; size_t bytes; } bufs[] = {
                {"x", L.x, rows * H * 2}, {"x1", L.x1, rows * H * 2}, {"qkv", L.qkv, rows * 3 * H * 2}, {"attn", L.attn, rows * H * 2},
                {"mid", L.mid, rows * F * 2}, {"part", L.part, ks * rows * H * 4}};
            unsigned char tag = 1;
            for (const auto& b : bufs) std::memset(b.p, tag++, b.bytes);
            std::printf("%zu %zu %zu %zu|%zu|", rows, H, F, ks, size);
            for (const auto& b : bufs) std::printf("%s:%td:%zu ", b.name, static_cast<char*>(b.p) - block, b.bytes);
            std::printf("|");
            tag = 1;
            for (const auto& b : bufs) {
                const unsigned char* q = static_cast<const unsigned char*>(b.p);
                if (!(q[0] == tag && std::memcmp(q, q + 1, b.bytes - 1) == 0)) std::printf("%s ", b.name);
                ++tag;
            }
            std::printf("\n");
            std::free(block);
        }
    return 0;
}
"""


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    """{(rows, hidden, ffn, ksplit): (size, [(buffer, offset, bytes)], [buffers whose tags were overwritten])}"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("encoder_scratch_layout")
    (d / "drv.cpp").write_text(_DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    f"-I{HEADER_DIR}", str(d / "drv.cpp"), "-o", str(d / "drv")], check=True)
    run = subprocess.run([str(d / "drv")], capture_output=True, text=True)  # (an ordinary child, the environment as it is)
    assert run.returncode == 0, run.stderr[-4000:]
    out = {}
    for line in run.stdout.splitlines():
        key, size, bufs, bad = line.split("|")
        out[tuple(map(int, key.split()))] = (int(size), [(b.split(":")[0], int(b.split(":")[1]), int(b.split(":")[2])) for b in bufs.split()],
                                             bad.split())
    assert len(out) == 7 * 12
    return out


def test_every_buffer_is_aligned_in_bounds_and_disjoint(records):
    for key, (size, parts, bad) in records.items():
        assert bad == [], (key, bad)
        assert [name for name, _, _ in parts] == ["x", "x1", "qkv", "attn", "mid", "part"]
        spans = sorted((off, off + n) for _, off, n in parts)
        assert all(off % 16 == 0 for off, _ in spans), key
        assert spans[0][0] == 0 and spans[-1][1] <= size and all(hi <= lo2 for (_, hi), (lo2, _) in zip(spans, spans[1:])), key
        assert sum(n for _, _, n in parts) <= size <= sum(n for _, _, n in parts) + 16 * len(parts), key  # the parts plus padding only


def test_a_call_of_fewer_rows_walks_a_prefix_of_the_block_reserved_for_the_cap(records):
    shapes = {key[1:] for key in records}
    for shape in shapes:
        sizes = [(rows, records[(rows, *shape)][0]) for rows in sorted(key[0] for key in records if key[1:] == shape)]
        assert sizes[-1][0] == CAP  # the sweep ends at the header's cap: what rl_encoder_create reserves
        assert all(a[1] < b[1] for a, b in zip(sizes, sizes[1:])), shape  # strictly growing with the rows, so never past the cap's size
