// The block parser of raglite_amd/csrc/markdown_blocks.h on the CPU: the code the device runs, compiled with the host compiler (under
// AddressSanitizer and UBSan in tests/test_markdown_blocks_host.py).
//   markdown_blocks_main <input>
// input (little-endian): int32 n_docs, int64 doc_offsets[n_docs + 1], uint32 codepoints[doc_offsets[n_docs]]
// output, per document three lines:  "<status> <n_lines>", the first_open values, the heading_end values.
// Every array is malloc'ed at exactly the size the parser may touch, so that a step outside it is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "markdown_blocks.h"

using namespace rl;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n_docs = 0;
    if (std::fread(&n_docs, 4, 1, f) != 1 || n_docs < 0) return 2;
    std::vector<int64_t> off((size_t)n_docs + 1);
    if (std::fread(off.data(), 8, off.size(), f) != off.size()) return 2;
    for (int32_t k = 0; k < n_docs; ++k) {
        const int32_t len = (int32_t)(off[k + 1] - off[k]);
        uint32_t* cp = static_cast<uint32_t*>(std::malloc((size_t)len * 4 + 1));  // its own block per document
        if (len && std::fread(cp, 4, (size_t)len, f) != (size_t)len) return 2;
        int32_t n_split = 0;
        bool other = false;
        for (int32_t i = 0; i < len; ++i) {
            n_split += mb_starts_line(cp, i) ? 1 : 0;
            other = other || mb_other_separator(cp[i]);
        }
        const size_t nl = (size_t)n_split;
        int32_t* bm = static_cast<int32_t*>(std::malloc(nl * 4 + 1));
        int32_t* em = static_cast<int32_t*>(std::malloc(nl * 4 + 1));
        int32_t* ts = static_cast<int32_t*>(std::malloc(nl * 4 + 1));
        int32_t* sc = static_cast<int32_t*>(std::malloc(nl * 4 + 1));
        uint8_t* lazy = static_cast<uint8_t*>(std::calloc(nl + 1, 1));
        uint8_t* first_open = static_cast<uint8_t*>(std::calloc(nl + 1, 1));
        int32_t* heading_end = static_cast<int32_t*>(std::calloc(nl + 1, 4));
        int32_t starts = 0, ends = 0;
        for (int32_t i = 0; i < len; ++i) {
            if (mb_starts_line(cp, i)) bm[starts++] = i;
            if (mb_ends_line(cp, i)) em[ends++] = i;
        }
        if (ends < starts) em[ends++] = len;
        if (ends != starts) return 3;
        bool tab = false;
        for (int32_t l = 0; l < n_split; ++l) {
            bool t;
            ts[l] = sc[l] = mb_indent(cp, bm[l], em[l], &t);
            tab = tab || t;
        }
        const int32_t save_cap = len + MB_SAVE_SLACK;
        MbSave* save = static_cast<MbSave*>(std::malloc((size_t)save_cap * sizeof(MbSave)));
        MbFrame* frames = static_cast<MbFrame*>(std::malloc(sizeof(MbFrame) * MB_MAX_FRAMES));
        int32_t status = MB_UNDECIDED;
        if (!other && !tab) {
            MbParser p;
            p.d = MbDoc{cp, len, mb_parser_lines(n_split, len, bm, em, ts), bm, em, ts, sc, lazy, save, save_cap, frames, first_open, heading_end};
            status = p.parse();
            if (status == MB_OK) {  // the parse leaves the line table as it found it
                for (int32_t l = 0; l < n_split; ++l) {
                    bool t;
                    if (lazy[l] || ts[l] != mb_indent(cp, bm[l], em[l], &t) || sc[l] != ts[l] || (l && bm[l] <= bm[l - 1])) return 4;
                }
            }
        }
        std::printf("%d %d\n", status, n_split);
        for (int32_t l = 0; l < n_split; ++l) std::printf("%d ", (int)first_open[l]);
        std::printf("\n");
        for (int32_t l = 0; l < n_split; ++l) std::printf("%d ", heading_end[l]);
        std::printf("\n");
        std::free(cp); std::free(bm); std::free(em); std::free(ts); std::free(sc); std::free(lazy); std::free(first_open);
        std::free(heading_end); std::free(save); std::free(frames);
    }
    std::fclose(f);
    return 0;
}
