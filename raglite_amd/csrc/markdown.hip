// Markdown block structure on the device: what the splitters read from `MarkdownIt().parse`, batched over
// documents (doc_batch.h).  The parser itself is markdown_blocks.h; this file gives it its line table, one wave per document, and turns
// its two per-line arrays into the arrays the partition kernels take.
//   mb_count_kernel     one document per wave: the number of lines (a ballot per 64 characters) and whether the text holds a line
//                       separator of str.splitlines that markdown-it does not know (the document is undecided then)
//   (an exclusive scan of the counts: the line offsets; launch_kb_exclusive_scan)
//   mb_fill_kernel      one document per wave: bMarks / eMarks by the rank of every line start / line end among the 64 characters of a
//                       ballot plus a carry, then 64 lines at a time, a lane per line: tShift = sCount (a tab in the leading white space
//                       makes the document undecided: the parser does no tab arithmetic)
//   mb_block_kernel     one document per wave runs MbParser::parse: all lanes execute the same statements on the same values, the scans
//                       over long lines (hr, fence open and close, setext underline) take 64 characters per step; the frames live in LDS
//   mb_heading_kernel / mb_known_kernel       heading_end -> the known sentence boundaries per character
//   mb_boundary_kernel / mb_runs_kernel       first_open  -> the chunklet boundary probability per sentence
// No atomics; every writer of a word writes the same value, or owns it.  Integer prefix sums only, so the bytes are the same run to run.
// Device callers' offsets are not validated (doc_batch.h): every kernel clamps a document's characters into [0, n] and its lines into
// [0, n_lines], so malformed offsets give unspecified results and no access outside the arrays.
#include "doc_batch.h"
#include "markdown_blocks.h"
#include "scratch_layout.h"

#include <cmath>

namespace rl {
namespace {

constexpr int64_t MB_DOC_MAX = 2147483647 - 64;  // positions are int32, and a scan may look 63 characters past the one it needs

// The lines [*base, *base + *nl) of document d in arrays of n_lines rows.
__device__ __forceinline__ void mb_doc_lines(const int64_t* __restrict__ line_off, int64_t d, int64_t n_lines, int64_t* base, int64_t* nl) {
    doc_rows(line_off, d, n_lines, base, nl, 2147483647);
    *nl -= *base;
}

__global__ __launch_bounds__(256) void mb_count_kernel(const uint32_t* __restrict__ cp, const int64_t* __restrict__ off, int64_t n_docs,
                                                        int64_t n, int64_t* __restrict__ line_count, int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    for (int64_t doc = wave0; doc < n_docs; doc += n_waves) {
        int64_t b, e;
        doc_rows(off, doc, n, &b, &e, MB_DOC_MAX);
        const uint32_t* c = cp + b;
        const int64_t len = e - b;
        int64_t count = 0;
        bool other = false;
        for (int64_t p = 0; p < len; p += 64) {
            const int64_t i = p + lane;
            const bool in = i < len;
            count += __popcll(__ballot(in && mb_starts_line(c, i)));
            other = other || (in && mb_other_separator(c[i]));
        }
        const bool any_other = __ballot(other) != 0;
        if (lane == 0) {
            line_count[doc] = count;
            flags[doc] = any_other ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(256) void mb_fill_kernel(const uint32_t* __restrict__ cp, const int64_t* __restrict__ off, int64_t n_docs,
                                                       int64_t n, const int64_t* __restrict__ line_off, int64_t n_lines, int32_t* bm,
                                                       int32_t* em, int32_t* __restrict__ ts, int32_t* __restrict__ sc,
                                                       int64_t* __restrict__ line_start, int32_t* flags) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    for (int64_t doc = wave0; doc < n_docs; doc += n_waves) {
        int64_t b, e, base, nl;
        doc_rows(off, doc, n, &b, &e, MB_DOC_MAX);
        mb_doc_lines(line_off, doc, n_lines, &base, &nl);
        const uint32_t* c = cp + b;
        const int64_t len = e - b;
        int64_t starts = 0, ends = 0;
        for (int64_t p = 0; p < len; p += 64) {
            const int64_t i = p + lane;
            const bool in = i < len;
            const bool is_start = in && mb_starts_line(c, i), is_end = in && mb_ends_line(c, i);
            const unsigned long long ms = __ballot(is_start), me = __ballot(is_end);
            const int64_t rs = starts + __popcll(ms & below), re = ends + __popcll(me & below);
            if (is_start && rs < nl) {
                bm[base + rs] = (int32_t)i;
                if (line_start) line_start[base + rs] = b + i;
            }
            if (is_end && re < nl) em[base + re] = (int32_t)i;
            starts += __popcll(ms);
            ends += __popcll(me);
        }
        if (lane == 0 && ends < starts && ends < nl) em[base + ends] = (int32_t)len;  // the last line has no line break
        __threadfence_block();  // the wave's bm and em before the lanes read other lanes' entries
        bool tab = false;
        for (int64_t p = 0; p < nl; p += 64) {
            const int64_t l = p + lane;
            if (l < nl) {
                int32_t lb = bm[base + l], le = em[base + l];
                lb = lb < 0 ? 0 : (lb > len ? (int32_t)len : lb);  // (malformed offsets: stay inside the document)
                le = le < lb ? lb : (le > len ? (int32_t)len : le);
                bool t;
                const int32_t indent = mb_indent(c, lb, le, &t);
                ts[base + l] = indent;
                sc[base + l] = indent;
                tab = tab || t;
            }
        }
        if (__ballot(tab) != 0 && lane == 0) flags[doc] = 1;
    }
}

__global__ __launch_bounds__(256) void mb_block_kernel(const uint32_t* __restrict__ cp, const int64_t* __restrict__ off, int64_t n_docs,
                                                        int64_t n, const int64_t* __restrict__ line_off, int64_t n_lines, int32_t* bm,
                                                        int32_t* em, int32_t* ts, int32_t* sc, uint8_t* lazy, MbSave* save,
                                                        const int32_t* __restrict__ flags, uint8_t* first_open, int32_t* heading_end,
                                                        int32_t* __restrict__ status) {
    __shared__ MbFrame frames[4][MB_MAX_FRAMES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + wave, n_waves = (int64_t)gridDim.x * 4;
    for (int64_t doc = wave0; doc < n_docs; doc += n_waves) {
        int64_t b, e, base, nl;
        doc_rows(off, doc, n, &b, &e, MB_DOC_MAX);
        mb_doc_lines(line_off, doc, n_lines, &base, &nl);
        const int32_t len = (int32_t)(e - b);
        int32_t st = MB_UNDECIDED;
        if (!flags[doc]) {
            MbParser p;
            p.d.cp = cp + b;
            p.d.len = len;
            p.d.bm = bm + base;
            p.d.em = em + base;
            p.d.ts = ts + base;
            p.d.sc = sc + base;
            p.d.n_lines = mb_parser_lines((int32_t)nl, len, p.d.bm, p.d.em, p.d.ts);
            p.d.lazy = lazy + base;
            p.d.save = save + b + doc * MB_SAVE_SLACK;  // [len + MB_SAVE_SLACK]: b + len <= n
            p.d.save_cap = len + MB_SAVE_SLACK;
            p.d.frames = frames[wave];
            p.d.first_open = first_open + base;
            p.d.heading_end = heading_end + base;
            st = p.parse();
        }
        if (lane == 0) status[doc] = st;
    }
}

// ---- heading_end -> known sentence boundaries (raglite_amd/_sentences.py: markdown_sentence_boundaries) -------------------------------
// A heading of lines [L, E) writes 1 before its first character, 0 on its lines and 1 on the first character behind them, and a later
// heading overwrites an earlier one.  Per character that is: 1 if the next line starts a heading and this is the last character before
// it; else 0 on a heading's lines; else 1 on the first character behind a heading; else NaN.
__global__ __launch_bounds__(256) void mb_heading_kernel(const int32_t* __restrict__ heading_end, const int64_t* __restrict__ line_off,
                                                          const int32_t* __restrict__ status, int64_t n_docs, int64_t n_lines,
                                                          uint8_t* __restrict__ body, uint8_t* __restrict__ behind) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n_lines; g += stride) {
        const int32_t end = heading_end[g];
        if (end <= 0) continue;
        const int64_t doc = doc_of(line_off, n_docs, g);
        int64_t base, nl;
        mb_doc_lines(line_off, doc, n_lines, &base, &nl);
        const int64_t l = g - base;
        if (l < 0 || l >= nl || status[doc] != MB_OK) continue;
        const int64_t stop = end < nl ? end : nl;
        for (int64_t k = l; k < stop; ++k) body[base + k] = 1;  // headings do not overlap: every byte has one writer
        if (end < nl) behind[base + end] = 1;
    }
}

__global__ __launch_bounds__(256) void mb_known_kernel(const int32_t* __restrict__ heading_end, const int64_t* __restrict__ line_start,
                                                        const int64_t* __restrict__ line_off, const int32_t* __restrict__ status,
                                                        const int64_t* __restrict__ off, int64_t n_docs, int64_t n, int64_t n_lines,
                                                        const uint8_t* __restrict__ body, const uint8_t* __restrict__ behind,
                                                        double* __restrict__ known) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        double v = NAN;
        const int64_t doc = doc_of(off, n_docs, i);
        int64_t b, e, base, nl;
        doc_rows(off, doc, n, &b, &e, MB_DOC_MAX);
        mb_doc_lines(line_off, doc, n_lines, &base, &nl);
        if (i >= b && i < e && nl > 0 && status[doc] == MB_OK) {
            int64_t lo = 0, hi = nl;  // the last line that starts at or before i
            while (hi - lo > 1) {
                const int64_t mid = (lo + hi) >> 1;
                if (line_start[base + mid] <= i) lo = mid; else hi = mid;
            }
            if (lo + 1 < nl && line_start[base + lo + 1] == i + 1 && heading_end[base + lo + 1] > 0) v = 1.0;
            else if (body[base + lo]) v = 0.0;
            else if (behind[base + lo] && line_start[base + lo] == i) v = 1.0;
        }
        known[i] = v;
    }
}

// ---- first_open -> chunklet boundary probabilities (raglite_amd/_chunklets.py: markdown_chunklet_boundaries) ---------------------------
__device__ __forceinline__ double mb_proba(uint8_t kind) {
    return kind == MB_HEADING ? 1.0 : kind == MB_BLOCKQUOTE ? 0.75 : kind == MB_PARAGRAPH ? 0.5 : kind != MB_NONE ? 0.25 : 0.0;
}

__global__ __launch_bounds__(256) void mb_boundary_kernel(const uint8_t* __restrict__ first_open, const int64_t* __restrict__ line_start,
                                                           const int64_t* __restrict__ line_off, const int32_t* __restrict__ status,
                                                           const int64_t* __restrict__ sent_off, const int64_t* __restrict__ sent_doc_off,
                                                           int64_t n_sent, int64_t n_docs, int64_t n_lines, double* __restrict__ raw) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < n_sent; s += stride) {
        double v = 0.0;
        const int64_t doc = doc_of(sent_doc_off, n_docs, s);
        int64_t sb, se, base, nl;
        doc_rows(sent_doc_off, doc, n_sent, &sb, &se);
        mb_doc_lines(line_off, doc, n_lines, &base, &nl);
        if (s >= sb && s < se && status[doc] == MB_OK) {
            const int64_t cs = sent_off[s], ce = sent_off[s + 1];
            int64_t lo = 0, hi = nl;  // the first line that starts at or behind cs
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (line_start[base + mid] < cs) lo = mid + 1; else hi = mid;
            }
            for (int64_t l = lo; l < nl && line_start[base + l] < ce; ++l) {
                const uint8_t kind = first_open[base + l];
                if (kind != MB_NONE) { v = mb_proba(kind); break; }
            }
        }
        raw[s] = v;
    }
}

// Of a run of consecutive non-zero sentences only the first largest keeps its value; the thread at a run's first sentence writes the run.
__global__ __launch_bounds__(256) void mb_runs_kernel(const double* __restrict__ raw, const int64_t* __restrict__ sent_doc_off,
                                                       int64_t n_sent, int64_t n_docs, double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < n_sent; s += stride) {
        if (raw[s] == 0.0) { out[s] = 0.0; continue; }
        const int64_t doc = doc_of(sent_doc_off, n_docs, s);
        int64_t sb, se;
        doc_rows(sent_doc_off, doc, n_sent, &sb, &se);
        if (s < sb || s >= se) { out[s] = 0.0; continue; }
        if (s > sb && raw[s - 1] != 0.0) continue;  // inside a run: its first sentence's thread writes this one
        int64_t keep = s, end = s;
        double best = raw[s];
        for (; end < se && raw[end] != 0.0; ++end)
            if (raw[end] > best) { best = raw[end]; keep = end; }
        for (int64_t k = s; k < end; ++k) out[k] = k == keep ? best : 0.0;
    }
}

inline int blocks_for(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 256 * 64)); }

}  // namespace

size_t markdown_blocks_scratch_bytes(int64_t n, int64_t n_docs) {
    return MarkdownScratch().lay(Carver(), (size_t)n, (size_t)n_docs, (size_t)n + (size_t)n_docs * MB_SAVE_SLACK, kb_scan_scratch_items(n_docs + 1));
}

int launch_markdown_blocks(const uint32_t* codepoints, const int64_t* doc_off, int64_t n, int64_t n_docs, uint8_t* first_open,
                           int32_t* heading_end, int64_t* line_start, int64_t* line_off, int32_t* status, void* scratch, hipStream_t s) {
    if (n_docs <= 0) return RL_OK;
    const int64_t n_lines = n + n_docs;
    MarkdownScratch w;
    w.lay(Carver(scratch), (size_t)n, (size_t)n_docs, (size_t)n + (size_t)n_docs * MB_SAVE_SLACK, kb_scan_scratch_items(n_docs + 1));
    RL_HIP(hipMemsetAsync(first_open, 0, (size_t)n_lines, s));
    RL_HIP(hipMemsetAsync(heading_end, 0, (size_t)n_lines * sizeof(int32_t), s));
    RL_HIP(hipMemsetAsync(w.lazy, 0, (size_t)n_lines, s));
    RL_HIP(hipMemsetAsync(line_off + n_docs, 0, sizeof(int64_t), s));
    const int wblocks = wave_per_item_blocks(n_docs);
    hipLaunchKernelGGL(mb_count_kernel, dim3(wblocks), dim3(256), 0, s, codepoints, doc_off, n_docs, n, line_off, w.flags);
    const int64_t* total = nullptr;
    RL_TRY(launch_kb_exclusive_scan(line_off, n_docs + 1, w.scan, &total, s));
    hipLaunchKernelGGL(mb_fill_kernel, dim3(wblocks), dim3(256), 0, s, codepoints, doc_off, n_docs, n, line_off, n_lines, w.bm, w.em, w.ts,
                       w.sc, line_start, w.flags);
    hipLaunchKernelGGL(mb_block_kernel, dim3(wblocks), dim3(256), 0, s, codepoints, doc_off, n_docs, n, line_off, n_lines, w.bm, w.em, w.ts,
                       w.sc, w.lazy, reinterpret_cast<MbSave*>(w.save), w.flags, first_open, heading_end, status);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

size_t markdown_known_scratch_bytes(int64_t n_lines) { return MarkdownKnownScratch().lay(Carver(), (size_t)n_lines); }

int launch_markdown_sentence_known(const int32_t* heading_end, const int64_t* line_start, const int64_t* line_off, const int32_t* status,
                                   const int64_t* doc_off, int64_t n, int64_t n_docs, int64_t n_lines, double* known, void* scratch,
                                   hipStream_t s) {
    if (n <= 0 || n_docs <= 0) return RL_OK;
    MarkdownKnownScratch w;
    const size_t bytes = w.lay(Carver(scratch), (size_t)n_lines);
    RL_HIP(hipMemsetAsync(scratch, 0, bytes, s));
    if (n_lines > 0)
        hipLaunchKernelGGL(mb_heading_kernel, dim3(blocks_for(n_lines)), dim3(256), 0, s, heading_end, line_off, status, n_docs, n_lines,
                           w.body, w.behind);
    hipLaunchKernelGGL(mb_known_kernel, dim3(blocks_for(n)), dim3(256), 0, s, heading_end, line_start, line_off, status, doc_off, n_docs, n,
                       n_lines, w.body, w.behind, known);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

size_t markdown_boundary_scratch_bytes(int64_t n_sent) { return (size_t)n_sent * sizeof(double) + 16; }

int launch_markdown_chunklet_boundary(const uint8_t* first_open, const int64_t* line_start, const int64_t* line_off, const int32_t* status,
                                      const int64_t* sent_off, const int64_t* sent_doc_off, int64_t n_sent, int64_t n_docs,
                                      int64_t n_lines, double* boundary, void* scratch, hipStream_t s) {
    if (n_sent <= 0 || n_docs <= 0) return RL_OK;
    double* raw = static_cast<double*>(scratch);
    hipLaunchKernelGGL(mb_boundary_kernel, dim3(blocks_for(n_sent)), dim3(256), 0, s, first_open, line_start, line_off, status, sent_off,
                       sent_doc_off, n_sent, n_docs, n_lines, raw);
    hipLaunchKernelGGL(mb_runs_kernel, dim3(blocks_for(n_sent)), dim3(256), 0, s, raw, sent_doc_off, n_sent, n_docs, boundary);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

}  // namespace rl
