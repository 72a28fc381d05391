// The block phase of markdown-it-py's `commonmark` preset (what `MarkdownIt().parse` runs before the inline phase), reduced to what the
// splitters read from its tokens: per line, the first of heading_open / blockquote_open / paragraph_open /
// bullet_list_open / ordered_list_open that starts there (first_open) and, where a heading starts, its map[1] (heading_end).
//
// The rules are the library's, in its order and with its terminator sets:
//     main chain   code, fence, blockquote, hr, list, reference, html_block, heading, lheading, paragraph
//     "paragraph" and "blockquote" terminators   fence, blockquote, hr, list, html_block, heading
//     "list" terminators                         fence, blockquote, hr
// The library recurses (tokenize -> blockquote -> tokenize, tokenize -> list -> tokenize per item).  Here every container is a frame on
// an explicit stack, and a frame carries the tokenize loop that runs inside it.  A blockquote rewrites the line records of its lines
// (bMarks, tShift, sCount) and puts them back when it closes: the old records go to a save stack.  At any time the open quotes' saved
// marker lines stand for distinct '>' characters, so the stack never holds more entries than the document has characters, plus one
// terminating line per open quote.  A lazy continuation line (the library sets its sCount to -1) keeps its record and gets the tag of the
// quote that made it lazy; every deeper quote finds it lazy already, and the tagging quote clears it on its way out.
//
// What is not ported, and why it cannot change a token's type or map: the tight / loose bookkeeping (it only sets `hidden`), token
// content (getLines, the ATX tail), parentType (the list rule reads it in silent mode only, where the caller is known: `in_paragraph`).
//
// Exact or undecided: a document is given up (MB_UNDECIDED) the moment the parse would need the html_block rule ('<' first on a line
// where block rules are tried), the reference rule ('[' where a paragraph would start), tab arithmetic (a tab behind a container marker;
// tabs in a line's leading white space are found when the line table is built), or a block at level >= MB_MAX_LEVEL.
//
// Plain C++ over plain pointers: markdown.hip runs it with one document per wave (every lane executes the same statements on the same
// values; the long-line scans split their characters over the lanes), and tests/test_markdown_blocks_host.py compiles it for the CPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MB_HD __host__ __device__ __forceinline__
#else
#define MB_HD inline
#endif

namespace rl {

constexpr int32_t MB_OK = 0, MB_UNDECIDED = 1;
constexpr int32_t MB_NONE = 0, MB_HEADING = 1, MB_BLOCKQUOTE = 2, MB_PARAGRAPH = 3, MB_BULLET_LIST = 4, MB_ORDERED_LIST = 5;
constexpr int32_t MB_MAX_LEVEL = 16;   // a block that would open at this level makes the document undecided (the library stops at 20)
constexpr int32_t MB_MAX_FRAMES = 18;  // the root and at most MB_MAX_LEVEL containers
constexpr int32_t MB_SAVE_SLACK = 2 * MB_MAX_FRAMES;  // save entries a document needs beyond one per character

struct MbSave { int32_t line, bm, ts, sc; };

struct MbFrame {
    int32_t kind;        // 0 root, 1 blockquote, 2 list
    int32_t line, end;   // the tokenize loop of this frame: the next line, one past its last
    int32_t start;       // blockquote: its first line; list: the current item's first line
    // blockquote
    int32_t scan_end, old_line_max, old_blk, save_base;
    // list
    int32_t list_end, ordered, marker_char, pos_after, old_ts, old_sc, old_list_indent;
};

// One document: the code points, the line table (positions relative to the document), the save stack and the two outputs.
struct MbDoc {
    const uint32_t* cp;
    int32_t len;       // characters
    int32_t n_lines;   // the lines the library's StateBlock holds (a last line of spaces without a line break is not among them)
    int32_t *bm, *em, *ts, *sc;  // [n_lines]
    uint8_t* lazy;     // [n_lines] 0, or the depth of the quote frame that made the line a lazy continuation
    MbSave* save;
    int32_t save_cap;
    MbFrame* frames;   // [MB_MAX_FRAMES]
    uint8_t* first_open;   // [n_lines], zeroed by the caller
    int32_t* heading_end;  // [n_lines], zeroed by the caller
};

struct MbState {
    int32_t blk = 0, line = 0, line_max = 0, list_indent = -1, level = 0, depth = 0, n_save = 0, status = MB_OK;
};

// ---- the lanes of a wave (one lane on the CPU) ------------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
constexpr int32_t MB_LANES = 64;
__device__ __forceinline__ int32_t mb_lane() { return (int32_t)(threadIdx.x & 63); }
__device__ __forceinline__ uint64_t mb_ballot(bool p) { return __ballot(p); }
__device__ __forceinline__ int32_t mb_popc(uint64_t m) { return __popcll(m); }
__device__ __forceinline__ int32_t mb_ctz(uint64_t m) { return __ffsll((long long)m) - 1; }
#else
constexpr int32_t MB_LANES = 1;
inline int32_t mb_lane() { return 0; }
inline uint64_t mb_ballot(bool p) { return p ? 1u : 0u; }
inline int32_t mb_popc(uint64_t m) { return (int32_t)(m & 1u); }
inline int32_t mb_ctz(uint64_t) { return 0; }
#endif

MB_HD bool mb_space(uint32_t c) { return c == 0x20u || c == 0x09u; }  // isStrSpace

// The first position in [pos, max) whose character is not `c` (max if there is none); the lanes take 64 characters at a time.
MB_HD int32_t mb_skip_char(const uint32_t* cp, int32_t pos, int32_t max, uint32_t c) {
    for (int32_t p = pos; p < max; p += MB_LANES) {
        const int32_t i = p + mb_lane();
        const uint64_t other = mb_ballot(i < max && cp[i] != c);
        if (other) return p + mb_ctz(other);
    }
    return max;
}
MB_HD int32_t mb_skip_spaces(const uint32_t* cp, int32_t pos, int32_t max) {
    for (int32_t p = pos; p < max; p += MB_LANES) {
        const int32_t i = p + mb_lane();
        const uint64_t other = mb_ballot(i < max && !mb_space(cp[i]));
        if (other) return p + mb_ctz(other);
    }
    return max;
}
MB_HD bool mb_contains(const uint32_t* cp, int32_t pos, int32_t max, uint32_t c) {
    for (int32_t p = pos; p < max; p += MB_LANES) {
        const int32_t i = p + mb_lane();
        if (mb_ballot(i < max && cp[i] == c)) return true;
    }
    return false;
}

// ---- the line table: markdown-it's normalisation (\r\n and a lone \r are \n) and StateBlock's caches ----------------------------------
// With these three predicates the lines are also Python's str.splitlines lines, unless the text holds one of the other separators.
MB_HD bool mb_other_separator(uint32_t c) {
    return c == 0x0Bu || c == 0x0Cu || (c >= 0x1Cu && c <= 0x1Eu) || c == 0x85u || c == 0x2028u || c == 0x2029u;
}
MB_HD bool mb_starts_line(const uint32_t* cp, int64_t i) {  // character i of a document (cp: the document's first character)
    return i == 0 || cp[i - 1] == 0x0Au || (cp[i - 1] == 0x0Du && cp[i] != 0x0Au);
}
MB_HD bool mb_ends_line(const uint32_t* cp, int64_t i) {  // the k-th such character ends line k at eMarks = i
    return cp[i] == 0x0Du || (cp[i] == 0x0Au && (i == 0 || cp[i - 1] != 0x0Du));
}
// tShift of the line [b, e) (== sCount while no tab is among the leading white space; *tab says whether one is)
MB_HD int32_t mb_indent(const uint32_t* cp, int32_t b, int32_t e, bool* tab) {
    int32_t p = b;
    *tab = false;
    while (p < e && mb_space(cp[p])) {
        if (cp[p] == 0x09u) *tab = true;
        ++p;
    }
    return p - b;
}
// The lines StateBlock holds, of n_split lines: its constructor never records a last line of spaces that has no line break.
MB_HD int32_t mb_parser_lines(int32_t n_split, int32_t len, const int32_t* bm, const int32_t* em, const int32_t* ts) {
    if (n_split > 0 && em[n_split - 1] == len && bm[n_split - 1] + ts[n_split - 1] >= len) return n_split - 1;
    return n_split;
}

struct MbParser {
    MbDoc d;
    MbState st;

    // ---- line records; line n_lines is the library's fake last entry -------------------------------------------------------------------
    // (a correct table holds positions in [0, len] already; a device caller's malformed offsets may not, and no character outside the
    // document is ever read: every read is at bm + ts < em)
    MB_HD int32_t in_doc(int32_t p) const { return p < 0 ? 0 : (p > d.len ? d.len : p); }
    MB_HD int32_t bm(int32_t l) const { return l < d.n_lines ? in_doc(d.bm[l]) : d.len; }
    MB_HD int32_t em(int32_t l) const { return l < d.n_lines ? in_doc(d.em[l]) : d.len; }
    MB_HD int32_t ts(int32_t l) const { return l < d.n_lines ? in_doc(d.ts[l]) : 0; }
    MB_HD int32_t sc(int32_t l) const { return l < d.n_lines ? (d.lazy[l] ? -1 : d.sc[l]) : 0; }
    MB_HD bool is_empty(int32_t l) const { return bm(l) + ts(l) >= em(l); }
    MB_HD bool is_code(int32_t l) const { return sc(l) - st.blk >= 4; }
    MB_HD uint32_t ch_at(int32_t pos, int32_t max) const { return pos < max ? d.cp[pos] : 0x0Au; }  // behind a line's end: its line break
    MB_HD int32_t skip_empty_lines(int32_t from) const {
        while (from < st.line_max && is_empty(from)) ++from;
        return from;
    }
    MB_HD void undecided() { st.status = MB_UNDECIDED; }
    MB_HD void open(int32_t line, int32_t type) {
        if (d.first_open[line] == MB_NONE) d.first_open[line] = (uint8_t)type;
    }
    MB_HD void save(int32_t l) {
        if (st.n_save >= d.save_cap) { undecided(); return; }  // (cannot happen: see the bound above)
        d.save[st.n_save++] = MbSave{l, d.bm[l], d.ts[l], d.sc[l]};
    }

    // ---- the rules in silent mode -----------------------------------------------------------------------------------------------------
    MB_HD bool fence_open(int32_t pos, int32_t max, uint32_t* marker, int32_t* length) const {
        if (pos + 3 > max) return false;
        const uint32_t m = d.cp[pos];
        if (m != 0x7Eu && m != 0x60u) return false;
        const int32_t after = mb_skip_char(d.cp, pos, max, m);
        if (after - pos < 3) return false;
        if (m == 0x60u && mb_contains(d.cp, after, max, m)) return false;
        *marker = m;
        *length = after - pos;
        return true;
    }
    MB_HD bool hr_at(int32_t pos, int32_t max) const {
        const uint32_t m = ch_at(pos, max);
        if (m != 0x2Au && m != 0x2Du && m != 0x5Fu) return false;
        int32_t cnt = 1;
        for (int32_t p = pos + 1; p < max; p += MB_LANES) {
            const int32_t i = p + mb_lane();
            const uint32_t c = i < max ? d.cp[i] : m;
            if (mb_ballot(c != m && !mb_space(c))) return false;
            cnt += mb_popc(mb_ballot(i < max && c == m));
        }
        return cnt >= 3;
    }
    MB_HD bool heading_at(int32_t pos, int32_t max) const {
        if (ch_at(pos, max) != 0x23u) return false;
        int32_t level = 1;
        ++pos;
        uint32_t c = ch_at(pos, max);
        while (c == 0x23u && pos < max && level <= 6) {
            ++level;
            ++pos;
            c = ch_at(pos, max);
        }
        return !(level > 6 || (pos < max && !mb_space(c)));
    }
    MB_HD int32_t skip_bullet_marker(int32_t l) const {
        int32_t pos = bm(l) + ts(l);
        const int32_t max = em(l);
        const uint32_t m = ch_at(pos, max);
        ++pos;
        if (m != 0x2Au && m != 0x2Du && m != 0x2Bu) return -1;
        if (pos < max && !mb_space(d.cp[pos])) return -1;
        return pos;
    }
    MB_HD int32_t skip_ordered_marker(int32_t l, int32_t* value) const {
        const int32_t start = bm(l) + ts(l), max = em(l);
        int32_t pos = start;
        if (pos + 1 >= max) return -1;
        uint32_t c = d.cp[pos++];
        if (c < 0x30u || c > 0x39u) return -1;
        int32_t v = (int32_t)(c - 0x30u);
        for (;;) {
            if (pos >= max) return -1;
            c = d.cp[pos++];
            if (c >= 0x30u && c <= 0x39u) {
                if (pos - start >= 10) return -1;
                v = v * 10 + (int32_t)(c - 0x30u);
                continue;
            }
            if (c == 0x29u || c == 0x2Eu) break;
            return -1;
        }
        if (pos < max && !mb_space(d.cp[pos])) return -1;
        *value = v;
        return pos;
    }
    // The checks of the list rule up to `if silent: return True`.  Returns the position behind the marker, or -1.
    MB_HD int32_t list_marker(int32_t l, bool terminating_paragraph, int32_t* ordered) const {
        if (st.list_indent >= 0 && sc(l) - st.list_indent >= 4 && sc(l) < st.blk) return -1;
        int32_t value = 0;
        int32_t p = skip_ordered_marker(l, &value);
        if (p >= 0) {
            *ordered = 1;
            if (terminating_paragraph && value != 1) return -1;
        } else {
            p = skip_bullet_marker(l);
            if (p < 0) return -1;
            *ordered = 0;
        }
        if (terminating_paragraph && mb_skip_spaces(d.cp, p, em(l)) >= em(l)) return -1;
        return p;
    }
    // Does a rule of the set terminate the block at line l?  with_list: the "paragraph" and "blockquote" sets (the "list" set is fence,
    // blockquote, hr).  in_paragraph: the caller is the paragraph or the lheading rule (parentType == "paragraph").
    MB_HD bool terminates(int32_t l, bool with_list, bool in_paragraph) {
        if (is_code(l)) return false;  // every rule of every set starts with this check
        const int32_t pos = bm(l) + ts(l), max = em(l);
        const uint32_t c = ch_at(pos, max);
        uint32_t marker;
        int32_t length;
        if (fence_open(pos, max, &marker, &length)) return true;
        if (c == 0x3Eu) return true;
        if (hr_at(pos, max)) return true;
        if (!with_list) return false;
        int32_t ordered;
        if (list_marker(l, in_paragraph && sc(l) >= st.blk, &ordered) >= 0) return true;
        if (c == 0x3Cu) {  // html_block
            undecided();
            return true;
        }
        return heading_at(pos, max);
    }

    // ---- the leaf rules ---------------------------------------------------------------------------------------------------------------
    MB_HD void code_rule(int32_t start, int32_t end) {
        int32_t next = start + 1, last = next;
        while (next < end) {
            if (is_empty(next)) { ++next; continue; }
            if (is_code(next)) { ++next; last = next; continue; }
            break;
        }
        st.line = last;
    }
    MB_HD void fence_rule(int32_t start, int32_t end, uint32_t marker, int32_t length) {
        int32_t next = start;
        bool closed = false;
        for (;;) {
            ++next;
            if (next >= end) break;
            const int32_t pos = bm(next) + ts(next), max = em(next);
            if (pos < max && sc(next) < st.blk) break;
            if (ch_at(pos, max) != marker) continue;
            if (is_code(next)) continue;
            int32_t p = mb_skip_char(d.cp, pos, max, marker);
            if (p - pos < length) continue;
            p = mb_skip_spaces(d.cp, p, max);
            if (p < max) continue;
            closed = true;
            break;
        }
        st.line = next + (closed ? 1 : 0);
    }
    MB_HD bool lheading_rule(int32_t start, int32_t end) {
        int32_t next = start + 1;
        bool found = false;
        while (next < end && !is_empty(next)) {
            if (sc(next) - st.blk > 3) { ++next; continue; }
            if (sc(next) >= st.blk) {
                const int32_t pos = bm(next) + ts(next), max = em(next);
                if (pos < max) {
                    const uint32_t m = d.cp[pos];
                    if (m == 0x2Du || m == 0x3Du) {
                        int32_t p = mb_skip_char(d.cp, pos, max, m);
                        p = mb_skip_spaces(d.cp, p, max);
                        if (p >= max) { found = true; break; }
                    }
                }
            }
            if (sc(next) < 0) { ++next; continue; }
            if (terminates(next, true, true)) break;
            ++next;
        }
        if (!found || st.status != MB_OK) return false;
        open(start, MB_HEADING);
        d.heading_end[start] = next + 1;
        st.line = next + 1;
        return true;
    }
    MB_HD void paragraph_rule(int32_t start) {
        const int32_t end = st.line_max;
        int32_t next = start + 1;
        while (next < end) {
            if (is_empty(next)) break;
            if (sc(next) - st.blk > 3) { ++next; continue; }
            if (sc(next) < 0) { ++next; continue; }
            if (terminates(next, true, true)) break;
            ++next;
        }
        open(start, MB_PARAGRAPH);
        st.line = next;
    }

    // ---- containers -------------------------------------------------------------------------------------------------------------------
    MB_HD MbFrame* push_frame(int32_t kind) {
        MbFrame* f = &d.frames[st.depth++];
        f->kind = kind;
        return f;
    }
    // One line of a quote: the marker at pos, one optional space behind it, the line's records as the quote's content sees them.
    MB_HD bool quote_line(int32_t l, int32_t pos, int32_t max) {
        ++pos;
        int32_t initial = sc(l) + 1, offset = initial;
        const uint32_t second = ch_at(pos, max);
        if (second == 0x20u) {
            ++pos;
            ++initial;
            ++offset;
        } else if (second == 0x09u) {
            undecided();
            return false;
        }
        save(l);
        d.bm[l] = pos;
        while (pos < max) {
            const uint32_t c = d.cp[pos];
            if (c == 0x09u) {
                undecided();
                return false;
            }
            if (c != 0x20u) break;
            ++offset;
            ++pos;
        }
        d.sc[l] = offset - initial;
        d.ts[l] = pos - d.bm[l];
        return pos >= max;  // the line is empty inside the quote
    }
    MB_HD void quote_begin(int32_t start, int32_t end) {
        MbFrame* f = push_frame(1);
        const int32_t tag = st.depth;
        f->start = start;
        f->old_line_max = st.line_max;
        f->old_blk = st.blk;
        f->save_base = st.n_save;
        bool last_empty = quote_line(start, bm(start) + ts(start), em(start));
        int32_t next = start + 1;
        while (next < end && st.status == MB_OK) {
            const bool outdented = sc(next) < st.blk;
            const int32_t pos = bm(next) + ts(next), max = em(next);
            if (pos >= max) break;
            if (d.cp[pos] == 0x3Eu && !outdented) {
                last_empty = quote_line(next, pos, max);
                ++next;
                continue;
            }
            if (last_empty) break;
            if (terminates(next, true, false)) {
                st.line_max = next;
                if (st.blk != 0 && !d.lazy[next]) {  // (a lazy line stays negative whatever is subtracted)
                    save(next);
                    d.sc[next] -= st.blk;
                }
                break;
            }
            if (!d.lazy[next]) d.lazy[next] = (uint8_t)tag;
            ++next;
        }
        st.blk = 0;
        open(start, MB_BLOCKQUOTE);
        ++st.level;
        f->scan_end = next;
        f->line = start;
        f->end = next;
    }
    MB_HD void quote_end(MbFrame* f) {
        --st.level;
        st.line_max = f->old_line_max;
        while (st.n_save > f->save_base) {
            const MbSave s = d.save[--st.n_save];
            d.bm[s.line] = s.bm;
            d.ts[s.line] = s.ts;
            d.sc[s.line] = s.sc;
        }
        const int32_t tag = st.depth;
        for (int32_t l = f->start; l < f->scan_end && l < d.n_lines; ++l)
            if (d.lazy[l] == tag) d.lazy[l] = 0;
        st.blk = f->old_blk;
        --st.depth;
    }
    // The head of the item loop: the item that starts at f->start with its marker ending at f->pos_after.
    MB_HD void item_begin(MbFrame* f) {
        const int32_t start = f->start, max = em(start);
        int32_t pos = f->pos_after;
        const int32_t initial = sc(start) + f->pos_after - (bm(start) + ts(start));
        int32_t offset = initial;
        while (pos < max) {
            const uint32_t c = d.cp[pos];
            if (c == 0x09u) {
                undecided();
                return;
            }
            if (c != 0x20u) break;
            ++offset;
            ++pos;
        }
        const int32_t content = pos;
        int32_t indent_after = content >= max ? 1 : offset - initial;
        if (indent_after > 4) indent_after = 1;
        if (st.level >= MB_MAX_LEVEL) {  // list_item_open
            undecided();
            return;
        }
        ++st.level;
        f->old_ts = d.ts[start];
        f->old_sc = d.sc[start];
        f->old_list_indent = st.list_indent;
        st.list_indent = st.blk;
        st.blk = initial + indent_after;
        d.ts[start] = content - d.bm[start];
        d.sc[start] = offset;
        if (content >= max && is_empty(start + 1)) {  // an empty item before an empty line: no tokenize
            st.line = st.line + 2 < f->list_end ? st.line + 2 : f->list_end;
            f->line = f->end = f->list_end;
        } else {
            f->line = start;
            f->end = f->list_end;
        }
    }
    // Behind an item's tokenize: true if another item follows (it is begun), false if the list is closed and its frame gone.
    MB_HD bool item_end(MbFrame* f) {
        st.blk = st.list_indent;
        st.list_indent = f->old_list_indent;
        d.ts[f->start] = f->old_ts;
        d.sc[f->start] = f->old_sc;
        --st.level;
        const int32_t next = st.line;
        f->start = next;
        bool more = next < f->list_end && !(sc(next) < st.blk) && !is_code(next) && !terminates(next, false, false);
        if (more) {
            int32_t value;
            const int32_t p = f->ordered ? skip_ordered_marker(next, &value) : skip_bullet_marker(next);
            more = p >= 0 && d.cp[p - 1] == (uint32_t)f->marker_char;
            f->pos_after = p;
        }
        if (more && st.status == MB_OK) {
            item_begin(f);
            return true;
        }
        --st.level;
        st.line = next;
        --st.depth;
        return false;
    }

    // ---- the main chain at a line where the tokenize loop tries its rules.  true: a container was pushed --------------------------------
    MB_HD bool try_rules(int32_t line, int32_t end) {
        if (st.level >= MB_MAX_LEVEL || st.depth >= MB_MAX_FRAMES) {
            undecided();
            return false;
        }
        if (is_code(line)) {
            code_rule(line, end);
            return false;
        }
        const int32_t pos = bm(line) + ts(line), max = em(line);
        const uint32_t c = ch_at(pos, max);
        uint32_t marker;
        int32_t length;
        if (fence_open(pos, max, &marker, &length)) {
            fence_rule(line, end, marker, length);
            return false;
        }
        if (c == 0x3Eu) {
            quote_begin(line, end);
            return true;
        }
        if (hr_at(pos, max)) {
            st.line = line + 1;
            return false;
        }
        int32_t ordered;
        const int32_t after = list_marker(line, false, &ordered);
        if (after >= 0) {
            MbFrame* f = push_frame(2);
            f->start = line;
            f->list_end = end;
            f->ordered = ordered;
            f->marker_char = (int32_t)d.cp[after - 1];
            f->pos_after = after;
            open(line, ordered ? MB_ORDERED_LIST : MB_BULLET_LIST);
            ++st.level;
            item_begin(f);
            return true;
        }
        if (c == 0x5Bu || c == 0x3Cu) {  // the reference rule, the html_block rule
            undecided();
            return false;
        }
        if (heading_at(pos, max)) {
            open(line, MB_HEADING);
            d.heading_end[line] = line + 1;
            st.line = line + 1;
            return false;
        }
        if (lheading_rule(line, end)) return false;
        if (st.status != MB_OK) return false;
        paragraph_rule(line);
        return false;
    }
    // Behind a rule, in the frame whose tokenize loop called it.
    MB_HD void after_rule(MbFrame* f) {
        int32_t line = st.line;
        if (line < f->end && is_empty(line)) {
            ++line;
            st.line = line;
        }
        f->line = line;
    }

    MB_HD int32_t parse() {
        st = MbState();
        st.line_max = d.n_lines;
        MbFrame* root = push_frame(0);
        root->line = 0;
        root->end = d.n_lines;
        // Every turn consumes a line in some frame, pushes a frame or pops one, and a frame is pushed at most once per line and depth.
        int64_t fuse = (int64_t)64 * ((int64_t)d.n_lines + 2);
        while (st.depth > 0 && st.status == MB_OK) {
            if (--fuse < 0) {
                undecided();
                break;
            }
            MbFrame* f = &d.frames[st.depth - 1];
            bool done = f->line >= f->end;
            if (!done) {
                const int32_t line = skip_empty_lines(f->line);
                st.line = line;
                done = line >= f->end || sc(line) < st.blk;
                if (!done) {
                    if (!try_rules(line, f->end) && st.status == MB_OK) after_rule(f);
                    continue;
                }
            }
            if (f->kind == 0) break;
            if (f->kind == 1) quote_end(f);
            else if (item_end(f)) continue;
            if (st.status == MB_OK) after_rule(&d.frames[st.depth - 1]);
        }
        return st.status;
    }
};

}  // namespace rl
