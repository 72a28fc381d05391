"""Writes tests/golden/markdown_blocks.json: documents and the block tokens markdown-it-py gives for them, the fixture of the device
Markdown block parser.

    python scripts/make_golden_markdown_blocks.py [--fuzz N]

Every case is {"text", "tokens"}; tokens is the list of [type, map[0], map[1]] of `MarkdownIt().parse(text)` for every block token
that has a map (inline tokens are left out).  Four groups: "hand" (named cases), "edges" (named cases sized for the kernels), "fuzz_a" (documents of 1-14 lines joined from
fragments, none of which can make the parser give a document up) and "fuzz_b" (the same with `<div>`, `[a]: b`, tabs and U+2028 among
the fragments).  With --fuzz N nothing is written: N fresh documents per corpus are generated and printed as one JSON object, for
checks beyond the fixture."""

from __future__ import annotations

import argparse
import json
import random
import sys
from pathlib import Path

from markdown_it import MarkdownIt

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "markdown_blocks.json"

HAND = {
    "atx_closing": "# one #\n## two ##   \n### three # x\n####### seven\n#nospace\n#\n# \n",
    "setext_eq": "Title\n=====\n\ntext\n",
    "setext_dash": "Title\nmore\n---\ntext\n",
    "setext_vs_hr": "para\n- - -\nnext\n\npara\n***\n",
    "setext_vs_empty_bullet": "para\n-\nnext\n\npara\n- \nnext\n",
    "indent3": "   # h\n   > q\n   - i\n   ---\n   ```\n   x\n   ```\n",
    "indent4": "    # h\n    > q\n\ntext\n    lazy code\n\n    code\n\n    more\nend\n",
    "fence_unclosed": "```py\ncode\n# not a heading\n",
    "fence_in_quote": "> ```\n> code\nnot lazy\n> after\n",
    "fence_in_list": "- ```\n  code\n outdented\n- next\n",
    "fence_tilde_backtick": "~~~ a`b\nx\n~~~~\n``` a`b\ny\n```\n",
    "lazy_quote": "> a\nlazy\n> b\n\n> c\n# h\n",
    "lazy_list": "- a\nlazy\n  b\n\n  c\n",
    "quote_then_empty": ">\ntext\n> x\n>\ntext\n",
    "ordered_interrupt": "para\n2. two\n1. one\n\n3. three\n4) four\n",
    "empty_item_no_interrupt": "para\n-\n*\n\n-\n\n  foo\n- \n  bar\n",
    "marker_change": "- a\n- b\n+ c\n* d\n1. e\n1) f\n",
    "four_level_continuation": "- item 1\n - item 2\n  - item 3\n   - item 4\n    - continuation\n",
    "container_heading": "> # h\n- # h\n1. ## h\n> - # h\n",
    "consecutive_headings": "# a\n## b\n### c\nd\n===\ne\n---\n# f",
    "heading_at_eof": "text\n\n# last",
    "empty": "",
    "blank_lines": "\n\n   \n\n",
    "trailing_spaces_line": "a\n   ",
    "crlf": "# h\r\ntext\r\n\r\n- a\r\n- b\r\n",
    "lone_cr": "# h\rtext\r\r> q\rlazy\r",
    "mixed_breaks": "a\r\n\rb\n\r\nc\r",
    "nested": "> - a\n>   b\n> - c\n>\n>   > d\n> e\n",
    "loose_list": "- a\n\n- b\n\n\n- c\n",
    "list_code_end": "- a\n\n      code\n    code4\n",
    "ordered_long": "123456789. ok\n1234567890. no\n",
    "quote_in_list_outdent": "1. a\n   > q\n2. b\n   > r\n  # h\n",
    "hr_kinds": "***\n---\n___\n* * *\n -  -  -\n**\n--\n__ _\n",
    "html_block": "<div>\nx\n</div>\n",
    "reference": "[a]: b\n\n[a]\n",
    "tab_indent": "\tcode\n-\tx\n>\ty\n",
    "u2028": "a\u2028# b\n",
    "angle_inside": "a < b\n\\<x\n    <code>\n```\n<in fence>\n```\n",
}

# Shapes that cross the kernels' own edges: more lines than one 64-line block of the line table, lines longer than the 64 characters a
# wave scans per step, and the nesting levels on both sides of the limit.
EDGES = {
    "lines_200": "# h\npara\n\n> q\n" * 50,
    "hr_300": "para\n" + "- " * 150 + "\n" + "* " * 150 + "\n" + "*" * 300 + "\n" + "_" * 64 + "\n" + "_" * 65 + "\n",
    "not_hr_300": "para\n" + "-" * 200 + "x" + "-" * 99 + "\n\n" + "*" * 299 + "x\n" + "_" * 63 + "x\n" + "_" * 64 + "x\n",
    "fence_long": "`" * 100 + "\ncode\n" + "`" * 99 + "\n# swallowed\n" + "`" * 130 + "  \n# h\n" + "~" * 70 + " a`b\n# in\n" + "~" * 70 + " x\n",
    "fence_info_backtick": "`" * 70 + " " * 70 + "`\n# h\n",
    "setext_long": "title\n" + "=" * 300 + "   \nt2\n" + "-" * 299 + " x\nt3\n" + "-" * 128 + "\n",
    "level_15": "> " * 15 + "a\n",
    "level_16": "> " * 16 + "a\n",
    "lists_7": "- " * 7 + "a\n",
    "lists_8": "- " * 8 + "a\n",
    "deep_lazy": "> > > a\nlazy\nlazy2\n> > b\n\n> - > c\nlazy3\n# h\n",
    "long_item": "-" + " " * 3 + "x" * 200 + "\n" + " " * 4 + "y" * 100 + "\n" + "1." + " " * 70 + "code\n",
}

FRAGMENTS_A = [
    "", "", " ", "text", "more text here", "  two", "   three", "    four", "     five", "# h", "## h ##", "#", "#x", "   ### h", "    # h",
    "===", "---", "--", "-", "- ", "***", "* * *", "___", " - - -", "=", "== ", "> q", ">", "> ", ">q", " > q", "> > q", ">> ", "> # h",
    "> - a", "> ```", "> ---", ">     code", "- a", "-a", "* b", "+ c", "  - n", "   - n3", "    - n4", "      - n6", "- - a", "- # h",
    "- > q", "- ```", "-   wide", "-      code", "1. a", "2. b", "1) c", "10. d", "  1. n", "   2. n", "1.", "1. ", "1.x", "```",
    "````", "``` x", "``` a`b", "~~~", "~~~~ ", "  ```", "    ```", "``", "\\# no", "&amp;", "*em*", "`code`",
    "  ", "   ", "    ", "  text  ", "- a\\", "> - > x", "1. > - y", "   > q3", "    > q4",
]
FRAGMENTS_B = [*FRAGMENTS_A, "<div>", "</div>", "<!-- c -->", " <b>x</b>", "[a]: b", "[link](x)", " [r]: /u 't'", "\tcode", " \tx", "-\tx",
               ">\ty", "1.\tz", "a\tb", "a\u2028b", "\u2028", "a < b", "a [b] c", "> <p>", "- [x] task", "-  [", "> [q]: r", "a\x0bb", "a\x85b"]
SEPARATORS = ["\n"] * 12 + ["\r\n", "\r"]


def tokens_of(text: str) -> list[list]:
    return [[t.type, t.map[0], t.map[1]] for t in MarkdownIt().parse(text) if t.map is not None and t.type != "inline"]


def fuzz(rng: random.Random, fragments: list[str], count: int) -> list[dict]:
    out = []
    for _ in range(count):
        lines = [rng.choice(fragments) for _ in range(rng.randint(1, 14))]
        sep = rng.choice(SEPARATORS) if rng.random() < 0.85 else None
        text = "".join(line + (sep or rng.choice(SEPARATORS)) for line in lines)
        if rng.random() < 0.4:
            text = text[: len(text) - (2 if text.endswith("\r\n") else 1)]  # no line break at the end
        out.append({"text": text, "tokens": tokens_of(text)})
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--fuzz", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.fuzz:
        rng = random.Random(args.seed)
        json.dump({"hand": [], "edges": [], "fuzz_a": fuzz(rng, FRAGMENTS_A, args.fuzz), "fuzz_b": fuzz(rng, FRAGMENTS_B, args.fuzz)}, sys.stdout)
        return
    rng = random.Random(20260)
    data = {
        "hand": [{"name": name, "text": text, "tokens": tokens_of(text)} for name, text in HAND.items()],
        "edges": [{"name": name, "text": text, "tokens": tokens_of(text)} for name, text in EDGES.items()],
        "fuzz_a": fuzz(rng, FRAGMENTS_A, 150),
        "fuzz_b": fuzz(rng, FRAGMENTS_B, 100),
    }
    OUT.write_text(json.dumps(data, ensure_ascii=True, separators=(",", ":")) + "\n")
    print(f"{OUT}: {OUT.stat().st_size} bytes, {sum(len(v) for v in data.values())} documents")


if __name__ == "__main__":
    main()
