"""The analyzer as a table and a rule (raglite_amd/_keyword.py: `fold_table`, `tokenize_by_table`): what the device
runs, checked on the host against the specification, `_keyword.normalize` / `_keyword.tokenize`."""

import random

import numpy as np

from raglite_amd import _keyword

# the code points the per-code-point fold has to get right: combining marks, dotted capital I, ligatures, the DZ digraph, the Kelvin
# sign, both sigmas, capital sharp s, circled digits, a squared unit, the longest image (U+FDFA), the longest letter image (U+2167),
# the six-symbol image (U+33AF), mathematical bold, Hangul, the three backslashes
SPECIAL = ("̧́̈İﬁﬃǄǆKσςΣẞß①⑳㏏ﷺⅧ㎯"
           "\U0001d400\U0001d41a한글ᄒ﹨＼ÉéüAZ")
LINE_ENDS = "\n\r\u0085 "


def _classes(text: str) -> list[int]:
    """The symbol classes of an already normalized string, separator runs collapsed (written out here, not taken from the module)."""
    out: list[int] = []
    for ch in text:
        if "a" <= ch <= "z":
            out.append(ord(ch) - ord("a"))
        elif ch == "\\":
            out.append(27)
        elif ch == "\n":
            out.append(28)
        elif not out or out[-1] != 26:
            out.append(26)
    return out


def _decode(entry: int) -> list[int]:
    out = []
    while entry & 31:
        out.append((entry & 31) - 1)
        entry >>= 5
    assert entry == 0  # nothing behind an empty field
    return out


def test_fold_table_matches_normalize_for_every_code_point():
    table = _keyword.fold_table()
    assert table.dtype == np.uint32 and table.shape == (0x110000,)
    entries = table.tolist()
    n_letters = n_empty = longest = longest_letters = 0
    backslashes, newlines = [], []
    for cp in range(0x110000):
        if 0xD800 <= cp <= 0xDFFF:
            continue
        want = _classes(_keyword.normalize(chr(cp)))
        got = _decode(entries[cp])
        assert got == want, hex(cp)
        letters = sum(s < 26 for s in got)
        n_letters += letters > 0
        n_empty += not got
        longest, longest_letters = max(longest, len(got)), max(longest_letters, letters)
        if 27 in got:
            backslashes.append(cp)
        if 28 in got:
            newlines.append(cp)
    assert longest <= _keyword.FOLD_IMAGE_MAX
    # the facts the device layout rests on
    assert backslashes == [0x5C, 0xFE68, 0xFF3C] and newlines == [0x0A]
    assert all(_decode(entries[cp]) == [27] for cp in backslashes) and _decode(entries[0x0A]) == [28]
    assert longest_letters == 4 and _decode(entries[0x2167]) == [ord(c) - 97 for c in "viii"]
    assert n_letters > 1000 and n_empty > 500
    assert all(_decode(entries[cp]) == [26] for cp in (0xD800, 0xDFFF))  # a lone surrogate separates


def _random_text(rng: random.Random) -> str:
    parts = []
    for _ in range(rng.randint(0, 14)):
        r = rng.random()
        if r < 0.30:
            parts.append("\\" * rng.randint(1, 9))
        elif r < 0.45:
            parts.append(rng.choice(LINE_ENDS))
        elif r < 0.65:
            parts.append(rng.choice(SPECIAL))
        elif r < 0.90:
            parts.append(rng.choice("abyz"))
        elif r < 0.95:
            parts.append(rng.choice(" .,-_0\t"))
        else:
            parts.append(chr(rng.choice((rng.randint(0x20, 0x24F), rng.randint(0x370, 0x3FF), rng.randint(0x2000, 0x33FF)))))
    return "".join(parts)


def test_restated_tokenizer_equals_tokenize_on_random_strings():
    rng = random.Random(20261019)
    for i in range(100_000):
        text = _random_text(rng)
        assert _keyword.tokenize_by_table(text) == _keyword.tokenize(text), (i, text)


def test_restated_tokenizer_on_the_named_cases():
    cases = {
        "\\ﬁx": ["ix"],               # the backslash consumes the f of the ligature
        "\\́a": [],                   # an empty image is no symbol: the a is consumed
        "\\\\a": ["a"],
        "\\\na": ["a"],                    # a newline is never consumed
        "a\\\r b": ["a", "b"],
        "ab﹨cd ＼＼ef": ["ab", "d", "ef"],
        "Ⅷ": ["viii"],
        "\\Ⅷ": ["iii"],
        "x\\": ["x"],
    }
    for text, want in cases.items():
        assert _keyword.tokenize(text) == want, text
        assert _keyword.tokenize_by_table(text) == want, text
