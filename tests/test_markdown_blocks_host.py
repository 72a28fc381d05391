"""The Markdown block parser (raglite_amd/csrc/markdown_blocks.h) on the CPU.

The header is plain C++ over plain pointers, so tests/c/markdown_blocks_main.cpp runs the code the device runs, compiled here with the
host compiler under AddressSanitizer and UBSan (a stand-alone program: nothing is loaded into Python under a sanitizer).  Over the
whole fixture (tests/golden/markdown_blocks.json: markdown-it-py's tokens, recorded by scripts/make_golden_markdown_blocks.py) every
decided document must give the recorded tokens' first_open and heading_end, the sanitizers must stay silent, corpus A must be decided
throughout, and a document may be undecided only if its text holds a character that allows it.

The second half needs markdown-it: it shows that the two per-line arrays carry all that the splitters' host functions take from the
tokens."""

import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import markdown_blocks_ref as ref

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "c" / "markdown_blocks_main.cpp"
HEADERS = ROOT / "raglite_amd" / "csrc"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("markdown_blocks") / "markdown_blocks_main"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{HEADERS}", str(DRIVER),
           "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _run(driver, tmp_path, texts):
    path = tmp_path / "input.bin"
    ref.write_driver_input(path, texts)
    res = subprocess.run([str(driver), str(path)], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, f"exit {res.returncode}\n{res.stderr[-4000:]}"  # a sanitizer report goes to stderr
    docs = ref.read_driver_output(res.stdout)
    assert len(docs) == len(texts)
    return docs


@pytest.mark.parametrize("group", ["hand", "edges", "fuzz_a", "fuzz_b"])
def test_fixture_tokens_on_the_cpu(driver, tmp_path, group):
    cases = ref.cases(group)
    docs = _run(driver, tmp_path, [c["text"] for c in cases])
    decided = 0
    for case, (status, first_open, heading_end) in zip(cases, docs):
        text = case["text"]
        if status == ref.UNDECIDED:
            assert (group == "edges" and case["name"] in ("level_16", "lists_8")) or (group != "fuzz_a" and ref.may_be_undecided(text)), \
                f"undecided without a reason: {text!r}"
            continue
        decided += 1
        assert len(first_open) == len(text.splitlines()), repr(text)
        want_open, want_end = ref.reduce_tokens(case["tokens"], len(first_open))
        assert np.array_equal(first_open, want_open) and np.array_equal(heading_end, want_end), f"{case.get('name')}: {text!r}"
    assert decided > 0
    if group == "fuzz_b":
        assert decided < len(cases), "corpus B must hold undecided documents"


def test_hand_cases_are_undecided_only_where_meant(driver, tmp_path):
    cases = ref.cases("hand")
    docs = _run(driver, tmp_path, [c["text"] for c in cases])
    undecided = {c["name"] for c, (status, _, _) in zip(cases, docs) if status == ref.UNDECIDED}
    assert undecided == {"html_block", "reference", "tab_indent", "u2028"}
    cases = ref.cases("edges")
    docs = _run(driver, tmp_path, [c["text"] for c in cases])
    undecided = {c["name"] for c, (status, _, _) in zip(cases, docs) if status == ref.UNDECIDED}
    assert undecided == {"level_16", "lists_8"}


def _nested(depth: int) -> str:
    return "> " * depth + "a\n"


def test_nesting_levels(driver, tmp_path):
    """A paragraph in 15 quotes opens at level 15 (decided), in 16 quotes at level 16 (undecided); lists count two levels each."""
    texts = [_nested(15), _nested(16), "- " * 7 + "a\n", "- " * 8 + "a\n"]
    (s15, open15, _), (s16, _, _), (l7, open7, _), (l8, _, _) = _run(driver, tmp_path, texts)
    assert (s15, s16, l7, l8) == (ref.OK, ref.UNDECIDED, ref.OK, ref.UNDECIDED)
    assert open15.tolist() == [2] and open7.tolist() == [4]


def test_reduction_reproduces_the_host_functions():
    pytest.importorskip("markdown_it")
    from markdown_it import MarkdownIt

    from raglite_amd._chunklets import markdown_chunklet_boundaries
    from raglite_amd._sentences import markdown_sentence_boundaries

    rng = np.random.default_rng(7)
    for case in ref.cases():
        text = case["text"]
        live = [[t.type, t.map[0], t.map[1]] for t in MarkdownIt().parse(text) if t.map is not None and t.type != "inline"]
        assert live == case["tokens"], f"the fixture is stale: {text!r}"
        first_open, heading_end = ref.reduce_tokens(live, len(text.splitlines()))
        assert np.array_equal(ref.known_from_lines(text, heading_end), markdown_sentence_boundaries(text), equal_nan=True), repr(text)
        for _ in range(2):
            sentences = ref.random_sentences(text, rng)
            assert np.array_equal(ref.boundaries_from_lines(sentences, first_open), markdown_chunklet_boundaries(sentences)), repr(sentences)
