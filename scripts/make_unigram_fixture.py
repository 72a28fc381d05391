#!/usr/bin/env python
"""Make the Unigram fixture of the device SentencePiece tokenizer: tests/golden/unigram_2k.model, a 2 000-piece Unigram
model with `nmt_nfkc` normalisation trained on this repository's own Markdown, and tests/golden/unigram_2k_cases.json, the test texts
with the library's ids and normalised strings recorded.  The tests read the two committed files and never retrain.

    python scripts/make_unigram_fixture.py
"""

from __future__ import annotations

import io
import json
import random
import re
import sys
from pathlib import Path

import sentencepiece as spm
from sentencepiece import sentencepiece_model_pb2 as pb

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tests.sentencepiece_ref import batch_of, digest  # noqa: E402 - the batch's texts and digest, stated once
GOLDEN = ROOT / "tests" / "golden"
TOOL_NAMES = ("gpu" + "run",)  # lines that name a job runner of some test machine teach the fixture nothing: left out of the corpus
OOV_CANDIDATES = "中文字🙂☃→∑ж漢仮한"  # main() keeps those that the trained vocabulary does not hold


def corpus() -> list[str]:
    lines = []
    for path in sorted([*ROOT.glob("*.md"), *ROOT.glob("docs/*.md"), *ROOT.glob("profiles/*.md")]):
        for line in path.read_text(encoding="utf-8", errors="replace").splitlines():
            line = line.strip()
            if line and not any(name in line.lower() for name in TOOL_NAMES):
                lines.append(line[:4000])
    return lines


def train(lines: list[str]) -> bytes:
    model = io.BytesIO()
    spm.SentencePieceTrainer.train(sentence_iterator=iter(lines), model_writer=model, model_type="unigram", vocab_size=2000,
                                   normalization_rule_name="nmt_nfkc", num_threads=1, unk_id=0, bos_id=1, eos_id=2, pad_id=-1,
                                   minloglevel=2)
    return model.getvalue()


def cases(sp: spm.SentencePieceProcessor, longest: int, words: list[str], OOV: str) -> dict:  # noqa: N803
    rng = random.Random(2025)
    word = lambda: rng.choice(words)  # noqa: E731
    sentence = lambda n: " ".join(word() for _ in range(n))  # noqa: E731
    oov = lambda n: "".join(rng.choice(OOV) for _ in range(n))  # noqa: E731
    edge = {
        "ascii": "The quick brown fox jumps over the lazy dog, and the kernel writes one row per query.",
        "runs_of_space": "a  b   c\t\td \n\n e \t\n f",
        "leading_only": "   leading spaces",
        "trailing_only": "trailing spaces   ",
        "nbsp_ideographic_zwsp": "no break 　ideographic　 zero​width  　 end",
        "empty_images_last": "control characters at the end \x7f\x01",  # (nmt_nfkc drops them: empty images)
        "empty_images_only": "\x7f\x01\x02",
        "space_then_empty_images": "word \x7f",
        "ligature_circled": "ﬁne ﬂow ① ② ㍿ ½ ǆ",
        "fdfa": "ﷺ",
        "fdfa_in_text": "before ﷺ after",
        "full_width": "ＡＢＣ　ｆｕｌｌ　ｗｉｄｔｈ　１２３！",
        "cjk": "漢字仮名交じり文 中文分词",
        "hangul_precomposed": "한국어 문장 입니다",
        "one_symbol": "▁",
        "one_letter": "a",
        "run_L": "e" * (longest - 1),
        "run_L_plus_1": "e" * longest,
        "run_long": "e" * (3 * longest + 5),
        "run_long_upper": "Q" * (2 * longest + 3),
        "oov_start": oov(3) + " then words",
        "oov_middle": "words " + oov(4) + " then words",
        "oov_end": "words then " + oov(2),
        "oov_across_space": "words " + oov(2) + " " + oov(3) + " words",
        "oov_inside_word": "ker" + oov(2) + "nel",
        "oov_only": oov(5),
        "empty": "",
        "space_only": "   \t \n ",
        "literal_mark": "a▁b ▁ c",
    }
    for n in (longest - 1, longest, longest + 1, 63, 64, 65):
        edge[f"symbols_{n}"] = ("ab " * n)[: n - 2] + "c"  # (n - 1 code points, a letter first and last: n symbols with the dummy prefix)
    for n in (255, 256, 257, 2047, 2048, 2049):
        edge[f"expanded_{n}"] = "x" * (n % 18) + "ﷺ" * (n // 18)  # n symbols after the expansion (U+FDFA has an image of 18)
    texts = dict(edge)
    texts["words_3000"] = sentence(3000)
    names = list(texts)
    rec = {"names": names, "texts": [texts[k] for k in names]}
    rec["ids"] = [sp.encode(t) for t in rec["texts"]]
    rec["normalized"] = [sp.normalize(t) for t in rec["texts"]]
    # about 20 000 words over 300 texts: many blocks, two scan levels.  The texts are arithmetic over the words of the 3 000-word text
    # (tests/sentencepiece_ref.py: batch_of), so only a digest of the library's ids is recorded
    batch = batch_of(sorted(set(texts["words_3000"].split())), OOV)
    rec["batch_sha256"] = digest(sp.encode(batch))
    rec["batch_tokens"] = sum(map(len, sp.encode(batch)))
    rec["longest_piece"] = longest
    return rec


def main() -> None:
    lines = corpus()
    proto = train(lines)
    m = pb.ModelProto()
    m.ParseFromString(proto)
    assert m.trainer_spec.model_type == 1 and m.pieces[0].type == 2, "a Unigram model with <unk> = 0"
    longest = max(len(p.piece) for p in m.pieces if p.type == 1)
    sp = spm.SentencePieceProcessor(model_proto=proto)
    oov = "".join(c for c in OOV_CANDIDATES if sp.encode(c) == [sp.piece_to_id("▁"), 0])
    assert len(oov) >= 4, "too few out-of-vocabulary characters"
    words = sorted({w for line in lines for w in re.findall(r"[A-Za-z][A-Za-z0-9_\-']{0,15}", line)})
    rec = cases(sp, longest, words, oov)
    rec["oov"] = oov
    GOLDEN.mkdir(parents=True, exist_ok=True)
    (GOLDEN / "unigram_2k.model").write_bytes(proto)
    (GOLDEN / "unigram_2k_cases.json").write_text(json.dumps(rec, ensure_ascii=False, separators=(",", ":")) + "\n", encoding="utf-8")
    print(f"unigram_2k.model {len(proto)} bytes, longest piece {longest}; {len(rec['texts'])} cases, "
          f"{rec['batch_tokens']} batch tokens, 3000-word text {len(rec['ids'][-1])} tokens")


if __name__ == "__main__":
    main()
