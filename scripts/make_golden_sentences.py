"""Generate `tests/golden/split_sentences.npz` by running the REFERENCE's own `_split_sentences` module -- TEST INFRASTRUCTURE.
Run in the authoring container only (needs the reference's source tree and markdown-it):

    python scripts/make_golden_sentences.py [--reference /root/reference/src]

`src/raglite/_split_sentences.py` needs numpy, markdown-it and `wtpsplit_lite`.  It is loaded through a stub `raglite` package with a
stub `raglite._typing` (the real one pulls in the database layer) and a stub `wtpsplit_lite` whose `SaT.predict_proba(doc, **kw)`
returns the stored synthetic probabilities of that document: the model is the one part of the reference that is not run.  The
documents are those of `tests/sentences_ref.py: DOCUMENTS` (a seed and parameters of its text generator; the texts are not stored).
Per document the file holds the predictions (float32 or float64), the reference's `markdown_sentence_boundaries` and, for every
(min_len, max_len) of `CASES`, the positions where the reference's sentences start, or the fact that it raised.  Data only.

Every stored case is checked on the spot: `raglite_amd._sentences.sentence_partition` with `whitespace_mask` must give the reference's
sentences (or status 3 where it raised), and the Markdown mirror the reference's array bit for bit.  No case is excluded.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import types
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from tests.sentences_ref import CASES, DOCUMENTS, GOLDEN, make_document, make_predictions

_PREDICTIONS: dict[str, np.ndarray] = {}


def load_reference(src: Path):
    pkg = types.ModuleType("raglite")
    pkg.__path__ = [str(src / "raglite")]
    sys.modules["raglite"] = pkg
    typing_stub = types.ModuleType("raglite._typing")
    typing_stub.FloatVector = np.ndarray
    sys.modules["raglite._typing"] = typing_stub

    class SaT:
        def __init__(self, name: str) -> None:
            self.name = name

        def predict_proba(self, doc: str, **kwargs):
            return _PREDICTIONS[doc]

    model_stub = types.ModuleType("wtpsplit_lite")
    model_stub.SaT = SaT
    sys.modules["wtpsplit_lite"] = model_stub
    from raglite import _split_sentences as ref  # REAL reference module

    return ref


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference/src")
    args = ap.parse_args()
    ref = load_reference(Path(args.reference))
    from raglite_amd._sentences import SENTENCES_NO_SPLIT, markdown_sentence_boundaries, sentence_partition, whitespace_mask

    out: dict[str, np.ndarray] = {}
    checked = raised = phase2 = 0
    for d, m in enumerate(DOCUMENTS):
        doc = make_document(m["seed"], m["blocks"], m["kind"], m.get("lead", ""), m.get("trail", ""))
        predictions = make_predictions(doc, m["seed"], m["dtype"])
        _PREDICTIONS[doc] = predictions
        known = np.asarray(ref.markdown_sentence_boundaries(doc), dtype=np.float64)
        assert markdown_sentence_boundaries(doc).tobytes() == known.tobytes(), f"document {d}: Markdown mirror"
        space = whitespace_mask(doc)
        assert space.tolist() == [int(c.isspace()) for c in doc], f"document {d}: white-space mirror"
        out[f"doc{d}_predictions"], out[f"doc{d}_known"], out[f"doc{d}_length"] = predictions, known, np.asarray(len(doc))
        for min_len, max_len in CASES:
            key = f"doc{d}_starts_{min_len}_{max_len or 0}"
            bounds, _, status = sentence_partition(predictions, space, min_len, max_len, known)
            try:
                sentences = ref.split_sentences(doc, min_len=min_len, max_len=max_len)
            except ValueError:
                assert status == SENTENCES_NO_SPLIT and not bounds, f"document {d}, {min_len, max_len}: the reference raised, status {status}"
                out[key], out[key + "_raised"] = np.zeros(0, np.int64), np.asarray(True)
                raised += 1
            else:
                assert "".join(sentences) == doc and all(sentences)
                starts = np.cumsum([len(s) for s in sentences])[:-1].tolist()
                assert [b + 1 for b in bounds] == starts, f"document {d}, {min_len, max_len}: sentence_partition != reference"
                longest = max(len(s) for s in sentences)
                assert status == int(max_len is not None and longest > max_len), f"document {d}, {min_len, max_len}: status {status}"
                if max_len is not None and len(starts) > len(sentence_partition(predictions, space, min_len, None, known)[0]):
                    phase2 += 1
                out[key], out[key + "_raised"] = np.asarray(starts, dtype=np.int64), np.asarray(False)
            checked += 1
    # the two tie rules on constant probabilities, from the reference's programme itself (40 characters, min_len 4)
    from raglite_amd._sentences import sentence_dp

    for name, proba, max_len in (("ties_earliest", 0.5, None), ("ties_latest", 0.25, 12)):
        lengths = [len(s) for s in ref._split_sentences("x" * 40, np.full(40, proba), min_len=4, max_len=max_len)]  # noqa: SLF001
        mine = np.diff([0, *[b + 1 for b in sentence_dp(np.full(40, proba), 4, max_len)[0]], 40]).tolist()
        assert mine == lengths, f"{name}: sentence_dp {mine} != reference {lengths}"
        out[name] = np.asarray(lengths, dtype=np.int64)
        checked += 1
    out["meta_json"] = np.asarray(json.dumps(list(DOCUMENTS)))
    np.savez_compressed(GOLDEN, **out)
    print(f"wrote {GOLDEN} ({GOLDEN.stat().st_size} bytes): {len(DOCUMENTS)} documents, {checked} cases ({raised} where the reference "
          f"raised, {phase2} where phase 2 added boundaries), 0 excluded: sentence_partition equals the reference on all of them")


if __name__ == "__main__":
    main()
