"""Generate `tests/golden/split_chunklets.npz` by running the REFERENCE's own `_split_chunklets` module -- TEST INFRASTRUCTURE.
Run in the authoring container only (needs the reference's source tree and markdown-it):

    python scripts/make_golden_chunklets.py [--reference /root/reference/src]

`src/raglite/_split_chunklets.py` needs numpy and markdown-it only; it is loaded through a stub `raglite` package (as
`oracle/make_golden_chunks.py` does) with a stub `raglite._typing`, because the real one pulls in the database layer.  The documents
are those of `tests/chunklets_ref.py: DOCUMENTS` (a seed and parameters of its text generator; the texts are not stored).  Per
document the file holds the reference's `boundary_probas`, `num_statements`, the sentence lengths (to notice a drifting generator)
and, for max_size in {64, 512, 2048}, the positions where the reference's chunklets start.  Data only.

Every stored case is checked on the spot: `raglite_amd._chunklets.chunklet_dp` must give the reference's cuts, and the two host
mirrors the reference's arrays bit for bit.  No case is excluded.
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

from tests.chunklets_ref import DOCUMENTS, GOLDEN, MAX_SIZES, make_sentences


def load_reference(src: Path):
    pkg = types.ModuleType("raglite")
    pkg.__path__ = [str(src / "raglite")]
    sys.modules["raglite"] = pkg
    typing_stub = types.ModuleType("raglite._typing")
    typing_stub.FloatVector = np.ndarray
    sys.modules["raglite._typing"] = typing_stub
    from raglite import _split_chunklets as ref  # REAL reference module

    return ref


def cuts_of(sentences: list[str], chunklets: list[str]) -> list[int]:
    """Where the chunklets start, from their lengths (the sentences are non-empty, so the character prefix is strictly ascending)."""
    pc = np.concatenate(([0], np.cumsum([len(s) for s in sentences])))
    ends = np.cumsum([len(c) for c in chunklets])
    pos = np.searchsorted(pc, ends)
    assert np.array_equal(pc[pos], ends) and pos[-1] == len(sentences) and "".join(chunklets) == "".join(sentences)
    return pos[:-1].tolist()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference/src")
    args = ap.parse_args()
    ref = load_reference(Path(args.reference))
    from raglite_amd._chunklets import chunklet_dp, compute_num_statements, markdown_chunklet_boundaries

    out: dict[str, np.ndarray] = {}
    checked = 0
    for d, m in enumerate(DOCUMENTS):
        sentences = make_sentences(m["seed"], m["n"], m["kind"], m.get("long_at", ()))
        assert len(sentences) == m["n"] and all(sentences)
        boundary = np.asarray(ref.markdown_chunklet_boundaries(sentences), dtype=np.float64)
        statements = np.asarray(ref.compute_num_statements(sentences), dtype=np.float64)
        lengths = np.asarray([len(s) for s in sentences], dtype=np.int64)
        assert markdown_chunklet_boundaries(sentences).tobytes() == boundary.tobytes(), f"document {d}: boundary mirror"
        assert compute_num_statements(sentences).tobytes() == statements.tobytes(), f"document {d}: statements mirror"
        out[f"doc{d}_boundary"], out[f"doc{d}_statements"], out[f"doc{d}_lengths"] = boundary, statements, lengths
        for max_size in MAX_SIZES:
            cuts = cuts_of(sentences, ref.split_chunklets(sentences, max_size=max_size))
            mine, _, status = chunklet_dp(boundary, statements, lengths, max_size)
            assert mine == cuts, f"document {d}, max_size {max_size}: chunklet_dp {mine} != reference {cuts}"
            assert status == int(lengths.max() > max_size)
            out[f"doc{d}_cuts_{max_size}"] = np.asarray(cuts, dtype=np.int64)
            checked += 1
    out["meta_json"] = np.asarray(json.dumps(list(DOCUMENTS)))
    np.savez_compressed(GOLDEN, **out)
    print(f"wrote {GOLDEN} ({GOLDEN.stat().st_size} bytes): {len(DOCUMENTS)} documents, {checked} cases, chunklet_dp equals the "
          "reference's cuts on all of them")


if __name__ == "__main__":
    main()
