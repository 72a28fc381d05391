"""The chunk-similarity operation of `rl_partition_similarity` (`_split_chunks.py:54-72`) stated in float64, NumPy only.

Per document, with the `nonoutlying` mask given explicitly (or None):

  1. X      = rows normalised to unit length;
  2. if any row is selected: d = normalised mean of the selected rows of X, X_mod = X - (X . d) d;
  3. branch:
       `no_selection`  no mask, or no selected row: the plain rows X;
       `degenerate`    some ||X_mod row|| <= eps32: the plain rows X;
       `mod`           otherwise: the rows of X_mod, re-normalised;
  4. s[i]   = row i . row i + 1;
  5. sim[i] = max((s[i] + 1) / 2, sqrt(eps32)), eps32 and its root being the float32 constants;
  6. sim[last row] = 0 (the layout of the kernel: one entry per row, the last unused).

The one-selected-row rule.  A document whose mask selects exactly ONE row has d equal to that row, so in exact arithmetic that
row's X_mod is zero and the document is `degenerate`.  In float64, as in float32, the residual is rounding noise of the size of
the threshold, so arithmetic cannot decide it; this statement therefore decides it by the count: one selected row -> `degenerate`,
the smallest ||X_mod row|| reported as 0.  (The reference's own float32 code decides this case by rounding.)

Documents whose SEVERAL selected rows are all identical sit on the same threshold; callers that need a deterministic answer there
build them so that the arithmetic is exact (all selected rows one axis e_j: norms, d and the projection are then exact).
"""

import numpy as np

EPS32 = np.float32(np.finfo(np.float32).eps)
SQRT_EPS32 = np.sqrt(EPS32)  # float32
BRANCHES = ("no_selection", "degenerate", "mod")


def document(X, sel=None):
    """One document.  X (n, dim), sel bool / uint8 [n] or None ->
    (sim float64[n], branch, smallest ||X_mod row|| (nan without a selection), ||X_mod row|| float64[n] (nan likewise))."""
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    no_norms = np.full(n, np.nan)
    if n == 0:
        return np.zeros(0), "no_selection", np.nan, no_norms
    with np.errstate(invalid="ignore", divide="ignore"):
        X = X / np.linalg.norm(X, axis=1, keepdims=True)
    rows, branch, smallest, norms = X, "no_selection", np.nan, no_norms
    mask = None if sel is None else np.asarray(sel).astype(bool)
    if mask is not None and mask.any():
        with np.errstate(invalid="ignore", divide="ignore"):
            d = X[mask].mean(axis=0)
            d = d / np.linalg.norm(d)
            X_mod = X - np.outer(X @ d, d)
            norms = np.linalg.norm(X_mod, axis=1)
            if int(mask.sum()) == 1:  # the one-selected-row rule (module docstring)
                norms = norms.copy()
                norms[np.flatnonzero(mask)[0]] = 0.0
            smallest = float(np.min(norms))
            if np.any(norms <= np.float64(EPS32)):
                branch = "degenerate"
            else:
                branch, rows = "mod", X_mod / norms[:, None]
    sim = np.zeros(n)
    s = np.sum(rows[:-1] * rows[1:], axis=1)
    sim[:-1] = np.maximum((s + 1.0) / 2.0, np.float64(SQRT_EPS32))
    return sim, branch, smallest, norms


def batch(X, doc_offsets=None, sel=None):
    """`document` over a CSR batch -> (sim float64[n], branches [n_docs], smallest float64[n_docs], norms float64[n])."""
    X = np.asarray(X)
    off = np.asarray([0, len(X)] if doc_offsets is None else doc_offsets, dtype=np.int64)
    sim, norms = np.zeros(len(X)), np.full(len(X), np.nan)
    branches, smallest = [], np.full(len(off) - 1, np.nan)
    for d in range(len(off) - 1):
        b, e = int(off[d]), int(off[d + 1])
        sim[b:e], branch, smallest[d], norms[b:e] = document(X[b:e], None if sel is None else sel[b:e])
        branches.append(branch)
    return sim, branches, smallest, norms


def tol_plain(dim):
    """Worst-case float32 error of a plain similarity: ~3 roundings per normalised element, a chain of ceil(dim / 64) fmas and 6
    butterfly adds per dot -> (ceil(dim / 64) + 16) * 2^-24."""
    return (-(-int(dim) // 64) + 16) * 2.0 ** -24


def tolerance(dim, branches, doc_offsets, norms):
    """Per-entry bound float64[n]: `tol_plain` on the plain branches; on `mod` the division by na * nb after three such reductions
    gives 4 * tol_plain / min(na, nb)^2, na and nb being this statement's ||X_mod|| of the two rows."""
    off = np.asarray(doc_offsets, dtype=np.int64)
    tol = np.full(int(off[-1]), tol_plain(dim))
    for d, branch in enumerate(branches):
        b, e = int(off[d]), int(off[d + 1])
        if branch == "mod" and e - b >= 2:
            lo = np.minimum(norms[b:e - 1], norms[b + 1:e])
            tol[b:e - 1] = 4.0 * tol_plain(dim) / lo ** 2
    return tol
