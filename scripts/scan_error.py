"""Measured error of the row scan (scan.hip, scan16.hip) against float64 (tests/scan_ref.py) on the same-sign cases of
tests/test_gpu_scan.py, next to the derived bound.

    python scripts/scan_error.py [--label TEXT] > profiles/scan_error.txt     (needs the GPU)

Per width (both ends of every class), family, metric and storage, over every row of every query of the largest batch the test runs:
  max |score - reference|, the bound at that element, and the largest error / bound over all elements (the figure the tests hold <= 1);
  the same error in units of the fp32 spacing of the reference (how many roundings deep the kernels actually sit);
  the smallest distance, in bounds, from the reference to the reference with one column dropped (tests/test_scan_ref_host.py: > 2).
Everything is measured against the float64 reference, never against the code under test; no number in the tests comes from this file.
The library under measurement is the one the package loads (RAGLITE_HIP_LIB selects another build)."""

import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

import raglite_amd  # noqa: E402
from tests import scan_ref as ref  # noqa: E402
from tests import test_gpu_scan as t  # noqa: E402


def line(dim, storage, aligned, metric, n, B, how):
    E, Q = ref.float_case(dim, storage, n, B)
    k = ref.instantiation(dim, storage, aligned)
    if how == "adapter":
        got = raglite_amd.adapter_apply(E, Q)
    else:
        rows = t.shifted(torch, E) if how == "misaligned" else E
        idx = t.make_index(rows, metric, storage)
        try:
            with idx.options(planes_gemm=0, fused_topk=0):
                got = ref.scatter(*t.search_all(idx, Q, n), n)
        finally:
            idx.close()
    full, bnd = ref.reference(E, Q, metric), ref.bound(E, Q, metric, storage, aligned)
    err = np.abs(got.astype(np.float64) - full)
    i = np.unravel_index(int(np.argmax(err)), err.shape)
    ratio = float(np.max(err / bnd))
    ulps = float(np.max(err / np.abs(np.spacing(full.astype(np.float32)).astype(np.float64))))
    gap = np.inf
    for col in ref.dropped_columns(dim, storage, aligned):
        with np.errstate(invalid="ignore", divide="ignore"):
            lost = [ref.reference(E, Q, metric, drop_dot=col)] + ([ref.reference(E, Q, metric, drop_norm=col)] if metric == "cosine" else [])
            for x in lost:
                d = np.abs(x - full) / bnd
                gap = min(gap, float(np.min(np.where(np.isfinite(d), d, np.inf))))
    print(f"{k['family']:7s} {how:10s} {dim:5d} {k['nv']:3d} {k['terms']:4d} {metric:7s} {n:5d} {B:3d} {err[i]:11.3e} {bnd[i]:11.3e} {ratio:8.4f} {ulps:8.2f} {gap:10.1f}")
    return ratio


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this commit")
    args = ap.parse_args()
    raglite_amd.set_device(0)
    print(f"# row scan vs float64 ({args.label}); bound: tests/scan_ref.py::bound; data: scan_ref.float_case (same-sign)")
    print("# family  rows         dim  NV chain metric      n   B  max|error|  bound there  err/bnd  /spacing  lost col/bnd")
    worst = 0.0
    for dim, storage, aligned, metrics, n, B in ref.float_cases():
        how = "adapter" if metrics == ("raw",) else "misaligned" if (storage == "f32" and not aligned and dim % 4 == 0) else "stored"
        if how == "stored" and storage == "f32" and aligned and t.mfma_route(dim):
            B = 4  # (what the test runs there: from five queries up an MFMA route takes the batch)
        for metric in metrics:
            worst = max(worst, line(dim, storage, aligned, metric, n, B, how))
    print(f"# worst error / bound over all lines: {worst:.4f}")


if __name__ == "__main__":
    main()
