"""Measured error of `rl_partition_similarity` against the float64 statement (tests/partition_sim_ref.py) on the batches of
tests/test_gpu_partition_sim.py, next to the derived bound, and the count of one-selected-row documents off the plain values.

    python scripts/partition_sim_error.py [--label TEXT] > profiles/partition_sim_error.txt     (needs the GPU)

The library under measurement is the one the package loads (RAGLITE_HIP_LIB selects another build, e.g. the parent commit's)."""

import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import raglite_amd  # noqa: E402
from tests import partition_sim_ref as ref  # noqa: E402
from tests import test_gpu_partition_sim as t  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this commit")
    args = ap.parse_args()
    raglite_amd.set_device(0)
    print(f"# rl_partition_similarity vs float64 ({args.label}); bound = (ceil(dim / 64) + 16) * 2^-24 plain, 4 * that / min(na, nb)^2 mod")
    print("# batch      dim   rows  max|error| plain   bound plain  ratio   max|error| mod     bound there  ratio")
    for name, make, dims in (("widths", t.widths_batch, t.WIDTHS), ("branches", t.branches_batch, (100, 1024))):
        for dim in dims:
            X, off, sel, want = make(dim)
            sim, tol, branches = t.checked(X, off, sel, want)
            err = np.abs(t.similarity(X, off, sel).astype(np.float64) - sim)
            is_mod = np.repeat(np.asarray(branches) == "mod", np.diff(off))
            cols = []
            for part in (~is_mod, is_mod):
                i = int(np.argmax(np.where(part, err / tol, -1.0)))
                cols.append(f"{err[part].max():18.3e} {tol[i]:13.3e} {err[i] / tol[i]:6.3f}")
            print(f"{name:10s} {dim:5d} {len(X):6d} {cols[0]} {cols[1]}")
    print("# one selected row (sel = [0, 1, 0], 200 documents of three rows per width): documents with an entry further than the plain")
    print("# bound from the float64 plain values, and the largest such distance")
    for dim in (64, 128, 256, 1024):
        X, off, sel = t.one_selected_batch(dim)
        plain = ref.batch(X, off, None)[0]
        got = t.similarity(X, off, sel)
        print(f"one_selected {dim:5d}: {t.documents_off_the_plain_values(got, plain, dim, off):3d} of 200 differ; "
              f"max |error| {np.nanmax(np.abs(got - plain)):.3e} (bound {ref.tol_plain(dim):.3e})")


if __name__ == "__main__":
    main()
