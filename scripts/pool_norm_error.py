"""Measured error of `rl_pool_norm` against float64 (`oracle.pool_norm_cast`) on the batches of tests/test_gpu_pool_norm.py's register
and DMA tests, next to the derived bound of tests/pool_norm_ref.py.

    python scripts/pool_norm_error.py [--label TEXT] > profiles/pool_norm_error.txt     (needs the GPU)

The kernels' float64 values are seen only through their rounded outputs, so per width and kernel this prints, over all elements:
  max |fp32 output - reference| (float64), the bound at that element and their ratio -- the distance is fp32's own rounding, ~2^-25
      relative, eight orders above the bound: the bound says nothing about it, it says WHERE the rounding may fall the other way;
  the same distance in units of half an fp32 ulp of the reference (<= 1: the output is a nearest fp32 value);
  eligible: elements whose reference lies within the bound of an fp32 / fp16 rounding boundary, where the comparator would accept the
      other neighbour;
  excepted: elements where the output IS that other neighbour (what the tests cap at 1e-6 of a batch).
No number in the tests comes from this file.  The library under measurement is the one the package loads (RAGLITE_HIP_LIB selects
another build, e.g. the parent commit's)."""

import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

import raglite_amd  # noqa: E402
from tests import pool_norm_ref as ref  # noqa: E402
from tests import test_gpu_pool_norm as t  # noqa: E402


def eligible(r64, bnd, dtype):
    """Elements whose reference lies within the bound of the boundary to either neighbour of its rounded value."""
    with np.errstate(all="ignore"):
        w = r64.astype(dtype)
        n = 0
        for to in (np.inf, -np.inf):
            nb = np.nextafter(w, dtype(to)).astype(np.float64)
            n += int(np.sum(np.abs(r64 - 0.5 * (w.astype(np.float64) + nb)) <= bnd))
    return n


def line(name, batch, normalize):
    got32, got16 = t.pool(batch.tokens, batch.begins, batch.ends, normalize, torch=torch)
    r64, _r16, bnd = batch.ref(normalize)
    n32 = ref.assert_rounds_like(got32, r64, bnd, np.float32, name)
    n16 = ref.assert_rounds_like(got16, r64, bnd, np.float16, name)
    with np.errstate(all="ignore"):
        err = np.abs(got32.astype(np.float64) - r64)
        fin = np.isfinite(err) & np.isfinite(bnd) & (bnd > 0)
        i = int(np.argmax(np.where(fin, err, -1.0)))
        half_ulp = 0.5 * np.abs(np.spacing(r64.astype(np.float32)).astype(np.float64))
        in_ulps = float(np.max(np.where(fin, err / half_ulp, 0.0)))
    e, b = float(err.ravel()[i]), float(bnd.ravel()[i])
    print(f"{name:34s} {batch.dim:5d} {batch.n_spans:6d} {int(normalize):4d} {r64.size:9d} {e:11.3e} {b:11.3e} {e / b:10.3e} {in_ulps:9.6f} "
          f"{eligible(r64, bnd, np.float32):6d} {eligible(r64, bnd, np.float16):6d} {n32:6d} {n16:6d}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this commit")
    args = ap.parse_args()
    raglite_amd.set_device(0)
    print(f"# rl_pool_norm vs float64 ({args.label}); bound: tests/pool_norm_ref.py::bound")
    print("# kernel                               dim  spans norm  elements  max|error|   bound there      ratio  /half ulp  elig32 elig16  exc32  exc16")
    for dim in ref.VEC4_DIMS + ref.SCALAR_DIMS:
        for normalize in (True, False):
            line(t.kernel_id(dim).split("-")[0], ref.registers_batch(dim), normalize)
    for dim in ref.DMA_DIMS:
        for n_spans in ref.DMA_SPANS:
            for normalize in (True, False):
                line(t.dma_id(dim).split("-")[0], ref.dma_batch(dim, n_spans), normalize)


if __name__ == "__main__":
    main()
