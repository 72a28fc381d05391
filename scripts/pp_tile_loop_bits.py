"""Are the approximate pass's scores (rl_maxsim_approx_scores, the sixteen-query kernel) byte-identical under two builds of the library?

python scripts/pp_tile_loop_bits.py LIB_A LIB_B     two child processes, one per library (RAGLITE_HIP_LIB), SHA-256 of every score array
python scripts/pp_tile_loop_bits.py --child         what a child runs: one JSON line {shape: digest}

Float data on the shapes of tests/test_gpu_pp_tile_loop.py (widths 256 / 320 / 288 / 1024; workgroups of one tile and of up to eight;
ragged, uniform and 300-row chunks; 1, 16 and 17 queries; an index that ends inside a 16-row block) and the bench's own (1 M x 1024,
128 queries of 32 vectors, bench.chunk_offsets)."""
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

RANGE_ROWS = {256: 1024, 320: 832, 288: 912, 1024: 256}  # tests/test_gpu_pp_tile_loop.py: the smallest index the pass runs over, per width
LAYOUTS = (("ragged", 17, 32), ("uniform8", 16, 9), ("rows300", 1, 1), ("one_tile", 16, 9))
SHAPES = [(256 * r, d, lay, nqs, nq) for d, r in RANGE_ROWS.items() for lay, nqs, nq in LAYOUTS]
SHAPES += [(256 * RANGE_ROWS[d] + 13, d, lay, 16, 9) for d in (256, 1024) for lay in ("ones", "ragged")]


def child():
    import numpy as np
    import torch

    import raglite_amd
    from bench import DIM, N_ROWS, NQ, QUERIES_PER_STEP, SEED_CORPUS, SEED_QUERY, chunk_offsets
    from tests.test_gpu_pp_tile_loop import _offsets

    raglite_amd.set_device(0)
    out = {}
    for n, dim, layout, n_queries, nq in SHAPES + [(N_ROWS, DIM, "bench", QUERIES_PER_STEP, NQ)]:
        off = chunk_offsets(n) if layout == "bench" else _offsets(layout, n, dim)
        E = torch.empty((n, dim), dtype=torch.float32, device="cuda")
        raglite_amd.synth_fill(E, seed=SEED_CORPUS if layout == "bench" else 40_000 + dim, kind="uniform")
        Q = torch.empty((n_queries, nq, dim), dtype=torch.float32, device="cuda")
        raglite_amd.synth_fill(Q, seed=SEED_QUERY if layout == "bench" else 40_001 + dim, kind="uniform")
        idx = raglite_amd.DeviceIndex(E, off, metric="dot")
        a, m = idx.maxsim_approx_scores(Q, kernel=0)
        a = a.cpu().numpy()
        assert np.isfinite(a).all()
        out[f"{n}x{dim} {layout} {n_queries}x{nq}"] = hashlib.sha256(a.tobytes() + m.cpu().numpy().tobytes()).hexdigest()
        idx.close()
        del E, Q
    print(json.dumps(out))


def main():
    digests = []
    for lib in sys.argv[1:3]:
        env = dict(os.environ, RAGLITE_HIP_LIB=str(Path(lib).resolve()))
        res = subprocess.run([sys.executable, __file__, "--child"], env=env, capture_output=True, text=True, timeout=600)
        if res.returncode != 0:
            sys.exit(f"{lib}: exit {res.returncode}\n{res.stderr[-2000:]}")
        digests.append(json.loads(res.stdout.strip().splitlines()[-1]))
    a, b = digests
    print(f"approximate scores (rl_maxsim_approx_scores, kernel 0), float data, SHA-256 of scores + bounds; A = {sys.argv[1]}, B = {sys.argv[2]}")
    same = 0
    for name in a:
        eq = a[name] == b[name]
        same += eq
        print(f"{name:34s} A {a[name][:16]}  B {b[name][:16]}  {'identical' if eq else 'DIFFERENT'}")
    print(f"{same} of {len(a)} shapes byte-identical")
    sys.exit(0 if same == len(a) else 1)


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
