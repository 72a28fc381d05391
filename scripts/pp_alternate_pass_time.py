"""The 128-query pass launch (rl_time_kernel kind 7) under the tile loop (pp_loop = 0) and the alternating loop (pp_loop = 1) of
maxsim_pp.hip, alternated in ONE process.  With the experiments library (RAGLITE_HIP_LIB = libraglite_hip_exp.so) also the two bare
loops, no block epilogues, wrong results: RAGLITE_PP_DBG = 128 (the slab-counting loop) and 132 (the alternating loop), read at every
launch.  python scripts/pp_alternate_pass_time.py [samples = 7] [launches per sample = 20]"""
import os
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import raglite_amd  # noqa: E402
from bench import DIM, N_ROWS, NQ, QUERIES_PER_STEP, SEED_CORPUS, SEED_QUERY, chunk_offsets  # noqa: E402

samples = int(sys.argv[1]) if len(sys.argv) > 1 else 7
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
exp = "exp" in os.environ.get("RAGLITE_HIP_LIB", "")
raglite_amd.set_device(0)
E = torch.empty((N_ROWS, DIM), dtype=torch.float32, device="cuda")
raglite_amd.synth_fill(E, seed=SEED_CORPUS)
idx = raglite_amd.DeviceIndex(E, chunk_offsets(N_ROWS), metric="dot")
Q = torch.empty((QUERIES_PER_STEP, NQ, DIM), dtype=torch.float32, device="cuda")
raglite_amd.synth_fill(Q, seed=SEED_QUERY)
qv = Q.reshape(QUERIES_PER_STEP * NQ, DIM)
# (name, pp_loop, RAGLITE_PP_DBG)
LOOPS = [("tile loop", 0, "0"), ("alternating loop", 1, "0")]
if exp:
    LOOPS += [("bare slab-counting loop", 0, "128"), ("bare alternating loop", 0, "132")]


def launch(loop, dbg, n):
    os.environ["RAGLITE_PP_DBG"] = dbg
    with idx.options(pp_loop=loop):
        return idx.time_kernel(7, qv, n)


ms = {name: [] for name, _, _ in LOOPS}
for name, loop, dbg in LOOPS:  # warm all
    launch(loop, dbg, 3)
for s in range(samples):
    for name, loop, dbg in LOOPS:
        ms[name].append(launch(loop, dbg, iters) / iters)
    print(f"sample {s + 1}: " + ", ".join(f"{name} {ms[name][-1]:.4f} ms" for name, _, _ in LOOPS), flush=True)
med = {name: statistics.median(v) for name, v in ms.items()}
for name, v in ms.items():
    print(f"{name}: median {med[name]:.4f} ms ({min(v):.4f}-{max(v):.4f}) per launch of {QUERIES_PER_STEP} queries, {samples} samples of {iters} launches")
for base, new in (("tile loop", "alternating loop"), ("bare slab-counting loop", "bare alternating loop")):
    if new in med:
        wins = sum(t < p for p, t in zip(ms[base], ms[new]))
        print(f"{new} against {base}: {100.0 * (med[new] - med[base]) / med[base]:+.2f} %, faster in {wins} of {samples} samples")
