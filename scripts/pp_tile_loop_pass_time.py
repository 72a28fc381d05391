"""The 128-query pass launch (rl_time_kernel kind 7) under the slab-counting loop and the tile loop of maxsim_pp.hip, alternated in ONE
process of the experiments library (RAGLITE_HIP_LIB = libraglite_hip_exp.so; RAGLITE_PP_DBG = 1 selects the slab-counting loop, read at
every launch).  python scripts/pp_tile_loop_pass_time.py [samples = 7] [launches per sample = 20]"""
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
if "exp" not in os.environ.get("RAGLITE_HIP_LIB", ""):
    sys.exit("needs the experiments library: RAGLITE_HIP_LIB=raglite_amd/_lib/libraglite_hip_exp.so")
raglite_amd.set_device(0)
E = torch.empty((N_ROWS, DIM), dtype=torch.float32, device="cuda")
raglite_amd.synth_fill(E, seed=SEED_CORPUS)
idx = raglite_amd.DeviceIndex(E, chunk_offsets(N_ROWS), metric="dot")
Q = torch.empty((QUERIES_PER_STEP, NQ, DIM), dtype=torch.float32, device="cuda")
raglite_amd.synth_fill(Q, seed=SEED_QUERY)
qv = Q.reshape(QUERIES_PER_STEP * NQ, DIM)
LOOPS = (("slab-counting loop (parent)", "1"), ("tile loop", "0"))
ms = {name: [] for name, _ in LOOPS}
for name, dbg in LOOPS:  # warm both
    os.environ["RAGLITE_PP_DBG"] = dbg
    idx.time_kernel(7, qv, 3)
for s in range(samples):
    for name, dbg in LOOPS:
        os.environ["RAGLITE_PP_DBG"] = dbg
        ms[name].append(idx.time_kernel(7, qv, iters) / iters)
    print(f"sample {s + 1}: " + ", ".join(f"{name} {ms[name][-1]:.4f} ms" for name, _ in LOOPS), flush=True)
med = {name: statistics.median(v) for name, v in ms.items()}
for name, v in ms.items():
    print(f"{name}: median {med[name]:.4f} ms ({min(v):.4f}-{max(v):.4f}) per launch of {QUERIES_PER_STEP} queries, {samples} samples of {iters} launches")
a, b = (med[name] for name, _ in LOOPS)
wins = sum(t < p for p, t in zip(*(ms[name] for name, _ in LOOPS)))
print(f"tile loop against slab-counting loop: {100.0 * (b - a) / a:+.2f} %, faster in {wins} of {samples} samples")
