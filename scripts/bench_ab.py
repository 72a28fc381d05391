"""`bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs` under another build of the library (RAGLITE_HIP_LIB, e.g. the parent commit's)
and under this tree's, alternated in pairs in one call; the dumped outputs are compared bitwise after every pair.  The merge rule the
pass kernel's changes go by: the change wins every pair, and its median gain is at least three times the other build's own spread.

python scripts/bench_ab.py OTHER_LIB [pairs = 6] [scratch dir = a fresh temporary directory]"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
other = str(Path(sys.argv[1]).resolve())
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 6
work = Path(sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="bench_ab_"))
work.mkdir(parents=True, exist_ok=True)


def run(name, lib, i):
    env = dict(os.environ)
    env.pop("RAGLITE_HIP_LIB", None)
    if lib:
        env["RAGLITE_HIP_LIB"] = lib
    out = work / f"{name}_{i}"
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", str(out)],
                         env=env, capture_output=True, text=True, timeout=400, cwd=ROOT)
    if res.returncode != 0:
        sys.exit(f"{name} {i}: bench.py exit {res.returncode}\n{res.stderr[-2000:]}")
    d = json.loads(res.stdout.strip().splitlines()[-1])
    (work / f"{name}_{i}.json").write_text(json.dumps(d))
    print(f"{name} {i} queries/s {d['value']:.1f} ms_per_step {d.get('ms_per_step', float('nan')):.4f}", flush=True)
    return d["value"], out


qps = {"parent": [], "pr": []}
for i in range(1, pairs + 1):
    va, da = run("parent", other, i)
    vb, db = run("pr", None, i)
    qps["parent"].append(va)
    qps["pr"].append(vb)
    names = sorted(p.name for p in da.glob("*.npy"))
    same = bool(names) and all(np.load(da / n).tobytes() == np.load(db / n).tobytes() for n in names)
    print(f"pair {i}: {' and '.join(names)} bitwise equal: {same}", flush=True)
a, b = qps["parent"], qps["pr"]
spread = max(a) - min(a)
gain = statistics.median(b) - statistics.median(a)
print(f"parent: {min(a):.1f}-{max(a):.1f} queries/s, median {statistics.median(a):.1f}, spread (max - min) {spread:.1f} = {100 * spread / statistics.median(a):.2f} %")
print(f"change: {min(b):.1f}-{max(b):.1f} queries/s, median {statistics.median(b):.1f}; wins {sum(y > x for x, y in zip(a, b))} of {pairs} pairs; "
      f"median gain {100 * gain / statistics.median(a):+.2f} % = {gain / spread if spread else float('inf'):.1f} x the parent's spread (rule: every pair and >= 3 x)")
