"""Yardstick table for bench.py --dump-outputs directories:  python tools/bench_tools/compare_dumps.py NEW_DIR PARENT_DIR PARENT_DIR [...]
yardstick = largest pairwise |difference| of the parent dumps / largest |entry|; new-vs-parent = largest |new - parent_i| / largest |entry|.
Arrays (gen, G_params, D_params) must stay within 2 x the yardstick; for the 0-d losses the differences are also given in steps of the
last fp32 bit of the value (profiles/thin_output_bwd.txt section 5: one scalar can pass 2 x by chance)."""
import itertools, os, sys
import numpy as np

new_dir, parents = sys.argv[1], sys.argv[2:]
assert len(parents) >= 2, "at least two parent dumps give the yardstick"
names = sorted(f for f in os.listdir(new_dir) if f.endswith(".npy"))
print("%-40s %12s %13s %8s" % ("array", "yardstick", "new-vs-parent", "ratio"))
worst, over = 0.0, []
for f in names:
    new = np.load(os.path.join(new_dir, f)).astype(np.float64)
    ps = [np.load(os.path.join(p, f)).astype(np.float64) for p in parents]
    big = max(float(np.abs(p).max()) for p in ps) or 1.0
    yard = max(float(np.abs(a - b).max()) for a, b in itertools.combinations(ps, 2)) / big
    diff = max(float(np.abs(new - p).max()) for p in ps) / big
    ratio = diff / yard if yard > 0 else (0.0 if diff == 0 else float("inf"))
    line = "%-40s %12.3e %13.3e %8.2f" % (f[:-4], yard, diff, ratio)
    if new.ndim == 0:
        ulp = float(np.spacing(np.float32(abs(ps[0]))))
        line += "   last-bit steps: parents %.1f, new %.1f" % (yard * big / ulp, diff * big / ulp)
    elif ratio > 2.0:
        over.append(f)
    print(line)
    worst = max(worst, ratio)
print("arrays %d, worst ratio %.2f, arrays (not scalars) over 2x: %s" % (len(names), worst, over))
sys.exit(1 if over else 0)
