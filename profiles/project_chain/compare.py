"""bits.py's two runs side by side: python3 profiles/project_chain/compare.py A.jsonl B.jsonl [A.npz B.npz]

Every hash of A must be B's. The splat rows (sums of float atomics) are compared as numbers: the largest difference between
the libraries' takes over the largest entry, beside the same figure for two takes of one library."""
import json
import sys

import numpy as np


def hashes(path):
    return {r["output"]: r["sha256"] for r in map(json.loads, open(path)) if "output" in r}


a, b = hashes(sys.argv[1]), hashes(sys.argv[2])
bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
print(json.dumps({"outputs": len(a), "equal": len(a) - len(bad), "different": bad}))
if len(sys.argv) > 4:
    ra, rb = np.load(sys.argv[3]), np.load(sys.argv[4])
    for path in ra.files:
        x, y = ra[path].astype(np.float64), rb[path].astype(np.float64)
        top = np.abs(x).max()
        within = max(np.abs(x[1:] - x[0]).max(), np.abs(y[1:] - y[0]).max()) / top
        between = np.abs(x[:, None] - y[None]).max() / top
        print(json.dumps({"splat rows": path, "entries": int(x[0].size), "nonzero": int(np.count_nonzero(x[0])),
                          "largest difference between two takes of one library / largest entry": within,
                          "largest difference between the libraries / largest entry": between}))
sys.exit(1 if bad else 0)
