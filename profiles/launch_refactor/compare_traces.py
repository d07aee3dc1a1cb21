"""Compare two rocprofv3 runs of trace_frames.py (csv output directories): the sequence of HIP API function names, and
the sequence of kernel names per stream (streams numbered by first appearance; the queue id where the trace carries no
stream id). Prints what it compared and exits 1 on a difference.

  python3 profiles/launch_refactor/compare_traces.py <dir of run A> <dir of run B>
"""
import csv
import glob
import os
import sys


def rows(d, suffix):
    files = sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True))
    if not files:
        sys.exit(f"no *{suffix} under {d}")
    out = []
    for f in files:
        with open(f, newline="") as fh:
            out += list(csv.DictReader(fh))
    return out


def api_names(d):
    r = rows(d, "hip_api_trace.csv")
    r.sort(key=lambda x: (int(x["Start_Timestamp"]), int(x.get("Correlation_Id") or 0)))
    return [x["Function"] for x in r]


def kernels(d):
    r = rows(d, "kernel_trace.csv")
    key = "Stream_Id" if "Stream_Id" in r[0] else "Queue_Id"
    r.sort(key=lambda x: int(x.get("Dispatch_Id") or x["Start_Timestamp"]))
    streams, per = {}, {}
    for x in r:
        sid = streams.setdefault(x[key], len(streams))
        per.setdefault(sid, []).append(x["Kernel_Name"])
    return key, per


def main(a, b):
    na, nb = api_names(a), api_names(b)
    ka, pa = kernels(a)
    kb, pb = kernels(b)
    same_api, same_k = na == nb, (ka, pa) == (kb, pb)
    print(f"HIP API calls: {len(na)} vs {len(nb)}, sequences {'equal' if same_api else 'DIFFER'}")
    if not same_api:
        i = next((i for i, (x, y) in enumerate(zip(na, nb)) if x != y), min(len(na), len(nb)))
        print(f"  first difference at call {i}: {na[i - 2:i + 3]} vs {nb[i - 2:i + 3]}")
    print(f"kernels by {ka}: {sum(map(len, pa.values()))} on {len(pa)} streams vs {sum(map(len, pb.values()))} on "
          f"{len(pb)}, per-stream sequences {'equal' if same_k else 'DIFFER'}")
    for sid in sorted(set(pa) | set(pb)):
        x, y = pa.get(sid, []), pb.get(sid, [])
        print(f"  stream {sid}: {len(x)} vs {len(y)} kernels{'' if x == y else '  <-- differ'}")
    return 0 if same_api and same_k else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
