"""Condense a rocprofv3 kernel trace of float-net forwards into one line per launch of a pass.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o k -- python <a script that calls FloatDnn.calculateDevice a few times>
    python tools/kernel_trace_digest.py DIR

The dispatches are walked in start order; an input_step launch begins a chunk's pass, and every dispatch is filed under
(position in the pass, kernel, grid size x).  Printed per group: launches counted, mean / min / max of the kernel time in
microseconds over the LATER HALF of the group's dispatches (the first half is warm-up).  profiles/float_kernel_trace.txt
was made with it."""
import collections
import csv
import glob
import sys


def main():
    files = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        sys.exit("kernel_trace_digest: no *kernel_trace.csv under " + sys.argv[1])
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    groups = collections.defaultdict(list)
    idx, passes = 0, 0
    for r in rows:
        name = r["Kernel_Name"].replace("fdnn::(anonymous namespace)::", "").replace("fdnn::fl::(anonymous namespace)::", "")[:48]
        if "input_step" in name:
            idx = 0
            passes += 1
        groups[(idx, name, r["Grid_Size_X"])].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        idx += 1
    print("chunks seen:", passes)
    for k in sorted(groups):
        v = groups[k][len(groups[k]) // 2:]
        print(k, "n=%d" % len(v), "mean %.1f us  min %.1f  max %.1f" % (sum(v) / len(v), min(v), max(v)))
    first = min(int(r["Start_Timestamp"]) for r in rows[len(rows) // 2:])
    last = max(int(r["End_Timestamp"]) for r in rows)
    print("wall of the later half of the dispatches: %.1f us" % ((last - first) / 1e3))


if __name__ == "__main__":
    main()
