#!/usr/bin/env python3
"""Timeline of one evaluation's integral stage from a rocprofv3 kernel trace (scripts/eri_timeline.sh):
per hardware queue, the kernels in start order with start / end relative to the evaluation's first dispatch.

    python scripts/eri_timeline.py <tag>/kernel_trace.csv [evaluation index, default last] [--min-us N]

Dispatches shorter than N microseconds are left out (default 150).  The grid is printed as x*y: a task launch of
shared entries is the one whose grid is far smaller than (entries x fragments), a dense launch has y = 1."""
import csv
import re
import sys


def short(n):
    n = re.sub(r"\(.*", "", n).replace("void mqc::", "").replace("(anonymous namespace)::", "").replace("mqc::", "")
    return n[:44]


def main():
    args = sys.argv[1:]
    min_ns = 150_000
    if "--min-us" in args:
        k = args.index("--min-us")
        min_ns = int(float(args[k + 1]) * 1000)
        del args[k:k + 2]
    rows = list(csv.DictReader(open(args[0])))
    ev = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), int(r["Queue_Id"]), int(r["Grid_Size_X"]),
           int(r["VGPR_Count"]) + int(r["Accum_VGPR_Count"]), int(r.get("Grid_Size_Y") or 1), r.get("Stream_Id", "")) for r in rows]
    ev.sort()
    # evaluations are separated by idle gaps; cut at the big jk launches' first occurrence after a gap > 2 ms
    cuts = [0]
    last_end = ev[0][1]
    for i, e in enumerate(ev):
        if e[0] - last_end > 1_500_000:
            cuts.append(i)
        last_end = max(last_end, e[1])
    cuts.append(len(ev))
    which = int(args[1]) if len(args) > 1 else len(cuts) - 2
    seg = ev[cuts[which]:cuts[which + 1]]
    t0 = seg[0][0]
    print("evaluation %d of %d: %d dispatches, %.2f ms" % (which, len(cuts) - 1, len(seg), (max(e[1] for e in seg) - t0) / 1e6))
    for e in seg:
        if e[1] - e[0] < min_ns:
            continue
        grid = "%d" % e[4] if e[6] == 1 else "%d*%d" % (e[4], e[6])
        print("q%-3d s%-3s %8.2f -> %8.2f  (%6.2f ms)  grid %13s  regs %3d  %s" % (e[3], e[7], (e[0] - t0) / 1e6, (e[1] - t0) / 1e6, (e[1] - e[0]) / 1e6, grid, e[5], e[2]))


if __name__ == "__main__":
    main()
