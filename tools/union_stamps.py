#!/usr/bin/env python3
"""Per-slot barrier intervals of k_skm_union from a stamp build (tools/build_diag.sh).

    KHOICE_HIP_LIB=khoice_amd/lib/diag/libkhoice_hip_diag.so KHOICE_STAMP_DUMP=stamps.txt python bench.py --steps 1 --warmup 0 --no-cpu-baseline
    python tools/union_stamps.py stamps.txt [--json out.json]

Thread 0 of a workgroup stores the shader clock per slot: 0 before barrier 1, 1 behind it, 2 at the end of its merge,
10 behind barrier 2, 3 behind the key clear, 4 behind barrier 3, 5 at the end of its insertions, 6 behind barrier 4,
7 at the end of a read-out (a lean slot's runs in the NEXT slot's merge interval: the stamp is the PREVIOUS slot's
then, between stamps 2 and 10; a multi-subset slot's own, behind stamp 6), 8 at the
slot's end; words 12 and 13 are the workgroup + 1 and the slot's place in the workgroup's walk.  The last union block
of the file is read (one per call).  Printed: medians over all slots, and medians over the workgroups of the sums
along a walk, in ticks of the stamp clock; the share of each interval in the walk."""
import argparse
import json
import statistics
import sys
from collections import defaultdict


def last_union_block(path):
    block, cur, keep = [], [], False
    with open(path) as fh:
        for line in fh:
            if line.startswith("#"):
                if keep:
                    block = cur
                cur, keep = [], line.startswith("# skm_union")
            elif keep:
                cur.append([int(x) for x in line.split()])
    return cur if keep else block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dump")
    ap.add_argument("--json")
    a = ap.parse_args()
    rows = last_union_block(a.dump)
    walks = defaultdict(list)
    for r in rows:
        t = r[1:17]
        if t[0] and t[1] and t[12]:
            walks[t[12] - 1].append((t[13], t))
    names = ["B1->B2 (merge%s)", "B2->B3 (key clear)", "B3->B4 (expand + insert)", "B4->next B1 (%sstaging)",
             "B3->next B1 (slot without insertion)", "thread 0: merge", "thread 0: read-out",
             "thread 0: merge and read-out, in a row"]
    per_slot = defaultdict(list)
    per_wg = defaultdict(list)
    nslots, overlap = 0, False
    for wg, w in walks.items():
        w.sort()
        sums = defaultdict(int)
        for i, (_, t) in enumerate(w):
            nslots += 1
            nxt = w[i + 1][1] if i + 1 < len(w) else None
            d = {}
            if t[10]:
                d[0] = t[10] - t[1]
                if t[4]:
                    d[1] = t[4] - t[10]
            if t[4] and t[6]:
                d[2] = t[6] - t[4]
                if nxt:
                    d[3] = nxt[1] - t[6]
            elif t[4] and nxt:
                d[4] = nxt[1] - t[4]
            if t[7] and t[2] and t[10] and t[1] < t[7] < t[10]:
                # the previous slot's read-out inside the merge interval: thread 0 did both jobs one after the other
                # (which one first is the kernel's switch; stamps 2 and 7 both lie behind the second one in order 2)
                overlap = True
                d[7] = max(t[2], t[7]) - t[1]
            else:
                if t[2]:
                    d[5] = t[2] - t[1]
                if t[6] and t[7] and t[7] > t[6]:
                    d[6] = t[7] - t[6]
            for j, v in d.items():
                per_slot[j].append(v)
                sums[j] += v
        if len(w) > 1:
            sums["walk"] = w[-1][1][8] - w[0][1][1] if w[-1][1][8] else 0
            sums["slots"] = len(w)
            for j, v in sums.items():
                per_wg[j].append(v)
    med = lambda v: statistics.median(v) if v else 0
    walk = med(per_wg["walk"])
    out = {"slots": nslots, "workgroups": len(walks), "slots_per_workgroup_median": med(per_wg["slots"]),
           "walk_ticks_median": walk, "overlap": overlap, "intervals": {}}
    print(f"{nslots} slots in {len(walks)} workgroups, {out['slots_per_workgroup_median']} slots per workgroup (median); "
          f"a walk: {walk} ticks (median, first barrier 1 to the last slot's end)")
    print(f"{'interval':44s} {'slots':>7s} {'median':>8s} {'sum per workgroup':>18s} {'share':>6s}")
    for j, n in enumerate(names):
        n = n % ((" + previous read-out" if overlap else "") if j == 0 else ("" if overlap else "read-out + ")) if "%s" in n else n
        s = med(per_wg[j])
        out["intervals"][n] = {"slots": len(per_slot[j]), "median": med(per_slot[j]), "sum_per_workgroup_median": s}
        print(f"{n:44s} {len(per_slot[j]):7d} {med(per_slot[j]):8.0f} {s:18.0f} {100.0 * s / walk if walk else 0:5.1f}%")
    if not overlap:
        a_, b_ = med(per_slot[0]), med(per_slot[3])
        bound = min(a_, b_) * out["slots_per_workgroup_median"]
        out["upper_bound_ticks"] = bound
        print(f"upper bound of an overlap: the shorter of B1->B2 ({a_:.0f}) and B4->next B1 ({b_:.0f}) x slots per workgroup = "
              f"{bound:.0f} ticks, {100.0 * bound / walk if walk else 0:.1f}% of the walk")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
