#!/usr/bin/env python3
"""Per-launch times of qfec_locate and qfec_verify from a kernel trace of tools/locate_ab.py:

  rocprofv3 --kernel-trace --stats -d DIR -o locate -- python tools/locate_ab.py --rounds 3 --reps 5
  python tools/locate_trace.py DIR/locate_results.db [--out FILE]

A qfec_locate is four launches (preset of the bad-rows words, preset of the candidate words, the
main kernel, the finish kernel), a qfec_verify two (preset, main kernel).  The trace does not say
which batch a call worked on; the tool's first three locate calls per shape are its checks of the
consistent, the 1 % and the all-damaged batch, in that order, and the finish kernel's time differs
between the three (one counter add per block that holds a damaged group), so every later call goes
to the check whose finish time is nearest.  `span` is first launch start to last launch end.
"""
import argparse
import collections
import os
import re
import sqlite3
import statistics

KINDS = ["clean", "1 % damaged", "all damaged"]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("db")
    p.add_argument("--out", default="")
    a = p.parse_args()
    rows = sqlite3.connect(a.db).execute("select name, start, end, duration from kernels order by start").fetchall()
    locate, verify = collections.defaultdict(list), collections.defaultdict(list)
    for i, (name, start, end, dur) in enumerate(rows):
        shape = re.search(r"k_(?:locate|verify)_perm<(\d+), (\d+)>", name)
        if not shape:
            continue
        key = f"RS({shape.group(1)},{shape.group(2)})"
        if "k_locate_perm" in name:
            f0, f1, fin = rows[i - 2], rows[i - 1], rows[i + 1]
            assert "fillBuffer" in f0[0] and "fillBuffer" in f1[0] and "k_locate_finish" in fin[0], (f0[0], f1[0], fin[0])
            locate[key].append((f0[3] + f1[3], dur, fin[3], fin[2] - f0[1]))
        else:
            f0 = rows[i - 1]
            assert "fillBuffer" in f0[0], f0[0]
            verify[key].append((f0[3], dur, end - f0[1]))
    lines = []
    med = lambda xs: statistics.median(xs) / 1e3  # noqa: E731
    for key in locate:
        v = verify[key]
        lines.append(f"{key}: launch times in us, median (min) over the calls in the trace")
        lines.append(f"  {'verify':20s} n={len(v):3d}  preset {med([c[0] for c in v]):5.1f}  main {med([c[1] for c in v]):7.1f} "
                     f"({min(c[1] for c in v) / 1e3:7.1f})  span {med([c[2] for c in v]):7.1f}")
        centres = [c[2] for c in locate[key][:3]]
        for kind, centre in zip(KINDS, centres):
            calls = [c for c in locate[key] if min(centres, key=lambda x: abs(x - c[2])) == centre]
            lines.append(f"  {'locate, ' + kind:20s} n={len(calls):3d}  presets {med([c[0] for c in calls]):5.1f}  "
                         f"main {med([c[1] for c in calls]):7.1f} ({min(c[1] for c in calls) / 1e3:7.1f})  "
                         f"finish {med([c[2] for c in calls]):5.1f}  span {med([c[3] for c in calls]):7.1f}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
