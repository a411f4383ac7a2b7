#!/usr/bin/env python3
"""Interleaved timing, in ONE process on the same buffers, of

  qfec_locate on a consistent batch, twice (A/A: the spread, and the yardstick)
  qfec_locate2 on the same consistent batch: expected to cost qfec_locate's time plus the added
      launches (the counter's preset, the list, pair and finish kernels), nothing else
  qfec_locate2 with 1 % of the groups holding one corrupted byte (stage 1 settles them)
  qfec_locate2 with 1 % of the groups holding two corrupted shards (the pair search runs on them)
  qfec_locate2 with EVERY group holding two corrupted shards, on a smaller batch: not the design
      point (the pair search is VALU work), reported only

Every round times each side back to back (device events around `reps` calls, warm-up first), and the
order within a round is drawn anew every round, because a side's time depends on what ran before it
(caches, clocks).  Every output is checked against the construction of the damage: culprits, marks
and counts.  Bytes are algorithmic: (k + m) B G.

The added launches' own times come from a kernel trace of this tool in a run of its own:

  rocprofv3 --kernel-trace --stats -d DIR -o locate2 -- python tools/locate2_ab.py --clean-only --rounds 3 --reps 5
  python tools/locate2_ab.py --trace-db DIR/locate2_results.db [--out FILE]

  python tools/locate2_ab.py [--shape 16,4,1400,250000,20000] [--rounds 15] [--reps 10] [--out FILE]
"""
import argparse
import collections
import os
import random
import re
import sqlite3
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12  # MI355X HBM3E, bytes per second
SHAPES = ["16,4,1400,250000,20000", "8,4,1024,100000,20000"]  # k, m, B, G, G of the all-damaged batch


def run(shape, rounds, reps, warmup, clean_only, emit):
    import numpy as np
    import torch

    import quicknet_amd as qa
    from quicknet_amd.synth import marks_to_rs_layout

    k, m, B, G, G_all = (int(x, 0) for x in shape.split(","))
    n = k + m
    dev = torch.device("cuda:0")
    pitch = (B + 15) // 16 * 16
    code = qa.Code.cauchy(k, m)
    data = torch.empty((G, k, pitch), dtype=torch.uint8, device=dev)
    qa.synth_fill(data, 0x5EED0002)
    par = torch.empty((G, m, pitch), dtype=torch.uint8, device=dev)
    code.encode(data, par, B)
    rng = np.random.default_rng(0x5EED0007)
    CLEAN = qa.QFEC_LOC_CLEAN

    def damaged(groups, shards, of=G):
        """One corrupted byte in each of `shards` random shards of every listed group, on copies of
        the first `of` groups -> (data, parity, expected culprit [of, 2])."""
        expect = np.full((of, 2), CLEAN, np.int32)
        ids = np.sort(np.argsort(rng.random((len(groups), n)), axis=1)[:, :shards], axis=1)
        expect[groups, :shards] = ids
        d, p = data[:of].clone(), par[:of].clone()
        for s in range(shards):
            shard = ids[:, s]
            byte = rng.integers(0, B, len(groups))
            val = torch.from_numpy(rng.integers(1, 256, len(groups)).astype(np.uint8)).to(dev)
            isd = shard < k
            off = np.where(isd, (groups * k + shard) * pitch, (groups * m + shard - k) * pitch) + byte
            for buf, sel in ((d, isd), (p, ~isd)):
                at = torch.from_numpy(off[sel]).to(dev)
                buf.view(-1)[at] ^= val[torch.from_numpy(sel).to(dev)]
        return d, p, expect

    some = np.sort(rng.choice(G, G // 100, replace=False))
    batches = {"clean": (data, par, np.full((G, 2), CLEAN, np.int32))}
    if not clean_only:
        batches["1 % one-damaged"] = damaged(some, 1)
        batches["1 % two-damaged"] = damaged(some, 2)
        batches[f"all two-damaged, G={G_all}"] = damaged(np.arange(G_all), 2, of=G_all)
    culprit1 = torch.empty(G, dtype=torch.int32, device=dev)
    culprit = torch.empty((G, 2), dtype=torch.int32, device=dev)
    marks = torch.empty(G * n, dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)

    def locate2(d, p):
        g = d.shape[0]
        return code.locate2(d, p, B, culprit=culprit[:g], marks=marks[: g * n], counts=counts)

    for name, (d, p, expect) in batches.items():
        counts.zero_()
        g = d.shape[0]
        locate2(d, p)
        torch.cuda.synchronize()
        assert np.array_equal(culprit[:g].cpu().numpy(), expect), f"locate2, {name}: wrong culprits"
        gm = np.zeros((g, n), np.uint8)
        for slot in range(2):
            hit = expect[:, slot] >= 0
            gm[np.nonzero(hit)[0], expect[hit, slot]] = 1
        assert np.array_equal(marks[: g * n].cpu().numpy(), marks_to_rs_layout(gm, k)), f"locate2, {name}: wrong marks"
        one, two = int(((expect[:, 0] >= 0) & (expect[:, 1] < 0)).sum()), int((expect[:, 1] >= 0).sum())
        assert list(counts.cpu().numpy()) == [one, two, 0, 0], f"locate2, {name}: wrong counts"
    code.locate(data, par, B, culprit=culprit1)
    torch.cuda.synchronize()
    assert bool((culprit1 == CLEAN).all()), "locate flags an encoded batch"

    sides = [("locate (A)", G, lambda: code.locate(data, par, B, culprit=culprit1)),
             ("locate (B)", G, lambda: code.locate(data, par, B, culprit=culprit1))]
    for name, (d, p, _) in batches.items():
        sides.append((f"locate2, {name}", d.shape[0], lambda d=d, p=p: locate2(d, p)))
    s = torch.cuda.current_stream()
    for _, _, fn in sides:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in sides}
    order = random.Random(0x5EED0008)
    for _ in range(rounds):
        for name, _, fn in order.sample(sides, len(sides)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(reps):
                fn()
            e1.record(s)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps)
    emit(f"RS({k},{m}) B={B} G={G}: {rounds} interleaved rounds x {reps} calls, device events")
    med = {}
    for name, g, _ in sides:
        med[name] = statistics.median(times[name])
        nbytes = n * B * g
        rate = nbytes / (med[name] * 1e-3)
        emit(f"  {name:34s} median {med[name] * 1e3:8.1f} us  min {min(times[name]) * 1e3:8.1f} us  "
             f"max {max(times[name]) * 1e3:8.1f} us  {nbytes / 1e6:9.1f} MB  {rate / 1e9:7.1f} GB/s = {rate / PEAK:5.3f} of 8 TB/s")
    aa = abs(med["locate (A)"] - med["locate (B)"])
    base = min(med["locate (A)"], med["locate (B)"]), max(med["locate (A)"], med["locate (B)"])
    c = med["locate2, clean"]
    emit(f"  locate A/A: medians differ by {aa * 1e3:.1f} us ({aa / med['locate (A)'] * 100:.2f} %); "
         f"locate2, clean - locate: {(c - base[1]) * 1e3:+.1f} .. {(c - base[0]) * 1e3:+.1f} us "
         f"({(c / base[1] - 1) * 100:+.2f} .. {(c / base[0] - 1) * 100:+.2f} %), the four added launches included")


def trace(db, emit):
    """Per-kernel launch times of a --clean-only run: what the trace attributes to the launches
    qfec_locate2 adds to qfec_locate on a consistent batch."""
    rows = sqlite3.connect(db).execute("select name, duration from kernels order by start").fetchall()
    by = collections.defaultdict(list)
    for name, dur in rows:
        short = re.sub(r"\(.*", "", re.sub(r"^void |qfec::", "", name))
        if "locate" in short or "fillBuffer" in short:
            by[short].append(dur / 1e3)
    emit("launch times in us from the kernel trace: median (min) over n launches")
    for name in sorted(by):
        emit(f"  {name:44s} n={len(by[name]):5d}  {statistics.median(by[name]):8.1f} ({min(by[name]):8.1f})")
    both = statistics.median(by["k_locate2_list"]) + statistics.median(by["k_locate2_finish"])
    fills = [t for name in by if "fillBuffer" in name for t in by[name]]
    for name in sorted(k for k in by if "k_locate2_pairs" in k):
        emit(f"  list + {name} + finish on a consistent batch, medians summed: {both + statistics.median(by[name]):.1f} us "
             f"(the preset of the list's counter, 16 bytes, is one of the fillBuffer launches: {min(fills):.1f} us at the least)")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append", help="k,m,B,G,G_all (repeatable); default: " + " and ".join(SHAPES))
    p.add_argument("--rounds", type=int, default=15)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--clean-only", action="store_true", help="only the sides on the consistent batch (for a kernel trace)")
    p.add_argument("--trace-db", default="", help="summarise a rocprofv3 kernel trace of a --clean-only run instead")
    p.add_argument("--out", default="", help="also write the report to this file")
    a = p.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    if a.trace_db:
        trace(a.trace_db, emit)
    else:
        import torch

        import quicknet_amd as qa

        emit(f"{qa.lib().qfec_version().decode()} on {torch.cuda.get_device_name(0)}")
        for shape in a.shape or SHAPES:
            run(shape, a.rounds, a.reps, a.warmup, a.clean_only, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
