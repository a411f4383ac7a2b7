#!/usr/bin/env python3
"""Interleaved timing, in ONE process on the same buffers, of

  qfec_locate_erased with no marks, consistent   against  qfec_locate (the call for complete groups;
                                                          same rows read) and qfec_locate against
                                                          itself (A/A: the spread)
  qfec_locate_erased with one random lost shard  against  qfec_repair with the same marks (locate reads
  per group, consistent                                   n - 1 rows; repair reads k and writes one) and
                                                          qfec_repair against itself (A/A)
  the same with 1 % of the groups, and with every group, holding one corrupted byte in a surviving
  shard (the cold branch, and its worst case): reported only

Every round times each side back to back (device events around `reps` calls, warm-up first); the
order within a round is drawn anew every round, because a side's time depends on what ran before it
(caches, clocks).  Every output is checked against the construction before and after the timing:
culprits, marks_out, counts, and the repaired rows against the originals.  Bytes are algorithmic:
(k + m - t) B G for locate_erased, (k + m) B G for locate, (k + 1) B G for repair.  No profiler.

  python tools/locate_erased_ab.py [--shape 10,3,1024,100000] [--rounds 15] [--reps 10] [--out FILE]
"""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import quicknet_amd as qa  # noqa: E402
from quicknet_amd.synth import marks_to_rs_layout  # noqa: E402

PEAK = 8.0e12  # MI355X HBM3E, bytes per second
SHAPES = ["10,3,1024,100000", "16,4,1400,250000"]


def run(shape, rounds, reps, warmup, emit):
    k, m, B, G = (int(x, 0) for x in shape.split(","))
    n = k + m
    dev = torch.device("cuda:0")
    pitch = (B + 15) // 16 * 16
    code = qa.Code.cauchy(k, m)
    data = torch.empty((G, k, pitch), dtype=torch.uint8, device=dev)
    qa.synth_fill(data, 0x5EED0002)
    par = torch.empty((G, m, pitch), dtype=torch.uint8, device=dev)
    code.encode(data, par, B)
    code.prepare_repair()
    code.prepare_locate_erased()
    rng = np.random.default_rng(0x5EED0007)
    to = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=t)  # noqa: E731

    # one random lost shard per group, its row filled with junk (never read by locate_erased)
    lost = rng.integers(0, n, G)
    gm = (np.arange(n)[None, :] == lost[:, None]).astype(np.uint8)
    no_marks = torch.zeros(G * n, dtype=torch.uint8, device=dev)
    marks = to(marks_to_rs_layout(gm, k), torch.uint8)

    def with_lost_rows_junked():
        d, p = data.clone(), par.clone()
        isd = to(lost < k, torch.bool)
        g = torch.arange(G, device=dev)
        li = to(lost, torch.int64)
        d[g[isd], li[isd]] = 0xC3
        p[g[~isd], li[~isd] - k] = 0x3C
        return d, p

    def corrupted(groups):
        """One byte XORed into one random surviving shard of each listed group."""
        d, p = with_lost_rows_junked()
        expect = np.full(G, qa.QFEC_LOC_CLEAN, np.int32)
        shard = (lost[groups] + rng.integers(1, n, len(groups))) % n  # any shard but the lost one
        byte = rng.integers(0, B, len(groups))
        val = rng.integers(1, 256, len(groups)).astype(np.uint8)
        expect[groups] = shard
        isd = shard < k
        d_off = to((groups[isd] * k + shard[isd]) * pitch + byte[isd], torch.int64)
        p_off = to((groups[~isd] * m + shard[~isd] - k) * pitch + byte[~isd], torch.int64)
        d.view(-1)[d_off] ^= to(val[isd], torch.uint8)
        p.view(-1)[p_off] ^= to(val[~isd], torch.uint8)
        return d, p, expect

    dl, pl = with_lost_rows_junked()
    d1, p1, exp1 = corrupted(np.sort(rng.choice(G, G // 100, replace=False)))
    dall, pall, expall = corrupted(np.arange(G))
    clean = np.full(G, qa.QFEC_LOC_CLEAN, np.int32)
    culprit = torch.empty(G, dtype=torch.int32, device=dev)
    culprit_b = torch.empty(G, dtype=torch.int32, device=dev)
    marks_out = torch.empty(G * n, dtype=torch.uint8, device=dev)
    marks_b = torch.empty(G * n, dtype=torch.uint8, device=dev)
    counts = torch.zeros(5, dtype=torch.int32, device=dev)
    counts3 = torch.zeros(3, dtype=torch.int32, device=dev)

    def check(d, p, mk, gmarks, expect):
        counts.zero_()
        code.locate_erased(d, p, mk, B, culprit=culprit, marks_out=marks_out, counts=counts)
        torch.cuda.synchronize()
        assert np.array_equal(culprit.cpu().numpy(), expect), "locate_erased: wrong culprits"
        want = gmarks.copy()
        want[np.nonzero(expect >= 0)[0], expect[expect >= 0]] = 1
        assert np.array_equal(marks_out.cpu().numpy(), marks_to_rs_layout(want, k)), "locate_erased: wrong marks_out"
        assert list(counts.cpu().numpy()) == [int((expect >= 0).sum()), 0, 0, 0, 0], "locate_erased: wrong counts"

    def check_all():
        check(data, par, no_marks, np.zeros((G, n), np.uint8), clean)
        check(dl, pl, marks, gm, clean)
        check(d1, p1, marks, gm, exp1)
        check(dall, pall, marks, gm, expall)
        code.locate(data, par, B, culprit=culprit_b, marks=marks_b, counts=counts3)
        torch.cuda.synchronize()
        assert bool((culprit_b == qa.QFEC_LOC_CLEAN).all()) and not bool(marks_b.any()), "locate flags an encoded batch"

    check_all()
    full, less, rep = n * B * G, (n - 1) * B * G, (k + 1) * B * G
    le = lambda d, p, mk: code.locate_erased(d, p, mk, B, culprit=culprit, marks_out=marks_out, counts=counts)  # noqa: E731
    sides = [("locate (A)", full, lambda: code.locate(data, par, B, culprit=culprit_b, marks=marks_b, counts=counts3)),
             ("locate (B)", full, lambda: code.locate(data, par, B, culprit=culprit, marks=marks_out, counts=counts3)),
             ("locate_erased, no marks", full, lambda: le(data, par, no_marks)),
             ("repair, 1 lost (A)", rep, lambda: code.repair(dl, pl, marks, B)),
             ("repair, 1 lost (B)", rep, lambda: code.repair(dl, pl, marks, B)),
             ("locate_erased, 1 lost", less, lambda: le(dl, pl, marks)),
             ("locate_erased, 1 lost, 1 % corrupted", less, lambda: le(d1, p1, marks)),
             ("locate_erased, 1 lost, all corrupted", less, lambda: le(dall, pall, marks))]
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
    check_all()
    assert torch.equal(dl[..., :B], data[..., :B]) and torch.equal(pl[..., :B], par[..., :B]), "repair: wrong rows"
    emit(f"RS({k},{m}) B={B} G={G}: {rounds} interleaved rounds x {reps} calls, device events")
    med = {}
    for name, nbytes, _ in sides:
        med[name] = statistics.median(times[name])
        rate = nbytes / (med[name] * 1e-3)
        emit(f"  {name:38s} median {med[name] * 1e3:8.1f} us  min {min(times[name]) * 1e3:8.1f} us  "
             f"max {max(times[name]) * 1e3:8.1f} us  {nbytes / 1e6:9.1f} MB  {rate / 1e9:7.1f} GB/s = {rate / PEAK:5.3f} of 8 TB/s")
    for a, b, x in (("locate (A)", "locate (B)", "locate_erased, no marks"),
                    ("repair, 1 lost (A)", "repair, 1 lost (B)", "locate_erased, 1 lost")):
        aa = abs(med[a] - med[b])
        emit(f"  {a[:-4]} A/A: medians differ by {aa * 1e3:.1f} us ({aa / med[a] * 100:.2f} %); "
             f"{x} - {a}: {(med[x] - med[a]) * 1e3:+.1f} us ({(med[x] / med[a] - 1) * 100:+.2f} %)")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append", help="k,m,B,G (repeatable); default: " + " and ".join(SHAPES))
    p.add_argument("--rounds", type=int, default=15)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default="", help="also write the report to this file")
    a = p.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit(f"{qa.lib().qfec_version().decode()} on {torch.cuda.get_device_name(0)}")
    for shape in a.shape or SHAPES:
        run(shape, a.rounds, a.reps, a.warmup, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
