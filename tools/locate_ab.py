#!/usr/bin/env python3
"""Interleaved timing, in ONE process on the same buffers, of

  qfec_locate on a consistent batch   against  qfec_verify (the yardstick; same rows read) and
                                               qfec_verify against itself (A/A: the spread)
  qfec_locate with 1 % of the groups and with every group holding one corrupted byte (the cold
  branch, and its worst case): reported only
  qfec_scrub at 1 % damage            against  qfec_verify + read-back of bad_rows + upload of marks
                                               + qfec_repair.  The two-call side is handed the marks
                                               from the construction of the damage: without
                                               qfec_locate nothing on the device could name them, so
                                               it is a lower bound for any host-driven way.

Every round times each side back to back (device events around `reps` calls, warm-up first), so
drift between runs does not pass for a kernel difference; the order within a round is drawn anew
every round, because a side's time depends on what ran before it (caches, clocks).  The scrub
comparison is timed with the host clock around one call that ends in a synchronise (the read-back is part of it), the damage put
back before each call outside the timed span.  Every output is checked: culprits, marks and counts
against the construction, scrubbed buffers against the originals.  Bytes are algorithmic:
(k + m) B G for verify and locate.

The two presets and the finish kernel of qfec_locate are separate launches; their own times come
from a kernel trace of this tool (rocprofv3 --kernel-trace --stats -- python tools/locate_ab.py
--rounds 3), in a run of its own.

  python tools/locate_ab.py [--shape 10,3,1024,100000] [--rounds 15] [--reps 10] [--out FILE]
"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import quicknet_amd as qa  # noqa: E402
from quicknet_amd.synth import marks_to_rs_layout  # noqa: E402

PEAK = 8.0e12  # MI355X HBM3E, bytes per second
SHAPES = ["10,3,1024,100000", "16,4,1400,250000"]


def one_byte_damage(rng, G, k, m, B, pitch, groups):
    """One corrupted byte in one random shard of each listed group -> (flat byte offsets into data,
    xor values, the same for parity, expected culprit [G])."""
    n = k + m
    expect = np.full(G, qa.QFEC_LOC_CLEAN, np.int32)
    shard = rng.integers(0, n, len(groups))
    byte = rng.integers(0, B, len(groups))
    val = rng.integers(1, 256, len(groups)).astype(np.uint8)
    expect[groups] = shard
    isd = shard < k
    d_off = (groups[isd] * k + shard[isd]) * pitch + byte[isd]
    p_off = (groups[~isd] * m + shard[~isd] - k) * pitch + byte[~isd]
    return d_off, val[isd], p_off, val[~isd], expect


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
    rng = np.random.default_rng(0x5EED0005)

    def damaged(groups):
        d_off, d_val, p_off, p_val, expect = one_byte_damage(rng, G, k, m, B, pitch, groups)
        to = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=t)  # noqa: E731
        fix = (to(d_off, torch.int64), to(d_val, torch.uint8), to(p_off, torch.int64), to(p_val, torch.uint8))
        d, p = data.clone(), par.clone()

        def hurt():  # xor the bytes in (on buffers that hold the original bytes there)
            d.view(-1)[fix[0]] = data.view(-1)[fix[0]] ^ fix[1]
            p.view(-1)[fix[2]] = par.view(-1)[fix[2]] ^ fix[3]

        hurt()
        return d, p, expect, hurt

    some = np.sort(rng.choice(G, G // 100, replace=False))
    d1, p1, exp1, hurt1 = damaged(some)
    dall, pall, expall, _ = damaged(np.arange(G))
    bad_a = torch.empty(G, dtype=torch.int32, device=dev)
    bad_b = torch.empty(G, dtype=torch.int32, device=dev)
    culprit = torch.empty(G, dtype=torch.int32, device=dev)
    marks = torch.empty(G * n, dtype=torch.uint8, device=dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)

    def check_locate(d, p, expect):
        counts.zero_()
        code.locate(d, p, B, culprit=culprit, marks=marks, counts=counts)
        torch.cuda.synchronize()
        assert np.array_equal(culprit.cpu().numpy(), expect), "locate: wrong culprits"
        gm = np.zeros((G, n), np.uint8)
        gm[np.nonzero(expect >= 0)[0], expect[expect >= 0]] = 1
        assert np.array_equal(marks.cpu().numpy(), marks_to_rs_layout(gm, k)), "locate: wrong marks"
        assert list(counts.cpu().numpy()) == [int((expect >= 0).sum()), 0, 0], "locate: wrong counts"

    check_locate(data, par, np.full(G, qa.QFEC_LOC_CLEAN, np.int32))
    check_locate(d1, p1, exp1)
    check_locate(dall, pall, expall)
    code.verify(data, par, B, bad_rows=bad_a)
    torch.cuda.synchronize()
    assert not bool(bad_a.any()), "verify flags an encoded batch"

    nbytes = n * B * G
    sides = [("verify (A)", lambda: code.verify(data, par, B, bad_rows=bad_a)),
             ("verify (B)", lambda: code.verify(data, par, B, bad_rows=bad_b)),
             ("locate, clean", lambda: code.locate(data, par, B, culprit=culprit, marks=marks, counts=counts)),
             ("locate, 1 % damaged", lambda: code.locate(d1, p1, B, culprit=culprit, marks=marks, counts=counts)),
             ("locate, all damaged", lambda: code.locate(dall, pall, B, culprit=culprit, marks=marks, counts=counts))]
    s = torch.cuda.current_stream()
    for _, fn in sides:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in sides}
    order = random.Random(0x5EED0006)
    for _ in range(rounds):
        # a fresh order every round: what ran before a side (caches, clocks) shifts its time
        for name, fn in order.sample(sides, len(sides)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(reps):
                fn()
            e1.record(s)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps)
    emit(f"RS({k},{m}) B={B} G={G}: {rounds} interleaved rounds x {reps} calls, device events")
    med = {}
    for name, _ in sides:
        med[name] = statistics.median(times[name])
        rate = nbytes / (med[name] * 1e-3)
        emit(f"  {name:22s} median {med[name] * 1e3:8.1f} us  min {min(times[name]) * 1e3:8.1f} us  "
             f"max {max(times[name]) * 1e3:8.1f} us  {nbytes / 1e6:9.1f} MB  {rate / 1e9:7.1f} GB/s = {rate / PEAK:5.3f} of 8 TB/s")
    aa = abs(med["verify (A)"] - med["verify (B)"])
    emit(f"  verify A/A: medians differ by {aa * 1e3:.1f} us ({aa / med['verify (A)'] * 100:.2f} %); "
         f"locate, clean - verify (A): {(med['locate, clean'] - med['verify (A)']) * 1e3:+.1f} us "
         f"({(med['locate, clean'] / med['verify (A)'] - 1) * 100:+.2f} %), two presets and the finish kernel included")

    # scrub against verify + read-back + repair, 1 % damage, host clock around one synchronised call
    marks1 = torch.from_numpy(marks_to_rs_layout((np.arange(n)[None, :] == exp1[:, None]).astype(np.uint8), k))
    flagged = exp1 >= 0

    def scrub():
        code.scrub(d1, p1, B, culprit=culprit, counts=counts)
        torch.cuda.synchronize()

    def two_calls():
        code.verify(d1, p1, B, bad_rows=bad_a)
        host = bad_a.cpu().numpy()  # synchronises
        assert np.array_equal(host != 0, flagged)
        code.repair(d1, p1, marks1.to(dev), B)
        torch.cuda.synchronize()

    host_t = {"scrub": [], "verify + read-back + repair": []}
    for r in range(warmup + rounds):
        for name, fn in (("scrub", scrub), ("verify + read-back + repair", two_calls)):
            hurt1()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            assert torch.equal(d1[..., :B], data[..., :B]) and torch.equal(p1[..., :B], par[..., :B]), name
            if r >= warmup:
                host_t[name].append(dt * 1e3)
    emit(f"  1 % of the groups with one corrupted byte, host clock around one call that ends in a synchronise, {rounds} rounds:")
    for name, ts in host_t.items():
        emit(f"  {name:28s} median {statistics.median(ts) * 1e3:8.1f} us  min {min(ts) * 1e3:8.1f} us")


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
