#!/usr/bin/env python3
"""Interleaved timing, in ONE process, of qfec_locate_ptrs_wide (single-shard error location at any
k + m on a table of shard addresses) against qfec_locate_wide on the same bytes:

  qfec_locate_wide on the contiguous batch, twice (A/A: the yardstick and its spread)
  qfec_locate_ptrs_wide, the table pointing at those same rows in order (every row 16-B aligned)
  qfec_locate_ptrs_wide, the rows permuted at random inside one pool, slot pitch = B rounded up to 128

per shape with 0 and 4 lost shards per group, on a consistent batch and on one with a single damaged
shard (one byte) in 1 % of the groups.  The rows of lost shards hold what the batch held: they are
not read.

Every round times each leg (a device event pair around every call, `reps` calls, warm-up first) in an
order drawn anew every round.  Before anything is timed the verdicts of the three layouts are checked
against how the damage was made, and the marks and counts of the table calls against the contiguous
call's.  Each table leg is stated as a ratio to the contiguous call's A/A median of the same case.

  python tools/locate_ptrs_wide_ab.py [--shape 32,8,1024,1024,20000] [--rounds 15] [--reps 5] [--out FILE]
"""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from locate_wide_ab import CASES, PEAK, WIDE, batch, make_case, outputs  # noqa: E402
from ptrs_ab import Scattered  # noqa: E402


def run(shape, rounds, reps, warmup, emit):
    import numpy as np
    import torch

    code, data, par, dims = batch(shape)
    k, m, B, pitch, G = dims
    n = k + m
    dev = data.device
    r128 = (B + 127) // 128 * 128
    emit(f"RS({k},{m}) B={B} pitch={pitch} G={G}: qfec_locate_wide against qfec_locate_ptrs_wide, check plan stride "
         f"{code.check_stride()} B, {rounds} interleaved rounds x {reps} calls, a device event pair per call")
    s0 = torch.cuda.current_stream()

    def timed(fn, count):
        pairs = []
        for _ in range(count):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s0)
            fn()
            e1.record(s0)
            pairs.append((e0, e1))
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in pairs) / count

    for lost in (0, 4):
        for name in ("clean", "one"):
            d, p, marks, expect = make_case(code, data, par, dims, lost, CASES[name], 0x5EED0200 + lost)
            inorder = torch.cat([torch.arange(G * k, device=dev, dtype=torch.int64) * pitch + d.data_ptr(),
                                 torch.arange(G * m, device=dev, dtype=torch.int64) * pitch + p.data_ptr()]).contiguous()
            pool = Scattered(torch, dev, G * n, B, r128, 0, 0x5EED0011)
            pool.put(0, d.view(G * k, pitch))
            pool.put(G * k, p.view(G * m, pitch))
            tables = {"in order": inorder, "permuted, slot pitch %d" % r128: pool.table}
            # ---- every leg is right before it is timed
            c0, o0, n0 = outputs(G, n, dev)
            code.locate_wide(d, p, marks, B, culprit=c0, marks_out=o0, counts=n0)
            torch.cuda.synchronize()
            assert np.array_equal(c0.cpu().numpy(), expect), "qfec_locate_wide disagrees with the damage"
            for tname, t in tables.items():
                c1, o1, n1 = outputs(G, n, dev)
                code.locate_ptrs_wide(t, B, marks, culprit=c1, marks_out=o1, counts=n1)
                torch.cuda.synchronize()
                assert torch.equal(c1, c0) and torch.equal(o1, o0) and torch.equal(n1, n0), f"locate_ptrs_wide, {tname}: differs"
            nbytes = (n - lost) * B * G + G * code.check_stride()
            sides = [("locate_wide (A)", nbytes, lambda: code.locate_wide(d, p, marks, B, culprit=c0)),
                     ("locate_wide (B)", nbytes, lambda: code.locate_wide(d, p, marks, B, culprit=c0))]
            for tname, t in tables.items():
                sides.append((f"locate_ptrs_wide, {tname}", nbytes + 8 * n * G,
                              lambda t=t: code.locate_ptrs_wide(t, B, marks, culprit=c0)))
            for _, _, fn in sides:
                timed(fn, warmup)
            times = {s[0]: [] for s in sides}
            order = random.Random(0x5EED0008 + lost)
            for _ in range(rounds):
                for sname, _, fn in order.sample(sides, len(sides)):
                    times[sname].append(timed(fn, reps))
            emit(f" {lost} lost per group, {name}: {(expect >= 0).sum()} of {G} groups corrupted; apply kernel's algorithmic "
                 f"bytes {nbytes / 1e6:.1f} MB = {nbytes / PEAK * 1e6:.1f} us at 8 TB/s")
            med = {}
            for sname, nb, _ in sides:
                med[sname] = statistics.median(times[sname])
                emit(f"  {sname:44s} median {med[sname] * 1e3:9.1f} us  min {min(times[sname]) * 1e3:9.1f} us  "
                     f"max {max(times[sname]) * 1e3:9.1f} us  {nb / (med[sname] * 1e-3) / 1e9:7.1f} GB/s")
            a, b = med["locate_wide (A)"], med["locate_wide (B)"]
            mid = statistics.median(times["locate_wide (A)"] + times["locate_wide (B)"])
            emit(f"  A/A: medians differ by {abs(a - b) * 1e3:.1f} us ({(max(a, b) / min(a, b) - 1) * 100:.2f} %); yardstick "
                 f"(median of both) {mid * 1e3:.1f} us")
            for tname in tables:
                emit(f"    locate_ptrs_wide, {tname}: {med[f'locate_ptrs_wide, {tname}'] / mid:.3f} x qfec_locate_wide")
            del pool, d, p


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append", help="k,m,B,pitch,G (repeatable); default: " + " and ".join(WIDE))
    p.add_argument("--rounds", type=int, default=15)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default="", help="also write the report to this file")
    a = p.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    import torch

    import quicknet_amd as qa

    emit(f"{qa.lib().qfec_version().decode()} on {torch.cuda.get_device_name(0)}")
    for shape in a.shape or WIDE:
        run(shape, a.rounds, a.reps, a.warmup, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
