#!/usr/bin/env python3
"""Interleaved timing, in ONE process, of qfec_locate_ptrs_wide_var (single-shard error location at any
k + m on a table of shard addresses, every data shard with its own length) against qfec_locate_ptrs_wide
on the same rows zero-padded to max_len:

  qfec_locate_ptrs_wide on the padded rows, twice (A/A: the yardstick and its spread)
  qfec_locate_ptrs_wide_var on the same table with the lengths

per shape with 0 and 4 lost shards per group, one byte damaged in one surviving shard of 1 % of the
groups (inside the shard's own length), and three length cases: every length = max_len (the var call's
fixed-length body), every data length of one group in ten drawn from [64, max_len], every data length
of every group drawn from there (the ragged body; a short shard's bytes are not loaded).  Every group's
parity length is max_len, so the padded rows are the same bytes in both calls.  The rows lie in order
in one buffer, 16-byte aligned; the rows of lost shards hold what the batch held and are not read.

Every round times each leg (a device event pair around every call, `reps` calls, warm-up first) in an
order drawn anew every round.  Before anything is timed the verdicts of both calls are checked against
how the damage was made, and the var call's marks and counts against the fixed-length call's.

  python tools/locate_ptrs_wide_var_ab.py [--shape 32,8,1024,1024,20000] [--rounds 15] [--reps 5] [--out FILE]
"""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from locate_wide_ab import CLEAN, PEAK, WIDE, outputs  # noqa: E402

LENGTHS = ["all lengths = max_len", "one group in ten short", "every length drawn"]


def make_case(code, dims, lost, lengths, seed):
    """(data, parity, marks, lens, group_len on the device, expected culprits, bytes the var call reads)."""
    import numpy as np
    import torch

    import quicknet_amd as qa
    from quicknet_amd.synth import erasure_marks, marks_to_rs_layout

    k, m, B, pitch, G = dims
    n = k + m
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(seed)
    lens = np.full((G, k), B, np.int32)
    drawn = rng.integers(min(64, B), B + 1, size=(G, k)).astype(np.int32)
    if lengths == LENGTHS[1]:
        lens[::10] = drawn[::10]
    elif lengths == LENGTHS[2]:
        lens = drawn
    data = torch.empty((G, k, pitch), dtype=torch.uint8, device=dev)
    qa.synth_fill(data, 0x5EED0002)
    d_lens = torch.from_numpy(lens).to(dev)
    data *= (torch.arange(pitch, device=dev)[None, None, :] < d_lens[:, :, None]).to(torch.uint8)  # zero from each end on
    par = torch.empty((G, m, pitch), dtype=torch.uint8, device=dev)
    code.encode(data, par, B)
    torch.cuda.synchronize()
    gm = erasure_marks(seed, G, n, lost) if lost else np.zeros((G, n), np.uint8)
    expect = np.full(G, CLEAN, np.int32)
    for g in np.nonzero(rng.random(G) < 0.01)[0]:
        c = int(rng.integers(0, n))
        while gm[g, c]:
            c = (c + 1) % n
        expect[g] = c
        b = int(rng.integers(0, lens[g, c] if c < k else B))
        (data[g, c] if c < k else par[g, c - k])[b] ^= int(rng.integers(1, 256))
    read = int(np.where(gm[:, :k] == 0, lens, 0).sum()) + int((gm[:, k:] == 0).sum()) * B
    marks = torch.from_numpy(marks_to_rs_layout(gm, k)).to(dev)
    glen = torch.full((G,), B, dtype=torch.int32, device=dev)
    return data, par, marks, d_lens.reshape(-1).contiguous(), glen, expect, read


def run(shape, rounds, reps, warmup, emit):
    import numpy as np
    import torch

    import quicknet_amd as qa

    k, m, B, pitch, G = dims = tuple(int(x, 0) for x in shape.split(","))
    n = k + m
    code = qa.Code.cauchy(k, m)
    dev = torch.device("cuda:0")
    emit(f"RS({k},{m}) max_len={B} pitch={pitch} G={G}: qfec_locate_ptrs_wide on zero-padded rows against "
         f"qfec_locate_ptrs_wide_var, check plan stride {code.check_stride()} B, {rounds} interleaved rounds x {reps} calls, "
         f"a device event pair per call")
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
        for li, lengths in enumerate(LENGTHS):
            d, p, marks, lens, glen, expect, read = make_case(code, dims, lost, lengths, 0x5EED0300 + 16 * lost + li)
            table = torch.cat([torch.arange(G * k, device=dev, dtype=torch.int64) * pitch + d.data_ptr(),
                               torch.arange(G * m, device=dev, dtype=torch.int64) * pitch + p.data_ptr()]).contiguous()
            # ---- both legs are right before they are timed
            c0, o0, n0 = outputs(G, n, dev)
            code.locate_ptrs_wide(table, B, marks, culprit=c0, marks_out=o0, counts=n0)
            c1, o1, n1 = outputs(G, n, dev)
            inv = torch.zeros(1, dtype=torch.int32, device=dev)
            code.locate_ptrs_wide_var(table, lens, glen, B, marks, culprit=c1, marks_out=o1, counts=n1, invalid=inv)
            torch.cuda.synchronize()
            assert np.array_equal(c0.cpu().numpy(), expect), "qfec_locate_ptrs_wide disagrees with the damage"
            assert torch.equal(c1, c0) and torch.equal(o1, o0) and torch.equal(n1, n0) and int(inv.item()) == 0, \
                "locate_ptrs_wide_var differs"
            padded = (n - lost) * B * G + G * code.check_stride() + 8 * n * G
            ragged = read + G * code.check_stride() + 8 * n * G + 4 * (k + 1) * G
            fixed = lambda: code.locate_ptrs_wide(table, B, marks, culprit=c0)  # noqa: E731
            sides = [("locate_ptrs_wide, padded (A)", padded, fixed), ("locate_ptrs_wide, padded (B)", padded, fixed),
                     ("locate_ptrs_wide_var", ragged,
                      lambda: code.locate_ptrs_wide_var(table, lens, glen, B, marks, culprit=c1))]
            for _, _, fn in sides:
                timed(fn, warmup)
            times = {s[0]: [] for s in sides}
            order = random.Random(0x5EED0008 + lost + li)
            for _ in range(rounds):
                for sname, _, fn in order.sample(sides, len(sides)):
                    times[sname].append(timed(fn, reps))
            emit(f" {lost} lost per group, {lengths}: {(expect >= 0).sum()} of {G} groups corrupted; bytes read {padded / 1e6:.1f} MB "
                 f"padded = {padded / PEAK * 1e6:.1f} us at 8 TB/s, {ragged / 1e6:.1f} MB with lengths")
            med = {}
            for sname, nb, _ in sides:
                med[sname] = statistics.median(times[sname])
                emit(f"  {sname:32s} median {med[sname] * 1e3:9.1f} us  min {min(times[sname]) * 1e3:9.1f} us  "
                     f"max {max(times[sname]) * 1e3:9.1f} us  {nb / (med[sname] * 1e-3) / 1e9:7.1f} GB/s")
            a, b = med[sides[0][0]], med[sides[1][0]]
            mid = statistics.median(times[sides[0][0]] + times[sides[1][0]])
            emit(f"  A/A: medians differ by {abs(a - b) * 1e3:.1f} us ({(max(a, b) / min(a, b) - 1) * 100:.2f} %); yardstick "
                 f"(median of both) {mid * 1e3:.1f} us")
            emit(f"    locate_ptrs_wide_var: {med['locate_ptrs_wide_var'] / mid:.3f} x qfec_locate_ptrs_wide")
            del d, p, table


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append", help="k,m,max_len,pitch,G (repeatable); default: " + " and ".join(WIDE))
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
