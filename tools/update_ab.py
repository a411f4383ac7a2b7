#!/usr/bin/env python3
"""Interleaved timing, in ONE process on the same buffers, of the incremental parity calls against
the only way to do their job without them, a full qfec_encode of the batch:

  qfec_encode of the batch, twice (A/A: the spread, and the yardstick)
  qfec_update with every group touched at a random shard
  qfec_update with 10 % of the groups touched
  qfec_update with no group touched: the call's floor
  qfec_update in delta-only mode, every group touched
  qfec_encode_update with count = 1, accumulate on
  qfec_encode_update with count = k, accumulate off

Every round times each side back to back (device events around `reps` calls, warm-up first), and the
order within a round is drawn anew every round, because a side's time depends on what ran before it
(caches, clocks).  Before anything is timed the calls are checked: an updated copy of the batch
verifies clean (qfec_verify) and equals a fresh encode of the new data, also in delta mode, and the range form over [0, 1) + [1, k) equals the encode.  Bytes are each leg's own
algorithmic bytes: per touched group 2 + m rows read and 1 + m written (delta mode: 1 + m and m),
plus the 4-byte id of every group; count + m rows (+ m with accumulate) per group for the range form.

  python tools/update_ab.py [--shape 10,3,1024,1024,100000] [--rounds 15] [--reps 10] [--out FILE]
"""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12  # MI355X HBM3E, bytes per second
SHAPES = ["10,3,1024,1024,100000", "16,4,1400,1408,250000"]  # k, m, B, pitch, G


def run(shape, rounds, reps, warmup, emit):
    import numpy as np
    import torch

    import quicknet_amd as qa

    k, m, B, pitch, G = (int(x, 0) for x in shape.split(","))
    dev = torch.device("cuda:0")
    code = qa.Code.cauchy(k, m)
    data = torch.empty((G, k, pitch), dtype=torch.uint8, device=dev)
    qa.synth_fill(data, 0x5EED0002)
    par = torch.empty((G, m, pitch), dtype=torch.uint8, device=dev)
    code.encode(data, par, B)
    rows = torch.empty((G, pitch), dtype=torch.uint8, device=dev)
    qa.synth_fill(rows, 0x5EED0009)
    rng = np.random.default_rng(0x5EED000A)
    every = rng.integers(0, k, G).astype(np.int32)
    tenth = np.full(G, qa.QFEC_UPD_NONE, np.int32)
    some = rng.choice(G, G // 10, replace=False)
    tenth[some] = every[some]
    shard = {"all": torch.from_numpy(every).to(dev), "10 %": torch.from_numpy(tenth).to(dev),
             "none": torch.full((G,), qa.QFEC_UPD_NONE, dtype=torch.int32, device=dev)}
    touched = {"all": G, "10 %": len(some), "none": 0}

    # ---- the calls are right before they are timed
    gi = torch.arange(G, device=dev)
    for which in ("all", "10 %", "none"):
        ids = shard[which]
        hit = ids >= 0
        want = data.clone()
        want[gi[hit], ids[hit].long()] = rows[hit]
        fresh = torch.empty_like(par)
        code.encode(want, fresh, B)
        delta = rows.clone()
        delta[hit] ^= data[gi[hit], ids[hit].long()]
        d, p = data.clone(), par.clone()
        code.update(ids, rows, p, data=d, block_size=B)
        bad = code.verify(d, p, B)
        assert not bool(bad.any()), f"update, {which} touched: verify finds bad groups"
        assert torch.equal(d[..., :B], want[..., :B]) and torch.equal(p[..., :B], fresh[..., :B]), which
        p = par.clone()
        code.update(ids, delta, p, data=None, block_size=B)
        assert torch.equal(p[..., :B], fresh[..., :B]), f"delta only, {which} touched"
    p = torch.empty_like(par)
    code.encode_update(data[:, :1].contiguous(), p, 0, B, accumulate=False)
    code.encode_update(data[:, 1:].contiguous(), p, 1, B, accumulate=True)
    assert torch.equal(p[..., :B], par[..., :B]), "encode_update over [0, 1) + [1, k) differs from the encode"
    code.encode_update(data, p, 0, B, accumulate=False)
    assert torch.equal(p[..., :B], par[..., :B]), "encode_update over [0, k) differs from the encode"
    del want, fresh, delta, d, p

    # ---- timing: scratch copies, so the yardstick's buffers keep their bytes
    wd, wp = data.clone(), par.clone()
    one = data[:, :1].contiguous()
    row = B  # bytes of a row that count

    def upd(which, with_data=True):  # any bytes do as deltas
        return lambda: code.update(shard[which], rows, wp, data=wd if with_data else None, block_size=B)

    sides = [("encode (A)", (k + m) * row * G, lambda: code.encode(data, par, B)),
             ("encode (B)", (k + m) * row * G, lambda: code.encode(data, par, B))]
    for which in ("all", "10 %", "none"):
        sides.append((f"update, {which} touched", touched[which] * (3 + 2 * m) * row + 4 * G, upd(which)))
    sides.append(("update, delta only, all touched", G * (1 + 2 * m) * row + 4 * G, upd("all", with_data=False)))
    sides.append(("encode_update, count = 1, accumulate", (1 + 2 * m) * row * G,
                  lambda: code.encode_update(one, wp, k - 1, B, accumulate=True)))
    sides.append((f"encode_update, count = {k}, overwrite", (k + m) * row * G,
                  lambda: code.encode_update(data, wp, 0, B, accumulate=False)))
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
    emit(f"RS({k},{m}) B={B} pitch={pitch} G={G}: {rounds} interleaved rounds x {reps} calls, device events")
    med = {}
    for name, nbytes, _ in sides:
        med[name] = statistics.median(times[name])
        rate = nbytes / (med[name] * 1e-3)
        emit(f"  {name:44s} median {med[name] * 1e3:8.1f} us  min {min(times[name]) * 1e3:8.1f} us  "
             f"max {max(times[name]) * 1e3:8.1f} us  {nbytes / 1e6:9.1f} MB  {rate / 1e9:7.1f} GB/s = {rate / PEAK:5.3f} of 8 TB/s")
    enc = min(med["encode (A)"], med["encode (B)"]), max(med["encode (A)"], med["encode (B)"])
    emit(f"  encode A/A: medians differ by {(enc[1] - enc[0]) * 1e3:.1f} us ({(enc[1] / enc[0] - 1) * 100:.2f} %)")
    a, t = med["update, all touched"], med["update, 10 % touched"]
    emit(f"  update all touched / encode = {a / enc[1]:.3f} .. {a / enc[0]:.3f} (bytes: {(3 + 2 * m) / (k + m):.3f}); "
         f"10 % touched / all touched = {t / a:.3f}")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append", help="k,m,B,pitch,G (repeatable); default: " + " and ".join(SHAPES))
    p.add_argument("--rounds", type=int, default=15)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default="", help="also write the report to this file")
    a = p.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    import torch

    import quicknet_amd as qa

    emit(f"{qa.lib().qfec_version().decode()} on {torch.cuda.get_device_name(0)}")
    for shape in a.shape or SHAPES:
        run(shape, a.rounds, a.reps, a.warmup, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
