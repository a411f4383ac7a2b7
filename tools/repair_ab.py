#!/usr/bin/env python3
"""Interleaved timing, in ONE process on the same buffers, of

  qfec_repair                       against  qfec_reconstruct + qfec_encode (the two-call way of
                                             bringing a batch back to full strength)
  qfec_verify                       against  qfec_encode (same rows read; m rows compared, not written)

Every round times each side back to back (device events, warm-up first), so drift between runs
does not pass for a kernel difference.  Before timing, repair and the two-call sequence must leave
identical data and identical marked parity rows.  Bytes are algorithmic (what has to move):
repair sum (k + t_g) B over repaired groups; two calls sum (k + e_g) B over groups with erased data
plus (k + m) B G; verify and encode (k + m) B G.

  python tools/repair_ab.py [--shape 10,3,1024,100000,0x5EED0003] [--rounds 12] [--reps 10] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import quicknet_amd as qa  # noqa: E402
from quicknet_amd.synth import erasure_marks, marks_to_rs_layout  # noqa: E402

PEAK = 8.0e12  # MI355X HBM3E, bytes per second
SHAPES = ["10,3,1024,100000,0x5EED0003", "16,4,1400,250000,0x5EED0004"]


def run(shape, rounds, reps, warmup, emit):
    k, m, B, G, seed = (int(x, 0) for x in shape.split(","))
    dev = torch.device("cuda:0")
    pitch = (B + 15) // 16 * 16
    code = qa.Code.cauchy(k, m)
    gm = erasure_marks(seed, G, k + m, m)  # m erasures per group, uniform over the n positions
    t_g, e_g = gm.sum(1), gm[:, :k].sum(1)
    marks = torch.from_numpy(marks_to_rs_layout(gm, k)).to(dev)
    data = torch.empty((G, k, pitch), dtype=torch.uint8, device=dev)
    qa.synth_fill(data, 0x5EED0002)
    par = torch.empty((G, m, pitch), dtype=torch.uint8, device=dev)
    code.encode(data, par, B)
    lost_d = torch.from_numpy(gm[:, :k].astype(bool)).to(dev)
    lost_p = torch.from_numpy(gm[:, k:].astype(bool)).to(dev)
    # side A (repair) and side B (two calls) each work on their own damaged copy
    da, pa, db, pb = data.clone(), par.clone(), data.clone(), par.clone()
    for d, p in ((da, pa), (db, pb)):
        d[lost_d] = 0x5A
        p[lost_p] = 0x5A
    code.prepare_repair()
    code.prepare_reconstruct()
    bad = torch.empty(G, dtype=torch.int32, device=dev)

    def repair():
        code.repair(da, pa, marks, B)

    def two_calls():
        code.reconstruct(db, pb, marks, B)
        code.encode(db, pb, B)

    def verify():
        code.verify(data, par, B, bad_rows=bad)

    def encode():
        code.encode(data, par, B)

    repair()
    two_calls()
    torch.cuda.synchronize()
    assert torch.equal(da[..., :B], db[..., :B]), "repair and reconstruct + encode leave different data"
    assert torch.equal(pa[..., :B][lost_p], pb[..., :B][lost_p]), "different marked parity rows"
    assert torch.equal(da[..., :B], data[..., :B]) and torch.equal(pa[..., :B], par[..., :B])
    verify()
    torch.cuda.synchronize()
    assert not bool(bad.any()), "verify flags an encoded batch"

    rep_bytes = int((k * (t_g > 0).sum() + t_g.sum()) * B)  # every group has t = m <= m: all repaired
    two_bytes = int((k * (e_g > 0).sum() + e_g.sum()) * B) + (k + m) * B * G
    vfy_bytes = (k + m) * B * G
    sides = [("repair", repair, rep_bytes), ("reconstruct + encode", two_calls, two_bytes),
             ("verify", verify, vfy_bytes), ("encode", encode, vfy_bytes)]
    s = torch.cuda.current_stream()
    for _, fn, _ in sides:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in sides}
    for _ in range(rounds):
        for name, fn, _ in sides:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(reps):
                fn()
            e1.record(s)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps)
    emit(f"RS({k},{m}) B={B} G={G} seed {seed:#x}: {m} erasures per group over n = {k + m}, "
         f"{rounds} interleaved rounds x {reps} launches")
    med = {}
    for name, _, nbytes in sides:
        med[name] = statistics.median(times[name])
        rate = nbytes / (med[name] * 1e-3)
        emit(f"  {name:22s} median {med[name] * 1e3:8.1f} us  min {min(times[name]) * 1e3:8.1f} us  "
             f"{nbytes / 1e6:9.1f} MB  {rate / 1e9:7.1f} GB/s = {rate / PEAK:5.3f} of 8 TB/s")
    emit(f"  two calls / repair: time {med['reconstruct + encode'] / med['repair']:.2f}x, "
         f"bytes {two_bytes / rep_bytes:.2f}x (the expectation for HBM-bound kernels)")
    emit(f"  verify / encode: time {med['verify'] / med['encode']:.2f}x on the same bytes")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append", help="k,m,B,G,seed (repeatable); default: " + " and ".join(SHAPES))
    p.add_argument("--rounds", type=int, default=12)
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
