#!/usr/bin/env python3
"""Interleaved timing, in ONE process on the same buffers, of qfec_reconstruct_wide (decode plans
built on the device) against qfec_reconstruct on a wide code, k + m > 24, where qfec_reconstruct
reads the marks back, builds decode records per distinct pattern on the host and returns after its
kernel has run (the host-record path):

  random mix   every group draws min(m, 4) erasures of its own over the k + m shards
    qfec_reconstruct, marks it has not seen (A) and (B)   every timed call gets a marks set of its own and a
                                                          code object of its own (the host keeps the records
                                                          of the patterns a code has seen, and patterns recur
                                                          between sets), so the host inverts for every
                                                          distinct pattern of the set
    qfec_reconstruct, the same marks again                the code's host cache of records is warm
    qfec_reconstruct_wide
  one pattern  every group shares one pattern
    qfec_reconstruct (A) and (B), qfec_reconstruct_wide

Each timed call runs from the call to a stream synchronise on a host clock (qfec_reconstruct
synchronises inside; the wide call is asynchronous), one call per timing, and the order within a
round is drawn anew every round.  (A) and (B) are the same side twice: their difference is the
spread.  Before anything is timed the two calls' outputs are compared byte for byte.  The apply
kernel's algorithmic bytes, (k + e) x B per touched group plus the plan bytes, are printed for the
kernel trace (--profile MIX runs only the wide call on one mix, for `rocprofv3 --kernel-trace --stats
-- python tools/wide_ab.py --shape ... --profile random`).

  python tools/wide_ab.py [--shape 32,8,1024,1024,20000] [--rounds 3] [--out FILE] [--profile random|one]
"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12  # MI355X HBM3E, bytes per second
SHAPES = ["32,8,1024,1024,20000", "64,16,1024,1024,20000"]  # k, m, B, pitch, G


def run(shape, rounds, profile, emit):
    import numpy as np
    import torch

    import quicknet_amd as qa
    from quicknet_amd.synth import erasure_marks, marks_to_rs_layout

    k, m, B, pitch, G = (int(x, 0) for x in shape.split(","))
    n, lose = k + m, min(m, 4)
    dev = torch.device("cuda:0")
    code = qa.Code.cauchy(k, m)
    data = torch.empty((G, k, pitch), dtype=torch.uint8, device=dev)
    qa.synth_fill(data, 0x5EED0002)
    par = torch.empty((G, m, pitch), dtype=torch.uint8, device=dev)
    code.encode(data, par, B)
    torch.cuda.synchronize()

    def marks_set(seed):
        gm = erasure_marks(seed, G, n, lose)
        return gm, torch.from_numpy(marks_to_rs_layout(gm, k)).to(dev)

    fresh = [marks_set(0x5EED1000 + i) for i in range(1 if profile else 2 * rounds + 2)]
    one = np.tile(erasure_marks(0x5EED0F00, 1, n, lose), (G, 1))
    while not one[0, :k].any():  # the shared pattern must lose data
        one = np.roll(one, 1, axis=1)
    one_d = torch.from_numpy(marks_to_rs_layout(one, k)).to(dev)

    def algorithmic(gm):
        e = gm[:, :k].sum(1)
        return int(((k + e[e > 0]) * B).sum()) + G * code.plan_stride(), int((e > 0).sum())

    emit(f"RS({k},{m}) B={B} pitch={pitch} G={G}, {lose} erasures per group, plan stride {code.plan_stride()} B")
    for name, gm in (("random mix", fresh[0][0]), ("one pattern", one)):
        nbytes, touched = algorithmic(gm)
        pats = len({r.tobytes() for r in gm})
        emit(f"  {name}: {pats} distinct patterns, {touched} groups lose data, k_plan_apply algorithmic bytes "
             f"{nbytes / 1e6:.1f} MB = {nbytes / PEAK * 1e6:.1f} us at 8 TB/s")

    def damaged(gm):
        d = data.clone()
        d.view(G * k, pitch)[torch.from_numpy(gm[:, :k].reshape(-1) == 1).to(dev)] = 0x5A
        return d

    if profile:
        for gm, md in ((fresh[0],) if profile == "random" else ((one, one_d),)):
            d = damaged(gm)
            for _ in range(5):
                code.reconstruct_wide(d, par, md, B)
            torch.cuda.synchronize()
            assert torch.equal(d[..., :B], data[..., :B])
        return

    # ---- the two calls agree before they are timed
    for gm, md in (fresh[-1], (one, one_d)):
        d1, d2 = damaged(gm), damaged(gm)
        f1 = torch.zeros(1, dtype=torch.int32, device=dev)
        f2 = torch.zeros(1, dtype=torch.int32, device=dev)
        code.reconstruct(d1, par, md, B, f1)
        code.reconstruct_wide(d2, par, md, B, f2)
        torch.cuda.synchronize()
        assert torch.equal(d1, d2) and torch.equal(d1[..., :B], data[..., :B]) and f1.item() == f2.item() == 0

    work = damaged(fresh[-1][0])  # the erased rows are rewritten with the same bytes every call
    work_one = damaged(one)
    sets = iter(fresh[:-1])
    unseen = iter([qa.Code.cauchy(k, m) for _ in fresh[:-1]])  # codes that have seen no pattern yet

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    warm_d = fresh[-1][1]
    sides = [
        ("random: reconstruct, unseen marks (A)", lambda: next(unseen).reconstruct(work, par, next(sets)[1], B)),
        ("random: reconstruct, unseen marks (B)", lambda: next(unseen).reconstruct(work, par, next(sets)[1], B)),
        ("random: reconstruct, same marks again", lambda: code.reconstruct(work, par, warm_d, B)),
        ("random: reconstruct_wide", lambda: code.reconstruct_wide(work, par, warm_d, B)),
        ("one pattern: reconstruct (A)", lambda: code.reconstruct(work_one, par, one_d, B)),
        ("one pattern: reconstruct (B)", lambda: code.reconstruct(work_one, par, one_d, B)),
        ("one pattern: reconstruct_wide", lambda: code.reconstruct_wide(work_one, par, one_d, B)),
    ]
    for name, fn in sides[2:]:  # warm-up; the unseen-marks sides must stay unseen
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in sides}
    order = random.Random(0x5EED0008)
    for _ in range(rounds):
        for name, fn in order.sample(sides, len(sides)):
            times[name].append(timed(fn))
    emit(f"  {rounds} interleaved rounds, one call per timing, host clock from the call to a stream synchronise")
    med = {}
    for name, _ in sides:
        med[name] = statistics.median(times[name])
        emit(f"  {name:42s} median {med[name]:10.3f} ms  min {min(times[name]):10.3f} ms  max {max(times[name]):10.3f} ms")
    for mix, a, b, w in (("random mix, unseen marks", sides[0][0], sides[1][0], sides[3][0]),
                         ("one pattern", sides[4][0], sides[5][0], sides[6][0])):
        lo, hi = sorted((med[a], med[b]))
        emit(f"  {mix}: A/A medians differ by {hi - lo:.3f} ms ({(hi / lo - 1) * 100:.1f} %); "
             f"reconstruct / reconstruct_wide = {lo / med[w]:.2f} .. {hi / med[w]:.2f}")
    emit(f"  random mix, same marks again / reconstruct_wide = {med[sides[2][0]] / med[sides[3][0]]:.2f}")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append", help="k,m,B,pitch,G (repeatable); default: " + " and ".join(SHAPES))
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--profile", choices=["random", "one"],
                   help="run only qfec_reconstruct_wide on this mix, five times (for a kernel trace)")
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
        run(shape, a.rounds, a.profile, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
