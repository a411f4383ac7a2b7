#!/usr/bin/env python3
"""Interleaved timing, in ONE process, of the plan calls on pointer tables against the calls they join.

Wide codes (--shape k,m,B,pitch,G; 4 erasures per group; a random mix and one shared pattern):
  reconstruct_wide / repair_wide (A) and (B)   contiguous rows: the same side twice, their difference is the spread
  reconstruct_ptrs_wide / repair_ptrs_wide on
    in order                                   a table over the same contiguous rows: the price of the indirection
    permuted, slot pitch P                     every row at a random slot of a pool, slots a multiple of 128 B
    permuted, misaligned                       every row 8 B off a 16-B boundary: the byte body
Narrow codes (--narrow k,m,B,pitch,G; m erasures per group):
  reconstruct_ptrs (A) and (B) against reconstruct_ptrs_wide on a permuted, aligned pool
module/rs.h (--rs k,m,B,G --rs-wide 0|1): reed_solomon_reconstruct on all-device scattered rows with
  rs_dev_ptrs = 1 and rs_dev_ptrs_wide as given, wall clock, one call, one setting per process.

Device events around `reps` calls, the order within a round drawn anew every round.  Before anything
is timed every leg's output is compared byte for byte with the contiguous call's.  --profile runs only
the contiguous and the in-order pointer reconstruct on the random mix, five times each (for
`rocprofv3 --kernel-trace --stats -- python tools/ptrs_wide_ab.py --shape ... --profile`).

  python tools/ptrs_wide_ab.py [--shape 32,8,1024,1024,20000] [--narrow 10,3,1024,1024,100000] [--rounds 5] [--out FILE]
"""
import argparse
import ctypes as C
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ptrs_ab import Scattered  # noqa: E402

SHAPES = ["32,8,1024,1024,20000", "64,16,1024,1024,20000"]
NARROW = ["10,3,1024,1024,100000", "16,4,1400,1408,250000"]


def interleave(torch, sides, rounds, reps, warmup):
    """{name: [ms per call]} over `rounds` rounds in a fresh order each."""
    s0 = torch.cuda.current_stream()
    for _, fn in sides:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in sides}
    order = random.Random(0x5EED0008)
    for _ in range(rounds):
        for name, fn in order.sample(sides, len(sides)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s0)
            for _ in range(reps):
                fn()
            e1.record(s0)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps)
    return times


def report(emit, times, sides):
    med = {}
    for name, _ in sides:
        med[name] = statistics.median(times[name])
        emit(f"  {name:52s} median {med[name] * 1e3:9.1f} us  min {min(times[name]) * 1e3:9.1f} us  max {max(times[name]) * 1e3:9.1f} us")
    return med


def batch(torch, qa, k, m, B, pitch, G):
    dev = torch.device("cuda:0")
    code = qa.Code.cauchy(k, m)
    data = torch.empty((G, k, pitch), dtype=torch.uint8, device=dev)
    qa.synth_fill(data, 0x5EED0002)
    par = torch.empty((G, m, pitch), dtype=torch.uint8, device=dev)
    code.encode(data, par, B)
    torch.cuda.synchronize()
    return dev, code, data, par


def run_wide(shape, rounds, reps, warmup, profile, emit):
    import numpy as np
    import torch

    import quicknet_amd as qa
    from quicknet_amd.synth import erasure_marks, marks_to_rs_layout

    k, m, B, pitch, G = (int(x, 0) for x in shape.split(","))
    n, lose = k + m, min(m, 4)
    dev, code, data, par = batch(torch, qa, k, m, B, pitch, G)
    drows, prows = data.view(G * k, pitch), par.view(G * m, pitch)
    mixes = {"random mix": erasure_marks(0x5EED1000, G, n, lose)}
    one = np.tile(erasure_marks(0x5EED0F00, 1, n, lose), (G, 1))
    while not (one[0, :k].any() and one[0, k:].any()):  # the shared pattern loses data and parity
        one = np.roll(one, 1, axis=1)
    mixes["one pattern"] = one
    base = torch.arange(G * k, device=dev, dtype=torch.int64) * pitch + data.data_ptr()
    pbase = torch.arange(G * m, device=dev, dtype=torch.int64) * pitch + par.data_ptr()
    r128 = (B + 127) // 128 * 128
    legs = {"in order": None,
            "permuted, slot pitch %d" % r128: Scattered(torch, dev, G * n, B, r128, 0, 0x5EED0011),
            "permuted, misaligned": Scattered(torch, dev, G * n, B, (B + 15) // 16 * 16 + 16, 8, 0x5EED0012)}
    tables = {name: (torch.cat([base, pbase]).contiguous() if s is None else s.table) for name, s in legs.items()}
    emit(f"RS({k},{m}) B={B} pitch={pitch} G={G}, {lose} erasures per group, plan stride {code.plan_stride()} B: "
         f"{rounds} interleaved rounds x {reps} calls, device events")

    for mix, gm in mixes.items():
        marks_h = marks_to_rs_layout(gm, k)
        marks = torch.from_numpy(marks_h).to(dev)
        hit_d = torch.from_numpy(marks_h[:G * k] == 1).to(dev)
        hit_p = torch.from_numpy(marks_h[G * k:] == 1).to(dev)

        def hurt_contiguous():
            d, p = data.clone(), par.clone()
            d.view(G * k, pitch)[hit_d, :B] = 0x5A
            p.view(G * m, pitch)[hit_p, :B] = 0x5A
            return d, p

        # ---- what every leg must leave: the contiguous calls' rows (the parity is the encode of the
        # data, so the repair restores both and the reconstruct restores the data)
        d, p = hurt_contiguous()
        code.repair_wide(d, p, marks, B)
        torch.cuda.synchronize()
        assert torch.equal(d[..., :B], data[..., :B]) and torch.equal(p[..., :B], par[..., :B]), "repair_wide"
        rec_d, rec_p = hurt_contiguous()
        hurt_p = rec_p.clone()
        code.reconstruct_wide(rec_d, rec_p, marks, B)
        torch.cuda.synchronize()
        assert torch.equal(rec_d[..., :B], data[..., :B]) and torch.equal(rec_p, hurt_p), "reconstruct_wide"
        for name, s in legs.items():
            for call, want_p in ((code.reconstruct_ptrs_wide, hurt_p), (code.repair_ptrs_wide, par)):
                failed = torch.zeros(1, dtype=torch.int32, device=dev)
                if s is None:
                    keep_d, keep_p = data.clone(), par.clone()
                    drows[hit_d, :B] = 0x5A
                    prows[hit_p, :B] = 0x5A
                    call(tables[name], marks, B, failed)
                    ok = torch.equal(data[..., :B], keep_d[..., :B]) and torch.equal(par[..., :B], want_p[..., :B])
                    data.copy_(keep_d)
                    par.copy_(keep_p)
                else:
                    s.put(0, drows)
                    s.put(G * k, prows)
                    s.rows2d[s.perm[:G * k][hit_d], s.lead:s.lead + B] = 0x5A
                    s.rows2d[s.perm[G * k:][hit_p], s.lead:s.lead + B] = 0x5A
                    call(tables[name], marks, B, failed)
                    ok = (torch.equal(s.get(0, G * k), drows[:, :B]) and
                          torch.equal(s.get(G * k, G * m), want_p.view(G * m, pitch)[:, :B]))
                assert ok and int(failed.item()) == 0, f"{mix}, {name}: differs from the contiguous call"
        # timed state: every marked row holds 0x5A before the first call and the restored bytes after
        # it; the survivors never change, so every call does the same work
        wd, wp = hurt_contiguous()
        for s in legs.values():
            if s is not None:
                s.put(0, drows)
                s.put(G * k, prows)
        if profile:
            for _ in range(5):
                code.reconstruct_wide(wd, wp, marks, B)
                code.reconstruct_ptrs_wide(tables["in order"], marks, B)
            torch.cuda.synchronize()
            return
        for call in ("reconstruct", "repair"):
            wide = getattr(code, call + "_wide")
            pw = getattr(code, call + "_ptrs_wide")
            sides = [(f"{mix}: {call}_wide (A)", lambda: wide(wd, wp, marks, B)),
                     (f"{mix}: {call}_wide (B)", lambda: wide(wd, wp, marks, B))]
            for name in legs:
                sides.append((f"{mix}: {call}_ptrs_wide, {name}", lambda t=tables[name]: pw(t, marks, B)))
            times = interleave(torch, sides, rounds, reps, warmup)
            med = report(emit, times, sides)
            a, b = med[sides[0][0]], med[sides[1][0]]
            mid = statistics.median(times[sides[0][0]] + times[sides[1][0]])
            emit(f"  {mix}: {call}_wide A/A medians differ by {abs(a - b) * 1e3:.1f} us ({(max(a, b) / min(a, b) - 1) * 100:.2f} %); "
                 f"yardstick (median of both) {mid * 1e3:.1f} us")
            for name in legs:
                emit(f"    {call}_ptrs_wide, {name}: {med[f'{mix}: {call}_ptrs_wide, {name}'] / mid:.3f} x the contiguous call")


def run_narrow(shape, rounds, reps, warmup, emit):
    import torch

    import quicknet_amd as qa
    from quicknet_amd.synth import erasure_marks, marks_to_rs_layout

    k, m, B, pitch, G = (int(x, 0) for x in shape.split(","))
    n = k + m
    dev, code, data, par = batch(torch, qa, k, m, B, pitch, G)
    drows, prows = data.view(G * k, pitch), par.view(G * m, pitch)
    marks_h = marks_to_rs_layout(erasure_marks(0x5EED0003, G, n, m), k)
    marks = torch.from_numpy(marks_h).to(dev)
    hit_d = torch.from_numpy(marks_h[:G * k] == 1).to(dev)
    s = Scattered(torch, dev, G * n, B, (B + 127) // 128 * 128, 0, 0x5EED0011)
    for call in (code.reconstruct_ptrs, code.reconstruct_ptrs_wide):
        s.put(0, drows)
        s.put(G * k, prows)
        s.rows2d[s.perm[:G * k][hit_d], :B] = 0x5A
        call(s.table, marks, B)
        assert torch.equal(s.get(0, G * k), drows[:, :B]) and torch.equal(s.get(G * k, G * m), prows[:, :B])
    sides = [("reconstruct_ptrs (A)", lambda: code.reconstruct_ptrs(s.table, marks, B)),
             ("reconstruct_ptrs (B)", lambda: code.reconstruct_ptrs(s.table, marks, B)),
             ("reconstruct_ptrs_wide", lambda: code.reconstruct_ptrs_wide(s.table, marks, B))]
    emit(f"narrow RS({k},{m}) B={B} G={G}, {m} erasures per group, permuted aligned pool: {rounds} interleaved rounds x {reps} calls")
    times = interleave(torch, sides, rounds, reps, warmup)
    med = report(emit, times, sides)
    mid = statistics.median(times[sides[0][0]] + times[sides[1][0]])
    a, b = med[sides[0][0]], med[sides[1][0]]
    emit(f"  reconstruct_ptrs A/A medians differ by {abs(a - b) * 1e3:.1f} us ({(max(a, b) / min(a, b) - 1) * 100:.2f} %); "
         f"reconstruct_ptrs_wide = {med[sides[2][0]] / mid:.3f} x reconstruct_ptrs")


def run_rs(shape, wide, emit):
    """reed_solomon_reconstruct on all-device scattered rows at rs_dev_ptrs = 1, wall clock, one call."""
    import numpy as np
    import torch

    import quicknet_amd as qa
    from quicknet_amd.synth import erasure_marks, marks_to_rs_layout

    k, m, B, G = (int(x, 0) for x in shape.split(","))
    n = k + m
    dev = torch.device("cuda:0")
    qa.tune("rs_dev_ptrs", 1)
    qa.tune("rs_dev_ptrs_wide", wide)
    s = Scattered(torch, dev, G * n, B, (B + 127) // 128 * 128, 0, 0x5EED0021)
    data = torch.empty((G * k, B), dtype=torch.uint8, device=dev)
    qa.synth_fill(data, 0x5EED0022)
    s.put(0, data)
    par = torch.empty((G, m, B), dtype=torch.uint8, device=dev)
    qa.Code.cauchy(k, m).encode(data.view(G, k, B), par, B)
    s.put(G * k, par.view(G * m, B))
    arr = (C.c_void_p * (G * n))(*s.table.cpu().numpy().tolist())
    rs = qa.ReedSolomon(k, m)
    marks = marks_to_rs_layout(erasure_marks(0x5EED0023, G, n, min(m, 4)), k)
    erased = torch.from_numpy(marks[:G * k] == 1).to(dev)
    s.rows2d[s.perm[:G * k][erased], :B] = 0x5A
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = qa.lib().reed_solomon_reconstruct(rs._h, arr, C.c_void_p(np.ascontiguousarray(marks).ctypes.data), G * n, B)
    t1 = time.perf_counter()
    assert rc == 0 and torch.equal(s.get(0, G * k), data), "rs reconstruct did not restore the data"
    emit(f"module/rs.h, RS({k},{m}) B={B} G={G}, all-device scattered rows, rs_dev_ptrs=1 rs_dev_ptrs_wide={wide}: "
         f"reed_solomon_reconstruct {(t1 - t0) * 1e3:.1f} ms (wall clock, first call)")
    rs.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append", help="wide code k,m,B,pitch,G (repeatable); default: " + " and ".join(SHAPES))
    p.add_argument("--narrow", action="append", help="narrow code k,m,B,pitch,G (repeatable); default: " + " and ".join(NARROW))
    p.add_argument("--rs", help="k,m,B,G: time module/rs.h instead")
    p.add_argument("--rs-wide", type=int, choices=[0, 1], default=1)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--profile", action="store_true", help="only the reconstruct on the random mix, for a kernel trace")
    p.add_argument("--out", default="", help="also append the report to this file")
    a = p.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    import torch

    import quicknet_amd as qa

    emit(f"{qa.lib().qfec_version().decode()} on {torch.cuda.get_device_name(0)}")
    if a.rs:
        run_rs(a.rs, a.rs_wide, emit)
    else:
        for shape in a.shape or SHAPES:
            run_wide(shape, a.rounds, a.reps, a.warmup, a.profile, emit)
        if not a.profile:
            for shape in a.narrow or ([] if a.shape else NARROW):
                run_narrow(shape, a.rounds, a.reps, a.warmup, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
