#!/usr/bin/env python3
"""Interleaved timing, in ONE process, of the pointer-table calls (qfec_encode_ptrs /
qfec_reconstruct_ptrs) against the contiguous calls on the same bytes:

  qfec_encode / qfec_reconstruct on the contiguous batch, twice (A/A: the yardstick and its spread)
  *_ptrs, the table pointing at those same rows in order: the price of the indirection and of the
      one-wave-per-(group, slab) mapping alone
  *_ptrs, the rows permuted at random inside one pool, slot pitch = B rounded up to 128: the price
      of scatter
  *_ptrs, permuted likewise, slot pitch = B rounded up to 16, + 16, every row 8 bytes into its slot:
      every row is misaligned, so every group runs the byte body

Every round times each leg back to back (device events around `reps` calls, warm-up first), in an
order drawn anew every round.  Before anything is timed every leg's output is checked: the parity
the encode legs write equals the contiguous encode's, and the reconstruct legs bring back the
original data from m erasures per group.  Each *_ptrs leg is stated as a ratio to the contiguous A/A
median of the same run.  Bytes: the (k + m) rows of a group for the encode, k survivors read and e
rows written for the reconstruct, plus 8 bytes per table entry on the *_ptrs legs.

  python tools/ptrs_ab.py [--shape 10,3,1024,1024,100000] [--rounds 15] [--reps 5] [--out FILE]

Separately, module/rs.h end to end on all-device scattered rows, wall clock, one setting of the knob
rs_dev_ptrs per process (at 0 the staged branch issues one copy per row):

  python tools/ptrs_ab.py --rs-knob 0|1 [--rs-shape 10,3,1024,20000] [--out FILE]   (appends)
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

PEAK = 8.0e12  # MI355X HBM3E, bytes per second
SHAPES = ["10,3,1024,1024,100000", "16,4,1400,1408,250000"]  # k, m, B, pitch, G


class Scattered:
    """All G * (k + m) rows of a batch at random slots of one pool; row i is rs.c's shard i."""

    def __init__(self, torch, dev, nrows, B, slot, lead, seed):
        g = torch.Generator(device="cpu")
        g.manual_seed(seed)
        self.perm = torch.randperm(nrows, generator=g).to(dev)
        self.pool = torch.zeros(nrows * slot + 16, dtype=torch.uint8, device=dev)
        self.rows2d = self.pool[:nrows * slot].view(nrows, slot)
        self.B, self.lead = B, lead
        assert self.pool.data_ptr() % 16 == 0
        self.table = (self.perm * slot + (self.pool.data_ptr() + lead)).contiguous()

    def put(self, first, rows, step=1 << 18):  # rows [r, >= B] -> rows first .. first + r - 1
        for i in range(0, rows.shape[0], step):
            j = min(i + step, rows.shape[0])
            self.rows2d[self.perm[first + i:first + j], self.lead:self.lead + self.B] = rows[i:j, :self.B]

    def get(self, first, count, step=1 << 18):
        import torch
        return torch.cat([self.rows2d[self.perm[first + i:min(first + i + step, first + count)], self.lead:self.lead + self.B]
                          for i in range(0, count, step)])


def run(shape, rounds, reps, warmup, emit):
    import torch

    import quicknet_amd as qa
    from quicknet_amd.synth import erasure_marks, marks_to_rs_layout

    k, m, B, pitch, G = (int(x, 0) for x in shape.split(","))
    n = k + m
    dev = torch.device("cuda:0")
    code = qa.Code.cauchy(k, m)
    data = torch.empty((G, k, pitch), dtype=torch.uint8, device=dev)
    qa.synth_fill(data, 0x5EED0002)
    par = torch.empty((G, m, pitch), dtype=torch.uint8, device=dev)
    code.encode(data, par, B)
    gm = erasure_marks(0x5EED0003, G, n, m)
    marks_h = marks_to_rs_layout(gm, k)
    marks = torch.from_numpy(marks_h).to(dev)
    erased = torch.from_numpy(marks_h[:G * k] == 1).to(dev)
    e_rows = int(erased.sum().item())
    drows, prows = data.view(G * k, pitch), par.view(G * m, pitch)

    base = torch.arange(G * k, device=dev, dtype=torch.int64) * pitch + data.data_ptr()
    pbase = torch.arange(G * m, device=dev, dtype=torch.int64) * pitch + par.data_ptr()
    inorder = torch.cat([base, pbase]).contiguous()
    r128 = (B + 127) // 128 * 128
    legs = {"in order": None,
            "permuted, slot pitch %d" % r128: Scattered(torch, dev, G * n, B, r128, 0, 0x5EED0011),
            "permuted, misaligned": Scattered(torch, dev, G * n, B, (B + 15) // 16 * 16 + 16, 8, 0x5EED0012)}
    tables = {name: (inorder if s is None else s.table) for name, s in legs.items()}
    for s in legs.values():
        if s is not None:
            s.put(0, drows)
            assert s.table.min().item() % 16 == s.lead % 16

    # ---- every leg is right before it is timed
    for name, s in legs.items():
        if s is None:
            keep = par.clone()
            par.zero_()
            code.encode_ptrs(tables[name], B)
            assert torch.equal(par[..., :B], keep[..., :B]), f"encode_ptrs, {name}: parity differs from qfec_encode"
            hurt = data.clone()
            data.view(G * k, pitch)[erased, :B] = 0x5A
            code.reconstruct_ptrs(tables[name], marks, B)
            assert torch.equal(data[..., :B], hurt[..., :B]), f"reconstruct_ptrs, {name}: data not restored"
            del keep, hurt
        else:
            code.encode_ptrs(tables[name], B)
            assert torch.equal(s.get(G * k, G * m), prows[:, :B]), f"encode_ptrs, {name}: parity differs from qfec_encode"
            s.rows2d[s.perm[:G * k][erased], s.lead:s.lead + B] = 0x5A
            failed = torch.zeros(1, dtype=torch.int32, device=dev)
            code.reconstruct_ptrs(tables[name], marks, B, failed)
            assert int(failed.item()) == 0
            assert torch.equal(s.get(0, G * k), drows[:, :B]), f"reconstruct_ptrs, {name}: data not restored"
    wd = data.clone()  # the contiguous reconstruct's scratch copy
    wd.view(G * k, pitch)[erased, :B] = 0x5A
    code.reconstruct(wd, par, marks, B)
    assert torch.equal(wd[..., :B], data[..., :B])

    enc_bytes, rec_bytes, tab_bytes = n * B * G, k * B * G + e_rows * B, 8 * n * G
    sides = [("encode (A)", enc_bytes, lambda: code.encode(data, par, B)),
             ("encode (B)", enc_bytes, lambda: code.encode(data, par, B)),
             ("reconstruct (A)", rec_bytes, lambda: code.reconstruct(wd, par, marks, B)),
             ("reconstruct (B)", rec_bytes, lambda: code.reconstruct(wd, par, marks, B))]
    for name in legs:
        t = tables[name]
        sides.append((f"encode_ptrs, {name}", enc_bytes + tab_bytes, lambda t=t: code.encode_ptrs(t, B)))
        sides.append((f"reconstruct_ptrs, {name}", rec_bytes + tab_bytes, lambda t=t: code.reconstruct_ptrs(t, marks, B)))
    s0 = torch.cuda.current_stream()
    for _, _, fn in sides:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in sides}
    order = random.Random(0x5EED0008)
    for _ in range(rounds):
        for name, _, fn in order.sample(sides, len(sides)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s0)
            for _ in range(reps):
                fn()
            e1.record(s0)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps)
    emit(f"RS({k},{m}) B={B} pitch={pitch} G={G}, {m} erasures per group: {rounds} interleaved rounds x {reps} calls, device events")
    med = {}
    for name, nbytes, _ in sides:
        med[name] = statistics.median(times[name])
        rate = nbytes / (med[name] * 1e-3)
        emit(f"  {name:46s} median {med[name] * 1e3:9.1f} us  min {min(times[name]) * 1e3:9.1f} us  "
             f"max {max(times[name]) * 1e3:9.1f} us  {nbytes / 1e6:9.1f} MB  {rate / 1e9:7.1f} GB/s = {rate / PEAK:5.3f} of 8 TB/s")
    for call in ("encode", "reconstruct"):
        a, b = med[f"{call} (A)"], med[f"{call} (B)"]
        mid = statistics.median(times[f"{call} (A)"] + times[f"{call} (B)"])
        emit(f"  {call} A/A: medians differ by {abs(a - b) * 1e3:.1f} us ({(max(a, b) / min(a, b) - 1) * 100:.2f} %); "
             f"yardstick (median of both) {mid * 1e3:.1f} us")
        for name in legs:
            emit(f"    {call}_ptrs, {name}: {med[f'{call}_ptrs, {name}'] / mid:.3f} x the contiguous {call}")


def run_rs(shape, knob, emit):
    """reed_solomon_encode + reed_solomon_reconstruct on all-device scattered rows, wall clock."""
    import numpy as np
    import torch

    import quicknet_amd as qa
    from quicknet_amd.synth import erasure_marks, marks_to_rs_layout

    k, m, B, G = (int(x, 0) for x in shape.split(","))
    n = k + m
    dev = torch.device("cuda:0")
    qa.tune("rs_dev_ptrs", knob)
    s = Scattered(torch, dev, G * n, B, (B + 127) // 128 * 128, 0, 0x5EED0021)
    data = torch.empty((G * k, B), dtype=torch.uint8, device=dev)
    qa.synth_fill(data, 0x5EED0022)
    s.put(0, data)
    want = torch.empty((G, m, B), dtype=torch.uint8, device=dev)
    qa.Code.cauchy(k, m).encode(data.view(G, k, B), want, B)
    table = s.table.cpu().numpy()
    arr = (C.c_void_p * (G * n))(*table.tolist())
    rs = qa.ReedSolomon(k, m)
    L = qa.lib()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = L.reed_solomon_encode(rs._h, arr, G * n, B)
    t1 = time.perf_counter()
    assert rc == 0 and torch.equal(s.get(G * k, G * m), want.view(G * m, B)), "rs encode differs from qfec_encode"
    marks = marks_to_rs_layout(erasure_marks(0x5EED0023, G, n, m), k)
    erased = torch.from_numpy(marks[:G * k] == 1).to(dev)
    s.rows2d[s.perm[:G * k][erased], :B] = 0x5A
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    rc = L.reed_solomon_reconstruct(rs._h, arr, C.c_void_p(np.ascontiguousarray(marks).ctypes.data), G * n, B)
    t3 = time.perf_counter()
    assert rc == 0 and torch.equal(s.get(0, G * k), data), "rs reconstruct did not restore the data"
    emit(f"module/rs.h, RS({k},{m}) B={B} G={G}, all-device scattered rows, rs_dev_ptrs={knob}: "
         f"reed_solomon_encode {(t1 - t0) * 1e3:.1f} ms, reed_solomon_reconstruct {(t3 - t2) * 1e3:.1f} ms (wall clock, first call)")
    rs.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append", help="k,m,B,pitch,G (repeatable); default: " + " and ".join(SHAPES))
    p.add_argument("--rounds", type=int, default=15)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--rs-knob", type=int, choices=[0, 1], help="time module/rs.h at this rs_dev_ptrs instead")
    p.add_argument("--rs-shape", default="10,3,1024,20000", help="k,m,B,G")
    p.add_argument("--out", default="", help="also write the report to this file (--rs-knob: append)")
    a = p.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    import torch

    import quicknet_amd as qa

    if a.rs_knob is not None:
        run_rs(a.rs_shape, a.rs_knob, emit)
    else:
        emit(f"{qa.lib().qfec_version().decode()} on {torch.cuda.get_device_name(0)}")
        for shape in a.shape or SHAPES:
            run(shape, a.rounds, a.reps, a.warmup, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.rs_knob is not None else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
