#!/usr/bin/env python3
"""Interleaved timing, in ONE process on the same buffers, of qfec_locate_wide (check plans built on
the device, any k + m):

  narrow codes  against qfec_locate_erased (host-built records behind a LUT, compiled (k, m)
                instances) on the same batch, with no marks and with one lost shard per group:
                  locate_erased (A) and (B), locate_wide
  wide codes    where nothing else locates: a consistent batch, 1 % of the groups corrupted and
                every group corrupted (one byte of one surviving shard), each with 0 and 4 lost
                shards per group:
                  locate_wide (A) and (B)

Each timed call runs from the call to a stream synchronise on a host clock (both calls are
asynchronous once qfec_locate_erased's tables exist), one call per timing, and the order within a
round is drawn anew every round.  (A) and (B) are the same side twice: their difference is the
spread.  Before anything is timed the verdicts are checked against how the damage was made, and on
narrow codes the two calls' verdicts, marks and counts against each other.  The apply kernel's
algorithmic bytes, (k + m - t) x B per group plus the plan bytes, are printed for the kernel trace
(--profile CASE runs only qfec_locate_wide on one case, five times, for `rocprofv3 --kernel-trace
--stats -- python tools/locate_wide_ab.py --shape ... --profile clean0`).

  python tools/locate_wide_ab.py [--shape 32,8,1024,1024,20000] [--rounds 7] [--out FILE]
                                 [--profile clean0|clean4|one0|one4|all0|all4]
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
NARROW = ["10,3,1024,1024,100000", "16,4,1400,1408,250000"]  # k, m, B, pitch, G
WIDE = ["32,8,1024,1024,20000", "64,16,1024,1024,20000"]
CLEAN = -1


def batch(shape):
    import torch

    import quicknet_amd as qa

    k, m, B, pitch, G = (int(x, 0) for x in shape.split(","))
    dev = torch.device("cuda:0")
    code = qa.Code.cauchy(k, m)
    data = torch.empty((G, k, pitch), dtype=torch.uint8, device=dev)
    qa.synth_fill(data, 0x5EED0002)
    par = torch.empty((G, m, pitch), dtype=torch.uint8, device=dev)
    code.encode(data, par, B)
    torch.cuda.synchronize()
    return code, data, par, (k, m, B, pitch, G)


def make_case(code, data, par, dims, lost, frac, seed):
    """(data, parity, marks on the device, expected culprits): `lost` marked shards per group and one
    byte flipped in one surviving shard of a fraction `frac` of the groups."""
    import numpy as np
    import torch

    from quicknet_amd.synth import erasure_marks, marks_to_rs_layout

    k, m, B, pitch, G = dims
    n = k + m
    rng = np.random.default_rng(seed)
    gm = erasure_marks(seed, G, n, lost) if lost else np.zeros((G, n), np.uint8)
    expect = np.full(G, CLEAN, np.int32)
    hit = np.nonzero(rng.random(G) < frac)[0] if frac < 1 else np.arange(G)
    d, p = data.clone(), par.clone()
    dg, dc, pg, pc, db, pb = [], [], [], [], [], []
    for g in hit:
        c = int(rng.integers(0, n))
        while gm[g, c]:
            c = (c + 1) % n
        expect[g] = c
        b = int(rng.integers(0, B))
        if c < k:
            dg.append(g); dc.append(c); db.append(b)
        else:
            pg.append(g); pc.append(c - k); pb.append(b)
    dev = data.device
    if dg:
        d[torch.tensor(dg, device=dev), torch.tensor(dc, device=dev), torch.tensor(db, device=dev)] ^= 0x5A
    if pg:
        p[torch.tensor(pg, device=dev), torch.tensor(pc, device=dev), torch.tensor(pb, device=dev)] ^= 0x5A
    marks = torch.from_numpy(marks_to_rs_layout(gm, k)).to(dev)
    return d, p, marks, expect


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def interleave(sides, rounds, emit, seed):
    import torch

    for _, fn in sides:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in sides}
    order = random.Random(seed)
    for _ in range(rounds):
        for name, fn in order.sample(sides, len(sides)):
            times[name].append(timed(fn))
    med = {}
    for name, _ in sides:
        med[name] = statistics.median(times[name])
        emit(f"  {name:44s} median {med[name]:9.3f} ms  min {min(times[name]):9.3f} ms  max {max(times[name]):9.3f} ms")
    return med


def outputs(G, n, dev):
    import torch

    return (torch.empty(G, dtype=torch.int32, device=dev), torch.empty(G * n, dtype=torch.uint8, device=dev),
            torch.zeros(5, dtype=torch.int32, device=dev))


def run_narrow(shape, rounds, emit):
    import numpy as np
    import torch

    code, data, par, dims = batch(shape)
    k, m, B, pitch, G = dims
    n = k + m
    code.prepare_locate_erased()
    emit(f"RS({k},{m}) B={B} pitch={pitch} G={G}: qfec_locate_erased against qfec_locate_wide, check plan stride "
         f"{code.check_stride()} B")
    for lost in (0, 1):
        d, p, marks, expect = make_case(code, data, par, dims, lost, 0.01, 0x5EED0100 + lost)
        c1, o1, n1 = outputs(G, n, data.device)
        c2, o2, n2 = outputs(G, n, data.device)
        code.locate_erased(d, p, marks, B, culprit=c1, marks_out=o1, counts=n1)
        code.locate_wide(d, p, marks, B, culprit=c2, marks_out=o2, counts=n2)
        torch.cuda.synchronize()
        assert np.array_equal(c1.cpu().numpy(), expect)
        assert torch.equal(c1, c2) and torch.equal(o1, o2) and torch.equal(n1, n2)
        emit(f" {lost} lost per group, 1 % of the groups corrupted, {rounds} interleaved rounds")
        sides = [("locate_erased (A)", lambda: code.locate_erased(d, p, marks, B, culprit=c1)),
                 ("locate_erased (B)", lambda: code.locate_erased(d, p, marks, B, culprit=c1)),
                 ("locate_wide", lambda: code.locate_wide(d, p, marks, B, culprit=c2))]
        med = interleave(sides, rounds, emit, 0x5EED0008 + lost)
        lo, hi = sorted((med[sides[0][0]], med[sides[1][0]]))
        emit(f"  A/A medians differ by {hi - lo:.3f} ms ({(hi / lo - 1) * 100:.1f} %); locate_wide / locate_erased = "
             f"{med['locate_wide'] / hi:.2f} .. {med['locate_wide'] / lo:.2f}")


CASES = {"clean": 0.0, "one": 0.01, "all": 1.0}


def run_wide(shape, rounds, profile, emit):
    import numpy as np
    import torch

    code, data, par, dims = batch(shape)
    k, m, B, pitch, G = dims
    n = k + m
    emit(f"RS({k},{m}) B={B} pitch={pitch} G={G}: qfec_locate_wide, check plan stride {code.check_stride()} B")
    for lost in (0, 4):
        nbytes = (n - lost) * B * G + G * code.check_stride()
        emit(f" {lost} lost per group: k_check_apply algorithmic bytes {nbytes / 1e6:.1f} MB = {nbytes / PEAK * 1e6:.1f} us at 8 TB/s")
        for name, frac in CASES.items():
            if profile and profile != f"{name}{lost}":
                continue
            d, p, marks, expect = make_case(code, data, par, dims, lost, frac, 0x5EED0200 + lost)
            c, o, cnt = outputs(G, n, data.device)
            code.locate_wide(d, p, marks, B, culprit=c, marks_out=o, counts=cnt)
            torch.cuda.synchronize()
            assert np.array_equal(c.cpu().numpy(), expect) and int(cnt[0]) == (expect >= 0).sum()
            if profile:
                for _ in range(5):
                    code.locate_wide(d, p, marks, B, culprit=c)
                torch.cuda.synchronize()
                return
            emit(f"  {name}: {(expect >= 0).sum()} of {G} groups corrupted, {rounds} interleaved rounds")
            sides = [("locate_wide (A)", lambda: code.locate_wide(d, p, marks, B, culprit=c)),
                     ("locate_wide (B)", lambda: code.locate_wide(d, p, marks, B, culprit=c))]
            med = interleave(sides, rounds, emit, 0x5EED0010 + lost)
            lo, hi = sorted(med.values())
            emit(f"   A/A medians differ by {hi - lo:.3f} ms ({(hi / lo - 1) * 100:.1f} %)")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append", help="k,m,B,pitch,G (repeatable; narrow when k + m <= 24); default: "
                   + " and ".join(NARROW + WIDE))
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--profile", choices=[f"{c}{t}" for c in CASES for t in (0, 4)],
                   help="run only qfec_locate_wide on this case of a wide shape, five times (for a kernel trace)")
    p.add_argument("--out", default="", help="also write the report to this file")
    a = p.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    import torch

    import quicknet_amd as qa

    emit(f"{qa.lib().qfec_version().decode()} on {torch.cuda.get_device_name(0)}")
    for shape in a.shape or NARROW + WIDE:
        k, m = (int(x, 0) for x in shape.split(",")[:2])
        if k + m <= 24 and not a.profile:
            run_narrow(shape, a.rounds, emit)
        else:
            run_wide(shape, a.rounds, a.profile, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
