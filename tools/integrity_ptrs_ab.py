#!/usr/bin/env python3
"""Interleaved timing, in ONE process, of the integrity family on pointer tables (qfec_verify_ptrs /
qfec_locate_ptrs / qfec_scrub_ptrs) against the contiguous calls on the same bytes:

  qfec_verify / qfec_locate / qfec_scrub on the contiguous batch, twice (A/A: the yardstick and its spread)
  *_ptrs, the table pointing at those same rows in order (every row 16-B aligned)
  *_ptrs, the rows permuted at random inside one pool, slot pitch = B rounded up to 128

on two batches: a consistent one, and one with a single damaged shard (one byte) in 1 % of the groups.
qfec_encode against qfec_encode_ptrs is timed in the same run, on the consistent batch: the same
change of mapping on the same traffic less the parity stores, so its ratio is the yardstick the
verify ratio is read against.

Every round times each leg (a device event pair around every call, `reps` calls, warm-up first) in an
order drawn anew every round.  The damage is an XOR, put in and taken out again outside the timed
span; a scrub repairs its batch, so the damage goes back in before every scrub call.  Before anything
is timed every leg's output is checked: verify bits and culprits of the three layouts agree with each
other and with how the damage was made, and a scrub brings back the original bytes.  Each *_ptrs leg
is stated as a ratio to the contiguous call's A/A median of the same run and batch.

  python tools/integrity_ptrs_ab.py [--shape 10,3,1024,1024,100000] [--rounds 15] [--reps 5] [--out FILE]
"""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ptrs_ab import PEAK, SHAPES, Scattered  # noqa: E402

CALLS = ("verify", "locate", "scrub")


def run(shape, rounds, reps, warmup, emit):
    import torch

    import quicknet_amd as qa

    k, m, B, pitch, G = (int(x, 0) for x in shape.split(","))
    n = k + m
    dev = torch.device("cuda:0")
    code = qa.Code.cauchy(k, m)
    data = torch.empty((G, k, pitch), dtype=torch.uint8, device=dev)
    qa.synth_fill(data, 0x5EED0002)
    par = torch.empty((G, m, pitch), dtype=torch.uint8, device=dev)
    code.encode(data, par, B)
    drows, prows = data.view(G * k, pitch), par.view(G * m, pitch)
    base = torch.arange(G * k, device=dev, dtype=torch.int64) * pitch + data.data_ptr()
    pbase = torch.arange(G * m, device=dev, dtype=torch.int64) * pitch + par.data_ptr()
    inorder = torch.cat([base, pbase]).contiguous()
    r128 = (B + 127) // 128 * 128
    pool = Scattered(torch, dev, G * n, B, r128, 0, 0x5EED0011)
    pool.put(0, drows)
    pool.put(G * k, prows)
    tables = {"in order": inorder, "permuted, slot pitch %d" % r128: pool.table}

    # ---- the damage: one byte of one shard in 1 % of the groups, as an XOR (its own inverse)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0x5EED0031)
    hurt = torch.randperm(G, generator=gen)[:max(1, G // 100)].sort().values
    shard = torch.randint(0, n, hurt.shape, generator=gen)
    byte = torch.randint(0, B, hurt.shape, generator=gen).to(dev)
    val = torch.randint(1, 256, hurt.shape, generator=gen).to(torch.uint8).to(dev)
    rid = torch.where(shard < k, hurt * k + shard, G * k + hurt * m + (shard - k)).to(dev)  # rs.c row id
    is_d = (shard < k).to(dev)
    d_rid, d_byte, d_val = rid[is_d], byte[is_d], val[is_d]
    p_rid, p_byte, p_val = rid[~is_d] - G * k, byte[~is_d], val[~is_d]
    slot = pool.perm[rid]
    expect = torch.full((G,), -1, dtype=torch.int32)
    expect[hurt] = shard.to(torch.int32)
    expect = expect.to(dev)

    def toggle_rows():
        drows[d_rid, d_byte] ^= d_val
        prows[p_rid, p_byte] ^= p_val

    def toggle_pool():
        pool.rows2d[slot, byte] ^= val

    # ---- outputs, one set per leg family so that no leg waits for another's
    rows_w = torch.empty(G, dtype=torch.int32, device=dev)
    culprit = torch.empty(G, dtype=torch.int32, device=dev)

    def contiguous(call):
        if call == "verify":
            return lambda: code.verify(data, par, B, bad_rows=rows_w)
        if call == "locate":
            return lambda: code.locate(data, par, B, culprit=culprit)
        return lambda: code.scrub(data, par, B, culprit=culprit)

    def on_table(call, t):
        if call == "verify":
            return lambda: code.verify_ptrs(t, B, bad_rows=rows_w)
        if call == "locate":
            return lambda: code.locate_ptrs(t, B, culprit=culprit)
        return lambda: code.scrub_ptrs(t, B, culprit=culprit)

    # ---- every leg is right before it is timed
    keep = par.clone()
    for name, t in tables.items():
        if name == "in order":
            par.zero_()
        code.encode_ptrs(t, B)
    assert torch.equal(par[..., :B], keep[..., :B]) and torch.equal(pool.get(G * k, G * m), prows[:, :B]), "encode_ptrs differs from qfec_encode"
    del keep
    for damaged in (False, True):
        if damaged:
            toggle_rows()
            toggle_pool()
        want_c = expect if damaged else torch.full_like(expect, -1)
        ref_rows = code.verify(data, par, B).clone()
        assert torch.equal(ref_rows != 0, want_c >= 0), "qfec_verify disagrees with the damage"
        assert torch.equal(code.locate(data, par, B), want_c), "qfec_locate disagrees with the damage"
        for name, t in tables.items():
            assert torch.equal(code.verify_ptrs(t, B), ref_rows), f"verify_ptrs, {name}: bits differ from qfec_verify"
            assert torch.equal(code.locate_ptrs(t, B), want_c), f"locate_ptrs, {name}: culprits differ"
    clean_d, clean_p = drows[d_rid, d_byte] ^ d_val, prows[p_rid, p_byte] ^ p_val
    clean_pool = pool.rows2d[slot, byte] ^ val
    for which, fn in [("qfec_scrub", contiguous("scrub"))] + [(f"scrub_ptrs, {nm}", on_table("scrub", t)) for nm, t in tables.items()]:
        fn()  # the in-order table names the contiguous rows, so the damage goes back in for it
        assert torch.equal(culprit, expect), f"{which}: culprits differ"
        if which.endswith("slot pitch %d" % r128):
            assert torch.equal(pool.rows2d[slot, byte], clean_pool), f"{which}: bytes not restored"
            assert not code.verify_ptrs(pool.table, B).any(), f"{which}: the pool is not consistent"
        else:
            assert torch.equal(drows[d_rid, d_byte], clean_d) and torch.equal(prows[p_rid, p_byte], clean_p), f"{which}: bytes not restored"
            assert not code.verify(data, par, B).any(), f"{which}: the batch is not consistent"
            if which == "qfec_scrub":
                toggle_rows()
    torch.cuda.synchronize()  # both layouts are consistent again

    nbytes, tab_bytes = n * B * G, 8 * n * G
    noop = lambda: None
    # (name, bytes, fn, before a round's calls, before each call, after a round's calls)
    sides = [("encode (A)", nbytes, lambda: code.encode(data, par, B), noop, noop, noop),
             ("encode (B)", nbytes, lambda: code.encode(data, par, B), noop, noop, noop)]
    for name, t in tables.items():
        sides.append((f"encode_ptrs, {name}", nbytes + tab_bytes, lambda t=t: code.encode_ptrs(t, B), noop, noop, noop))
    for batch in ("consistent", "1 % damaged"):
        hurt_it = batch != "consistent"
        for call in CALLS:
            each = hurt_it and call == "scrub"   # a scrub takes the damage out: it goes back in before every call
            around = hurt_it and not each
            for ab in "AB":
                sides.append((f"{call} ({ab}), {batch}", nbytes, contiguous(call), toggle_rows if around else noop,
                              toggle_rows if each else noop, toggle_rows if around else noop))
            for name, t in tables.items():
                tg = toggle_rows if name == "in order" else toggle_pool
                sides.append((f"{call}_ptrs, {name}, {batch}", nbytes + tab_bytes, on_table(call, t), tg if around else noop,
                              tg if each else noop, tg if around else noop))
    s0 = torch.cuda.current_stream()

    def timed(side, count):
        _, _, fn, before, each, after = side
        before()
        total = 0.0
        pairs = []
        for _ in range(count):
            each()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s0)
            fn()
            e1.record(s0)
            pairs.append((e0, e1))
        after()
        torch.cuda.synchronize()
        for e0, e1 in pairs:
            total += e0.elapsed_time(e1)
        return total / count

    for side in sides:
        timed(side, warmup)
    times = {side[0]: [] for side in sides}
    order = random.Random(0x5EED0008)
    for _ in range(rounds):
        for side in order.sample(sides, len(sides)):
            times[side[0]].append(timed(side, reps))
    assert not code.verify(data, par, B).any() and not code.verify_ptrs(pool.table, B).any(), "a leg left damage behind"

    emit(f"RS({k},{m}) B={B} pitch={pitch} G={G}, {hurt.numel()} damaged groups in the damaged batch: "
         f"{rounds} interleaved rounds x {reps} calls, a device event pair per call")
    med = {}
    for name, nb, *_ in sides:
        med[name] = statistics.median(times[name])
        rate = nb / (med[name] * 1e-3)
        emit(f"  {name:58s} median {med[name] * 1e3:9.1f} us  min {min(times[name]) * 1e3:9.1f} us  "
             f"max {max(times[name]) * 1e3:9.1f} us  {rate / 1e9:7.1f} GB/s = {rate / PEAK:5.3f} of 8 TB/s")

    def ratios(call, suffix):
        a, b = med[f"{call} (A){suffix}"], med[f"{call} (B){suffix}"]
        mid = statistics.median(times[f"{call} (A){suffix}"] + times[f"{call} (B){suffix}"])
        emit(f"  {call}{suffix} A/A: medians differ by {abs(a - b) * 1e3:.1f} us ({(max(a, b) / min(a, b) - 1) * 100:.2f} %); "
             f"yardstick (median of both) {mid * 1e3:.1f} us")
        for name in tables:
            emit(f"    {call}_ptrs, {name}{suffix}: {med[f'{call}_ptrs, {name}{suffix}'] / mid:.3f} x the contiguous {call}")

    ratios("encode", "")
    for batch in ("consistent", "1 % damaged"):
        for call in CALLS:
            ratios(call, f", {batch}")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append", help="k,m,B,pitch,G (repeatable); default: " + " and ".join(SHAPES))
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
    for shape in a.shape or SHAPES:
        run(shape, a.rounds, a.reps, a.warmup, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
