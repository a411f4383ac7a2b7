#!/usr/bin/env python3
"""Interleaved timing, in ONE process, of the integrity calls on pointer tables with per-shard lengths
(qfec_verify_ptrs_var / qfec_locate_ptrs_var / qfec_scrub_ptrs_var) against the fixed-length
pointer-table calls (qfec_verify_ptrs / qfec_locate_ptrs / qfec_scrub_ptrs) on the same rows
zero-padded to max_len.  The rows lie in order in an aligned pool, slot pitch = max_len rounded up to
128; the parity is qfec_encode_ptrs' on the zero-padded rows.  Three settings of the lengths, as in
tools/ptrs_var_ab.py:

  full      all lengths = max_len: the price of the feature on full packets
  short10   one group in ten short: its last 1 .. k - 1 shards empty, the rest max_len
  drawn     every length drawn deterministically (quicknet_amd.synth) between 64 and max_len

and two batches per setting: consistent, and 1 % damaged (one byte of data shard 0 in every hundredth
group).  Per batch every round times, back to back and in an order drawn anew, each fixed-length call
twice (A/A: the yardstick and its spread), each new call, and the pair encode_ptrs / encode_ptrs_var
on a parity buffer of their own (what the same change of mapping costs the encode in this run), device
events around `reps` calls.  The scrubs are timed one call per event pair, the damage put back before
every call outside the events.  Before anything is timed every leg's output is checked: the verify
words and the verdicts of both families agree with each other and with how the damage was made, both
scrubs bring the data back byte for byte.  Each new leg is stated as a ratio to the fixed-length A/A
median of the same run, beside the byte ratio (sum len + m * sum L) / ((k + m) * max_len * G).

  python tools/integrity_ptrs_var_ab.py [--shape 10,3,1024,100000] [--rounds 15] [--reps 5] [--out FILE]
"""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ptrs_var_ab import SHAPES, lengths  # noqa: E402

CLEAN = -1


def run(shape, setting, damaged, rounds, reps, warmup, emit):
    import numpy as np
    import torch

    import quicknet_amd as qa

    k, m, max_len, G = (int(x, 0) for x in shape.split(","))
    n = k + m
    pitch = (max_len + 127) // 128 * 128
    dev = torch.device("cuda:0")
    code = qa.Code.cauchy(k, m)
    lens_h = lengths(setting, k, max_len, G)
    L_h = lens_h.max(1)
    assert (lens_h[:, 0] >= 4).all()  # the damage lands inside shard 0
    lens = torch.from_numpy(lens_h.astype(np.int32).reshape(-1)).to(dev)
    glen = torch.from_numpy(L_h.astype(np.int32)).to(dev)
    cols = torch.arange(pitch, device=dev, dtype=torch.int32)

    data = torch.empty((G * k, pitch), dtype=torch.uint8, device=dev)
    qa.synth_fill(data, 0x5EED0002)
    step = 1 << 18
    for i in range(0, G * k, step):  # rows zero-padded: what the fixed-length calls need
        data[i:i + step] *= (cols[None, :] < lens[i:i + step, None]).to(torch.uint8)
    par = torch.zeros((G * m, pitch), dtype=torch.uint8, device=dev)
    par_e = torch.zeros((G * m, pitch), dtype=torch.uint8, device=dev)  # the encode pair writes here

    def table(p):
        d = torch.arange(G * k, device=dev, dtype=torch.int64) * pitch + data.data_ptr()
        q = torch.arange(G * m, device=dev, dtype=torch.int64) * pitch + p.data_ptr()
        return torch.cat([d, q]).contiguous()

    tab, tab_e = table(par), table(par_e)
    assert data.data_ptr() % 16 == 0 and par.data_ptr() % 16 == 0 and par_e.data_ptr() % 16 == 0
    code.encode_ptrs(tab, max_len)
    hurt = torch.arange(0, G, 100, device=dev, dtype=torch.int64) if damaged else torch.zeros(0, dtype=torch.int64, device=dev)
    keep = data[hurt * k, 3].clone()

    def damage():
        data[hurt * k, 3] = keep ^ 0x5A

    damage()
    expect = torch.full((G,), CLEAN, dtype=torch.int32, device=dev)
    expect[hurt] = 0

    # ---- every leg is right before it is timed
    cf, cv, inv = (torch.zeros(3, dtype=torch.int32, device=dev) for _ in range(3))
    rows_f = code.verify_ptrs(tab, max_len, bad_groups=cf[:1])
    rows_v = code.verify_ptrs_var(tab, lens, glen, max_len, bad_groups=cv[:1], invalid=inv[:1])
    assert torch.equal(rows_f, rows_v) and int(cf[0]) == int(cv[0]) == len(hurt) and int(inv[0]) == 0, f"{setting}: verify"
    assert torch.equal(rows_v != 0, expect >= 0)
    cf.zero_(), cv.zero_()
    cul_f = code.locate_ptrs(tab, max_len, counts=cf)
    cul_v = code.locate_ptrs_var(tab, lens, glen, max_len, counts=cv, invalid=inv[:1])
    assert torch.equal(cul_f, expect) and torch.equal(cul_v, expect) and torch.equal(cf, cv) and int(inv[0]) == 0, \
        f"{setting}: locate"
    good = data.clone()
    good[hurt * k, 3] = keep
    for name, call in (("scrub_ptrs", lambda: code.scrub_ptrs(tab, max_len)),
                       ("scrub_ptrs_var", lambda: code.scrub_ptrs_var(tab, lens, glen, max_len))):
        damage()
        assert torch.equal(call(), expect) and torch.equal(data, good), f"{setting}: {name} did not restore the data"
    del good
    damage()

    glen_out = torch.empty_like(glen)
    sides = [("verify_ptrs (A)", lambda: code.verify_ptrs(tab, max_len, bad_rows=rows_f)),
             ("verify_ptrs (B)", lambda: code.verify_ptrs(tab, max_len, bad_rows=rows_f)),
             ("verify_ptrs_var", lambda: code.verify_ptrs_var(tab, lens, glen, max_len, bad_rows=rows_v)),
             ("locate_ptrs (A)", lambda: code.locate_ptrs(tab, max_len, culprit=cul_f)),
             ("locate_ptrs (B)", lambda: code.locate_ptrs(tab, max_len, culprit=cul_f)),
             ("locate_ptrs_var", lambda: code.locate_ptrs_var(tab, lens, glen, max_len, culprit=cul_v)),
             ("scrub_ptrs (A)", lambda: code.scrub_ptrs(tab, max_len, culprit=cul_f)),
             ("scrub_ptrs (B)", lambda: code.scrub_ptrs(tab, max_len, culprit=cul_f)),
             ("scrub_ptrs_var", lambda: code.scrub_ptrs_var(tab, lens, glen, max_len, culprit=cul_v)),
             ("encode_ptrs (A)", lambda: code.encode_ptrs(tab_e, max_len)),
             ("encode_ptrs (B)", lambda: code.encode_ptrs(tab_e, max_len)),
             ("encode_ptrs_var", lambda: code.encode_ptrs_var(tab_e, lens, max_len, glen_out))]
    s0 = torch.cuda.current_stream()
    for name, fn in sides:
        for _ in range(warmup):
            if name.startswith("scrub"):
                damage()
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in sides}
    order = random.Random(0x5EED0008)
    for _ in range(rounds):
        for name, fn in order.sample(sides, len(sides)):
            total = 0.0
            if name.startswith("scrub"):  # one call per event pair, the damage put back outside it
                for _ in range(reps):
                    damage()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s0)
                    fn()
                    e1.record(s0)
                    torch.cuda.synchronize()
                    total += e0.elapsed_time(e1)
                damage()
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s0)
                for _ in range(reps):
                    fn()
                e1.record(s0)
                torch.cuda.synchronize()
                total = e0.elapsed_time(e1)
            times[name].append(total / reps)
    byte_ratio = (int(lens_h.sum()) + m * int(L_h.sum())) / (n * max_len * G)
    emit(f"RS({k},{m}) max_len={max_len} G={G} lengths={setting} batch={'1 % damaged' if damaged else 'consistent'}: "
         f"byte ratio {byte_ratio:.3f}; {rounds} interleaved rounds x {reps} calls, device events")
    med = {}
    for name, _ in sides:
        med[name] = statistics.median(times[name])
        emit(f"  {name:20s} median {med[name] * 1e3:9.1f} us  min {min(times[name]) * 1e3:9.1f} us  max {max(times[name]) * 1e3:9.1f} us")
    for call in ("verify_ptrs", "locate_ptrs", "scrub_ptrs", "encode_ptrs"):
        a, b = med[f"{call} (A)"], med[f"{call} (B)"]
        mid = statistics.median(times[f"{call} (A)"] + times[f"{call} (B)"])
        emit(f"  {call} A/A: medians differ by {abs(a - b) * 1e3:.1f} us ({(max(a, b) / min(a, b) - 1) * 100:.2f} %); "
             f"yardstick (median of both) {mid * 1e3:.1f} us")
        emit(f"    {call}_var, lengths={setting}: {med[call + '_var'] / mid:.3f} x the fixed-length {call} at max_len "
             f"(byte ratio {byte_ratio:.3f})")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append", help="k,m,max_len,G (repeatable); default: " + " and ".join(SHAPES))
    p.add_argument("--setting", action="append", choices=["full", "short10", "drawn"], help="default: all three")
    p.add_argument("--batch", action="append", choices=["consistent", "damaged"], help="default: both")
    p.add_argument("--rounds", type=int, default=15)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default="", help="also write the report to this file")
    a = p.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
        if a.out:  # kept up to date: a run cut short leaves what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    import torch

    import quicknet_amd as qa

    emit(f"{qa.lib().qfec_version().decode()} on {torch.cuda.get_device_name(0)}")
    for shape in a.shape or SHAPES:
        for setting in a.setting or ["full", "short10", "drawn"]:
            for batch in a.batch or ["consistent", "damaged"]:
                run(shape, setting, batch == "damaged", a.rounds, a.reps, a.warmup, emit)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
