#!/usr/bin/env python3
"""Interleaved timing, in ONE process, of the pointer-table calls with per-shard lengths
(qfec_encode_ptrs_var / qfec_reconstruct_ptrs_var) against the fixed-length pointer-table calls
(qfec_encode_ptrs / qfec_reconstruct_ptrs) on the same rows zero-padded to max_len.  The rows lie in
order in an aligned pool, slot pitch = max_len rounded up to 128.  Three settings of the lengths:

  full      all lengths = max_len: the price of the feature on full packets
  drawn     lengths drawn deterministically (quicknet_amd.synth) between 64 and max_len
  short10   one group in ten short: its last 1 .. k - 1 shards empty, the rest max_len

Per setting every round times, back to back and in an order drawn anew, the fixed-length encode and
reconstruct twice each (A/A: the yardstick and its spread) and the two new calls (device events around
`reps` calls, warm-up first).  Before anything is timed every leg's output is checked: the new encode's
parity equals the fixed call's in [0, L) and is untouched past L, d_group_len is right, and both
reconstructs bring back the zero-padded data from m erasures per group.  Each new leg is stated as a
ratio to the fixed-length A/A median of the same run, beside the byte ratio
(sum len + m * sum L) / ((k + m) * max_len * G).

  python tools/ptrs_var_ab.py [--shape 10,3,1024,100000] [--rounds 15] [--reps 5] [--out FILE]
"""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ["10,3,1024,100000", "16,4,1400,250000"]  # k, m, max_len, G
UNTOUCHED = 0xEE


def lengths(setting, k, max_len, G):
    import numpy as np

    from quicknet_amd.synth import splitmix_words

    lens = np.full((G, k), max_len, np.int64)
    if setting == "drawn":
        lo = min(64, max_len)
        lens = lo + (splitmix_words(0x5EED0031, G * k) % np.uint64(max_len - lo + 1)).astype(np.int64).reshape(G, k)
    elif setting == "short10":
        for g in range(0, G, 10):
            lens[g, k - (1 + (g // 10) % (k - 1)):] = 0
    return lens


def run(shape, setting, rounds, reps, warmup, emit):
    import numpy as np
    import torch

    import quicknet_amd as qa
    from quicknet_amd.synth import erasure_marks, marks_to_rs_layout

    k, m, max_len, G = (int(x, 0) for x in shape.split(","))
    n = k + m
    pitch = (max_len + 127) // 128 * 128
    dev = torch.device("cuda:0")
    code = qa.Code.cauchy(k, m)
    lens_h = lengths(setting, k, max_len, G)
    L_h = lens_h.max(1)
    lens = torch.from_numpy(lens_h.astype(np.int32).reshape(-1)).to(dev)
    L = torch.from_numpy(L_h.astype(np.int32)).to(dev)
    cols = torch.arange(pitch, device=dev, dtype=torch.int32)

    data = torch.empty((G * k, pitch), dtype=torch.uint8, device=dev)
    qa.synth_fill(data, 0x5EED0002)
    step = 1 << 18
    for i in range(0, G * k, step):  # rows zero-padded: what the fixed-length call needs, and the reference
        data[i:i + step] *= (cols[None, :] < lens[i:i + step, None]).to(torch.uint8)
    par_f = torch.zeros((G * m, pitch), dtype=torch.uint8, device=dev)
    par_v = torch.full((G * m, pitch), UNTOUCHED, dtype=torch.uint8, device=dev)

    def table(par):
        d = torch.arange(G * k, device=dev, dtype=torch.int64) * pitch + data.data_ptr()
        p = torch.arange(G * m, device=dev, dtype=torch.int64) * pitch + par.data_ptr()
        return torch.cat([d, p]).contiguous()

    tab_f, tab_v = table(par_f), table(par_v)
    assert data.data_ptr() % 16 == 0 and par_f.data_ptr() % 16 == 0 and par_v.data_ptr() % 16 == 0
    gm = erasure_marks(0x5EED0003, G, n, m)
    marks_h = marks_to_rs_layout(gm, k)
    marks = torch.from_numpy(marks_h).to(dev)
    erased = torch.from_numpy(marks_h[:G * k] == 1).to(dev)

    # ---- every leg is right before it is timed
    glen = torch.full((G,), -7, dtype=torch.int32, device=dev)
    invalid = torch.zeros(1, dtype=torch.int32, device=dev)
    code.encode_ptrs(tab_f, max_len)
    code.encode_ptrs_var(tab_v, lens, max_len, glen, invalid)
    assert torch.equal(glen, L) and int(invalid.item()) == 0, "d_group_len"
    Lrow = L.repeat_interleave(m)
    for i in range(0, G * m, step):
        inside = cols[None, :] < Lrow[i:i + step, None]
        assert torch.equal(torch.where(inside, par_v[i:i + step], 0), torch.where(inside, par_f[i:i + step], 0)), \
            f"{setting}: encode_ptrs_var differs from encode_ptrs inside [0, L)"
        assert bool((torch.where(inside, UNTOUCHED, par_v[i:i + step]) == UNTOUCHED).all()), \
            f"{setting}: encode_ptrs_var wrote past L"
    keep = data.clone()
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    for name, call in (("reconstruct_ptrs", lambda: code.reconstruct_ptrs(tab_f, marks, max_len, failed)),
                       ("reconstruct_ptrs_var", lambda: code.reconstruct_ptrs_var(tab_v, lens, glen, marks, max_len, failed, invalid))):
        data[erased, :max_len] = 0x5A
        call()
        assert int(failed.item()) == 0 and int(invalid.item()) == 0
        # the new call writes [0, L) of a marked shard only: what it leaves past L is the damage
        Ld = L.repeat_interleave(k)
        for i in range(0, G * k, step):
            inside = cols[None, :] < (Ld[i:i + step, None] if name.endswith("var") else max_len)
            assert torch.equal(torch.where(inside, data[i:i + step], 0), torch.where(inside, keep[i:i + step], 0)), \
                f"{setting}: {name} did not restore the data"
        data.copy_(keep)
    del keep

    sides = [("encode_ptrs (A)", lambda: code.encode_ptrs(tab_f, max_len)),
             ("encode_ptrs (B)", lambda: code.encode_ptrs(tab_f, max_len)),
             ("reconstruct_ptrs (A)", lambda: code.reconstruct_ptrs(tab_f, marks, max_len)),
             ("reconstruct_ptrs (B)", lambda: code.reconstruct_ptrs(tab_f, marks, max_len)),
             ("encode_ptrs_var", lambda: code.encode_ptrs_var(tab_v, lens, max_len, glen)),
             ("reconstruct_ptrs_var", lambda: code.reconstruct_ptrs_var(tab_v, lens, glen, marks, max_len))]
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
    byte_ratio = (int(lens_h.sum()) + m * int(L_h.sum())) / (n * max_len * G)
    emit(f"RS({k},{m}) max_len={max_len} G={G} lengths={setting}: byte ratio {byte_ratio:.3f}; {m} erasures per group; "
         f"{rounds} interleaved rounds x {reps} calls, device events")
    med = {}
    for name, _ in sides:
        med[name] = statistics.median(times[name])
        emit(f"  {name:24s} median {med[name] * 1e3:9.1f} us  min {min(times[name]) * 1e3:9.1f} us  max {max(times[name]) * 1e3:9.1f} us")
    for call in ("encode_ptrs", "reconstruct_ptrs"):
        a, b = med[f"{call} (A)"], med[f"{call} (B)"]
        mid = statistics.median(times[f"{call} (A)"] + times[f"{call} (B)"])
        emit(f"  {call} A/A: medians differ by {abs(a - b) * 1e3:.1f} us ({(max(a, b) / min(a, b) - 1) * 100:.2f} %); "
             f"yardstick (median of both) {mid * 1e3:.1f} us")
        emit(f"    {call}_var, lengths={setting}: {med[call + '_var'] / mid:.3f} x the fixed-length {call} at max_len "
             f"(byte ratio {byte_ratio:.3f})")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append", help="k,m,max_len,G (repeatable); default: " + " and ".join(SHAPES))
    p.add_argument("--setting", action="append", choices=["full", "drawn", "short10"], help="default: all three")
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
        for setting in a.setting or ["full", "drawn", "short10"]:
            run(shape, setting, a.rounds, a.reps, a.warmup, emit)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
