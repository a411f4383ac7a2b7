#!/usr/bin/env python3
"""Interleaved timing, in ONE process, of incremental parity on pointer tables (qfec_update_ptrs,
qfec_encode_update_ptrs and their forms with per-shard lengths) against their contiguous twins
(qfec_update, qfec_encode_update) on the same bytes:

  update, every group touched, twice (A/A: the spread, and the yardstick)
  update_ptrs with the table in order over the same buffers; with the rows permuted in a pool
  update / update_ptrs with one group in ten touched, and with none: the calls' floors
  update_ptrs_var with all lengths = max_len; with lengths drawn between 64 and max_len
  encode_update over count = 1 accumulating, and encode_update_ptrs the same in order / permuted
  encode_update_ptrs_var over count = 1 with all lengths = max_len; with drawn lengths
  encode_ptrs of the whole group, which is what a sender without the range form waits for

Every round times each side back to back (device events around `reps` calls, warm-up first), and the
order within a round is drawn anew every round.  Before anything is timed every call is checked: each
pointer-table call leaves the bytes its contiguous twin leaves, and the forms with lengths leave a batch
that qfec_verify_ptrs_var finds clean.

  python tools/update_ptrs_ab.py [--shape 10,3,1024,100000] [--rounds 15] [--reps 10] [--out FILE]
"""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ["10,3,1024,100000", "16,4,1400,250000"]  # k, m, B, G


def run(shape, rounds, reps, warmup, emit):
    import numpy as np
    import torch

    import quicknet_amd as qa

    k, m, B, G = (int(x, 0) for x in shape.split(","))
    P = (B + 15) // 16 * 16
    dev = torch.device("cuda:0")
    code = qa.Code.cauchy(k, m)
    rng = np.random.default_rng(0x5EED0B01)

    def up(a, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).to(dev)

    data = torch.empty((G, k, P), dtype=torch.uint8, device=dev)
    qa.synth_fill(data, 0x5EED0B02)
    par = torch.empty((G, m, P), dtype=torch.uint8, device=dev)
    code.encode(data, par, B)
    rows = torch.empty((G, P), dtype=torch.uint8, device=dev)
    qa.synth_fill(rows, 0x5EED0B03)
    torch.cuda.synchronize()
    d0, p0 = data.clone(), par.clone()

    def restore():
        data.copy_(d0)
        par.copy_(p0)

    # the table in order: the rows of the contiguous buffers themselves
    def in_order(d, p):
        return np.concatenate([d.data_ptr() + np.arange(G * k, dtype=np.int64) * P,
                               p.data_ptr() + np.arange(G * m, dtype=np.int64) * P])

    table = up(in_order(data, par))
    new = up(rows.data_ptr() + np.arange(G, dtype=np.int64) * P)
    # the same bytes permuted in a pool of G * (k + m + 1) slots of P bytes
    n_rows = G * (k + m + 1)
    pool = torch.empty((n_rows, P), dtype=torch.uint8, device=dev)
    slot = torch.from_numpy(rng.permutation(n_rows)).to(dev)

    def fill_pool():
        pool[slot[:G * k]] = d0.view(G * k, P)
        pool[slot[G * k:G * (k + m)]] = p0.view(G * m, P)
        pool[slot[G * (k + m):]] = rows

    fill_pool()
    slot_addr = pool.data_ptr() + slot.cpu().numpy().astype(np.int64) * P
    ptable, pnew = up(slot_addr[:G * (k + m)]), up(slot_addr[G * (k + m):])

    every = rng.integers(0, k, G).astype(np.int32)
    tenth = np.full(G, qa.QFEC_UPD_NONE, np.int32)
    some = rng.choice(G, G // 10, replace=False)
    tenth[some] = every[some]
    shard = {"all": up(every), "10 %": up(tenth), "none": up(np.full(G, qa.QFEC_UPD_NONE, np.int32))}
    full_lens, full_glen, full_n = (torch.full((n,), B, dtype=torch.int32, device=dev) for n in (G * k, G, G))
    drawn = rng.integers(64, B + 1, (G, k)).astype(np.int32)
    drawn_n = rng.integers(64, B + 1, G).astype(np.int32)
    drawn_lens, drawn_new = up(drawn), up(drawn_n)

    # ---- every call is right before it is timed
    def same_as_pool():
        return (torch.equal(pool[slot[:G * k]][:, :B], data.view(G * k, P)[:, :B]) and
                torch.equal(pool[slot[G * k:G * (k + m)]][:, :B], par.view(G * m, P)[:, :B]))

    for which in ("all", "10 %", "none"):
        restore()
        code.update(shard[which], rows, par, data=data, block_size=B)
        want_d, want_p = data.clone(), par.clone()
        for name, fn in (("update_ptrs", lambda: code.update_ptrs(table, shard[which], new, B)),
                         ("update_ptrs_var", lambda: code.update_ptrs_var(table, full_lens, full_glen, shard[which], new, full_n, B))):
            restore()
            fn()
            assert torch.equal(data[..., :B], want_d[..., :B]) and torch.equal(par[..., :B], want_p[..., :B]), f"{name}, {which} touched"
        fill_pool()
        code.update_ptrs(ptable, shard[which], pnew, B)
        assert same_as_pool(), f"update_ptrs on the permuted pool, {which} touched"
    restore()
    one = data[:, k - 1:].contiguous()
    code.encode_update(one, par, k - 1, B, accumulate=True)
    want_p = par.clone()
    for name, fn in (("encode_update_ptrs", lambda: code.encode_update_ptrs(table, k - 1, 1, B)),
                     ("encode_update_ptrs_var", lambda: code.encode_update_ptrs_var(table, k - 1, 1, full_lens, full_glen, B))):
        restore()
        fn()
        assert torch.equal(par[..., :B], want_p[..., :B]), name
    fill_pool()
    code.encode_update_ptrs(ptable, k - 1, 1, B)
    assert same_as_pool(), "encode_update_ptrs on the permuted pool"
    restore()
    par.fill_(0x77)
    code.encode_update_ptrs(table, 0, 1, B, accumulate=False)
    code.encode_update_ptrs(table, 1, k - 1, B)
    assert torch.equal(par[..., :B], p0[..., :B]), "encode_update_ptrs over [0, 1) + [1, k) differs from the encode"
    # drawn lengths: pieces, then an update, the caller's store of the new lengths, and the parity check
    code.encode_update_ptrs_var(table, 0, 1, drawn_lens, full_glen, B, accumulate=False)
    code.encode_update_ptrs_var(table, 1, k - 1, drawn_lens, full_glen, B)
    assert not bool(code.verify_ptrs_var(table, drawn_lens, full_glen, B).any()), "encode_update_ptrs_var, drawn lengths"
    code.update_ptrs_var(table, drawn_lens, full_glen, shard["all"], new, drawn_new, B)
    stored = drawn.copy()
    stored[np.arange(G), every] = drawn_n
    assert not bool(code.verify_ptrs_var(table, up(stored), full_glen, B).any()), "update_ptrs_var, drawn lengths"
    restore()
    fill_pool()
    torch.cuda.synchronize()
    del want_d, want_p

    # ---- timing
    last = k - 1
    sides = [
        ("update (A)", lambda: code.update(shard["all"], rows, par, data=data, block_size=B)),
        ("update (B)", lambda: code.update(shard["all"], rows, par, data=data, block_size=B)),
        ("update_ptrs, in order", lambda: code.update_ptrs(table, shard["all"], new, B)),
        ("update_ptrs, permuted", lambda: code.update_ptrs(ptable, shard["all"], pnew, B)),
        ("update, 10 % touched", lambda: code.update(shard["10 %"], rows, par, data=data, block_size=B)),
        ("update_ptrs, in order, 10 % touched", lambda: code.update_ptrs(table, shard["10 %"], new, B)),
        ("update, none touched", lambda: code.update(shard["none"], rows, par, data=data, block_size=B)),
        ("update_ptrs, in order, none touched", lambda: code.update_ptrs(table, shard["none"], new, B)),
        ("update_ptrs_var, lengths = max_len", lambda: code.update_ptrs_var(table, full_lens, full_glen, shard["all"], new, full_n, B)),
        ("update_ptrs_var, lengths 64 .. max_len", lambda: code.update_ptrs_var(table, drawn_lens, full_glen, shard["all"], new, drawn_new, B)),
        ("encode_update, count = 1", lambda: code.encode_update(one, par, last, B, accumulate=True)),
        ("encode_update_ptrs, count = 1, in order", lambda: code.encode_update_ptrs(table, last, 1, B)),
        ("encode_update_ptrs, count = 1, permuted", lambda: code.encode_update_ptrs(ptable, last, 1, B)),
        ("encode_update_ptrs_var, count = 1, lengths = max_len", lambda: code.encode_update_ptrs_var(table, last, 1, full_lens, full_glen, B)),
        ("encode_update_ptrs_var, count = 1, lengths 64 .. max_len", lambda: code.encode_update_ptrs_var(table, last, 1, drawn_lens, full_glen, B)),
        ("encode_ptrs, whole group, in order", lambda: code.encode_ptrs(table, B)),
    ]
    s = torch.cuda.current_stream()
    for _, fn in sides:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in sides}
    order = random.Random(0x5EED0B04)
    for _ in range(rounds):
        for name, fn in order.sample(sides, len(sides)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(reps):
                fn()
            e1.record(s)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps)
    emit(f"RS({k},{m}) B={B} pitch={P} G={G}: {rounds} interleaved rounds x {reps} calls, device events")
    med = {}
    for name, _ in sides:
        med[name] = statistics.median(times[name])
        emit(f"  {name:58s} median {med[name] * 1e3:8.1f} us  min {min(times[name]) * 1e3:8.1f} us  max {max(times[name]) * 1e3:8.1f} us")
    lo, hi = sorted((med["update (A)"], med["update (B)"]))
    emit(f"  update A/A: medians differ by {(hi - lo) * 1e3:.1f} us ({(hi / lo - 1) * 100:.2f} %)")

    def ratio(a, b):
        emit(f"  {a}  /  {b}  =  {med[a] / med[b]:.3f}")

    ratio("update_ptrs, in order", "update (A)")
    ratio("update_ptrs, permuted", "update_ptrs, in order")
    ratio("update_ptrs, in order, 10 % touched", "update, 10 % touched")
    ratio("update_ptrs, in order, 10 % touched", "update_ptrs, in order")
    ratio("update_ptrs, in order, none touched", "update, none touched")
    ratio("update_ptrs_var, lengths = max_len", "update_ptrs, in order")
    ratio("update_ptrs_var, lengths 64 .. max_len", "update_ptrs, in order")
    ratio("encode_update_ptrs, count = 1, in order", "encode_update, count = 1")
    ratio("encode_update_ptrs, count = 1, permuted", "encode_update_ptrs, count = 1, in order")
    ratio("encode_update_ptrs_var, count = 1, lengths = max_len", "encode_update_ptrs, count = 1, in order")
    ratio("encode_update_ptrs_var, count = 1, lengths 64 .. max_len", "encode_update_ptrs, count = 1, in order")
    ratio("encode_update_ptrs, count = 1, in order", "encode_ptrs, whole group, in order")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append", help="k,m,B,G (repeatable); default: " + " and ".join(SHAPES))
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
