#!/usr/bin/env python3
"""Interleaved timing of the plan calls on pointer tables with per-shard lengths
(qfec_reconstruct_ptrs_wide_var / qfec_repair_ptrs_wide_var) against the fixed-length plan calls
(qfec_reconstruct_ptrs_wide / qfec_repair_ptrs_wide) at block_size = max_len on the same rows
zero-padded.  The rows lie in order in an aligned pool, slot pitch = max_len rounded up to 128; 4
erasures per group, a random mix over data and parity.  Three settings of the lengths:

  full      all lengths = max_len: the price of the feature on full packets (every wave runs plan_column)
  short10   one group in ten short: its last 1 .. k - 1 shards empty, the rest max_len
  drawn     lengths drawn deterministically (quicknet_amd.synth) between 64 and max_len: the ragged path

A step is one (shape, setting).  Each step runs in a child process of its own under its own time
limit (--step-timeout), and the first step that fails or runs out of time ends the run.  Inside a
step, in ONE process: every leg's output is compared byte for byte first (the fixed call restores the
zero-padded rows; the new call restores [0, L) of every marked shard and leaves what lies at or past
L as it was); then every round times, in an order drawn anew, the fixed-length reconstruct and repair
twice each (A/A: the yardstick and its spread) and the two new calls, device events around `reps`
calls, warm-up first.  Each new leg is stated as a ratio to the fixed-length A/A median of the same
step, beside the byte ratio (sum len + m * sum L) / ((k + m) * max_len * G).

  python tools/ptrs_wide_var_ab.py [--shape 32,8,1024,20000] [--setting drawn] [--rounds 15] [--reps 5] [--out FILE]
"""
import argparse
import os
import random
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ptrs_var_ab import lengths  # noqa: E402

SHAPES = ["32,8,1024,20000", "64,16,1024,20000"]  # k, m, max_len, G
SETTINGS = ["full", "short10", "drawn"]
DAMAGE = 0x5A


def run(shape, setting, rounds, reps, warmup, emit):
    import numpy as np
    import torch

    import quicknet_amd as qa
    from quicknet_amd.synth import erasure_marks, marks_to_rs_layout

    k, m, max_len, G = (int(x, 0) for x in shape.split(","))
    n, lose = k + m, min(m, 4)
    pitch = (max_len + 127) // 128 * 128
    dev = torch.device("cuda:0")
    code = qa.Code.cauchy(k, m)
    lens_h = lengths(setting, k, max_len, G)
    L_h = lens_h.max(1)
    lens = torch.from_numpy(lens_h.astype(np.int32).reshape(-1)).to(dev)
    L = torch.from_numpy(L_h.astype(np.int32)).to(dev)
    cols = torch.arange(pitch, device=dev, dtype=torch.int32)

    rows = torch.empty((G * n, pitch), dtype=torch.uint8, device=dev)  # data rows, then parity rows
    qa.synth_fill(rows, 0x5EED0002)
    step = 1 << 18
    for i in range(0, G * k, step):  # data rows zero-padded: what the fixed-length call needs, and the reference
        j = min(i + step, G * k)
        rows[i:j] *= (cols[None, :] < lens[i:j, None]).to(torch.uint8)
    table = (torch.arange(G * n, device=dev, dtype=torch.int64) * pitch + rows.data_ptr()).contiguous()
    assert rows.data_ptr() % 16 == 0
    code.encode_ptrs(table, max_len)  # parity of the zero-padded rows: zero from L on
    marks_h = marks_to_rs_layout(erasure_marks(0x5EED1000, G, n, lose), k)
    marks = torch.from_numpy(marks_h).to(dev)
    hit = torch.from_numpy(marks_h == 1).to(dev)  # rs.c layout = the row order of `rows`
    hit_d = hit.clone()
    hit_d[G * k:] = False
    Lrow = torch.cat([L.repeat_interleave(k), L.repeat_interleave(m)])
    torch.cuda.synchronize()
    keep = rows.clone()

    # ---- every leg is right before it is timed
    failed, invalid = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    for call in ("reconstruct", "repair"):
        written = hit_d if call == "reconstruct" else hit
        for var in (False, True):
            rows[written, :max_len] = DAMAGE
            if var:
                getattr(code, call + "_ptrs_wide_var")(table, lens, L, marks, max_len, failed, invalid)
            else:
                getattr(code, call + "_ptrs_wide")(table, marks, max_len, failed)
            assert int(failed.item()) == 0 and int(invalid.item()) == 0
            for i in range(0, G * n, step):
                inside = cols[None, :] < (Lrow[i:i + step, None] if var else max_len)
                assert torch.equal(torch.where(inside, rows[i:i + step], 0), torch.where(inside, keep[i:i + step], 0)), \
                    f"{setting}: {call}_ptrs_wide{'_var' if var else ''} did not restore the rows"
                if var:  # what lies at or past L of a written shard is the damage still; elsewhere nothing changed
                    was = torch.where(written[i:i + step, None] & (cols[None, :] < max_len), DAMAGE, keep[i:i + step])
                    assert torch.equal(torch.where(inside, 0, rows[i:i + step]), torch.where(inside, 0, was)), \
                        f"{setting}: {call}_ptrs_wide_var wrote at or past L"
            rows.copy_(keep)
    del keep

    sides = []
    for call in ("reconstruct", "repair"):
        fixed, var = getattr(code, call + "_ptrs_wide"), getattr(code, call + "_ptrs_wide_var")
        sides += [(f"{call}_ptrs_wide (A)", lambda f=fixed: f(table, marks, max_len)),
                  (f"{call}_ptrs_wide (B)", lambda f=fixed: f(table, marks, max_len)),
                  (f"{call}_ptrs_wide_var", lambda v=var: v(table, lens, L, marks, max_len))]
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
    emit(f"RS({k},{m}) max_len={max_len} G={G} lengths={setting}: byte ratio {byte_ratio:.3f}; {lose} erasures per group; "
         f"{rounds} interleaved rounds x {reps} calls, device events")
    med = {}
    for name, _ in sides:
        med[name] = statistics.median(times[name])
        emit(f"  {name:30s} median {med[name] * 1e3:9.1f} us  min {min(times[name]) * 1e3:9.1f} us  max {max(times[name]) * 1e3:9.1f} us")
    for call in ("reconstruct_ptrs_wide", "repair_ptrs_wide"):
        a, b = med[f"{call} (A)"], med[f"{call} (B)"]
        mid = statistics.median(times[f"{call} (A)"] + times[f"{call} (B)"])
        emit(f"  {call} A/A: medians differ by {abs(a - b) * 1e3:.1f} us ({(max(a, b) / min(a, b) - 1) * 100:.2f} %); "
             f"yardstick (median of both) {mid * 1e3:.1f} us")
        emit(f"    {call}_var, lengths={setting}: {med[call + '_var'] / mid:.3f} x the fixed-length {call} at max_len "
             f"(byte ratio {byte_ratio:.3f})")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", action="append", help="k,m,max_len,G (repeatable); default: " + " and ".join(SHAPES))
    p.add_argument("--setting", action="append", choices=SETTINGS, help="default: all three")
    p.add_argument("--rounds", type=int, default=15)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--step-timeout", type=int, default=150, help="seconds a (shape, setting) step may take")
    p.add_argument("--out", default="", help="also write the report to this file")
    p.add_argument("--one-step", action="store_true", help=argparse.SUPPRESS)  # the child: one shape, one setting
    a = p.parse_args()
    if a.one_step:
        import torch

        import quicknet_amd as qa

        print(f"{qa.lib().qfec_version().decode()} on {torch.cuda.get_device_name(0)}", flush=True)
        run(a.shape[0], a.setting[0], a.rounds, a.reps, a.warmup, lambda line: print(line, flush=True))
        return 0
    lines = []
    for shape in a.shape or SHAPES:
        for setting in a.setting or SETTINGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--one-step", "--shape", shape, "--setting", setting,
                   "--rounds", str(a.rounds), "--reps", str(a.reps), "--warmup", str(a.warmup)]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.step_timeout)
                out, rc = r.stdout, r.returncode
            except subprocess.TimeoutExpired as e:
                out, rc = (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""), 124
            print(out, end="", flush=True)
            got = [x for x in out.splitlines() if "amdgpu.ids" not in x]  # libdrm's complaint about its id table
            lines += got[1:] if lines and got and got[0] == lines[0] else got
            if rc:  # nothing more is started on the GPU after a step that failed or hung
                print(f"step {shape} {setting} ended with status {rc}: stopping", flush=True)
                return rc
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
