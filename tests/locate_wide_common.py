"""Shared by test_locate_wide_host.py and test_gpu_locate_wide.py: the public layout of a check plan
(include/qfec.h, qfec_check_build), read from Python; the plan a group must get, built from the
existing host query qfec_locate_erased_plan; and a numpy model of what single-shard location is
DEFINED to answer (include/qfec.h, qfec_locate_erased), not of how the kernel finds it: syndromes from
a GF multiply table, then every position of K and every spare tested over every byte of
[0, block_size)."""
import functools

import numpy as np

import quicknet_amd as qa
from quicknet_amd.synth import marks_to_rs_layout
from wide_common import gf_tables

NONE, WORK, FAILED = 0, 1, 2
CLEAN, MULTI, AMBIGUOUS = qa.QFEC_LOC_CLEAN, qa.QFEC_LOC_MULTI, qa.QFEC_LOC_AMBIGUOUS
UNCHECKED, LOST = qa.QFEC_LOC_UNCHECKED, qa.QFEC_LOC_LOST
MARKS_OFF, IDS_OFF = 16, 48


def round16(x):
    return (x + 15) // 16 * 16


def layout(k, m):
    """(a_off, r_off, stride): a 16-byte header, 32 bytes of mark bits, k survivor ids and m spare
    ids padded to 16, m x k rows padded to 16, k x (m - 1) ratios padded to 16."""
    a = round16(IDS_OFF + k + m)
    r = round16(a + m * k)
    return a, r, round16(r + k * max(m - 1, 0))


def header(plan):
    """(S, t, status) of one plan."""
    return int(plan[0]) | int(plan[1]) << 8, int(plan[2]) | int(plan[3]) << 8, int(plan[4])


def mark_bits(marks_n):
    """32 bytes: one bit per shard id, four little-endian u64 words."""
    bits = np.zeros(256, np.uint8)
    bits[:len(marks_n)] = np.asarray(marks_n) != 0
    return np.packbits(bits, bitorder="little")


def expected_check(code, marks_n):
    """The check plan of one group from qfec_locate_erased_plan; every byte not given is zero.  With
    t >= m only the header and the marks are set."""
    k, m = code.k, code.m
    a_off, r_off, stride = layout(k, m)
    marks_n = np.asarray(marks_n, np.uint8)
    t = int((marks_n != 0).sum())
    S, surv, spares, rows, ratios = code.locate_erased_plan(marks_n)
    p = np.zeros(stride, np.uint8)
    status = FAILED if t > m else NONE if t == m else WORK
    assert S == (-1 if t > m else m - t)
    S = max(S, 0)
    p[0], p[1], p[2], p[3], p[4] = S & 255, S >> 8, t & 255, t >> 8, status
    p[MARKS_OFF:MARKS_OFF + 32] = mark_bits(marks_n)
    if status == WORK:
        p[IDS_OFF:IDS_OFF + k] = surv
        p[IDS_OFF + k:IDS_OFF + k + S] = spares
        p[a_off:a_off + S * k] = rows.reshape(-1)
        p[r_off:r_off + k * (S - 1)] = ratios.reshape(-1)
    return p


def masks_of_every_t(seed, n, m, per_t):
    """[*, n] uint8: per_t random masks of every t from 0 to m + 1 (as far as n allows)."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(min(m + 1, n) + 1):
        for _ in range(per_t):
            v = np.zeros(n, np.uint8)
            v[rng.choice(n, size=t, replace=False)] = rng.integers(1, 256, size=t)
            out.append(v)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def gf_mul_table():
    """[256, 256] uint8: the GF(2^8) product (polynomial 0x11D, as the library's)."""
    exp, log = gf_tables()
    a = np.arange(256)
    t = exp[(log[a][:, None] + log[a][None, :]) % 255].astype(np.uint8)
    t[0, :] = 0
    t[:, 0] = 0
    return t


def model_group(code, shards, marks_n, B):
    """The verdict of one group by the definition.  shards: [n, >= B] uint8 (marked rows are not
    read); marks_n: [n]."""
    k = code.k
    mul = gf_mul_table()
    S, surv, spares, rows, ratios = code.locate_erased_plan(marks_n)
    if S < 0:
        return LOST
    if S == 0:
        return UNCHECKED
    x = shards[:, :B]
    syn = x[spares] ^ np.bitwise_xor.reduce(mul[rows[:, :, None], x[surv][None, :, :]], axis=1)  # [S, B]
    if not syn.any():
        return CLEAN
    cands = []
    # position i of K: s_x = (A_x[i] / A_x0[i]) . s_x0 in every byte, for every other spare x
    if S == 1:
        cands += [int(s) for s in surv]
    else:
        pred = mul[ratios[:, :, None], syn[0][None, None, :]]  # [k, S - 1, B]
        holds = (pred == syn[None, 1:, :]).all(axis=(1, 2))
        cands += [int(surv[i]) for i in np.nonzero(holds)[0]]
    # spare y: every other syndrome is zero in every byte
    for y in range(S):
        if not np.delete(syn, y, axis=0).any():
            cands.append(int(spares[y]))
    return MULTI if not cands else AMBIGUOUS if len(cands) > 1 else cands[0]


def model(code, data, par, gm, B, scrub=False):
    """data [G, k, pitch], par [G, m, pitch], gm [G, n] group-order marks -> (culprit [G] int32,
    marks_out [G*n] in the rs.c layout, counts [5]).  scrub: MULTI / AMBIGUOUS groups get no marks."""
    G, k = data.shape[0], code.k
    culprit = np.zeros(G, np.int32)
    out = (gm != 0).astype(np.uint8)
    counts = np.zeros(5, np.int64)
    for g in range(G):
        v = model_group(code, np.concatenate([data[g], par[g]]), gm[g], B)
        culprit[g] = v
        if v >= 0:
            out[g, v] = 1
            counts[0] += 1
        elif v != CLEAN:
            counts[-v - 1] += 1
            if scrub and v in (MULTI, AMBIGUOUS):
                out[g] = 0
    return culprit, marks_to_rs_layout(out, k), counts
