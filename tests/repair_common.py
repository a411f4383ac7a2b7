"""Shared by test_repair_rows.py, test_gpu_repair.py and test_gpu_verify.py: the expectation of a
group repair, built from the oracle's reconstruct and encode (nothing new in oracle/)."""
import itertools

import numpy as np

from quicknet_amd.synth import marks_to_rs_layout


def round16(x):
    return (x + 15) // 16 * 16


def padded(a, pitch, fill=0):
    """[..., B] -> [..., pitch] with pad bytes = fill."""
    out = np.full(a.shape[:-1] + (pitch,), fill, dtype=np.uint8)
    out[..., : a.shape[-1]] = a
    return out


def masks_up_to(n, bits):
    """[M, n] uint8: every mark vector over n positions with at most `bits` bits set."""
    out = []
    for t in range(bits + 1):
        for pos in itertools.combinations(range(n), t):
            v = np.zeros(n, np.uint8)
            v[list(pos)] = 1
            out.append(v)
    return np.stack(out)


def random_marks(rng, G, n, most):
    """[G, n] uint8: each group draws 0..most erasures over the n positions."""
    gm = np.zeros((G, n), np.uint8)
    for g in range(G):
        gm[g, rng.choice(n, size=int(rng.integers(0, most + 1)), replace=False)] = 1
    return gm


def damage(data, par, gm, fill=0x5A):
    """Copies of data / parity with every marked row of BOTH filled with `fill`."""
    k = data.shape[1]
    d, p = data.copy(), par.copy()
    d[gm[:, :k] == 1] = fill
    p[gm[:, k:] == 1] = fill
    return d, p


def expected_repair(oracle, code, flavour, data, par, gm, B):
    """What a repair must leave in [0, B) of data [G, k, B] and par [G, m, B] (damaged inputs):
    the oracle's reconstruct on a copy of the data, its encode of the result into a temporary, and
    only the marked parity rows of groups with t <= m copied over.  Returns (data, parity, failed)."""
    k, m = code.k, code.m
    rec, enc = ((oracle.rs_reconstruct, oracle.rs_encode) if flavour == "cauchy"
                else (oracle.fec_reconstruct, oracle.fec_encode))
    rows = code.rows
    exp = np.ascontiguousarray(data).copy()
    rec(rows, exp, np.ascontiguousarray(par).copy(), marks_to_rs_layout(gm, k), B)
    tmp = np.zeros_like(par)
    enc(rows, exp, tmp, B)
    ok = gm.sum(1) <= m
    exp_par = par.copy()
    sel = (gm[:, k:] == 1) & ok[:, None]
    exp_par[sel] = tmp[sel]
    # a group with t > m is left alone by the oracle's reconstruct too (e > surviving parity)
    assert np.array_equal(exp[~ok], data[~ok])
    return exp, exp_par, int((~ok).sum())
