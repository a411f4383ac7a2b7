"""Shared by test_repair_rows.py and the GPU tests of repair, verify, locate and locate_erased: the
expectation of a group repair, built from the oracle's reconstruct and encode (nothing new in
oracle/), and the device batches those GPU tests start from.  torch is imported inside the helpers
that need it, so the CPU tests that import this module need no device."""
import functools
import itertools

import numpy as np

from quicknet_amd.synth import marks_to_rs_layout, synth_bytes


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


def to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _encoded(flavour, k, m, B, pitch, G):
    import torch

    import quicknet_amd as qa

    code = getattr(qa.Code, flavour)(k, m)
    data = to_dev(synth_bytes(k * 3 + B, G * k * pitch).reshape(G, k, pitch))
    par = torch.empty((G, m, pitch), dtype=torch.uint8, device=data.device)
    code.encode(data, par, B)
    torch.cuda.synchronize()
    if pitch > B:
        par[..., B:] = to_dev(synth_bytes(k * 5 + B, G * m * (pitch - B)).reshape(G, m, pitch - B))
    return code, data, par


def encoded(flavour, k, m, B, pitch, G):
    """A consistent batch: (code, data [G, k, pitch], parity [G, m, pitch]) on the device with random
    garbage in [B, pitch) of both.  Encoded once per case; every test gets copies of its own."""
    code, data, par = _encoded(flavour, k, m, B, pitch, G)
    return code, data.clone(), par.clone()


def shard(data, par, g, c):
    """Row c of group g over all n shards (a view)."""
    k = data.shape[1]
    return data[g, c] if c < k else par[g, c - k]


def one_hot_marks(culprit, k, n):
    """rs.c-layout marks with one mark per group whose culprit is a shard id."""
    gm = np.zeros((len(culprit), n), np.uint8)
    hit = culprit >= 0
    gm[np.nonzero(hit)[0], culprit[hit]] = 1
    return marks_to_rs_layout(gm, k)
