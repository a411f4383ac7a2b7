"""Shared by test_locate2_host.py and test_gpu_locate2.py: GF(2^8) linear algebra built on the
oracle's multiply alone, and the brute-force expectation of qfec_locate2 -- syndromes from the
oracle's encode, span membership per byte and per candidate by GF elimination.  Nothing here reads
the library's constants."""
import functools
import itertools

import numpy as np

CLEAN, MULTI, AMBIGUOUS = -1, -2, -3


@functools.lru_cache(maxsize=None)
def mul_table():
    """[256, 256] uint8 products, from the oracle's multiply: the powers of 2 by 255 calls, the
    rest by logarithms, and a sample of entries checked against the oracle again."""
    from oracle.oracle import Oracle

    orc = Oracle()
    exp, x = [], 1
    for _ in range(255):
        exp.append(x)
        x = orc.mul(x, 2)
    assert x == 1 and len(set(exp)) == 255
    log = np.zeros(256, np.int64)
    log[exp] = np.arange(255)
    e = np.array(exp + exp, np.uint8)
    t = e[log[:, None] + log[None, :]]
    t[0, :] = 0
    t[:, 0] = 0
    for a, b in [(3, 7), (0x53, 0xCA), (255, 255), (1, 200), (0, 9), (0x80, 2)]:
        assert t[a, b] == orc.mul(a, b)
    return t


def columns(rows):
    """The n columns of H = [rows | I_m] as tuples of m ints."""
    rows = np.asarray(rows)
    m, k = rows.shape
    return [tuple(int(v) for v in rows[:, x]) for x in range(k)] + [tuple(int(j == x) for j in range(m)) for x in range(m)]


def left_null(cols):
    """Rows spanning the left null space of the matrix with the given columns (each a tuple of m
    ints): Gaussian elimination on [A | I_m] by rows; where A's part ends up zero, the I part is a
    null vector.  -> list of m - rank tuples."""
    mul = mul_table()
    m, c = len(cols[0]), len(cols)
    a = [[cols[x][j] for x in range(c)] + [int(i == j) for i in range(m)] for j in range(m)]
    rank = 0
    for col in range(c):
        piv = next((j for j in range(rank, m) if a[j][col]), None)
        if piv is None:
            continue
        a[rank], a[piv] = a[piv], a[rank]
        p = a[rank][col]
        for j in range(m):
            if j != rank and a[j][col]:
                # row_j = p * row_j ^ a[j][col] * row_rank: no division needed
                q = a[j][col]
                a[j] = [int(mul[p, u]) ^ int(mul[q, v]) for u, v in zip(a[j], a[rank])]
        rank += 1
    return [tuple(r[c:]) for r in a[rank:]]


def rank(cols):
    return len(cols[0]) - len(left_null(cols))


def every_subset_independent(rows, size):
    """Is every set of `size` columns of [rows | I] linearly independent?"""
    h = columns(rows)
    return all(rank([h[x] for x in sub]) == size for sub in itertools.combinations(range(len(h)), size))


def times(f, s):
    """F [r, m] x s [m, N] over GF(2^8) -> [r, N]."""
    mul = mul_table()
    out = np.zeros((len(f), s.shape[1]), np.uint8)
    for r, row in enumerate(f):
        for j, c in enumerate(row):
            if c:
                out[r] ^= mul[c, s[j]]
    return out


def syndromes(oracle, rows, flavour, data, par, B):
    """s = parity ^ rows x data over [0, B), the product by the oracle's encode -> [G, m, B]."""
    tmp = np.zeros_like(par)
    d = np.ascontiguousarray(data)
    (oracle.fec_encode if flavour == "vandermonde" else oracle.rs_encode)(np.ascontiguousarray(rows), d, tmp, B)
    return (tmp ^ par)[..., :B]


def expected_locate2(oracle, rows, flavour, data, par, B):
    """What qfec_locate2 must answer on host arrays data [G, k, pitch], par [G, m, pitch]:
    culprit [G, 2].  A set of shards is a candidate iff the syndromes lie in the span of its columns
    at every byte; single shards first (qfec_locate's verdict), pairs where no single shard explains
    the group."""
    h = columns(rows)
    n = len(h)
    singles = [left_null([h[x]]) for x in range(n)]
    pairs = list(itertools.combinations(range(n), 2))
    pair_null = [left_null([h[a], h[b]]) for a, b in pairs]
    s_all = syndromes(oracle, rows, flavour, data, par, B)
    out = np.full((len(data), 2), CLEAN, np.int32)
    for g in np.nonzero(s_all.any(axis=(1, 2)))[0]:
        s = s_all[g][:, s_all[g].any(axis=0)]  # zero columns lie in every span
        one = [x for x in range(n) if not times(singles[x], s).any()]
        if len(one) == 1:
            out[g] = (one[0], CLEAN)
        elif one:
            out[g] = AMBIGUOUS
        else:
            two = [p for p, f in zip(pairs, pair_null) if not times(f, s).any()]
            out[g] = two[0] if len(two) == 1 else AMBIGUOUS if two else MULTI
    return out


def marks_of(culprit, k, n):
    """rs.c-layout marks with one mark per shard id in culprit [G, 2]."""
    from quicknet_amd.synth import marks_to_rs_layout

    gm = np.zeros((len(culprit), n), np.uint8)
    for slot in range(2):
        hit = culprit[:, slot] >= 0
        gm[np.nonzero(hit)[0], culprit[hit, slot]] = 1
    return marks_to_rs_layout(gm, k)


def counts_of(culprit):
    """[one, two, multi, ambiguous] of culprit [G, 2]."""
    a, b = culprit[:, 0], culprit[:, 1]
    return [int(((a >= 0) & (b < 0)).sum()), int((b >= 0).sum()), int((a == MULTI).sum()), int((a == AMBIGUOUS).sum())]


def random_damage(rng, data, par, B, most):
    """In place on host arrays: each group gets 0..most corrupted shards (every number as likely),
    each at 1-4 random bytes with random non-zero error values.  -> hits [G]."""
    G, k = data.shape[:2]
    n = k + par.shape[1]
    hits = rng.integers(0, most + 1, size=G)
    for g in range(G):
        for c in rng.choice(n, size=int(hits[g]), replace=False):
            row = data[g, c] if c < k else par[g, c - k]
            for b in rng.choice(B, size=int(rng.integers(1, 5)), replace=False):
                row[b] ^= rng.integers(1, 256)
    return hits
