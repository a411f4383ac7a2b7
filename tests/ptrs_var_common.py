"""Shared by the GPU tests of the pointer-table calls with per-shard lengths (qfec_encode_ptrs_var /
qfec_reconstruct_ptrs_var).  The rows live in a ptrs_common.Pool whose row size is max_len; a row of
length `len` is written into [0, len) of its slot and the slot bytes past `len` stay the guard byte
0xC3, so a read past `len` that reaches a result shows as a wrong byte, and a write past the group's
length shows in the whole-pool compare.  Table entries of shards of length 0 point at one extra guard
row (a valid address, never NULL: a wrong kernel must fail the compare, not fault), which must stay
untouched.  The expected bytes come from the oracle run on rows zero-padded on the CPU.

Every pattern list asserts its own coverage on the CPU before the GPU is called.
"""
import numpy as np

import ptrs_common as pc

INT_MIN, INT_MAX = -2**31, 2**31 - 1
GUARD_ROW_OFFSET = 7  # the guard row is misaligned: shards of length 0 take no part in the alignment judgement


def ladder(k, max_len):
    """0, 1, 15, 16, 17, 31, 32, 33, ... clipped to max_len, the last two shards max_len - 1 and
    max_len: partial columns in different lanes and different sources."""
    base = [v for j in range(k) for v in (16 * j - 1, 16 * j, 16 * j + 1) if v >= 0][:k]
    lens = np.minimum(np.array(base, np.int64), max_len)
    if k >= 2:
        lens[k - 2] = max(max_len - 1, 0)
    lens[k - 1] = max_len
    return lens


def around(k, L):
    """Group length exactly L: even shards L, odd shards a little shorter."""
    return np.array([L if i % 2 == 0 else max(L - (3 * i) % 17, 0) for i in range(k)], np.int64)


def length_patterns(k, max_len):
    """[(name, lens[k])] of valid groups: every pattern of the issue that max_len allows."""
    pats = [("full", np.full(k, max_len, np.int64)),
            ("short", np.full(k, (max_len + 1) // 2, np.int64)),
            ("ladder", ladder(k, max_len)),
            ("stairs", np.maximum(max_len - 37 * np.arange(k, dtype=np.int64), 0)),
            ("steps", np.maximum(max_len - 1 - 5 * np.arange(k, dtype=np.int64), 0)),
            ("one-long", np.array([0] * (k - 1) + [max_len], np.int64)),
            ("short-last-group", np.array([max_len, max(max_len - 3, 1)] + [0] * (k - 2), np.int64)),
            ("empty", np.zeros(k, np.int64))]
    for L in (16, 1024, 1025):
        if L <= max_len:
            pats.append((f"L={L}", around(k, L)))
    return pats


def void_patterns(k, max_len):
    out = []
    for i, bad in enumerate((-1, max_len + 1, INT_MIN, INT_MAX)):
        lens = ladder(k, max_len)
        lens[(i + 1) % k] = bad
        out.append((f"void{bad}", lens))
    return out


def assert_lengths_cover(pats, k, max_len):
    """The coverage the tests rely on, checked on the patterns themselves."""
    names = [n for n, _ in pats]
    lens = [l for _, l in pats]
    valid = [l for l in lens if ((l >= 0) & (l <= max_len)).all()]
    voids = [l for l in lens if not ((l >= 0) & (l <= max_len)).all()]
    assert {int(v[(v < 0) | (v > max_len)][0]) for v in voids} == {-1, max_len + 1, INT_MIN, INT_MAX}, names
    assert any((l == max_len).all() for l in valid), "all lengths = max_len"
    assert any(l.max() == 0 for l in valid), "an all-empty group"
    assert any(l.max() > 0 and (l == 0).sum() == k - 1 for l in valid), "one long shard, the rest empty"
    assert any(l.max() > 0 and (l == 0).any() for l in valid), "an empty shard in a live group"
    assert any(len(set(l.tolist())) == 1 and 0 < l[0] < max_len for l in valid) or max_len == 1, "all equal and short"
    if max_len >= 17:
        part = {i for l in valid for i in np.flatnonzero((l % 16 != 0) & (l < l.max())).tolist()}
        assert len(part) >= 2, "partial columns in several sources"
        assert any(l.max() == 16 for l in valid), "L on a column border"
    if max_len >= 1025:
        assert any(l.max() == 1024 for l in valid) and any(l.max() == 1025 for l in valid), "L on / past a wave border"


class VarPool:
    """ptrs_common.Pool of G * (k + m) rows of max_len bytes plus one guard row; rows written to
    their own lengths only."""

    def __init__(self, G, k, m, max_len, mode, seed):
        self.G, self.k, self.m, self.max_len = G, k, m, max_len
        self.nrows = G * (k + m)
        offs = np.concatenate([pc.offsets_for(mode, G, k, m), [GUARD_ROW_OFFSET]])
        self.pool = pc.Pool(self.nrows + 1, max_len, offs, seed)
        self.guard_row = self.nrows
        self.alias = {}

    def put(self, i, row, n):
        s = self.pool.start[i]
        self.pool.host[s:s + n] = row[:n]

    def put_data(self, data, lens, keep=()):
        """data [G, k, max_len], lens [G, k] (lengths outside [0, max_len]: nothing written); shards of
        length 0 get the guard row's address, except the rows in `keep` (shards a call will write)."""
        for i in range(self.G * self.k):
            n = int(lens.reshape(-1)[i])
            if 0 < n <= self.max_len:
                self.put(i, data.reshape(-1, self.max_len)[i], n)
            elif n == 0 and i not in keep:
                self.alias[i] = self.guard_row

    def put_parity(self, par, n_of_group):
        for g in range(self.G):
            for r in range(self.m):
                self.put(self.G * self.k + g * self.m + r, par[g, r], int(n_of_group[g]))

    def clone_host(self):
        return self.pool.host.copy()

    def row(self, flat, i, n):
        s = self.pool.start[i]
        return flat[s:s + n]

    def to_device(self, torch, dev):
        """(pool tensor, the table without the guard row's own entry)."""
        t, table = pc.to_device(torch, dev, self.pool, self.alias)
        return t, table[:self.nrows].contiguous()


def zero_padded(data, lens):
    """data [G, k, max_len] with every row zero from its length on (rows of void groups as they are)."""
    out = data.copy()
    G, k, B = data.shape
    for g in range(G):
        for i in range(k):
            n = int(lens[g, i])
            if 0 <= n <= B:
                out[g, i, n:] = 0
    return out


def group_lengths(lens, max_len):
    """What the encode reports per group: -1 void, else the longest length."""
    bad = ((lens < 0) | (lens > max_len)).any(1)
    return np.where(bad, -1, lens.max(1)).astype(np.int32)
