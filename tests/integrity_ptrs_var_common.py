"""Shared by the tests of the integrity family on pointer tables with per-shard lengths
(qfec_verify_ptrs_var, qfec_locate_ptrs_var, qfec_scrub_ptrs_var): the shapes and length patterns the
GPU tests walk and the coverage they promise, consistent batches in a ptrs_var_common.VarPool (encoded
by the oracle on zero-padded rows; every byte outside a row's own length random), and a CPU model of
the three calls: the oracle's parity of the zero-padded rows gives the syndromes, the verdict is
qfec_locate's on them plus the beyond-length rule, the correction is the formula of include/qfec.h.

Nothing here needs a device; torch is imported by the GPU test alone."""
import functools

import numpy as np

import integrity_ptrs_common as ic
import ptrs_var_common as pv
from integrity_ptrs_common import AMBIGUOUS, CLEAN, MULTI
from locate2_common import mul_table

INVALID = -6
INT_MIN, INT_MAX = pv.INT_MIN, pv.INT_MAX
TEMPLATED, RUNTIME, VERIFY_ONLY, LOCATE_ONLY = ic.TEMPLATED, ic.RUNTIME, ic.VERIFY_ONLY, ic.LOCATE_ONLY
SCRUB_ONLY = [(20, 8)]
MAX_LENS = [17, 1025, 1400]   # 1025: the smallest with two slabs; 1400: a short second slab plus a tail
GROUP_LENS = [1, 15, 16, 17, 1024, 1025]
MODES = ic.MODES
G = 37
WILD = 0x7FFF_DEAD_BEE0_0005  # the table entry of a shard that must never be dereferenced (misaligned too)


def patterns(k, max_len):
    """[(name, lens[k], L)] of valid groups: ptrs_var_common's patterns with L = the longest shard, the
    group lengths of GROUP_LENS below max_len, L above every shard, and shards that end on a column, on
    the slab boundary, one byte before and one byte after."""
    out = [(n, l, int(l.max())) for n, l in pv.length_patterns(k, max_len)]
    for L in GROUP_LENS:
        if L <= max_len:
            out.append((f"L={L}", pv.around(k, L), L))
    out.append(("L-above", np.maximum(pv.ladder(k, max_len) - 3, 0), max_len))
    edges = [e for e in (16, 32, 1023, 1024, 1025, 15, 17, 1040) if e <= max_len]
    out.append(("edges", np.array([edges[i % len(edges)] for i in range(k)], np.int64), max_len))
    out.append(("zeros", np.array([0 if i % 2 else max_len for i in range(k)], np.int64), max_len))
    out.append(("equal", np.full(k, max_len, np.int64), max_len))
    return out


def assert_patterns_cover(pats, k, max_len):
    """The coverage the GPU tests rely on, checked on the patterns themselves."""
    pv.assert_lengths_cover([(n, l) for n, l, _ in pats] + pv.void_patterns(k, max_len), k, max_len)
    Ls = {L for _, _, L in pats}
    assert {L for L in GROUP_LENS if L <= max_len} <= Ls and 0 in Ls and max_len in Ls
    assert any(L < max_len and L > 0 for L in Ls), "a group shorter than max_len"
    assert any((l < L).all() for _, l, L in pats if L), "L above every shard"
    assert any((l == L).all() and L == max_len for _, l, L in pats), "all lengths equal"
    assert any((l == 0).any() and L > 0 for _, l, L in pats), "a shard of length 0 in a live group"
    ends = {int(v) for _, l, _ in pats for v in l}
    if max_len >= 33:
        assert {15, 16, 17} <= ends, "a shard ending on a column, one byte before and after"
    if max_len >= 1025:
        assert {1023, 1024, 1025} <= ends, "a shard ending on the slab boundary, one byte before and after"
    for _, l, L in pats:
        assert ((l >= 0) & (l <= L)).all() and 0 <= L <= max_len


def cells():
    """[(k, m, max_len, mode)]: every code at every max_len, every mode at (10,3) and (9,5)."""
    rng = np.random.default_rng(0x22AB)
    out = []
    for k, m in TEMPLATED + RUNTIME + VERIFY_ONLY + LOCATE_ONLY:
        for ml in MAX_LENS:
            out.append((k, m, ml, MODES[int(rng.integers(len(MODES)))]))
    for mode in MODES:
        for k, m in ((10, 3), (9, 5)):
            out.append((k, m, MAX_LENS[int(rng.integers(len(MAX_LENS)))], mode))
    return sorted(set(out))


def assert_coverage(cs):
    have = set(c[:3] for c in cs)
    for k, m in TEMPLATED + RUNTIME + VERIFY_ONLY + LOCATE_ONLY:
        for ml in MAX_LENS:
            assert (k, m, ml) in have, (k, m, ml)
            assert_patterns_cover(patterns(k, ml), k, ml)
    for mode in MODES:
        for km in ((10, 3), (9, 5)):
            assert any(c[:2] == km and c[3] == mode for c in cs), (km, mode)
    for k, m in SCRUB_ONLY:
        assert k + m > 24


def cell_id(c):
    return "k%d-m%d-L%d-%s" % c


class Batch:
    """A consistent batch: G groups whose lengths cycle through patterns(), rows in a VarPool in permuted
    slots, parity by the oracle on the zero-padded rows.  host: the image (every byte outside a row's
    own length random); lens [G, k], glen [G]; shards of length 0 have the table entry WILD."""

    def __init__(self, rows, max_len, mode, lens, glen, seed):
        self.rows = np.ascontiguousarray(rows, np.uint8)
        self.m, self.k = self.rows.shape
        self.G, self.max_len = len(glen), max_len
        self.lens, self.glen = np.asarray(lens, np.int64), np.asarray(glen, np.int64)
        k, m, Gn = self.k, self.m, self.G
        self.vp = pv.VarPool(Gn, k, m, max_len, mode, seed)
        pool = self.vp.pool
        data = ic.pc.batch_bytes(seed * 3 + 1, Gn, k, max_len)
        par = ic.encode(self.rows, pv.zero_padded(data, self.lens), max_len)
        img = np.random.default_rng(seed + 77).integers(0, 256, pool.host.size, dtype=np.uint8)
        for g in np.flatnonzero(~invalid_groups(self.lens, self.glen, max_len)):  # an invalid group holds no rows
            for c in range(k + m):
                n = int(self.lens[g, c]) if c < k else int(self.glen[g])
                s = pool.start[ic.row_id(Gn, k, m, g, c)]
                img[s:s + n] = (data[g, c] if c < k else par[g, c - k])[:n]
        self.host = img
        self.host.setflags(write=False)

    def row(self, g, c):
        return ic.row_id(self.G, self.k, self.m, g, c)

    def span(self, g, c):
        """(first pool index, readable length) of shard c of group g."""
        n = int(self.lens[g, c]) if c < self.k else int(self.glen[g])
        return int(self.vp.pool.start[self.row(g, c)]), n

    def table(self, base):
        """The int64 address table for a pool at device address `base`; WILD where a data shard has
        length 0 or its group is invalid."""
        t = base + self.vp.pool.start[:self.vp.nrows].astype(np.int64)
        bad = invalid_groups(self.lens, self.glen, self.max_len)
        for g in range(self.G):
            for c in range(self.k + self.m):
                if bad[g] or (c < self.k and self.lens[g, c] == 0):
                    t[self.row(g, c)] = WILD + 16 * (g * 64 + c)
        return t

    def hit(self, img, g, c, where, salt):
        ic.hit(self.vp.pool, img, self.row(g, c), where, salt)


def cycle_lengths(k, max_len, Gn=G):
    pats = patterns(k, max_len)
    lens = np.stack([pats[g % len(pats)][1] for g in range(Gn)])
    glen = np.array([pats[g % len(pats)][2] for g in range(Gn)], np.int64)
    return lens, glen


@functools.lru_cache(maxsize=None)
def _batch(rows_key, k, m, max_len, mode):
    rows = np.frombuffer(rows_key, np.uint8).reshape(m, k)
    lens, glen = cycle_lengths(k, max_len)
    return Batch(rows, max_len, mode, lens, glen, seed=k * 100 + max_len + m)


def batch(code, max_len, mode):
    """(batch, image): the batch is shared and read-only, the image is the caller's own copy."""
    b = _batch(np.ascontiguousarray(code.rows).tobytes(), code.k, code.m, max_len, mode)
    return b, b.host.copy()


def invalid_groups(lens, glen, max_len):
    lens, glen = np.asarray(lens, np.int64), np.asarray(glen, np.int64)
    return (glen < 0) | (glen > max_len) | ((lens < 0) | (lens > glen[:, None])).any(1)


def spots(n):
    """Damage kinds of a shard of n >= 1 readable bytes: first byte, last byte, last byte of the last
    whole column, first byte of the part column, a byte in each of two slabs, the whole shard."""
    v = n // 16 * 16
    s = {"first": [0], "last": [n - 1], "row": list(range(n))}
    if v:
        s["col-end"] = [v - 1]
    if v < n:
        s["part"] = [v]
    if n > 1024:
        s["two-slabs"] = [5, 1024 + (n - 1025) // 2]
    return s


# ---------------------------------------------------------------- the CPU model

def padded_rows(b, img):
    """(data [G, k, max_len] zero from each length on, parity [G, m, max_len] zero from L on) of an
    image; an invalid group's rows are all zero (nothing of it is read)."""
    d = np.zeros((b.G, b.k, b.max_len), np.uint8)
    p = np.zeros((b.G, b.m, b.max_len), np.uint8)
    bad = invalid_groups(b.lens, b.glen, b.max_len)
    for g in np.flatnonzero(~bad):
        for c in range(b.k + b.m):
            s, n = b.span(g, c)
            (d[g, c] if c < b.k else p[g, c - b.k])[:n] = img[s:s + n]
    return d, p


def syndromes(b, img):
    d, p = padded_rows(b, img)
    return ic.encode(b.rows, d, b.max_len) ^ p


def model_verify(b, img):
    """-> (bad_rows [G] int32, inconsistent groups, invalid groups)."""
    S = syndromes(b, img)
    bits = np.zeros(b.G, np.int64)
    for j in range(b.m):
        bits |= S[:, j].any(-1).astype(np.int64) << j
    return bits.astype(np.uint32).view(np.int32), int((bits != 0).sum()), int(invalid_groups(b.lens, b.glen, b.max_len).sum())


def model_locate(b, img):
    """-> (culprit [G], counts [located, multi, ambiguous], invalid): qfec_locate's verdict on the
    zero-padded rows; a data shard i is a candidate iff s_j == (rows[j][i] / rows[0][i]) x s_0 in every
    byte and row, and every syndrome is zero in every byte >= len_i."""
    mul = mul_table()
    S = syndromes(b, img)
    bad = invalid_groups(b.lens, b.glen, b.max_len)
    out = np.full(b.G, CLEAN, np.int32)
    for g in range(b.G):
        if bad[g]:
            out[g] = INVALID
            continue
        s = S[g]
        rows_bad = s.any(-1)
        if not rows_bad.any():
            continue
        cands = []
        for i in range(b.k):
            n = int(b.lens[g, i])
            ok = not s[:, n:].any()
            for j in range(1, b.m):
                ok = ok and np.array_equal(mul[b.rows[0, i], s[j]], mul[b.rows[j, i], s[0]])
            if ok:
                cands.append(i)
        if rows_bad.sum() == 1:
            cands.append(b.k + int(np.flatnonzero(rows_bad)[0]))
        out[g] = MULTI if not cands else AMBIGUOUS if len(cands) > 1 else cands[0]
    counts = [int((out >= 0).sum()), int((out == MULTI).sum()), int((out == AMBIGUOUS).sum())]
    return out, counts, int(bad.sum())


def model_scrub(b, img):
    """-> (culprit, counts, invalid, image after the scrub): a located data shard i gets
    (parity_0 ^ sum_{c != i} rows[0][c] x data_c) / rows[0][i] over [0, len_i), a located parity shard j
    the oracle's row j over [0, L); nothing else changes."""
    mul = mul_table()
    culprit, counts, inv = model_locate(b, img)
    d, p = padded_rows(b, img)
    out = img.copy()
    for g in np.flatnonzero(culprit >= 0):
        c = int(culprit[g])
        s, n = b.span(g, c)
        if c >= b.k:
            out[s:s + n] = ic.encode(b.rows, d[g:g + 1], b.max_len)[0, c - b.k, :n]
        else:
            acc = p[g, 0].copy()
            for x in range(b.k):
                if x != c:
                    acc ^= mul[b.rows[0, x], d[g, x]]
            recip = int(np.flatnonzero(mul[b.rows[0, c]] == 1)[0])
            out[s:s + n] = mul[recip, acc][:n]
    return culprit, counts, inv, out
