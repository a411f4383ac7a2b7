"""Shared by test_locate_ptrs_wide_var_host.py and test_gpu_locate_ptrs_wide_var.py: a numpy model of what
qfec_check_apply_ptrs_var / qfec_locate_ptrs_wide_var / qfec_scrub_ptrs_wide_var are DEFINED to answer
(include/qfec.h), and the batches the GPU tests walk, built and judged without a device so that the
CPU tests can assert what they cover.

The model is locate_wide_common.model_group's definition on the rows zero-padded to the group's length
L -- syndromes from a GF multiply table, every position of K and every spare tested over every byte of
[0, L) -- plus: the judgement order (a failed plan, then the lengths, then a plan without work), the
invalid rule (L outside [0, max_len], an UNMARKED data shard outside [0, L]), the length condition (a data
shard of K stays a candidate only if every syndrome is zero from its own end on) and the S = 1 rule (an
inconsistent group with one spare is AMBIGUOUS whatever the lengths say).

A Case holds a batch in a ptrs_var_common.VarPool: data rows written to their own lengths, parity rows to
L, every other byte of the pool random (so a byte read past a shard's end turns a verdict, and a byte
written there fails the whole-pool compare).  Table entries that must never be dereferenced -- marked
shards (locates), unmarked data shards of length 0, every shard of an invalid group -- are WILD."""
import functools

import numpy as np

import integrity_ptrs_common as ic
import integrity_ptrs_var_common as iv
import locate_wide_common as lw
import ptrs_common as pc
import ptrs_var_common as pv
import ptrs_wide_var_common as wv
import quicknet_amd as qa
from locate_wide_common import AMBIGUOUS, CLEAN, LOST, MULTI, UNCHECKED
from quicknet_amd.synth import marks_to_rs_layout

INVALID = qa.QFEC_LOC_INVALID
INT_MIN, INT_MAX = pv.INT_MIN, pv.INT_MAX
WILD = iv.WILD
MODES = iv.MODES
MAX_LENS = iv.MAX_LENS
# (10,3): NP 1, narrow; (32,8): one syndrome pass; (70,10): NP 2, two syndrome passes, a candidate at
# position 69 of K; (200,55): NP 4
CODES = [(10, 3), (32, 8), (70, 10), (200, 55)]
FAMILY = [(k, m, ml) for k, m in CODES for ml in (17, 1025)] + [(10, 3, 1400), (32, 8, 1400)]
KINDS = ["none", "data-first", "data-last", "parity-in-K", "spare-last", "two", "past-end"]


def six_ts(m):
    return sorted({0, 1, m - 2, m - 1, m, m + 1})


def invalid_group(marks_n, lens, L, k, max_len):
    un = np.asarray(marks_n[:k]) == 0
    lens = np.asarray(lens, np.int64)
    return bool(L < 0 or L > max_len or (un & ((lens < 0) | (lens > L))).any())


def model_group(code, shards, marks_n, lens, L, max_len):
    """The verdict of one group by the definition.  shards: [n, >= L] uint8, data rows zero from their
    own length on (marked rows are not read); marks_n [n]; lens [k]; L the group's length."""
    k = code.k
    S, surv, spares, rows, ratios = code.locate_erased_plan(marks_n)
    if S < 0:
        return LOST
    if invalid_group(marks_n, lens, L, k, max_len):
        return INVALID
    if S == 0:
        return UNCHECKED
    if L == 0:
        return CLEAN
    mul = lw.gf_mul_table()
    x = shards[:, :L]
    syn = x[spares] ^ np.bitwise_xor.reduce(mul[rows[:, :, None], x[surv][None, :, :]], axis=1)  # [S, L]
    if not syn.any():
        return CLEAN
    if S == 1:
        return AMBIGUOUS  # no ratio to test; the lengths are not used to narrow it
    cands = []
    pred = mul[ratios[:, :, None], syn[0][None, None, :]]  # [k, S - 1, L]
    holds = (pred == syn[None, 1:, :]).all(axis=(1, 2))
    for i in np.nonzero(holds)[0]:
        s = int(surv[i])
        if s < k and syn[:, int(lens[s]):].any():
            continue  # known zero from its own end on: it cannot be wrong there
        cands.append(s)
    for y in range(S):
        if not np.delete(syn, y, axis=0).any():
            cands.append(int(spares[y]))
    return MULTI if not cands else AMBIGUOUS if len(cands) > 1 else cands[0]


def model(code, data, par, gm, lens, glen, max_len, scrub=False):
    """data [G, k, max_len] zero from each length on, par [G, m, max_len], gm [G, n], lens [G, k], glen [G]
    -> (culprit [G] int32, marks_out [G*n] in the rs.c layout, counts [5], invalid)."""
    G, k = len(gm), code.k
    culprit = np.zeros(G, np.int32)
    out = (gm != 0).astype(np.uint8)
    counts = np.zeros(5, np.int64)
    for g in range(G):
        v = model_group(code, np.concatenate([data[g], par[g]]), gm[g], lens[g], int(glen[g]), max_len)
        culprit[g] = v
        if v >= 0:
            out[g, v] = 1
            counts[0] += 1
        elif v not in (CLEAN, INVALID):
            counts[-v - 1] += 1
        if scrub and v in (MULTI, AMBIGUOUS, INVALID):
            out[g] = 0
    return culprit, marks_to_rs_layout(out, k), counts, int((culprit == INVALID).sum())


# ---------------------------------------------------------------- batches
class Case:
    """specs: [dict(lens [k], L, marks [n], hits [(shard, byte, xor)], phantom [(data shard, byte, value)])].
    A phantom byte sits in the encoder's input at or past the shard's own end, where the shard is known
    to be zero: the parity then says that the shard is wrong there.  Rows of marked shards hold junk
    over [0, L); clean holds their true bytes (what a repair must write)."""

    def __init__(self, code, specs, max_len, mode, seed, hold=None):
        k, m = code.k, code.m
        n = k + m
        self.code, self.k, self.m, self.max_len, self.mode = code, k, m, max_len, mode
        G = self.G = len(specs)
        self.gm = np.stack([np.asarray(s["marks"], np.uint8) for s in specs])
        self.lens = np.stack([np.asarray(s["lens"], np.int64) for s in specs])
        self.glen = np.array([s["L"] for s in specs], np.int64)
        self.bad = np.array([invalid_group(self.gm[g], self.lens[g], self.glen[g], k, max_len) for g in range(G)])
        Lc = np.clip(self.glen, 0, max_len)
        # a marked data shard has room for L bytes and its d_lens entry is not looked at
        room = np.where(self.gm[:, :k] != 0, Lc[:, None], np.clip(self.lens, 0, Lc[:, None]))
        room[self.bad] = 0
        self.room = room
        if hold is None:
            src = pv.zero_padded(pc.batch_bytes(seed, G, k, max_len), room)
            for g, s in enumerate(specs):
                for c, b, v in s.get("phantom", ()):
                    assert not self.gm[g, c] and room[g, c] <= b < Lc[g] and v
                    src[g, c, b] = v
            par = ic.encode(np.ascontiguousarray(code.rows), src, max_len)  # zero from L on, as src is
            true = src.copy()
            for g, s in enumerate(specs):
                for c, b, v in s.get("phantom", ()):
                    src[g, c, b] = 0  # the shard itself ends before it
            rng = np.random.default_rng(seed + 5)
            hd, hp = src.copy(), par.copy()
            for g, s in enumerate(specs):
                for c in np.flatnonzero(self.gm[g]):  # junk where a lost shard lies
                    row = hd[g, c] if c < k else hp[g, c - k]
                    row[:Lc[g]] = rng.integers(0, 256, size=Lc[g], dtype=np.uint8)
                for c, b, v in s.get("hits", ()):
                    assert not self.gm[g, c] and v and 0 <= b < (room[g, c] if c < k else Lc[g])
                    (hd[g, c] if c < k else hp[g, c - k])[b] ^= v
            hold = (true, par, hd, hp)
            for a in hold:
                a.setflags(write=False)
        self.hold = hold
        self.true_d, self.true_p, self.hd, self.hp = hold
        # what the model sees: the unmarked rows, data rows zero from their own length on
        self.vp = pv.VarPool(G, k, m, max_len, mode, seed + 2)
        pool = self.vp.pool
        pool.host[:] = np.random.default_rng(seed + 9).integers(0, 256, size=len(pool.host), dtype=np.uint8)
        plen = np.repeat(np.where(self.bad, 0, Lc), m)
        self.clean = self._image(self.true_d, self.true_p, room, plen)
        self.image = self._image(self.hd, self.hp, room, plen)

    def _image(self, d, p, room, plen):
        saved = self.vp.pool.host
        img = saved.copy()
        self.vp.pool.host = img
        wv.fill_rows(self.vp, 0, d.reshape(self.G * self.k, self.max_len), room)
        wv.fill_rows(self.vp, self.G * self.k, p.reshape(self.G * self.m, self.max_len), plen)
        self.vp.pool.host = saved
        return img

    def in_mode(self, mode):
        """The same batch in another alignment mode: the rows and their damage are shared."""
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        Case.__init__(c, self.code, self.specs, self.max_len, mode, self.seed, hold=self.hold)
        c.expect = self.expect  # the verdicts do not depend on where the rows lie
        return c

    def row(self, g, c):
        return ic.row_id(self.G, self.k, self.m, g, c)

    def table(self, base, scrub=False):
        """int64 [G * n] addresses for a pool at device address `base`.  WILD: the unmarked data shards
        of length 0, every shard of an invalid group, and (the locates) every marked shard."""
        t = base + self.vp.pool.start[:self.vp.nrows].astype(np.int64)
        k = self.k
        for g in range(self.G):
            for c in range(k + self.m):
                marked = self.gm[g, c] != 0
                if self.bad[g] or (marked and not scrub) or (not marked and c < k and self.lens[g, c] == 0):
                    t[self.row(g, c)] = WILD + 16 * (g * 256 + c)
        return t

    def d_lens(self):
        """int32 [G * k]: the entries of marked shards hold what must not be looked at."""
        junk = np.array([INT_MIN, INT_MAX, -1, 1 << 20], np.int64)
        idx = (np.arange(self.G)[:, None] + np.arange(self.k)[None, :]) % 4
        return np.where(self.gm[:, :self.k] != 0, junk[idx], self.lens).astype(np.int32).reshape(-1)

    def marks(self):
        return marks_to_rs_layout(self.gm, self.k)

    @functools.lru_cache(maxsize=None)
    def expect(self, scrub=False):
        return model(self.code, self.hd, self.hp, self.gm, self.lens, self.glen, self.max_len, scrub)

    def scrubbed(self):
        """The pool after the scrub: the healed groups' rows as in `clean`, everything else as it was."""
        v = self.expect(True)[0]
        healed = ~np.isin(v, (INVALID, MULTI, AMBIGUOUS, LOST))
        out = self.image.copy()
        B = self.max_len
        for g in np.flatnonzero(healed):
            for c in range(self.k + self.m):
                s = self.vp.pool.start[self.row(g, c)]
                out[s:s + B] = self.clean[s:s + B]
        return out


def make(code, specs, max_len, mode, seed):
    c = Case(code, specs, max_len, mode, seed)
    c.specs, c.seed = specs, seed
    return c


def lose(rng, n, t, keep=(), first=()):
    """marks [n] with t lost shards outside `keep`, those of `first` among them."""
    ids = [i for i in first if i not in keep][:t]
    rest = [i for i in range(n) if i not in keep and i not in ids]
    ids += list(rng.choice(rest, size=t - len(ids), replace=False))
    gm = np.zeros(n, np.uint8)
    gm[ids] = rng.integers(1, 256, size=len(ids))
    return gm


def spec_for(rng, k, m, lens, L, t, kind):
    """One valid group of `kind` (KINDS) beside t lost shards; where the kind has no room (too few
    spares, no shard of the wanted shape) the group stays consistent."""
    n = k + m
    lens = np.asarray(lens, np.int64)
    some = [i for i in range(k) if lens[i] > 0]
    short = [i for i in some if lens[i] < L]
    keep, first, hits, phantom = (), (), [], []
    x = int(rng.integers(1, 256))
    if t < m and L > 0:
        if kind in ("data-first", "data-last") and some:
            c = short[len(short) // 2] if short and kind == "data-last" else some[(3 * t) % len(some)]
            keep, hits = (c,), [(c, 0 if kind == "data-first" else int(lens[c]) - 1, x)]
        elif kind == "parity-in-K" and t >= 1:
            keep, first, hits = (k,), (0,), [(k, L - 1, x)]  # data shard 0 lost: parity shard k enters K
        elif kind == "spare-last":
            keep, hits = (n - 1,), [(n - 1, L - 1, x)]
        elif kind == "two" and some:
            keep, hits = (some[0], n - 1), [(some[0], int(lens[some[0]]) // 2, x), (n - 1, L // 2, x ^ 0x5B or 1)]
        elif kind == "past-end" and short:
            c = short[(5 * t) % len(short)]
            keep, phantom = (c,), [(c, int(lens[c]), x)]
    return dict(lens=lens, L=int(L), marks=lose(rng, n, t, keep, first), hits=hits, phantom=phantom)


def void_specs(rng, k, m, max_len):
    """Ten groups: six invalid -- L = -1, L = max_len + 1, an unmarked data shard of -1, L + 1, INT_MIN,
    INT_MAX -- and the same four values on a MARKED shard, which is not invalid."""
    n = k + m
    L = max(max_len - 1, 1)
    base = np.minimum(pv.ladder(k, max_len), L)
    out = []
    for bad_L in (-1, max_len + 1):
        out.append(dict(lens=np.minimum(base, max(bad_L, 0)), L=bad_L, marks=lose(rng, n, 1)))
    for i, v in enumerate((-1, L + 1, INT_MIN, INT_MAX)):
        lens = base.copy()
        lens[(i + 2) % k] = v
        out.append(dict(lens=lens, L=L, marks=lose(rng, n, i % 2, keep=((i + 2) % k,))))
    for i, v in enumerate((-1, L + 1, INT_MIN, INT_MAX)):
        lens = base.copy()
        c = (i + 3) % k
        lens[c] = v
        out.append(dict(lens=lens, L=L, marks=lose(rng, n, 1, first=(c,)), hits=[(n - 1, 0, 0x31)] if m > 2 else []))
    return out


@functools.lru_cache(maxsize=None)
def family(k, m, max_len, mode="aligned"):
    """The batch of one code at one max_len: the length patterns of integrity_ptrs_var_common.patterns in
    turn (all L, all 0 but one, cycling, shards ending at byte 0, on a column, in the tail, at 1023 / 1024
    / 1025; L = 1, 15, 16, 17, 1024, 1025, 0), every t of six_ts(m) under every kind of KINDS, then
    void_specs.  The rows are shared by the alignment modes."""
    if mode != "aligned":
        return family(k, m, max_len).in_mode(mode)
    code = qa.Code.cauchy(k, m)
    rng = np.random.default_rng(1000 * k + 10 * m + max_len)
    pats = iv.patterns(k, max_len)
    iv.assert_patterns_cover(pats, k, max_len)
    ts = six_ts(m)
    specs = []
    G = max(len(KINDS) * len(ts), len(pats))
    for g in range(G):
        _, lens, L = pats[g % len(pats)]
        specs.append(spec_for(rng, k, m, lens, L, ts[(g // len(KINDS)) % len(ts)], KINDS[g % len(KINDS)]))
    # the kinds that need a short shard, on the pattern that has them, at the t that lets them work
    ladder = next(l for nme, l, _ in pats if nme == "L-above")
    for t in sorted({0, 1, max(m - 2, 0)}):
        for kind in KINDS[1:]:
            specs.append(spec_for(rng, k, m, ladder, max_len, t, kind))
    specs += void_specs(rng, k, m, max_len)
    return make(code, specs, max_len, "aligned", 7 * k + m + max_len)


def assert_family_covers(case):
    """Every verdict class the GPU tests promise, as conditions on the model's output."""
    k = case.k
    v = case.expect()[0]
    S = np.array([case.m - int((case.gm[g] != 0).sum()) for g in range(case.G)])
    in_K = [g for g in range(case.G) if v[g] >= k and v[g] in np.flatnonzero(case.gm[g] == 0)[:k]]
    spare = [g for g in range(case.G) if v[g] >= 0 and v[g] in np.flatnonzero(case.gm[g] == 0)[k:]]
    phantom = [g for g, s in enumerate(case.specs) if s.get("phantom")]
    two = [g for g, s in enumerate(case.specs) if len(s.get("hits", ())) == 2 and S[g] >= 3]
    assert ((v >= 0) & (v < k)).any(), "a located data id"
    assert in_K, "a parity id inside K"
    assert spare, "a spare"
    assert two and (v[two] == MULTI).all(), "MULTI by two shards"
    assert phantom and all(v[g] == (MULTI if S[g] >= 2 else AMBIGUOUS) for g in phantom), "wrong past its own end"
    assert any(S[g] >= 2 for g in phantom), "MULTI by wrong past its own end"
    for what in (AMBIGUOUS, UNCHECKED, LOST, CLEAN, INVALID):
        assert (v == what).any(), what
    assert ((case.glen == 0) & (v == CLEAN)).any() and ((case.glen == 0) & (S >= 1)).any(), "L = 0 with a working plan"
    assert (v == INVALID).sum() == 6 == case.bad.sum(), "six invalid groups; the four with a bad marked entry are valid"
    ends = {int(case.lens[g, v[g]]) for g in range(case.G) if 0 <= v[g] < k}
    assert len(ends) > 1 and any(e < case.glen[g] for g in range(case.G) if 0 <= v[g] < k for e in [case.lens[g, v[g]]])
