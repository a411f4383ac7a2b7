"""Shared by the GPU tests of the plan calls on pointer tables with per-shard lengths
(qfec_plan_apply_ptrs_var, qfec_reconstruct_ptrs_wide_var, qfec_repair_ptrs_wide_var).  A batch is a
list of groups (name, lens[k], L, marks[k + m]) in a ptrs_var_common.VarPool: data rows written to their
own lengths, parity rows to L, marked rows filled with 0x5A over the L bytes a receiver gives them, the
d_lens entries of marked data shards INT_MIN, shards of length 0 pointing at the pool's misaligned guard
row.  The parity is random, not the encode of the data: that pins which survivors are read.

The expected pool is the pool before the call in which only bytes [0, L) of the rows to write carry
the oracle's bytes: oracle.rs_reconstruct (reconstruct) or repair_common.expected_repair (repair) per
group on its rows zero-padded on the CPU, with B = L.  Which groups fail and which are invalid follows
the rule of include/qfec.h, computed here from the marks and the lengths alone.
"""
import numpy as np

import ptrs_common as pc
import ptrs_var_common as pv
from quicknet_amd.synth import marks_to_rs_layout
from repair_common import expected_repair

FILL = 0x5A
_WRITES = {}  # the oracle's rows of a batch, computed once and shared by the alignment modes


def fill_rows(vp, first, rows, lens):
    """rows [count, max_len] into pool rows first .., each to its own length (outside [0, max_len]:
    nothing); VarPool.put, vectorised."""
    B = vp.max_len
    lens = np.asarray(lens, np.int64).reshape(-1)
    n = np.where((lens < 0) | (lens > B), 0, lens)
    idx = vp.pool.start[first:first + len(rows), None] + np.arange(B)
    mask = np.arange(B)[None, :] < n[:, None]
    vp.pool.host[idx[mask]] = rows.reshape(len(rows), B)[mask]


def classify(gm, lens, L, k, m, max_len, repair):
    """(failed, invalid, work) bool [G] by the header's rule: failed from the marks alone (t > m; a
    reconstruct with no erased data is status 0 whatever else is marked); then invalid from L and the
    lengths of the unmarked data shards; work: status 1, valid, L > 0."""
    t, e = gm.sum(1), gm[:, :k].sum(1)
    failed = (t > m) & (repair | (e > 0))
    status1 = ~failed & ((t if repair else e) > 0)
    unmarked = gm[:, :k] == 0
    bad = (L < 0) | (L > max_len) | (unmarked & ((lens < 0) | (lens > L[:, None]))).any(1)
    invalid = ~failed & bad
    return failed, invalid, status1 & ~bad & (L > 0)


def survivors(gm, k):
    """[G, n] bool: the k lowest unmarked ids (all False where fewer than k are left)."""
    un = gm == 0
    K = un & (np.cumsum(un, 1) <= k)
    K[un.sum(1) < k] = False
    return K


class Batch:
    """groups: [(name, lens[k], L, marks[k + m])].  tripwire: every entry of a shard the group's plan
    neither reads nor writes points at the guard row as well."""

    def __init__(self, oracle, code, groups, max_len, mode, seed, repair, rows=None, tripwire=False, singular=()):
        k, m = code.k, code.m
        self.k, self.m, self.max_len, self.repair, self.groups = k, m, max_len, repair, groups
        G = self.G = len(groups)
        gm = self.gm = np.stack([g[3] for g in groups]).astype(np.uint8)
        lens = self.lens = np.stack([g[1] for g in groups]).astype(np.int64)
        L = self.L = np.array([g[2] for g in groups], np.int64)
        Lc = np.clip(L, 0, max_len)
        self.failed, self.invalid, self.work = classify(gm, lens, L, k, m, max_len, repair)
        for g in singular:  # the build finds no inverse: failed like an under-determined group
            assert self.work[g]
            self.failed[g], self.invalid[g], self.work[g] = True, False, False
        self.nfail, self.ninv = int(self.failed.sum()), int(self.invalid.sum())
        dmark, pmark = gm[:, :k] == 1, gm[:, k:] == 1
        data = pc.batch_bytes(seed, G, k, max_len)
        par = pc.batch_bytes(seed + 1, G, m, max_len)
        data[dmark] = FILL
        par[pmark] = FILL
        plens = np.where(dmark, L[:, None], lens)  # a marked shard has room for L bytes
        self.data, self.par, self.plens = data, par, plens
        vp = self.vp = pv.VarPool(G, k, m, max_len, mode, seed + 2)
        fill_rows(vp, 0, data.reshape(G * k, max_len), plens)
        fill_rows(vp, G * k, par.reshape(G * m, max_len), np.repeat(Lc, m))
        for i in np.flatnonzero((plens.reshape(-1) == 0) & ~dmark.reshape(-1)):
            vp.alias[int(i)] = vp.guard_row  # a shard of length 0 is never dereferenced
        if tripwire:
            K = survivors(gm, k)
            status1 = ~self.failed & ((gm.sum(1) if repair else gm[:, :k].sum(1)) > 0)
            written = gm == 1 if repair else np.concatenate([dmark, np.zeros_like(pmark)], 1)
            idle = ~(K | written) | ~status1[:, None]
            g, s = np.nonzero(idle)
            self.idle = np.where(s < k, g * k + s, G * k + g * m + (s - k))
            for i in self.idle:
                vp.alias[int(i)] = vp.guard_row
        self.dl = np.where(dmark, pv.INT_MIN, lens)  # the entries of marked shards are not looked at
        self.marks = marks_to_rs_layout(gm, k)
        self.initial = vp.clone_host()
        self.expect = self.initial.copy()
        key = (seed, k, m, max_len, bool(repair), gm.tobytes(), lens.tobytes(), L.tobytes(),
               (code.rows if rows is None else rows).tobytes())
        if key not in _WRITES:
            for old in [o for o in _WRITES if o[1:4] != key[1:4]]:
                del _WRITES[old]  # one shape's references at a time
            _WRITES[key] = self._oracle_rows(oracle, code, rows)
        for i, n, row in _WRITES[key]:
            s = vp.pool.start[i]
            self.expect[s:s + n] = row

    def _oracle_rows(self, oracle, code, rows):
        """[(pool row, L, bytes)] of every row a call must write."""
        k, m, G, B = self.k, self.m, self.G, self.max_len
        out = []
        for g in np.flatnonzero(self.work):
            n = int(self.L[g])
            d = pv.zero_padded(self.data[g:g + 1], self.plens[g:g + 1])
            p = self.par[g:g + 1].copy()
            p[..., n:] = 0
            mk = np.ascontiguousarray(self.gm[g])
            if self.repair:
                assert rows is None
                d, p, nf = expected_repair(oracle, code, "cauchy", d, p, self.gm[g:g + 1], n)
                assert nf == 0
                out += [(G * k + g * m + j, n, p[0, j, :n].copy()) for j in np.flatnonzero(mk[k:])]
            else:
                rc = oracle.rs_reconstruct(code.rows if rows is None else rows, d, p, mk, n)
                assert rc == 0
            out += [(g * k + i, n, d[0, i, :n].copy()) for i in np.flatnonzero(mk[:k])]
        return out

    def row(self, flat, i, n=None):
        s = self.vp.pool.start[i]
        return flat[s:s + (self.max_len if n is None else n)]

    def describe(self, g):
        return f"[{self.groups[g][0]}, L={self.L[g]}, marks={np.flatnonzero(self.gm[g]).tolist()}]"


def crossed(k, m, max_len):
    """Every pattern of recon_marks under every pattern of length_patterns, coverage asserted."""
    gm = pc.recon_marks(k, m)
    pc.assert_marks_cover(gm, k, m)
    pats = pv.length_patterns(k, max_len)
    pv.assert_lengths_cover(pats + pv.void_patterns(k, max_len), k, max_len)
    return [(n, l.copy(), int(l.max()), q) for n, l in pats for q in gm]


def cycled(k, m, max_len):
    """One length pattern per marks pattern of recon_marks: the groups with work (status 1 under the
    reconstruct rule, hence under the repair rule too) take the patterns in turn, the others likewise,
    so that every pattern meets a group with work.  Asserts that, and at k > 64 that a survivor with id
    >= 64 has a partial column and another one length 0 in a group with work."""
    gm = pc.recon_marks(k, m)
    pc.assert_marks_cover(gm, k, m)
    pats = pv.length_patterns(k, max_len)
    pv.assert_lengths_cover(pats + pv.void_patterns(k, max_len), k, max_len)
    work = (gm.sum(1) <= m) & (gm[:, :k].sum(1) > 0)
    turn = {True: 0, False: 0}
    groups, met = [], set()
    for q, w in zip(gm, work):
        n, l = pats[turn[bool(w)] % len(pats)]
        turn[bool(w)] += 1
        groups.append((n, l.copy(), int(l.max()), q))
        if w:
            met.add(n)
    assert met == {n for n, _ in pats}, "every length pattern meets a group with work"
    if k > 64:
        part = zero = False
        for (n, l, L, q), w in zip(groups, work):
            hi = [i for i in range(64, k) if w and L > 0 and not q[i]]
            part |= any(l[i] % 16 and l[i] < L for i in hi)
            zero |= any(l[i] == 0 for i in hi)
        assert part and zero, "a partial column and a length 0 among the survivors with id >= 64"
    return groups
