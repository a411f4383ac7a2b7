"""Shared by the GPU tests of the plan calls on pointer tables (qfec_plan_apply_ptrs,
qfec_reconstruct_ptrs_wide, qfec_repair_ptrs_wide): a damaged batch in a guard-filled pool
(ptrs_common.Pool) and the pool the call must leave -- the pool before the call with only the rows
the call must write replaced: erased data rows by oracle.rs_reconstruct's, marked parity rows (repair)
by repair_common.expected_repair's.  The WHOLE pool is compared, so one byte outside [0, B) of a
written shard, or anywhere in an unwritten one, fails."""
import numpy as np

import ptrs_common as pc
from quicknet_amd.synth import marks_to_rs_layout
from repair_common import damage, expected_repair


_REFERENCE = {}  # the oracle's rows, computed once per batch and shared by the alignment modes


def put_rows(pool, flat, first, rows):
    """rows [count, B] into the pool image `flat` at rows first .. (Pool.put_all, vectorised)."""
    idx = pool.start[first:first + len(rows), None] + np.arange(pool.B)
    flat[idx] = rows


class Case:
    """G groups of (k, m), rows of B bytes: random data and parity (the parity is NOT the encode of
    the data: that pins which survivors are read), every marked row of both filled with 0x5A.
    extra: guard-filled rows after the batch's, 16-B aligned (row G * n is the tripwire)."""

    def __init__(self, seed, gm, k, m, B, mode, extra=0, tweak=None):
        self.k, self.m, self.B, self.gm = k, m, B, gm
        self.key = None if tweak else (seed, k, m, B, gm.tobytes())
        self.G, self.n = len(gm), k + m
        G, n = self.G, self.n
        self.marks = marks_to_rs_layout(gm, k)
        data = pc.batch_bytes(seed, G, k, B)
        par = pc.batch_bytes(seed + 1, G, m, B) if m else np.zeros((G, 0, B), np.uint8)
        if tweak:
            tweak(data, par)
        self.data, self.par = damage(data, par, gm)
        offs = np.concatenate([pc.offsets_for(mode, G, k, m), np.zeros(extra, np.int64)])
        self.pool = pc.Pool(G * n + extra, B, offs, seed + 2)
        put_rows(self.pool, self.pool.host, 0, self.data.reshape(G * k, B))
        put_rows(self.pool, self.pool.host, G * k, self.par.reshape(G * m, B))

    def expected(self, oracle, code, repair, rows=None):
        """(whole pool, data, parity, failed groups) after the call.  rows: the code's rows where the
        stale-row quirk matters (reconstruct only: oracle.rs_reconstruct has it)."""
        G, k, m, B = self.G, self.k, self.m, self.B
        rows = code.rows if rows is None else rows
        key = self.key and self.key + (bool(repair), rows.tobytes())
        if key in _REFERENCE:
            d, p, nfail = _REFERENCE[key]
        elif repair:
            d, p, nfail = expected_repair(oracle, code, "cauchy", self.data, self.par, self.gm, B)
        else:
            d, p = self.data.copy(), self.par
            oracle.rs_reconstruct(rows, d, self.par.copy(), self.marks, B)
            nfail = pc.oracle_failed(oracle, rows, self.data, self.par, self.gm, k, B)
        if key and key not in _REFERENCE:
            for old in [o for o in _REFERENCE if o[1:3] != key[1:3]]:
                del _REFERENCE[old]  # one code's references at a time
            _REFERENCE[key] = (d, p, nfail)
        assert nfail == int((self.gm.sum(1) > m).sum())
        flat = self.pool.host.copy()
        put_rows(self.pool, flat, 0, d.reshape(G * k, B))
        put_rows(self.pool, flat, G * k, p.reshape(G * m, B))
        return flat, d, p, nfail

    def survivors(self):
        """[G, n] bool: the k lowest unmarked ids of each group (all False where fewer than k are left)."""
        un = self.gm == 0
        K = un & (np.cumsum(un, 1) <= self.k)
        K[un.sum(1) < self.k] = False
        return K

    def untouched(self, repair):
        """Pool rows whose shards a plan neither reads nor writes: parity rows outside K (reconstruct),
        unmarked shards outside K (repair); rs.c row order."""
        G, k, m = self.G, self.k, self.m
        K = self.survivors()
        idle = ~K & (self.gm == 0) if repair else ~K
        if not repair:
            idle[:, :k] = False  # unmarked data is in K, marked data is written
        g, s = np.nonzero(idle)
        return np.where(s < k, g * k + s, G * k + g * m + (s - k))
