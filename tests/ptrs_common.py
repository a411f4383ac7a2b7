"""Shared by the GPU tests of the pointer-table calls (qfec_encode_ptrs / qfec_reconstruct_ptrs): the
rows of a batch carved out of one pool that is full of a guard byte, in a random permutation of
slots, each row at a chosen offset inside its slot with at least 32 guard bytes on either side.  A
test builds the expected pool on the CPU -- the pool before the call with only the rows the call must
write replaced by the oracle's bytes -- and compares the WHOLE pool, so a byte written outside
[0, block_size) of a written shard, or anywhere in an unwritten one, fails it.

Row order is rs.c's: data row (g, c) is row g * k + c, parity row (g, r) is row G * k + g * m + r.
"""
import numpy as np

from quicknet_amd.synth import synth_bytes

GUARD = 0xC3
SIDE = 32  # guard bytes before and after every row, at least


def offsets_for(mode, G, k, m):
    """Byte offset of every row inside its slot.  aligned: every row 16-B aligned; residues: row i at
    i % 16, so every residue occurs and every group is misaligned; one-data / one-parity: exactly one
    group (group 3) has exactly one misaligned pointer."""
    n = G * (k + m)
    if mode == "aligned":
        return np.zeros(n, np.int64)
    if mode == "residues":
        return np.arange(n, dtype=np.int64) % 16
    off = np.zeros(n, np.int64)
    g = min(3, G - 1)
    if mode == "one-data":
        off[g * k + 1] = 5
    elif mode == "one-parity":
        off[G * k + g * m + (m - 1)] = 9
    else:
        raise ValueError(mode)
    return off


class Pool:
    """nrows rows of B bytes in a guard-filled host pool; start[i] = the pool index of row i."""

    def __init__(self, nrows, B, offsets, seed):
        assert len(offsets) == nrows and 0 <= min(offsets) and max(offsets) < 16
        self.B = B
        self.slot = (SIDE + 15 + B + SIDE + 15) // 16 * 16
        perm = np.random.default_rng(seed).permutation(nrows)
        self.start = perm.astype(np.int64) * self.slot + SIDE + np.asarray(offsets, np.int64)
        self.host = np.full(nrows * self.slot, GUARD, np.uint8)
        # the layout keeps its promise: rows inside their slots, guards on both sides, no overlap
        lo, hi = self.start - perm * self.slot, self.start - perm * self.slot + B
        assert (lo >= SIDE).all() and (hi + SIDE <= self.slot).all()

    def put(self, i, row):
        self.host[self.start[i]:self.start[i] + self.B] = row

    def put_all(self, first, rows):
        for j, row in enumerate(rows):
            self.put(first + j, row)

    def rows_of(self, flat, first, count):
        """Rows first .. first + count - 1 of a pool image `flat` -> [count, B]."""
        return np.stack([flat[self.start[i]:self.start[i] + self.B] for i in range(first, first + count)])


def to_device(torch, dev, pool, alias=None):
    """(pool tensor, int64 address table).  alias: {row: row whose address it repeats}."""
    t = torch.from_numpy(pool.host).to(dev)
    assert t.data_ptr() % 16 == 0
    start = pool.start.copy()
    for i, j in (alias or {}).items():
        start[i] = start[j]
    return t, torch.from_numpy(t.data_ptr() + start).to(dev)


def padded(torch, dev, rows3, B):
    """[G, r, B] host rows -> the contiguous layout of qfec_encode / qfec_reconstruct, pitch round16(B)."""
    G, r, _ = rows3.shape
    out = np.zeros((G, r, (B + 15) // 16 * 16), np.uint8)
    out[..., :B] = rows3
    return torch.from_numpy(out).to(dev)


def batch_bytes(seed, G, rows, B):
    return synth_bytes(seed, G * rows * B).reshape(G, rows, B)


def recon_marks(k, m):
    """Deterministic group-order marks [G, k + m], G = 2 (m + 3): every erased-data count 0 .. m, a
    group with parity erasures only, under-determined groups (more than m marked), a group with
    exactly m erasures spread over data and parity, erased data next to an erased parity row 0 (the
    survivors then start at parity row 1)."""
    G = 2 * (m + 3)
    gm = np.zeros((G, k + m), np.uint8)
    g = 1                                   # group 0: nothing
    for e in range(1, m + 1):               # e = 1 .. m data rows, spaced
        gm[g, [(2 * j + e) % k for j in range(e)]] = 1
        g += 1
    gm[g, k] = 1                            # parity only
    g += 1
    gm[g, :m] = 1                           # m data + 1 parity: m + 1 marked
    gm[g, k + m - 1] = 1
    g += 1
    nd = (m + 1) // 2                       # exactly m, over data and parity
    gm[g, k - nd:k] = 1
    gm[g, k:k + m - nd] = 1
    g += 1
    gm[g, :m + 1] = 1                       # m + 1 data rows
    g += 1
    gm[g, k - m:k] = 1                      # the last m data rows
    g += 1
    for e in range(1, m + 1):               # e data rows and parity row 0 (m + 1 marked when e = m)
        gm[g, [(2 * j + 1) % k for j in range(e)]] = 1
        gm[g, k] = 1
        assert gm[g, :k].sum() == e and gm[g - m - 5, :k].sum() == e
        g += 1
    assert g == G
    return gm


def assert_marks_cover(gm, k, m):
    """The coverage the reconstruct tests rely on, checked on the marks themselves."""
    e = gm[:, :k].sum(1)
    t = gm.sum(1)
    assert set(range(m + 1)) <= set(e[t <= m].tolist()), "every erased-data count 0 .. m among recoverable groups"
    assert ((e == 0) & (gm[:, k:].sum(1) > 0)).any(), "a group with parity erasures only"
    assert (t > m).any(), "an under-determined group"
    assert ((t == m) & (e > 0) & (e < m)).any(), "exactly m erasures over data and parity"
    assert (t == 0).any(), "an untouched group"


def oracle_failed(oracle, rows, data, par, gm, k, B):
    """How many groups the oracle leaves under-determined: one call per group."""
    count = 0
    for g in range(len(gm)):
        d, p = data[g:g + 1].copy(), par[g:g + 1].copy()
        count += oracle.rs_reconstruct(rows, d, p, np.ascontiguousarray(gm[g]), B) == -1
    return count
