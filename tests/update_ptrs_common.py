"""Shared by the GPU tests of incremental parity on pointer tables (qfec_encode_update_ptrs,
qfec_update_ptrs and their forms with per-shard lengths).  The rows of a batch, the rows d_new points at
included, live in one ptrs_var_common.VarPool: guard-filled, slots permuted, every row written to its
own length only.  A test builds the expected pool on the CPU and compares the WHOLE pool, so a byte
written outside a stated extent, or a byte read past a length that reaches a result, fails it.  Table
entries a call must not address point at the misaligned guard row (never NULL: a wrong kernel must
fail a compare, not fault), which must come back untouched.

Row order: data row (g, c) is row g * k + c, parity row (g, r) is row G * k + g * m + r, the guard row
is row G * (k + m), and new row (round j, group g) is row G * (k + m) + 1 + j * G + g.
"""
import numpy as np

import ptrs_common as pc
import ptrs_var_common as pv

INT_MIN, INT_MAX = pv.INT_MIN, pv.INT_MAX
NONE = -1
MODES = ["aligned", "residues", "one-data", "one-parity", "one-new"]


class UpdPool(pv.VarPool):
    """VarPool plus `rounds` * G rows for d_new.  Mode one-new: every shard is aligned and only the new
    row of one group (group 3, or the last) is not."""

    def __init__(self, G, k, m, max_len, mode, seed, rounds=1):
        base_mode = "aligned" if mode == "one-new" else mode
        super().__init__(G, k, m, max_len, base_mode, seed)  # the fields; the pool is rebuilt with the new rows
        new_offs = np.zeros(rounds * G, np.int64)
        if mode == "one-new":
            new_offs[np.arange(rounds) * G + min(3, G - 1)] = 11
        elif mode == "residues":
            new_offs = (np.arange(rounds * G, dtype=np.int64) * 5 + 3) % 16
        base = pc.offsets_for(base_mode, G, k, m)
        offs = np.concatenate([base, [pv.GUARD_ROW_OFFSET], new_offs])
        self.pool = pc.Pool(self.nrows + 1 + rounds * G, max_len, offs, seed)

    def data_row(self, g, c):
        return g * self.k + c

    def parity_row(self, g, r):
        return self.G * self.k + g * self.m + r

    def new_row(self, g, j=0):
        return self.nrows + 1 + j * self.G + g

    def upload(self, torch, dev):
        """(pool tensor, host int64 addresses of every row): a test cuts its tables out of them."""
        t = torch.from_numpy(self.pool.host).to(dev)
        assert t.data_ptr() % 16 == 0
        addr = t.data_ptr() + self.pool.start
        assert addr[self.guard_row] % 16 != 0, "the guard row is misaligned"
        return t, addr

    def table(self, addr, keep_data=None, dead_groups=()):
        """The qfec_encode_ptrs table as host int64.  keep_data: bool [G, k], the data entries the call
        may address; every other data entry, and every entry of a group in dead_groups, is the guard
        row's address."""
        tab = addr[:self.nrows].copy()
        guard = addr[self.guard_row]
        if keep_data is not None:
            tab[:self.G * self.k][~np.asarray(keep_data, bool).reshape(-1)] = guard
        for g in dead_groups:
            tab[g * self.k:(g + 1) * self.k] = guard
            tab[self.G * self.k + g * self.m:self.G * self.k + (g + 1) * self.m] = guard
        return tab

    def write(self, flat, i, row, n, at=0):
        """Bytes [at, n) of row i of the pool image `flat` become row[at:n]."""
        s = self.pool.start[i]
        if n > at:
            flat[s + at:s + n] = row[at:n]


def encode_padded(oracle, rows, data, lens, B, cols=None):
    """The oracle's encode of data [G, k, B] zero-padded from lens [G, k] on, over the data columns in
    `cols` alone (a bool [k]; None: all): the rows outside it count as zero -> parity [G, m, B]."""
    z = pv.zero_padded(data, lens)
    if cols is not None:
        z[:, ~np.asarray(cols, bool)] = 0
    out = np.zeros((data.shape[0], rows.shape[0], B), np.uint8)
    oracle.rs_encode(rows, np.ascontiguousarray(z), out, B)
    return out


def shard_ids(k, G):
    """tests/test_gpu_update.py's pattern: groups 0 and G-1 touched, ids 0 and k-1 both present, every
    third group untouched."""
    s = np.array([(g * 7) % k for g in range(G)], np.int32)
    s[1::3] = NONE
    s[0], s[G - 1] = 0, k - 1
    return s


def assert_ids_cover(s, k, G):
    assert s[0] >= 0 and s[G - 1] >= 0 and (s == 0).any() and (s == k - 1).any()
    assert (s[1:G - 1:3] == NONE).all() and (s < 0).any()


def partitions(k):
    """Every two-way partition of [0, k) and one three-way: lists of (first, count)."""
    out = [[(0, a), (a, k - a)] for a in range(1, k)]
    if k >= 3:
        a, b = max(1, k // 3), max(2, k - 1)
        out.append([(0, a), (a, b - a), (b, k - b)])
    for p in out:
        assert p[0][0] == 0 and sum(c for _, c in p) == k and all(c >= 1 for _, c in p)
        assert all(p[i][0] + p[i][1] == p[i + 1][0] for i in range(len(p) - 1))
    return out


def range_mask(k, first, count):
    m = np.zeros(k, bool)
    m[first:first + count] = True
    return m


# ---------------------------------------------------------------- per-group patterns with lengths

def update_patterns(k, max_len):
    """[(name, lens[k] before, i, n, L)] of valid groups of qfec_update_ptrs_var."""
    half, full = (max_len + 1) // 2, np.full(k, max_len, np.int64)
    pats = []

    def add(name, lens, i, n, L=max_len):
        lens = np.asarray(lens, np.int64).copy()
        assert 0 <= i < k and 0 <= n <= L <= max_len and 0 <= lens[i] <= L, name
        pats.append((name, lens, i, n, L))

    add("shrink", full, 0, half)
    add("grow-to-L", np.full(k, half), 1 % k, max_len)
    add("same", np.full(k, half), k - 1, half)
    add("to-empty", full, 0, 0)
    lens = pv.ladder(k, max_len)
    lens[0] = 0
    add("from-empty", lens, 0, half)
    add("both-empty", np.zeros(k), k - 1, 0)
    add("both-empty-L0", np.zeros(k), 0, 0, 0)
    lens = np.maximum(max_len // 3 - np.arange(k, dtype=np.int64), 0)
    lens[k // 2] = max_len
    add("longest-shrinks", lens, k // 2, max(max_len // 5, 1))
    add("ladder", pv.ladder(k, max_len), min(2, k - 1), min(max_len, 7))
    add("tight-L", np.full(k, half), 0, half // 2 + 1, half)
    for b in (16, 1024, 1025):
        if b + 1 <= max_len:
            add(f"o={b}", np.full(k, b), 1 % k, max(b - 9, 1))
            add(f"n={b}", np.full(k, 3), 0, b)
            add(f"o={b + 1},n={b}", np.full(k, b + 1), k - 1, b)
    return pats


def assert_updates_cover(pats, k, max_len):
    """The (o, n) pairs the issue lists, checked on the patterns themselves."""
    on = [(int(l[i]), int(n), int(L), l) for _, l, i, n, L in pats]
    assert any(n < o for o, n, _, _ in on) and any(n > o for o, n, _, _ in on) and any(n == o > 0 for o, n, _, _ in on)
    assert any(n == 0 and o > 0 for o, n, _, _ in on), "n = 0"
    assert any(o == 0 and n > 0 for o, n, _, _ in on), "o = 0"
    assert any(o == 0 and n == 0 and L > 0 for o, n, L, _ in on) and any(L == 0 for _, _, L, _ in on), "both 0"
    assert any(n == L > 0 for _, n, L, _ in on), "n = L"
    assert any(o == l.max() and (l == o).sum() == 1 and n < np.sort(l)[-2] for o, n, _, l in on if len(l) > 1), \
        "the group's longest shard shrinking below the next one"
    borders = [b for b in (16, 1024, 1025) if b + 1 <= max_len]
    for b in borders:
        assert any(o == b for o, _, _, _ in on) and any(n == b for _, n, _, _ in on), f"o and n at {b}"
    if max_len >= 17:
        assert borders, "a 16-B border"
