"""Shared by test_gpu_dispatch.py and test_dispatch_table.py: the shapes, layouts, guarded device
buffers, damage plans and expectations that take the integrity and update calls (verify, locate,
locate_erased, locate2, repair, the scrubs, update, encode_update) down every kernel the host can
pick -- a templated (k, m) instance, the runtime-k,m kernel, the byte-granular kernel -- and through
the second pass of every 64-column loop.

Every expectation comes from the oracle's encode / reconstruct / multiply (locate2_common,
repair_common) or from how the damage was made; none from device output or the library's tables.
torch is imported inside the helpers that need it, so the CPU suite can import this module."""
import collections
import functools

import numpy as np

from locate2_common import AMBIGUOUS, CLEAN, MULTI, columns, mul_table, syndromes
from quicknet_amd.synth import synth_bytes

# ------------------------------------------------------------------ layouts

# B, pitch, and the byte offset mod 16 of the data, parity and rows / part bases
Layout = collections.namedtuple("Layout", "name B pitch data_off parity_off rows_off")

LAYOUTS = {l.name: l for l in (
    Layout("fast", 100, 128, 0, 0, 0),               # 16-B kernels, 7 columns, masked tail of 4 bytes
    Layout("fast-wide", 1100, 1120, 0, 0, 0),        # 69 columns: a second pass with 5 live lanes; wpg = 2, wpg8 = 3
    Layout("bytes-pitch", 300, 300, 0, 0, 0),        # byte kernels: two 256-lane blocks, five wave passes per row
    Layout("bytes-data-off", 100, 128, 1, 0, 0),     # byte path by the data base alone; second pass of 36 lanes
    Layout("bytes-parity-off", 100, 128, 0, 8, 0),   # byte path by the parity base alone
    Layout("bytes-rows-off", 100, 128, 0, 0, 4),     # update / encode_update only: by the rows / part base alone
)}
WIDE = ("fast-wide", "bytes-pitch", "bytes-data-off", "bytes-parity-off")
OFF_BASE = ("bytes-data-off", "bytes-parity-off", "bytes-rows-off")


def byte_path(layout):
    """Does the host pick the byte-granular kernels on this layout?"""
    return bool(layout.pitch % 16 or layout.data_off or layout.parity_off or layout.rows_off)


def lanes(layout):
    """Lanes per row of the flat mapping: bytes on the byte path, 16-B columns otherwise."""
    return layout.B if byte_path(layout) else (layout.B + 15) // 16


def written_from(layout):
    """The first byte of a row that no call may write: B on the byte path (one lane per byte of
    [0, B)), the end of the last 16-B column otherwise."""
    return layout.B if byte_path(layout) else (layout.B + 15) // 16 * 16


def groups_for(k, m):
    """The odd one of 3n + 2 and 3n + 3: a group of its own for every shard id with clean groups
    between them, never a multiple of 4 (the last block of a one-wave-per-group launch is part empty)."""
    n = k + m
    return 3 * n + 2 if (3 * n + 2) % 2 else 3 * n + 3


# ------------------------------------------------------------------ shape sets

# the (k, m) instance lists of quicknet_amd/csrc/*.hip, literally (test_dispatch_table.py holds them
# to the source); update: one shape per rung of the a.m == 1..4 ladder of qfec_update.hip
INSTANCES = {
    "verify": [(10, 3), (16, 4), (4, 2), (2, 1), (2, 2), (3, 1), (3, 2), (4, 1), (5, 1), (5, 3), (6, 2), (7, 1), (8, 2),
               (8, 4), (12, 4), (20, 4)],
    "locate": [(10, 3), (16, 4), (4, 2), (2, 2), (3, 2), (5, 3), (6, 2), (8, 2), (8, 4), (12, 4), (20, 4)],
    "locate2": [(16, 4), (8, 4), (12, 4), (20, 4)],
    "locate_erased": [(10, 3), (16, 4), (4, 2), (3, 2), (8, 4), (12, 4), (5, 3), (6, 2), (8, 2), (20, 4)],
    "repair": [(10, 3), (16, 4), (4, 2), (2, 1), (3, 2), (8, 4), (12, 4), (5, 3), (6, 2), (7, 1), (8, 2), (20, 4)],
    "update": [(7, 1), (6, 2), (10, 3), (16, 4)],
}
# no instance in any family: one row chunk of 4, and two
GENERIC = {f: [(7, 3), (6, 5)] for f in INSTANCES}
GENERIC["locate2"] = [(6, 5), (7, 4)]
N24 = [(20, 4), (19, 5)]  # the edge of everything keyed by an n-bit mask
LIMITS = {
    "verify": [(4, 32), (32, 32)],                     # bit 31 of bad_rows
    "locate": [(32, 2), (2, 32), (32, 32)] + N24,      # ids and marks >= 32; N24: the scrub
    "locate2": N24,
    "locate_erased": N24,
    "repair": N24,
    "update": [(7, 1), (6, 2), (254, 1)],
}
# the QFEC_ENC_CASE entries that no encode test names
ENCODE_EXTRA = [(2, 2), (3, 1), (4, 1), (5, 1), (5, 3), (8, 4)]


def cases(family):
    """[(k, m, layout name)]: every instance on fast; an instance with the family's smallest m,
    (20,4) and the generic shapes on fast and the four wide / byte layouts; the limits on fast and
    bytes-data-off; update also on bytes-rows-off."""
    first = (8, 4) if family == "locate2" else (10, 3)
    wide = [first, (20, 4)] + GENERIC[family]
    out = [(k, m, "fast") for k, m in INSTANCES[family] + wide]
    out += [(k, m, l) for k, m in wide for l in WIDE]
    out += [(k, m, l) for k, m in LIMITS[family] for l in ("fast", "bytes-data-off")]
    if family == "update":
        out += [(k, m, "bytes-rows-off") for k, m in wide + LIMITS[family]]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


def case_ids(family, names=None):
    return [f"{names or family}-{k}-{m}-{l}" for k, m, l in cases(family)]


# ------------------------------------------------------------------ guarded device buffers

GUARD = 256


def guard_pattern(nbytes):
    return ((np.arange(nbytes, dtype=np.int64) * 37 + 11) & 0xFF).astype(np.uint8)


class Guarded:
    """A host array placed on the device as a contiguous view into a larger flat uint8 tensor, its
    base `off` bytes past a 16-B boundary, with GUARD bytes of a fixed pattern before and after."""

    def __init__(self, host, off=0):
        import torch

        host = np.ascontiguousarray(host)
        assert host.dtype == np.uint8 and 0 <= off < 16
        n = host.size
        self.flat = torch.empty(GUARD + n + GUARD + 32, dtype=torch.uint8, device="cuda:0")
        self.start = (-self.flat.data_ptr()) % 16 + GUARD + off
        self.n = n
        self.pattern = guard_pattern(self.flat.numel())
        self.flat.copy_(torch.from_numpy(self.pattern))
        self.t = self.flat[self.start:self.start + n].view(host.shape)
        self.t.copy_(torch.from_numpy(host))
        # a change in the allocator must not silently turn the case into an aligned one
        assert self.t.data_ptr() % 16 == off and self.t.is_contiguous()

    def host(self):
        return self.t.cpu().numpy()

    def check_guards(self, what=""):
        end = self.start + self.n
        head, tail = self.flat[:self.start].cpu().numpy(), self.flat[end:].cpu().numpy()
        assert np.array_equal(head, self.pattern[:self.start]), f"{what}: bytes before the buffer written"
        assert np.array_equal(tail, self.pattern[end:]), f"{what}: bytes after the buffer written"


def check_all(bufs, what):
    for name, b in bufs.items():
        b.check_guards(f"{what} {name}")


# ------------------------------------------------------------------ consistent batches

@functools.lru_cache(maxsize=None)
def _batch(oracle, k, m, B, pitch, G):
    rows = oracle.cauchy(k, m)
    data = synth_bytes(k * 3 + m + B, G * k * pitch).reshape(G, k, pitch).copy()
    par = synth_bytes(k * 5 + m + B, G * m * pitch).reshape(G, m, pitch).copy()  # garbage in [B, pitch)
    tmp = np.zeros_like(par)
    oracle.rs_encode(rows, data, tmp, B)
    par[..., :B] = tmp[..., :B]
    for a in (rows, data, par):
        a.setflags(write=False)
    return rows, data, par


def batch(oracle, k, m, layout):
    """(rows [m, k], data [G, k, pitch], parity [G, m, pitch]) on the host: the oracle's Cauchy rows,
    seeded data, the oracle's parity over [0, B) and garbage in [B, pitch) of both.  Computed once
    per shape and row geometry; every caller gets copies of the two buffers."""
    rows, data, par = _batch(oracle, k, m, layout.B, layout.pitch, groups_for(k, m))
    return rows, data.copy(), par.copy()


def shard(data, par, g, c):
    """Row c of group g over all n shards (a view)."""
    k = data.shape[1]
    return data[g, c] if c < k else par[g, c - k]


# ------------------------------------------------------------------ damage

def second_pass(B):
    """The first bytes of later passes of the 64-lane loops at this B: byte 1024 where 16-B columns
    make a second pass, byte 64 where the byte kernels do, byte 256 where a row leaves a 256-lane block."""
    return [1024] if B > 1024 else [64, 256] if B > 256 else [64]


def damage_kinds(B):
    """[(name, [(byte, xor)] or None = the whole row)]: byte 0, byte B - 1, the first byte of every
    later pass, two bytes in different passes, the whole row."""
    return ([("b0", [(0, 0x01)]), ("last", [(B - 1, 0x80)])] + [(f"b{p}", [(p, 0x3C)]) for p in second_pass(B)] +
            [("two", [(1, 0x55), (B - 2, 0xA7)]), ("row", None)])


def hit(row, kind, B, seed):
    """Apply one damage kind to a host row in place, inside [0, B) only."""
    if kind is None:
        row[:B] ^= synth_bytes(900 + seed, B) | 1  # every byte changes
    else:
        for b, x in kind:
            assert 0 <= b < B
            row[b] ^= x


def damage_every_shard(data, par, B):
    """In place: shard c damaged in group 3c + 1, the kind rotating over the ids, every other group
    clean.  -> culprit [G] by construction."""
    G, k = data.shape[:2]
    n = k + par.shape[1]
    kinds = damage_kinds(B)
    culprit = np.full(G, CLEAN, np.int32)
    for c in range(n):
        hit(shard(data, par, 3 * c + 1, c), kinds[(c + k) % len(kinds)][1], B, c)
        culprit[3 * c + 1] = c
    return culprit


# ------------------------------------------------------------------ expectations

def bad_rows_model(oracle, rows, data, par, B):
    """qfec_verify's word per group: bit j = parity row j differs from the oracle's encode in [0, B)."""
    s = syndromes(oracle, rows, "cauchy", data, par, B)
    bad = s.any(axis=2)  # [G, m]
    return (bad.astype(np.uint64) << np.arange(bad.shape[1], dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def explains(h, s):
    """Is every column of s [m, N] a multiple of h (m ints, not all zero)?  With p a row where h is
    non-zero: h[p] x s[j] == h[j] x s[p] for every j, by the oracle's multiply."""
    mul = mul_table()
    h = np.asarray(h, np.int64)
    p = int(np.nonzero(h)[0][0])
    return not (mul[h[p], s] ^ mul[h[:, None], s[p][None, :]]).any()


def expected_locate1(oracle, rows, data, par, B):
    """What qfec_locate must answer: culprit [G].  The single-shard stage of
    locate2_common.expected_locate2 without the pair enumeration, so it also serves k + m > 24."""
    h = columns(rows)
    s_all = syndromes(oracle, rows, "cauchy", data, par, B)
    out = np.full(len(data), CLEAN, np.int32)
    for g in np.nonzero(s_all.any(axis=(1, 2)))[0]:
        s = s_all[g][:, s_all[g].any(axis=0)]
        one = [x for x in range(len(h)) if explains(h[x], s)]
        out[g] = one[0] if len(one) == 1 else AMBIGUOUS if one else MULTI
    return out


def counts_of1(culprit):
    """[located, multi, ambiguous] of culprit [G]."""
    return [int((culprit >= 0).sum()), int((culprit == MULTI).sum()), int((culprit == AMBIGUOUS).sum())]


def marks_n(culprit, n):
    """Group-order marks [G, n] with one mark per shard id >= 0 in culprit [G] or [G, slots]."""
    c = culprit.reshape(len(culprit), -1)
    gm = np.zeros((len(c), n), np.uint8)
    for slot in range(c.shape[1]):
        ok = c[:, slot] >= 0
        gm[np.nonzero(ok)[0], c[ok, slot]] = 1
    return gm


def oracle_parity(oracle, rows, data, B):
    """The oracle's encode of host data [G, k, pitch] -> parity [G, m, B]."""
    data = np.ascontiguousarray(data)
    out = np.zeros((data.shape[0], rows.shape[0], data.shape[2]), np.uint8)
    oracle.rs_encode(rows, data, out, B)
    return out[..., :B]


# ------------------------------------------------------------------ damage plans of the two-shard and erased calls

def locate2_damage(data, par, B):
    """In place, for qfec_locate2.  Pairs a < b with a damaged only in bytes of the first pass and b
    only in bytes of a later one (data-data, data-parity, parity-parity: no single pass names the
    pair), pairs damaged in the same byte, single shards, and with m >= 5 one three-shard group.
    Every second group is damaged.  -> [(group, its two verdict slots by construction)]; the test's
    expectation is locate2_common.expected_locate2's, which must agree."""
    G, k = data.shape[:2]
    m = par.shape[1]
    n = k + m
    p2 = second_pass(B)[-1]
    assert 17 < min(second_pass(B)) and p2 + 1 < B - 1
    split = [(0, k - 1), (k // 2, k + 1), (k, n - 1), (1, 2), (k - 1, k), (k + 1, k + 2)]
    same = [(0, 1, p2), (2, n - 1, 0), (k, k + 1, B - 1)]
    made = []
    for a, b in split:
        assert 0 <= a < b < n
        g = 1 + 2 * len(made)
        hit(shard(data, par, g, a), [(0, 0x1D), (17, 0x80)], B, g)
        hit(shard(data, par, g, b), [(p2, 0x6B), (B - 1, 0x02)], B, g)
        made.append((g, (a, b)))
    for a, b, at in same:
        g = 1 + 2 * len(made)
        hit(shard(data, par, g, a), [(at, 0x21)], B, g)
        hit(shard(data, par, g, b), [(at, 0x9E)], B, g)
        made.append((g, (a, b)))
    for c, kind in ((3, damage_kinds(B)[-2][1]), (n - 2, None), (k - 1, [(p2, 0xFF)])):
        g = 1 + 2 * len(made)
        hit(shard(data, par, g, c), kind, B, g)
        made.append((g, (c, CLEAN)))
    if m >= 5:
        g = 1 + 2 * len(made)
        for c, at in ((0, 0), (k, p2), (1, B - 1)):
            hit(shard(data, par, g, c), [(at, 0x47)], B, g)
        made.append((g, (MULTI, MULTI)))
    assert made[-1][0] < G
    return made


def erased_damage(data, par, B, seed):
    """In place, for qfec_locate_erased: shard c damaged in group 3c + 1 beside 0 .. m - 2 lost shards
    (their rows junk over the whole pitch); clean groups with lost shards; group 0: a culprit damaged
    in the first and in a later pass beside m - 2 lost shards; group 3 (m >= 3): two corrupted
    survivors damaged in different passes with every spare left, which must come out MULTI.
    -> (gm [G, n] with non-zero = lost, culprit [G] by construction)."""
    G, k, pitch = data.shape
    m = par.shape[1]
    n = k + m
    rng = np.random.default_rng(seed)
    kinds = damage_kinds(B)
    gm = np.zeros((G, n), np.uint8)
    expect = np.full(G, CLEAN, np.int32)

    def lose(g, t, keep):
        ids = rng.choice([i for i in range(n) if i not in keep], size=t, replace=False)
        gm[g, ids] = rng.integers(1, 256, size=t)
        for c in ids:
            shard(data, par, g, c)[:] = rng.integers(0, 256, size=pitch, dtype=np.uint8)

    for c in range(n):
        g = 3 * c + 1
        lose(g, int(rng.integers(0, m - 1)), (c,))
        hit(shard(data, par, g, c), kinds[(c + m) % len(kinds)][1], B, c)
        expect[g] = c
        if c % 2 == 0:
            lose(g + 1, int(rng.integers(0, m - 1)), ())
    lose(0, m - 2, (k - 1,))
    hit(shard(data, par, 0, k - 1), [(1, 0x55), (second_pass(B)[-1], 0x10), (B - 2, 0xA7)], B, 0)
    expect[0] = k - 1
    if m >= 3:
        hit(shard(data, par, 3, 0), [(0, 0x10)], B, 3)
        hit(shard(data, par, 3, n - 1), [(B - 1, 0x04)], B, 3)
        expect[3] = MULTI
    return gm, expect


def erased_marks(gm, culprit):
    """Group-order: the marks as 0 / 1 plus 1 at every located culprit."""
    out = (gm != 0).astype(np.uint8)
    ok = culprit >= 0
    out[np.nonzero(ok)[0], culprit[ok]] = 1
    return out


# ------------------------------------------------------------------ update

UPD_NONE = -1


def update_ids(k, G):
    """Groups 0 and G - 1 touched, ids 0 and k - 1 both present, every third group untouched."""
    s = np.array([(g * 7) % k for g in range(G)], np.int32)
    s[1::3] = UPD_NONE
    s[0], s[G - 1] = 0, k - 1
    return s


def apply_rows(data, ids, rows, B):
    """Host copy of data [G, k, pitch] with row ids[g] of every touched group replaced in [0, B)."""
    out = data.copy()
    on = np.nonzero(ids >= 0)[0]
    out[on, ids[on], :B] = rows[on, :B]
    return out
