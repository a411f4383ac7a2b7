"""Shared by the tests of the integrity family on pointer tables (qfec_verify_ptrs, qfec_locate_ptrs,
qfec_scrub_ptrs): the shapes the GPU tests walk and the coverage they promise, consistent batches in a
ptrs_common.Pool (encoded once per shape by the oracle, every test gets a copy of the image), the
damage kinds and where they land, and the CPU expectation of the verify bits.

A batch is a host image of the pool; row ids are rs.c's (ptrs_common).  Nothing here needs a device;
torch is imported by the GPU test alone."""
import functools

import numpy as np

import ptrs_common as pc

CLEAN, MULTI, AMBIGUOUS = -1, -2, -3

TEMPLATED = [(10, 3), (16, 4), (4, 2), (8, 4)]   # (16,4) takes its inputs in two halves
RUNTIME = [(9, 5), (5, 3)]                       # 5 rows: two chunks
VERIFY_ONLY = [(60, 8)]                          # k + m > 64: the table is read in place
LOCATE_ONLY = [(32, 32)]                         # every lane holds an address
BLOCKS = [1, 15, 16, 17, 1000, 1024, 1025, 1040, 1400]
MODES = ["aligned", "residues", "one-data", "one-parity"]
G_SMALL, G_LARGE = 37, 300


def cells():
    """[(k, m, B, mode, G)]: every code at B = 17, 1025, 1400; every mode at (10,3) and (9,5); every
    block size; the rest from one seeded draw; one case of 300 groups."""
    rng = np.random.default_rng(0x1D7E)
    codes = TEMPLATED + RUNTIME + VERIFY_ONLY + LOCATE_ONLY
    out = []
    for k, m in codes:
        for B in (17, 1025, 1400):
            out.append((k, m, B, MODES[int(rng.integers(len(MODES)))], G_SMALL))
    for mode in MODES:
        for k, m in ((10, 3), (9, 5)):
            out.append((k, m, BLOCKS[int(rng.integers(len(BLOCKS)))], mode, G_SMALL))
    for B in BLOCKS:
        k, m = (TEMPLATED + RUNTIME)[int(rng.integers(len(TEMPLATED + RUNTIME)))]
        out.append((k, m, B, MODES[int(rng.integers(len(MODES)))], G_SMALL))
    out.append((10, 3, 1000, "aligned", G_LARGE))
    return sorted(set(out))


def assert_coverage(cs):
    have = set((k, m, B) for k, m, B, _, _ in cs)
    for k, m in TEMPLATED + RUNTIME + VERIFY_ONLY + LOCATE_ONLY:
        for B in (17, 1025, 1400):
            assert (k, m, B) in have, (k, m, B)
    for mode in MODES:
        for km in ((10, 3), (9, 5)):
            assert any((k, m) == km and md == mode for k, m, _, md, _ in cs), (km, mode)
    assert set(BLOCKS) <= set(B for _, _, B, _, _ in cs)
    assert {G_SMALL, G_LARGE} == set(G for *_, G in cs)


def cell_id(c):
    return "k%d-m%d-B%d-%s-G%d" % c


def row_id(G, k, m, g, c):
    """Pool row of shard c (0 .. k + m - 1) of group g."""
    return g * k + c if c < k else G * k + g * m + (c - k)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle()


def encode(rows, data, B):
    par = np.zeros((data.shape[0], rows.shape[0], B), np.uint8)
    _oracle().rs_encode(rows, np.ascontiguousarray(data), par, B)
    return par


@functools.lru_cache(maxsize=None)
def _batch(rows_key, k, m, B, mode, G):
    rows = np.frombuffer(rows_key, np.uint8).reshape(m, k)
    data = pc.batch_bytes(k * 7 + m * 3 + B, G, k, B)
    par = encode(rows, data, B)
    pool = pc.Pool(G * (k + m), B, pc.offsets_for(mode, G, k, m), seed=k * 100 + B)
    pool.put_all(0, data.reshape(G * k, B))
    pool.put_all(G * k, par.reshape(G * m, B))
    pool.host.setflags(write=False)
    return pool


def batch(code, B, mode, G):
    """(pool, image): a consistent batch of `code`; the pool (its start[] and read-only host image) is
    shared, the image is the caller's own copy."""
    pool = _batch(np.ascontiguousarray(code.rows).tobytes(), code.k, code.m, B, mode, G)
    return pool, pool.host.copy()


def random_guards(pool, img, seed):
    """The image with every byte outside the rows replaced by seeded random bytes."""
    out = np.random.default_rng(seed).integers(0, 256, img.size, dtype=np.uint8)
    for s in pool.start:
        out[s:s + pool.B] = img[s:s + pool.B]
    return out


def split(pool, img, G, k, m):
    """(data [G, k, B], parity [G, m, B]) of an image."""
    return (pool.rows_of(img, 0, G * k).reshape(G, k, pool.B),
            pool.rows_of(img, G * k, G * m).reshape(G, m, pool.B))


def expected_bits(code, pool, img, G):
    """qfec_verify's word per group: the oracle's parity of the image's data against the image's
    parity, row by row."""
    data, par = split(pool, img, G, code.k, code.m)
    ref = encode(np.ascontiguousarray(code.rows), data, pool.B)
    bits = np.zeros(G, np.int64)
    for j in range(code.m):
        bits |= (ref[:, j] != par[:, j]).any(-1).astype(np.int64) << j
    return bits.astype(np.uint32).view(np.int32)


def spots(B):
    """The byte positions a damage kind hits, by name; a kind the block size has no room for is absent.
    first / last byte, the last byte of the last whole column, the first tail byte, one byte in slab 0
    and one in slab 1 (two waves report the same row), the whole row."""
    v = B // 16 * 16
    s = {"first": [0], "last": [B - 1], "row": list(range(B))}
    if v:
        s["col-end"] = [v - 1]
    if v < B:
        s["tail"] = [v]
    if B > 1024:
        s["two-slabs"] = [5, 1024 + (B - 1025) // 2]
    return s


def hit(pool, img, row, where, salt):
    """XOR non-zero bytes into the positions `where` of pool row `row`."""
    vals = (np.random.default_rng(salt).integers(0, 255, len(where)) + 1).astype(np.uint8)
    idx = pool.start[row] + np.asarray(where, np.int64)
    img[idx] ^= vals


def one_hot(culprit, G, k, m):
    """rs.c-layout marks of culprits [G] (a mark where the culprit is a shard id)."""
    out = np.zeros(G * (k + m), np.uint8)
    for g, c in enumerate(culprit):
        if c >= 0:
            out[row_id(G, k, m, g, int(c))] = 1
    return out


def random_damage(rng, pool, img, G, k, m, doubles):
    """In place: about a third of the groups get one corrupted shard at 1-4 random bytes; with
    `doubles` a few get two.  -> (expect [G], double [G] bool)."""
    n = k + m
    expect = np.full(G, CLEAN, np.int32)
    double = np.zeros(G, bool)
    for g in range(G):
        r = rng.random()
        cnt = 2 if doubles and r < 0.08 else 1 if r < 0.42 else 0
        ids = rng.choice(n, size=cnt, replace=False)
        for c in ids:
            where = rng.choice(pool.B, size=min(pool.B, int(rng.integers(1, 5))), replace=False)
            hit(pool, img, row_id(G, k, m, g, int(c)), where, int(rng.integers(1 << 30)))
        expect[g] = MULTI if cnt == 2 else int(ids[0]) if cnt == 1 else CLEAN
        double[g] = cnt == 2
    return expect, double
