"""GPU tests of qfec_locate2 / qfec_scrub2: per group the one or two shards whose corruption explains
the syndromes; CLEAN / MULTI / AMBIGUOUS otherwise; marks in the rs.c layout that qfec_repair takes
unchanged; bytes past block_size never count.  Expected culprits come from how the damage was made,
and for the random batches from the brute-force expectation of locate2_common.py.

Run on an MI355X:  python -m pytest tests/test_gpu_locate2.py -m gpu -q
"""
import itertools

import numpy as np
import pytest

import quicknet_amd as qa
from quicknet_amd.synth import synth_bytes
from locate2_common import counts_of, expected_locate2, marks_of, random_damage
from repair_common import encoded, shard, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
CLEAN, MULTI, AMBIGUOUS = qa.QFEC_LOC_CLEAN, qa.QFEC_LOC_MULTI, qa.QFEC_LOC_AMBIGUOUS

# (flavour, k, m, B, pitch, G): one column; a masked tail; the (16,4) instance with 88 columns, so two
# column passes; the (8,4) instance; the runtime kernel with m >= 5; the byte kernel; the runtime
# kernel with the other matrix flavour; G = 301 so that the last block of the one-lane-per-group
# kernels is part empty
CASES = [("cauchy", 4, 4, 16, 16, 300), ("cauchy", 4, 4, 17, 32, 300), ("cauchy", 16, 4, 1400, 1424, 300),
         ("cauchy", 8, 4, 1024, 1040, 300), ("cauchy", 5, 5, 100, 128, 300), ("cauchy", 4, 4, 37, 37, 300),
         ("vandermonde", 10, 4, 1024, 1040, 300), ("cauchy", 8, 4, 1024, 1040, 301)]
CASES_M5 = [c for c in CASES if c[2] >= 5]  # distance >= 6: three corrupted shards never pass for two
case_params = pytest.mark.parametrize("flavour,k,m,B,pitch,G", CASES)
DISTANCE4_ROWS = [[1, 3, 3], [2, 1, 3], [4, 7, 3], [8, 5, 13]]


def locate2(code, data, par, B, counts=None, junk=False):
    """-> (culprit [G, 2], marks [G*n], counts [4]) on the host."""
    G, n = data.shape[0], code.k + code.m
    counts = torch.zeros(4, dtype=torch.int32, device=DEV) if counts is None else counts
    culprit = torch.full((G, 2), 0x5A5A5A5A, dtype=torch.int32, device=DEV) if junk else None
    marks = torch.full((G * n,), 0xEE if junk else 0, dtype=torch.uint8, device=DEV)
    out = code.locate2(data, par, B, culprit=culprit, marks=marks, counts=counts)
    torch.cuda.synchronize()
    assert culprit is None or out is culprit
    return out.cpu().numpy(), marks.cpu().numpy(), counts.cpu().numpy()


def pairs_of(k, m, most=59):
    """Pairs (a, b), a < b, of the three classes: all of them when they fit, else every parity pair,
    every data shard with a parity row (each row with data shards 0 and k-1), neighbouring and far
    data shards, topped up to 48 with seeded random ones."""
    n = k + m
    every = list(itertools.combinations(range(n), 2))
    if len(every) <= most:
        return every
    some = set(itertools.combinations(range(k, n), 2))
    some |= {(i, k + i % m) for i in range(k)} | {(0, k + j) for j in range(m)} | {(k - 1, k + j) for j in range(m)}
    some |= {(i, i + 1) for i in range(k - 1)} | {(0, k - 1)}
    rng = np.random.default_rng(k * 100 + m)
    while len(some) < 48:
        some.add(every[int(rng.integers(len(every)))])
    out = sorted(some)
    assert 40 <= len(out) <= most
    assert all(any((a >= k) + (b >= k) == c for a, b in out) for c in (0, 1, 2))
    return out


def damage_pair(data, par, g, a, b, B, kind):
    """The five patterns of two corrupted shards a, b in group g."""
    ra, rb = shard(data, par, g, a), shard(data, par, g, b)
    if kind == 0:    # the same byte
        ra[B // 2] ^= 0x3C
        rb[B // 2] ^= 0xC5
    elif kind == 1:  # both at byte 0 and at byte B-1 (the masked tail)
        ra[0] ^= 0x01
        rb[0] ^= 0x80
        ra[B - 1] ^= 0x7E
        rb[B - 1] ^= 0x11
    elif kind == 2:  # disjoint bytes as far apart as the row allows (different column passes at B = 1400)
        ra[1] ^= 0x55
        rb[B - 2] ^= 0xA7
    elif kind == 3:  # a on bytes {1, 2}, b on byte {2}
        ra[1] ^= 0x09
        ra[2] ^= 0x90
        rb[2] ^= 0x42
    else:            # whole rows: every byte changes
        ra[:B] ^= to_dev(synth_bytes(700 + a, B) | 1)
        rb[:B] ^= to_dev(synth_bytes(800 + b, B) | 1)


@case_params
def test_clean_batch(flavour, k, m, B, pitch, G):
    """Every slot CLEAN, marks all zero, counts zero; culprit and marks handed in full of junk come
    back fully overwritten; a byte flipped only in [B, pitch) of a data and of a parity row stays
    clean (pitch == B has no such byte)."""
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    culprit, marks, counts = locate2(code, data, par, B, junk=True)
    assert culprit.shape == (G, 2) and (culprit == CLEAN).all()
    assert marks.shape == (G * (k + m),) and not marks.any() and not counts.any()
    if pitch > B:
        data[7, k - 1, B] ^= 0x80
        par[G - 1, 0, pitch - 1] ^= 0x01
        culprit, marks, counts = locate2(code, data, par, B, junk=True)
        assert (culprit == CLEAN).all() and not marks.any() and not counts.any()


@case_params
def test_one_shard_every_id(flavour, k, m, B, pitch, G):
    """Each shard id gets a group of its own, corrupted in that shard alone: slot 0, the marks and
    counts[0] are qfec_locate's on the same batch, slot 1 is CLEAN."""
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    n = k + m
    expect = np.full(G, CLEAN, np.int32)
    for c in range(n):
        g = 2 + 12 * c  # n <= 20: below 300
        row = shard(data, par, g, c)
        if c % 3 == 0:
            row[c % B] ^= 0x01
        elif c % 3 == 1:
            row[1] ^= 0x55
            row[B - 1] ^= 0xA7
        else:
            row[:B] ^= to_dev(synth_bytes(900 + c, B) | 1)
        expect[g] = c
    ref_marks = torch.full((G * n,), 0xEE, dtype=torch.uint8, device=DEV)
    ref_counts = torch.zeros(3, dtype=torch.int32, device=DEV)
    ref = code.locate(data, par, B, marks=ref_marks, counts=ref_counts).cpu().numpy()
    assert np.array_equal(ref, expect)
    culprit, marks, counts = locate2(code, data, par, B, junk=True)
    assert np.array_equal(culprit[:, 0], ref) and (culprit[:, 1] == CLEAN).all()
    assert np.array_equal(marks, ref_marks.cpu().numpy())
    assert list(counts) == [int(ref_counts[0]), 0, 0, 0] and counts[0] == n


@case_params
def test_pairs(flavour, k, m, B, pitch, G):
    """Every pair of RS(4,4) and RS(5,5), at least 40 pairs of all three classes of the larger
    shapes; each pair has a group of its own and the damage patterns rotate.  Exactly (a, b), two
    marks per group, counts[1]; a second call on the same counts accumulates."""
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    pairs = pairs_of(k, m)
    expect = np.full((G, 2), CLEAN, np.int32)
    for x, (a, b) in enumerate(pairs):
        g = 1 + 5 * x
        damage_pair(data, par, g, a, b, B, (x + a) % 5)
        expect[g] = (a, b)
    culprit, marks, counts = locate2(code, data, par, B, junk=True)
    assert np.array_equal(culprit, expect)
    assert np.array_equal(marks, marks_of(expect, k, k + m)) and marks.sum() == 2 * len(pairs)
    assert list(counts) == [0, len(pairs), 0, 0]
    culprit, marks, counts = locate2(code, data, par, B, counts=to_dev(counts))
    assert np.array_equal(culprit, expect) and list(counts) == [0, 2 * len(pairs), 0, 0]
    bare = code.locate2(data, par, B)  # marks and counts are optional
    torch.cuda.synchronize()
    assert np.array_equal(bare.cpu().numpy(), expect)


@pytest.mark.parametrize("flavour,k,m,B,pitch,G", CASES_M5)
def test_three_shards_are_multi(flavour, k, m, B, pitch, G):
    """m >= 5 only: three corrupted shards of every mix of data and parity give MULTI, no marks."""
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    triples = [(0, 1, 2), (0, k - 1, k), (1, k, k + m - 1), (k, k + 1, k + 2), (2, 3, k + 1)]
    expect = np.full((G, 2), CLEAN, np.int32)
    for x, ids in enumerate(triples):
        g = 3 + 60 * x if x < 4 else G - 1
        for y, c in enumerate(ids):
            shard(data, par, g, c)[(5 * x + (y if x % 2 else 0)) % B] ^= 0x21 + 0x35 * y
        expect[g] = MULTI
    culprit, marks, counts = locate2(code, data, par, B, junk=True)
    assert np.array_equal(culprit, expect)
    assert not marks.any() and list(counts) == [0, 0, len(triples), 0]


def test_ambiguous_rows():
    """Explicit rows of distance exactly 4 (h_0 ^ h_1 ^ h_2 ^ e_0 = 0): the same value XORed into
    shards 0 and 1 at one byte is explained by {0, 1} and by {2, 3}: AMBIGUOUS, no marks.  Different
    values: the pair (0, 1).  One shard alone is located as ever."""
    code = qa.Code.from_rows(DISTANCE4_ROWS)
    G, B = 6, 64
    data = to_dev(synth_bytes(43, G * 3 * B).reshape(G, 3, B))
    par = torch.empty((G, 4, B), dtype=torch.uint8, device=DEV)
    code.encode(data, par)
    data[1, 0, 9] ^= 0x77
    data[1, 1, 9] ^= 0x77
    data[3, 0, 63] ^= 0x77
    data[3, 1, 63] ^= 0x78
    par[5, 2, 0] ^= 0x02
    culprit, marks, counts = locate2(code, data, par, B, junk=True)
    expect = np.array([[CLEAN, CLEAN], [AMBIGUOUS, AMBIGUOUS], [CLEAN, CLEAN], [0, 1], [CLEAN, CLEAN], [5, CLEAN]], np.int32)
    assert np.array_equal(culprit, expect)
    assert np.array_equal(marks, marks_of(expect, 3, 7))
    assert list(counts) == [1, 1, 0, 1]


@pytest.mark.parametrize("flavour,k,m,B,pitch,G", [CASES[1], CASES[3]])
def test_list_edges(flavour, k, m, B, pitch, G):
    """The list of MULTI groups full (every group two-damaged), and with one entry: only group 0,
    only group G-1.  (The empty list is test_clean_batch.)"""
    n = k + m
    pairs = list(itertools.combinations(range(n), 2))
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    expect = np.zeros((G, 2), np.int32)
    for g in range(G):
        a, b = pairs[(7 * g) % len(pairs)]
        shard(data, par, g, a)[g % B] ^= 1 + g % 255
        shard(data, par, g, b)[(3 * g + 1) % B] ^= 1 + (g + 9) % 255
        expect[g] = (a, b)
    culprit, marks, counts = locate2(code, data, par, B, junk=True)
    assert np.array_equal(culprit, expect)
    assert np.array_equal(marks, marks_of(expect, k, n)) and list(counts) == [0, G, 0, 0]
    for only in (0, G - 1):
        code, data, par = encoded(flavour, k, m, B, pitch, G)
        data[only, 0, 3] ^= 0x10
        par[only, 1, B - 1] ^= 0x04
        expect = np.full((G, 2), CLEAN, np.int32)
        expect[only] = (0, k + 1)
        culprit, marks, counts = locate2(code, data, par, B, junk=True)
        assert np.array_equal(culprit, expect)
        assert np.array_equal(marks, marks_of(expect, k, n)) and list(counts) == [0, 1, 0, 0]


def random_batch(flavour, k, m, B, pitch, G):
    """-> (code, original data, parity, damaged host data, parity, hits)."""
    code, d0, p0 = encoded(flavour, k, m, B, pitch, G)
    hd, hp = d0.cpu().numpy().copy(), p0.cpu().numpy().copy()
    hits = random_damage(np.random.default_rng(2000 * k + m + B), hd, hp, B, most=3 if m >= 5 else 2)
    assert all((hits == t).sum() >= 20 for t in range(4 if m >= 5 else 3))
    return code, d0.cpu().numpy(), p0.cpu().numpy(), hd, hp, hits


@case_params
def test_random_batch_against_brute_force(oracle, flavour, k, m, B, pitch, G):
    """0, 1 or 2 corrupted shards per group (3 too where m >= 5), random non-zero error bytes:
    culprit, marks and counts equal the brute-force expectation; none of these inputs is undefined."""
    code, _, _, hd, hp, hits = random_batch(flavour, k, m, B, pitch, G)
    expect = expected_locate2(oracle, code.rows, flavour, hd, hp, B)
    # the expectation itself agrees with how the damage was made
    assert np.array_equal((expect >= 0).sum(1), np.where(hits == 3, 0, hits))
    assert (expect[hits == 3] == MULTI).all() and (expect != AMBIGUOUS).all()
    culprit, marks, counts = locate2(code, to_dev(hd), to_dev(hp), B, junk=True)
    assert np.array_equal(culprit, expect)
    assert np.array_equal(marks, marks_of(expect, k, k + m))
    assert list(counts) == counts_of(expect)


@case_params
def test_scrub2(flavour, k, m, B, pitch, G):
    """The same random batch: after scrub2 every one- and two-damaged group equals the original in
    [0, B) of data and parity, every MULTI group its damaged self over the whole pitch, untouched
    groups too; verify afterwards flags exactly the MULTI groups.  d_culprit may be NULL."""
    code, d0, p0, hd, hp, hits = random_batch(flavour, k, m, B, pitch, G)
    dd, dp = to_dev(hd), to_dev(hp)
    counts = torch.zeros(4, dtype=torch.int32, device=DEV)
    culprit = code.scrub2(dd, dp, B, counts=counts)
    torch.cuda.synchronize()
    culprit = culprit.cpu().numpy()
    assert culprit.shape == (G, 2)
    assert np.array_equal((culprit >= 0).sum(1), np.where(hits == 3, 0, hits))
    assert list(counts.cpu().numpy()) == [(hits == 1).sum(), (hits == 2).sum(), (hits == 3).sum(), 0]
    rd, rp = dd.cpu().numpy(), dp.cpu().numpy()
    fixed, multi, none = (hits == 1) | (hits == 2), hits == 3, hits == 0
    assert np.array_equal(rd[fixed][..., :B], d0[fixed][..., :B])
    assert np.array_equal(rp[fixed][..., :B], p0[fixed][..., :B])
    assert np.array_equal(rd[multi], hd[multi]) and np.array_equal(rp[multi], hp[multi])
    assert np.array_equal(rd[none], hd[none]) and np.array_equal(rp[none], hp[none])
    bad = code.verify(dd, dp, B)
    torch.cuda.synchronize()
    assert np.array_equal(bad.cpu().numpy() != 0, multi)
    # the verdicts are optional
    dd2, dp2 = to_dev(hd), to_dev(hp)
    assert qa.lib().qfec_scrub2(code._h, dd2.data_ptr(), dp2.data_ptr(), G, B, pitch, None, None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dd2, dd) and torch.equal(dp2, dp)


@pytest.mark.parametrize("make,why", [(lambda: qa.Code.cauchy(4, 3), "m = 3"), (lambda: qa.Code.cauchy(21, 4), "k \\+ m = 25"),
                                      (lambda: qa.Code.from_rows([[1, 3, 2], [2, 1, 3], [4, 7, 3], [8, 5, 13]]),
                                       "linearly dependent")])
def test_refused_codes_launch_nothing(make, why):
    code = make()
    d = torch.zeros((2, code.k, 64), dtype=torch.uint8, device=DEV)
    p = torch.ones((2, code.m, 64), dtype=torch.uint8, device=DEV)
    with pytest.raises(qa.QfecError, match=why):
        code.locate2(d, p)
    with pytest.raises(qa.QfecError, match=why):
        code.scrub2(d, p)
    torch.cuda.synchronize()
    assert not d.any() and bool((p == 1).all())
