"""GPU tests of qfec_locate / qfec_scrub: per group the one shard, data or parity, whose corruption
explains the syndromes; CLEAN / MULTI / AMBIGUOUS otherwise; one-hot marks in the rs.c layout that
qfec_repair takes unchanged; bytes past block_size never count.  Expected culprits come from how
the damage was made.

Run on an MI355X:  python -m pytest tests/test_gpu_locate.py -m gpu -q
"""
import numpy as np
import pytest

import quicknet_amd as qa
from quicknet_amd.synth import synth_bytes
from repair_common import encoded, one_hot_marks, shard, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
CLEAN, MULTI, AMBIGUOUS = qa.QFEC_LOC_CLEAN, qa.QFEC_LOC_MULTI, qa.QFEC_LOC_AMBIGUOUS

# (flavour, k, m, B, pitch, G): the templated kernel; two-half inputs with a masked tail column and
# 88 columns per group, so that groups straddle waves and blocks; the generic kernel; the byte
# kernel (pitch 37; 37 lanes per group, so groups straddle waves there too); G = 301 so that the
# last block is part empty; the other matrix flavour
CASES = [("cauchy", 10, 3, 1024, 1040, 300), ("cauchy", 16, 4, 1400, 1424, 300), ("cauchy", 9, 5, 100, 128, 300),
         ("cauchy", 4, 2, 37, 37, 300), ("cauchy", 10, 3, 1024, 1040, 301), ("vandermonde", 10, 3, 1024, 1040, 300)]
CASES_M3 = [c for c in CASES if c[2] >= 3]  # distance >= 4: two corrupted shards never pass for one
case_params = pytest.mark.parametrize("flavour,k,m,B,pitch,G", CASES)


def locate(code, data, par, B, counts=None, junk=False):
    """-> (culprit [G], marks [G*n], counts [3]) on the host."""
    G, n = data.shape[0], code.k + code.m
    counts = torch.zeros(3, dtype=torch.int32, device=DEV) if counts is None else counts
    culprit = torch.full((G,), 0x5A5A5A5A, dtype=torch.int32, device=DEV) if junk else None
    marks = torch.full((G * n,), 0xEE if junk else 0, dtype=torch.uint8, device=DEV)
    out = code.locate(data, par, B, culprit=culprit, marks=marks, counts=counts)
    torch.cuda.synchronize()
    assert culprit is None or out is culprit
    return out.cpu().numpy(), marks.cpu().numpy(), counts.cpu().numpy()


@case_params
def test_clean_batch(flavour, k, m, B, pitch, G):
    """Every culprit -1, marks all zero, counts zero; culprit and marks handed in full of junk come
    back fully overwritten; a byte flipped only in [B, pitch) of a data and of a parity row stays
    clean (pitch 37 has no such byte)."""
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    culprit, marks, counts = locate(code, data, par, B, junk=True)
    assert culprit.shape == (G,) and (culprit == CLEAN).all()
    assert marks.shape == (G * (k + m),) and not marks.any() and not counts.any()
    if pitch > B:
        data[7, k - 1, B] ^= 0x80
        par[G - 1, 0, pitch - 1] ^= 0x01
        culprit, marks, counts = locate(code, data, par, B, junk=True)
        assert (culprit == CLEAN).all() and not marks.any() and not counts.any()


@case_params
def test_one_shard_every_id(flavour, k, m, B, pitch, G):
    """Each shard id c gets a group of its own, corrupted in that shard alone.  Across the ids the
    corrupted bytes are byte 0, byte B-1 (the masked tail), a middle byte, two bytes as far apart as
    the row allows (bytes 1 and B-2: 87 columns apart at B = 1400, different waves wherever a group
    spans more than one) and a whole row.  Exactly c, one-hot marks, counts[0] == n; a second call
    on the same counts accumulates."""
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    n = k + m
    expect = np.full(G, CLEAN, np.int32)
    for c in range(n):
        g = 2 + 13 * c  # n <= 20: below 300
        row = shard(data, par, g, c)
        kind = c % 5
        if kind == 0:
            row[0] ^= 0x01
        elif kind == 1:
            row[B - 1] ^= 0x80
        elif kind == 2:
            row[B // 2] ^= 0x3C
        elif kind == 3:
            row[1] ^= 0x55
            row[B - 2] ^= 0xA7
        else:
            row[:B] ^= to_dev(synth_bytes(900 + c, B) | 1)  # every byte changes
        expect[g] = c
    culprit, marks, counts = locate(code, data, par, B, junk=True)
    assert np.array_equal(culprit, expect)
    assert np.array_equal(marks, one_hot_marks(expect, k, n))
    assert list(counts) == [n, 0, 0]
    acc = to_dev(counts)
    culprit, marks, counts = locate(code, data, par, B, counts=acc)
    assert np.array_equal(culprit, expect) and list(counts) == [2 * n, 0, 0]


@pytest.mark.parametrize("flavour,k,m,B,pitch,G", CASES_M3)
def test_two_shards_are_multi(flavour, k, m, B, pitch, G):
    """m >= 3 only (with m = 2, distance 3, the verdict for two errors is not defined): two shards
    hit in the same byte, and two shards hit in bytes of different columns (byte 3 and byte B-2),
    both give MULTI, all-zero marks, counts[1] == 2."""
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    data[11, 1, 5] ^= 0x21
    data[11, 2, 5] ^= 0x9E
    data[G - 2, 0, 3] ^= 0x10
    par[G - 2, 1, B - 2] ^= 0x04
    expect = np.full(G, CLEAN, np.int32)
    expect[[11, G - 2]] = MULTI
    culprit, marks, counts = locate(code, data, par, B, junk=True)
    assert np.array_equal(culprit, expect)
    assert not marks.any() and list(counts) == [0, 2, 0]


def test_ambiguous_rows():
    """rows [[1,2,3],[1,2,5]]: columns 0 and 1 are proportional, so a corrupted shard 0 is also
    explained by shard 1: AMBIGUOUS, counts[2] == 1, no marks.  Shard 2 is located."""
    code = qa.Code.from_rows([[1, 2, 3], [1, 2, 5]])
    G, B = 6, 64
    data = to_dev(synth_bytes(41, G * 3 * B).reshape(G, 3, B))
    par = torch.empty((G, 2, B), dtype=torch.uint8, device=DEV)
    code.encode(data, par)
    data[1, 0, 9] ^= 0x77
    data[4, 2, 63] ^= 0x02
    culprit, marks, counts = locate(code, data, par, B, junk=True)
    assert list(culprit) == [CLEAN, AMBIGUOUS, CLEAN, CLEAN, 2, CLEAN]
    assert np.array_equal(marks, one_hot_marks(np.array([-1, -1, -1, -1, 2, -1]), 3, 5))
    assert list(counts) == [1, 0, 1]


@pytest.mark.parametrize("make,why", [(lambda: qa.Code.cauchy(4, 1), "m = 1"), (lambda: qa.Code.cauchy(33, 2), "k = 33"),
                                      (lambda: qa.Code.from_rows([[1, 2, 3], [1, 0, 5]]), "zero coefficient")])
def test_refused_codes(make, why):
    code = make()
    d = torch.zeros((2, code.k, 64), dtype=torch.uint8, device=DEV)
    p = torch.zeros((2, code.m, 64), dtype=torch.uint8, device=DEV)
    with pytest.raises(qa.QfecError, match=why):
        code.locate(d, p)
    with pytest.raises(qa.QfecError, match=why):
        code.scrub(d, p)


def random_damage(rng, data, par, B, doubles):
    """In place on host arrays: each group gets 0 or 1 corrupted shards at 1-4 random bytes; with
    `doubles` about 5 % get 2.  -> hits [G]: number of corrupted shards, expect [G]: the culprit."""
    G, k = data.shape[:2]
    n = k + par.shape[1]
    hits = np.zeros(G, np.int64)
    expect = np.full(G, CLEAN, np.int32)
    for g in range(G):
        r = rng.random()
        hits[g] = 2 if doubles and r < 0.05 else 1 if r < 0.55 else 0
        ids = rng.choice(n, size=hits[g], replace=False)
        for c in ids:
            row = data[g, c] if c < k else par[g, c - k]
            for b in rng.choice(B, size=int(rng.integers(1, 5)), replace=False):
                row[b] ^= rng.integers(1, 256)
        expect[g] = MULTI if hits[g] == 2 else int(ids[0]) if hits[g] == 1 else CLEAN
    return hits, expect


@case_params
def test_scrub(flavour, k, m, B, pitch, G):
    """Seeded random damage.  After scrub every single-damage group equals the original in [0, B)
    of data and parity, every double-damage group (m >= 3 cases) its damaged self over the whole
    pitch; culprit and counts match the construction; verify afterwards flags exactly the
    double-damage groups."""
    code, d0, p0 = encoded(flavour, k, m, B, pitch, G)
    hd, hp = d0.cpu().numpy().copy(), p0.cpu().numpy().copy()
    hits, expect = random_damage(np.random.default_rng(1000 * k + m), hd, hp, B, doubles=m >= 3)
    assert (hits == 1).sum() > 100 and (m < 3 or (hits == 2).sum() >= 5)
    dd, dp = to_dev(hd), to_dev(hp)
    counts = torch.zeros(3, dtype=torch.int32, device=DEV)
    culprit = code.scrub(dd, dp, B, counts=counts)
    torch.cuda.synchronize()
    assert np.array_equal(culprit.cpu().numpy(), expect)
    assert list(counts.cpu().numpy()) == [(hits == 1).sum(), (hits == 2).sum(), 0]
    rd, rp = dd.cpu().numpy(), dp.cpu().numpy()
    one, two, none = hits == 1, hits == 2, hits == 0
    assert np.array_equal(rd[one][..., :B], d0.cpu().numpy()[one][..., :B])
    assert np.array_equal(rp[one][..., :B], p0.cpu().numpy()[one][..., :B])
    assert np.array_equal(rd[two], hd[two]) and np.array_equal(rp[two], hp[two])
    assert np.array_equal(rd[none], hd[none]) and np.array_equal(rp[none], hp[none])
    bad = code.verify(dd, dp, B)
    torch.cuda.synchronize()
    assert np.array_equal(bad.cpu().numpy() != 0, two)
    # the verdicts are optional
    dd2, dp2 = to_dev(hd), to_dev(hp)
    assert qa.lib().qfec_scrub(code._h, dd2.data_ptr(), dp2.data_ptr(), G, B, pitch, None, None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dd2, dd) and torch.equal(dp2, dp)


def test_scrub_refuses_more_than_24_shards():
    code = qa.Code.cauchy(20, 10)
    d = torch.zeros((2, 20, 64), dtype=torch.uint8, device=DEV)
    p = torch.ones((2, 10, 64), dtype=torch.uint8, device=DEV)
    with pytest.raises(qa.QfecError, match="k \\+ m = 30"):
        code.scrub(d, p)
    torch.cuda.synchronize()
    assert not d.any() and bool((p == 1).all())  # nothing was launched
    assert list(code.locate(d, p).cpu().numpy()) == [MULTI, MULTI]  # locate itself has no such limit
