"""GPU tests of qfec_locate_erased / qfec_scrub_erased: per group the one SURVIVING shard whose
corruption explains the syndromes of the spare parity rows, in groups that also have lost (marked)
shards; CLEAN / MULTI / AMBIGUOUS / UNCHECKED / LOST otherwise; marks_out = the marks plus the
culprit, which qfec_repair takes unchanged.  Expected verdicts come from how the damage was made.
The rows of lost shards are filled with junk: they are never read.

Run on an MI355X:  python -m pytest tests/test_gpu_locate_erased.py -m gpu -q
"""
import numpy as np
import pytest

import quicknet_amd as qa
from quicknet_amd.synth import marks_to_rs_layout, synth_bytes
from repair_common import encoded, shard, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
CLEAN, MULTI, AMBIGUOUS = qa.QFEC_LOC_CLEAN, qa.QFEC_LOC_MULTI, qa.QFEC_LOC_AMBIGUOUS
UNCHECKED, LOST = qa.QFEC_LOC_UNCHECKED, qa.QFEC_LOC_LOST

# (flavour, k, m, B, pitch, G): the templated kernel at two 8-B columns per 16 (k < 14; 2 waves per
# group, one group per block); at one 8-B column per 8 bytes with a masked tail column (175 columns on
# 3 waves, G = 301 so that nothing divides evenly); the generic kernel (2 x 16-B-column passes of
# which the second is part empty); the byte kernel (pitch 37); the other matrix flavour
CASES = [("cauchy", 10, 3, 1024, 1040, 300), ("cauchy", 16, 4, 1400, 1424, 301), ("cauchy", 9, 5, 100, 128, 300),
         ("cauchy", 5, 4, 37, 37, 300), ("vandermonde", 10, 3, 1024, 1040, 300)]
# a row of more than 4 waves leaves the one-group-per-block launch: 5 waves per group, 4 per block,
# so blocks straddle groups and the last block is part empty (41 x 5 = 205 waves)
WIDE = ("cauchy", 10, 3, 2100, 2112, 41)
case_params = pytest.mark.parametrize("flavour,k,m,B,pitch,G", CASES + [WIDE])


def damage(row, kind, B, seed):
    """The five kinds of test_gpu_locate: byte 0, byte B-1 (the masked tail), a middle byte, bytes 1
    and B-2 (different waves wherever a group spans more than one), the whole row."""
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
        row[:B] ^= to_dev(synth_bytes(900 + seed, B) | 1)  # every byte changes


def junk_lost_rows(data, par, gm, seed):
    """Fill every marked row, over the whole pitch, with junk on the device."""
    k = data.shape[1]
    for buf, sel in ((data, gm[:, :k]), (par, gm[:, k:])):
        sel = sel != 0
        if sel.any():
            rows = int(sel.sum())
            buf[to_dev(sel)] = to_dev(synth_bytes(seed + rows, rows * buf.shape[2]).reshape(rows, buf.shape[2]))


def run(code, data, par, gm, B, counts=None, junk=False, alias=False):
    """qfec_locate_erased with group-order marks gm [G, n] -> (culprit [G], marks_out [G*n] in the
    rs.c layout, counts [5]) on the host."""
    G, n = gm.shape
    counts = torch.zeros(5, dtype=torch.int32, device=DEV) if counts is None else counts
    culprit = torch.full((G,), 0x5A5A5A5A, dtype=torch.int32, device=DEV) if junk else None
    marks = to_dev(marks_to_rs_layout(gm, code.k))
    out = marks if alias else torch.full((G * n,), 0xEE if junk else 0, dtype=torch.uint8, device=DEV)
    res = code.locate_erased(data, par, marks, B, culprit=culprit, marks_out=out, counts=counts)
    torch.cuda.synchronize()
    assert culprit is None or res is culprit
    return res.cpu().numpy(), out.cpu().numpy(), counts.cpu().numpy()


def expected_marks(gm, culprit, k):
    """The marks as 0 / 1 plus 1 at every located culprit, in the rs.c layout."""
    out = (gm != 0).astype(np.uint8)
    hit = culprit >= 0
    out[np.nonzero(hit)[0], culprit[hit]] = 1
    return marks_to_rs_layout(out, k)


@case_params
def test_no_marks_is_qfec_locate(flavour, k, m, B, pitch, G):
    """t = 0 everywhere: culprit, marks and the first three counts equal qfec_locate's on the same
    damaged batch -- every shard id hit once in a group of its own, clean groups, and with m >= 3 two
    two-shard groups."""
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    n = k + m
    expect = np.full(G, CLEAN, np.int32)
    for c in range(n):
        g = (2 + 13 * c) % G
        damage(shard(data, par, g, c), c % 5, B, c)
        expect[g] = c
    if m >= 3:
        data[1, 1, 5] ^= 0x21
        data[1, 2, 5] ^= 0x9E
        data[G - 1, 0, 3] ^= 0x10
        par[G - 1, 1, B - 2] ^= 0x04
        expect[[1, G - 1]] = MULTI
    ref_counts = torch.zeros(3, dtype=torch.int32, device=DEV)
    ref_marks = torch.zeros(G * n, dtype=torch.uint8, device=DEV)
    ref = code.locate(data, par, B, marks=ref_marks, counts=ref_counts)
    culprit, marks_out, counts = run(code, data, par, np.zeros((G, n), np.uint8), B, junk=True)
    assert np.array_equal(ref.cpu().numpy(), expect)  # the construction is right
    assert np.array_equal(culprit, expect)
    assert np.array_equal(marks_out, ref_marks.cpu().numpy())
    assert list(counts[:3]) == list(ref_counts.cpu().numpy()) == [n, 2 if m >= 3 else 0, 0] and not counts[3:].any()


def pair_batch(flavour, k, m, B, pitch, G):
    """For each t in 1..m-2 and every shard id c: a group of its own with t random lost shards (junk
    rows) and survivor c corrupted, the kind of damage varying over the ids."""
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    n = k + m
    rng = np.random.default_rng(31 * k + m)
    gm = np.zeros((G, n), np.uint8)
    expect = np.full(G, CLEAN, np.int32)
    idx = 0
    for t in range(1, m - 1):
        for c in range(n):
            g = (3 + 7 * idx) % G  # distinct: no wrap at G >= 300, and 7 is coprime to 41
            assert expect[g] == CLEAN and not gm[g].any()
            gm[g, rng.choice([i for i in range(n) if i != c], size=t, replace=False)] = rng.integers(1, 256, size=t)
            damage(shard(data, par, g, c), (c + t) % 5, B, idx)
            expect[g] = c
            idx += 1
    junk_lost_rows(data, par, gm, 77)
    return code, data, par, gm, expect, idx


@case_params
def test_every_lost_and_corrupted_pair(flavour, k, m, B, pitch, G):
    """culprit == c, marks_out == marks + one-hot c, counts exact; a second call on the same counts
    accumulates; marks_out aliased to marks gives the same bytes."""
    code, data, par, gm, expect, hits = pair_batch(flavour, k, m, B, pitch, G)
    assert hits == (m - 2) * (k + m)
    culprit, marks_out, counts = run(code, data, par, gm, B, junk=True)
    assert np.array_equal(culprit, expect)
    want = expected_marks(gm, expect, k)
    assert np.array_equal(marks_out, want)
    assert list(counts) == [hits, 0, 0, 0, 0]
    acc = to_dev(counts)
    culprit, marks_out, counts = run(code, data, par, gm, B, counts=acc)
    assert np.array_equal(culprit, expect) and list(counts) == [2 * hits, 0, 0, 0, 0]
    culprit, aliased, _ = run(code, data, par, gm, B, alias=True)
    assert np.array_equal(culprit, expect) and np.array_equal(aliased, want)


@case_params
def test_verdict_classes(flavour, k, m, B, pitch, G):
    """t = m: UNCHECKED (even with a corrupted survivor); t > m: LOST; t = m - 1 consistent: CLEAN;
    t = m - 1 with a shard of K or the spare corrupted: AMBIGUOUS; with 3 spares two corrupted
    survivors, in the same byte and in bytes of different columns: MULTI; a byte flipped only in
    [B, pitch) of a group with a lost shard: CLEAN.  Junk-filled culprit and marks_out come back
    fully overwritten."""
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    n = k + m
    rng = np.random.default_rng(5 * k + m)
    gm = np.zeros((G, n), np.uint8)
    expect = np.full(G, CLEAN, np.int32)

    def lose(g, t, keep=()):
        ids = rng.choice([i for i in range(n) if i not in keep], size=t, replace=False)
        gm[g, ids] = rng.integers(1, 256, size=t)
        return [i for i in range(n) if not gm[g, i]]  # the unmarked ids: K, then the spares

    left = lose(1, m)
    shard(data, par, 1, left[0])[4] ^= 0x11
    expect[1] = UNCHECKED
    lose(G - 1, m + 1)
    expect[G - 1] = LOST
    lose(3, m - 1)
    left = lose(4, m - 1)
    shard(data, par, 4, left[k // 2])[B - 1] ^= 0x40
    left = lose(5, m - 1)
    shard(data, par, 5, left[k])[0] ^= 0x02  # the one spare
    expect[[4, 5]] = AMBIGUOUS
    left = lose(6, m - 3)
    shard(data, par, 6, left[1])[5] ^= 0x21
    shard(data, par, 6, left[2])[5] ^= 0x9E
    left = lose(G - 2, m - 3)
    shard(data, par, G - 2, left[0])[3] ^= 0x10
    shard(data, par, G - 2, left[k + 1])[B - 2] ^= 0x04  # a survivor and a spare
    expect[[6, G - 2]] = MULTI
    if pitch > B:
        left = lose(8, 1)
        shard(data, par, 8, left[0])[B] ^= 0x80
        shard(data, par, 8, left[k])[pitch - 1] ^= 0x01
    junk_lost_rows(data, par, gm, 99)
    culprit, marks_out, counts = run(code, data, par, gm, B, junk=True)
    assert np.array_equal(culprit, expect)
    assert np.array_equal(marks_out, expected_marks(gm, expect, k))
    assert list(counts) == [0, 2, 2, 1, 1]


def random_loss_and_damage(rng, data, par, B):
    """In place on host arrays -> (gm [G, n], expect [G], corrupted [G]).  Per group t lost shards
    (junk rows over the whole pitch) and 0, 1 or 2 corrupted survivors at 1-4 random bytes each: 60 %
    t <= m - 2 with one corrupted survivor (the locate-and-repair path), 10 % t <= m - 2 intact, 6 %
    two corrupted survivors where 3 spares remain (MULTI), 8 % t = m - 1 (half of them with a corrupted
    survivor: AMBIGUOUS), 8 % t = m intact (UNCHECKED), 8 % t = m + 1 (LOST)."""
    G, k, pitch = data.shape
    m = par.shape[1]
    n = k + m
    gm = np.zeros((G, n), np.uint8)
    expect = np.full(G, CLEAN, np.int32)
    corrupted = np.zeros(G, np.int64)
    for g in range(G):
        r = rng.random()
        if r < 0.60:
            t, nc = int(rng.integers(0, m - 1)), 1
        elif r < 0.70:
            t, nc = int(rng.integers(0, m - 1)), 0
        elif r < 0.76:
            t, nc = (int(rng.integers(0, m - 2)), 2) if m >= 3 else (0, 0)
        elif r < 0.84:
            t, nc = m - 1, int(rng.integers(0, 2))
        elif r < 0.92:
            t, nc = m, 0
        else:
            t, nc = m + 1, 0
        lost = rng.choice(n, size=t, replace=False)
        gm[g, lost] = rng.integers(1, 256, size=t)
        for c in lost:
            (data[g, c] if c < k else par[g, c - k])[:] = rng.integers(0, 256, size=pitch, dtype=np.uint8)
        ids = rng.choice([i for i in range(n) if not gm[g, i]], size=nc, replace=False)
        for c in ids:
            row = data[g, c] if c < k else par[g, c - k]
            for b in rng.choice(B, size=int(rng.integers(1, 5)), replace=False):
                row[b] ^= rng.integers(1, 256)
        corrupted[g] = nc
        expect[g] = (LOST if t > m else UNCHECKED if t == m else CLEAN if nc == 0 else
                     AMBIGUOUS if t == m - 1 else MULTI if nc == 2 else int(ids[0]))
    return gm, expect, corrupted


@pytest.mark.parametrize("flavour,k,m,B,pitch,G", CASES)
def test_scrub_erased(flavour, k, m, B, pitch, G):
    """Seeded random loss and damage.  After the scrub every group with at most one corrupted
    survivor that is CLEAN, located or UNCHECKED equals the original in [0, B) of data and parity;
    MULTI, AMBIGUOUS and LOST groups equal their damaged selves over the whole pitch; d_failed counts
    the LOST groups; culprit and counts match the construction; verify afterwards flags exactly the
    groups left alone (their junk rows or their corruption are still there)."""
    code, d0, p0 = encoded(flavour, k, m, B, pitch, G)
    hd, hp = d0.cpu().numpy().copy(), p0.cpu().numpy().copy()
    gm, expect, corrupted = random_loss_and_damage(np.random.default_rng(1000 * k + m), hd, hp, B)
    t = (gm != 0).sum(axis=1)
    located = expect >= 0
    # the locate-and-repair path cannot pass empty, nor without lost shards beside the culprit
    assert located.sum() >= 100 and (located & (t >= 1)).sum() >= 50
    left_alone = np.isin(expect, (MULTI, AMBIGUOUS, LOST))
    assert all((expect == v).sum() >= 3 for v in (CLEAN, AMBIGUOUS, UNCHECKED, LOST)) and (m < 3 or (expect == MULTI).sum() >= 3)
    dd, dp = to_dev(hd), to_dev(hp)
    marks = to_dev(marks_to_rs_layout(gm, k))
    counts = torch.zeros(5, dtype=torch.int32, device=DEV)
    failed = torch.zeros(1, dtype=torch.int32, device=DEV)
    culprit = code.scrub_erased(dd, dp, marks, B, counts=counts, failed=failed)
    torch.cuda.synchronize()
    assert np.array_equal(culprit.cpu().numpy(), expect)
    assert list(counts.cpu().numpy()) == [located.sum()] + [(expect == v).sum() for v in (MULTI, AMBIGUOUS, UNCHECKED, LOST)]
    assert int(failed.item()) == (expect == LOST).sum()
    assert np.array_equal(marks.cpu().numpy(), marks_to_rs_layout(gm, k))  # the caller's marks are not written
    rd, rp = dd.cpu().numpy(), dp.cpu().numpy()
    healed = ~left_alone
    assert np.array_equal(rd[healed][..., :B], d0.cpu().numpy()[healed][..., :B])
    assert np.array_equal(rp[healed][..., :B], p0.cpu().numpy()[healed][..., :B])
    assert np.array_equal(rd[left_alone], hd[left_alone]) and np.array_equal(rp[left_alone], hp[left_alone])
    bad = code.verify(dd, dp, B)
    torch.cuda.synchronize()
    assert np.array_equal(bad.cpu().numpy() != 0, left_alone)
    # the verdicts and counters are optional
    dd2, dp2 = to_dev(hd), to_dev(hp)
    assert qa.lib().qfec_scrub_erased(code._h, dd2.data_ptr(), dp2.data_ptr(), marks.data_ptr(), G, B, pitch,
                                      None, None, None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dd2, dd) and torch.equal(dp2, dp)


NOT_MDS = [[1, 1, 1], [1, 2, 3], [2, 2, 7]]  # tests/test_locate_erased_host.py says why


@pytest.mark.parametrize("make,why", [(lambda: qa.Code.cauchy(4, 1), "m = 1"), (lambda: qa.Code.cauchy(20, 10), "k \\+ m = 30"),
                                      (lambda: qa.Code.from_rows([[1, 2, 3], [1, 0, 5], [1, 4, 6]]), "zero coefficient"),
                                      (lambda: qa.Code.from_rows(NOT_MDS), "not MDS")])
def test_refused_codes(make, why):
    """QFEC_EUNSUP from both calls; nothing is launched: data, parity, marks, culprit and counts are
    as they were."""
    code = make()
    n = code.k + code.m
    d = torch.full((2, code.k, 64), 3, dtype=torch.uint8, device=DEV)
    p = torch.full((2, code.m, 64), 5, dtype=torch.uint8, device=DEV)
    marks = torch.zeros(2 * n, dtype=torch.uint8, device=DEV)
    marks[0] = 1
    culprit = torch.full((2,), 1234, dtype=torch.int32, device=DEV)
    counts = torch.full((5,), 7, dtype=torch.int32, device=DEV)
    out = torch.full((2 * n,), 0xEE, dtype=torch.uint8, device=DEV)
    with pytest.raises(qa.QfecError, match=why):
        code.locate_erased(d, p, marks, culprit=culprit, marks_out=out, counts=counts)
    with pytest.raises(qa.QfecError, match=why):
        code.scrub_erased(d, p, marks, culprit=culprit, counts=counts)
    torch.cuda.synchronize()
    assert bool((d == 3).all()) and bool((p == 5).all()) and bool((out == 0xEE).all())
    assert bool((culprit == 1234).all()) and bool((counts == 7).all())
    assert int(marks.sum()) == 1
