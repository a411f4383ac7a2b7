"""GPU tests of the integrity family on pointer tables: qfec_verify_ptrs, qfec_locate_ptrs and
qfec_scrub_ptrs (include/qfec.h; kernels in qfec_integrity_ptrs.hip).  Batches live in a guard-filled
ptrs_common.Pool in permuted slots, encoded by the oracle on the CPU; expected culprits come from how
the damage was made, expected verify bits from the oracle's parity compared row by row on the CPU.
After every verify and locate call the whole pool is compared with its image before the call: nothing
is written.  Shapes and their coverage: integrity_ptrs_common.cells().  The launches of a batch beyond
one launch's index space are not reached here (no cheap way to force them)."""
import ctypes as C

import numpy as np
import pytest

import integrity_ptrs_common as ic
import ptrs_common as pc
import quicknet_amd as qa
from integrity_ptrs_common import AMBIGUOUS, CLEAN, MULTI

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
CELLS = ic.cells()
ic.assert_coverage(CELLS)
VERIFY_CELLS = [c for c in CELLS if (c[0], c[1]) not in ic.LOCATE_ONLY]
LOCATE_CELLS = [c for c in CELLS if (c[0], c[1]) not in ic.VERIFY_ONLY]
JUNK = 0x5A5A5A5A


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def counter(n=1, start=0):
    return torch.full((n,), start, dtype=torch.int32, device=DEV)


def upload(pool, img, alias=None):
    """(pool tensor, table) of an image; the pool object only lends its layout."""
    t = dev(img)
    assert t.data_ptr() % 16 == 0
    start = pool.start.copy()
    for i, j in (alias or {}).items():
        start[i] = start[j]
    return t, dev(t.data_ptr() + start)


def unchanged(t, img):
    torch.cuda.synchronize()
    return np.array_equal(t.cpu().numpy(), img)


def verify(code, pool, img, G, bad_groups=None, alias=None):
    """-> (bad_rows, counter value): the output starts full of junk; the pool must come back as it was."""
    t, table = upload(pool, img, alias)
    rows = torch.full((G,), JUNK, dtype=torch.int32, device=DEV)
    cnt = counter() if bad_groups is None else bad_groups
    code.verify_ptrs(table, pool.B, bad_rows=rows, bad_groups=cnt)
    assert unchanged(t, img), "verify_ptrs wrote into the pool"
    return rows.cpu().numpy(), int(cnt.cpu()[0])


def locate(code, pool, img, G, counts=None, alias=None):
    """-> (culprit, marks, counts): the outputs start full of junk; the pool must come back as it was."""
    t, table = upload(pool, img, alias)
    culprit = torch.full((G,), JUNK, dtype=torch.int32, device=DEV)
    marks = torch.full((G * (code.k + code.m),), 0xEE, dtype=torch.uint8, device=DEV)
    cnt = counter(3) if counts is None else counts
    code.locate_ptrs(table, pool.B, culprit=culprit, marks=marks, counts=cnt)
    assert unchanged(t, img), "locate_ptrs wrote into the pool"
    return culprit.cpu().numpy(), marks.cpu().numpy(), cnt.cpu().numpy().tolist()


def case(c):
    k, m, B, mode, G = c
    code = qa.Code.cauchy(k, m)
    pool, img = ic.batch(code, B, mode, G)
    return code, pool, img


# ---------------------------------------------------------------- 1. clean batch

@pytest.mark.parametrize("c", CELLS, ids=ic.cell_id)
def test_clean_batch(c):
    """Every word 0 / CLEAN, zero marks, counters untouched, junk outputs fully overwritten; the same
    with every guard byte of the pool random (bytes -1 and block_size of every row included)."""
    k, m, B, mode, G = c
    code, pool, img = case(c)
    for image in (img, ic.random_guards(pool, img, seed=B + k)):
        if c in VERIFY_CELLS:
            rows, cnt = verify(code, pool, image, G, bad_groups=counter(start=7))
            assert not rows.any() and cnt == 7
        if c in LOCATE_CELLS:
            culprit, marks, counts = locate(code, pool, image, G, counts=counter(3, start=3))
            assert (culprit == CLEAN).all() and not marks.any() and counts == [3, 3, 3]


# ---------------------------------------------------------------- 2. verify bits

@pytest.mark.parametrize("c", VERIFY_CELLS, ids=ic.cell_id)
def test_verify_bits(c):
    """Parity row j damaged alone, for every j; a data shard damaged (every row's bit); each damage
    kind the block size has room for, the one in two slabs of one row included: the group is counted
    once although two waves report it.  Two calls on one counter accumulate; a counter-only call."""
    k, m, B, mode, G = c
    code, pool, img = case(c)
    kinds = sorted(ic.spots(B).items())
    plan = [(k + j, kinds[j % len(kinds)]) for j in range(m)] + [((3 * i) % k, kd) for i, kd in enumerate(kinds)]
    assert 2 * len(plan) < G
    expect = np.zeros(G, np.int32)
    for i, (shard, (_, where)) in enumerate(plan):
        g = 1 + 2 * i
        ic.hit(pool, img, ic.row_id(G, k, m, g, shard), where, salt=shard * 131 + i)
        expect[g] = 1 << (shard - k) if shard >= k else (1 << m) - 1
    assert np.array_equal(ic.expected_bits(code, pool, img, G), expect)  # the oracle agrees with the construction
    cnt = counter(start=5)
    rows, total = verify(code, pool, img, G, bad_groups=cnt)
    assert np.array_equal(rows, expect) and total == 5 + len(plan)
    rows, total = verify(code, pool, img, G, bad_groups=cnt)
    assert np.array_equal(rows, expect) and total == 5 + 2 * len(plan)
    t, table = upload(pool, img)
    only = counter()
    assert qa.lib().qfec_verify_ptrs(code._h, C.c_void_p(table.data_ptr()), G, B, None, C.c_void_p(only.data_ptr()),
                                     None) == 0
    assert unchanged(t, img) and int(only.cpu()[0]) == len(plan)


# ---------------------------------------------------------------- 3. one shard, every id

@pytest.mark.parametrize("c", LOCATE_CELLS, ids=ic.cell_id)
def test_one_shard_every_id(c):
    """Each shard id gets a group of its own, damaged in that shard alone by the kinds above and a
    whole row: exactly that id, one-hot marks, counts == [ids, 0, 0]; a second call accumulates."""
    k, m, B, mode, G = c
    code, pool, clean = case(c)
    n = k + m
    kinds = sorted(ic.spots(B).items())
    for base in range(0, n, G):  # n > G: more than one round
        img = clean.copy()
        ids = list(range(base, min(n, base + G)))
        expect = np.full(G, CLEAN, np.int32)
        for s in ids:
            g = (s - base) * (G // len(ids))
            ic.hit(pool, img, ic.row_id(G, k, m, g, s), kinds[s % len(kinds)][1], salt=900 + s)
            expect[g] = s
        acc = counter(3)
        culprit, marks, counts = locate(code, pool, img, G, counts=acc)
        assert np.array_equal(culprit, expect)
        assert np.array_equal(marks, ic.one_hot(expect, G, k, m))
        assert counts == [len(ids), 0, 0]
        culprit, marks, counts = locate(code, pool, img, G, counts=acc)
        assert np.array_equal(culprit, expect) and counts == [2 * len(ids), 0, 0]


# ---------------------------------------------------------------- 4. MULTI across waves

@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m", [(10, 3), (16, 4), (8, 4), (9, 5), (5, 3)])
def test_multi_across_waves(k, m, mode):
    """B = 1400, two slabs and a tail: shard a hit only in slab 0 and shard b only in slab 1 (each wave alone
    sees a single-shard pattern); a parity row in slab 0 and a data shard in slab 1; two shards in the
    same byte.  All MULTI, zero marks, counts[1]."""
    B, G = 1400, ic.G_SMALL
    code = qa.Code.cauchy(k, m)
    pool, img = ic.batch(code, B, mode, G)
    row = lambda g, s: ic.row_id(G, k, m, g, s)
    ic.hit(pool, img, row(2, 1), [7], 1)
    ic.hit(pool, img, row(2, 3), [1024 + 9], 2)
    ic.hit(pool, img, row(5, k + 1), [100], 3)
    ic.hit(pool, img, row(5, 0), [1024 + 300], 4)
    ic.hit(pool, img, row(9, 2), [555], 5)
    ic.hit(pool, img, row(9, 4), [555], 6)
    ic.hit(pool, img, row(20, k - 1), [3, B - 1], 7)  # and one single shard, in both slabs
    expect = np.full(G, CLEAN, np.int32)
    expect[[2, 5, 9]] = MULTI
    expect[20] = k - 1
    culprit, marks, counts = locate(code, pool, img, G)
    assert np.array_equal(culprit, expect)
    assert np.array_equal(marks, ic.one_hot(expect, G, k, m))
    assert counts == [1, 3, 0]


# ---------------------------------------------------------------- 5. AMBIGUOUS

@pytest.mark.parametrize("B,mode", [(64, "aligned"), (17, "residues"), (1025, "one-data")])
def test_ambiguous_rows(B, mode):
    """rows [[1,2,3],[1,2,5]]: columns 0 and 1 are proportional, so a corrupted shard 0 is also
    explained by shard 1: AMBIGUOUS, counts[2], no marks.  Shard 2 is located."""
    code = qa.Code.from_rows([[1, 2, 3], [1, 2, 5]])
    G = 6
    pool, img = ic.batch(code, B, mode, G)
    ic.hit(pool, img, ic.row_id(G, 3, 2, 1, 0), [B // 2], 1)
    ic.hit(pool, img, ic.row_id(G, 3, 2, 4, 2), [B - 1], 2)
    culprit, marks, counts = locate(code, pool, img, G)
    assert list(culprit) == [CLEAN, AMBIGUOUS, CLEAN, CLEAN, 2, CLEAN]
    assert np.array_equal(marks, ic.one_hot(np.array([-1, -1, -1, -1, 2, -1]), G, 3, 2))
    assert counts == [1, 0, 1]
    rows, cnt = verify(code, pool, img, G)
    assert list(rows) == [0, 3, 0, 0, 3, 0] and cnt == 2


# ---------------------------------------------------------------- 6. aliased reads

@pytest.mark.parametrize("k,m,B,mode", [(10, 3, 1025, "aligned"), (9, 5, 17, "residues"), (16, 4, 1400, "one-parity")])
def test_aliased_reads(k, m, B, mode):
    """Data shard 1 of every group repeats data shard 0's address; the parity comes from
    qfec_encode_ptrs on that table.  Clean; after a parity byte is damaged, that row is named."""
    G = ic.G_SMALL
    code = qa.Code.cauchy(k, m)
    pool, img = ic.batch(code, B, mode, G)
    alias = {g * k + 1: g * k for g in range(G)}
    t, table = upload(pool, img, alias)
    code.encode_ptrs(table, B)
    torch.cuda.synchronize()
    img = t.cpu().numpy().copy()
    rows, cnt = verify(code, pool, img, G, alias=alias)
    assert not rows.any() and cnt == 0
    culprit, marks, counts = locate(code, pool, img, G, alias=alias)
    assert (culprit == CLEAN).all() and not marks.any() and counts == [0, 0, 0]
    ic.hit(pool, img, ic.row_id(G, k, m, 6, k + m - 1), [B - 1], 1)
    rows, cnt = verify(code, pool, img, G, alias=alias)
    expect = np.zeros(G, np.int32)
    expect[6] = 1 << (m - 1)
    assert np.array_equal(rows, expect) and cnt == 1
    culprit, marks, counts = locate(code, pool, img, G, alias=alias)
    assert culprit[6] == k + m - 1 and (np.delete(culprit, 6) == CLEAN).all() and counts == [1, 0, 0]
    assert marks.sum() == 1 and marks[ic.row_id(G, k, m, 6, k + m - 1)] == 1


# ---------------------------------------------------------------- 7. against the contiguous calls

@pytest.mark.parametrize("k,m,B,mode", [(10, 3, 1000, "aligned"), (16, 4, 1400, "residues"), (4, 2, 17, "one-data"),
                                        (8, 4, 1025, "aligned"), (9, 5, 1040, "one-parity"), (5, 3, 1, "aligned")])
def test_against_the_contiguous_calls(k, m, B, mode):
    """The same rows in padded contiguous buffers: qfec_verify / qfec_locate give the table calls'
    outputs word for word, on a batch of clean, single and (m >= 3) double damage."""
    G = ic.G_SMALL
    code = qa.Code.cauchy(k, m)
    pool, img = ic.batch(code, B, mode, G)
    expect, double = ic.random_damage(np.random.default_rng(k * B + m), pool, img, G, k, m, doubles=m >= 3)
    assert (expect == CLEAN).any() and (expect >= 0).any() and (m < 3 or double.any())
    data, par = ic.split(pool, img, G, k, m)
    d, p = pc.padded(torch, DEV, data, B), pc.padded(torch, DEV, par, B)
    ref_cnt, ref_counts = counter(), counter(3)
    ref_rows = code.verify(d, p, B, bad_groups=ref_cnt).cpu().numpy()
    ref_marks = torch.empty(G * (k + m), dtype=torch.uint8, device=DEV)
    ref_culprit = code.locate(d, p, B, marks=ref_marks, counts=ref_counts).cpu().numpy()
    rows, cnt = verify(code, pool, img, G)
    culprit, marks, counts = locate(code, pool, img, G)
    assert np.array_equal(rows, ref_rows) and cnt == int(ref_cnt.cpu()[0])
    assert np.array_equal(culprit, ref_culprit) and np.array_equal(culprit, expect)
    assert np.array_equal(marks, ref_marks.cpu().numpy()) and counts == ref_counts.cpu().numpy().tolist()
    assert np.array_equal(rows, ic.expected_bits(code, pool, img, G))


# ---------------------------------------------------------------- 8. scrub

@pytest.mark.parametrize("k,m,B,mode", [(10, 3, 1400, "aligned"), (16, 4, 1025, "one-data"), (9, 5, 1025, "residues"),
                                        (4, 2, 1000, "one-parity"), (20, 8, 17, "one-data"), (20, 8, 1400, "aligned")])
def test_scrub(k, m, B, mode):
    """Single damage in about a third of the groups, double damage (m >= 3) in a few: after the scrub
    the whole pool is the pre-damage pool except the double-damaged groups, which keep their damaged
    image; culprits and counts as for locate, *d_failed unchanged.  d_culprit = NULL; a side stream;
    the same pool as locate_ptrs followed by repair_ptrs_wide with the returned marks.  (20,8) is
    beyond qfec_scrub's k + m <= 24."""
    G = ic.G_SMALL
    code = qa.Code.cauchy(k, m)
    pool, clean = ic.batch(code, B, mode, G)
    img = clean.copy()
    expect, double = ic.random_damage(np.random.default_rng(k + B * m), pool, img, G, k, m, doubles=m >= 3)
    assert (expect >= 0).any() and (m < 3 or double.any())
    want = clean.copy()
    for g in np.nonzero(double)[0]:
        for s in range(k + m):
            a = pool.start[ic.row_id(G, k, m, g, s)]
            want[a:a + B] = img[a:a + B]
    located, multi = int((expect >= 0).sum()), int(double.sum())

    t, table = upload(pool, img)
    counts, failed = counter(3), counter(start=4)
    culprit = code.scrub_ptrs(table, B, counts=counts, failed=failed)
    torch.cuda.synchronize()
    assert np.array_equal(culprit.cpu().numpy(), expect)
    assert counts.cpu().numpy().tolist() == [located, multi, 0] and int(failed.cpu()[0]) == 4
    assert np.array_equal(t.cpu().numpy(), want)

    # no culprits wanted, on a side stream
    t2, table2 = upload(pool, img)
    counts2 = counter(3)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert qa.lib().qfec_scrub_ptrs(code._h, C.c_void_p(table2.data_ptr()), G, B, None,
                                        C.c_void_p(counts2.data_ptr()), None, C.c_void_p(side.cuda_stream)) == 0
    side.synchronize()
    assert np.array_equal(t2.cpu().numpy(), want) and counts2.cpu().numpy().tolist() == [located, multi, 0]

    # locate_ptrs, then repair_ptrs_wide with the marks it returned
    t3, table3 = upload(pool, img)
    marks = torch.empty(G * (k + m), dtype=torch.uint8, device=DEV)
    code.locate_ptrs(table3, B, marks=marks)
    code.repair_ptrs_wide(table3, marks, B)
    torch.cuda.synchronize()
    assert np.array_equal(t3.cpu().numpy(), t.cpu().numpy())
