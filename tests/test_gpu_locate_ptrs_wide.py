"""GPU tests of qfec_check_apply_ptrs / qfec_locate_ptrs_wide / qfec_scrub_ptrs_wide: single-shard error
location at any k + m on shards scattered in device memory.  Two references, never the code under
test: the numpy model of the definition (locate_wide_common.model) and the contiguous calls
qfec_locate_wide / qfec_scrub_wide on the same rows, zero-padded to a pitch of round16(B); on narrow codes
qfec_locate_erased / qfec_scrub_erased as well.  All comparisons are exact integers and bytes.

The rows lie in a guard-filled pool (ptrs_common.Pool), in a random permutation of slots, and the
WHOLE pool is compared after every call: a byte written anywhere by a locate fails, and so does a byte
written outside a rewritten shard by the scrub.  The rows of lost shards hold junk; they are never read.

Run on an MI355X:  python -m pytest tests/test_gpu_locate_ptrs_wide.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import ptrs_common as pc
import quicknet_amd as qa
from locate_wide_common import AMBIGUOUS, CLEAN, LOST, MULTI, UNCHECKED, model
from ptrs_wide_common import put_rows
from quicknet_amd.synth import marks_to_rs_layout
from repair_common import encoded, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
MODES = ["aligned", "residues", "one-data", "one-parity"]


# ---------------------------------------------------------------- batches, pools, calls
def host_batch(flavour, k, m, B, G):
    """A consistent batch on the host: (code, data [G, k, B], parity [G, m, B])."""
    code, data, par = encoded(flavour, k, m, B, B, G)
    return code, data.cpu().numpy(), par.cpu().numpy()


def row_of(hd, hp, g, c):
    k = hd.shape[1]
    return hd[g, c] if c < k else hp[g, c - k]


def lose(rng, hd, hp, gm, g, t, keep=(), first=()):
    """t lost shards outside `keep`, those of `first` among them (non-zero marks, junk rows); returns
    the unmarked ids: K, then the spares."""
    n = gm.shape[1]
    ids = list(first)[:t]
    rest = [i for i in range(n) if i not in keep and i not in ids]
    ids += list(rng.choice(rest, size=t - len(ids), replace=False))
    for c in ids:
        gm[g, c] = rng.integers(1, 256)
        row_of(hd, hp, g, c)[:] = rng.integers(0, 256, size=hd.shape[2], dtype=np.uint8)
    return [i for i in range(n) if not gm[g, i]]


def hurt(rng, row, kind):
    """0: one byte somewhere, 1: the last byte only, 2: several bytes."""
    B = len(row)
    if kind == 1:
        row[B - 1] ^= rng.integers(1, 256)
    elif kind == 2:
        for b in rng.choice(B, size=min(B, 5), replace=False):
            row[b] ^= rng.integers(1, 256)
    else:
        row[rng.integers(0, B)] ^= rng.integers(1, 256)


def row_id(G, k, m, g, c):
    """Pool row (= table entry) of shard c of group g."""
    return g * k + c if c < k else G * k + g * m + (c - k)


def pool_of(hd, hp, mode, seed, extra=(), hostile=False):
    """The batch's rows in a pool, table order; extra: offsets of further rows after them.  hostile:
    every byte that is not a row's is random instead of the guard byte."""
    G, k, B = hd.shape
    m = hp.shape[1]
    offs = np.concatenate([pc.offsets_for(mode, G, k, m), np.asarray(extra, np.int64)])
    pool = pc.Pool(G * (k + m) + len(extra), B, offs, seed)
    if hostile:
        pool.host[:] = np.random.default_rng(seed + 7).integers(0, 256, size=len(pool.host), dtype=np.uint8)
    put_rows(pool, pool.host, 0, hd.reshape(G * k, B))
    put_rows(pool, pool.host, G * k, hp.reshape(G * m, B))
    return pool


def run(code, pool, gm, B, call="locate", use_marks=True, alias_out=False, counts=None, alias=None, plans=None):
    """qfec_locate_ptrs_wide (or qfec_check_build + qfec_check_apply_ptrs) on the pool's table ->
    (culprit, marks_out, counts) on the host.  Also: the whole pool and the marks are as they were."""
    G, n = gm.shape
    t, ptrs = pc.to_device(torch, DEV, pool, alias)
    ptrs = ptrs[:G * n].contiguous()
    before = t.clone()
    marks_h = marks_to_rs_layout(gm, code.k)
    marks = to_dev(marks_h)
    out = marks if alias_out else torch.full((G * n,), 0xEE, dtype=torch.uint8, device=DEV)
    culprit = torch.full((G,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(5, dtype=torch.int32, device=DEV)
    if counts is not None:
        cnt.copy_(torch.from_numpy(np.asarray(counts, np.int32)))
    if call == "locate":
        res = code.locate_ptrs_wide(ptrs, B, marks if use_marks else None, culprit=culprit, marks_out=out, counts=cnt)
    else:
        if plans is None:
            plans = code.check_build(marks if use_marks else None, groups=G)
        res = code.check_apply_ptrs(ptrs, plans, B, culprit=culprit, marks_out=out, counts=cnt)
    torch.cuda.synchronize()
    assert res is culprit
    assert torch.equal(t, before), "a locate wrote into the pool"
    if not alias_out:
        assert np.array_equal(marks.cpu().numpy(), marks_h)
    return culprit.cpu().numpy(), out.cpu().numpy(), cnt.cpu().numpy()


def contiguous(code, hd, hp, gm, B, use_marks=True, erased=False):
    """qfec_locate_wide (erased: qfec_locate_erased) on the rows zero-padded to round16(B)."""
    G, n = gm.shape
    d, p = pc.padded(torch, DEV, hd, B), pc.padded(torch, DEV, hp, B)
    marks = to_dev(marks_to_rs_layout(gm, code.k))
    out = torch.full((G * n,), 0xEE, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(5, dtype=torch.int32, device=DEV)
    fn = code.locate_erased if erased else code.locate_wide
    culprit = fn(d, p, marks if use_marks or erased else None, B, marks_out=out, counts=cnt)
    torch.cuda.synchronize()
    return culprit.cpu().numpy(), out.cpu().numpy(), cnt.cpu().numpy()


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, np.nonzero(got[0] != want[0])[0][:8])
    assert np.array_equal(got[1], want[1]), what
    assert list(got[2]) == list(want[2]), what


def six_ts(m):
    return sorted({0, 1, m - 2, m - 1, m, m + 1})


# ---------------------------------------------------------------- 1. the contiguous call and the model
# (10,3): NP 1, narrow; (32,8): one syndrome pass; (70,10): NP 2, two syndrome passes with t <= 1, a
# candidate at position 69 of K; (200,55): NP 4
FAMILY = [(10, 3, 40), (32, 8, 33), (70, 10, 17), (200, 55, 18)]


@functools.lru_cache(maxsize=None)
def family(k, m, B):
    """For every t of six_ts(m): beside t lost shards, every shard id corrupted in turn (k + m <= 40), or
    a data id, a parity id inside K (position k - 1, which a lost data shard 0 makes one) and the last
    spare; then two corrupted survivors with three spares or more (never with two), and a corrupted
    first spare.  Groups are ordered by t, so the first ones are complete.  Returns the batch and the
    references, each computed once and shared by every alignment mode."""
    n = k + m
    ts = six_ts(m)
    per = n if n <= 40 else 3
    G = len(ts) * per + 3
    code, hd, hp = host_batch("cauchy", k, m, B, G)
    rng = np.random.default_rng(1000 * k + 10 * m + B)
    gm = np.zeros((G, n), np.uint8)
    g = 0
    for t in ts:
        for i in range(per):
            if n <= 40:
                lose(rng, hd, hp, gm, g, t, keep=(i,))
                hurt(rng, row_of(hd, hp, g, i), (i + t) % 3)
            else:
                left = lose(rng, hd, hp, gm, g, t, keep=(1, k, n - 1), first=(0,))
                if len(left) >= k:
                    c = left[1] if i == 0 else left[k - 1] if i == 1 or len(left) == k else left[-1]
                    assert i or c < k
                    assert i != 1 or not t or c >= k
                    hurt(rng, row_of(hd, hp, g, c), (i + t) % 3)
            g += 1
    left = lose(rng, hd, hp, gm, g, m - 3)  # two of K, the same byte: S = 3
    row_of(hd, hp, g, left[0])[B // 2] ^= 0x21
    row_of(hd, hp, g, left[k - 1])[B // 2] ^= 0x9E
    left = lose(rng, hd, hp, gm, g + 1, 0)  # one of K and the last spare, any bytes
    hurt(rng, row_of(hd, hp, g + 1, left[k // 2]), 0)
    hurt(rng, row_of(hd, hp, g + 1, left[-1]), 1)
    left = lose(rng, hd, hp, gm, g + 2, 1)  # the first spare alone
    hurt(rng, row_of(hd, hp, g + 2, left[k]), 0)
    want = model(code, hd, hp, gm, B)
    c = want[0]
    assert (c >= 0).sum() >= per and (c == MULTI).sum() >= 2
    assert all((c == v).any() for v in (AMBIGUOUS, UNCHECKED, LOST))
    refs = {"model": want, "locate_wide": contiguous(code, hd, hp, gm, B)}
    if k + m <= 24:
        refs["locate_erased"] = contiguous(code, hd, hp, gm, B, erased=True)
    whole = per  # the groups of t = 0
    refs["no marks"] = contiguous(code, hd[:whole], hp[:whole], gm[:whole], B, use_marks=False)
    assert not gm[:whole].any()
    return code, hd, hp, gm, refs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,m,B", FAMILY)
def test_answers_as_the_contiguous_call_and_the_model(k, m, B, mode):
    code, hd, hp, gm, refs = family(k, m, B)
    pool = pool_of(hd, hp, mode, k + m)
    got = run(code, pool, gm, B)
    for name in ("model", "locate_wide", "locate_erased"):
        if name in refs:
            same(got, refs[name], name)
    same(run(code, pool, gm, B, call="apply"), refs["model"], "check_apply_ptrs")
    # t = 0 with d_marks NULL: the complete groups as a batch of their own
    whole = len(refs["no marks"][0])
    sub = pool_of(hd[:whole], hp[:whole], mode, k + m + 1)
    same(run(code, sub, gm[:whole], B, use_marks=False), refs["no marks"], "no marks")
    same(run(code, sub, gm[:whole], B, call="apply", use_marks=False), refs["no marks"], "no marks, apply")


# ---------------------------------------------------------------- 2. block sizes at the seams
def seam_spots(B, mode):
    vcols = B // 16
    spots = {0, B - 1}
    if vcols:
        spots.add(vcols * 16 - 1)  # the last byte of the last whole column
    if B % 16:
        spots.add(vcols * 16)  # the first tail byte
    if mode == "residues" and B >= 1029:
        spots |= {1023, 1024}  # the byte body's slab seam
    return sorted(spots)


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33, 1024, 1040, 1029])
def test_block_sizes_at_the_seams(B, mode):
    """B = 1: tail only; 15, 16: one column or one tail; 1024: exactly one slab; 1040: two slabs; 1029: a
    tail on a last wave that holds one column.  One damaged byte per group at every seam; then a
    consistent batch: CLEAN, nothing flagged by lanes that have no column."""
    k, m = 32, 8
    n = k + m
    spots = seam_spots(B, mode)
    G = len(spots)
    code, hd, hp = host_batch("cauchy", k, m, B, G)
    clean = pool_of(hd, hp, mode, B)
    none = np.zeros((G, n), np.uint8)
    got = run(code, clean, none, B, use_marks=False)
    assert (got[0] == CLEAN).all() and not got[2].any() and not got[1].any()
    rng = np.random.default_rng(B)
    gm = np.zeros((G, n), np.uint8)
    expect = np.zeros(G, np.int32)
    for g, b in enumerate(spots):
        left = lose(rng, hd, hp, gm, g, g % 3)
        expect[g] = left[(7 * g + b) % len(left)]
        row_of(hd, hp, g, expect[g])[b] ^= rng.integers(1, 256)
    want = model(code, hd, hp, gm, B)
    assert np.array_equal(want[0], expect)
    got = run(code, pool_of(hd, hp, mode, B + 1), gm, B)
    same(got, want, "model")
    same(got, contiguous(code, hd, hp, gm, B), "locate_wide")


# ---------------------------------------------------------------- 3. guards
@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m,B", [(32, 8, 33), (70, 10, 17)])
def test_hostile_guards_change_nothing(k, m, B, mode):
    """Every byte of the pool that is not a row's is random: one of them read as a shard's byte makes
    a syndrome non-zero and turns a verdict.  The verdicts are those with constant guards."""
    code, hd, hp, gm, refs = family(k, m, B)
    same(run(code, pool_of(hd, hp, mode, 3 * k, hostile=True), gm, B), refs["model"], "model")


# ---------------------------------------------------------------- 4. marked entries
@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m,B", [(32, 8, 33), (70, 10, 17), (200, 55, 18)])
def test_marked_entries_are_never_dereferenced(k, m, B, mode):
    """Every marked shard's entry names one extra row of the pool, at an odd offset and full of random
    bytes; the results are those of the true table and the pool is unchanged."""
    code, hd, hp, gm, refs = family(k, m, B)
    G, n = gm.shape
    pool = pool_of(hd, hp, mode, 5 * k, extra=(7,))
    pool.put(G * n, np.random.default_rng(k).integers(0, 256, size=B, dtype=np.uint8))
    alias = {row_id(G, k, m, g, c): G * n for g, c in zip(*np.nonzero(gm))}
    assert len(alias) > G and pool.start[G * n] % 2 == 1
    same(run(code, pool, gm, B, alias=alias), refs["model"], "locate_ptrs_wide")
    same(run(code, pool, gm, B, call="apply", alias=alias), refs["model"], "check_apply_ptrs")


# ---------------------------------------------------------------- 5. plan reuse and aliasing
def test_one_check_plan_serves_two_tables():
    k, m, B = 70, 10, 17
    code, hd, hp, gm, refs = family(k, m, B)
    G, n = gm.shape
    plans = code.check_build(to_dev(marks_to_rs_layout(gm, k)))
    torch.cuda.synchronize()
    # a second batch with the same losses and other damage
    rng = np.random.default_rng(11)
    _, hd2, hp2 = host_batch("cauchy", k, m, B, G)
    for g in range(G):
        left = [i for i in range(n) if not gm[g, i]]
        for c in np.nonzero(gm[g])[0]:
            row_of(hd2, hp2, g, c)[:] = 0x77
        if g % 3 and len(left) >= k:
            hurt(rng, row_of(hd2, hp2, g, left[(5 * g) % len(left)]), g % 3)
    same(run(code, pool_of(hd, hp, "aligned", 21), gm, B, call="apply", plans=plans), refs["model"], "first table")
    same(run(code, pool_of(hd2, hp2, "residues", 22), gm, B, call="apply", plans=plans), model(code, hd2, hp2, gm, B),
         "second table")


@pytest.mark.parametrize("mode", ["aligned", "residues"])
def test_marks_out_may_be_marks_and_counts_accumulate(mode):
    code, hd, hp, gm, refs = family(32, 8, 33)
    pool = pool_of(hd, hp, mode, 9)
    first = run(code, pool, gm, 33)
    culprit, aliased, counts = run(code, pool, gm, 33, alias_out=True, counts=first[2])
    assert np.array_equal(culprit, refs["model"][0]) and np.array_equal(aliased, first[1])
    assert list(counts) == list(2 * refs["model"][2])


def test_a_survivor_row_may_repeat_in_two_groups():
    """Groups 1 and 2 hold the bytes of group 0, and group 1's entries of two survivors are the
    addresses of group 0's rows; group 2, damaged, reads group 0's row as a survivor as well."""
    k, m, B = 32, 8, 33
    n = k + m
    code, hd, hp = host_batch("cauchy", k, m, B, 4)
    hd[1], hp[1], hd[2], hp[2] = hd[0], hp[0], hd[0], hp[0]
    gm = np.zeros((4, n), np.uint8)
    rng = np.random.default_rng(5)
    left = lose(rng, hd, hp, gm, 2, 2, keep=(3, 4))
    hd[2, 4, B - 1] ^= 0x40
    want = model(code, hd, hp, gm, B)
    assert list(want[0]) == [CLEAN, CLEAN, 4, CLEAN] and 3 in left
    alias = {row_id(4, k, m, 1, 5): row_id(4, k, m, 0, 5), row_id(4, k, m, 1, k + 2): row_id(4, k, m, 0, k + 2),
             row_id(4, k, m, 2, 3): row_id(4, k, m, 0, 3)}
    for mode in ("aligned", "residues"):
        same(run(code, pool_of(hd, hp, mode, 13), gm, B, alias=alias), want, mode)


# ---------------------------------------------------------------- 6. chunking
def test_more_than_one_chunk_of_plans():
    """The one-shot keeps one chunk's plans under 64 MiB: (200,55) goes in chunks of 3 034 groups.  Damage
    on both sides of the cut and in the last group, beside lost shards; the model judges those groups,
    every other group is complete and consistent."""
    k, m, B = 200, 55, 16
    n = k + m
    per = (64 << 20) // qa.Code.cauchy(k, m).check_stride()
    G = per + 40
    assert (per, G) == (3034, 3074)
    code, hd, hp = host_batch("cauchy", k, m, B, G)
    rng = np.random.default_rng(3)
    gm = np.zeros((G, n), np.uint8)
    expect = np.full(G, CLEAN, np.int32)
    hit = [0, per - 1, per, per + 1, G - 1]
    for i, g in enumerate(hit):
        left = lose(rng, hd, hp, gm, g, 1 + i)
        c = left[(37 * i) % len(left)]
        hurt(rng, row_of(hd, hp, g, c), i % 3)
        expect[g] = c
    lose(rng, hd, hp, gm, per + 2, m)
    expect[per + 2] = UNCHECKED
    sub = hit + [per + 2]
    want = model(code, hd[sub], hp[sub], gm[sub], B)
    assert np.array_equal(want[0], expect[sub])
    culprit, marks_out, counts = run(code, pool_of(hd, hp, "aligned", 17), gm, B)
    assert np.array_equal(culprit, expect)
    marked = (gm != 0).astype(np.uint8)
    marked[hit, expect[hit]] = 1
    assert np.array_equal(marks_out, marks_to_rs_layout(marked, k))
    assert list(counts) == [len(hit), 0, 0, 1, 0]


# ---------------------------------------------------------------- 7. scrub
def random_loss_and_damage(rng, hd, hp):
    """In place -> gm [G, n].  Per group t lost shards (junk rows) and 0, 1 or 2 corrupted survivors, in
    a cycle of 20 groups: eleven with t <= m - 2 and one corrupted survivor; two intact; two with two
    corrupted survivors, only where three spares remain; t = m - 1 with and without damage; t = m;
    two with t = m + 1."""
    G, k, _ = hd.shape
    m = hp.shape[1]
    gm = np.zeros((G, k + m), np.uint8)
    for g in range(G):
        r = g % 20
        if r < 11:
            t, nc = int(rng.integers(0, m - 1)), 1
        elif r < 13:
            t, nc = int(rng.integers(0, m - 1)), 0
        elif r < 15:
            t, nc = int(rng.integers(0, m - 2)), 2
        elif r < 17:
            t, nc = m - 1, r % 2
        elif r < 18:
            t, nc = m, 0
        else:
            t, nc = m + 1, 0
        left = lose(rng, hd, hp, gm, g, t)
        for c in rng.choice(left, size=nc, replace=False):
            hurt(rng, row_of(hd, hp, g, c), int(rng.integers(0, 3)))
    return gm


@functools.lru_cache(maxsize=None)
def scrub_case(flavour, k, m, G, B, narrow=False):
    """The damaged batch, its originals, and the contiguous scrub's answer on the padded rows."""
    code, d0, p0 = host_batch(flavour, k, m, B, G)
    hd, hp = d0.copy(), p0.copy()
    gm = random_loss_and_damage(np.random.default_rng(k + m), hd, hp)
    expect, _, want_counts = model(code, hd, hp, gm, B)
    assert (expect >= 0).sum() >= G // 3 and all((expect == v).any() for v in (CLEAN, MULTI, AMBIGUOUS, UNCHECKED, LOST))
    d, p = pc.padded(torch, DEV, hd, B), pc.padded(torch, DEV, hp, B)
    counts = torch.zeros(5, dtype=torch.int32, device=DEV)
    failed = torch.zeros(1, dtype=torch.int32, device=DEV)
    fn = code.scrub_erased if narrow else code.scrub_wide
    culprit = fn(d, p, to_dev(marks_to_rs_layout(gm, k)), B, counts=counts, failed=failed)
    torch.cuda.synchronize()
    ref = (culprit.cpu().numpy(), d.cpu().numpy()[..., :B], p.cpu().numpy()[..., :B], counts.cpu().numpy(),
           int(failed.item()))
    assert np.array_equal(ref[0], expect) and list(ref[3]) == list(want_counts)
    return code, d0, p0, hd, hp, gm, expect, ref


def assert_scrub(case, mode, B):
    code, d0, p0, hd, hp, gm, expect, ref = case
    G, n = gm.shape
    k, m = code.k, code.m
    pool = pool_of(hd, hp, mode, k + m + B)
    t, ptrs = pc.to_device(torch, DEV, pool)
    marks_h = marks_to_rs_layout(gm, k)
    marks = to_dev(marks_h)
    counts = torch.zeros(5, dtype=torch.int32, device=DEV)
    failed = torch.zeros(1, dtype=torch.int32, device=DEV)
    culprit = code.scrub_ptrs_wide(ptrs, B, marks, counts=counts, failed=failed)
    torch.cuda.synchronize()
    assert np.array_equal(culprit.cpu().numpy(), ref[0])
    assert list(counts.cpu().numpy()) == list(ref[3]) and int(failed.item()) == ref[4] == (expect == LOST).sum()
    assert np.array_equal(marks.cpu().numpy(), marks_h)  # the caller's marks are not written
    # the pool before, with only the located shard and the marked shards of its group back to the
    # original bytes: every other row of a healed group holds them already
    left_alone = np.isin(expect, (MULTI, AMBIGUOUS, LOST))
    wd, wp = hd.copy(), hp.copy()
    wd[~left_alone], wp[~left_alone] = d0[~left_alone], p0[~left_alone]
    assert np.array_equal(wd, ref[1]) and np.array_equal(wp, ref[2])  # what the contiguous scrub left in [0, B)
    flat = pool.host.copy()
    put_rows(pool, flat, 0, wd.reshape(G * k, B))
    put_rows(pool, flat, G * k, wp.reshape(G * m, B))
    got = t.cpu().numpy()
    assert np.array_equal(got, flat), np.nonzero(got != flat)[0][:8]
    assert not np.array_equal(flat, pool.host)  # something was repaired
    return pool, marks


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("flavour,k,m,G", [("cauchy", 32, 8, 60), ("vandermonde", 64, 16, 48), ("cauchy", 200, 55, 40)])
def test_scrub_ptrs_wide(flavour, k, m, G, mode):
    B = 100
    case = scrub_case(flavour, k, m, G, B)
    pool, marks = assert_scrub(case, mode, B)
    # the verdicts and the counters are optional
    code = case[0]
    t2, ptrs2 = pc.to_device(torch, DEV, pool)
    assert qa.lib().qfec_scrub_ptrs_wide(code._h, ptrs2.data_ptr(), marks.data_ptr(), G, B, None, None, None, None) == 0
    torch.cuda.synchronize()
    t1, ptrs1 = pc.to_device(torch, DEV, pool)
    code.scrub_ptrs_wide(ptrs1, B, marks)
    torch.cuda.synchronize()
    assert torch.equal(t1, t2)


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("B", [96, 100])
def test_scrub_ptrs_wide_is_scrub_erased_on_a_narrow_code(B, mode):
    assert_scrub(scrub_case("cauchy", 16, 4, 80, B, narrow=True), mode, B)


# ---------------------------------------------------------------- 8. refusals on the device path
def test_misaligned_check_plan_is_refused():
    """A slice of a tensor that starts off the 16-byte grid; nothing is written."""
    code, hd, hp, gm, _ = family(32, 8, 33)
    G, n = gm.shape
    stride = code.check_stride()
    pool = pool_of(hd, hp, "aligned", 1)
    t, ptrs = pc.to_device(torch, DEV, pool)
    before = t.clone()
    flat = torch.full((G * stride + 16,), 0xEE, dtype=torch.uint8, device=DEV)
    culprit = torch.full((G,), 1234, dtype=torch.int32, device=DEV)
    out = torch.full((G * n,), 0xEE, dtype=torch.uint8, device=DEV)
    counts = torch.full((5,), 7, dtype=torch.int32, device=DEV)
    for off in (1, 4, 8):
        plans = flat[off:off + G * stride].view(G, stride)
        with pytest.raises(qa.QfecError, match="qfec_check_apply_ptrs: .*d_check not 16-byte aligned"):
            code.check_apply_ptrs(ptrs, plans, 33, culprit=culprit, marks_out=out, counts=counts)
    torch.cuda.synchronize()
    assert bool((flat == 0xEE).all()) and bool((culprit == 1234).all()) and bool((out == 0xEE).all())
    assert bool((counts == 7).all()) and torch.equal(t, before)
