"""GPU tests of qfec_check_apply_ptrs_var / qfec_locate_ptrs_wide_var / qfec_scrub_ptrs_wide_var: single-shard
error location at any k + m on shards scattered in device memory, each with its own length.  The
reference is never the code under test: the numpy model of the definition
(locate_ptrs_wide_var_common.model) for every case; where they are defined, qfec_locate_ptrs_wide and
qfec_scrub_ptrs_wide on the same rows zero-padded into slots of L bytes, and qfec_locate_ptrs_var on
complete groups of a narrow code.  All comparisons are exact integers and bytes.

The rows lie in a pool whose every other byte is random (locate_ptrs_wide_var_common.Case), in a random
permutation of slots, and the WHOLE pool is compared after every call: a byte written anywhere by a
locate fails, and so does a byte written outside [0, len_i) of a located data shard or outside [0, L) of
a lost shard by the scrub; a byte read past a shard's own end turns a verdict.  The table entries of
marked shards (locates), of unmarked shards of length 0 and of invalid groups are WILD, misaligned
addresses far from any allocation.

Run on an MI355X:  python -m pytest tests/test_gpu_locate_ptrs_wide_var.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import locate_ptrs_wide_var_common as lv
import ptrs_common as pc
import quicknet_amd as qa
from locate_ptrs_wide_var_common import AMBIGUOUS, CLEAN, INVALID, LOST, MULTI, UNCHECKED
from ptrs_wide_common import put_rows
from quicknet_amd.synth import marks_to_rs_layout

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
MODES = lv.MODES


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def on_device(case, scrub=False, image=None):
    """(pool tensor, table, d_lens, d_group_len) of a case."""
    t = dev(case.image if image is None else image)
    assert t.data_ptr() % 16 == 0
    return t, dev(case.table(t.data_ptr(), scrub)), dev(case.d_lens()), dev(case.glen.astype(np.int32))


def run(case, call="locate", use_marks=True, alias_out=False, counts=None, invalid=0, plans=None):
    """qfec_locate_ptrs_wide_var (or qfec_check_build + qfec_check_apply_ptrs_var) -> (culprit, marks_out,
    counts, invalid) on the host.  Also: the whole pool and the marks are as they were."""
    code, G, n = case.code, case.G, case.k + case.m
    t, ptrs, lens, glen = on_device(case)
    before = t.clone()
    marks_h = case.marks()
    marks = dev(marks_h)
    out = marks if alias_out else torch.full((G * n,), 0xEE, dtype=torch.uint8, device=DEV)
    culprit = torch.full((G,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(5, dtype=torch.int32, device=DEV)
    if counts is not None:
        cnt.copy_(torch.from_numpy(np.asarray(counts, np.int32)))
    inv = torch.full((1,), invalid, dtype=torch.int32, device=DEV)
    if call == "locate":
        res = code.locate_ptrs_wide_var(ptrs, lens, glen, case.max_len, marks if use_marks else None, culprit=culprit,
                                        marks_out=out, counts=cnt, invalid=inv)
    else:
        if plans is None:
            plans = code.check_build(marks if use_marks else None, groups=G)
        res = code.check_apply_ptrs_var(ptrs, lens, glen, plans, case.max_len, culprit=culprit, marks_out=out, counts=cnt,
                                        invalid=inv)
    torch.cuda.synchronize()
    assert res is culprit
    assert torch.equal(t, before), "a locate wrote into the pool"
    if not alias_out:
        assert np.array_equal(marks.cpu().numpy(), marks_h)
    return culprit.cpu().numpy(), out.cpu().numpy(), cnt.cpu().numpy(), int(inv.item())


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, np.nonzero(got[0] != want[0])[0][:8], got[0][got[0] != want[0]][:8],
                                             want[0][got[0] != want[0]][:8])
    assert np.array_equal(got[1], want[1]), what
    assert list(got[2]) == list(want[2]), what
    assert got[3] == want[3], what


# ---------------------------------------------------------------- 1. the model, every code, length and mode
@functools.lru_cache(maxsize=None)
def whole(k, m, max_len, mode="aligned"):
    """The family's complete groups as a batch of their own, for d_marks = NULL."""
    if mode != "aligned":
        return whole(k, m, max_len).in_mode(mode)
    fam = lv.family(k, m, max_len)
    specs = [s for s in fam.specs if not np.asarray(s["marks"]).any()]
    assert len(specs) >= 8
    return lv.make(fam.code, specs, max_len, "aligned", 11 * k + max_len)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,m,max_len", lv.FAMILY)
def test_answers_as_the_model(k, m, max_len, mode):
    case = lv.family(k, m, max_len, mode)
    want = case.expect()
    t = case.table(1 << 40)
    wild = (t >= lv.WILD).reshape(-1)
    marked = marks_to_rs_layout(case.gm, k) != 0
    assert (wild & marked).any() and (wild & ~marked).sum() > 5 * (k + m)  # marked; invalid groups and length 0
    same(run(case), want, "locate_ptrs_wide_var")
    same(run(case, call="apply"), want, "check_apply_ptrs_var")
    sub = whole(k, m, max_len, mode)
    assert (sub.expect()[0] >= 0).any() and (sub.expect()[0] == MULTI).any()
    same(run(sub, use_marks=False), sub.expect(), "no marks")
    same(run(sub, call="apply", use_marks=False), sub.expect(), "no marks, apply")


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("max_len", [17, 1025, 1400])
def test_complete_groups_of_a_narrow_code_as_locate_ptrs_var(max_len, mode):
    case = whole(10, 3, max_len, mode)
    t, ptrs, lens, glen = on_device(case)
    cnt = torch.zeros(3, dtype=torch.int32, device=DEV)
    inv = torch.zeros(1, dtype=torch.int32, device=DEV)
    narrow = case.code.locate_ptrs_var(ptrs, lens, glen, max_len, counts=cnt, invalid=inv)
    torch.cuda.synchronize()
    got = run(case, use_marks=False)
    assert np.array_equal(got[0], narrow.cpu().numpy())
    assert list(got[2][:3]) == list(cnt.cpu().numpy()) and got[3] == int(inv.item())


# ---------------------------------------------------------------- 2. the fixed-length call on padded rows
def fixed_length(case, groups, L):
    """qfec_locate_ptrs_wide with block_size = L on the rows of `groups`, zero-padded into slots of L bytes."""
    k, m, G = case.k, case.m, len(groups)
    hd, hp, gm = case.hd[groups][..., :L], case.hp[groups][..., :L], case.gm[groups]
    pool = pc.Pool(G * (k + m), L, np.zeros(G * (k + m), np.int64), L)
    put_rows(pool, pool.host, 0, np.ascontiguousarray(hd).reshape(G * k, L))
    put_rows(pool, pool.host, G * k, np.ascontiguousarray(hp).reshape(G * m, L))
    t, ptrs = pc.to_device(torch, DEV, pool)
    culprit = case.code.locate_ptrs_wide(ptrs, L, dev(marks_to_rs_layout(gm, k)))
    torch.cuda.synchronize()
    return culprit.cpu().numpy()


@pytest.mark.parametrize("k,m,max_len", [(10, 3, 17), (32, 8, 1025), (70, 10, 17), (200, 55, 17)])
def test_as_the_fixed_length_call_on_zero_padded_rows(k, m, max_len):
    """Per group length L: the verdicts are qfec_locate_ptrs_wide's on the padded rows, except where that
    call names a data shard although a syndrome is non-zero past the shard's own end: MULTI here."""
    case = lv.family(k, m, max_len)
    got = run(case)[0]
    differ = 0
    for L in sorted(set(case.glen[~case.bad & (case.glen > 0)].tolist())):
        groups = np.flatnonzero(~case.bad & (case.glen == L))
        ref = fixed_length(case, groups, int(L))
        for g, r in zip(groups, ref):
            if got[g] != r:
                assert 0 <= r < k and case.lens[g, r] < L and got[g] == MULTI and case.specs[g]["phantom"], (g, r, got[g])
                differ += 1
    assert differ >= 1


# ---------------------------------------------------------------- 3. group lengths and shard ends at the seams
def seam_ends(L):
    v = L // 16 * 16
    return sorted({e for e in (1, v, v + 1, 1023, 1024, 1025, L) if 1 <= e <= L})


@functools.lru_cache(maxsize=None)
def seam_case(L, max_len):
    """(32,8), every group of length L: per end e of seam_ends(L) one data shard of e bytes beside shards
    of L bytes and t = 0, 1, 2 lost shards; damage at byte 0 of it, at byte e - 1, at byte L - 1 of a parity
    shard, and a phantom byte at e (wrong past its own end); then the same groups undamaged."""
    k, m = 32, 8
    n = k + m
    code = qa.Code.cauchy(k, m)
    rng = np.random.default_rng(L)
    specs, expect = [], []
    for i, e in enumerate(seam_ends(L)):
        c = (7 * i + 3) % k
        lens = np.full(k, L, np.int64)
        lens[c] = e
        lens[(c + 5) % k] = 0
        for j, (hits, phantom, v) in enumerate([([(c, 0, 0x11)], [], c), ([(c, e - 1, 0x80)], [], c),
                                                ([(n - 2, L - 1, 0x3C)], [], n - 2), ([], [(c, e, 0x01)], MULTI), ([], [], CLEAN)]):
            if phantom and e == L:
                continue
            specs.append(dict(lens=lens, L=L, marks=lv.lose(rng, n, (i + j) % 3, keep=(c, n - 2)), hits=hits, phantom=phantom))
            expect.append(v)
    case = lv.make(code, specs, max_len, "aligned", 100 + L)
    assert np.array_equal(case.expect()[0], np.array(expect, np.int32))
    return case


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("L", [1, 15, 16, 17, 1024, 1025])
def test_group_lengths_and_shard_ends_at_the_seams(L, mode):
    """Also: an undamaged short shard is followed by random bytes, and stays CLEAN -- nothing is read there."""
    for max_len in sorted({L, 1400}):
        case = seam_case(L, max_len).in_mode(mode)
        same(run(case), case.expect(), f"max_len {max_len}")


# ---------------------------------------------------------------- 4. plan reuse, aliasing, counters, optional outputs
def test_one_check_plan_serves_two_tables():
    k, m, max_len = 70, 10, 17
    a = lv.family(k, m, max_len)
    plans = a.code.check_build(dev(a.marks()))
    torch.cuda.synchronize()
    # the same losses and lengths, other bytes and other damage
    specs = [dict(s, hits=[(c, b, v ^ 0xFF or 1) for c, b, v in s.get("hits", ())][:1]) for s in a.specs]
    b = lv.make(a.code, specs, max_len, "residues", 4242)
    assert not np.array_equal(a.expect()[0], b.expect()[0])
    same(run(a, call="apply", plans=plans), a.expect(), "first table")
    same(run(b, call="apply", plans=plans), b.expect(), "second table")


@pytest.mark.parametrize("mode", ["aligned", "residues"])
def test_marks_out_may_be_marks_and_counters_accumulate(mode):
    case = lv.family(32, 8, 1025, mode)
    want = case.expect()
    first = run(case)
    assert first[3] == 6 and first[2].sum() + (want[0] == CLEAN).sum() + 6 == case.G  # invalid groups count nowhere
    culprit, aliased, counts, invalid = run(case, alias_out=True, counts=first[2], invalid=first[3])
    assert np.array_equal(culprit, want[0]) and np.array_equal(aliased, first[1])
    assert list(counts) == list(2 * want[2]) and invalid == 12


def test_optional_outputs_may_be_null():
    case = lv.family(32, 8, 17)
    t, ptrs, lens, glen = on_device(case)
    culprit = torch.zeros(case.G, dtype=torch.int32, device=DEV)
    L = qa.lib()
    assert L.qfec_locate_ptrs_wide_var(case.code._h, ptrs.data_ptr(), lens.data_ptr(), glen.data_ptr(),
                                       dev(case.marks()).data_ptr(), case.G, 17, culprit.data_ptr(), None, None, None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(culprit.cpu().numpy(), case.expect()[0])
    plans = case.code.check_build(dev(case.marks()))
    culprit.zero_()
    assert L.qfec_check_apply_ptrs_var(case.code._h, ptrs.data_ptr(), lens.data_ptr(), glen.data_ptr(), plans.data_ptr(),
                                       case.G, 17, culprit.data_ptr(), None, None, None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(culprit.cpu().numpy(), case.expect()[0])


def test_misaligned_check_plan_is_refused():
    """A slice of a tensor that starts off the 16-byte grid; nothing is written."""
    case = lv.family(32, 8, 17)
    G, n = case.G, 40
    stride = case.code.check_stride()
    t, ptrs, lens, glen = on_device(case)
    before = t.clone()
    flat = torch.full((G * stride + 16,), 0xEE, dtype=torch.uint8, device=DEV)
    culprit = torch.full((G,), 1234, dtype=torch.int32, device=DEV)
    out = torch.full((G * n,), 0xEE, dtype=torch.uint8, device=DEV)
    counts = torch.full((5,), 7, dtype=torch.int32, device=DEV)
    inv = torch.full((1,), 9, dtype=torch.int32, device=DEV)
    for off in (1, 4, 8):
        plans = flat[off:off + G * stride].view(G, stride)
        with pytest.raises(qa.QfecError, match="qfec_check_apply_ptrs_var: .*d_check not 16-byte aligned"):
            case.code.check_apply_ptrs_var(ptrs, lens, glen, plans, 17, culprit=culprit, marks_out=out, counts=counts,
                                           invalid=inv)
    torch.cuda.synchronize()
    assert bool((flat == 0xEE).all()) and bool((culprit == 1234).all()) and bool((out == 0xEE).all())
    assert bool((counts == 7).all()) and int(inv.item()) == 9 and torch.equal(t, before)


# ---------------------------------------------------------------- 5. chunking
def test_more_than_one_chunk_of_plans():
    """The one-shot keeps one chunk's plans under 64 MiB: (200,55) goes in chunks of 3 034 groups.  Damage,
    short shards and invalid lengths on both sides of the cut and in the last group; the model judges
    those groups, every other group is complete, consistent and of full length."""
    k, m, max_len = 200, 55, 17
    n = k + m
    code = qa.Code.cauchy(k, m)
    per = (64 << 20) // code.check_stride()
    G = per + 40
    assert (per, G) == (3034, 3074)
    rng = np.random.default_rng(3)
    full = dict(lens=np.full(k, max_len, np.int64), L=max_len, marks=np.zeros(n, np.uint8))
    specs = [full] * G
    hit = [0, per - 1, per, per + 1, G - 1]
    lens = np.minimum(np.arange(k, dtype=np.int64) % 19, 16)
    for i, g in enumerate(hit):
        specs[g] = lv.spec_for(rng, k, m, lens, 16, 1 + i, lv.KINDS[1 + i % 4])
    bad = lens.copy()
    bad[7] = 17
    specs[per + 2] = dict(lens=bad, L=16, marks=np.zeros(n, np.uint8))
    specs[per - 2] = dict(lens=lens, L=16, marks=lv.lose(rng, n, m))
    case = lv.make(code, specs, max_len, "aligned", 17)
    sub = hit + [per + 2, per - 2]
    small = lv.make(code, [specs[g] for g in sub], max_len, "aligned", 17)
    # the same seed gives other bytes to the small batch, but the verdict of these groups follows from
    # the damage alone: the ids the specs name
    expect = np.full(G, CLEAN, np.int32)
    for g, v in zip(sub, small.expect()[0]):
        expect[g] = v
    assert (expect[hit] >= 0).all() and expect[per + 2] == INVALID and expect[per - 2] == UNCHECKED
    assert [s["hits"][0][0] for s in (specs[g] for g in hit)] == list(expect[hit])
    culprit, marks_out, counts, invalid = run(case)
    assert np.array_equal(culprit, expect)
    marked = (case.gm != 0).astype(np.uint8)
    marked[hit, expect[hit]] = 1
    assert np.array_equal(marks_out, marks_to_rs_layout(marked, k))
    assert list(counts) == [len(hit), 0, 0, 1, 0] and invalid == 1


# ---------------------------------------------------------------- 6. scrub
def scrub(case, image=None, raw=False):
    """qfec_scrub_ptrs_wide_var on the case's pool -> (pool after, culprit, counts, failed, invalid)."""
    t, ptrs, lens, glen = on_device(case, scrub=True, image=image)
    marks_h = case.marks()
    marks = dev(marks_h)
    counts = torch.zeros(5, dtype=torch.int32, device=DEV)
    failed = torch.zeros(1, dtype=torch.int32, device=DEV)
    inv = torch.zeros(1, dtype=torch.int32, device=DEV)
    if raw:  # the verdicts and the counters are optional
        assert qa.lib().qfec_scrub_ptrs_wide_var(case.code._h, ptrs.data_ptr(), lens.data_ptr(), glen.data_ptr(),
                                                 marks.data_ptr(), case.G, case.max_len, None, None, None, None, None) == 0
        torch.cuda.synchronize()
        return t.cpu().numpy(), None, None, None, None
    culprit = case.code.scrub_ptrs_wide_var(ptrs, lens, glen, case.max_len, marks, counts=counts, failed=failed, invalid=inv)
    torch.cuda.synchronize()
    assert np.array_equal(marks.cpu().numpy(), marks_h)  # the caller's marks are not written
    return t.cpu().numpy(), culprit.cpu().numpy(), counts.cpu().numpy(), int(failed.item()), int(inv.item())


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m,max_len", [(32, 8, 1025), (64, 16, 1025), (200, 55, 17)])
def test_scrub_ptrs_wide_var(k, m, max_len, mode):
    """Against the pool before the damage: lost shards rewritten in [0, L), a located data shard in
    [0, len_i) with the random bytes right behind it unchanged, a located parity shard in [0, L); MULTI,
    AMBIGUOUS, INVALID and LOST groups untouched byte for byte."""
    case = lv.family(k, m, max_len, mode)
    want = case.expect(True)
    v = want[0]
    short = [g for g in range(case.G) if 0 <= v[g] < k and case.lens[g, v[g]] < case.glen[g]]
    assert short and (v >= k).any() and all((v == x).any() for x in (CLEAN, MULTI, AMBIGUOUS, UNCHECKED, LOST, INVALID))
    assert any(case.gm[g].any() for g in np.flatnonzero(v == CLEAN)), "a CLEAN group with losses"
    after, culprit, counts, failed, invalid = scrub(case)
    assert np.array_equal(culprit, v), (np.nonzero(culprit != v)[0][:8])
    assert list(counts) == list(want[2]) and failed == (v == LOST).sum() and invalid == want[3] == 6
    expect = case.scrubbed()
    assert np.array_equal(after, expect), np.nonzero(after != expect)[0][:8]
    assert not np.array_equal(expect, case.image)  # something was repaired
    assert np.array_equal(scrub(case, raw=True)[0], expect)


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m,max_len", [(32, 8, 100), (200, 55, 17)])
def test_with_all_lengths_equal_the_scrub_is_scrub_ptrs_wide(k, m, max_len, mode):
    fam = lv.family(k, m, 17)
    specs = [dict(lens=np.full(k, max_len, np.int64), L=max_len, marks=s["marks"],
                  hits=[(c, b % max_len, x) for c, b, x in s.get("hits", ())]) for s in fam.specs[:len(fam.specs) - 10]]
    case = lv.make(fam.code, specs, max_len, mode, 5 * k)
    v = case.expect(True)[0]
    assert (v >= 0).sum() >= 8 and all((v == x).any() for x in (CLEAN, MULTI, AMBIGUOUS, UNCHECKED, LOST))
    after, culprit, counts, failed, invalid = scrub(case)
    t, ptrs, _, _ = on_device(case, scrub=True)
    c2 = torch.zeros(5, dtype=torch.int32, device=DEV)
    f2 = torch.zeros(1, dtype=torch.int32, device=DEV)
    ref = case.code.scrub_ptrs_wide(ptrs, max_len, dev(case.marks()), counts=c2, failed=f2)
    torch.cuda.synchronize()
    assert np.array_equal(culprit, ref.cpu().numpy()) and np.array_equal(culprit, v)
    assert list(counts) == list(c2.cpu().numpy()) and failed == int(f2.item()) and invalid == 0
    assert np.array_equal(after, t.cpu().numpy()) and np.array_equal(after, case.scrubbed())
