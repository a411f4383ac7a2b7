"""GPU tests of every host dispatch branch of the integrity and update calls: each templated (k, m)
instance on its 16-B path, the runtime-k,m kernels through the second pass of their 64-column loops,
the byte-granular kernels on wide rows and behind each misaligned base on its own, and the
documented limits (m = 32, k = 32, k + m = 24, k = 254).  Shapes, layouts, guarded buffers and the
expectations are dispatch_common's: every comparison is exact, against the oracle's encode /
reconstruct / multiply or the construction of the damage.  After every call both guards of every
buffer are held to their pattern, read-only calls to unchanged inputs over the whole pitch, and
writers to the bytes they own.  Ids read family-k-m-layout.

Run on an MI355X:  python -m pytest tests/test_gpu_dispatch.py -m gpu -q
"""
import functools
import types

import numpy as np
import pytest

import dispatch_common as dc
import quicknet_amd as qa
from dispatch_common import LAYOUTS, Guarded, batch, cases, case_ids, groups_for, written_from
from locate2_common import CLEAN, MULTI, counts_of, expected_locate2
from quicknet_amd.synth import marks_to_rs_layout, synth_bytes
from repair_common import damage, expected_repair, random_marks

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def code_for(k, m):
    """One code per shape for the whole module: its device tables and LUTs are built once."""
    return qa.Code.cauchy(k, m)


def geom(layout):
    """The layout less its name and base offsets: what a host-side plan depends on."""
    return layout._replace(name="", data_off=0, parity_off=0, rows_off=0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ints(n):
    return torch.zeros(n, dtype=torch.int32, device=DEV)


def out_ints(shape, fill=0x5A):
    """A guarded int32 output of the given shape, every byte preset to `fill` -> (buffer, tensor)."""
    shape = (shape,) if isinstance(shape, int) else shape
    g = Guarded(np.full(4 * int(np.prod(shape)), fill, np.uint8))
    return g, g.t.view(torch.int32).view(shape)


def out_marks(count):
    """A guarded uint8 marks output preset to 0xEE -> (buffer, tensor)."""
    g = Guarded(np.full(count, 0xEE, np.uint8))
    return g, g.t


def guards(*bufs):
    for b in bufs:
        b.check_guards("an output")


def place(layout, data, par):
    return Guarded(data, layout.data_off), Guarded(par, layout.parity_off)


def held(buf, before, what):
    """A buffer a call may only read: guards intact and every byte as before."""
    buf.check_guards(what)
    assert np.array_equal(buf.host(), before), f"{what}: a read-only buffer was written"


def start(oracle, k, m, lname):
    layout = LAYOUTS[lname]
    code = code_for(k, m)
    rows, d0, p0 = batch(oracle, k, m, layout)
    assert np.array_equal(code.rows, rows)
    assert (groups_for(k, m) * dc.lanes(layout)) % 256 and groups_for(k, m) % 4
    return layout, code, rows, d0, p0


def same_as_fast(run, oracle, k, m, lname, got):
    """The verdicts / [0, B) outputs on a misaligned-base layout equal those on `fast`: same B, same
    damage, the 16-B kernels against the byte kernels."""
    if lname in dc.OFF_BASE:
        for a, b in zip(got, run(oracle, k, m, "fast")):
            assert (a is None and b is None) or np.array_equal(a, b), "differs from the fast layout"


# ------------------------------------------------------------------ verify

@functools.lru_cache(maxsize=None)
def verify_plan(oracle, k, m, g):
    rows, d, p = batch(oracle, k, m, g)
    made = dc.damage_every_shard(d, p, g.B)
    want = dc.bad_rows_model(oracle, rows, d, p, g.B)
    for j in range(m):  # a damaged parity row shows in its own bit alone
        assert want[3 * (k + j) + 1] == np.uint32(1) << np.uint32(j)
    assert np.array_equal(want != 0, made >= 0)
    return d, p, want


@functools.lru_cache(maxsize=None)
def run_verify(oracle, k, m, lname):
    layout, code, rows, d0, p0 = start(oracle, k, m, lname)
    B, G = layout.B, len(d0)
    count = ints(1)
    dd, dp = place(layout, d0, p0)
    bad = code.verify(dd.t, dp.t, B, bad_groups=count)
    torch.cuda.synchronize()
    assert not bad.cpu().numpy().any() and int(count.item()) == 0
    held(dd, d0, "verify data")
    held(dp, p0, "verify parity")
    d1, p1, want = verify_plan(oracle, k, m, geom(layout))
    dd, dp = place(layout, d1, p1)
    gb, bad = out_ints(G)
    assert code.verify(dd.t, dp.t, B, bad_rows=bad, bad_groups=count) is bad
    torch.cuda.synchronize()
    guards(gb)
    got = bad.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want)
    if m == 32:
        assert got.max() >> 31 == 1
    assert int(count.item()) == int((want != 0).sum())
    held(dd, d1, "verify data")
    held(dp, p1, "verify parity")
    return (got,)


@pytest.mark.parametrize("k,m,lname", cases("verify"), ids=case_ids("verify"))
def test_verify(oracle, k, m, lname):
    """A consistent batch gives all zeros; with every shard damaged once, bad_rows read as uint32
    equals the model's bits and the counter the number of bad groups."""
    same_as_fast(run_verify, oracle, k, m, lname, run_verify(oracle, k, m, lname))


# ------------------------------------------------------------------ locate / scrub

@functools.lru_cache(maxsize=None)
def locate_plan(oracle, k, m, g):
    rows, d, p = batch(oracle, k, m, g)
    made = dc.damage_every_shard(d, p, g.B)
    want = dc.expected_locate1(oracle, rows, d, p, g.B)
    assert np.array_equal(want, made)
    if k + m <= 24:  # the single-shard stage of the two-shard model says the same
        assert np.array_equal(expected_locate2(oracle, rows, "cauchy", d, p, g.B)[:, 0], want)
    return d, p, want


def check_scrubbed(layout, got, damaged, original, healed, touched, what):
    """After a scrub / repair of host array damaged [G, r, pitch]: healed groups equal the original
    in [0, B), the others are as they were, no byte from written_from(layout) on and no row outside
    `touched` [G, r] moved."""
    B, wf = layout.B, written_from(layout)
    assert np.array_equal(got[healed][..., :B], original[healed][..., :B]), f"{what}: not the original bytes"
    assert np.array_equal(got[~healed], damaged[~healed]), f"{what}: a group left alone was written"
    assert np.array_equal(got[..., wf:], damaged[..., wf:]), f"{what}: bytes beyond the block written"
    assert np.array_equal(got[~touched], damaged[~touched]), f"{what}: an unmarked row was written"


@functools.lru_cache(maxsize=None)
def run_locate(oracle, k, m, lname):
    layout, code, rows, d0, p0 = start(oracle, k, m, lname)
    B, G, n = layout.B, len(d0), k + m
    d1, p1, want = locate_plan(oracle, k, m, geom(layout))
    want_marks = dc.marks_n(want, n)
    if k >= 32 or m >= 32:
        assert want.max() >= 32
    dd, dp = place(layout, d1, p1)
    (gc, culprit), (gk, marks), counts = out_ints(G), out_marks(G * n), ints(3)
    code.locate(dd.t, dp.t, B, culprit=culprit, marks=marks, counts=counts)
    torch.cuda.synchronize()
    guards(gc, gk)
    got = culprit.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(marks.cpu().numpy(), marks_to_rs_layout(want_marks, k))
    assert list(counts.cpu().numpy()) == dc.counts_of1(want)
    held(dd, d1, "locate data")
    held(dp, p1, "locate parity")
    if n > 24:
        return got, None, None
    counts = ints(3)
    got2 = code.scrub(dd.t, dp.t, B, counts=counts)
    torch.cuda.synchronize()
    assert np.array_equal(got2.cpu().numpy(), want) and list(counts.cpu().numpy()) == dc.counts_of1(want)
    dd.check_guards("scrub data")
    dp.check_guards("scrub parity")
    out_d, out_p = dd.host(), dp.host()
    healed = np.ones(G, bool)
    check_scrubbed(layout, out_d, d1, d0, healed, want_marks[:, :k] == 1, "scrub data")
    check_scrubbed(layout, out_p, p1, p0, healed, want_marks[:, k:] == 1, "scrub parity")
    return got, out_d[..., :B], out_p[..., :B]


@pytest.mark.parametrize("k,m,lname", cases("locate"), ids=case_ids("locate"))
def test_locate(oracle, k, m, lname):
    """Every shard id corrupted once, the other groups clean: culprit, marks and counts equal the
    model; up to k + m = 24 the scrub then restores [0, B) of every group."""
    same_as_fast(run_locate, oracle, k, m, lname, run_locate(oracle, k, m, lname))


# ------------------------------------------------------------------ locate_erased / scrub_erased

@functools.lru_cache(maxsize=None)
def erased_plan(oracle, k, m, g):
    rows, d, p = batch(oracle, k, m, g)
    gm, want = dc.erased_damage(d, p, g.B, 31 * k + m)
    t = (gm != 0).sum(1)
    assert t.max() == m - 2 and (m < 3 or ((want >= 0) & (t > 0)).any())
    return d, p, gm, want


@functools.lru_cache(maxsize=None)
def run_locate_erased(oracle, k, m, lname):
    layout, code, rows, d0, p0 = start(oracle, k, m, lname)
    B, G, n = layout.B, len(d0), k + m
    d1, p1, gm, want = erased_plan(oracle, k, m, geom(layout))
    want_marks = dc.erased_marks(gm, want)
    want_counts = [int((want >= 0).sum()), int((want == MULTI).sum()), 0, 0, 0]
    assert want_counts[1] == (m >= 3)
    marks_in = marks_to_rs_layout(gm, k)
    dd, dp = place(layout, d1, p1)
    marks = dev(marks_in)
    (gc, culprit), (gk, out), counts = out_ints(G), out_marks(G * n), ints(5)
    code.locate_erased(dd.t, dp.t, marks, B, culprit=culprit, marks_out=out, counts=counts)
    torch.cuda.synchronize()
    guards(gc, gk)
    got = culprit.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(out.cpu().numpy(), marks_to_rs_layout(want_marks, k))
    assert list(counts.cpu().numpy()) == want_counts
    assert np.array_equal(marks.cpu().numpy(), marks_in)
    held(dd, d1, "locate_erased data")
    held(dp, p1, "locate_erased parity")
    counts, failed = ints(5), ints(1)
    got2 = code.scrub_erased(dd.t, dp.t, marks, B, counts=counts, failed=failed)
    torch.cuda.synchronize()
    assert np.array_equal(got2.cpu().numpy(), want) and list(counts.cpu().numpy()) == want_counts
    assert int(failed.item()) == 0 and np.array_equal(marks.cpu().numpy(), marks_in)
    dd.check_guards("scrub_erased data")
    dp.check_guards("scrub_erased parity")
    out_d, out_p = dd.host(), dp.host()
    healed = want != MULTI
    check_scrubbed(layout, out_d, d1, d0, healed, want_marks[:, :k] == 1, "scrub_erased data")
    check_scrubbed(layout, out_p, p1, p0, healed, want_marks[:, k:] == 1, "scrub_erased parity")
    return got, out_d[..., :B], out_p[..., :B]


@pytest.mark.parametrize("k,m,lname", cases("locate_erased"), ids=case_ids("locate_erased"))
def test_locate_erased(oracle, k, m, lname):
    """Every shard id corrupted once beside 0 .. m - 2 lost shards, a culprit damaged in two passes,
    two survivors damaged in different passes (MULTI): verdicts, marks_out and counts by
    construction; the scrub restores every group but the MULTI one."""
    same_as_fast(run_locate_erased, oracle, k, m, lname, run_locate_erased(oracle, k, m, lname))


# ------------------------------------------------------------------ locate2 / scrub2

@functools.lru_cache(maxsize=None)
def locate2_plan(oracle, k, m, g):
    rows, d, p = batch(oracle, k, m, g)
    made = dc.locate2_damage(d, p, g.B)
    want = expected_locate2(oracle, rows, "cauchy", d, p, g.B)
    by_construction = np.full_like(want, CLEAN)
    for grp, slots in made:
        by_construction[grp] = slots
    assert np.array_equal(want, by_construction)
    return d, p, want


@functools.lru_cache(maxsize=None)
def run_locate2(oracle, k, m, lname):
    layout, code, rows, d0, p0 = start(oracle, k, m, lname)
    B, G, n = layout.B, len(d0), k + m
    d1, p1, want = locate2_plan(oracle, k, m, geom(layout))
    want_marks = dc.marks_n(want, n)
    dd, dp = place(layout, d1, p1)
    (gc, culprit), (gk, marks), counts = out_ints((G, 2)), out_marks(G * n), ints(4)
    code.locate2(dd.t, dp.t, B, culprit=culprit, marks=marks, counts=counts)
    torch.cuda.synchronize()
    guards(gc, gk)
    got = culprit.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(marks.cpu().numpy(), marks_to_rs_layout(want_marks, k))
    assert list(counts.cpu().numpy()) == counts_of(want)
    held(dd, d1, "locate2 data")
    held(dp, p1, "locate2 parity")
    counts = ints(4)
    got2 = code.scrub2(dd.t, dp.t, B, counts=counts)
    torch.cuda.synchronize()
    assert np.array_equal(got2.cpu().numpy(), want) and list(counts.cpu().numpy()) == counts_of(want)
    dd.check_guards("scrub2 data")
    dp.check_guards("scrub2 parity")
    out_d, out_p = dd.host(), dp.host()
    healed = want[:, 0] != MULTI
    check_scrubbed(layout, out_d, d1, d0, healed, want_marks[:, :k] == 1, "scrub2 data")
    check_scrubbed(layout, out_p, p1, p0, healed, want_marks[:, k:] == 1, "scrub2 parity")
    return got, out_d[..., :B], out_p[..., :B]


@pytest.mark.parametrize("k,m,lname", cases("locate2"), ids=case_ids("locate2"))
def test_locate2(oracle, k, m, lname):
    """Pairs split over the passes (data-data, data-parity, parity-parity), pairs in one byte, single
    shards and with m >= 5 a three-shard group: verdict slots, marks and the four counts equal
    expected_locate2; the scrub restores every located group."""
    same_as_fast(run_locate2, oracle, k, m, lname, run_locate2(oracle, k, m, lname))


# ------------------------------------------------------------------ repair / reconstruct

@functools.lru_cache(maxsize=None)
def repair_plan(oracle, k, m, g):
    rows, d0, p0 = batch(oracle, k, m, g)
    G, n = len(d0), k + m
    gm = random_marks(np.random.default_rng(100 * k + m), G, n, m + 1)
    gm[0] = 0
    gm[G - 1] = 0
    gm[G - 1, :m + 1] = 1  # one too many: left alone and counted
    gm[1] = 0
    gm[1, k:] = 1          # every parity row and nothing else
    gm[2] = 0
    gm[2, [0, n - 1][:m]] = 1
    dmg_d, dmg_p = damage(d0, p0, gm)
    exp_d, exp_p, nfail = expected_repair(oracle, types.SimpleNamespace(k=k, m=m, rows=rows), "cauchy", dmg_d, dmg_p, gm, g.B)
    ok = gm.sum(1) <= m
    assert nfail == int((~ok).sum()) >= 1
    assert np.array_equal(exp_d[ok][..., :g.B], d0[ok][..., :g.B]) and np.array_equal(exp_p[ok][..., :g.B], p0[ok][..., :g.B])
    return gm, dmg_d, dmg_p, exp_d, exp_p, nfail


@functools.lru_cache(maxsize=None)
def run_repair(oracle, k, m, lname):
    layout, code, rows, d0, p0 = start(oracle, k, m, lname)
    B = layout.B
    gm, dmg_d, dmg_p, exp_d, exp_p, nfail = repair_plan(oracle, k, m, geom(layout))
    healed = gm.sum(1) <= m
    marks = dev(marks_to_rs_layout(gm, k))
    dd, dp = place(layout, dmg_d, dmg_p)
    failed = ints(1)
    code.repair(dd.t, dp.t, marks, B, failed)
    torch.cuda.synchronize()
    dd.check_guards("repair data")
    dp.check_guards("repair parity")
    out_d, out_p = dd.host(), dp.host()
    assert np.array_equal(out_d[..., :B], exp_d[..., :B]) and np.array_equal(out_p[..., :B], exp_p[..., :B])
    check_scrubbed(layout, out_d, dmg_d, d0, healed, gm[:, :k] == 1, "repair data")
    check_scrubbed(layout, out_p, dmg_p, p0, healed, gm[:, k:] == 1, "repair parity")
    assert int(failed.item()) == nfail
    # reconstruct on the same marks: the data as repaired, the parity only read
    dd, dp = place(layout, dmg_d, dmg_p)
    failed = ints(1)
    code.reconstruct(dd.t, dp.t, marks, B, failed=failed)
    torch.cuda.synchronize()
    dd.check_guards("reconstruct data")
    held(dp, dmg_p, "reconstruct parity")
    rec_d = dd.host()
    assert np.array_equal(rec_d[..., :B], exp_d[..., :B])
    check_scrubbed(layout, rec_d, dmg_d, d0, healed, gm[:, :k] == 1, "reconstruct data")
    assert int(failed.item()) == nfail
    return out_d[..., :B], out_p[..., :B], rec_d[..., :B]


@pytest.mark.parametrize("k,m,lname", cases("repair"), ids=case_ids("repair"))
def test_repair(oracle, k, m, lname):
    """0 .. m + 1 erasures per group: [0, B) equals expected_repair and, where repairable, the
    original; bytes beyond the block and unmarked rows are bit-identical; the failed count matches.
    qfec_reconstruct on the same marks gives the same data and leaves the parity alone."""
    same_as_fast(run_repair, oracle, k, m, lname, run_repair(oracle, k, m, lname))


# ------------------------------------------------------------------ update / encode_update

@functools.lru_cache(maxsize=None)
def update_plan(oracle, k, m, g):
    rows, d0, p0 = batch(oracle, k, m, g)
    G = len(d0)
    ids = dc.update_ids(k, G)
    new = synth_bytes(1000 + k + g.B, G * g.pitch).reshape(G, g.pitch).copy()
    d1 = dc.apply_rows(d0, ids, new, g.B)
    assert not np.array_equal(d1, d0)
    return ids, new, d1, dc.oracle_parity(oracle, rows, d1, g.B)


def check_updated(layout, got, before, ids, what):
    """Bytes beyond the block of every row, and every byte of every untouched group, are as before."""
    wf = written_from(layout)
    assert np.array_equal(got[..., wf:], before[..., wf:]), f"{what}: bytes beyond the block written"
    assert np.array_equal(got[ids < 0], before[ids < 0]), f"{what}: an untouched group was written"


@functools.lru_cache(maxsize=None)
def run_update(oracle, k, m, lname):
    layout, code, rows, d0, p0 = start(oracle, k, m, lname)
    B, G = layout.B, len(d0)
    ids, new, d1, want_p = update_plan(oracle, k, m, geom(layout))
    shard = dev(ids)
    # the small write: data, rows and parity each on its own base
    dd, dp, dr = Guarded(d0, layout.data_off), Guarded(p0, layout.parity_off), Guarded(new, layout.rows_off)
    code.update(shard, dr.t, dp.t, data=dd.t, block_size=B)
    torch.cuda.synchronize()
    dd.check_guards("update data")
    dp.check_guards("update parity")
    held(dr, new, "update rows")
    got_d, got_p = dd.host(), dp.host()
    assert np.array_equal(got_d[..., :B], d1[..., :B]) and np.array_equal(got_p[..., :B], want_p)
    check_updated(layout, got_d, d0, ids, "update data")
    check_updated(layout, got_p, p0, ids, "update parity")
    keep = np.ones(d0.shape[:2], bool)
    keep[np.nonzero(ids >= 0)[0], ids[ids >= 0]] = False
    assert np.array_equal(got_d[keep], d0[keep]), "update: another data row was written"
    # delta only: rows = old ^ new, no data buffer (so no data base to misalign)
    delta_p = None
    if not layout.data_off:
        delta = new.copy()
        on = np.nonzero(ids >= 0)[0]
        delta[on] ^= d0[on, ids[on]]
        dp, dr = Guarded(p0, layout.parity_off), Guarded(delta, layout.rows_off)
        code.update(shard, dr.t, dp.t, data=None, block_size=B)
        torch.cuda.synchronize()
        dp.check_guards("delta parity")
        held(dr, delta, "delta rows")
        delta_p = dp.host()
        assert np.array_equal(delta_p[..., :B], want_p)
        check_updated(layout, delta_p, p0, ids, "delta parity")
        delta_p = delta_p[..., :B]
    # a three-piece partition of the columns: overwrite, then accumulate twice
    a, b = k // 2, k - 1
    assert 0 < a < b < k
    blank = np.full_like(p0, 0xA5)
    dp = Guarded(blank, layout.parity_off)
    for first, last, acc in ((0, a, False), (a, b, True), (b, k, True)):
        piece = np.ascontiguousarray(d0[:, first:last])
        part = Guarded(piece, layout.data_off or layout.rows_off)
        code.encode_update(part.t, dp.t, first, B, accumulate=acc)
        torch.cuda.synchronize()
        held(part, piece, "encode_update part")
    dp.check_guards("encode_update parity")
    part_p = dp.host()
    assert np.array_equal(part_p[..., :B], p0[..., :B])
    assert (part_p[..., written_from(layout):] == 0xA5).all(), "encode_update: bytes beyond the block written"
    return got_d[..., :B], got_p[..., :B], delta_p, part_p[..., :B]


@pytest.mark.parametrize("k,m,lname", cases("update"), ids=case_ids("update"))
def test_update(oracle, k, m, lname):
    """A small write, the same write as deltas alone, and a three-piece partition through
    encode_update: the parity is the oracle's encode of the new (or whole) data, untouched groups,
    other rows and bytes beyond the block keep their old bytes."""
    got = run_update(oracle, k, m, lname)
    if lname in dc.OFF_BASE:
        fast = run_update(oracle, k, m, "fast")
        for x, y in zip(got, fast):
            assert x is None or np.array_equal(x, y), "differs from the fast layout"


# ------------------------------------------------------------------ encode instances no encode test names

@pytest.mark.parametrize("k,m", dc.ENCODE_EXTRA, ids=[f"encode-{k}-{m}-fast" for k, m in dc.ENCODE_EXTRA])
def test_encode_instance(oracle, k, m):
    layout, code, rows, d0, p0 = start(oracle, k, m, "fast")
    B = layout.B
    dd, dp = Guarded(d0, 0), Guarded(np.full_like(p0, 0xA5), 0)
    code.encode(dd.t, dp.t, B)
    torch.cuda.synchronize()
    held(dd, d0, "encode data")
    dp.check_guards("encode parity")
    got = dp.host()
    assert np.array_equal(got[..., :B], p0[..., :B])
    assert (got[..., written_from(layout):] == 0xA5).all()
