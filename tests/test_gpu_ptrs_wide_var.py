"""GPU tests of the plan calls on pointer tables with per-shard lengths: qfec_plan_apply_ptrs_var,
qfec_reconstruct_ptrs_wide_var, qfec_repair_ptrs_wide_var (kernel k_plan_apply_ptrs_var).  The rows of a
batch live in a guard-filled pool and are written to their own lengths only (ptrs_wide_var_common.Batch);
after every call the WHOLE pool is compared with the pool before the call in which only bytes [0, L) of
the rows to write carry the oracle's bytes, so a byte read past a shard's length that reaches a result,
a byte written at or past L, or anything written elsewhere (the guard row that the shards of length 0
point at included) fails.  Every test asserts its own coverage on the CPU before the GPU is called.

Run on an MI355X:  python -m pytest tests/test_gpu_ptrs_wide_var.py -m gpu -q
"""
import numpy as np
import pytest

import quicknet_amd as qa
import ptrs_common as pc
import ptrs_var_common as pv
from ptrs_wide_common import Case, put_rows
from ptrs_wide_var_common import Batch, crossed, cycled, fill_rows
from quicknet_amd.synth import marks_to_rs_layout
from wide_common import RECONSTRUCT, REPAIR, singular_code, singular_marks, stale_code, stale_marks

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from test_gpu_ptrs_var import all_patterns, encode_batch, recon_batch, recon_groups  # noqa: E402

DEV = torch.device("cuda:0")
ALIGN = ["aligned", "residues", "one-data", "one-parity"]
MODES = [False, True]
MODE_IDS = ["reconstruct", "repair"]
ONE_REG = [(4, 2, 1), (4, 2, 17), (4, 2, 1000), (4, 2, 1400), (10, 3, 1), (10, 3, 17), (10, 3, 1000), (10, 3, 1400),
           (32, 8, 17), (32, 8, 1040)]
MORE_REGS = [(k, m, B) for k, m in ((60, 5), (120, 9), (200, 55)) for B in (17, 1040)]


def ids(shapes):
    return ["-".join(map(str, s)) for s in shapes]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32).reshape(-1)).to(DEV)


def counter():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def one_shot(code, repair):
    return code.repair_ptrs_wide_var if repair else code.reconstruct_ptrs_wide_var


def run(fn, t, stream=None):
    """fn() on the current stream, or on `stream` followed by a dependent copy there and a wait for
    that stream alone; returns the pool after it."""
    if stream is None:
        fn()
        torch.cuda.synchronize()
        return t.cpu().numpy()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn()
        after = t.clone()
    stream.synchronize()
    return after.cpu().numpy()


def check(code, b, what="", twice=True, stream=None, need_fail=True):
    """The one-shot of b's mode against the expected pool, both counters over two calls, null counters."""
    what = f"({b.k},{b.m}) max_len={b.max_len} {'repair' if b.repair else 'reconstruct'} {what}"
    assert not np.array_equal(b.expect, b.initial), f"{what}: nothing to write"
    assert b.nfail > 0 or not need_fail, what
    t, table = b.vp.to_device(torch, DEV)
    dl, gl, dm = i32(b.dl), i32(b.L), dev(b.marks)
    failed, inv = counter(), counter()
    got = run(lambda: one_shot(code, b.repair)(table, dl, gl, dm, b.max_len, failed, inv), t, stream)
    G, k, m = b.G, b.k, b.m
    for g in range(G):
        for s in range(k + m):
            r = g * k + s if s < k else G * k + g * m + (s - k)
            assert np.array_equal(b.row(got, r), b.row(b.expect, r)), f"{what}: shard ({g},{s}) {b.describe(g)}"
    assert np.array_equal(got, b.expect), f"{what}: a byte outside [0, L) of the rows to write was written"
    assert (int(failed.item()), int(inv.item())) == (b.nfail, b.ninv), what
    if twice:  # the survivors are unchanged, so are the results; the counters add up
        one_shot(code, b.repair)(table, dl, gl, dm, b.max_len, failed, inv)
        torch.cuda.synchronize()
        assert (int(failed.item()), int(inv.item())) == (2 * b.nfail, 2 * b.ninv), what
        assert np.array_equal(t.cpu().numpy(), b.expect), what
    t2, table2 = b.vp.to_device(torch, DEV)
    one_shot(code, b.repair)(table2, dl, gl, dm, b.max_len)  # both counters may be NULL
    torch.cuda.synchronize()
    assert np.array_equal(t2.cpu().numpy(), b.expect), f"{what}: null counters"
    return got


def invalid_groups(k, m, max_len):
    """Groups the apply must refuse for their lengths, a group that is failed AND badly sized (failed
    only), and status-0 groups with a bad length (invalid)."""
    short = dict(pv.length_patterns(k, max_len))["short"]
    Ls = int(short.max())
    n = k + m
    one = pc.recon_marks(k, m)[1]
    assert one[:k].sum() == 1 and one[k:].sum() == 0
    free = int(np.flatnonzero(one[:k] == 0)[0])
    none = np.zeros(n, np.uint8)
    ponly = none.copy()
    ponly[k] = 1
    over = none.copy()
    over[:m + 1] = 1

    def with_len(bad):
        lens = short.copy()
        lens[free] = bad
        return lens

    out = [("L=-1", short.copy(), -1, one), ("L=max_len+1", short.copy(), max_len + 1, one),
           ("L=INT_MIN", short.copy(), pv.INT_MIN, one), ("L=INT_MAX", short.copy(), pv.INT_MAX, one)]
    for bad in (Ls + 1, -1, pv.INT_MIN, pv.INT_MAX):
        out.append((f"len={bad}", with_len(bad), Ls, one))
    out.append(("no marks, len=L+1", with_len(Ls + 1), Ls, none))
    out.append(("no marks, L=-1", short.copy(), -1, none))
    out.append(("parity marks only, len=-1", with_len(-1), Ls, ponly))
    out.append(("t > m and L=-1", short.copy(), -1, over))
    out.append(("t > m and len=L+1", with_len(Ls + 1), Ls, over))
    return out


# ---------------------------------------------------------------- 1. one register, full cross

@pytest.mark.parametrize("mode", ALIGN)
@pytest.mark.parametrize("k,m,max_len", ONE_REG, ids=ids(ONE_REG))
def test_one_register_full_cross(oracle, k, m, max_len, mode):
    code = qa.Code.cauchy(k, m)
    groups = crossed(k, m, max_len) + invalid_groups(k, m, max_len)
    for repair in MODES:
        b = Batch(oracle, code, groups, max_len, mode, 0x1A00 + 16 * k + max_len, repair)
        assert b.ninv > 0
        check(code, b, mode)


# ---------------------------------------------------------------- 2. more registers

@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m,max_len", MORE_REGS, ids=ids(MORE_REGS))
def test_more_registers(oracle, k, m, max_len, mode):
    code = qa.Code.cauchy(k, m)
    groups = cycled(k, m, max_len) + invalid_groups(k, m, max_len)
    assert len(groups) == 2 * (m + 3) + len(invalid_groups(k, m, max_len))
    for repair in MODES:
        check(code, Batch(oracle, code, groups, max_len, mode, 0x2B00 + k + max_len, repair), mode)


# ---------------------------------------------------------------- 3. invalid and failed

@pytest.mark.parametrize("repair", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("k,m,max_len", [(10, 3, 1000), (120, 9, 17)], ids=["10-3-1000", "120-9-17"])
def test_invalid_and_failed_groups(oracle, k, m, max_len, repair):
    code = qa.Code.cauchy(k, m)
    bad = invalid_groups(k, m, max_len)
    groups = crossed(k, m, max_len)[:2 * (m + 3)] + bad
    b = Batch(oracle, code, groups, max_len, "aligned", 0x3C00 + k, repair)
    tail = slice(len(groups) - len(bad), None)
    # by the rule: the two groups with t > m are failed and not invalid, every other one of `bad` is invalid
    assert b.failed[tail].sum() == 2 and b.invalid[tail].sum() == len(bad) - 2 and not b.work[tail].any()
    assert not (b.failed & b.invalid).any() and b.nfail > 2 and b.ninv == len(bad) - 2
    check(code, b)


# ---------------------------------------------------------------- 4. rows past one pass

@pytest.mark.parametrize("repair", MODES, ids=MODE_IDS)
def test_rows_past_one_pass(oracle, repair):
    """(20,12) with t = 9 and t = 12 rows to write: the second pass of eight rows re-reads the clipped
    survivors."""
    k, m, max_len = 20, 12, 1040
    code = qa.Code.cauchy(k, m)
    more = np.zeros((4, k + m), np.uint8)
    more[0, [0, 3, 4, 7, 9, 11, 13, 19, k + 2]] = 1
    more[1, [0, 3, 4, 7, 9, 11, 13, k, k + 2, k + 5, k + 9, k + 11]] = 1
    more[2, :9] = 1
    more[3, 4:16] = 1
    assert more[0].sum() == 9 and more[1].sum() == 12 and more[2, :k].sum() == 9 and more[3, :k].sum() == 12
    pats = dict(pv.length_patterns(k, max_len))
    groups = [(n, pats[n].copy(), max_len, q) for n in ("ladder", "one-long") for q in more]
    for mode in ("aligned", "one-data"):
        b = Batch(oracle, code, groups, max_len, mode, 0x4D00, repair)
        assert b.work.all()
        check(code, b, mode, need_fail=False)


# ---------------------------------------------------------------- 5. narrow codes against qfec_reconstruct_ptrs_var

@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m", [(4, 2), (10, 3), (8, 4)], ids=["4-2", "10-3", "8-4"])
def test_narrow_codes_equal_reconstruct_ptrs_var(oracle, k, m, mode):
    """The groups of test_gpu_ptrs_var.recon_groups through both calls: the whole pool and `invalid` are
    equal.  Its four invalid groups are decodable, so the order of the two judgements (lengths before
    marks there, marks before lengths here) moves no group between the counters.  `failed` differs by
    exactly the under-determined groups of length L = 0: qfec_reconstruct_ptrs_var leaves an empty
    group before it looks at the marks and counts it nowhere, while here the build counts from the
    marks alone, whatever L is (include/qfec.h).  recon_groups crosses the "empty" length pattern with
    every under-determined mark pattern, so that difference is not zero; it is computed on the CPU and
    held exactly."""
    code = qa.Code.cauchy(k, m)
    for max_len in (17, 1000):
        groups = recon_groups(k, m, max_len)
        vp, dl, L, marks, expect, nfail, ninv = recon_batch(oracle, code.rows, k, m, max_len, mode, 0x5E00 + k + max_len, groups)
        assert nfail > 0 and ninv == 4 and not np.array_equal(expect, vp.pool.host)
        empty_failed = sum(1 for g in groups if not g[4] and g[2] == 0 and g[3][:k].any() and g[3].sum() > m)
        assert empty_failed > 0
        out = []
        for call in (code.reconstruct_ptrs_var, code.reconstruct_ptrs_wide_var):
            t, table = vp.to_device(torch, DEV)
            f, inv = counter(), counter()
            call(table, i32(dl), i32(L), dev(marks), max_len, f, inv)
            torch.cuda.synchronize()
            out.append((t.cpu().numpy(), int(f.item()), int(inv.item())))
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[1][0], expect)
        assert out[0][1:] == (nfail, ninv) and out[1][1:] == (nfail + empty_failed, ninv)


# ---------------------------------------------------------------- 6. all lengths = max_len against the fixed-length calls

@pytest.mark.parametrize("repair", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("k,m,max_len", [(32, 8, 1040), (120, 9, 17)], ids=["32-8-1040", "120-9-17"])
def test_full_lengths_equal_the_fixed_calls(oracle, k, m, max_len, repair):
    code = qa.Code.cauchy(k, m)
    gm = pc.recon_marks(k, m)
    pc.assert_marks_cover(gm, k, m)
    groups = [("full", np.full(k, max_len, np.int64), max_len, q) for q in gm]
    for mode in ("aligned", "residues"):
        b = Batch(oracle, code, groups, max_len, mode, 0x6F00 + k, repair)
        assert b.ninv == 0 and b.nfail > 0 and not np.array_equal(b.expect, b.initial)
        t1, table1 = b.vp.to_device(torch, DEV)
        t2, table2 = b.vp.to_device(torch, DEV)
        f1, f2, inv = counter(), counter(), counter()
        one_shot(code, repair)(table1, i32(b.dl), i32(b.L), dev(b.marks), max_len, f1, inv)
        (code.repair_ptrs_wide if repair else code.reconstruct_ptrs_wide)(table2, dev(b.marks), max_len, f2)
        torch.cuda.synchronize()
        assert np.array_equal(t1.cpu().numpy(), t2.cpu().numpy()) and np.array_equal(t1.cpu().numpy(), b.expect)
        assert int(f1.item()) == int(f2.item()) == b.nfail and int(inv.item()) == 0


# ---------------------------------------------------------------- 7. the plan

def test_one_plan_serves_two_tables_with_different_lengths(oracle):
    k, m, max_len = 60, 5, 1000
    code = qa.Code.cauchy(k, m)
    base = cycled(k, m, max_len)
    turned = [(n2, l2, L2, q) for (_, _, _, q), (n2, l2, L2, _) in zip(base, base[3:] + base[:3])]  # other lengths, same marks
    bad = invalid_groups(k, m, max_len)
    marks, failed = dev(marks_to_rs_layout(np.stack([g[3] for g in base + bad]), k)), counter()
    plan = code.plan_build(marks, REPAIR, failed=failed)
    marks.fill_(1)  # the apply reads no marks
    for seed, mode, groups in ((0x7A00, "aligned", base + bad), (0x7A10, "residues", turned + bad)):
        b = Batch(oracle, code, groups, max_len, mode, seed, True)
        assert b.ninv > 0 and b.nfail > 0 and not np.array_equal(b.expect, b.initial)
        t, table = b.vp.to_device(torch, DEV)
        inv = counter()
        code.plan_apply_ptrs_var(table, i32(b.dl), i32(b.L), plan, max_len, inv)
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), b.expect), mode
        assert int(inv.item()) == b.ninv and int(failed.item()) == b.nfail  # the apply counts invalid groups, nothing else
    # a RECONSTRUCT plan on the same table writes the data rows only: the parity is as before
    plan = code.plan_build(dev(b.marks), RECONSTRUCT)
    b = Batch(oracle, code, turned + bad, max_len, "residues", 0x7A10, False)
    t, table = b.vp.to_device(torch, DEV)
    code.plan_apply_ptrs_var(table, i32(b.dl), i32(b.L), plan, max_len)
    got = run(lambda: None, t)
    assert np.array_equal(got, b.expect) and not np.array_equal(b.expect, b.initial)
    for r in range(b.G * k, b.G * (k + m)):
        assert np.array_equal(b.row(got, r), b.row(b.initial, r))


# ---------------------------------------------------------------- 8. quirk and singular code

@pytest.mark.parametrize("mode", ["aligned", "residues"])
def test_stale_row_starts_from_the_old_bytes_below_L_only(oracle, mode):
    """The (30,4) code with rows[0][0] = 0, data shard 5 lost, the survivors short: with the quirk the
    row starts from its old bytes in [0, L), exactly as oracle.rs_reconstruct leaves it."""
    k, m, max_len = 30, 4, 1000
    other = np.zeros(k + m, np.uint8)
    other[[2, 9, k + 1]] = 1
    pats = dict(pv.length_patterns(k, max_len))
    groups = [("ladder", pats["ladder"].copy(), 700, stale_marks()), ("short", pats["short"].copy(), 777, other),
              ("steps", pats["steps"].copy(), 999, stale_marks()), ("full", pats["full"].copy(), 1000, np.zeros(k + m, np.uint8))]
    groups[0][1][:] = np.minimum(groups[0][1], 700)
    code, rows = stale_code(1)
    b = Batch(oracle, code, groups, max_len, mode, 0x8B00, False, rows=rows)
    got = check(code, b, mode, twice=False, need_fail=False)  # a second call starts from other bytes
    code0, rows0 = stale_code(0)
    b0 = Batch(oracle, code0, groups, max_len, mode, 0x8B00, False, rows=rows0)
    assert np.array_equal(b0.initial, b.initial)
    t, table = b0.vp.to_device(torch, DEV)
    code0.reconstruct_ptrs_wide_var(table, i32(b0.dl), i32(b0.L), dev(b0.marks), max_len)
    true = run(lambda: None, t)
    for g, L in ((0, 700), (2, 999)):
        assert np.array_equal(b.row(got, g * k + 5, L) ^ b.row(true, g * k + 5, L), np.full(L, 0x5A, np.uint8))
        assert np.array_equal(b.row(got, g * k + 5)[L:], b.row(b.initial, g * k + 5)[L:])
    for i in range(k):
        assert np.array_equal(b.row(got, 1 * k + i), b.row(true, 1 * k + i))


@pytest.mark.parametrize("repair", MODES, ids=MODE_IDS)
def test_singular_group_is_untouched_and_counted_failed(oracle, repair):
    k, m, max_len = 26, 2, 1000
    code, rows = singular_code()
    one = np.zeros(k + m, np.uint8)
    one[4] = 1
    pats = dict(pv.length_patterns(k, max_len))
    groups = [("ladder", pats["ladder"].copy(), max_len, singular_marks()), ("stairs", pats["stairs"].copy(), max_len, one),
              ("short", pats["short"].copy(), 600, singular_marks())]
    b = Batch(oracle, code, groups, max_len, "one-data", 0x9C00, False, rows=rows, singular=(0, 2))
    assert b.nfail == 2 and b.ninv == 0 and b.work.tolist() == [False, True, False]
    b.repair = repair  # one lost data shard: the repair writes the same row
    check(code, b, twice=False)


# ---------------------------------------------------------------- 9. tripwire

@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("repair", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("k,m,max_len", [(32, 8, 1000), (120, 9, 17)], ids=["32-8-1000", "120-9-17"])
def test_untouched_shards_and_empty_survivors_are_never_dereferenced(oracle, k, m, max_len, repair, mode):
    """Every entry of a shard the plan neither reads nor writes, and of every survivor of length 0,
    points at the misaligned guard row: the result is that of the true table, the guard row keeps its
    bytes, and an aligned group still counts as aligned."""
    code = qa.Code.cauchy(k, m)
    groups = cycled(k, m, max_len)
    b = Batch(oracle, code, groups, max_len, mode, 0xAD00 + k, repair, tripwire=True)
    plain = Batch(oracle, code, groups, max_len, mode, 0xAD00 + k, repair)
    assert len(b.idle) >= b.G and len(b.vp.alias) > len(plain.vp.alias) > 0
    assert np.array_equal(b.expect, plain.expect)
    got = check(code, b, mode, twice=False)
    assert (b.row(got, b.vp.guard_row) == pc.GUARD).all()


# ---------------------------------------------------------------- 10. two chunks of plans

def test_two_chunks_of_plans(oracle):
    """(200,55), max_len 16, three groups more than 64 MiB of plans hold: the one-shot runs two chunks,
    and the second one's lengths start at d_lens + g0 * k and d_group_len + g0."""
    k, m, max_len = 200, 55, 16
    n = k + m
    code = qa.Code.cauchy(k, m)
    G = (64 << 20) // code.plan_stride() + 3
    gm = np.zeros((G, n), np.uint8)
    gm[np.arange(G), np.arange(G) % k] = 1
    gm[-3:, k + 1] = gm[-2:, k + 54] = gm[-1, 7] = 1
    lens = np.tile(np.where(np.arange(k) % 2 == 0, 16, 9), (G, 1)).astype(np.int64)
    dmark = gm[:, :k] == 1
    data = pc.batch_bytes(0xBE00, G, k, max_len)
    par = pc.batch_bytes(0xBE01, G, m, max_len)
    data[dmark] = 0x5A
    par[gm[:, k:] == 1] = 0x5A
    plens = np.where(dmark, max_len, lens)
    vp = pv.VarPool(G, k, m, max_len, "aligned", 0xBE02)
    fill_rows(vp, 0, data.reshape(G * k, max_len), plens)
    fill_rows(vp, G * k, par.reshape(G * m, max_len), np.full(G * m, max_len))
    initial = vp.clone_host()
    t, table = vp.to_device(torch, DEV)
    marks, failed, inv = dev(marks_to_rs_layout(gm, k)), counter(), counter()
    code.repair_ptrs_wide_var(table, i32(np.where(dmark, pv.INT_MIN, lens)), i32(np.full(G, max_len)), marks, max_len, failed, inv)
    # the yardstick for the middle: the fixed-length call on the same rows zero-padded
    padded = data.copy()
    padded[np.arange(max_len)[None, None, :] >= plens[:, :, None]] = 0
    c = Case(0xBE00, gm, k, m, max_len, "aligned")
    put_rows(c.pool, c.pool.host, 0, padded.reshape(G * k, max_len))
    put_rows(c.pool, c.pool.host, G * k, par.reshape(G * m, max_len))
    t2, ptrs2 = pc.to_device(torch, DEV, c.pool)
    code.repair_ptrs_wide(ptrs2, marks, max_len)
    torch.cuda.synchronize()
    assert int(failed.item()) == 0 and int(inv.item()) == 0
    fixed = t2.cpu().numpy()
    expect = initial.copy()
    marked = np.concatenate([np.flatnonzero(dmark.reshape(-1)), G * k + np.flatnonzero((gm[:, k:] == 1).reshape(-1))])
    expect[vp.pool.start[marked, None] + np.arange(max_len)] = fixed[c.pool.start[marked, None] + np.arange(max_len)]
    got = t.cpu().numpy()
    assert not np.array_equal(got, initial)
    assert np.array_equal(got, expect)
    # the CPU model at both ends of the batch
    for lo, hi in ((0, 8), (G - 8, G)):
        groups = [("16/9", lens[g], max_len, gm[g]) for g in range(lo, hi)]
        b = Batch(oracle, code, groups, max_len, "aligned", 0xBE10 + lo, True)
        b.data[:], b.par[:] = data[lo:hi], par[lo:hi]  # this batch's bytes, not the Batch's own
        assert b.work.all()
        for i, nbytes, row in b._oracle_rows(oracle, code, None):
            g, s = (i // k, i % k) if i < b.G * k else ((i - b.G * k) // m, k + (i - b.G * k) % m)
            r = (lo + g) * k + s if s < k else G * k + (lo + g) * m + (s - k)
            assert np.array_equal(got[vp.pool.start[r]:vp.pool.start[r] + nbytes], row), (lo + g, s)


# ---------------------------------------------------------------- 11. round trip

@pytest.mark.parametrize("mode", ["aligned", "residues"])
def test_round_trip(oracle, mode):
    """encode_ptrs_var, drop up to m shards per group, data and parity, repair_ptrs_wide_var fed the
    encode's own d_group_len: every data shard is back in [0, len) and zero in [len, L), every parity
    shard equals the encode's in [0, L)."""
    k, m, max_len = 32, 8, 1040
    code = qa.Code.cauchy(k, m)
    pats = all_patterns(k, max_len)
    G, n = len(pats), k + m
    gm = np.zeros((G, n), np.uint8)
    for g in range(G):
        gm[g, [(g + 5 * j) % n for j in range(g % (m + 1))]] = 1
    assert {int(x) for x in gm.sum(1)} == set(range(m + 1)) and gm[:, :k].any() and gm[:, k:].any()
    dmark = gm[:, :k] == 1
    keep = set(np.flatnonzero(dmark.reshape(-1)).tolist())  # a shard that will be rewritten has a slot of its own
    vp, lens, data, after_encode, glen = encode_batch(oracle, code.rows, k, m, max_len, mode, 0xCF00, pats, keep=keep)
    t, table = vp.to_device(torch, DEV)
    gl = torch.full((G,), -77, dtype=torch.int32, device=DEV)
    code.encode_ptrs_var(table, i32(lens), max_len, gl)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), after_encode) and np.array_equal(gl.cpu().numpy(), glen)
    lost, expect = after_encode.copy(), after_encode.copy()
    padded = pv.zero_padded(data, lens)
    for g in range(G):
        L = int(glen[g])
        for s in np.flatnonzero(gm[g]):
            at = vp.pool.start[g * k + s if s < k else G * k + g * m + (s - k)]
            if L > 0:
                lost[at:at + L] = 0x5A
                if s < k:
                    expect[at:at + L] = padded[g, s, :L]
    assert not np.array_equal(lost, expect)
    t.copy_(dev(lost))
    failed, inv = counter(), counter()
    code.repair_ptrs_wide_var(table, i32(np.where(dmark, pv.INT_MIN, lens)), gl, dev(marks_to_rs_layout(gm, k)), max_len,
                              failed, inv)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), expect)
    # the encode's -1 makes a void group invalid here as well, whatever its marks (none has more than m)
    assert int(failed.item()) == 0 and int(inv.item()) == int((glen < 0).sum()) > 0


# ---------------------------------------------------------------- 12. a side stream

def test_on_a_side_stream(oracle):
    k, m, max_len = 120, 9, 1040
    code = qa.Code.cauchy(k, m)
    b = Batch(oracle, code, cycled(k, m, max_len) + invalid_groups(k, m, max_len), max_len, "one-parity", 0xD000, True)
    check(code, b, twice=False, stream=torch.cuda.Stream())
