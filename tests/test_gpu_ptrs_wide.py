"""GPU tests of the plan calls on pointer tables: qfec_plan_apply_ptrs, qfec_reconstruct_ptrs_wide,
qfec_repair_ptrs_wide (kernel k_plan_apply_ptrs).  The rows of a batch live in one guard-filled pool
(ptrs_common.Pool) in a random permutation of slots at chosen alignments; after every call the WHOLE
pool is compared with the pool before the call in which only the rows the call must write carry the
oracle's bytes (ptrs_wide_common.Case).  Shapes sit where the kernel can go wrong: k + m on either
side of 64, 128 and 192 (one to four registers of table entries per lane), more rows than one pass
accumulates, row lengths of a tail only, one column, one wave, a wave and a column.

Run on an MI355X:  python -m pytest tests/test_gpu_ptrs_wide.py -m gpu -q
"""
import numpy as np
import pytest

import quicknet_amd as qa
import ptrs_common as pc
from ptrs_wide_common import Case, put_rows
from quicknet_amd.synth import marks_to_rs_layout
from repair_common import expected_repair
from wide_common import RECONSTRUCT, REPAIR, random_masks, singular_code, singular_marks, stale_code, stale_marks

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
ALIGN = ["aligned", "residues", "one-data", "one-parity"]
MODES = [False, True]
MODE_IDS = ["reconstruct", "repair"]
ONE_REG = [(4, 2), (10, 3), (32, 8)]            # k + m <= 64: one register of table entries
MORE_REGS = [(60, 5), (120, 9), (200, 55)]      # shard 64 opens the second register; a third; lane 62 of the fourth
ALL_B = [1, 16, 17, 1000, 1024, 1040, 1400]     # tail only; one column, lanes idle; +1; tail of 8; one wave; +1 column; 1400


def ids(shapes):
    return [f"{k}-{m}" for k, m in shapes]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def counter():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def one_shot(code, repair):
    return code.repair_ptrs_wide if repair else code.reconstruct_ptrs_wide


def contiguous(code, repair):
    return code.repair_wide if repair else code.reconstruct_wide


def check(oracle, code, c, repair, rows=None, twice=True, alias=None, what=""):
    """Cases 1 and 2 on one batch: the one-shot against the oracle over the whole pool, the failed
    counter (which accumulates), a null counter, and the contiguous call on the same rows."""
    G, k, m, B = c.G, c.k, c.m, c.B
    what = f"({k},{m}) B={B} {'repair' if repair else 'reconstruct'} {what}"
    flat, d, p, nfail = c.expected(oracle, code, repair, rows)
    assert not np.array_equal(flat, c.pool.host), f"{what}: nothing to write"
    t, ptrs = pc.to_device(torch, DEV, c.pool, alias)
    marks, failed = dev(c.marks), counter()
    one_shot(code, repair)(ptrs, marks, B, failed)
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    assert np.array_equal(c.pool.rows_of(got, 0, G * k), d.reshape(G * k, B)), f"{what}: data differs from the oracle"
    if m:
        assert np.array_equal(c.pool.rows_of(got, G * k, G * m), p.reshape(G * m, B)), f"{what}: parity differs"
    assert np.array_equal(got, flat), f"{what}: a byte outside the rows to write was written"
    assert int(failed.item()) == nfail, what
    if twice:  # the survivors are unchanged, so are the results; the counter adds up
        one_shot(code, repair)(ptrs, marks, B, failed)
        torch.cuda.synchronize()
        assert int(failed.item()) == 2 * nfail, what
        assert np.array_equal(t.cpu().numpy(), flat), what
    t2, ptrs2 = pc.to_device(torch, DEV, c.pool, alias)
    one_shot(code, repair)(ptrs2, marks, B)  # d_failed may be NULL
    torch.cuda.synchronize()
    assert np.array_equal(t2.cpu().numpy(), flat), f"{what}: null counter"
    dd, pp, f2 = pc.padded(torch, DEV, c.data, B), pc.padded(torch, DEV, c.par, B), counter()
    contiguous(code, repair)(dd, pp, marks, B, f2)
    torch.cuda.synchronize()
    assert np.array_equal(dd.cpu().numpy()[..., :B], d) and np.array_equal(pp.cpu().numpy()[..., :B], p), f"{what}: contiguous"
    assert int(f2.item()) == nfail
    return got


def covered_marks(k, m):
    gm = pc.recon_marks(k, m)
    pc.assert_marks_cover(gm, k, m)  # before the GPU is called: the test cannot pass by omission
    return gm


# ---------------------------------------------------------------- 1, 2. one-shots against the oracle and the contiguous calls

@pytest.mark.parametrize("mode", ALIGN)
@pytest.mark.parametrize("k,m", ONE_REG, ids=ids(ONE_REG))
def test_one_shots_one_register(oracle, k, m, mode):
    code = qa.Code.cauchy(k, m)
    gm = covered_marks(k, m)
    for B in ALL_B:
        for repair in MODES:
            check(oracle, code, Case(0x1A00 + 16 * k + B, gm, k, m, B, mode), repair, what=mode)


@pytest.mark.parametrize("mode", ALIGN)
@pytest.mark.parametrize("k,m", MORE_REGS, ids=ids(MORE_REGS))
def test_one_shots_more_registers(oracle, k, m, mode):
    code = qa.Code.cauchy(k, m)
    gm = covered_marks(k, m)
    for B in (17, 1040):
        for repair in MODES:
            check(oracle, code, Case(0x2B00 + k + B, gm, k, m, B, mode), repair, what=mode)


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m", [(254, 1), (1, 254)], ids=["254-1", "1-254"])
def test_one_shots_edge_shapes(oracle, k, m, mode):
    code = qa.Code.cauchy(k, m)
    gm = random_masks(k, k + m, m, 8)
    for B in (17, 1040):
        for repair in MODES:
            check(oracle, code, Case(0x3C00 + k + B, gm, k, m, B, mode), repair, what=mode)


@pytest.mark.parametrize("mode", ["aligned", "one-data"])
@pytest.mark.parametrize("repair", MODES, ids=MODE_IDS)
def test_rows_past_one_pass(oracle, repair, mode):
    """(20,12) with t = 9 and t = 12 rows to write, data and parity mixed: the second pass of eight
    rows re-reads the survivors."""
    k, m, B = 20, 12, 1040
    code = qa.Code.cauchy(k, m)
    more = np.zeros((4, k + m), np.uint8)
    more[0, [0, 3, 4, 7, 9, 11, 13, 19, k + 2]] = 1                        # t = 9: e = 8 and a parity row
    more[1, [0, 3, 4, 7, 9, 11, 13, k, k + 2, k + 5, k + 9, k + 11]] = 1  # t = 12 = m: e = 7
    assert more[0].sum() == 9 and more[1].sum() == 12 and more[1, :k].sum() == 7
    # nine and twelve erased data rows: the reconstruct rule writes more than one pass too
    more[2, :9] = 1
    more[3, 4:16] = 1
    # recon_marks spaces its erased rows 2 apart and needs k >= 2 m: random masks stand in (the first
    # three are empty, one mark, m + 1 marks)
    gm = np.concatenate([random_masks(2012, k + m, m, 12), more])
    check(oracle, code, Case(0x4D00, gm, k, m, B, mode), repair, what=mode)


# ---------------------------------------------------------------- 3. narrow codes against qfec_reconstruct_ptrs

@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m", [(4, 2), (10, 3), (8, 4)], ids=["4-2", "10-3", "8-4"])
def test_narrow_codes_equal_reconstruct_ptrs(k, m, mode):
    code = qa.Code.cauchy(k, m)
    gm = covered_marks(k, m)
    for B in (17, 1000):
        c = Case(0x5E00 + k + B, gm, k, m, B, mode)
        marks = dev(c.marks)
        out = []
        for call in (code.reconstruct_ptrs, code.reconstruct_ptrs_wide):
            t, ptrs = pc.to_device(torch, DEV, c.pool)
            f = counter()
            call(ptrs, marks, B, f)
            torch.cuda.synchronize()
            out.append((t.cpu().numpy(), int(f.item())))
        assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] > 0
        assert not np.array_equal(out[1][0], c.pool.host)


# ---------------------------------------------------------------- 4, 5. the plan: device = host; one plan, two tables

def test_device_plan_equals_host_plan_and_serves_two_tables(oracle):
    k, m, B = 60, 5, 1000
    code = qa.Code.cauchy(k, m)
    gm = covered_marks(k, m)
    marks, failed = dev(marks_to_rs_layout(gm, k)), counter()
    plan = code.plan_build(marks, REPAIR, failed=failed)
    torch.cuda.synchronize()
    assert np.array_equal(plan.cpu().numpy(), np.stack([code.plan_host(mk, REPAIR) for mk in gm]))
    marks.fill_(1)  # the apply reads no marks
    for seed, mode in ((0x6F00, "aligned"), (0x6F10, "residues")):
        c = Case(seed, gm, k, m, B, mode)
        flat, _, _, nfail = c.expected(oracle, code, True)
        t, ptrs = pc.to_device(torch, DEV, c.pool)
        code.plan_apply_ptrs(ptrs, plan, B)
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), flat), mode
    assert int(failed.item()) == nfail  # the build counted; the applies counted nothing
    # a RECONSTRUCT plan on the same table writes the data rows only
    plan = code.plan_build(dev(marks_to_rs_layout(gm, k)), RECONSTRUCT)
    flat, _, _, _ = c.expected(oracle, code, False)
    t, ptrs = pc.to_device(torch, DEV, c.pool)
    code.plan_apply_ptrs(ptrs, plan, B)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), flat)


# ---------------------------------------------------------------- 6, 7. quirk and singular codes

@pytest.mark.parametrize("mode", ["aligned", "residues"])
def test_stale_row_starts_from_the_old_bytes(oracle, mode):
    """The (30,4) code with rows[0][0] = 0: data shard 5 lost, its decode row's column-0 coefficient is
    zero, so with the quirk the row starts from its old bytes, exactly as oracle.rs_reconstruct leaves
    it; without the quirk it is the true product."""
    k, m, B, G = 30, 4, 1000, 4
    gm = np.zeros((G, k + m), np.uint8)
    gm[1] = gm[3] = stale_marks()
    gm[2, [2, 9, k + 1]] = 1
    c = Case(0x7A00, gm, k, m, B, mode)
    code, rows = stale_code(1)
    got = check(oracle, code, c, False, rows=rows, twice=False, what=mode)  # a second call starts from other bytes
    stale = c.pool.rows_of(got, 0, G * k).reshape(G, k, B)
    code0, _ = stale_code(0)
    t, ptrs = pc.to_device(torch, DEV, c.pool)
    code0.reconstruct_ptrs_wide(ptrs, dev(c.marks), B)
    torch.cuda.synchronize()
    true = c.pool.rows_of(t.cpu().numpy(), 0, G * k).reshape(G, k, B)
    assert np.array_equal(stale[1, 5] ^ true[1, 5], np.full(B, 0x5A, np.uint8))  # the old bytes, XORed in
    assert np.array_equal(stale[2], true[2])
    # the repair rule treats the data row the same way
    t, ptrs = pc.to_device(torch, DEV, c.pool)
    code.repair_ptrs_wide(ptrs, dev(c.marks), B)
    torch.cuda.synchronize()
    assert np.array_equal(c.pool.rows_of(t.cpu().numpy(), 0, G * k).reshape(G, k, B), stale)


@pytest.mark.parametrize("repair", MODES, ids=MODE_IDS)
def test_singular_group_is_untouched_and_counted(oracle, repair):
    k, m, B, G = 26, 2, 1000, 3
    code, rows = singular_code()
    gm = np.zeros((G, k + m), np.uint8)
    gm[0] = gm[2] = singular_marks()
    gm[1, 4] = 1  # one lost shard decodes
    c = Case(0x8B00, gm, k, m, B, "one-data")
    want = c.data[1:2].copy()
    assert oracle.rs_reconstruct(rows, want, c.par[1:2].copy(), np.ascontiguousarray(gm[1]), B) == 0
    flat = c.pool.host.copy()
    put_rows(c.pool, flat, k, want[0])
    assert not np.array_equal(flat, c.pool.host)
    t, ptrs = pc.to_device(torch, DEV, c.pool)
    failed = counter()
    one_shot(code, repair)(ptrs, dev(c.marks), B, failed)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), flat)
    assert int(failed.item()) == 2


# ---------------------------------------------------------------- 8, 9. shards a plan does not touch; aliased inputs

@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("repair", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("k,m", [(32, 8), (60, 5)], ids=["32-8", "60-5"])
def test_untouched_shards_are_never_dereferenced(oracle, k, m, repair, mode):
    """Every table entry of a shard the group's plan neither reads nor writes points at one extra
    guard-filled row: the result is that of the true table and the extra row keeps its guard bytes."""
    B = 1000
    code = qa.Code.cauchy(k, m)
    gm = covered_marks(k, m)
    c = Case(0x9C00 + k, gm, k, m, B, mode, extra=1)
    wire = c.G * c.n
    idle = c.untouched(repair)
    assert len(idle) >= c.G and len(set(idle.tolist())) == len(idle) and idle.max() < wire
    flat, _, _, _ = c.expected(oracle, code, repair)
    outs = []
    for alias in (None, {int(i): wire for i in idle}):
        t, ptrs = pc.to_device(torch, DEV, c.pool, alias)
        one_shot(code, repair)(ptrs[:wire], dev(c.marks), B)  # the extra row is no shard of the batch
        torch.cuda.synchronize()
        outs.append(t.cpu().numpy())
    assert np.array_equal(outs[0], flat) and np.array_equal(outs[1], outs[0])
    assert (c.pool.rows_of(outs[1], wire, 1) == pc.GUARD).all()


@pytest.mark.parametrize("mode", ["aligned", "residues"])
def test_aliased_read_only_shards(oracle, mode):
    """One padding row's address repeated among the survivors of two other groups."""
    k, m, B = 32, 8, 1000
    code = qa.Code.cauchy(k, m)
    gm = covered_marks(k, m)
    src = 3  # row (0, 3): group 0 is untouched
    i = 1 * k + int(np.nonzero(gm[1, :k] == 0)[0][2])
    j = 2 * k + int(np.nonzero(gm[2, :k] == 0)[0][5])

    def tweak(data, par):
        flat = data.reshape(-1, B)
        flat[i] = flat[j] = flat[src]

    for repair in MODES:
        check(oracle, code, Case(0xAD00, gm, k, m, B, mode, tweak=tweak), repair, alias={i: src, j: src}, what=mode)


# ---------------------------------------------------------------- 10. two chunks of plans

def test_two_chunks_of_plans(oracle):
    """(200,55), rows of 16 bytes, three groups more than 64 MiB of plans hold: the one-shot runs two
    chunks, and the second one's table, marks and plans start at g0 * k / groups * k + g0 * m / 0."""
    k, m, B = 200, 55, 16
    n = k + m
    code = qa.Code.cauchy(k, m)
    G = (64 << 20) // code.plan_stride() + 3
    gm = np.zeros((G, n), np.uint8)
    gm[np.arange(G), np.arange(G) % k] = 1
    gm[-3:, k + 1] = gm[-2:, k + 54] = gm[-1, 7] = 1
    c = Case(0xBE00, gm, k, m, B, "aligned")
    t, ptrs = pc.to_device(torch, DEV, c.pool)
    marks, failed = dev(c.marks), counter()
    code.repair_ptrs_wide(ptrs, marks, B, failed)
    dd, pp = dev(c.data), dev(c.par)
    code.repair_wide(dd, pp, marks, B)
    torch.cuda.synchronize()
    assert int(failed.item()) == 0
    flat = c.pool.host.copy()
    put_rows(c.pool, flat, 0, dd.cpu().numpy().reshape(G * k, B))
    put_rows(c.pool, flat, G * k, pp.cpu().numpy().reshape(G * m, B))
    got = t.cpu().numpy()
    assert np.array_equal(got, flat)
    assert not np.array_equal(got, c.pool.host)
    for lo, hi in ((0, 8), (G - 8, G)):
        d, p, nfail = expected_repair(oracle, code, "cauchy", c.data[lo:hi], c.par[lo:hi], gm[lo:hi], B)
        assert nfail == 0
        assert np.array_equal(c.pool.rows_of(got, lo * k, (hi - lo) * k), d.reshape(-1, B))
        assert np.array_equal(c.pool.rows_of(got, G * k + lo * m, (hi - lo) * m), p.reshape(-1, B))


# ---------------------------------------------------------------- 11. stream and refusal

def test_on_a_side_stream(oracle):
    """On a non-default stream, followed by a dependent copy on that stream and a wait for that stream
    alone: no device-wide synchronisation is needed."""
    k, m, B = 120, 9, 1040
    code = qa.Code.cauchy(k, m)
    c = Case(0xCF00, covered_marks(k, m), k, m, B, "one-parity")
    flat, _, _, nfail = c.expected(oracle, code, True)
    t, ptrs = pc.to_device(torch, DEV, c.pool)
    marks, failed = dev(c.marks), counter()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        code.repair_ptrs_wide(ptrs, marks, B, failed)
        after = t.clone()
    stream.synchronize()
    assert np.array_equal(after.cpu().numpy(), flat) and int(failed.item()) == nfail


def test_misaligned_plan_is_refused():
    """A slice of a tensor that does not start on a 16-byte boundary is no plan base: refused, and
    nothing is launched."""
    k, m, B, G = 32, 8, 64, 4
    code = qa.Code.cauchy(k, m)
    stride = code.plan_stride()
    flat = torch.zeros(G * stride + 16, dtype=torch.uint8, device=DEV)
    assert flat.data_ptr() % 16 == 0
    c = Case(0xD000, np.zeros((G, k + m), np.uint8), k, m, B, "aligned")
    t, ptrs = pc.to_device(torch, DEV, c.pool)
    for off in (1, 4, 8):
        with pytest.raises(qa.QfecError, match="d_plan not 16-byte aligned"):
            code.plan_apply_ptrs(ptrs, flat[off:off + G * stride], B)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), c.pool.host)
