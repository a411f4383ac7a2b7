"""GPU tests of device-built decode plans: qfec_plan_build / qfec_plan_apply and the one-shot calls
qfec_reconstruct_wide / qfec_repair_wide, at any k + m.  The plan buffer is held byte for byte to
the host query qfec_plan_build_host; the one-shots to the oracle (repair_common.expected_repair,
oracle.rs_reconstruct) on wide codes and to the LUT calls qfec_reconstruct / qfec_repair on narrow
ones.  Every comparison is exact.

Run on an MI355X:  python -m pytest tests/test_gpu_wide.py -m gpu -q
"""
import numpy as np
import pytest

import quicknet_amd as qa
from quicknet_amd.synth import marks_to_rs_layout, synth_bytes
from repair_common import damage, expected_repair, masks_up_to, padded, random_marks, round16, to_dev
from wide_common import (FAILED, RECONSTRUCT, REPAIR, WORK, random_masks, singular_code, singular_marks, stale_code,
                         stale_marks, status_of)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")


def counter():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def all_masks(n):
    return ((np.arange(1 << n)[:, None] >> np.arange(n)) & 1).astype(np.uint8)


def batch(seed, G, k, m, B):
    """Random data and random, inconsistent parity: [G, k, B], [G, m, B]."""
    return (synth_bytes(seed, G * k * B).reshape(G, k, B), synth_bytes(seed + 1, G * m * B).reshape(G, m, B))


def expected_reconstruct(oracle, code, flavour, dmg_d, dmg_p, gm, B):
    """What a reconstruct must leave in [0, B) of the data: the oracle's reconstruct.  Returns
    (data, failed groups as a bool vector): e greater than the surviving parity."""
    k, m = code.k, code.m
    rec = oracle.rs_reconstruct if flavour == "cauchy" else oracle.fec_reconstruct
    exp = np.ascontiguousarray(dmg_d).copy()
    rec(code.rows, exp, np.ascontiguousarray(dmg_p).copy(), marks_to_rs_layout(gm, k), B)
    e, np_ = gm[:, :k].sum(1), gm[:, k:].sum(1)
    bad = e > m - np_
    assert np.array_equal(exp[bad], dmg_d[bad])
    return exp, bad


def run_wide(oracle, code, flavour, data, par, gm, B, pitch, repair, pad_fill=0xC3, expect=None):
    """Damage (marked rows of both buffers 0x5A), run one one-shot call and hold the result to the
    expectation: [0, B) equals it, every byte from round16(B) on is unchanged, unmarked rows and
    failed groups are bit-identical, the parity is unchanged by reconstruct_wide, failed as expected."""
    k, m = code.k, code.m
    dmg_d, dmg_p = damage(data, par, gm)
    if expect is not None:
        exp_d, exp_p, bad = expect(dmg_d, dmg_p)
    elif repair:
        exp_d, exp_p, nfail = expected_repair(oracle, code, flavour, dmg_d, dmg_p, gm, B)
        bad = gm.sum(1) > m
        assert nfail == int(bad.sum())
    else:
        exp_d, bad = expected_reconstruct(oracle, code, flavour, dmg_d, dmg_p, gm, B)
        exp_p = dmg_p
    in_d, in_p = padded(dmg_d, pitch, pad_fill), padded(dmg_p, pitch, pad_fill)
    dd, dp = to_dev(in_d), to_dev(in_p)
    failed = counter()
    (code.repair_wide if repair else code.reconstruct_wide)(dd, dp, to_dev(marks_to_rs_layout(gm, k)), B, failed)
    torch.cuda.synchronize()
    out_d, out_p = dd.cpu().numpy(), dp.cpu().numpy()
    assert np.array_equal(out_d[..., :B], exp_d)
    assert np.array_equal(out_p[..., :B], exp_p)
    span = min(round16(B), pitch)
    assert np.array_equal(out_d[..., span:], in_d[..., span:])
    assert np.array_equal(out_p[..., span:], in_p[..., span:])
    assert np.array_equal(out_d[gm[:, :k] == 0], in_d[gm[:, :k] == 0])
    assert np.array_equal(out_p[gm[:, k:] == 0], in_p[gm[:, k:] == 0])
    assert np.array_equal(out_d[bad], in_d[bad]) and np.array_equal(out_p[bad], in_p[bad])
    if not repair:
        assert np.array_equal(out_p, in_p)
    assert int(failed.item()) == int(bad.sum())
    return out_d, out_p


# ---------------------------------------------------------------- 1. device plan == host plan

def plan_masks(k, m, G):
    gm = random_masks(k * 1000 + m, k + m, m, G)
    if G < 16:  # the few groups of the large shapes: e = m exactly, and a mix of t = m marks over both
        rng = np.random.default_rng(k + m)
        gm[3] = 0
        gm[3, rng.choice(k, size=min(k, m), replace=False)] = 1
        gm[4] = 0
        gm[4, rng.choice(k + m, size=m, replace=False)] = 1
    return gm


@pytest.mark.parametrize("k,m,G", [
    (32, 8, 64),
    (60, 8, 64),      # marks straddle the 64-lane pass: k < 64 < k + m
    (70, 10, 64),     # k > 64
    (200, 55, 6),     # e reaches 55
    (128, 127, 6),    # e reaches 127
])
@pytest.mark.parametrize("mode", [RECONSTRUCT, REPAIR])
def test_device_plan_equals_host_plan(k, m, G, mode):
    code = qa.Code.cauchy(k, m)
    gm = plan_masks(k, m, G)
    want = np.stack([code.plan_host(mk, mode) for mk in gm])
    nfail = int((status_of(want) == FAILED).sum())
    assert nfail > 0 and (status_of(want) == WORK).any()
    if G < 16:
        assert want[3, 2] == min(k, m)  # e = m
    marks = to_dev(marks_to_rs_layout(gm, k))
    failed = counter()
    plan = torch.full((G, code.plan_stride()), 0xEE, dtype=torch.uint8, device=DEV)
    code.plan_build(marks, mode, plan, failed)
    torch.cuda.synchronize()
    got = plan.cpu().numpy()
    assert np.array_equal(got, want), np.nonzero((got != want).any(1))[0]
    assert int(failed.item()) == nfail
    again = code.plan_build(marks, mode, failed=failed)
    torch.cuda.synchronize()
    assert torch.equal(again, plan) and int(failed.item()) == 2 * nfail


# ---------------------------------------------------------------- 2. one-shots against the oracle

@pytest.mark.parametrize("k,m,B,G,flavour", [
    (32, 8, 256, 64, "cauchy"),
    (60, 8, 100, 48, "cauchy"),
    (20, 12, 1100, 33, "cauchy"),      # t up to 12: two passes of rows; 69 columns: a second wave with 5 live lanes
    (64, 16, 1024, 40, "cauchy"),
    (32, 8, 256, 64, "vandermonde"),
])
@pytest.mark.parametrize("repair", [False, True], ids=["reconstruct", "repair"])
def test_one_shots_vs_oracle(oracle, k, m, B, G, flavour, repair):
    code = getattr(qa.Code, flavour)(k, m)
    data, par = batch(k * 7 + B, G, k, m, B)
    rng = np.random.default_rng(k * 100 + B)
    gm = random_marks(rng, G, k + m, m + 1)
    gm[1:4] = 0
    gm[1, k + rng.choice(m, size=2, replace=False)] = 1             # parity only
    gm[2, rng.choice(k + m, size=m + 1, replace=False)] = 1         # more than the code takes
    gm[3, [int(rng.integers(0, k)), k + int(rng.integers(0, m))]] = 1  # one data, one parity
    if (k, m) == (20, 12):
        gm[0] = 0
        gm[0, [0, 3, 4, 7, 9, 11, 13, 20, 22, 25, 30, 31]] = 1  # t = 12, e = 7
    t, e = gm.sum(1), gm[:, :k].sum(1)
    assert (t > m).any() and ((e > 0) & (t > e) & (t <= m)).any() and ((t > 0) & (e == 0)).any() and (t == 0).any()
    run_wide(oracle, code, flavour, data, par, gm, B, round16(B) + 16, repair)


# ---------------------------------------------------------------- 3. edge shapes

@pytest.mark.parametrize("k,m", [(254, 1), (1, 254), (128, 127), (200, 55)])
@pytest.mark.parametrize("repair", [False, True], ids=["reconstruct", "repair"])
def test_edge_shapes(oracle, k, m, repair):
    G, B = 4, 48
    code = qa.Code.cauchy(k, m)
    data, par = batch(k + 3 * m, G, k, m, B)
    rng = np.random.default_rng(k)
    gm = np.zeros((G, k + m), np.uint8)
    gm[1, rng.choice(k + m, size=m + 1, replace=False)] = 1     # failed
    gm[1, 0] = 1
    gm[2, rng.choice(k, size=min(k, m), replace=False)] = 1      # the most erased data the code takes
    gm[3, rng.choice(k + m, size=m, replace=False)] = 1          # t = m over data and parity
    gm[3, 0] = 1
    if gm[3].sum() > m:
        gm[3, np.nonzero(gm[3, 1:])[0][0] + 1] = 0
    assert gm[1].sum() > m and gm[2].sum() == min(k, m) and gm[3].sum() == m
    run_wide(oracle, code, "cauchy", data, par, gm, B, round16(B) + 16, repair)


# ---------------------------------------------------------------- 4. narrow codes against the LUT calls

@pytest.mark.parametrize("k,m,B,masks", [
    # The LUT kernels run 8- or 12-byte lanes on some shapes and then write round_up(B, 8) or
    # round_up(B, 12) bytes of a row; every B here has those equal to round_up(B, 16), so both calls
    # write the same scratch bytes whichever lanes the LUT call picks
    (10, 3, 40, lambda: masks_up_to(13, 4)),
    (4, 2, 92, lambda: all_masks(6)),
    (20, 4, 93, lambda: random_marks(np.random.default_rng(204), 96, 24, 5)),
], ids=["10-3", "4-2", "20-4"])
def test_narrow_codes_equal_the_lut_calls(k, m, B, masks):
    """Whole output buffers, scratch bytes included, and the failed counts."""
    code = qa.Code.cauchy(k, m)
    gm = masks()
    G = gm.shape[0]
    pitch = round16(B) + 16
    data, par = batch(k * 13 + B, G, k, m, B)
    dmg_d, dmg_p = damage(data, par, gm)
    in_d = padded(dmg_d, pitch, 0)
    in_p = padded(dmg_p, pitch, 0)
    in_d[..., B:] = synth_bytes(5, G * k * (pitch - B)).reshape(G, k, pitch - B)
    in_p[..., B:] = synth_bytes(6, G * m * (pitch - B)).reshape(G, m, pitch - B)
    marks = to_dev(marks_to_rs_layout(gm, k))
    for lut, wide in ((code.reconstruct, code.reconstruct_wide), (code.repair, code.repair_wide)):
        d1, p1, f1 = to_dev(in_d), to_dev(in_p), counter()
        d2, p2, f2 = to_dev(in_d), to_dev(in_p), counter()
        lut(d1, p1, marks, B, f1)
        wide(d2, p2, marks, B, f2)
        torch.cuda.synchronize()
        assert torch.equal(d1, d2) and torch.equal(p1, p2)
        assert int(f1.item()) == int(f2.item()) > 0


# ---------------------------------------------------------------- 5. byte path

@pytest.mark.parametrize("repair", [False, True], ids=["reconstruct", "repair"])
def test_byte_path_odd_pitch(oracle, repair):
    """pitch = B = 37: no 16-B alignment; nothing past B exists."""
    k, m, B, G = 32, 8, 37, 48
    code = qa.Code.cauchy(k, m)
    data, par = batch(371, G, k, m, B)
    run_wide(oracle, code, "cauchy", data, par, random_marks(np.random.default_rng(37), G, k + m, m + 1), B, B, repair)


def test_byte_path_unaligned_base(oracle):
    """A 16-byte-aligned pitch with d_data one byte off a 16-byte boundary: the byte path, which
    writes [0, B) of the marked rows and not one byte more."""
    k, m, B, G = 32, 8, 40, 33
    pitch = 64
    code = qa.Code.cauchy(k, m)
    data, par = batch(401, G, k, m, B)
    gm = random_marks(np.random.default_rng(41), G, k + m, m + 1)
    dmg_d, dmg_p = damage(data, par, gm)
    exp_d, exp_p, nfail = expected_repair(oracle, code, "cauchy", dmg_d, dmg_p, gm, B)
    in_d, in_p = padded(dmg_d, pitch, 0xC3), padded(dmg_p, pitch, 0xC3)
    flat = torch.full((G * k * pitch + 16,), 0x77, dtype=torch.uint8, device=DEV)
    assert flat.data_ptr() % 16 == 0
    dd = flat[1:1 + G * k * pitch].view(G, k, pitch)
    dd.copy_(to_dev(in_d))
    dp = to_dev(in_p)
    failed = counter()
    code.repair_wide(dd, dp, to_dev(marks_to_rs_layout(gm, k)), B, failed)
    torch.cuda.synchronize()
    out_d, out_p = dd.cpu().numpy(), dp.cpu().numpy()
    exp_full_d, exp_full_p = in_d.copy(), in_p.copy()
    exp_full_d[..., :B] = exp_d
    exp_full_p[..., :B] = exp_p
    assert np.array_equal(out_d, exp_full_d) and np.array_equal(out_p, exp_full_p)
    edge = flat.cpu().numpy()
    assert edge[0] == 0x77 and (edge[1 + G * k * pitch:] == 0x77).all()
    assert int(failed.item()) == nfail


# ---------------------------------------------------------------- 6. quirk and singular codes

def test_stale_row_starts_from_the_old_bytes(oracle):
    """The (30,4) code with rows[0][0] = 0 and the quirk: data shard 5 lost, its decode row's column-0
    coefficient is zero, so rs.c leaves the row's old bytes in the sum.  Against oracle.rs_reconstruct
    with inconsistent parity; without the quirk the same row comes out as the true product."""
    k, m, B, G = 30, 4, 80, 4
    gm = np.zeros((G, k + m), np.uint8)
    gm[1] = gm[3] = stale_marks()
    gm[2, [2, 9, k + 1]] = 1
    data, par = batch(3004, G, k, m, B)
    outs = []
    for quirk in (1, 0):
        code, rows = stale_code(quirk)
        dmg_d, dmg_p = damage(data, par, gm)
        if quirk:
            want = dmg_d.copy()
            oracle.rs_reconstruct(rows, want, dmg_p.copy(), marks_to_rs_layout(gm, k), B)
            expect = lambda d, p: (want, p, np.zeros(G, bool))  # noqa: E731
            out_d, _ = run_wide(oracle, code, "cauchy", data, par, gm, B, round16(B) + 16, False, expect=expect)
        else:
            dd, dp = to_dev(dmg_d), to_dev(dmg_p)
            code.reconstruct_wide(dd, dp, to_dev(marks_to_rs_layout(gm, k)), B)
            torch.cuda.synchronize()
            out_d = dd.cpu().numpy()
        outs.append(out_d[..., :B])
    stale, true = outs
    assert np.array_equal(stale[1, 5] ^ true[1, 5], np.full(B, 0x5A, np.uint8))  # the old bytes, XORed in
    assert np.array_equal(stale[2], true[2])
    # the repair rule treats the data row the same way
    code, rows = stale_code(1)
    dmg_d, dmg_p = damage(data, par, gm)
    dd, dp = to_dev(dmg_d), to_dev(dmg_p)
    code.repair_wide(dd, dp, to_dev(marks_to_rs_layout(gm, k)), B)
    torch.cuda.synchronize()
    assert np.array_equal(dd.cpu().numpy()[:, :k], stale)


@pytest.mark.parametrize("repair", [False, True], ids=["reconstruct", "repair"])
def test_singular_group_is_untouched_and_counted(repair):
    k, m, B, G = 26, 2, 64, 3
    code, rows = singular_code()
    gm = np.zeros((G, k + m), np.uint8)
    gm[0] = gm[2] = singular_marks()
    gm[1, 4] = 1  # one lost shard decodes
    data, par = batch(2602, G, k, m, B)
    dmg_d, dmg_p = damage(data, par, gm)
    dd, dp, failed = to_dev(dmg_d), to_dev(dmg_p), counter()
    (code.repair_wide if repair else code.reconstruct_wide)(dd, dp, to_dev(marks_to_rs_layout(gm, k)), B, failed)
    torch.cuda.synchronize()
    out_d = dd.cpu().numpy()
    assert np.array_equal(out_d[[0, 2]], dmg_d[[0, 2]]) and np.array_equal(dp.cpu().numpy(), dmg_p)
    assert not np.array_equal(out_d[1, 4], dmg_d[1, 4]) and np.array_equal(np.delete(out_d[1], 4, 0), np.delete(dmg_d[1], 4, 0))
    assert int(failed.item()) == 2


# ---------------------------------------------------------------- 7. plan_apply reads the plan alone

def test_one_plan_two_batches_and_no_marks(oracle):
    k, m, B, G = 32, 8, 128, 40
    pitch = round16(B) + 16
    code = qa.Code.cauchy(k, m)
    gm = random_marks(np.random.default_rng(77), G, k + m, m + 1)
    marks = to_dev(marks_to_rs_layout(gm, k))
    failed = counter()
    plan = code.plan_build(marks, REPAIR, failed=failed)
    marks.fill_(1)  # apply reads no marks: overwriting them after the build changes nothing
    nfail = int((gm.sum(1) > m).sum())
    for seed in (7001, 7003):
        data, par = batch(seed, G, k, m, B)
        dmg_d, dmg_p = damage(data, par, gm)
        exp_d, exp_p, _ = expected_repair(oracle, code, "cauchy", dmg_d, dmg_p, gm, B)
        dd, dp = to_dev(padded(dmg_d, pitch, 0xC3)), to_dev(padded(dmg_p, pitch, 0xC3))
        code.plan_apply(dd, dp, plan, B)
        torch.cuda.synchronize()
        assert np.array_equal(dd.cpu().numpy()[..., :B], exp_d)
        assert np.array_equal(dp.cpu().numpy()[..., :B], exp_p)
    assert int(failed.item()) == nfail  # the build counted; the two applies counted nothing


def test_misaligned_plan_is_refused():
    """A plan buffer must start on a 16-byte boundary; a slice that does not is refused by build and
    by apply, and nothing is launched."""
    k, m, B, G = 32, 8, 64, 4
    code = qa.Code.cauchy(k, m)
    stride = code.plan_stride()
    flat = torch.zeros(G * stride + 16, dtype=torch.uint8, device=DEV)
    assert flat.data_ptr() % 16 == 0
    marks = torch.zeros(G * (k + m), dtype=torch.uint8, device=DEV)
    data = torch.zeros((G, k, B), dtype=torch.uint8, device=DEV)
    par = torch.zeros((G, m, B), dtype=torch.uint8, device=DEV)
    for off in (1, 4, 8):
        bad = flat[off:off + G * stride]
        with pytest.raises(qa.QfecError, match="d_plan not 16-byte aligned"):
            code.plan_build(marks, REPAIR, plan=bad)
        with pytest.raises(qa.QfecError, match="d_plan not 16-byte aligned"):
            code.plan_apply(data, par, bad, B)
    code.plan_apply(data, par, code.plan_build(marks, REPAIR, plan=flat[16:]), B)
    torch.cuda.synchronize()
