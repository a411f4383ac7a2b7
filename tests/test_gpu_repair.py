"""GPU tests of qfec_repair: one launch rewrites every marked shard, data and parity, of every
repairable group.  The expectation is the oracle's reconstruct followed by its encode, with only
the marked parity rows of groups with t <= m taken over (repair_common.expected_repair).  Bit-exact.

Run on an MI355X:  python -m pytest tests/test_gpu_repair.py -m gpu -q
"""
import numpy as np
import pytest

import quicknet_amd as qa
from quicknet_amd.synth import marks_to_rs_layout, synth_bytes
from repair_common import damage, expected_repair, masks_up_to, padded, random_marks, round16, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")


def run_repair(oracle, code, flavour, data, par, gm, B, pitch, pad_fill=0xC3):
    """Damage, repair on the device, and hold the result to the expectation: [0, B) equals it,
    every byte from round16(B) on is unchanged, unmarked rows are bit-identical, failed counts t > m."""
    k, m = code.k, code.m
    dmg_d, dmg_p = damage(data, par, gm)
    exp_d, exp_p, nfail = expected_repair(oracle, code, flavour, dmg_d, dmg_p, gm, B)
    in_d, in_p = padded(dmg_d, pitch, pad_fill), padded(dmg_p, pitch, pad_fill)
    dd, dp = to_dev(in_d), to_dev(in_p)
    failed = torch.zeros(1, dtype=torch.int32, device=DEV)
    code.repair(dd, dp, to_dev(marks_to_rs_layout(gm, k)), B, failed)
    torch.cuda.synchronize()
    out_d, out_p = dd.cpu().numpy(), dp.cpu().numpy()
    assert np.array_equal(out_d[..., :B], exp_d)
    assert np.array_equal(out_p[..., :B], exp_p)
    span = min(round16(B), pitch)
    assert np.array_equal(out_d[..., span:], in_d[..., span:])
    assert np.array_equal(out_p[..., span:], in_p[..., span:])
    assert np.array_equal(out_d[gm[:, :k] == 0], in_d[gm[:, :k] == 0])
    assert np.array_equal(out_p[gm[:, k:] == 0], in_p[gm[:, k:] == 0])
    untouched = gm.sum(1) > m
    assert np.array_equal(out_d[untouched], in_d[untouched]) and np.array_equal(out_p[untouched], in_p[untouched])
    assert int(failed.item()) == nfail == int(untouched.sum())
    return out_d, out_p


@pytest.mark.parametrize("k,m,B,flavour", [
    (10, 3, 1024, "cauchy"),       # templated instance
    (16, 4, 1400, "cauchy"),       # templated, B not a multiple of 64
    (4, 2, 100, "cauchy"),         # templated, B not a multiple of 16: the tail column
    (20, 4, 1400, "cauchy"),       # n = 24, the LUT's edge
    (9, 5, 100, "cauchy"),         # generic fallback, five rows
    (5, 2, 1024, "vandermonde"),   # generic fallback
    (10, 3, 1024, "vandermonde"),  # templated instance
])
def test_repair_random_vs_oracle(oracle, k, m, B, flavour):
    """Random patterns of 0..m+1 erasures over the n positions (parity-only, mixed and failed
    groups), random inconsistent parity, erased rows of both buffers filled with 0x5A, one spare
    16-B column per row that nothing may write."""
    G = 700
    code = getattr(qa.Code, flavour)(k, m)
    rng = np.random.default_rng(k * 100 + B)
    data = synth_bytes(k * 7 + B, G * k * B).reshape(G, k, B)
    par = synth_bytes(k * 11 + B, G * m * B).reshape(G, m, B)
    gm = random_marks(rng, G, k + m, m + 1)
    t = gm.sum(1)
    e = gm[:, :k].sum(1)
    assert ((t > 0) & (e == 0)).any() and ((e > 0) & (t > e) & (t <= m)).any() and (t > m).any()
    run_repair(oracle, code, flavour, data, par, gm, B, round16(B) + 16)


@pytest.mark.parametrize("k,m,bits", [(4, 2, 6), (10, 3, 4)])
def test_repair_every_mask(oracle, k, m, bits):
    """One group per mask: all 64 masks of (4,2), all 1 093 masks with <= 4 bits of (10,3)."""
    B = 48
    gm = masks_up_to(k + m, bits)
    G = gm.shape[0]
    assert G == (64 if k == 4 else 1093)
    code = qa.Code.cauchy(k, m)
    data = synth_bytes(k + 1, G * k * B).reshape(G, k, B)
    par = synth_bytes(k + 2, G * m * B).reshape(G, m, B)
    run_repair(oracle, code, "cauchy", data, par, gm, B, round16(B) + 16)


def test_repair_byte_path(oracle):
    """pitch = B = 37: no 16-B alignment, the byte-granular kernel; nothing past B exists."""
    k, m, B, G = 4, 2, 37, 700
    code = qa.Code.cauchy(k, m)
    rng = np.random.default_rng(37)
    data = synth_bytes(371, G * k * B).reshape(G, k, B)
    par = synth_bytes(372, G * m * B).reshape(G, m, B)
    run_repair(oracle, code, "cauchy", data, par, random_marks(rng, G, k + m, m + 1), B, B)


def test_repair_equals_reconstruct_then_encode():
    """code.repair on one copy, code.reconstruct + code.encode on another, every group
    recoverable: identical data, identical parity on the marked rows."""
    k, m, B, G = 10, 3, 1024, 700
    code = qa.Code.cauchy(k, m)
    rng = np.random.default_rng(1003)
    data = synth_bytes(5, G * k * B).reshape(G, k, B)
    d0, p0 = to_dev(data), torch.empty((G, m, B), dtype=torch.uint8, device=DEV)
    code.encode(d0, p0)
    torch.cuda.synchronize()
    gm = random_marks(rng, G, k + m, m)
    dmg_d, dmg_p = damage(data, p0.cpu().numpy(), gm)
    marks = to_dev(marks_to_rs_layout(gm, k))
    d1, p1 = to_dev(dmg_d), to_dev(dmg_p)
    code.repair(d1, p1, marks)
    d2, p2 = to_dev(dmg_d), to_dev(dmg_p)
    code.reconstruct(d2, p2, marks)
    full = torch.empty_like(p2)
    code.encode(d2, full)
    torch.cuda.synchronize()
    assert torch.equal(d1, d2) and torch.equal(d1, d0)
    sel = to_dev(gm[:, k:] == 1)
    assert torch.equal(p1[sel], full[sel])
    assert torch.equal(p1, p0)  # consistent parity in, so the whole group is back as it was


def test_repair_refuses_wide_codes():
    code = qa.Code.cauchy(32, 8)
    G, B = 4, 64
    d = torch.zeros((G, 32, B), dtype=torch.uint8, device=DEV)
    p = torch.zeros((G, 8, B), dtype=torch.uint8, device=DEV)
    marks = torch.zeros(G * 40, dtype=torch.uint8, device=DEV)
    rc = qa.lib().qfec_repair(code._h, d.data_ptr(), p.data_ptr(), marks.data_ptr(), G, B, B, None, None)
    assert rc == -5  # QFEC_EUNSUP
    assert "k + m = 40" in qa.lib().qfec_last_error().decode()
    with pytest.raises(qa.QfecError):
        code.repair(d, p, marks)
    with pytest.raises(qa.QfecError):
        code.prepare_repair()


def test_repair_zero_groups_is_a_noop():
    code = qa.Code.cauchy(4, 2)
    code.prepare_repair()
    d = torch.zeros((0, 4, 64), dtype=torch.uint8, device=DEV)
    p = torch.zeros((0, 2, 64), dtype=torch.uint8, device=DEV)
    failed = torch.zeros(1, dtype=torch.int32, device=DEV)
    code.repair(d, p, torch.zeros(0, dtype=torch.uint8, device=DEV), 64, failed)
    assert qa.lib().qfec_repair(code._h, None, None, None, 0, 64, 64, None, None) == 0
    torch.cuda.synchronize()
    assert int(failed.item()) == 0
