"""GPU tests of qfec_verify: bit j of bad_rows[g] is set iff parity row j of group g differs from
rows[j] x data[g] in some byte of [0, block_size); bytes past block_size never count; the counter
gains one per inconsistent group and accumulates.

Run on an MI355X:  python -m pytest tests/test_gpu_verify.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import quicknet_amd as qa
from quicknet_amd.synth import marks_to_rs_layout, synth_bytes
from repair_common import damage, padded, random_marks, round16, to_dev
from repair_common import encoded as encoded_flavour

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")

# (k, m, B, pitch, G): two templated instances, the generic kernel, the byte kernel (pitch 37),
# and G = 301 so that groups * columns is no multiple of the 256-lane block
CASES = [(10, 3, 1024, 1040, 300), (16, 4, 1400, 1424, 300), (9, 5, 100, 128, 300), (4, 2, 37, 37, 300),
         (10, 3, 1024, 1040, 301)]


encoded = functools.partial(encoded_flavour, "cauchy")  # (k, m, B, pitch, G) -> code, data, parity


def verify(code, data, par, B, count=None):
    count = torch.zeros(1, dtype=torch.int32, device=DEV) if count is None else count
    bad = code.verify(data, par, B, bad_groups=count)
    torch.cuda.synchronize()
    return bad.cpu().numpy(), int(count.item())


@pytest.mark.parametrize("k,m,B,pitch,G", CASES)
def test_verify_consistent_and_padding_ignored(k, m, B, pitch, G):
    """After an encode every word is 0 and the count is 0, whatever lies in [B, pitch) of the data
    and the parity (the parity's garbage there differs from any product of the data's)."""
    code, data, par = encoded(k, m, B, pitch, G)
    bad, n = verify(code, data, par, B)
    assert bad.shape == (G,) and not bad.any() and n == 0
    # bad_rows handed in full of ones comes back zeroed; the counter alone also works
    pre = torch.full((G,), -1, dtype=torch.int32, device=DEV)
    assert code.verify(data, par, B, bad_rows=pre) is pre
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    check = qa.lib().qfec_verify(code._h, data.data_ptr(), par.data_ptr(), G, B, pitch, None, count.data_ptr(), None)
    torch.cuda.synchronize()
    assert check == 0 and not pre.cpu().numpy().any() and int(count.item()) == 0


@pytest.mark.parametrize("k,m,B,pitch,G", CASES)
def test_verify_finds_exactly_the_flipped_rows(k, m, B, pitch, G):
    """Byte 0 of one parity row, byte B-1 of another and a middle byte of a third, in different
    groups: exactly those bits, count 3.  One data byte in a fourth group: all m bits (Cauchy
    coefficients are non-zero), count 4.  A second call on the same counter accumulates."""
    code, data, par = encoded(k, m, B, pitch, G)
    flips = [(5, 0, 0), (G // 2, m - 1, B - 1), (G - 1, 1 % m, B // 2)]
    for g, j, b in flips:
        par[g, j, b] ^= 0x40
    expect = np.zeros(G, np.int32)
    for g, j, _ in flips:
        expect[g] = 1 << j
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    bad, n = verify(code, data, par, B, count)
    assert np.array_equal(bad, expect) and n == 3
    data[77, k - 1, B - 1] ^= 0x01
    expect[77] = (1 << m) - 1
    bad, n = verify(code, data, par, B, count)
    assert np.array_equal(bad, expect)
    assert n == 3 + 4  # the counter is not reset between calls


def test_verify_after_repair():
    """A damaged batch with every group recoverable and parity from the encode: after code.repair
    the whole batch verifies, and before it the damaged groups do not."""
    k, m, B, G = 10, 3, 1000, 300
    pitch = round16(B)
    code = qa.Code.cauchy(k, m)
    data = synth_bytes(99, G * k * B).reshape(G, k, B)
    d0 = to_dev(padded(data, pitch))
    p0 = torch.zeros((G, m, pitch), dtype=torch.uint8, device=DEV)
    code.encode(d0, p0, B)
    torch.cuda.synchronize()
    gm = random_marks(np.random.default_rng(7), G, k + m, m)
    dmg_d, dmg_p = damage(d0.cpu().numpy(), p0.cpu().numpy(), gm)
    dd, dp = to_dev(dmg_d), to_dev(dmg_p)
    bad, n = verify(code, dd, dp, B)
    assert n == int((gm.sum(1) > 0).sum()) and np.array_equal(bad != 0, gm.sum(1) > 0)
    code.repair(dd, dp, to_dev(marks_to_rs_layout(gm, k)), B)
    bad, n = verify(code, dd, dp, B)
    assert not bad.any() and n == 0
    assert torch.equal(dd[..., :B], d0[..., :B]) and torch.equal(dp[..., :B], p0[..., :B])


def test_verify_refuses_more_than_32_parity_rows():
    code = qa.Code.cauchy(4, 33)
    d = torch.zeros((2, 4, 64), dtype=torch.uint8, device=DEV)
    p = torch.zeros((2, 33, 64), dtype=torch.uint8, device=DEV)
    with pytest.raises(qa.QfecError, match="m = 33"):
        code.verify(d, p)
