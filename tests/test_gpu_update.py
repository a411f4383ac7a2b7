"""GPU tests of incremental parity: qfec_encode_update (a range of the k columns, accumulated piece by
piece) and qfec_update (one replaced data shard per group).  Every comparison is exact, against the
oracle's encode of the whole data, and every byte the calls must not write is held to its old value.

Run on an MI355X:  python -m pytest tests/test_gpu_update.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import quicknet_amd as qa
from quicknet_amd.synth import synth_bytes
from repair_common import encoded, round16, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
NONE = qa.QFEC_UPD_NONE

# (k, m, B, pitch, G): two templated m, the runtime-m kernels, the byte kernels (pitch 37), a lane
# count that is no multiple of the block, and k + m above every LUT limit elsewhere
SHAPES = [(10, 3, 1024, 1040, 300), (16, 4, 1400, 1424, 300), (9, 5, 100, 128, 300), (4, 2, 37, 37, 300),
          (10, 3, 1024, 1040, 301), (40, 8, 64, 64, 50)]
CASES = [("cauchy",) + s for s in SHAPES] + [("vandermonde",) + SHAPES[0], ("vandermonde",) + SHAPES[2]]
case_ids = [f"{c[0]}-{c[1]}-{c[2]}-B{c[3]}-G{c[5]}" for c in CASES]


def oracle_parity(oracle, code, data, B):
    """The oracle's encode of host data [G, k, pitch] -> parity [G, m, B]."""
    data = np.ascontiguousarray(data)
    out = np.zeros((data.shape[0], code.m, data.shape[2]), np.uint8)
    oracle.rs_encode(code.rows, data, out, B)
    return out[..., :B]


def shard_ids(k, G):
    """Groups 0 and G-1 touched, ids 0 and k-1 both present, every third group untouched."""
    s = np.array([(g * 7) % k for g in range(G)], np.int32)
    s[1::3] = NONE
    s[0], s[G - 1] = 0, k - 1
    return s


def new_rows(seed, G, pitch):
    return synth_bytes(seed, G * pitch).reshape(G, pitch)


def apply(data, shard, rows, B):
    """Host copy of data [G, k, pitch] with row shard[g] of every touched group replaced in [0, B)."""
    out = data.copy()
    hit = np.nonzero((shard >= 0) & (shard < data.shape[1]))[0]
    out[hit, shard[hit], :B] = rows[hit, :B]
    return out


def check_untouched(before, after, shard, B, what):
    """[G, r, pitch] host arrays: bytes [round16(B), pitch) of every row, and every byte of every
    group whose id is negative, are as before."""
    assert np.array_equal(before[..., round16(B):], after[..., round16(B):]), f"{what}: padding written"
    idle = shard < 0
    assert np.array_equal(before[idle], after[idle]), f"{what}: an untouched group was written"


def check_other_rows(before, after, shard):
    """Data rows other than shard[g] are unchanged over the whole pitch."""
    keep = np.ones(before.shape[:2], bool)
    hit = np.nonzero(shard >= 0)[0]
    keep[hit, shard[hit]] = False
    assert np.array_equal(before[keep], after[keep])


# ------------------------------------------------------------------ the range form

@pytest.mark.parametrize("flavour,k,m,B,pitch,G", CASES, ids=case_ids)
def test_partition_gives_the_encode(oracle, flavour, k, m, B, pitch, G):
    """[0, a) overwriting, then [a, b) and [b, k) accumulating, onto parity full of 0xA5: bytes
    [0, B) equal code.encode of the whole data and the oracle's encode; so does count = k alone."""
    code, data, enc = encoded(flavour, k, m, B, pitch, G)
    ref = oracle_parity(oracle, code, data.cpu().numpy(), B)
    assert np.array_equal(enc[..., :B].cpu().numpy(), ref)
    for a, b in ((1, 2), (k // 2, k - 1)):
        assert 0 < a < b < k
        par = torch.full((G, m, pitch), 0xA5, dtype=torch.uint8, device=DEV)
        code.encode_update(data[:, :a].contiguous(), par, 0, B, accumulate=False)
        code.encode_update(data[:, a:b].contiguous(), par, a, B, accumulate=True)
        code.encode_update(data[:, b:].contiguous(), par, b, B)
        torch.cuda.synchronize()
        got = par.cpu().numpy()
        assert np.array_equal(got[..., :B], ref), (a, b)
        assert (got[..., round16(B):] == 0xA5).all(), "padding written"
    par = torch.full((G, m, pitch), 0xA5, dtype=torch.uint8, device=DEV)
    code.encode_update(data, par, 0, B, accumulate=False)
    torch.cuda.synchronize()
    got = par.cpu().numpy()
    assert np.array_equal(got[..., :B], ref)
    assert (got[..., round16(B):] == 0xA5).all(), "padding written"


@pytest.mark.parametrize("flavour,k,m,B,pitch,G", CASES, ids=case_ids)
def test_accumulate_is_xor(flavour, k, m, B, pitch, G):
    """The same piece accumulated twice leaves [0, B) of the parity as it was, and changes it in between."""
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    before = par.cpu().numpy()
    piece = data[:, k - 2:].contiguous()
    code.encode_update(piece, par, k - 2, B, accumulate=True)
    torch.cuda.synchronize()
    once = par.cpu().numpy()
    assert not np.array_equal(once[..., :B], before[..., :B])
    code.encode_update(piece, par, k - 2, B, accumulate=True)
    torch.cuda.synchronize()
    twice = par.cpu().numpy()
    assert np.array_equal(twice[..., :B], before[..., :B])
    assert np.array_equal(twice[..., round16(B):], before[..., round16(B):])


# ------------------------------------------------------------------ the per-group form

@functools.lru_cache(maxsize=None)
def small_write(flavour, k, m, B, pitch, G):
    """The host side of one small-write case, computed once: the start, two rounds of ids and new
    rows, and the data after each round."""
    _, data, par = encoded(flavour, k, m, B, pitch, G)
    d0, p0 = data.cpu().numpy(), par.cpu().numpy()
    s1 = shard_ids(k, G)
    s2 = np.where(s1 >= 0, (s1 + 1) % k, NONE).astype(np.int32)
    r1, r2 = new_rows(1000 + B, G, pitch), new_rows(2000 + B, G, pitch)
    d1 = apply(d0, s1, r1, B)
    d2 = apply(d1, s2, r2, B)
    return d0, p0, s1, s2, r1, r2, d1, d2


@pytest.mark.parametrize("flavour,k,m,B,pitch,G", CASES, ids=case_ids)
def test_small_write(oracle, flavour, k, m, B, pitch, G):
    """After update: the touched row is the new row, the parity is the oracle's encode of the new
    data, verify finds nothing, and nothing else moved.  A second update of another shard in the
    same groups composes."""
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    d0, p0, s1, s2, r1, r2, d1, d2 = small_write(flavour, k, m, B, pitch, G)
    assert s1[0] >= 0 and s1[G - 1] >= 0 and (s1 == 0).any() and (s1 == k - 1).any()
    assert (s1[1:G - 1:3] == NONE).all()  # every third group, but for the last, which is touched
    before_d, before_p = d0, p0
    for shard, rows, after in ((s1, r1, d1), (s2, r2, d2)):
        rows_dev = to_dev(rows)
        code.update(to_dev(shard), rows_dev, par, data=data, block_size=B)
        bad = code.verify(data, par, B)
        torch.cuda.synchronize()
        got_d, got_p = data.cpu().numpy(), par.cpu().numpy()
        assert np.array_equal(got_d[..., :B], after[..., :B])
        assert np.array_equal(got_p[..., :B], oracle_parity(oracle, code, after, B))
        assert not bad.cpu().numpy().any()
        check_untouched(before_d, got_d, shard, B, "data")
        check_untouched(before_p, got_p, shard, B, "parity")
        check_other_rows(before_d, got_d, shard)
        assert np.array_equal(rows_dev.cpu().numpy(), rows)
        before_d, before_p = got_d, got_p


@pytest.mark.parametrize("flavour,k,m,B,pitch,G", CASES, ids=case_ids)
def test_delta_only(oracle, flavour, k, m, B, pitch, G):
    """data = None and rows = old ^ new from the host: the parity of test_small_write, and no data."""
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    d0, p0, s1, _, r1, _, d1, _ = small_write(flavour, k, m, B, pitch, G)
    delta = r1.copy()
    hit = np.nonzero(s1 >= 0)[0]
    delta[hit] ^= d0[hit, s1[hit]]
    code.update(to_dev(s1), to_dev(delta), par, data=None, block_size=B)
    torch.cuda.synchronize()
    got_p = par.cpu().numpy()
    assert np.array_equal(got_p[..., :B], oracle_parity(oracle, code, d1, B))
    check_untouched(p0, got_p, s1, B, "parity")
    assert np.array_equal(data.cpu().numpy(), d0)


@pytest.mark.parametrize("flavour,k,m,B,pitch,G", CASES, ids=case_ids)
def test_invalid_ids(oracle, flavour, k, m, B, pitch, G):
    """Ids k, k + m and 2^31 - 1: those groups are unchanged byte for byte and counted, the counter
    accumulates over a second call, and the valid groups beside them are still updated."""
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    d0, p0, s1, _, r1, _, _, _ = small_write(flavour, k, m, B, pitch, G)
    shard = s1.copy()
    shard[[3, 4, G // 2, G - 2]] = [k, k + m, 2**31 - 1, k]
    n_bad = int((shard >= k).sum())
    assert n_bad == 4
    expect = apply(d0, shard, r1, B)
    count = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    sd, rd = to_dev(shard), to_dev(r1)
    code.update(sd, rd, par, data=data, block_size=B, invalid=count)
    torch.cuda.synchronize()
    got_d, got_p = data.cpu().numpy(), par.cpu().numpy()
    assert int(count.item()) == 5 + n_bad
    valid = np.where(shard >= k, NONE, shard)
    check_untouched(d0, got_d, valid, B, "data")
    check_untouched(p0, got_p, valid, B, "parity")
    assert np.array_equal(got_d[..., :B], expect[..., :B])
    assert np.array_equal(got_p[..., :B], oracle_parity(oracle, code, expect, B))
    # again: the rows are already in place, so the delta is zero; only the counter moves
    code.update(sd, rd, par, data=data, block_size=B, invalid=count)
    torch.cuda.synchronize()
    assert int(count.item()) == 5 + 2 * n_bad
    assert np.array_equal(par.cpu().numpy()[..., :B], got_p[..., :B])
    # no counter: the same outcome
    code.update(sd, rd, par, data=data, block_size=B)
    torch.cuda.synchronize()
    assert np.array_equal(data.cpu().numpy(), got_d)


@functools.lru_cache(maxsize=None)
def mul_table(oracle):
    return np.array([[oracle.mul(a, b) for b in range(256)] for a in range(256)], np.uint8)


def test_true_products_with_a_stale_quirk_code(oracle):
    """Explicit rows with rs_stale_quirk and a zero in column 0 of row 1: update of shard 0 and
    encode_update over [0, 1) are plain GF products -- the zero coefficient contributes nothing,
    where qfec_encode would start that row from the parity's previous bytes."""
    k, m, B, G = 4, 3, 64, 40
    rows = np.array([[3, 7, 11, 19], [0, 5, 9, 33], [2, 4, 8, 16]], np.uint8)
    code = qa.Code.from_rows(rows, rs_stale_quirk=True)
    mul = mul_table(oracle)
    data = synth_bytes(61, G * k * B).reshape(G, k, B)
    par0 = synth_bytes(62, G * m * B).reshape(G, m, B)
    new = new_rows(63, G, B)
    delta = data[:, 0] ^ new
    # update of shard 0 in every group
    dd, dp = to_dev(data), to_dev(par0)
    code.update(to_dev(np.zeros(G, np.int32)), to_dev(new), dp, data=dd)
    torch.cuda.synchronize()
    expect = par0.copy()
    for j in range(m):
        expect[:, j] ^= mul[rows[j, 0], delta]
    assert np.array_equal(dp.cpu().numpy(), expect)
    assert np.array_equal(expect[:, 1], par0[:, 1])
    assert np.array_equal(dd.cpu().numpy()[:, 0], new) and np.array_equal(dd.cpu().numpy()[:, 1:], data[:, 1:])
    # encode_update over column 0: overwriting, then accumulating
    piece = to_dev(data[:, :1])
    dp = to_dev(par0)
    code.encode_update(piece, dp, 0, accumulate=False)
    torch.cuda.synchronize()
    prod = np.stack([mul[rows[j, 0], data[:, 0]] for j in range(m)], axis=1)
    assert not prod[:, 1].any()
    assert np.array_equal(dp.cpu().numpy(), prod)
    dp = to_dev(par0)
    code.encode_update(piece, dp, 0, accumulate=True)
    torch.cuda.synchronize()
    assert np.array_equal(dp.cpu().numpy(), par0 ^ prod)


def test_update_then_verify_on_a_side_stream():
    """update and the verify that checks it on a non-default stream, nothing between them."""
    flavour, k, m, B, pitch, G = CASES[0]
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    _, _, s1, _, r1, _, d1, _ = small_write(flavour, k, m, B, pitch, G)
    shard, rows = to_dev(s1), to_dev(r1)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        code.update(shard, rows, par, data=data, block_size=B)
        bad = code.verify(data, par, B, bad_groups=count)
    side.synchronize()
    assert int(count.item()) == 0 and not bad.cpu().numpy().any()
    assert np.array_equal(data.cpu().numpy()[..., :B], d1[..., :B])
