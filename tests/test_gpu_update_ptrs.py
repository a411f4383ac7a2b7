"""GPU tests of incremental parity on pointer tables: qfec_encode_update_ptrs (a range of the k data
shards of every group, accumulated piece by piece) and qfec_update_ptrs (one replaced data shard per
group).  Every comparison is exact.  Expected bytes come from the oracle's rs_encode (the quirk case:
from its GF tables).  The rows, those d_new points at included, live in a guard-filled pool
(update_ptrs_common.UpdPool) in permuted slots, and after every call the WHOLE pool is compared with
the expected image.  Every table entry a call must not address holds the address of the misaligned
guard row: data outside the range, every entry (and the d_new entry) of a group with a negative or an
invalid id, every data entry but the replaced one, and in delta mode every data entry.

Run on an MI355X:  python -m pytest tests/test_gpu_update_ptrs.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import quicknet_amd as qa
import ptrs_common as pc
import update_ptrs_common as uc
from update_ptrs_common import NONE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")

# (k, m, B, G): a slab border and one byte past it, an 8-byte tail, runtime m, the small odd sizes,
# k + m = 68: more entries than a wave has lanes, and m = 70: so many in the per-group form as well
SHAPES = [(10, 3, 1024, 60), (10, 3, 1025, 60), (16, 4, 1400, 60), (9, 5, 100, 60), (4, 2, 37, 60), (4, 2, 1, 9),
          (4, 2, 15, 9), (4, 2, 17, 9), (40, 8, 64, 20), (60, 8, 48, 12), (3, 70, 33, 9)]
CASES = [("cauchy",) + s for s in SHAPES] + [("vandermonde",) + SHAPES[0], ("vandermonde",) + SHAPES[3]]
case_ids = [f"{c[0]}-{c[1]}-{c[2]}-B{c[3]}-G{c[4]}" for c in CASES]
modes = pytest.mark.parametrize("mode", uc.MODES)
cases = pytest.mark.parametrize("flavour,k,m,B,G", CASES, ids=case_ids)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def counter(start=0):
    return torch.full((1,), start, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def batch_bytes(flavour, k, m, B, G):
    """The host side of one shape, computed once and never changed: the code's rows, data, stale parity
    bytes, two rounds of new rows."""
    code = getattr(qa.Code, flavour)(k, m)
    seed = 0x0D00 + 64 * k + B
    out = (code.rows, pc.batch_bytes(seed, G, k, B), pc.batch_bytes(seed + 1, G, m, B), pc.batch_bytes(seed + 2, 2, G, B))
    for a in out:
        a.setflags(write=False)
    return out


def make_pool(flavour, k, m, B, G, mode, parity):
    """UpdPool holding the data, `parity` [G, m, B] and the two rounds of new rows."""
    _, data, _, new = batch_bytes(flavour, k, m, B, G)
    vp = uc.UpdPool(G, k, m, B, mode, 0xB00 + k + B, rounds=2)
    full = np.full((G, k), B)
    vp.put_data(data, full)
    vp.put_parity(parity, np.full(G, B))
    for j in range(2):
        for g in range(G):
            vp.put(vp.new_row(g, j), new[j, g], B)
    return vp


def with_parity(vp, img, par):
    """The pool image `img` with [0, B) of every parity row replaced."""
    out = img.copy()
    for g in range(vp.G):
        for r in range(vp.m):
            vp.write(out, vp.parity_row(g, r), par[g, r], vp.max_len)
    return out


def oracle_parity(oracle, rows, data, B, cols=None):
    return uc.encode_padded(oracle, rows, data, np.full(data.shape[:2], B), B, cols)


# ------------------------------------------------------------------ the range form

@modes
@cases
def test_partitions_give_the_encode(oracle, flavour, k, m, B, G, mode):
    """Every two-way and one three-way partition of [0, k), the first piece overwriting parity shards
    full of other bytes, the others accumulating: the pool equals the one qfec_encode_ptrs leaves, and
    the oracle's.  Data entries outside a call's range hold the guard row's address."""
    rows, data, stale, _ = batch_bytes(flavour, k, m, B, G)
    code = getattr(qa.Code, flavour)(k, m)
    vp = make_pool(flavour, k, m, B, G, mode, stale)
    start = vp.clone_host()
    expect = with_parity(vp, start, oracle_parity(oracle, rows, data, B))
    t, addr = vp.upload(torch, DEV)
    backup = t.clone()
    code.encode_ptrs(dev(vp.table(addr)), B)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), expect), "encode_ptrs and the oracle disagree"
    parts = uc.partitions(k)
    assert len(parts) == k - 1 + (k >= 3) and any(len(p) == 3 for p in parts)
    for pieces in parts:
        t.copy_(backup)
        for j, (first, count) in enumerate(pieces):
            keep = np.tile(uc.range_mask(k, first, count), (G, 1))
            code.encode_update_ptrs(dev(vp.table(addr, keep)), first, count, B, accumulate=j > 0)
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), expect), (mode, pieces)
    # count = k alone, overwriting
    t.copy_(backup)
    code.encode_update_ptrs(dev(vp.table(addr)), 0, k, B, accumulate=False)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), expect), mode


@modes
@cases
def test_pieces_one_by_one(oracle, flavour, k, m, B, G, mode):
    """After each piece of the three-way partition the pool holds exactly the products of the shards
    seen so far, and accumulating the same piece twice leaves the pool as it was: accumulate is an XOR."""
    rows, data, stale, _ = batch_bytes(flavour, k, m, B, G)
    code = getattr(qa.Code, flavour)(k, m)
    vp = make_pool(flavour, k, m, B, G, mode, stale)
    start = vp.clone_host()
    t, addr = vp.upload(torch, DEV)
    seen = np.zeros(k, bool)
    pieces = uc.partitions(k)[-1]
    for j, (first, count) in enumerate(pieces):
        seen |= uc.range_mask(k, first, count)
        keep = np.tile(uc.range_mask(k, first, count), (G, 1))
        code.encode_update_ptrs(dev(vp.table(addr, keep)), first, count, B, accumulate=j > 0)
        torch.cuda.synchronize()
        expect = with_parity(vp, start, oracle_parity(oracle, rows, data, B, seen))
        assert np.array_equal(t.cpu().numpy(), expect), (mode, first, count)
    first, count = pieces[-1]
    table = dev(vp.table(addr, np.tile(uc.range_mask(k, first, count), (G, 1))))
    code.encode_update_ptrs(table, first, count, B)
    torch.cuda.synchronize()
    once = t.cpu().numpy()
    assert np.array_equal(once, with_parity(vp, start, oracle_parity(oracle, rows, data, B, seen & ~uc.range_mask(k, first, count))))
    assert not np.array_equal(once, expect)
    code.encode_update_ptrs(table, first, count, B, accumulate=True)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), expect), mode


# ------------------------------------------------------------------ the per-group form

def apply(data, shard, new):
    """data [G, k, B] with row shard[g] of every touched group replaced by new[g]."""
    out = data.copy()
    hit = np.nonzero((shard >= 0) & (shard < data.shape[1]))[0]
    out[hit, shard[hit]] = new[hit]
    return out


def image(vp, start, data, par):
    """The pool image `start` with every data and parity row replaced."""
    out = with_parity(vp, start, par)
    for g in range(vp.G):
        for c in range(vp.k):
            vp.write(out, vp.data_row(g, c), data[g, c], vp.max_len)
    return out


def per_group_tables(vp, addr, shard, j, delta=False):
    """(table, d_new) of one update: only the replaced data entry of a valid group is real."""
    G, k = vp.G, vp.k
    valid = (shard >= 0) & (shard < k)
    keep = np.zeros((G, k), bool)
    if not delta:
        keep[np.nonzero(valid)[0], shard[valid]] = True
    table = vp.table(addr, keep, dead_groups=np.nonzero(~valid)[0])
    new = np.where(valid, addr[[vp.new_row(g, j) for g in range(G)]], addr[vp.guard_row])
    return dev(table), dev(new.astype(np.int64))


@modes
@cases
def test_small_write(oracle, flavour, k, m, B, G, mode):
    """After update_ptrs the replaced shard is the new row, the parity is the oracle's encode of the new
    data, verify_ptrs finds nothing and nothing else in the pool moved; a second update of another shard
    of the same groups composes."""
    rows, d0, _, new = batch_bytes(flavour, k, m, B, G)
    code = getattr(qa.Code, flavour)(k, m)
    vp = make_pool(flavour, k, m, B, G, mode, oracle_parity(oracle, rows, d0, B))
    start = vp.clone_host()
    t, addr = vp.upload(torch, DEV)
    s1 = uc.shard_ids(k, G)
    uc.assert_ids_cover(s1, k, G)
    s2 = np.where(s1 >= 0, (s1 + 1) % k, NONE).astype(np.int32)
    data = d0
    for j, shard in enumerate((s1, s2)):
        data = apply(data, shard, new[j])
        table, dn = per_group_tables(vp, addr, shard, j)
        inv = counter(3)
        code.update_ptrs(table, dev(shard), dn, B, invalid=inv)
        bad = code.verify_ptrs(dev(vp.table(addr)), B) if m <= 32 else None  # qfec_verify_ptrs takes m <= 32
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), image(vp, start, data, oracle_parity(oracle, rows, data, B))), (mode, j)
        assert (bad is None or not bad.cpu().numpy().any()) and int(inv.item()) == 3


@modes
@cases
def test_delta_only(oracle, flavour, k, m, B, G, mode):
    """d_new holds old ^ new and every data entry the guard row's address: the parity of
    test_small_write, and no data shard written."""
    rows, d0, _, new = batch_bytes(flavour, k, m, B, G)
    code = getattr(qa.Code, flavour)(k, m)
    s1 = uc.shard_ids(k, G)
    hit = np.nonzero(s1 >= 0)[0]
    vp = make_pool(flavour, k, m, B, G, mode, oracle_parity(oracle, rows, d0, B))
    for g in hit:  # the delta takes the new row's place in the pool
        vp.put(vp.new_row(g, 0), new[0, g] ^ d0[g, s1[g]], B)
    start = vp.clone_host()
    t, addr = vp.upload(torch, DEV)
    table, dn = per_group_tables(vp, addr, s1, 0, delta=True)
    code.update_ptrs(table, dev(s1), dn, B, delta_only=True)
    torch.cuda.synchronize()
    expect = with_parity(vp, start, oracle_parity(oracle, rows, apply(d0, s1, new[0]), B))
    assert np.array_equal(t.cpu().numpy(), expect), mode


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@cases
def test_invalid_ids(oracle, flavour, k, m, B, G, mode):
    """Ids k, k + m and 2^31 - 1: those groups are unchanged byte for byte and each counted exactly
    once, the counter accumulates over a second call, and the valid groups beside them are updated."""
    rows, d0, _, new = batch_bytes(flavour, k, m, B, G)
    code = getattr(qa.Code, flavour)(k, m)
    shard = uc.shard_ids(k, G).copy()
    where = [2, 5, G - 2]
    shard[where] = [k, k + m, 2**31 - 1]
    assert len(set(where)) == 3 and 0 not in where and G - 1 not in where
    vp = make_pool(flavour, k, m, B, G, mode, oracle_parity(oracle, rows, d0, B))
    start = vp.clone_host()
    t, addr = vp.upload(torch, DEV)
    table, dn = per_group_tables(vp, addr, shard, 0)
    after = apply(d0, shard, new[0])
    expect = image(vp, start, after, oracle_parity(oracle, rows, after, B))
    inv = counter(5)
    code.update_ptrs(table, dev(shard), dn, B, invalid=inv)
    torch.cuda.synchronize()
    assert int(inv.item()) == 5 + 3
    assert np.array_equal(t.cpu().numpy(), expect), mode
    # again: the rows are already in place, so the delta is zero; only the counter moves.  Then no counter.
    code.update_ptrs(table, dev(shard), dn, B, invalid=inv)
    code.update_ptrs(table, dev(shard), dn, B)
    torch.cuda.synchronize()
    assert int(inv.item()) == 5 + 6
    assert np.array_equal(t.cpu().numpy(), expect), mode


@functools.lru_cache(maxsize=None)
def mul_table(oracle):
    return np.array([[oracle.mul(a, b) for b in range(256)] for a in range(256)], np.uint8)


@pytest.mark.parametrize("mode", ["aligned", "residues"])
def test_true_products_with_a_stale_quirk_code(oracle, mode):
    """Explicit rows with rs_stale_quirk and a zero in column 0 of row 1: update_ptrs of shard 0 and
    encode_update_ptrs over [0, 1) are plain GF products -- the zero coefficient contributes nothing,
    where qfec_encode_ptrs would start that row from the parity's previous bytes."""
    k, m, B, G = 4, 3, 70, 12
    rows = np.array([[3, 7, 11, 19], [0, 5, 9, 33], [2, 4, 8, 16]], np.uint8)
    code = qa.Code.from_rows(rows, rs_stale_quirk=True)
    mul = mul_table(oracle)
    data, par0, new = pc.batch_bytes(61, G, k, B), pc.batch_bytes(62, G, m, B), pc.batch_bytes(63, 1, G, B)[0]
    vp = uc.UpdPool(G, k, m, B, mode, 0x57A1E)
    vp.put_data(data, np.full((G, k), B))
    vp.put_parity(par0, np.full(G, B))
    for g in range(G):
        vp.put(vp.new_row(g), new[g], B)
    start = vp.clone_host()
    t, addr = vp.upload(torch, DEV)
    backup = t.clone()
    shard = np.zeros(G, np.int32)
    table, dn = per_group_tables(vp, addr, shard, 0)
    code.update_ptrs(table, dev(shard), dn, B)
    torch.cuda.synchronize()
    par = par0.copy()
    for j in range(m):
        par[:, j] ^= mul[rows[j, 0], data[:, 0] ^ new]
    assert np.array_equal(par[:, 1], par0[:, 1])
    assert np.array_equal(t.cpu().numpy(), image(vp, start, apply(data, shard, new), par))
    prod = np.stack([mul[rows[j, 0], data[:, 0]] for j in range(m)], axis=1)
    assert not prod[:, 1].any()
    for accumulate, want in ((False, prod), (True, par0 ^ prod)):
        t.copy_(backup)
        code.encode_update_ptrs(dev(vp.table(addr, np.tile(uc.range_mask(k, 0, 1), (G, 1)))), 0, 1, B, accumulate=accumulate)
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), with_parity(vp, start, want)), accumulate


def test_update_then_verify_on_a_side_stream(oracle):
    """update_ptrs and the verify_ptrs that checks it on a non-default stream, nothing between them."""
    flavour, k, m, B, G = CASES[0]
    rows, d0, _, new = batch_bytes(flavour, k, m, B, G)
    code = getattr(qa.Code, flavour)(k, m)
    vp = make_pool(flavour, k, m, B, G, "one-new", oracle_parity(oracle, rows, d0, B))
    start = vp.clone_host()
    t, addr = vp.upload(torch, DEV)
    s1 = uc.shard_ids(k, G)
    table, dn = per_group_tables(vp, addr, s1, 0)
    shard, full, count = dev(s1), dev(vp.table(addr)), counter()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        code.update_ptrs(table, shard, dn, B)
        bad = code.verify_ptrs(full, B, bad_groups=count)
    side.synchronize()
    assert int(count.item()) == 0 and not bad.cpu().numpy().any()
    after = apply(d0, s1, new[0])
    assert np.array_equal(t.cpu().numpy(), image(vp, start, after, oracle_parity(oracle, rows, after, B)))
