"""GPU tests of incremental parity on pointer tables with per-shard lengths: qfec_encode_update_ptrs_var
and qfec_update_ptrs_var.  Every comparison is exact.  Rows live in a guard-filled pool
(update_ptrs_common.UpdPool, a ptrs_var_common.VarPool with the rows d_new points at) and are written to
their own lengths only, so a byte read past a length that reaches a result shows as a wrong byte; the
WHOLE pool is compared after every call, so a byte written outside a stated extent fails.  Expected
bytes come from the oracle's rs_encode on rows zero-padded on the CPU.  Entries of shards of length 0
and entries a call must not address hold the address of the misaligned guard row.  Every pattern list
asserts its own coverage on the CPU before the GPU is called.

Run on an MI355X:  python -m pytest tests/test_gpu_update_ptrs_var.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import quicknet_amd as qa
import ptrs_common as pc
import ptrs_var_common as pv
import update_ptrs_common as uc
from update_ptrs_common import INT_MAX, INT_MIN, NONE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
# (60,8) and (3,70): the entries a group may dereference pass 64 (count + m, 2 + m), so addresses and
# lengths are read at the point of use.  The integrity calls take m <= 32 (locate: k <= 32 as well).
CONFIGS = [(4, 2, 37), (9, 5, 100), (10, 3, 1040), (16, 4, 1400), (40, 8, 64), (60, 8, 48), (3, 70, 40)]
config_ids = [f"{k}-{m}-max{ml}" for k, m, ml in CONFIGS]
configs = pytest.mark.parametrize("k,m,max_len", CONFIGS, ids=config_ids)
modes = pytest.mark.parametrize("mode", uc.MODES)
STALE = 0x5C  # what no oracle byte is compared against: parity bytes at or past L before a call


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def i32(a):
    return dev(np.clip(np.asarray(a, np.int64), INT_MIN, INT_MAX).astype(np.int32).reshape(-1))


def counter(start=0):
    return torch.full((1,), start, dtype=torch.int32, device=DEV)


def put_rows(vp, flat, row_of, rows, lens, at=0):
    """Bytes [at, lens[g]) of row row_of(g, j) of the image become rows[g, j]."""
    for g in range(rows.shape[0]):
        for j in range(rows.shape[1]):
            n = int(np.broadcast_to(lens, rows.shape[:2])[g, j])
            vp.write(flat, row_of(g, j), rows[g, j], n, at)


# ------------------------------------------------------------------ the range form

def range_batch(k, m, max_len, mode, pats, glen, seed):
    """(UpdPool, lens [G,k], data, stale parity): data rows written to their lengths, parity rows to
    max_len with other bytes; entries of data shards of length 0 (void lengths included: they are judged
    before anything is dereferenced) and the parity entries of a group with L outside (0, max_len] are
    the guard row."""
    G = len(pats)
    lens = np.stack([l for _, l in pats]).astype(np.int64)
    data, stale = pc.batch_bytes(seed, G, k, max_len), pc.batch_bytes(seed + 1, G, m, max_len)
    vp = uc.UpdPool(G, k, m, max_len, mode, seed + 2)
    vp.put_data(data, lens)
    vp.put_parity(stale, np.full(G, max_len))
    for g in range(G):
        if not 0 < glen[g] <= max_len:
            for r in range(m):
                vp.alias[vp.parity_row(g, r)] = vp.guard_row
    return vp, lens, data, stale


def range_table(vp, addr, first, count):
    """Data entries outside [first, first + count), and the aliased entries, are the guard row."""
    tab = vp.table(addr, np.tile(uc.range_mask(vp.k, first, count), (vp.G, 1)))
    for i, j in vp.alias.items():
        tab[i] = addr[j]
    return dev(tab)


def valid_patterns(k, max_len):
    pats = pv.length_patterns(k, max_len)
    pv.assert_lengths_cover(pats + pv.void_patterns(k, max_len), k, max_len)  # before the GPU is called
    return pats


@modes
@configs
@pytest.mark.parametrize("tight", [False, True], ids=["L=max_len", "L=longest"])
def test_partitions_give_encode_ptrs_var(oracle, k, m, max_len, mode, tight):
    """A two-way and a three-way partition of [0, k), the first piece overwriting: after every piece
    exactly [0, L) of the parity rows holds the products of the shards seen so far -- zero from the
    longest of them on after the overwrite, untouched there by an accumulate -- and nothing at or past L
    moved.  At the end [0, longest) is what encode_ptrs_var writes and verify_ptrs_var is clean."""
    code = qa.Code.cauchy(k, m)
    pats = valid_patterns(k, max_len)
    G = len(pats)
    longest = np.stack([l for _, l in pats]).max(1)
    glen = longest if tight else np.full(G, max_len)
    assert (longest < glen).any() or tight
    vp, lens, data, stale = range_batch(k, m, max_len, mode, pats, glen, 0xE700 + 32 * k + max_len)
    start = vp.clone_host()
    t, addr = vp.upload(torch, DEV)
    backup = t.clone()
    dl, gl = i32(lens), i32(glen)
    parts = uc.partitions(k)
    for pieces in (parts[k // 2 - 1], parts[-1]):
        t.copy_(backup)
        seen, inv = np.zeros(k, bool), counter(4)
        for j, (first, count) in enumerate(pieces):
            seen |= uc.range_mask(k, first, count)
            code.encode_update_ptrs_var(range_table(vp, addr, first, count), first, count, dl, gl, max_len,
                                        accumulate=j > 0, invalid=inv)
            torch.cuda.synchronize()
            expect = start.copy()
            put_rows(vp, expect, vp.parity_row, uc.encode_padded(oracle, code.rows, data, lens, max_len, seen), glen[:, None])
            assert np.array_equal(t.cpu().numpy(), expect), (mode, pieces, j)
        assert int(inv.item()) == 4
        # the whole: equal to encode_ptrs_var below the longest length, zero from there to L, clean
        full_table = range_table(vp, addr, 0, k)
        bad = code.verify_ptrs_var(full_table, dl, gl, max_len) if m <= 32 else None
        t2 = backup.clone()
        shift = t2.data_ptr() - t.data_ptr()
        code.encode_ptrs_var(full_table + shift, dl, max_len)
        torch.cuda.synchronize()
        assert bad is None or not bad.cpu().numpy().any()
        got, ref = t.cpu().numpy(), t2.cpu().numpy()
        for g in range(G):
            for r in range(m):
                i = vp.parity_row(g, r)
                assert np.array_equal(vp.row(got, i, longest[g]), vp.row(ref, i, longest[g])), (pats[g][0], r)
                assert not vp.row(got, i, glen[g])[longest[g]:].any(), (pats[g][0], r)


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@configs
def test_range_invalid_groups(oracle, k, m, max_len, mode):
    """L outside [0, max_len], or a length of the range outside [0, L] with all four void values: the
    group is counted once and untouched.  The same bad length outside the range is not looked at: the
    group is worked on like its neighbours."""
    code = qa.Code.cauchy(k, m)
    voids = pv.void_patterns(k, max_len)
    lad = pv.ladder(k, max_len)
    pats = voids + [("ok", lad)] + [(f"L={L}", lad) for L in (-1, max_len + 1, INT_MIN, INT_MAX)] + [("short-L", lad)]
    G = len(pats)
    glen = np.array([max_len] * (len(voids) + 1) + [-1, max_len + 1, INT_MIN, INT_MAX] + [max_len - 1], np.int64)
    bad_at = [int(np.flatnonzero((l < 0) | (l > max_len))[0]) for _, l in voids]
    assert len(set(bad_at)) > 1 or k < 3
    vp, lens, data, stale = range_batch(k, m, max_len, mode, pats, glen, 0x1BAD + k + max_len)
    start = vp.clone_host()
    t, addr = vp.upload(torch, DEV)
    backup = t.clone()
    dl, gl = i32(lens), i32(glen)
    hit = 0
    for first, count in [(0, k)] + [(c, 1) for c in sorted(set(bad_at))] + [(0, 1), (k - 1, 1)]:
        cols = uc.range_mask(k, first, count)
        invalid = np.array([not 0 <= glen[g] <= max_len or bool(((lens[g][cols] < 0) | (lens[g][cols] > glen[g])).any())
                            for g in range(G)])
        assert invalid[-1] == bool(cols[k - 1]) and not invalid[len(voids)], "short-L: max_len > L only in the last shard"
        hit += int((invalid[:len(voids)] != np.array([cols[c] for c in bad_at])).sum() == 0)
        for accumulate in (False, True):
            t.copy_(backup)
            inv = counter(9)
            code.encode_update_ptrs_var(range_table(vp, addr, first, count), first, count, dl, gl, max_len,
                                        accumulate=accumulate, invalid=inv)
            torch.cuda.synchronize()
            clipped = np.where((lens < 0) | (lens > max_len), 0, lens)  # outside the range: columns that count as absent
            prod = uc.encode_padded(oracle, code.rows, data, clipped, max_len, cols)
            extent = np.where(invalid, 0, lens[:, cols].max(1) if accumulate else glen)
            expect = start.copy()
            put_rows(vp, expect, vp.parity_row, (stale ^ prod) if accumulate else prod, extent[:, None])
            assert np.array_equal(t.cpu().numpy(), expect), (mode, first, count, accumulate)
            assert int(inv.item()) == 9 + int(invalid.sum()), (first, count)
    assert hit >= 3


# ------------------------------------------------------------------ the per-group form

EXTRA = [  # (name, i, o, n, L): groups that must be left alone; o None: the ladder's own length
    ("none", NONE, None, 5, None), ("id=k", "k", None, 5, None), ("id=k+m", "k+m", None, 5, None), ("id=max", INT_MAX, None, 5, None),
    ("n=-1", 0, None, -1, None), ("n=L+1", 0, None, "L+1", "short"), ("n=INT_MIN", 0, None, INT_MIN, None), ("n=INT_MAX", 0, None, INT_MAX, None),
    ("bad-o=-1", 1, -1, 5, None), ("bad-o=L+1", 1, "L+1", 5, "short"), ("bad-o=INT_MIN", 1, INT_MIN, 5, None), ("bad-o=INT_MAX", 1, INT_MAX, 5, None),
    ("L=-1", 0, None, 0, -1), ("L=max+1", 0, None, 5, "max+1"), ("L=INT_MIN", 0, None, 0, INT_MIN), ("L=INT_MAX", 0, None, 5, INT_MAX),
]


@functools.lru_cache(maxsize=None)
def update_groups(k, m, max_len):
    """(names, lens [G,k], shard, n, L, counted, acts): the valid patterns, then the groups of EXTRA."""
    pats = uc.update_patterns(k, max_len)
    uc.assert_updates_cover(pats, k, max_len)  # before the GPU is called
    names, lens, shard, n, L = [p[0] for p in pats], [p[1] for p in pats], [p[2] for p in pats], [p[3] for p in pats], [p[4] for p in pats]
    short = max(max_len - 3, 0)
    sym = {"k": k, "k+m": k + m, "max+1": max_len + 1, "short": short, None: max_len}
    for name, i, o, nn, LL in EXTRA:
        LL = sym.get(LL, LL)
        i = sym.get(i, i) if isinstance(i, str) else i
        l = np.minimum(pv.ladder(k, max_len), max(min(LL, max_len), 0))
        if o is not None:
            l[i] = LL + 1 if o == "L+1" else o
        names.append(name), lens.append(l), shard.append(i), n.append(LL + 1 if nn == "L+1" else nn), L.append(LL)
    lens, shard, n, L = np.stack(lens).astype(np.int64), np.array(shard, np.int64), np.array(n, np.int64), np.array(L, np.int64)
    G = len(names)
    ids_ok = (shard >= 0) & (shard < k)
    o = np.where(ids_ok, lens[np.arange(G), np.clip(shard, 0, k - 1)], 0)
    lens_ok = (L >= 0) & (L <= max_len) & (n >= 0) & (n <= L) & (o >= 0) & (o <= L)
    counted = (shard >= k) | (ids_ok & ~lens_ok)
    acts = ids_ok & lens_ok
    assert counted.sum() == len(EXTRA) - 1 and acts.sum() == len(pats) and not acts[len(pats):].any()
    return names, lens, shard, n, L, counted, acts


def update_case(oracle, k, m, max_len, mode, delta):
    code = qa.Code.cauchy(k, m)
    names, lens, shard, n, L, counted, acts = update_groups(k, m, max_len)
    G, rows = len(names), np.arange(len(names))
    seed = 0x0D17 + 8 * k + max_len
    data, new = pc.batch_bytes(seed, G, k, max_len), pc.batch_bytes(seed + 1, 1, G, max_len)[0]
    sane = np.where((lens < 0) | (lens > max_len), 0, lens)  # what the pool holds of a shard with a void length
    o = np.where(acts, sane[rows, np.clip(shard, 0, k - 1)], 0)
    nn = np.where(acts, n, 0)
    extent = np.maximum(o, nn)
    vp = uc.UpdPool(G, k, m, max_len, mode, seed + 2)
    written = {vp.data_row(g, int(shard[g])) for g in range(G) if acts[g] and nn[g] > 0}
    vp.put_data(data, sane, keep=written)
    par0 = uc.encode_padded(oracle, code.rows, data, sane, max_len)
    padL = np.clip(L, 0, max_len)
    for g in range(G):  # parity: the encode below L, other bytes from there on
        for r in range(m):
            vp.put(vp.parity_row(g, r), np.concatenate([par0[g, r, :padL[g]], np.full(max_len - padL[g], STALE, np.uint8)]), max_len)
    after, new_lens = data.copy(), sane.copy()
    for g in np.flatnonzero(acts):
        after[g, shard[g], :nn[g]] = new[g, :nn[g]]
        new_lens[g, shard[g]] = nn[g]
    par1 = uc.encode_padded(oracle, code.rows, after, new_lens, max_len)
    sent = new.copy()  # what d_new points at, and its length
    sent_len = nn.copy()
    if delta:
        zo, zn = pv.zero_padded(data, sane)[rows, np.clip(shard, 0, k - 1)], pv.zero_padded(after, new_lens)[rows, np.clip(shard, 0, k - 1)]
        sent, sent_len = zo ^ zn, extent
    for g in np.flatnonzero(acts):
        vp.put(vp.new_row(g), sent[g], int(sent_len[g]))
    start = vp.clone_host()
    expect = start.copy()
    for g in np.flatnonzero(acts):
        if not delta:
            vp.write(expect, vp.data_row(g, int(shard[g])), new[g], int(nn[g]))
        for r in range(m):
            vp.write(expect, vp.parity_row(g, r), par1[g, r], int(extent[g]))
            assert np.array_equal(par1[g, r, extent[g]:padL[g]], par0[g, r, extent[g]:padL[g]])
    t, addr = vp.upload(torch, DEV)
    # the table: only shard i of a group that acts is real (not even that in delta mode), its d_new entry
    # only with a length to read; the lengths: garbage everywhere but at (g, i)
    keep = np.zeros((G, k), bool)
    if not delta:
        live = acts & (extent > 0)  # o = n = 0: shard i is not dereferenced either
        keep[np.flatnonzero(live), shard[live]] = True
    table = vp.table(addr, keep, dead_groups=np.flatnonzero(~acts))
    dn = np.where(acts & (sent_len > 0), addr[[vp.new_row(g) for g in range(G)]], addr[vp.guard_row]).astype(np.int64)
    call_lens = np.full((G, k), INT_MIN, np.int64)
    ids_ok = (shard >= 0) & (shard < k)
    call_lens[np.flatnonzero(ids_ok), shard[ids_ok]] = lens[np.flatnonzero(ids_ok), shard[ids_ok]]
    call_n = np.where(acts, sent_len, n)
    counted_here = counted & ~(delta & np.array([nm.startswith("bad-o=") for nm in names]))  # o is not read in delta mode
    if delta:  # a group refused for o alone acts in delta mode: leave those out of the delta batch
        drop = np.array([nm.startswith("bad-o=") for nm in names])
        shard = np.where(drop, NONE, shard)
    inv = counter(2)
    code.update_ptrs_var(dev(table), None if delta else i32(call_lens), i32(L), i32(shard), dev(dn), i32(call_n), max_len,
                         delta_only=delta, invalid=inv)
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    what = f"({k},{m}) max_len={max_len} {mode} delta={delta}"
    for g in range(G):
        for i in [vp.data_row(g, c) for c in range(k)] + [vp.parity_row(g, r) for r in range(m)]:
            assert np.array_equal(vp.row(got, i, max_len), vp.row(expect, i, max_len)), f"{what}: group {names[g]} row {i - g * k}"
    assert np.array_equal(got, expect), what
    assert int(inv.item()) == 2 + int(counted_here.sum()), what
    if delta:
        return
    # the caller stores the new lengths; then the integrity calls find nothing
    full = vp.table(addr)
    for g in range(G):
        for c in range(k):
            if new_lens[g, c] == 0 and vp.data_row(g, c) not in written:
                full[vp.data_row(g, c)] = addr[vp.guard_row]
    dl, gl = i32(np.minimum(new_lens, padL[:, None])), i32(padL)  # the groups left alone for a length: judged below L
    bad = code.verify_ptrs_var(dev(full), dl, gl, max_len) if m <= 32 else None
    culprit = code.locate_ptrs_var(dev(full), dl, gl, max_len) if k <= 32 and m <= 32 else None
    torch.cuda.synchronize()
    assert bad is None or not bad.cpu().numpy().any(), what
    assert culprit is None or (culprit.cpu().numpy() == qa.QFEC_LOC_CLEAN).all(), what
    assert np.array_equal(t.cpu().numpy(), expect), what


@modes
@configs
def test_update_ptrs_var(oracle, k, m, max_len, mode):
    """Per (o, n) pair: exactly [0, n) of the shard is written, exactly [0, max(o, n)) of each parity
    shard rewritten, and the parity matches the oracle over [0, L); groups refused for an id, n, o or L
    are counted once and untouched; no length but the replaced shard's is read; verify_ptrs_var and
    locate_ptrs_var are clean once the caller has stored the new lengths."""
    update_case(oracle, k, m, max_len, mode, delta=False)


@modes
@configs
def test_update_ptrs_var_delta_only(oracle, k, m, max_len, mode):
    """d_new holds the delta of the zero-padded rows over [0, max(o, n)), d_lens is NULL and every data
    entry the guard row's address: the same parity, no data shard written."""
    update_case(oracle, k, m, max_len, mode, delta=True)
