"""GPU tests of qfec_encode_ptrs_var / qfec_reconstruct_ptrs_var: the pointer-table calls on shards that
each have their own length.  Rows live in a guard-filled pool (ptrs_var_common.VarPool) and are written
to their own lengths only; the WHOLE pool is compared after every call with the pool before it in which
only the bytes the call must write carry the oracle's, so a byte read past a shard's length that
reaches a result, a byte written past a group's length, or anything written elsewhere (the guard row
that the shards of length 0 point at included) fails.  The expected bytes come from the oracle on rows
zero-padded on the CPU: rs_encode over max_len, of which [0, L) of each parity row is taken, and
rs_reconstruct per group with B = L.

Run on an MI355X:  python -m pytest tests/test_gpu_ptrs_var.py -m gpu -q
"""
import numpy as np
import pytest

import quicknet_amd as qa
from quicknet_amd.synth import marks_to_rs_layout
import ptrs_common as pc
import ptrs_var_common as pv

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")

SHAPES = [(10, 3), (16, 4), (4, 2), (8, 4), (9, 3), (3, 2)]
ALIGN = ["aligned", "residues", "one-data", "one-parity"]
ENC_MAX = [1, 17, 1000, 1040, 1400]
REC_MAX = [1, 17, 1000, 1400]
SENTINEL = -77  # what d_group_len holds before the encode


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32).reshape(-1)).to(DEV)


def counter():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def run(fn, t, stream):
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


# ------------------------------------------------------------------ encode

def encode_batch(oracle, rows, k, m, max_len, mode, seed, pats, alias=False, keep=()):
    """(VarPool, lens [G,k], data, expected pool, expected group_len) of one encode."""
    G = len(pats)
    lens = np.stack([l for _, l in pats]).astype(np.int64)
    data = pc.batch_bytes(seed, G, k, max_len)
    aliased = {}
    if alias:  # shard (g2, c2) is the first half of shard (g1, c1), at the same address
        for (g2, c2), (g1, c1) in alias.items():
            assert 0 < lens[g1, c1] <= max_len and 0 <= lens[g2].max() <= max_len
            lens[g2, c2] = lens[g1, c1] // 2 + 1
            data[g2, c2] = data[g1, c1]
            aliased[g2 * k + c2] = g1 * k + c1
    stale = pc.batch_bytes(seed + 1, G, m, max_len)  # what the parity shards hold before
    vp = pv.VarPool(G, k, m, max_len, mode, seed + 2)
    vp.put_data(data, lens, keep)
    vp.alias.update(aliased)
    vp.put_parity(stale, np.full(G, max_len))
    glen = pv.group_lengths(lens, max_len)
    want = stale.copy()
    oracle.rs_encode(rows, pv.zero_padded(data, lens), want, max_len)
    expect = vp.clone_host()
    for g in range(G):
        for r in range(m):
            if glen[g] > 0:
                s = vp.pool.start[G * k + g * m + r]
                expect[s:s + glen[g]] = want[g, r, :glen[g]]
    return vp, lens, data, expect, glen


def encode_case(oracle, code, rows, k, m, max_len, mode, seed, pats, alias=False, stream=None, repeat=True):
    vp, lens, _, expect, glen = encode_batch(oracle, rows, k, m, max_len, mode, seed, pats, alias)
    G = len(pats)
    nvoid = int((glen < 0).sum())
    t, table = vp.to_device(torch, DEV)
    dl, gl, inv = i32(lens), torch.full((G,), SENTINEL, dtype=torch.int32, device=DEV), counter()
    got = run(lambda: code.encode_ptrs_var(table, dl, max_len, gl, inv), t, stream)
    what = f"({k},{m}) max_len={max_len} G={G} {mode}"
    for g in range(G):
        for r in range(m):
            i = G * k + g * m + r
            n = max(int(glen[g]), 0)
            assert np.array_equal(vp.row(got, i, n), vp.row(expect, i, n)), f"{what}: parity ({g},{r}) [{pats[g][0]}]"
            assert np.array_equal(vp.row(got, i, max_len)[n:], vp.row(expect, i, max_len)[n:]), \
                f"{what}: parity ({g},{r}) written past L [{pats[g][0]}]"
    assert np.array_equal(got, expect), f"{what}: a byte outside [0, L) of the parity shards was written"
    assert np.array_equal(gl.cpu().numpy(), glen), f"{what}: d_group_len"
    assert int(inv.item()) == nvoid, what
    if not repeat:
        return
    # a second call adds to the counter and leaves the same bytes; then without counter and lengths
    code.encode_ptrs_var(table, dl, max_len, gl, inv)
    code.encode_ptrs_var(table, dl, max_len)
    torch.cuda.synchronize()
    assert int(inv.item()) == 2 * nvoid, what
    assert np.array_equal(t.cpu().numpy(), expect), what


def all_patterns(k, max_len):
    pats = pv.length_patterns(k, max_len) + pv.void_patterns(k, max_len)
    pv.assert_lengths_cover(pats, k, max_len)  # before the GPU is called: the test cannot pass by omission
    return pats


@pytest.mark.parametrize("mode", ALIGN)
@pytest.mark.parametrize("k,m", SHAPES, ids=[f"{k}-{m}" for k, m in SHAPES])
def test_encode_ptrs_var(oracle, k, m, mode):
    """One batch per max_len mixes: all lengths = max_len, all equal and short, the ladder 0, 1, 15, 16,
    17, ..., a staircase, one long shard and the rest empty, the short last group of a flush, an
    all-empty group, L on a column border and just past a wave border, and four void groups."""
    code = qa.Code.cauchy(k, m)
    for max_len in ENC_MAX:
        encode_case(oracle, code, code.rows, k, m, max_len, mode, 0x7A00 + 16 * k + max_len, all_patterns(k, max_len))


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m,max_len", [(10, 3, 1024), (16, 4, 1400), (9, 3, 1000)], ids=["10-3", "16-4", "9-3"])
def test_encode_ptrs_var_full_lengths_equal_the_fixed_call(oracle, k, m, max_len, mode):
    """All lengths = max_len: the whole pool equals the one qfec_encode_ptrs leaves."""
    code = qa.Code.cauchy(k, m)
    pats = [("full", np.full(k, max_len, np.int64))] * 5
    vp, lens, _, expect, _ = encode_batch(oracle, code.rows, k, m, max_len, mode, 0xF0 + k, pats)
    t1, table1 = vp.to_device(torch, DEV)
    t2, table2 = vp.to_device(torch, DEV)
    code.encode_ptrs_var(table1, i32(lens), max_len)
    code.encode_ptrs(table2, max_len)
    torch.cuda.synchronize()
    assert np.array_equal(t1.cpu().numpy(), t2.cpu().numpy())
    assert np.array_equal(t1.cpu().numpy(), expect)


def test_encode_ptrs_var_wide_code(oracle):
    """RS(60,8): k + m > 64, the addresses and lengths come from the tables where they are used."""
    k, m, max_len = 60, 8, 1040
    code = qa.Code.cauchy(k, m)
    for mode in ("aligned", "one-data"):
        encode_case(oracle, code, code.rows, k, m, max_len, mode, 0x6008, all_patterns(k, max_len))


@pytest.mark.parametrize("mode", ["aligned", "one-parity"])
def test_encode_ptrs_var_many_blocks(oracle, mode):
    """300 groups of RS(10,3) at max_len 1024: 75 blocks."""
    pats = all_patterns(10, 1024)
    pats = [pats[i % len(pats)] for i in range(300)]
    code = qa.Code.cauchy(10, 3)
    encode_case(oracle, code, code.rows, 10, 3, 1024, mode, 0x301, pats)


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m", [(10, 3), (16, 4), (9, 3)], ids=["10-3", "16-4", "9-3"])
def test_encode_ptrs_var_stale_row_quirk(oracle, k, m, mode):
    """rs.c's column-0 quirk on the vector bodies and the byte body: a flagged parity row starts from
    the bytes its shard held before, in [0, L) only."""
    rows = oracle.cauchy(k, m).copy()
    rows[1, 0] = 0
    code = qa.Code.from_rows(rows, rs_stale_quirk=True)
    for max_len in (17, 1000):
        encode_case(oracle, code, rows, k, m, max_len, mode, 0x5A1F + max_len + k, all_patterns(k, max_len), repeat=False)


@pytest.mark.parametrize("mode", ["aligned", "residues"])
def test_encode_ptrs_var_aliased_inputs(oracle, mode):
    """A data shard's address repeated in other groups with a shorter length: inputs may alias."""
    k, m, max_len = 10, 3, 1000
    code = qa.Code.cauchy(k, m)
    pats = all_patterns(k, max_len)
    names = [n for n, _ in pats]
    full, short, stairs = names.index("full"), names.index("short"), names.index("stairs")
    encode_case(oracle, code, code.rows, k, m, max_len, mode, 0xA11B, pats,
                alias={(short, 1): (full, 3), (stairs, 0): (full, 3)})


def test_encode_ptrs_var_on_a_stream(oracle):
    code = qa.Code.cauchy(10, 3)
    encode_case(oracle, code, code.rows, 10, 3, 1000, "one-data", 0x57D, all_patterns(10, 1000), stream=torch.cuda.Stream())


# ------------------------------------------------------------------ reconstruct

def recon_groups(k, m, max_len, full_only=False):
    """[(name, lens[k] true lengths, L, marks[k+m], invalid)]: every mark pattern of recon_marks under
    every length pattern, then the groups that must be invalid."""
    gm = pc.recon_marks(k, m)
    pc.assert_marks_cover(gm, k, m)
    pats = pv.length_patterns(k, max_len)
    pv.assert_lengths_cover(pats + pv.void_patterns(k, max_len), k, max_len)
    if full_only:
        pats = pats[:1]
    out = [(n, l.copy(), int(l.max()), q, False) for n, l in pats for q in gm]
    if full_only:
        return out
    short = dict(pats)["short"]
    one = gm[1]  # one erased data shard
    free = int(np.flatnonzero(one[:k] == 0)[0])
    assert one[:k].sum() == 1
    out.append(("L=-1", short.copy(), -1, one, True))
    out.append(("L=max_len+1", short.copy(), max_len + 1, one, True))
    for bad in (int(short.max()) + 1, -1):
        lens = short.copy()
        lens[free] = bad
        out.append((f"len={bad}", lens, int(short.max()), one, True))
    assert sum(1 for g in out if g[4]) == 4
    return out


def recon_batch(oracle, rows, k, m, max_len, mode, seed, groups):
    """(VarPool, device lens, L per group, marks, expected pool, nfail, ninvalid)."""
    G = len(groups)
    gm = np.stack([g[3] for g in groups]).astype(np.uint8)
    lens = np.stack([g[1] for g in groups]).astype(np.int64)
    L = np.array([g[2] for g in groups], np.int64)
    Lc = np.clip(L, 0, max_len)
    data = pc.batch_bytes(seed, G, k, max_len)
    par = pc.batch_bytes(seed + 1, G, m, max_len)  # not the encode of data: pins which survivors are read
    marked = gm[:, :k] == 1
    pdata = data.copy()
    pdata[marked] = 0x5A
    plens = np.where(marked, L[:, None], lens)  # a marked shard has room for L bytes
    vp = pv.VarPool(G, k, m, max_len, mode, seed + 2)
    vp.put_data(pdata, plens, keep=set(np.flatnonzero(marked.reshape(-1)).tolist()))
    vp.put_parity(par, Lc)
    expect = vp.clone_host()
    nfail = 0
    for g in range(G):
        if groups[g][4] or L[g] == 0:
            continue
        d = pv.zero_padded(pdata[g:g + 1], plens[g:g + 1])
        rc = oracle.rs_reconstruct(rows, d, par[g:g + 1].copy(), np.ascontiguousarray(gm[g]), int(L[g]))
        nfail += rc == -1
        for i in np.flatnonzero(marked[g]):
            s = vp.pool.start[g * k + i]
            expect[s:s + L[g]] = d[0, i, :L[g]]
    dl = np.where(marked, pv.INT_MIN, lens)  # the entries of marked shards are not looked at
    return vp, dl, L, marks_to_rs_layout(gm, k), expect, nfail, sum(1 for g in groups if g[4])


def reconstruct_case(oracle, code, rows, k, m, max_len, mode, seed, stream=None, repeat=True):
    groups = recon_groups(k, m, max_len)
    vp, dl, L, marks, expect, nfail, ninv = recon_batch(oracle, rows, k, m, max_len, mode, seed, groups)
    assert nfail > 0 and ninv == 4
    t, table = vp.to_device(torch, DEV)
    dl, gl, dm = i32(dl), i32(L), torch.from_numpy(marks).to(DEV)
    failed, inv = counter(), counter()
    got = run(lambda: code.reconstruct_ptrs_var(table, dl, gl, dm, max_len, failed, inv), t, stream)
    what = f"({k},{m}) max_len={max_len} {mode}"
    G = len(groups)
    for g in range(G):
        for i in range(k):
            r = g * k + i
            assert np.array_equal(vp.row(got, r, max_len), vp.row(expect, r, max_len)), \
                f"{what}: data ({g},{i}) [{groups[g][0]}, L={L[g]}, marks={groups[g][3].tolist()}]"
    assert np.array_equal(got, expect), f"{what}: a byte outside [0, L) of the marked data shards was written"
    assert int(failed.item()) == nfail and int(inv.item()) == ninv, what
    if not repeat:
        return
    # a second call adds to both counters (the survivors are unchanged, so are the results); then none
    code.reconstruct_ptrs_var(table, dl, gl, dm, max_len, failed, inv)
    code.reconstruct_ptrs_var(table, dl, gl, dm, max_len)
    torch.cuda.synchronize()
    assert int(failed.item()) == 2 * nfail and int(inv.item()) == 2 * ninv, what
    assert np.array_equal(t.cpu().numpy(), expect), what


@pytest.mark.parametrize("mode", ALIGN)
@pytest.mark.parametrize("k,m", SHAPES, ids=[f"{k}-{m}" for k, m in SHAPES])
def test_reconstruct_ptrs_var(oracle, k, m, mode):
    """Every mark pattern of ptrs_common.recon_marks under every length pattern; the d_lens entries of
    marked shards are INT_MIN; L = -1, L = max_len + 1, an unmarked shard of L + 1 and one of -1 are
    invalid and counted apart from the under-determined groups."""
    code = qa.Code.cauchy(k, m)
    for max_len in REC_MAX:
        reconstruct_case(oracle, code, code.rows, k, m, max_len, mode, 0x4ED0 + 16 * k + max_len)


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m", [(10, 3), (9, 3)], ids=["10-3", "9-3"])
def test_reconstruct_ptrs_var_stale_row_quirk(oracle, k, m, mode):
    rows = oracle.cauchy(k, m).copy()
    rows[1, 0] = 0
    code = qa.Code.from_rows(rows, rs_stale_quirk=True)
    for max_len in (17, 1000):
        reconstruct_case(oracle, code, rows, k, m, max_len, mode, 0x5A2F + max_len + k, repeat=False)


def test_reconstruct_ptrs_var_on_a_stream(oracle):
    code = qa.Code.cauchy(16, 4)
    reconstruct_case(oracle, code, code.rows, 16, 4, 1400, "one-parity", 0x57C, stream=torch.cuda.Stream())


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m,max_len", [(10, 3, 1000), (16, 4, 1400), (3, 2, 17)], ids=["10-3", "16-4", "3-2"])
def test_reconstruct_ptrs_var_full_lengths_equal_the_fixed_call(oracle, k, m, max_len, mode):
    """All lengths = max_len: the whole pool and the failed counter equal qfec_reconstruct_ptrs's."""
    code = qa.Code.cauchy(k, m)
    groups = recon_groups(k, m, max_len, full_only=True)
    vp, dl, L, marks, expect, nfail, ninv = recon_batch(oracle, code.rows, k, m, max_len, mode, 0xF1 + k, groups)
    assert ninv == 0 and (L == max_len).all()
    t1, table1 = vp.to_device(torch, DEV)
    t2, table2 = vp.to_device(torch, DEV)
    dm = torch.from_numpy(marks).to(DEV)
    f1, f2, inv = counter(), counter(), counter()
    code.reconstruct_ptrs_var(table1, i32(dl), i32(L), dm, max_len, f1, inv)
    code.reconstruct_ptrs(table2, dm, max_len, f2)
    torch.cuda.synchronize()
    assert np.array_equal(t1.cpu().numpy(), t2.cpu().numpy())
    assert np.array_equal(t1.cpu().numpy(), expect)
    assert int(f1.item()) == int(f2.item()) == nfail and int(inv.item()) == 0


# ------------------------------------------------------------------ round trip

@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m,max_len", [(10, 3, 1000), (16, 4, 1400), (4, 2, 17), (9, 3, 1040)],
                         ids=["10-3", "16-4", "4-2", "9-3"])
def test_round_trip(oracle, k, m, max_len, mode):
    """encode_var, drop up to m shards per group, reconstruct_var fed the encode's own d_group_len:
    every recovered shard equals the original in [0, len) and is zero in [len, L)."""
    code = qa.Code.cauchy(k, m)
    pats = all_patterns(k, max_len)
    G, n = len(pats), k + m
    gm = np.zeros((G, n), np.uint8)
    for g in range(G):
        gm[g, [(g + 3 * j) % n for j in range(g % (m + 1))]] = 1
    assert {int(x) for x in gm.sum(1)} == set(range(m + 1)) and gm[:, :k].any() and gm[:, k:].any()
    marked = gm[:, :k] == 1
    keep = set(np.flatnonzero(marked.reshape(-1)).tolist())  # a shard that will be rewritten has a slot of its own
    vp, lens, data, after_encode, glen = encode_batch(oracle, code.rows, k, m, max_len, mode, 0x7219 + k, pats, keep=keep)
    t, table = vp.to_device(torch, DEV)
    gl, inv = torch.full((G,), SENTINEL, dtype=torch.int32, device=DEV), counter()
    code.encode_ptrs_var(table, i32(lens), max_len, gl, inv)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), after_encode) and np.array_equal(gl.cpu().numpy(), glen)
    # the lost shards: their bytes are gone (0x5A over the room a receiver gives them, L bytes)
    lost = after_encode.copy()
    expect = after_encode.copy()
    padded = pv.zero_padded(data, lens)
    for g in range(G):
        L = int(glen[g])
        for i in np.flatnonzero(marked[g]):
            s = vp.pool.start[g * k + i]
            if L > 0:
                lost[s:s + L] = 0x5A
                expect[s:s + L] = padded[g, i, :L]
                assert not padded[g, i, lens[g, i]:L].any()
    t.copy_(torch.from_numpy(lost).to(DEV))
    dl = np.where(marked, pv.INT_MIN, lens)
    failed, inv = counter(), counter()
    code.reconstruct_ptrs_var(table, i32(dl), gl, torch.from_numpy(marks_to_rs_layout(gm, k)).to(DEV), max_len, failed, inv)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), expect)
    # the encode's -1 makes a void group invalid for the reconstruct as well, whatever its marks
    assert int(failed.item()) == 0 and int(inv.item()) == int((glen < 0).sum())
