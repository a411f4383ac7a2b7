"""GPU tests of edits to a LIVE reed_solomon handle: use -> edit rs->parity / rs->m -> use again.

Every per-code cache (handle_edits_common.CACHES: the encode tables, the three pattern LUTs, the
locate ratio tables, the locate2 constants, the host records of wide codes, the acceptance checks of
the plan families) is warmed by a call, the handle is edited, and the same call runs again on the
same buffers.  At every step

1. the output equals the CPU expectation for that step's matrices (the oracle's encode / reconstruct,
   dispatch_common, locate2_common, locate_wide_common, repair_common, wide_common), exactly;
2. where rs->m is [I; rows], the whole output buffers equal what a cold Code.from_rows twin of the
   step's rows writes on the same inputs;
3. the expectation differs from the previous step's (asserted on the expectations), so a table left
   over from the previous matrices cannot pass.

The locate families judge two batches with the same data and damage: A's parity is encoded with the
original rows, B's with the scaled ones, so a stale ratio or encode table changes a verdict whichever
way the edit goes.  One fresh handle per test; B = 100 at pitch 112 (16-byte path, masked tail) and at
pitch 100 (byte path).

Run on an MI355X:  python -m pytest tests/test_gpu_handle_edits.py -m gpu -q
"""
import collections
import ctypes as C
import types

import numpy as np
import pytest

import dispatch_common as dc
import handle_edits_common as he
import locate_wide_common as lw
import quicknet_amd as qa
from dispatch_common import Guarded, groups_for, written_from
from locate2_common import counts_of, expected_locate2
from quicknet_amd.synth import marks_to_rs_layout, synth_bytes
from repair_common import damage, expected_repair
from rs_abi_common import device_rows, fetch, knobs, ptr_array  # noqa: F401  (knobs is a fixture)
from wide_common import RECONSTRUCT, REPAIR, expected_plan

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
P112 = dc.Layout("pitch112", 100, 112, 0, 0, 0)  # 16-B kernels, 7 columns, a masked tail of 4 bytes
P100 = dc.Layout("pitch100", 100, 100, 0, 0, 0)  # the byte kernels by the pitch
assert not dc.byte_path(P112) and dc.byte_path(P100)
NARROW = [(8, 4), (6, 5)]  # an instance of every integrity family; the runtime-k,m kernels (m >= 4 for locate2)
WIDE = (26, 4)             # n > 24: host records, device plans, check plans
LAYOUT_IDS = {"pitch112": P112, "pitch100": P100}
FORMS = ("contig", "ptrs", "var")  # contiguous batches; a pointer table; a table with per-shard lengths


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ints(n):
    return torch.zeros(n, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------ the handle and its steps

Step = collections.namedtuple("Step", "name code rows full twin")


class Live:
    """One fresh handle; at(name) edits it and fetches its code again (handle_edits_common.step)."""

    def __init__(self, k, m):
        self.rs = qa.ReedSolomon(k, m)
        self.k, self.m = k, m
        self.p0, self.m0 = self.rs.parity.copy(), self.rs.m_matrix.copy()

    def at(self, name):
        if name == "original":
            code, rows, full = he.step(self.rs), self.rs.parity.copy(), self.rs.m_matrix.copy()
            assert np.array_equal(rows, self.p0) and np.array_equal(full, self.m0)
        else:
            code, rows, full = he.apply(self.rs, name, self.p0, self.m0)
        twin = qa.Code.from_rows(rows, rs_stale_quirk=True) if he.consistent(self.k, rows, full) else None
        return Step(name, code, rows, full, twin)


@pytest.fixture
def live():
    made = []

    def new(k, m):
        made.append(Live(k, m))
        return made[-1]

    yield new
    for h in made:
        h.rs.close()


def flat(x):
    if isinstance(x, (tuple, list)):
        return [y for e in x for y in flat(e)]
    return [np.asarray(x)]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def both(st, run, what):
    """run(code) -> host arrays, on the handle's code; where a twin models the handle, also on the
    twin, and every array (whole buffers) must be equal."""
    got = run(st.code)
    if st.twin is not None:
        for i, (a, b) in enumerate(zip(flat(got), flat(run(st.twin)))):
            assert np.array_equal(a, b), f"{what} at {st.name}: output {i} differs from the cold twin's"
    return got


def refused(call, text, bufs, before, what):
    """The call must raise QFEC_EUNSUP with `text`, and write nothing."""
    with pytest.raises(qa.QfecError) as e:
        call()
    torch.cuda.synchronize()
    assert "(-5)" in str(e.value) and text in str(e.value), f"{what}: {e.value}"
    for b, was in zip(bufs, before):
        b.check_guards(what)
        assert np.array_equal(b.host(), was), f"{what}: a refused call wrote"


# ------------------------------------------------------------------ batches

def ns(k, m, rows):
    """What repair_common.expected_repair reads of a code, from the step's rows."""
    return types.SimpleNamespace(k=k, m=m, rows=np.ascontiguousarray(rows))


def data_of(k, m, layout):
    G = groups_for(k, m)
    return synth_bytes(0xED17 + k * 3 + m, G * k * layout.pitch).reshape(G, k, layout.pitch).copy()


def garbage_parity(k, m, layout, seed=0):
    G = groups_for(k, m)
    return synth_bytes(0x0DD + k * 5 + m + seed, G * m * layout.pitch).reshape(G, m, layout.pitch).copy()


def encoded(oracle, rows, data, layout):
    """Parity of `rows` over [0, B), garbage in [B, pitch)."""
    k, m = data.shape[1], rows.shape[0]
    par = garbage_parity(k, m, layout)
    par[..., :layout.B] = dc.oracle_parity(oracle, rows, data, layout.B)
    return par


def two_batches(oracle, h, layout, hurt):
    """[(data, parity)] A and B: the same data and the same damage (hurt(data, parity) in place), parity
    from the original rows and from the scaled rows.  -> (batches, what hurt returned on A)"""
    out, made = [], None
    for rows in (h.p0, he.scaled_rows(h.p0)):
        d = data_of(h.k, h.m, layout)
        p = encoded(oracle, rows, d, layout)
        r = hurt(d, p)
        made = r if made is None else made
        out.append((d, p))
    return out, made


def table(dt, pt):
    """The pointer table of contiguous device batches: every group's data rows, then every group's
    parity rows, each shard exactly B bytes of its pitch-wide row."""
    G, k, pitch = dt.shape
    m = pt.shape[1]
    a = np.concatenate([dt.data_ptr() + np.arange(G * k, dtype=np.int64) * pitch,
                        pt.data_ptr() + np.arange(G * m, dtype=np.int64) * pitch])
    return dev(a)


def lens_of(G, k, B):
    """(lens [G * k], group_len [G]) of the calls with per-shard lengths: every shard B bytes long.  What
    differing lengths do is the subject of the families' own tests; here the calls must read the tables
    of the handle's current matrices, like their fixed-length forms."""
    return dev(np.full(G * k, B, np.int32)), dev(np.full(G, B, np.int32))


def wf_of(layout, ptrs):
    """The first byte of a row a call may not write: a shard on a table is exactly B bytes."""
    return layout.B if ptrs else written_from(layout)


def held(buf, before, what):
    buf.check_guards(what)
    assert np.array_equal(buf.host(), before), f"{what}: a read-only buffer was written"


def written(got, want_b, before, layout, ptrs, what):
    """[0, B) equals the expectation; nothing from the write limit on moved."""
    B, wf = layout.B, wf_of(layout, ptrs)
    assert np.array_equal(got[..., :B], want_b[..., :B]), f"{what}: wrong bytes"
    assert np.array_equal(got[..., wf:], before[..., wf:]), f"{what}: bytes beyond the block written"


# ------------------------------------------------------------------ encode side

def check_encode(oracle, st, layout, form, data):
    """form: contig / ptrs / var."""
    G, k, m = data.shape[0], data.shape[1], st.rows.shape[0]
    ptrs = form != "contig"
    p_in = garbage_parity(k, m, layout, 7)
    want = p_in.copy()
    oracle.rs_encode(st.rows, data, want, layout.B)  # a stale row keeps its old bytes where column 0 contributes

    def run(code):
        dd, dp = Guarded(data), Guarded(p_in)
        if form == "var":
            lens, glen = lens_of(G, k, layout.B)
            out_len, invalid = ints(G), ints(1)
            code.encode_ptrs_var(table(dd.t, dp.t), lens, layout.B, group_len=out_len, invalid=invalid)
            assert np.array_equal(out_len.cpu().numpy(), glen.cpu().numpy()) and int(invalid.item()) == 0
        elif form == "ptrs":
            code.encode_ptrs(table(dd.t, dp.t), layout.B)
        else:
            code.encode(dd.t, dp.t, layout.B)
        torch.cuda.synchronize()
        held(dd, data, "encode data")
        dp.check_guards("encode parity")
        return dp.host()

    written(both(st, run, f"encode-{form}"), want, p_in, layout, ptrs, f"encode-{form} at {st.name}")
    return want[..., :layout.B]


def check_verify(oracle, st, layout, form, batches):
    wants = []
    for tag, (d, p) in zip("AB", batches):
        want = dc.bad_rows_model(oracle, st.rows, d, p, layout.B)

        def run(code):
            dd, dp = Guarded(d), Guarded(p)
            count = ints(1)
            if form == "var":
                lens, glen = lens_of(len(d), d.shape[1], layout.B)
                invalid = ints(1)
                bad = code.verify_ptrs_var(table(dd.t, dp.t), lens, glen, layout.B, bad_groups=count, invalid=invalid)
                assert int(invalid.item()) == 0
            elif form == "ptrs":
                bad = code.verify_ptrs(table(dd.t, dp.t), layout.B, bad_groups=count)
            else:
                bad = code.verify(dd.t, dp.t, layout.B, bad_groups=count)
            torch.cuda.synchronize()
            held(dd, d, "verify data")
            held(dp, p, "verify parity")
            return bad.cpu().numpy().view(np.uint32), int(count.item())

        got, count = both(st, run, f"verify-{form}")
        assert np.array_equal(got, want), f"verify-{form} {tag} at {st.name}"
        assert count == int((want != 0).sum())
        wants.append(want)
    return wants


def check_update(oracle, st, layout, form, data):
    """qfec_update (form contig), qfec_update_ptrs (ptrs), qfec_update_ptrs_var (var) on a batch consistent
    under the step's rows: the new parity is the oracle's encode of the new data in every touched group."""
    ptrs = form != "contig"
    G, k, pitch = data.shape
    m, B = st.rows.shape[0], layout.B
    par = encoded(oracle, st.rows, data, layout)
    ids = dc.update_ids(k, G)
    new = synth_bytes(0x0FD + k, G * pitch).reshape(G, pitch).copy()
    want_d = dc.apply_rows(data, ids, new, B)
    want_p = par.copy()
    on = ids >= 0
    want_p[on, :, :B] = dc.oracle_parity(oracle, st.rows, want_d, B)[on]

    def run(code):
        dd, dp, dn = Guarded(data), Guarded(par), Guarded(new)
        invalid = ints(1)
        if ptrs:
            new_at = dev(dn.t.data_ptr() + np.arange(G, dtype=np.int64) * pitch)
            if form == "var":
                lens, glen = lens_of(G, k, B)
                code.update_ptrs_var(table(dd.t, dp.t), lens, glen, dev(ids), new_at, dev(np.full(G, B, np.int32)), B,
                                     invalid=invalid)
            else:
                code.update_ptrs(table(dd.t, dp.t), dev(ids), new_at, B, invalid=invalid)
        else:
            code.update(dev(ids), dn.t, dp.t, data=dd.t, block_size=B, invalid=invalid)
        torch.cuda.synchronize()
        held(dn, new, "update rows")
        dd.check_guards("update data")
        dp.check_guards("update parity")
        assert int(invalid.item()) == 0
        return dd.host(), dp.host()

    got_d, got_p = both(st, run, f"update-{form}")
    written(got_d, want_d, data, layout, ptrs, f"update-{form} data at {st.name}")
    written(got_p, want_p, par, layout, ptrs, f"update-{form} parity at {st.name}")
    assert np.array_equal(got_p[~on], par[~on]) and np.array_equal(got_d[~on], data[~on])
    return want_p[..., :B]


def check_encode_update(oracle, st, layout, form, data):
    """parity ^= rows[:, 1 : k - 1] x data[:, 1 : k - 1] on garbage parity."""
    ptrs = form != "contig"
    G, k, pitch = data.shape
    m, B = st.rows.shape[0], layout.B
    first, count = 1, k - 2
    part = np.ascontiguousarray(data[:, first:first + count])
    p_in = garbage_parity(k, m, layout, 11)
    want = p_in.copy()
    want[..., :B] ^= dc.oracle_parity(oracle, np.ascontiguousarray(st.rows[:, first:first + count]), part, B)

    def run(code):
        dp = Guarded(p_in)
        if ptrs:
            dd = Guarded(data)
            if form == "var":
                lens, glen = lens_of(G, k, B)
                invalid = ints(1)
                code.encode_update_ptrs_var(table(dd.t, dp.t), first, count, lens, glen, B, accumulate=True, invalid=invalid)
                assert int(invalid.item()) == 0
            else:
                code.encode_update_ptrs(table(dd.t, dp.t), first, count, B, accumulate=True)
        else:
            dd = Guarded(part)
            code.encode_update(dd.t, dp.t, first, B, accumulate=True)
        torch.cuda.synchronize()
        held(dd, data if ptrs else part, "encode_update data")
        dp.check_guards("encode_update parity")
        return dp.host()

    written(both(st, run, f"encode_update-{form}"), want, p_in, layout, ptrs, f"encode_update-{form} at {st.name}")
    return want[..., :B]


@pytest.mark.parametrize("lname", sorted(LAYOUT_IDS))
@pytest.mark.parametrize("k,m", NARROW + [WIDE], ids=lambda v: str(v))
def test_encode_side(oracle, live, k, m, lname):
    """enc_version.  encode, verify, update, encode_update, contiguous, on a pointer table and on one with
    per-shard lengths, follow rs->parity: original -> scaled -> zero_col0 (the encode paths only, against the
    oracle's encode over stale parity, as the cold tests assert) -> restore."""
    layout = LAYOUT_IDS[lname]
    h = live(k, m)
    data = data_of(k, m, layout)
    batches, _ = two_batches(oracle, h, layout, lambda d, p: dc.damage_every_shard(d, p, layout.B))

    def check(st):
        out = [check_encode(oracle, st, layout, form, data) for form in FORMS][:1]
        if st.name != "zero_col0":
            out += [check_verify(oracle, st, layout, form, batches) for form in FORMS][0]
            out += [check_update(oracle, st, layout, form, data) for form in FORMS][:1]
            out += [check_encode_update(oracle, st, layout, form, data) for form in FORMS][:1]
        return out[0] if st.name == "zero_col0" else out

    seen = {}
    for name in ("original", "scaled", "zero_col0", "restore"):
        st = h.at(name)
        seen[name] = flat(check(st))
    assert not same(seen["original"], seen["scaled"]) and same(seen["original"], seen["restore"])
    assert not same(seen["zero_col0"], seen["scaled"][:1]) and not same(seen["zero_col0"], seen["restore"][:1])


# ------------------------------------------------------------------ reconstruct and repair

def marks_for(k, m):
    """[G, n] group-order marks, fixed per shape: nothing; every erased-data count 1 .. m; a parity
    row alone; m + 1 data rows (under-determined); exactly m over data and parity; e data rows beside
    parity row 0 (the survivors then start at parity row 1; under-determined at e = m); then random
    groups of 0 .. m + 1 marks."""
    n, G = k + m, groups_for(k, m)
    rng = np.random.default_rng(97 * k + m)
    pats = [[]] + [list(rng.choice(k, e, replace=False)) for e in range(1, m + 1)]
    pats += [[k], list(range(m + 1)), list(range(k - (m + 1) // 2, k + m - (m + 1) // 2))]
    pats += [list(rng.choice(k, e, replace=False)) + [k] for e in range(1, m + 1)]
    assert len(pats) < G and max(map(len, pats)) == m + 1 <= k
    gm = np.zeros((G, n), np.uint8)
    for g in range(G):
        gm[g, pats[g] if g < len(pats) else rng.choice(n, int(rng.integers(0, m + 2)), replace=False)] = 1
    return gm


def fixed_batches(oracle, h, layout):
    """[(data, parity)] A and B for the decoders: the same data, parity from the original and from the
    scaled rows.  Whatever the handle holds, one of them is not what its matrix would have sent, so
    its decode differs from step to step."""
    return two_batches(oracle, h, layout, lambda d, p: None)[0]


def check_reconstruct(oracle, st, layout, form, batches, gm):
    """form: contig / ptrs / var.  The oracle's rs.c reconstruct with the whole rs->m of the step."""
    B = layout.B
    wants = []
    for tag, (data, par) in zip("AB", batches):
        G, k, pitch = data.shape
        m = par.shape[1]
        d_in, p_in = damage(data, par, gm)
        marks = marks_to_rs_layout(gm, k)
        want = d_in.copy()
        oracle.rs_reconstruct_full(st.full, want, p_in.copy(), marks, B)
        bad = gm[:, :k].sum(1) > m - gm[:, k:].sum(1)
        assert bad.any() and not bad.all()

        def run(code):
            dd, dp = Guarded(d_in), Guarded(p_in)
            failed = ints(1)
            if form == "var":
                lens, glen = lens_of(G, k, B)
                invalid = ints(1)
                code.reconstruct_ptrs_var(table(dd.t, dp.t), lens, glen, dev(marks), B, failed=failed, invalid=invalid)
                assert int(invalid.item()) == 0
            elif form == "ptrs":
                code.reconstruct_ptrs(table(dd.t, dp.t), dev(marks), B, failed=failed)
            else:
                code.reconstruct(dd.t, dp.t, dev(marks), B, failed=failed)
            torch.cuda.synchronize()
            held(dp, p_in, "reconstruct parity")
            dd.check_guards("reconstruct data")
            return dd.host(), int(failed.item())

        got, failed = both(st, run, f"reconstruct-{form} {tag}")
        what = f"reconstruct-{form} {tag} at {st.name}"
        written(got, want, d_in, layout, form != "contig", what)
        assert np.array_equal(got[gm[:, :k] == 0], d_in[gm[:, :k] == 0]), what + ": an unmarked row was written"
        assert failed == int(bad.sum()), what
        wants.append(want[..., :B])
    return wants


def heals(want, batches, gm, which):
    """Does the expectation of batch `which` hold the original data in every recoverable group?"""
    data = batches[which][0]
    k, m = data.shape[1], gm.shape[1] - data.shape[1]
    ok = gm[:, :k].sum(1) <= m - gm[:, k:].sum(1)
    return np.array_equal(want[which][ok], data[ok][..., :want[which].shape[-1]])


@pytest.mark.parametrize("lname", sorted(LAYOUT_IDS))
@pytest.mark.parametrize("k,m", NARROW + [WIDE], ids=lambda v: str(v))
def test_reconstruct(oracle, live, k, m, lname):
    """dec.version (n <= 24: the reconstruct LUT, read by qfec_reconstruct, qfec_reconstruct_ptrs and _ptrs_var) and
    rec_cache_version ((26,4): the host records).  Batch A decodes to the original data under the
    original matrix, batch B under the scaled one.  original -> scaled -> parity_only (rs->m is the
    original again: the decode must be the original one while rs->parity is not) -> restore."""
    layout = LAYOUT_IDS[lname]
    h = live(k, m)
    batches, gm = fixed_batches(oracle, h, layout), marks_for(k, m)
    forms = ("contig",) if k + m > 24 else FORMS

    def check(st):
        out = [check_reconstruct(oracle, st, layout, f, batches, gm) for f in forms]
        assert all(same(out[0], o) for o in out)
        return out[0]

    seen = [check(h.at(name)) for name in ("original", "scaled", "parity_only", "restore")]
    assert heals(seen[0], batches, gm, 0) and not heals(seen[0], batches, gm, 1)
    assert heals(seen[1], batches, gm, 1) and not heals(seen[1], batches, gm, 0)
    assert not same(seen[1], seen[2]) and same(seen[2], seen[0]) and same(seen[3], seen[0])


def check_repair(oracle, st, layout, batches, gm):
    B = layout.B
    wants = []
    for tag, (data, par) in zip("AB", batches):
        G, k, pitch = data.shape
        m = par.shape[1]
        d_in, p_in = damage(data, par, gm)
        want_d, want_p, nfail = expected_repair(oracle, ns(k, m, st.rows), "cauchy", d_in, p_in, gm, B)
        ok = gm.sum(1) <= m

        def run(code):
            dd, dp = Guarded(d_in), Guarded(p_in)
            failed = ints(1)
            code.repair(dd.t, dp.t, dev(marks_to_rs_layout(gm, k)), B, failed=failed)
            torch.cuda.synchronize()
            dd.check_guards("repair data")
            dp.check_guards("repair parity")
            return dd.host(), dp.host(), int(failed.item())

        got_d, got_p, failed = both(st, run, f"repair {tag}")
        what = f"repair {tag} at {st.name}"
        written(got_d, want_d, d_in, layout, False, what + " data")
        written(got_p, want_p, p_in, layout, False, what + " parity")
        assert np.array_equal(got_d[gm[:, :k] == 0], d_in[gm[:, :k] == 0]), what
        assert np.array_equal(got_p[gm[:, k:] == 0], p_in[gm[:, k:] == 0]), what
        assert failed == nfail == int((~ok).sum()) > 0, what
        wants += [want_d[..., :B], want_p[..., :B]]
    return wants


@pytest.mark.parametrize("lname", sorted(LAYOUT_IDS))
@pytest.mark.parametrize("k,m", NARROW, ids=lambda v: str(v))
def test_repair(oracle, live, k, m, lname):
    """rep.version: qfec_repair's LUT and records, on the two batches.  original -> scaled -> restore."""
    layout = LAYOUT_IDS[lname]
    h = live(k, m)
    batches, gm = fixed_batches(oracle, h, layout), marks_for(k, m)
    ok = gm.sum(1) <= m
    seen = [check_repair(oracle, h.at(name), layout, batches, gm) for name in ("original", "scaled", "restore")]
    assert not same(seen[0], seen[1]) and same(seen[2], seen[0])
    for step, which in ((0, 0), (1, 1)):  # the batch the handle's rows encoded comes back whole
        d, p = batches[which]
        assert np.array_equal(seen[step][2 * which][ok], d[ok][..., :layout.B])
        assert np.array_equal(seen[step][2 * which + 1][ok], p[ok][..., :layout.B])


# ------------------------------------------------------------------ locate / scrub

def check_locate(oracle, st, layout, form, batches):
    """form: contig / ptrs / var.  culprit, marks, counts by dispatch_common.expected_locate1 on both batches;
    the scrub rewrites every located shard as a repair with those marks would."""
    B = layout.B
    wants = []
    for tag, (d, p) in zip("AB", batches):
        G, k = d.shape[:2]
        m = p.shape[1]
        want = dc.expected_locate1(oracle, st.rows, d, p, B)
        want_gm = dc.marks_n(want, k + m)
        want_d, want_p, _ = expected_repair(oracle, ns(k, m, st.rows), "cauchy", d, p, want_gm, B)

        def run(code):
            dd, dp = Guarded(d), Guarded(p)
            culprit, counts = ints(G), ints(3)
            marks = dev(np.full(G * (k + m), 0xEE, np.uint8))
            invalid = ints(1)
            if form != "contig":
                t = table(dd.t, dp.t)
                lens, glen = lens_of(G, k, B)
            if form == "var":
                code.locate_ptrs_var(t, lens, glen, B, culprit=culprit, marks=marks, counts=counts, invalid=invalid)
            elif form == "ptrs":
                code.locate_ptrs(t, B, culprit=culprit, marks=marks, counts=counts)
            else:
                code.locate(dd.t, dp.t, B, culprit=culprit, marks=marks, counts=counts)
            torch.cuda.synchronize()
            held(dd, d, "locate data")
            held(dp, p, "locate parity")
            out = [culprit.cpu().numpy(), marks.cpu().numpy(), counts.cpu().numpy()]
            counts2 = ints(3)
            if form == "var":
                got2 = code.scrub_ptrs_var(t, lens, glen, B, counts=counts2, invalid=invalid)
            elif form == "ptrs":
                got2 = code.scrub_ptrs(t, B, counts=counts2)
            else:
                got2 = code.scrub(dd.t, dp.t, B, counts=counts2)
            torch.cuda.synchronize()
            assert int(invalid.item()) == 0
            dd.check_guards("scrub data")
            dp.check_guards("scrub parity")
            return out + [got2.cpu().numpy(), counts2.cpu().numpy(), dd.host(), dp.host()]

        culprit, marks, counts, culprit2, counts2, got_d, got_p = both(st, run, f"locate-{form} {tag}")
        what = f"locate-{form} {tag} at {st.name}"
        assert np.array_equal(culprit, want) and np.array_equal(culprit2, want), what
        assert np.array_equal(marks, marks_to_rs_layout(want_gm, k)), what
        assert list(counts) == dc.counts_of1(want) == list(counts2), what
        written(got_d, want_d, d, layout, form != "contig", what + " scrub data")
        written(got_p, want_p, p, layout, form != "contig", what + " scrub parity")
        assert np.array_equal(got_d[want_gm[:, :k] == 0], d[want_gm[:, :k] == 0]), what
        assert np.array_equal(got_p[want_gm[:, k:] == 0], p[want_gm[:, k:] == 0]), what
        wants.append(want)
    return wants


def locate_refused(st, layout, d, p, calls):
    """zero_col0: every locate entry refuses with locate_code_check's text and writes nothing."""
    G, k = d.shape[:2]
    for name, call in calls.items():
        dd, dp = Guarded(d), Guarded(p)
        refused(lambda: call(st.code, dd, dp), he.EUNSUP_ZERO, (dd, dp), (d, p), f"{name} at {st.name}")


@pytest.mark.parametrize("lname", sorted(LAYOUT_IDS))
@pytest.mark.parametrize("k,m", NARROW, ids=lambda v: str(v))
def test_locate(oracle, live, k, m, lname):
    """loc_version (the ratio tables), enc_version (the syndromes) and rep.version (the scrub's repair):
    qfec_locate / qfec_scrub and their forms on a pointer table, with and without per-shard lengths.  Under the original code batch A names its
    culprits and batch B is what the model says; under the scaled code it is the reverse.  zero_col0:
    refused.  original -> scaled -> zero_col0 -> restore."""
    layout = LAYOUT_IDS[lname]
    B = layout.B
    h = live(k, m)
    batches, made = two_batches(oracle, h, layout, lambda d, p: dc.damage_every_shard(d, p, B))
    seen = []
    for name in ("original", "scaled", "zero_col0", "restore"):
        st = h.at(name)
        if name == "zero_col0":
            locate_refused(st, layout, *batches[0], {
                "locate": lambda c, dd, dp: c.locate(dd.t, dp.t, B),
                "scrub": lambda c, dd, dp: c.scrub(dd.t, dp.t, B),
                "locate_ptrs": lambda c, dd, dp: c.locate_ptrs(table(dd.t, dp.t), B),
                "scrub_ptrs": lambda c, dd, dp: c.scrub_ptrs(table(dd.t, dp.t), B),
                "locate_ptrs_var": lambda c, dd, dp: c.locate_ptrs_var(table(dd.t, dp.t), *lens_of(len(dd.t), k, B), B),
                "scrub_ptrs_var": lambda c, dd, dp: c.scrub_ptrs_var(table(dd.t, dp.t), *lens_of(len(dd.t), k, B), B)})
            continue
        want = [check_locate(oracle, st, layout, form, batches) for form in FORMS][0]
        seen.append(flat(want))
    a, b = seen[0]
    assert np.array_equal(a, made) and not np.array_equal(b, made) and (b == dc.MULTI).sum() > len(b) // 2
    assert np.array_equal(seen[1][1], made) and not np.array_equal(seen[1][0], made)  # the reverse
    assert same(seen[2], seen[0])


def check_locate2(oracle, st, layout, batches):
    B = layout.B
    wants = []
    for tag, (d, p) in zip("AB", batches):
        G, k = d.shape[:2]
        m = p.shape[1]
        want = expected_locate2(oracle, st.rows, "cauchy", d, p, B)
        want_gm = dc.marks_n(want, k + m)
        want_d, want_p, _ = expected_repair(oracle, ns(k, m, st.rows), "cauchy", d, p, want_gm, B)

        def run(code):
            dd, dp = Guarded(d), Guarded(p)
            culprit, counts = torch.zeros((G, 2), dtype=torch.int32, device=DEV), ints(4)
            marks = dev(np.full(G * (k + m), 0xEE, np.uint8))
            code.locate2(dd.t, dp.t, B, culprit=culprit, marks=marks, counts=counts)
            torch.cuda.synchronize()
            held(dd, d, "locate2 data")
            held(dp, p, "locate2 parity")
            out = [culprit.cpu().numpy(), marks.cpu().numpy(), counts.cpu().numpy()]
            counts2 = ints(4)
            got2 = code.scrub2(dd.t, dp.t, B, counts=counts2)
            torch.cuda.synchronize()
            dd.check_guards("scrub2 data")
            dp.check_guards("scrub2 parity")
            return out + [got2.cpu().numpy(), counts2.cpu().numpy(), dd.host(), dp.host()]

        culprit, marks, counts, culprit2, counts2, got_d, got_p = both(st, run, f"locate2 {tag}")
        what = f"locate2 {tag} at {st.name}"
        assert np.array_equal(culprit, want) and np.array_equal(culprit2, want), what
        assert np.array_equal(marks, marks_to_rs_layout(want_gm, k)), what
        assert list(counts) == counts_of(want) == list(counts2), what
        written(got_d, want_d, d, layout, False, what + " scrub2 data")
        written(got_p, want_p, p, layout, False, what + " scrub2 parity")
        assert np.array_equal(got_d[want_gm[:, :k] == 0], d[want_gm[:, :k] == 0]), what
        assert np.array_equal(got_p[want_gm[:, k:] == 0], p[want_gm[:, k:] == 0]), what
        wants.append(want)
    return wants


@pytest.mark.parametrize("lname", sorted(LAYOUT_IDS))
@pytest.mark.parametrize("k,m", NARROW, ids=lambda v: str(v))
def test_locate2(oracle, live, k, m, lname):
    """l2_host_version (the checks of every pair, built on the host) and loc2_version (their device
    copy): qfec_locate2 / qfec_scrub2 on the two batches.  original -> scaled -> zero_col0 (refused)
    -> restore."""
    layout = LAYOUT_IDS[lname]
    B = layout.B
    h = live(k, m)
    batches, made = two_batches(oracle, h, layout, lambda d, p: dc.locate2_damage(d, p, B))
    seen = []
    for name in ("original", "scaled", "zero_col0", "restore"):
        st = h.at(name)
        if name == "zero_col0":
            locate_refused(st, layout, *batches[0], {"locate2": lambda c, dd, dp: c.locate2(dd.t, dp.t, B),
                                                     "scrub2": lambda c, dd, dp: c.scrub2(dd.t, dp.t, B)})
            continue
        seen.append(flat(check_locate2(oracle, st, layout, batches)))
    for g, slots in made:  # the consistent batch names what was damaged
        assert tuple(seen[0][0][g]) == tuple(slots) == tuple(seen[1][1][g])
    assert not same(seen[0], seen[1]) and same(seen[2], seen[0])
    assert not np.array_equal(seen[0][0], seen[0][1]) and not np.array_equal(seen[1][0], seen[1][1])


def erased_marks_after(gm, culprit, scrub):
    """Group-order marks of marks_out: the input marks as 0 / 1 plus the located culprit; a scrub
    leaves MULTI / AMBIGUOUS groups unmarked."""
    out = dc.erased_marks(gm, culprit)
    if scrub:
        out[(culprit == lw.MULTI) | (culprit == lw.AMBIGUOUS)] = 0
    return out


def check_erased(oracle, st, layout, batches, gm, entry="erased"):
    """qfec_locate_erased / qfec_scrub_erased (entry erased) or qfec_locate_wide / qfec_scrub_wide (entry
    wide; wide-ptrs on a table; wide-var on a table with per-shard lengths) against locate_wide_common.model over a cold code of the step's rows."""
    B = layout.B
    cold = qa.Code.from_rows(st.rows, rs_stale_quirk=True)
    wants = []
    for tag, (d, p) in zip("AB", batches):
        G, k = d.shape[:2]
        m = p.shape[1]
        want, want_marks, want_counts = lw.model(cold, d, p, gm, B)
        scrub_gm = erased_marks_after(gm, want, True)
        scrub_gm[want == lw.LOST] = 0
        want_d, want_p, _ = expected_repair(oracle, ns(k, m, st.rows), "cauchy", d, p, scrub_gm, B)
        marks_in = marks_to_rs_layout(gm, k)

        def run(code):
            dd, dp = Guarded(d), Guarded(p)
            culprit, counts = ints(G), ints(5)
            marks, out = dev(marks_in), dev(np.full(G * (k + m), 0xEE, np.uint8))
            counts2, failed = ints(5), ints(1)
            if entry == "erased":
                code.locate_erased(dd.t, dp.t, marks, B, culprit=culprit, marks_out=out, counts=counts)
            elif entry == "wide":
                code.locate_wide(dd.t, dp.t, marks, B, culprit=culprit, marks_out=out, counts=counts)
            elif entry == "wide-ptrs":
                t = table(dd.t, dp.t)
                code.locate_ptrs_wide(t, B, marks=marks, culprit=culprit, marks_out=out, counts=counts)
            else:
                t = table(dd.t, dp.t)
                lens, glen = lens_of(G, k, B)
                invalid = ints(1)
                code.locate_ptrs_wide_var(t, lens, glen, B, marks=marks, culprit=culprit, marks_out=out, counts=counts,
                                          invalid=invalid)
            torch.cuda.synchronize()
            held(dd, d, "locate data")
            held(dp, p, "locate parity")
            res = [culprit.cpu().numpy(), out.cpu().numpy(), counts.cpu().numpy()]
            if entry == "erased":
                got2 = code.scrub_erased(dd.t, dp.t, marks, B, counts=counts2, failed=failed)
            elif entry == "wide":
                got2 = code.scrub_wide(dd.t, dp.t, marks, B, counts=counts2, failed=failed)
            elif entry == "wide-ptrs":
                got2 = code.scrub_ptrs_wide(t, B, marks=marks, counts=counts2, failed=failed)
            else:
                got2 = code.scrub_ptrs_wide_var(t, lens, glen, B, marks=marks, counts=counts2, failed=failed, invalid=invalid)
                assert int(invalid.item()) == 0
            torch.cuda.synchronize()
            dd.check_guards("scrub data")
            dp.check_guards("scrub parity")
            assert np.array_equal(marks.cpu().numpy(), marks_in)
            return res + [got2.cpu().numpy(), counts2.cpu().numpy(), int(failed.item()), dd.host(), dp.host()]

        culprit, out, counts, culprit2, counts2, failed, got_d, got_p = both(st, run, f"locate-{entry} {tag}")
        what = f"locate-{entry} {tag} at {st.name}"
        assert np.array_equal(culprit, want) and np.array_equal(culprit2, want), what
        assert np.array_equal(out, want_marks), what
        assert list(counts) == list(want_counts) == list(counts2), what
        assert failed == int((want == lw.LOST).sum()) == 0
        ptrs = entry in ("wide-ptrs", "wide-var")
        written(got_d, want_d, d, layout, ptrs, what + " scrub data")
        written(got_p, want_p, p, layout, ptrs, what + " scrub parity")
        assert np.array_equal(got_d[scrub_gm[:, :k] == 0], d[scrub_gm[:, :k] == 0]), what
        assert np.array_equal(got_p[scrub_gm[:, k:] == 0], p[scrub_gm[:, k:] == 0]), what
        wants.append(want)
    return wants


def erased_batches(oracle, h, layout):
    """(batches A and B, marks gm, culprits by construction on the consistent batch)"""
    batches, made = two_batches(oracle, h, layout, lambda d, p: dc.erased_damage(d, p, layout.B, 31 * h.k + h.m))
    return batches, made[0], made[1]


@pytest.mark.parametrize("lname", sorted(LAYOUT_IDS))
@pytest.mark.parametrize("k,m", NARROW, ids=lambda v: str(v))
def test_locate_erased(oracle, live, k, m, lname):
    """le_host_version (the records of every mask, built on the host) and le.version (the device LUT):
    qfec_locate_erased / qfec_scrub_erased on the two batches, beside lost shards.  The consistent batch
    gives the culprits by construction.  original -> scaled -> zero_col0 (refused) -> restore."""
    layout = LAYOUT_IDS[lname]
    B = layout.B
    h = live(k, m)
    batches, gm, made = erased_batches(oracle, h, layout)
    marks = marks_to_rs_layout(gm, k)
    seen = []
    for name in ("original", "scaled", "zero_col0", "restore"):
        st = h.at(name)
        if name == "zero_col0":
            locate_refused(st, layout, *batches[0], {
                "locate_erased": lambda c, dd, dp: c.locate_erased(dd.t, dp.t, dev(marks), B),
                "scrub_erased": lambda c, dd, dp: c.scrub_erased(dd.t, dp.t, dev(marks), B)})
            continue
        seen.append(flat(check_erased(oracle, st, layout, batches, gm)))
    assert np.array_equal(seen[0][0], made) and np.array_equal(seen[1][1], made)
    assert not np.array_equal(seen[0][1], made) and not np.array_equal(seen[1][0], made)
    assert same(seen[2], seen[0])


# ------------------------------------------------------------------ device plans at (26,4)

ONE_SHOTS = ("repair_wide", "reconstruct_wide", "repair_ptrs_wide", "reconstruct_ptrs_wide", "repair_ptrs_wide_var",
             "reconstruct_ptrs_wide_var")


def check_plans(oracle, st, layout, data, gm):
    """plan_build against wide_common.expected_plan over a cold code of the step's rows; plan_apply in
    its three forms, repair_wide, reconstruct_wide and the one-shots on a table (ONE_SHOTS) against the
    oracle."""
    G, k, pitch = data.shape
    m, B = st.rows.shape[0], layout.B
    cold = qa.Code.from_rows(st.rows, rs_stale_quirk=True)
    par = encoded(oracle, st.rows, data, layout)
    d_in, p_in = damage(data, par, gm)
    marks = marks_to_rs_layout(gm, k)
    rep_d, rep_p, nfail = expected_repair(oracle, ns(k, m, st.rows), "cauchy", d_in, p_in, gm, B)
    rec_d = d_in.copy()
    oracle.rs_reconstruct_full(st.full, rec_d, p_in.copy(), marks, B)
    rec_bad = int((gm[:, :k].sum(1) > m - gm[:, k:].sum(1)).sum())
    want_plans = {mode: np.stack([expected_plan(cold, gm[g], mode, True) for g in range(G)]) for mode in (REPAIR, RECONSTRUCT)}

    def run(code):
        out = []
        for mode in (REPAIR, RECONSTRUCT):
            failed = ints(1)
            plan = code.plan_build(dev(marks), mode, failed=failed)
            torch.cuda.synchronize()
            out += [plan.cpu().numpy(), int(failed.item())]
            for form in FORMS:
                dd, dp = Guarded(d_in), Guarded(p_in)
                if form == "var":
                    invalid = ints(1)
                    code.plan_apply_ptrs_var(table(dd.t, dp.t), *lens_of(G, k, B), plan, B, invalid=invalid)
                    assert int(invalid.item()) == 0
                elif form == "ptrs":
                    code.plan_apply_ptrs(table(dd.t, dp.t), plan, B)
                else:
                    code.plan_apply(dd.t, dp.t, plan, B)
                torch.cuda.synchronize()
                dd.check_guards("plan_apply data")
                dp.check_guards("plan_apply parity")
                out += [dd.host(), dp.host()]
        for name in ONE_SHOTS:
            dd, dp = Guarded(d_in), Guarded(p_in)
            failed = ints(1)
            if "var" in name:
                invalid = ints(1)
                getattr(code, name)(table(dd.t, dp.t), *lens_of(G, k, B), dev(marks), B, failed=failed, invalid=invalid)
                assert int(invalid.item()) == 0
            elif "ptrs" in name:
                getattr(code, name)(table(dd.t, dp.t), dev(marks), B, failed=failed)
            else:
                getattr(code, name)(dd.t, dp.t, dev(marks), B, failed=failed)
            torch.cuda.synchronize()
            dd.check_guards(name)
            dp.check_guards(name)
            out += [dd.host(), dp.host(), int(failed.item())]
        return out

    got = both(st, run, "plans")
    what = f"plans at {st.name}"
    i = 0
    for mode, wd, wp, nf in ((REPAIR, rep_d, rep_p, nfail), (RECONSTRUCT, rec_d, p_in, rec_bad)):
        assert np.array_equal(got[i], want_plans[mode]) and got[i + 1] == nf, what
        for j, form in zip((i + 2, i + 4, i + 6), FORMS):
            written(got[j], wd, d_in, layout, form != "contig", f"{what} plan_apply-{form} data")
            written(got[j + 1], wp, p_in, layout, form != "contig", f"{what} plan_apply-{form} parity")
        i += 8
    for name in ONE_SHOTS:
        wd, wp, nf = (rep_d, rep_p, nfail) if name.startswith("repair") else (rec_d, p_in, rec_bad)
        written(got[i], wd, d_in, layout, "ptrs" in name, f"{what} {name} data")
        written(got[i + 1], wp, p_in, layout, "ptrs" in name, f"{what} {name} parity")
        assert got[i + 2] == nf, f"{what} {name}"
        i += 3
    return want_plans[REPAIR], want_plans[RECONSTRUCT]


def plan_calls(marks, B, check=False):
    """{name: call(code, dd, dp)} of every plan entry (or every check-plan entry) that must refuse an
    unsupported handle before it writes."""
    def lens(dd):
        return lens_of(dd.t.shape[0], dd.t.shape[1], B)

    if check:
        return {
            "check_build": lambda c, dd, dp: c.check_build(dev(marks)),
            "locate_wide": lambda c, dd, dp: c.locate_wide(dd.t, dp.t, dev(marks), B),
            "scrub_wide": lambda c, dd, dp: c.scrub_wide(dd.t, dp.t, dev(marks), B),
            "locate_ptrs_wide": lambda c, dd, dp: c.locate_ptrs_wide(table(dd.t, dp.t), B, marks=dev(marks)),
            "scrub_ptrs_wide": lambda c, dd, dp: c.scrub_ptrs_wide(table(dd.t, dp.t), B, marks=dev(marks)),
            "locate_ptrs_wide_var": lambda c, dd, dp: c.locate_ptrs_wide_var(table(dd.t, dp.t), *lens(dd), B, marks=dev(marks)),
            "scrub_ptrs_wide_var": lambda c, dd, dp: c.scrub_ptrs_wide_var(table(dd.t, dp.t), *lens(dd), B, marks=dev(marks)),
        }
    return {
        "plan_build": lambda c, dd, dp: c.plan_build(dev(marks), REPAIR),
        "repair_wide": lambda c, dd, dp: c.repair_wide(dd.t, dp.t, dev(marks), B),
        "reconstruct_wide": lambda c, dd, dp: c.reconstruct_wide(dd.t, dp.t, dev(marks), B),
        "repair_ptrs_wide": lambda c, dd, dp: c.repair_ptrs_wide(table(dd.t, dp.t), dev(marks), B),
        "reconstruct_ptrs_wide": lambda c, dd, dp: c.reconstruct_ptrs_wide(table(dd.t, dp.t), dev(marks), B),
        "repair_ptrs_wide_var": lambda c, dd, dp: c.repair_ptrs_wide_var(table(dd.t, dp.t), *lens(dd), dev(marks), B),
        "reconstruct_ptrs_wide_var": lambda c, dd, dp: c.reconstruct_ptrs_wide_var(table(dd.t, dp.t), *lens(dd), dev(marks), B),
    }


def all_refused(st, d, p, calls, text):
    for name, call in calls.items():
        dd, dp = Guarded(d), Guarded(p)
        refused(lambda: call(st.code, dd, dp), text, (dd, dp), (d, p), f"{name} at {st.name}")


def apply_refused(st, d, p, B, plan, check, text):
    """A plan built while the handle was accepted must not be applied once it is not."""
    dd, dp = Guarded(d), Guarded(p)
    lens = lens_of(d.shape[0], d.shape[1], B)
    calls = ({"check_apply": lambda: st.code.check_apply(dd.t, dp.t, plan, B),
              "check_apply_ptrs": lambda: st.code.check_apply_ptrs(table(dd.t, dp.t), plan, B),
              "check_apply_ptrs_var": lambda: st.code.check_apply_ptrs_var(table(dd.t, dp.t), *lens, plan, B)} if check else
             {"plan_apply": lambda: st.code.plan_apply(dd.t, dp.t, plan, B),
              "plan_apply_ptrs": lambda: st.code.plan_apply_ptrs(table(dd.t, dp.t), plan, B),
              "plan_apply_ptrs_var": lambda: st.code.plan_apply_ptrs_var(table(dd.t, dp.t), *lens, plan, B)})
    for name, call in calls.items():
        refused(call, text, (dd, dp), (d, p), f"{name} at {st.name}")


@pytest.mark.parametrize("lname", sorted(LAYOUT_IDS))
def test_plans_wide(oracle, live, lname):
    """plan_chk_version and enc_version (the build kernel reads the coefficients from the encode tables):
    plan_build / plan_apply, reconstruct_wide / repair_wide and their pointer-table forms at (26,4).
    original -> scaled (still [I; rows]: accepted, other plans) -> parity_only (QFEC_EUNSUP, nothing
    written) -> restore (accepted again, the first plans)."""
    layout = LAYOUT_IDS[lname]
    k, m = WIDE
    h = live(k, m)
    data, gm = data_of(k, m, layout), marks_for(k, m)
    marks = marks_to_rs_layout(gm, k)
    seen = []
    for name in ("original", "scaled", "parity_only", "restore"):
        st = h.at(name)
        if name == "parity_only":
            d_in, p_in = damage(data, encoded(oracle, st.rows, data, layout), gm)
            all_refused(st, d_in, p_in, plan_calls(marks, layout.B), he.EUNSUP_EDITED)
            apply_refused(st, d_in, p_in, layout.B, plan, False, he.EUNSUP_EDITED)
            continue
        seen.append(flat(check_plans(oracle, st, layout, data, gm)))
        plan = dev(seen[-1][0])
    assert not same(seen[0], seen[1]) and same(seen[2], seen[0])


# ------------------------------------------------------------------ check plans at (26,4) and (8,4)

def check_checks(oracle, st, layout, batches, gm):
    """check_build against locate_wide_common.expected_check over a cold code; check_apply, locate_wide /
    scrub_wide and the table forms against locate_wide_common.model."""
    G, k = batches[0][0].shape[:2]
    cold = qa.Code.from_rows(st.rows, rs_stale_quirk=True)
    want_plan = np.stack([lw.expected_check(cold, gm[g]) for g in range(G)])
    marks = marks_to_rs_layout(gm, k)
    B = layout.B

    def run(code):
        plan = code.check_build(dev(marks))
        torch.cuda.synchronize()
        out = [plan.cpu().numpy()]
        for d, p in batches:
            for form in FORMS:
                dd, dp = Guarded(d), Guarded(p)
                culprit, counts = ints(G), ints(5)
                mo = dev(np.full(len(marks), 0xEE, np.uint8))
                if form == "var":
                    invalid = ints(1)
                    code.check_apply_ptrs_var(table(dd.t, dp.t), *lens_of(G, k, B), plan, B, culprit=culprit, marks_out=mo,
                                              counts=counts, invalid=invalid)
                    assert int(invalid.item()) == 0
                elif form == "ptrs":
                    code.check_apply_ptrs(table(dd.t, dp.t), plan, B, culprit=culprit, marks_out=mo, counts=counts)
                else:
                    code.check_apply(dd.t, dp.t, plan, B, culprit=culprit, marks_out=mo, counts=counts)
                torch.cuda.synchronize()
                held(dd, d, "check_apply data")
                held(dp, p, "check_apply parity")
                out += [culprit.cpu().numpy(), mo.cpu().numpy(), counts.cpu().numpy()]
        return out

    got = both(st, run, "check plans")
    assert np.array_equal(got[0], want_plan), f"check_build at {st.name}"
    i = 1
    for d, p in batches:
        want, want_marks, want_counts = lw.model(cold, d, p, gm, B)
        for form in FORMS:
            assert np.array_equal(got[i], want) and np.array_equal(got[i + 1], want_marks), f"check_apply-{form} at {st.name}"
            assert list(got[i + 2]) == list(want_counts)
            i += 3
    wants = [check_erased(oracle, st, layout, batches, gm, entry) for entry in ("wide", "wide-ptrs", "wide-var")][0]
    return [want_plan] + wants


@pytest.mark.parametrize("lname", sorted(LAYOUT_IDS))
@pytest.mark.parametrize("k,m", [WIDE, (8, 4)], ids=lambda v: str(v))
def test_check_plans(oracle, live, k, m, lname):
    """check_chk_version: check_build / check_apply, locate_wide / scrub_wide and their pointer-table
    forms accept only generated rows.  original (accepted: the model's verdicts on both batches) ->
    scaled (refused: not the generated rows) -> parity_only (refused: edited handle) -> restore
    (accepted, the first results).  Nothing is written by a refused call."""
    layout = LAYOUT_IDS[lname]
    h = live(k, m)
    batches, gm, made = erased_batches(oracle, h, layout)
    marks = marks_to_rs_layout(gm, k)
    first = flat(check_checks(oracle, h.at("original"), layout, batches, gm))
    assert np.array_equal(first[1], made) and not np.array_equal(first[2], made)
    plan = dev(first[0])
    for name, text in (("scaled", he.EUNSUP_NOT_GENERATED), ("parity_only", he.EUNSUP_EDITED)):
        st = h.at(name)
        all_refused(st, *batches[0], plan_calls(marks, layout.B, check=True), text)
        apply_refused(st, *batches[0], layout.B, plan, True, text)
    assert same(flat(check_checks(oracle, h.at("restore"), layout, batches, gm)), first)


# ------------------------------------------------------------------ the ABI itself

def ref_codec():
    from oracle.oracle import RefCodec
    if not RefCodec.available():
        return None
    return RefCodec()


def host_ptrs(d, p):
    G, k, B = d.shape
    m = p.shape[1]
    return (C.c_void_p * (G * (k + m)))(*([d.ctypes.data + i * B for i in range(G * k)] +
                                           [p.ctypes.data + i * B for i in range(G * m)]))


@pytest.mark.parametrize("where", ["host", "device", "device-ptrs"])
@pytest.mark.parametrize("k,m", NARROW + [WIDE], ids=lambda v: str(v))
def test_abi(oracle, live, knobs, capfd, monkeypatch, k, m, where):
    """reed_solomon_encode / reed_solomon_reconstruct on one live handle through every edit: host
    pointers (the pipelined path: enc_version, dec.version and lut_seed_version, which decides whether
    the erased rows are staged), device rows one allocation each (staged), and the same with
    rs_dev_ptrs 1 (the pointer-table kernels; at (26,4) with rs_dev_ptrs_wide 1 the device plans, which
    an inconsistent handle must leave for the staged path: the trace names the branch taken).  Bytes and
    return codes equal the oracle's rs.c at every step.  original -> scaled -> parity_only -> zero_col0 -> restore."""
    knobs("rs_dev_ptrs", int(where == "device-ptrs"))
    knobs("rs_dev_ptrs_wide", int(where == "device-ptrs"))
    traced = where == "device-ptrs" and k + m > 24
    if traced:
        monkeypatch.setenv("QFEC_RS_TRACE", "1")
    B, G, n = 100, groups_for(k, m), k + m
    h = live(k, m)
    L = qa.lib()
    data = synth_bytes(0xAB1 + k, G * k * B).reshape(G, k, B).copy()
    stale = synth_bytes(0xAB2 + k, G * m * B).reshape(G, m, B).copy()
    gm = marks_for(k, m)
    marks = marks_to_rs_layout(gm, k)
    seen = []
    for name in ("original", "scaled", "parity_only", "zero_col0", "restore"):
        st = h.at(name)
        want_p = stale.copy()
        oracle.rs_encode(st.rows, data, want_p, B)
        d_in = damage(data, want_p, gm)[0]
        want_d = d_in.copy()
        want_rc = oracle.rs_reconstruct_full(st.full, want_d, want_p.copy(), marks, B)
        if where == "host":
            p = stale.copy()
            assert L.reed_solomon_encode(h.rs._h, host_ptrs(data, p), G * n, B) == 0
            d = d_in.copy()
            p2 = want_p.copy()
            rc = L.reed_solomon_reconstruct(h.rs._h, host_ptrs(d, p2), C.c_void_p(marks.ctypes.data), G * n, B)
        else:
            rows = device_rows(list(data.reshape(G * k, B)) + list(stale.reshape(G * m, B)))
            assert L.reed_solomon_encode(h.rs._h, ptr_array(rows), G * n, B) == 0
            p = fetch(rows[G * k:]).reshape(G, m, B)
            assert np.array_equal(fetch(rows[:G * k]).reshape(G, k, B), data)
            rows = device_rows(list(d_in.reshape(G * k, B)) + list(want_p.reshape(G * m, B)))
            capfd.readouterr()
            rc = L.reed_solomon_reconstruct(h.rs._h, ptr_array(rows), C.c_void_p(marks.ctypes.data), G * n, B)
            if traced:  # device plans only while rs->m is [I; rows] (plan_chk_version)
                tag = "ptrs wide" if st.twin is not None else "staged"
                assert f"reed_solomon_reconstruct ({tag})" in capfd.readouterr().err, name
            d, p2 = fetch(rows[:G * k]).reshape(G, k, B), fetch(rows[G * k:]).reshape(G, m, B)
        assert np.array_equal(p, want_p), f"encode at {name}"
        assert rc == want_rc == -1 and np.array_equal(d, want_d), f"reconstruct at {name}"
        assert np.array_equal(p2, want_p), f"reconstruct at {name}: parity written"
        seen.append([want_p, want_d])
    for a, b in zip(seen, seen[1:]):
        assert not np.array_equal(a[0], b[0]) or not np.array_equal(a[1], b[1])
    assert not np.array_equal(seen[0][0], seen[1][0]) and not np.array_equal(seen[1][1], seen[2][1])
    assert np.array_equal(seen[1][0], seen[2][0]) and same(seen[0], seen[4])


@pytest.mark.parametrize("k,m", NARROW + [WIDE], ids=lambda v: str(v))
def test_abi_vs_reference_rs(live, k, m):
    """The same edit sequence on a handle of the reference's own rs.c, which has no caches: bytes and
    return codes of encode and reconstruct equal at every step, on host rows."""
    ref = ref_codec()
    if ref is None:
        pytest.skip("reference libraries not built (make -C oracle ref)")
    B, G, n = 100, groups_for(k, m), k + m
    h = live(k, m)
    L = qa.lib()
    rh = ref.rs.reed_solomon_new(k, m)
    try:
        r_par = np.ctypeslib.as_array(rh.contents.parity, shape=(m, k))
        r_m = np.ctypeslib.as_array(rh.contents.m, shape=(n, k))
        assert np.array_equal(r_par, h.p0) and np.array_equal(r_m, h.m0)
        ref_side = types.SimpleNamespace(k=k, m=m, parity=r_par, m_matrix=r_m)
        data = synth_bytes(0xAB3 + k, G * k * B).reshape(G, k, B).copy()
        stale = synth_bytes(0xAB4 + k, G * m * B).reshape(G, m, B).copy()
        marks = marks_to_rs_layout(marks_for(k, m), k)
        for name in ("original", "scaled", "parity_only", "zero_col0", "restore"):
            if name != "original":
                he.EDITS[name](ref_side, h.p0, h.m0)
                h.at(name)
            p, rp = stale.copy(), stale.copy()
            assert L.reed_solomon_encode(h.rs._h, host_ptrs(data, p), G * n, B) == \
                ref.rs_encode(rh, host_ptrs(data, rp), G * n, B) == 0
            assert np.array_equal(p, rp), f"encode at {name}"
            d = data.copy()
            d.reshape(G * k, B)[marks[:G * k] == 1] = 0x5A
            rd = d.copy()
            rc = L.reed_solomon_reconstruct(h.rs._h, host_ptrs(d, p), C.c_void_p(marks.ctypes.data), G * n, B)
            rrc = ref.rs_reconstruct(rh, host_ptrs(rd, rp), marks, G * n, B)
            assert rc == rrc and np.array_equal(d, rd) and np.array_equal(p, rp), f"reconstruct at {name}"
    finally:
        ref.rs.reed_solomon_release(rh)


# ------------------------------------------------------------------ order

def test_order(oracle, live):
    """A family that refreshes a shared table for itself must not leave another family's stamp looking
    current: on one (8,4) handle every n <= 24 family is warmed, the handle is scaled, and the families
    are called in the reverse of the order that warmed them, each against its own expectation."""
    k, m = 8, 4
    layout = P112
    B = layout.B
    h = live(k, m)
    data, gm = data_of(k, m, layout), marks_for(k, m)
    fixed = fixed_batches(oracle, h, layout)
    one, _ = two_batches(oracle, h, layout, lambda d, p: dc.damage_every_shard(d, p, B))
    two, _ = two_batches(oracle, h, layout, lambda d, p: dc.locate2_damage(d, p, B))
    era, egm, _ = erased_batches(oracle, h, layout)
    families = [
        ("encode", lambda st: check_encode(oracle, st, layout, "contig", data)),
        ("verify", lambda st: check_verify(oracle, st, layout, "contig", one)),
        ("update", lambda st: check_update(oracle, st, layout, "contig", data)),
        ("encode_update_ptrs", lambda st: check_encode_update(oracle, st, layout, "ptrs", data)),
        ("reconstruct", lambda st: check_reconstruct(oracle, st, layout, "contig", fixed, gm)),
        ("reconstruct_ptrs", lambda st: check_reconstruct(oracle, st, layout, "ptrs", fixed, gm)),
        ("repair", lambda st: check_repair(oracle, st, layout, fixed, gm)),
        ("locate", lambda st: check_locate(oracle, st, layout, "contig", one)),
        ("locate_ptrs", lambda st: check_locate(oracle, st, layout, "ptrs", one)),
        ("locate2", lambda st: check_locate2(oracle, st, layout, two)),
        ("locate_erased", lambda st: check_erased(oracle, st, layout, era, egm)),
    ]
    st = h.at("original")
    first = {name: flat(check(st)) for name, check in families}
    st = h.at("scaled")
    for name, check in reversed(families):
        assert not same(flat(check(st)), first[name]), f"{name}: the expectation did not change with the edit"
    st = h.at("restore")
    for name, check in families[::2] + families[1::2]:
        assert same(flat(check(st)), first[name]), name
