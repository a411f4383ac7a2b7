"""GPU tests of the integrity family on pointer tables with per-shard lengths: qfec_verify_ptrs_var,
qfec_locate_ptrs_var and qfec_scrub_ptrs_var (include/qfec.h; kernels in qfec_integrity_ptrs_var.hip).
Batches live in a ptrs_var_common.VarPool in permuted slots, encoded by the oracle on zero-padded rows;
the guards and every byte at or past a shard's length are random, and a shard of length 0 has a wild
table entry.  Expected results come from how the damage was made and from the CPU model of
integrity_ptrs_var_common (the oracle on zero-padded rows, the beyond-length rule, the correction
formula); both must agree before the GPU is asked.  After every verify and locate call the whole pool
is compared with its image before the call; after a scrub with the expected image.  Shapes and their
coverage: integrity_ptrs_var_common.cells().  The launches of a batch beyond one launch's index space
are not reached here (no cheap way to force them)."""
import ctypes as C

import numpy as np
import pytest

import integrity_ptrs_common as ic
import integrity_ptrs_var_common as iv
import ptrs_common as pc
import quicknet_amd as qa
from integrity_ptrs_var_common import AMBIGUOUS, CLEAN, INVALID, MULTI
from locate2_common import mul_table

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
CELLS = iv.cells()
iv.assert_coverage(CELLS)
VERIFY_CELLS = [c for c in CELLS if c[:2] not in iv.LOCATE_ONLY]
LOCATE_CELLS = [c for c in CELLS if c[:2] not in iv.VERIFY_ONLY]
JUNK = 0x5A5A5A5A


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def counter(n=1, start=0):
    return torch.full((n,), start, dtype=torch.int32, device=DEV)


class Up:
    """A batch's image on the device with its table and lengths."""

    def __init__(self, b, img):
        self.b, self.img = b, img
        self.t = dev(img)
        assert self.t.data_ptr() % 16 == 0
        self.table = dev(b.table(self.t.data_ptr()))
        self.lens = dev(np.clip(b.lens, iv.INT_MIN, iv.INT_MAX).astype(np.int32).reshape(-1))
        self.glen = dev(np.clip(b.glen, iv.INT_MIN, iv.INT_MAX).astype(np.int32))

    def same(self, img):
        torch.cuda.synchronize()
        return np.array_equal(self.t.cpu().numpy(), img)


def verify(code, b, img, bad_groups=None, invalid=None):
    """-> (bad_rows, bad_groups, invalid): the output starts full of junk; the pool must come back as it was."""
    u = Up(b, img)
    rows = torch.full((b.G,), JUNK, dtype=torch.int32, device=DEV)
    cnt = counter() if bad_groups is None else bad_groups
    inv = counter() if invalid is None else invalid
    code.verify_ptrs_var(u.table, u.lens, u.glen, b.max_len, bad_rows=rows, bad_groups=cnt, invalid=inv)
    assert u.same(img), "verify_ptrs_var wrote into the pool"
    return rows.cpu().numpy(), int(cnt.cpu()[0]), int(inv.cpu()[0])


def locate(code, b, img, counts=None, invalid=None):
    """-> (culprit, marks, counts, invalid): junk outputs; the pool must come back as it was."""
    u = Up(b, img)
    culprit = torch.full((b.G,), JUNK, dtype=torch.int32, device=DEV)
    marks = torch.full((b.G * (b.k + b.m),), 0xEE, dtype=torch.uint8, device=DEV)
    cnt = counter(3) if counts is None else counts
    inv = counter() if invalid is None else invalid
    code.locate_ptrs_var(u.table, u.lens, u.glen, b.max_len, culprit=culprit, marks=marks, counts=cnt, invalid=inv)
    assert u.same(img), "locate_ptrs_var wrote into the pool"
    return culprit.cpu().numpy(), marks.cpu().numpy(), cnt.cpu().numpy().tolist(), int(inv.cpu()[0])


def scrub(code, b, img, counts=None, invalid=None):
    """-> (culprit, counts, invalid, the pool after the call)."""
    u = Up(b, img)
    cnt = counter(3) if counts is None else counts
    inv = counter() if invalid is None else invalid
    culprit = code.scrub_ptrs_var(u.table, u.lens, u.glen, b.max_len, counts=cnt, invalid=inv)
    torch.cuda.synchronize()
    return culprit.cpu().numpy(), cnt.cpu().numpy().tolist(), int(inv.cpu()[0]), u.t.cpu().numpy()


def check_locate(code, b, img, expect):
    """The model agrees with the construction, then the GPU with both."""
    model, mcounts, minv = iv.model_locate(b, img)
    assert np.array_equal(model, expect), (model, expect)
    culprit, marks, counts, inv = locate(code, b, img)
    assert np.array_equal(culprit, expect), (culprit, expect)
    assert np.array_equal(marks, ic.one_hot(expect, b.G, b.k, b.m))
    assert counts == mcounts and inv == minv
    return counts


def case(c):
    k, m, ml, mode = c
    code = qa.Code.cauchy(k, m)
    b, img = iv.batch(code, ml, mode)
    return code, b, img


def live_shards(b, g):
    """The shards of group g that have a byte to damage."""
    return [c for c in range(b.k + b.m) if b.span(g, c)[1] > 0]


# ---------------------------------------------------------------- 1. clean batch

@pytest.mark.parametrize("c", CELLS, ids=iv.cell_id)
def test_clean_batch(c):
    """Every word 0 / CLEAN, zero marks, counters untouched, junk outputs fully overwritten.  The image
    has random bytes everywhere outside [0, len) of a row, and wild entries for shards of length 0 (in
    the aligned modes they are misaligned as well, and must not matter)."""
    code, b, img = case(c)
    if c in VERIFY_CELLS:
        rows, cnt, inv = verify(code, b, img, bad_groups=counter(start=7), invalid=counter(start=9))
        assert not rows.any() and cnt == 7 and inv == 9
    if c in LOCATE_CELLS:
        culprit, marks, counts, inv = locate(code, b, img, counts=counter(3, start=3), invalid=counter(start=2))
        assert (culprit == CLEAN).all() and not marks.any() and counts == [3, 3, 3] and inv == 2


# ---------------------------------------------------------------- 2. verify bits

@pytest.mark.parametrize("c", VERIFY_CELLS, ids=iv.cell_id)
def test_verify_bits(c):
    """Every parity row damaged alone; a data shard per damage kind its length has room for (every row's
    bit), the one in two slabs included: the group is counted once although two waves report it.  Two
    calls on one counter accumulate; a counter-only call."""
    k, m, ml, mode = c
    code, b, img = case(c)
    expect = np.zeros(b.G, np.int32)
    groups = [g for g in range(b.G) if b.glen[g] > 0]
    n = 0
    for j in range(m):  # parity row j alone
        g = groups[(5 * j) % len(groups)]
        if expect[g]:
            continue
        kinds = sorted(iv.spots(int(b.glen[g])).items())
        b.hit(img, g, k + j, kinds[j % len(kinds)][1], salt=31 * j + 1)
        expect[g] = 1 << j
        n += 1
    kinds_seen = set()
    for g in groups:  # a data shard, each kind once where a group has room for it
        if expect[g]:
            continue
        i = int(np.argmax(b.lens[g]))
        for name, where in sorted(iv.spots(int(b.lens[g, i])).items()):
            if name not in kinds_seen:
                kinds_seen.add(name)
                b.hit(img, g, i, where, salt=g * 7 + 3)
                expect[g] = (1 << m) - 1
                n += 1
                break
    assert kinds_seen >= {"first", "last", "row"} and (ml < 1025 or "two-slabs" in kinds_seen)
    rows_m, bad_m, inv_m = iv.model_verify(b, img)
    assert np.array_equal(rows_m, expect) and bad_m == n and inv_m == 0
    cnt = counter(start=5)
    rows, total, inv = verify(code, b, img, bad_groups=cnt)
    assert np.array_equal(rows, expect) and total == 5 + n and inv == 0
    rows, total, inv = verify(code, b, img, bad_groups=cnt)
    assert np.array_equal(rows, expect) and total == 5 + 2 * n
    u = Up(b, img)
    only = counter()
    assert qa.lib().qfec_verify_ptrs_var(code._h, C.c_void_p(u.table.data_ptr()), C.c_void_p(u.lens.data_ptr()),
                                         C.c_void_p(u.glen.data_ptr()), b.G, ml, None, C.c_void_p(only.data_ptr()),
                                         None, None) == 0
    assert u.same(img) and int(only.cpu()[0]) == n


# ---------------------------------------------------------------- 3. one shard, every id; every damage kind

@pytest.mark.parametrize("c", LOCATE_CELLS, ids=iv.cell_id)
def test_one_shard_every_id(c):
    """Each shard id gets a group of its own in which it has bytes, damaged in that shard alone by one of
    the kinds of its own length (first byte, last byte below len_i, last byte of its last whole column,
    first byte of its part column, a byte in each of two slabs, the whole shard): exactly that id,
    one-hot marks, counts == [ids, 0, 0]; a second call accumulates."""
    k, m, ml, mode = c
    code, b, clean = case(c)
    n = k + m
    todo = list(range(n))
    rounds = 0
    while todo:
        img, expect, used, left = clean.copy(), np.full(b.G, CLEAN, np.int32), set(), []
        for s in todo:
            g = next((g for g in range(b.G) if g not in used and b.span(g, s)[1] > 0), None)
            if g is None:
                left.append(s)
                continue
            used.add(g)
            kinds = sorted(iv.spots(b.span(g, s)[1]).items())
            b.hit(img, g, s, kinds[(s + rounds) % len(kinds)][1], salt=900 + s)
            expect[g] = s
        assert len(left) < len(todo)
        ids = len(todo) - len(left)
        acc = counter(3)
        assert np.array_equal(iv.model_locate(b, img)[0], expect)
        culprit, marks, counts, inv = locate(code, b, img, counts=acc)
        assert np.array_equal(culprit, expect)
        assert np.array_equal(marks, ic.one_hot(expect, b.G, k, m))
        assert counts == [ids, 0, 0] and inv == 0
        culprit, marks, counts, inv = locate(code, b, img, counts=acc)
        assert np.array_equal(culprit, expect) and counts == [2 * ids, 0, 0]
        todo, rounds = left, rounds + 1


@pytest.mark.parametrize("k,m,ml,mode", [(10, 3, 1400, "aligned"), (16, 4, 1400, "aligned"), (9, 5, 1400, "aligned"),
                                         (10, 3, 1400, "residues"), (8, 4, 1025, "one-data")])
def test_every_damage_kind_on_a_short_shard(k, m, ml, mode):
    """One data shard, every damage kind of its own length, in groups whose shard is short (a part
    column inside the group's whole columns: the ragged path) and in groups of equal lengths."""
    code = qa.Code.cauchy(k, m)
    b, img = iv.batch(code, ml, mode)
    expect = np.full(b.G, CLEAN, np.int32)
    seen = set()
    for g in range(b.G):
        short = [i for i in range(k) if 16 < b.lens[g, i] < b.glen[g] and b.lens[g, i] % 16]
        i = short[g % len(short)] if short else int(np.argmax(b.lens[g]))
        if b.lens[g, i] == 0:
            continue
        for name, where in sorted(iv.spots(int(b.lens[g, i])).items()):
            if (name, bool(short)) not in seen:
                seen.add((name, bool(short)))
                b.hit(img, g, i, where, salt=g + 11)
                expect[g] = i
                break
    assert {n for n, s in seen if s} >= {"first", "last", "col-end", "part", "row"}
    check_locate(code, b, img, expect)


# ---------------------------------------------------------------- 4. the beyond-length rule

def padded_locate(code, b, img):
    """qfec_locate_ptrs on a copy of the batch with every row zero-padded to max_len (every group of the
    batch has L = max_len)."""
    assert (b.glen == b.max_len).all()
    d, p = iv.padded_rows(b, img)
    pool = pc.Pool(b.G * (b.k + b.m), b.max_len, np.zeros(b.G * (b.k + b.m), np.int64), seed=1)
    pool.put_all(0, d.reshape(-1, b.max_len))
    pool.put_all(b.G * b.k, p.reshape(-1, b.max_len))
    t, table = pc.to_device(torch, DEV, pool)
    return code.locate_ptrs(table, b.max_len).cpu().numpy()


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m", [(10, 3), (16, 4), (9, 5)])
def test_beyond_length_is_multi(k, m, mode):
    """For a short shard i, rows[j][i] x e XORed into every parity row at a position p >= len_i is what a
    corrupted byte p of shard i would look like on padded rows -- qfec_locate_ptrs on the padded copy
    says i -- but shard i has no byte p: MULTI, and the scrub changes nothing.  p in i's part column,
    in a later column and in a later slab (ragged waves); len_i = 1393 and p = 1397 (every wave of the
    group is full, the tail bytes judge); residues: the byte body.  The same error below len_i is
    located as i and corrected."""
    ml, Gn = 1400, 12
    mul = mul_table()
    code = qa.Code.cauchy(k, m)
    lens = np.full((Gn, k), ml, np.int64)
    plan = {1: (2, 100, 105), 2: (2, 100, 300), 3: (2, 100, 1100), 4: (k - 1, 1393, 1397), 5: (0, 1030, 1039),
            6: (3, 16, 16), 7: (1, 1024, 1024), 9: (2, 100, 99), 10: (k - 1, 1393, 1392)}
    for g, (i, n, _) in plan.items():
        lens[g, i] = n
    lens[8, 4] = 0
    b = iv.Batch(code.rows, ml, mode, lens, np.full(Gn, ml), seed=k + 41)
    img = b.host.copy()
    expect = np.full(Gn, CLEAN, np.int32)
    for g, (i, n, p) in plan.items():
        for j in range(m):
            img[b.span(g, k + j)[0] + p] ^= mul[int(code.rows[j, i]), 0x3B + g]
        expect[g] = MULTI if p >= n else i
    assert np.array_equal(padded_locate(code, b, img), np.where(expect == MULTI, [plan.get(g, (CLEAN,))[0] for g in range(Gn)], expect))
    counts = check_locate(code, b, img, expect)
    assert counts == [2, 7, 0]
    culprit, counts, inv, after = scrub(code, b, img)
    _, _, _, want = iv.model_scrub(b, img)
    assert np.array_equal(culprit, expect) and counts == [2, 7, 0] and inv == 0
    assert np.array_equal(after, want)
    for g in range(Gn):  # MULTI groups byte for byte as they were; the two located ones changed in one byte
        for c in range(k + m):
            s, n = b.span(g, c)
            same = np.array_equal(after[s:s + n], img[s:s + n])
            assert same == (expect[g] < 0 or c != expect[g]), (g, c)


# ---------------------------------------------------------------- 5. invalid groups

@pytest.mark.parametrize("k,m,ml,mode", [(10, 3, 1400, "aligned"), (9, 5, 1025, "residues"), (16, 4, 17, "one-data"),
                                         (60, 8, 1025, "aligned"), (32, 32, 1400, "aligned")])
def test_invalid_groups(k, m, ml, mode):
    """L = -1, max_len + 1, INT_MIN, INT_MAX; a len_i of L + 1 or -1 (in the last shard: all k lengths are
    judged).  Every table entry of an invalid group is wild.  Each is counted once, whatever the number
    of slabs; QFEC_LOC_INVALID, a zero bad_rows word and zero marks; it counts in no other counter;
    damaged and clean neighbours keep their verdicts; the scrub leaves the pool as the model says."""
    code = qa.Code.cauchy(k, m)
    lens, glen = iv.cycle_lengths(k, ml, 16)
    lens, glen = lens.copy(), glen.copy()
    lens[:, :] = np.minimum(lens, ml)
    for g, L in ((1, -1), (4, ml + 1), (6, iv.INT_MIN), (9, iv.INT_MAX)):
        glen[g] = L
    lens[11] = ml // 2
    glen[11] = ml // 2
    lens[11, k - 1] = ml // 2 + 1
    lens[13] = ml
    glen[13] = ml
    lens[13, k - 1] = -1
    lens[0], glen[0], lens[2], glen[2] = ml, ml, ml - 1, ml
    bad = iv.invalid_groups(lens, glen, ml)
    assert list(np.flatnonzero(bad)) == [1, 4, 6, 9, 11, 13]
    b = iv.Batch(code.rows, ml, mode, lens, glen, seed=k * 3 + ml)
    img = b.host.copy()
    b.hit(img, 0, k, [ml - 1], 1)          # a parity row next to an invalid group
    b.hit(img, 2, 1, [0], 2)               # a data shard between two
    expect = np.where(bad, INVALID, CLEAN).astype(np.int32)
    expect[0], expect[2] = k, 1
    if (k, m) not in iv.LOCATE_ONLY:
        rows_m, bad_m, inv_m = iv.model_verify(b, img)
        assert inv_m == 6 and bad_m == 2 and not rows_m[bad].any()
        inv = counter(start=10)
        rows, cnt, total = verify(code, b, img, invalid=inv)
        assert np.array_equal(rows, rows_m) and cnt == 2 and total == 16
        rows, cnt, total = verify(code, b, img, invalid=inv)
        assert total == 22
    if (k, m) not in iv.VERIFY_ONLY:
        counts = check_locate(code, b, img, expect)
        assert counts == [2, 0, 0]
        culprit, counts, inv, after = scrub(code, b, img)
        assert np.array_equal(culprit, expect) and counts == [2, 0, 0] and inv == 6
        assert np.array_equal(after, iv.model_scrub(b, img)[3]) and np.array_equal(after, b.host)


# ---------------------------------------------------------------- 6. MULTI across waves

@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m", [(10, 3), (16, 4), (8, 4), (9, 5), (5, 3)])
def test_multi_across_waves(k, m, mode):
    """max_len = 1400, two slabs and a tail: shard a hit only in slab 0 and shard b only in slab 1 (each
    wave alone sees a single-shard pattern); a parity row in slab 0 and a data shard in slab 1; two
    shards in the same byte.  All MULTI, zero marks, counts[1]."""
    ml = 1400
    code = qa.Code.cauchy(k, m)
    b, img = iv.batch(code, ml, mode)
    full = [g for g in range(b.G) if (b.lens[g] >= ml - 1).all()]
    part = [g for g in range(b.G) if b.glen[g] == ml and g not in full and b.lens[g, 0] > 1100 and b.lens[g, 1] > 8]
    g1, g2, g3, g4 = full[0], part[0], full[1], part[1]
    b.hit(img, g1, 1, [7], 1)
    b.hit(img, g1, 3, [1024 + 9], 2)
    b.hit(img, g2, k + 1, [100], 3)
    b.hit(img, g2, 0, [1024 + 70], 4)
    b.hit(img, g3, 2, [555], 5)
    b.hit(img, g3, 4, [555], 6)
    b.hit(img, g4, 0, [3, int(b.lens[g4, 0]) - 1], 7)  # and one single shard, in both slabs
    expect = np.full(b.G, CLEAN, np.int32)
    expect[[g1, g2, g3]] = MULTI
    expect[g4] = 0
    assert check_locate(code, b, img, expect) == [1, 3, 0]


# ---------------------------------------------------------------- 7. AMBIGUOUS

@pytest.mark.parametrize("ml,mode", [(64, "aligned"), (17, "residues"), (1025, "one-data")])
def test_ambiguous_rows(ml, mode):
    """rows [[1,2,3],[1,2,5]]: columns 0 and 1 are proportional, so a corrupted shard 0 is also
    explained by shard 1: AMBIGUOUS, counts[2], no marks -- unless the damage lies past shard 1's end,
    where only shard 0 is left.  Shard 2 is located."""
    code = qa.Code.from_rows([[1, 2, 3], [1, 2, 5]])
    Gn = 6
    lens = np.array([[ml, ml, ml], [ml, ml - 1, ml], [ml, ml, ml], [ml, ml // 2, ml], [ml - 2, ml, ml - 1], [0, 0, 0]])
    b = iv.Batch(code.rows, ml, mode, lens, np.array([ml] * 5 + [0]), seed=ml)
    img = b.host.copy()
    b.hit(img, 1, 0, [ml // 3], 1)
    b.hit(img, 3, 0, [ml - 1], 3)   # past the end of shard 1: shard 1 is no candidate
    b.hit(img, 4, 2, [ml - 2], 2)
    expect = np.array([CLEAN, AMBIGUOUS, CLEAN, 0, 2, CLEAN], np.int32)
    assert check_locate(code, b, img, expect) == [2, 0, 1]
    rows, cnt, inv = verify(code, b, img)
    assert list(rows) == [0, 3, 0, 3, 3, 0] and cnt == 3 and inv == 0


# ---------------------------------------------------------------- 8. against the fixed-length calls

@pytest.mark.parametrize("k,m,ml,mode", [(10, 3, 1000, "aligned"), (16, 4, 1400, "residues"), (4, 2, 17, "one-data"),
                                         (8, 4, 1025, "aligned"), (9, 5, 1040, "one-parity"), (5, 3, 1, "aligned")])
def test_against_the_fixed_length_calls(k, m, ml, mode):
    """All lengths = max_len: qfec_verify_ptrs / qfec_locate_ptrs / qfec_scrub_ptrs on the same table give
    the var calls' outputs word for word and, after the scrub, the same pool byte for byte, on a batch of
    clean, single and (m >= 3) double damage."""
    Gn = iv.G
    code = qa.Code.cauchy(k, m)
    b = iv.Batch(code.rows, ml, mode, np.full((Gn, k), ml), np.full(Gn, ml), seed=ml + k)
    pool = b.vp.pool
    img = b.host.copy()
    expect, double = ic.random_damage(np.random.default_rng(k * ml + m), pool, img, Gn, k, m, doubles=m >= 3)
    assert (expect == CLEAN).any() and (expect >= 0).any() and (m < 3 or double.any())
    u = Up(b, img)
    ref_cnt, ref_counts = counter(), counter(3)
    ref_rows = code.verify_ptrs(u.table, ml, bad_groups=ref_cnt).cpu().numpy()
    ref_marks = torch.empty(Gn * (k + m), dtype=torch.uint8, device=DEV)
    ref_culprit = code.locate_ptrs(u.table, ml, marks=ref_marks, counts=ref_counts).cpu().numpy()
    rows, cnt, inv = verify(code, b, img)
    culprit, marks, counts, inv2 = locate(code, b, img)
    assert np.array_equal(rows, ref_rows) and cnt == int(ref_cnt.cpu()[0]) and inv == 0 and inv2 == 0
    assert np.array_equal(culprit, ref_culprit) and np.array_equal(culprit, expect)
    assert np.array_equal(marks, ref_marks.cpu().numpy()) and counts == ref_counts.cpu().numpy().tolist()
    ref_scrubbed = code.scrub_ptrs(u.table, ml).cpu().numpy()
    torch.cuda.synchronize()
    culprit, counts, inv, after = scrub(code, b, img)
    assert np.array_equal(culprit, ref_scrubbed) and np.array_equal(after, u.t.cpu().numpy())
    assert np.array_equal(after, iv.model_scrub(b, img)[3])


# ---------------------------------------------------------------- 9. scrub

@pytest.mark.parametrize("k,m,ml,mode", [(10, 3, 1400, "aligned"), (16, 4, 1025, "one-data"), (9, 5, 1025, "residues"),
                                         (4, 2, 1400, "one-parity"), (20, 8, 17, "one-data"), (20, 8, 1400, "aligned"),
                                         (8, 4, 1400, "residues")])
def test_scrub(k, m, ml, mode):
    """Single damage in about half of the groups -- short data culprits, parity culprits, shards next to
    shards of length 0 -- and double damage (m >= 3) in a few.  After the scrub the whole pool is the
    pre-damage pool (so the random bytes right after len_i of a corrected shard are intact) except the
    double-damaged groups, which keep their damaged image; culprits and counts as the model says.
    d_culprit = NULL on a side stream; counters accumulate across two calls.  (20,8) is beyond
    qfec_scrub's k + m <= 24."""
    code = qa.Code.cauchy(k, m)
    b, clean = iv.batch(code, ml, mode)
    img = clean.copy()
    rng = np.random.default_rng(k + ml * m)
    expect = np.full(b.G, CLEAN, np.int32)
    want = clean.copy()
    for g in range(b.G):
        live = live_shards(b, g)
        r = rng.random()
        cnt = 0 if not live or r > 0.6 else 2 if (m >= 3 and r < 0.1 and len(live) > 1) else 1
        for c in rng.choice(live, size=cnt, replace=False) if cnt else []:
            n = b.span(g, int(c))[1]
            where = rng.choice(n, size=min(n, int(rng.integers(1, 5))), replace=False)
            b.hit(img, g, int(c), where, int(rng.integers(1 << 30)))
        expect[g] = MULTI if cnt == 2 else int(c) if cnt == 1 else CLEAN
        if cnt == 2:
            for s in range(k + m):
                a, n = b.span(g, s)
                want[a:a + n] = img[a:a + n]
    located, multi = int((expect >= 0).sum()), int((expect == MULTI).sum())
    assert located > 3 and (m < 3 or multi) and (expect[expect >= 0] >= k).any()
    assert any(0 <= expect[g] < k and b.lens[g, expect[g]] < b.glen[g] for g in range(b.G)), "a short data culprit"
    m_culprit, m_counts, _, m_after = iv.model_scrub(b, img)
    assert np.array_equal(m_culprit, expect) and np.array_equal(m_after, want) and m_counts == [located, multi, 0]

    acc, inv = counter(3), counter(start=4)
    culprit, counts, invalid, after = scrub(code, b, img, counts=acc, invalid=inv)
    assert np.array_equal(culprit, expect) and counts == [located, multi, 0] and invalid == 4
    assert np.array_equal(after, want)
    culprit, counts, invalid, after = scrub(code, b, img, counts=acc, invalid=inv)
    assert counts == [2 * located, 2 * multi, 0] and invalid == 4 and np.array_equal(after, want)

    # no culprits wanted, on a side stream
    u = Up(b, img)
    counts2 = counter(3)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert qa.lib().qfec_scrub_ptrs_var(code._h, C.c_void_p(u.table.data_ptr()), C.c_void_p(u.lens.data_ptr()),
                                            C.c_void_p(u.glen.data_ptr()), b.G, ml, None, C.c_void_p(counts2.data_ptr()),
                                            None, C.c_void_p(side.cuda_stream)) == 0
    side.synchronize()
    assert np.array_equal(u.t.cpu().numpy(), want) and counts2.cpu().numpy().tolist() == [located, multi, 0]

    # a clean pool comes back as it was
    culprit, counts, invalid, after = scrub(code, b, clean)
    assert (culprit == CLEAN).all() and counts == [0, 0, 0] and np.array_equal(after, clean)


def test_round_trip_32_8():
    """encode_ptrs_var -> damage -> scrub_ptrs_var -> verify_ptrs_var on (32,8): the parity the encode
    wrote and the lengths it reported are what the integrity calls take."""
    k, m, ml = 32, 8, 1400
    code = qa.Code.cauchy(k, m)
    lens, _ = iv.cycle_lengths(k, ml)
    b = iv.Batch(code.rows, ml, "aligned", lens, lens.max(1), seed=328)
    u = Up(b, b.host.copy())
    glen = torch.full((b.G,), -7, dtype=torch.int32, device=DEV)
    code.encode_ptrs_var(u.table, u.lens, ml, group_len=glen)
    torch.cuda.synchronize()
    assert np.array_equal(glen.cpu().numpy(), b.glen.astype(np.int32))
    encoded = u.t.cpu().numpy().copy()
    assert np.array_equal(encoded, b.host)  # the oracle's parity, and nothing outside it
    rows = code.verify_ptrs_var(u.table, u.lens, glen, ml)
    assert not rows.cpu().numpy().any()
    img = encoded.copy()
    expect = np.full(b.G, CLEAN, np.int32)
    for g in range(0, b.G, 3):
        live = live_shards(b, g)
        if live:
            c = live[(5 * g) % len(live)]
            b.hit(img, g, c, [b.span(g, c)[1] - 1], g + 1)
            expect[g] = c
    u.t.copy_(dev(img))
    bad = counter()
    rows = code.verify_ptrs_var(u.table, u.lens, glen, ml, bad_groups=bad)
    assert int(bad.cpu()[0]) == int((expect >= 0).sum()) and np.array_equal(rows.cpu().numpy() != 0, expect >= 0)
    culprit = code.scrub_ptrs_var(u.table, u.lens, glen, ml)
    assert np.array_equal(culprit.cpu().numpy(), expect)
    rows = code.verify_ptrs_var(u.table, u.lens, glen, ml, bad_groups=bad)
    assert not rows.cpu().numpy().any() and u.same(encoded)
