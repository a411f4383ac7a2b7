"""GPU tests of qfec_check_build / qfec_check_apply / qfec_locate_wide / qfec_scrub_wide: single-shard
error location at any k + m, beside lost shards or not.  The check plans the device builds are held
to the host's over the whole buffer; on narrow codes the verdicts, marks and counts are held to
qfec_locate_erased's on the same batch; on wide codes to a numpy model of the definition
(locate_wide_common.model).  All comparisons are exact bytes and integers.  The rows of lost shards
are filled with junk (they are never read), every buffer sits between guard bytes, and the inputs are
compared unwritten.

Run on an MI355X:  python -m pytest tests/test_gpu_locate_wide.py -m gpu -q
"""
import numpy as np
import pytest

import quicknet_amd as qa
from quicknet_amd.synth import marks_to_rs_layout
from locate_wide_common import AMBIGUOUS, CLEAN, LOST, MULTI, UNCHECKED, masks_of_every_t, model
from repair_common import encoded, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
GUARD, GUARD_BYTE = 64, 0xC3


class Guarded:
    """A device tensor of `shape` inside a flat buffer with GUARD bytes on either side, `skew` bytes
    off the 16-byte grid when asked."""

    def __init__(self, shape, dtype=torch.uint8, fill=0, skew=0):
        size = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.flat = torch.full((GUARD + skew + size + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        assert self.flat.data_ptr() % 16 == 0
        self.lo, self.hi = GUARD + skew, GUARD + skew + size
        self.t = self.flat[self.lo:self.hi].view(dtype).view(shape)
        self.t.fill_(fill)

    @classmethod
    def of(cls, host, skew=0):
        g = cls(host.shape, skew=skew)
        g.t.copy_(torch.from_numpy(np.ascontiguousarray(host)))
        return g

    def intact(self):
        return bool((self.flat[:self.lo] == GUARD_BYTE).all()) and bool((self.flat[self.hi:] == GUARD_BYTE).all())


def host_batch(flavour, k, m, B, pitch, G):
    """A consistent batch on the host: (code, data [G, k, pitch], parity [G, m, pitch]), garbage in
    [B, pitch) of both."""
    code, data, par = encoded(flavour, k, m, B, pitch, G)
    return code, data.cpu().numpy(), par.cpu().numpy()


def row_of(hd, hp, g, c):
    k = hd.shape[1]
    return hd[g, c] if c < k else hp[g, c - k]


def lose(rng, hd, hp, gm, g, t, keep=()):
    """t random lost shards outside `keep` (non-zero marks, junk rows over the whole pitch); returns
    the unmarked ids: K, then the spares."""
    n = gm.shape[1]
    ids = rng.choice([i for i in range(n) if i not in keep], size=t, replace=False)
    gm[g, ids] = rng.integers(1, 256, size=t)
    for c in ids:
        row_of(hd, hp, g, c)[:] = rng.integers(0, 256, size=hd.shape[2], dtype=np.uint8)
    return [i for i in range(n) if not gm[g, i]]


def hurt(rng, row, B, kind):
    """0: one byte somewhere, 1: the last byte of [0, B) only, 2: several bytes, 3: bytes >= B only
    (must change nothing; falls back to kind 0 without padding)."""
    if kind == 3 and len(row) > B:
        row[B:] ^= rng.integers(1, 256, size=len(row) - B, dtype=np.uint8)
        return False
    if kind == 1:
        row[B - 1] ^= rng.integers(1, 256)
    elif kind == 2:
        for b in rng.choice(B, size=min(B, 5), replace=False):
            row[b] ^= rng.integers(1, 256)
    else:
        row[rng.integers(0, B)] ^= rng.integers(1, 256)
    return True


def run_locate(code, hd, hp, gm, B, skew=0, alias=False, counts=None, use_marks=True):
    """qfec_locate_wide on host arrays between guards -> (culprit, marks_out, counts) on the host.
    Also: nothing outside the outputs was written."""
    G, n = gm.shape
    d, p = Guarded.of(hd, skew), Guarded.of(hp, skew)
    marks_h = marks_to_rs_layout(gm, code.k)
    marks = Guarded.of(marks_h)
    out = marks if alias else Guarded((G * n,), fill=0xEE)
    culprit = Guarded((G,), torch.int32, fill=0x5A5A5A5A)
    cnt = Guarded((5,), torch.int32)
    if counts is not None:
        cnt.t.copy_(torch.from_numpy(np.asarray(counts, np.int32)))
    res = code.locate_wide(d.t, p.t, marks.t if use_marks else None, B, culprit=culprit.t, marks_out=out.t, counts=cnt.t)
    torch.cuda.synchronize()
    assert res is culprit.t
    assert all(x.intact() for x in (d, p, marks, out, culprit, cnt))
    assert np.array_equal(d.t.cpu().numpy(), hd) and np.array_equal(p.t.cpu().numpy(), hp)
    if not alias:
        assert np.array_equal(marks.t.cpu().numpy(), marks_h)
    return culprit.t.cpu().numpy(), out.t.cpu().numpy(), cnt.t.cpu().numpy()


def assert_is_model(code, hd, hp, gm, B, **kw):
    want_c, want_m, want_n = model(code, hd, hp, gm, B)
    culprit, marks_out, counts = run_locate(code, hd, hp, gm, B, **kw)
    assert np.array_equal(culprit, want_c), np.nonzero(culprit != want_c)[0][:8]
    assert np.array_equal(marks_out, want_m)
    assert list(counts) == list(want_n)
    return want_c


# ---------------------------------------------------------------- 1. device plan = host plan
# k + m > 24; k > 32; k + m > 64 (the marks span two ballot passes); S > 8; the widest shapes
PLAN_SHAPES = [("cauchy", 32, 8), ("vandermonde", 32, 8), ("cauchy", 60, 8), ("cauchy", 70, 10), ("cauchy", 200, 55),
               ("cauchy", 128, 127)]


@pytest.mark.parametrize("flavour,k,m", PLAN_SHAPES)
def test_device_check_plan_is_the_host_plan(flavour, k, m):
    code = getattr(qa.Code, flavour)(k, m)
    n, stride = k + m, code.check_stride()
    gm = masks_of_every_t(k + m, n, m, 2 if m < 20 else 1)
    G = len(gm)
    want = np.stack([code.check_host(mk) for mk in gm])
    buf = Guarded((G, stride), fill=0xEE)
    marks = Guarded.of(marks_to_rs_layout(gm, k))
    assert code.check_build(marks.t, check_plan=buf.t) is buf.t
    torch.cuda.synchronize()
    got = buf.t.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert buf.intact() and marks.intact()
    # no marks at all: every group gets the plan of the empty mask
    none = Guarded((3, stride), fill=0xEE)
    code.check_build(None, groups=3, check_plan=none.t)
    torch.cuda.synchronize()
    empty = code.check_host(np.zeros(n, np.uint8))
    assert np.array_equal(none.t.cpu().numpy(), np.stack([empty] * 3)) and none.intact()


# ---------------------------------------------------------------- 2. narrow codes: qfec_locate_erased
def narrow_batch(flavour, k, m, B, pitch):
    """Every (lost, corrupted) pair, every shard corrupted in a complete group, and the verdict
    classes; never two corrupted survivors beside two spares."""
    n = k + m
    G = n * (n - 1) + n + 12
    code, hd, hp = host_batch(flavour, k, m, B, pitch, G)
    rng = np.random.default_rng(100 * k + m)
    gm = np.zeros((G, n), np.uint8)
    g = 0
    for lost in range(n):
        for c in range(n):
            if c != lost:
                gm[g, lost] = 1 + (g % 255)
                row_of(hd, hp, g, lost)[:] = rng.integers(0, 256, size=pitch, dtype=np.uint8)
                hurt(rng, row_of(hd, hp, g, c), B, g % 4)
                g += 1
    for c in range(n):
        hurt(rng, row_of(hd, hp, g, c), B, c % 3)
        g += 1
    left = lose(rng, hd, hp, gm, g, m)  # UNCHECKED, even with a corrupted survivor
    row_of(hd, hp, g, left[0])[0] ^= 0x11
    lose(rng, hd, hp, gm, g + 1, m + 1)  # LOST
    lose(rng, hd, hp, gm, g + 2, m - 1)  # CLEAN with one spare
    left = lose(rng, hd, hp, gm, g + 3, m - 1)  # AMBIGUOUS: a shard of K
    row_of(hd, hp, g + 3, left[k // 2])[B - 1] ^= 0x40
    left = lose(rng, hd, hp, gm, g + 4, m - 1)  # AMBIGUOUS: the one spare
    row_of(hd, hp, g + 4, left[k])[0] ^= 0x02
    left = lose(rng, hd, hp, gm, g + 5, m - 3)  # MULTI: two of K in one byte
    row_of(hd, hp, g + 5, left[1])[B // 2] ^= 0x21
    row_of(hd, hp, g + 5, left[2])[B // 2] ^= 0x9E
    left = lose(rng, hd, hp, gm, g + 6, m - 3)  # MULTI: one of K and a spare, different bytes
    row_of(hd, hp, g + 6, left[0])[0] ^= 0x10
    row_of(hd, hp, g + 6, left[k + 1])[B - 1] ^= 0x04
    lose(rng, hd, hp, gm, g + 7, 1)  # CLEAN with a loss; the rest stay complete and clean
    return code, hd, hp, gm


@pytest.mark.parametrize("flavour,k,m,B,pitch", [("cauchy", 10, 3, 40, 48), ("cauchy", 16, 4, 33, 48),
                                                 ("vandermonde", 16, 4, 33, 48), ("cauchy", 20, 4, 17, 17)])
def test_narrow_codes_answer_as_locate_erased(flavour, k, m, B, pitch):
    code, hd, hp, gm = narrow_batch(flavour, k, m, B, pitch)
    G, n = gm.shape
    d, p = to_dev(hd), to_dev(hp)
    marks = to_dev(marks_to_rs_layout(gm, k))
    ref_counts = torch.zeros(5, dtype=torch.int32, device=DEV)
    ref_out = torch.full((G * n,), 0xEE, dtype=torch.uint8, device=DEV)
    ref = code.locate_erased(d, p, marks, B, marks_out=ref_out, counts=ref_counts)
    torch.cuda.synchronize()
    ref, ref_counts = ref.cpu().numpy(), ref_counts.cpu().numpy()
    assert all((ref == v).any() for v in (CLEAN, MULTI, AMBIGUOUS, UNCHECKED, LOST)) and (ref >= 0).sum() >= n * (n - 1) // 2
    culprit, marks_out, counts = run_locate(code, hd, hp, gm, B)
    assert np.array_equal(culprit, ref), np.nonzero(culprit != ref)[0][:8]
    assert np.array_equal(marks_out, ref_out.cpu().numpy())
    assert list(counts) == list(ref_counts)
    # complete groups, no marks buffer at all: the same as all-zero marks
    whole = ~gm.any(axis=1)
    zero = np.zeros((int(whole.sum()), n), np.uint8)
    a = run_locate(code, hd[whole], hp[whole], zero, B, use_marks=False)
    b = run_locate(code, hd[whole], hp[whole], zero, B)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[0], ref[whole])


# ---------------------------------------------------------------- 3. wide codes: the numpy model
def wide_batch(flavour, k, m, B, pitch, ts):
    """Every shard id corrupted beside t lost shards for every t of ts, the damage placement varying
    over the ids (one byte, the last byte, several bytes, bytes >= B only); then two corrupted
    survivors with three spares or more, and a corrupted spare beside one lost shard."""
    n = k + m
    G = len(ts) * n + 4
    code, hd, hp = host_batch(flavour, k, m, B, pitch, G)
    rng = np.random.default_rng(1000 * k + 10 * m + B)
    gm = np.zeros((G, n), np.uint8)
    g = 0
    for t in ts:
        for c in range(n):
            lose(rng, hd, hp, gm, g, t, keep=(c,))
            hurt(rng, row_of(hd, hp, g, c), B, (c + t) % 4)
            g += 1
    left = lose(rng, hd, hp, gm, g, m - 3)  # two of K, the same byte
    row_of(hd, hp, g, left[0])[B // 2] ^= 0x21
    row_of(hd, hp, g, left[k - 1])[B // 2] ^= 0x9E
    left = lose(rng, hd, hp, gm, g + 1, 0)  # one of K and the last spare, any bytes
    hurt(rng, row_of(hd, hp, g + 1, left[k // 2]), B, 0)
    hurt(rng, row_of(hd, hp, g + 1, left[-1]), B, 1)
    left = lose(rng, hd, hp, gm, g + 2, 1)  # the last spare alone
    hurt(rng, row_of(hd, hp, g + 2, left[-1]), B, 2)
    left = lose(rng, hd, hp, gm, g + 3, 1)  # the first spare alone
    hurt(rng, row_of(hd, hp, g + 3, left[k]), B, 0)
    return code, hd, hp, gm


def six_ts(m):
    return sorted({0, 1, m - 2, m - 1, m, m + 1})


# block_size 1, 15, 16, 17 on 16-byte lanes (the masked tail column); (70,10) with t <= 1 has S > 8:
# two syndrome passes; (200,55) and (128,127): the marks span ballot passes, up to 16 passes
WIDE = [("cauchy", 32, 8, 1, 16), ("cauchy", 32, 8, 15, 16), ("cauchy", 32, 8, 16, 16), ("cauchy", 32, 8, 17, 32),
        ("vandermonde", 32, 8, 17, 48), ("cauchy", 70, 10, 17, 32), ("cauchy", 200, 55, 16, 32),
        ("cauchy", 128, 127, 5, 16)]


@pytest.mark.parametrize("flavour,k,m,B,pitch", WIDE)
def test_wide_codes_answer_as_the_model(flavour, k, m, B, pitch):
    ts = six_ts(m) if k + m < 200 else [0, m - 2] if m < 100 else [m - 3]
    code, hd, hp, gm = wide_batch(flavour, k, m, B, pitch, ts)
    want = assert_is_model(code, hd, hp, gm, B)
    n = k + m
    assert (want >= 0).sum() >= n // 2 and (want == MULTI).sum() >= 2
    if len(ts) == 6:
        assert all((want == v).any() for v in (AMBIGUOUS, UNCHECKED, LOST)) and (pitch == B or (want == CLEAN).any())
    # marks_out aliasing marks, and counts accumulating over a second call
    first = run_locate(code, hd, hp, gm, B)
    culprit, aliased, counts = run_locate(code, hd, hp, gm, B, alias=True, counts=first[2])
    assert np.array_equal(culprit, want) and np.array_equal(aliased, first[1]) and list(counts) == list(2 * first[2])


def test_two_waves_per_group():
    """block_size 1040: 65 columns, two waves per group.  Damage in the second wave only; in both
    waves by one shard; in both waves by different shards (MULTI only across waves); a spare in one
    wave and a shard of K in the other."""
    k, m, B, pitch = 32, 8, 1040, 1040
    n = k + m
    ts = [0, 1, m - 2]
    G = 5 * len(ts) + 1
    code, hd, hp = host_batch("cauchy", k, m, B, pitch, G)
    rng = np.random.default_rng(7)
    gm = np.zeros((G, n), np.uint8)
    expect = np.full(G, CLEAN, np.int32)
    for i, t in enumerate(ts):
        g = 5 * i
        left = lose(rng, hd, hp, gm, g, t)
        row_of(hd, hp, g, left[3])[1030] ^= 0x80
        expect[g] = left[3]
        left = lose(rng, hd, hp, gm, g + 1, t)
        row_of(hd, hp, g + 1, left[k])[B - 1] ^= 0x01  # the first spare, the last byte
        expect[g + 1] = left[k]
        left = lose(rng, hd, hp, gm, g + 2, t)
        row_of(hd, hp, g + 2, left[k - 1])[[5, 1039]] ^= 0x3C
        expect[g + 2] = left[k - 1]
        left = lose(rng, hd, hp, gm, g + 3, t)
        row_of(hd, hp, g + 3, left[0])[7] ^= 0x55
        row_of(hd, hp, g + 3, left[1])[1025] ^= 0x55
        expect[g + 3] = MULTI
        left = lose(rng, hd, hp, gm, g + 4, t)
        row_of(hd, hp, g + 4, left[k + 1])[1000] ^= 0x02
        row_of(hd, hp, g + 4, left[2])[1024] ^= 0x02
        expect[g + 4] = MULTI
    want = assert_is_model(code, hd, hp, gm, B)
    assert np.array_equal(want, expect)


@pytest.mark.parametrize("B,pitch,skew", [(17, 33, 0), (17, 32, 1), (64, 71, 0), (100, 112, 1)])
def test_byte_path(B, pitch, skew):
    """An odd pitch, or bases one byte off the 16-byte grid: one byte per lane."""
    code, hd, hp, gm = wide_batch("cauchy", 32, 8, B, pitch, six_ts(8))
    assert_is_model(code, hd, hp, gm, B, skew=skew)
    code, hd, hp, gm = wide_batch("cauchy", 70, 10, B, pitch, [0, 1])
    assert_is_model(code, hd, hp, gm, B, skew=skew)


# ---------------------------------------------------------------- 4. one check plan, two batches
def test_one_check_plan_serves_two_batches():
    k, m, B, pitch = 60, 8, 48, 48
    n = k + m
    code, hd, hp, gm = wide_batch("cauchy", k, m, B, pitch, [0, 2, m - 1, m])
    G = len(gm)
    marks = to_dev(marks_to_rs_layout(gm, k))
    plans = code.check_build(marks)
    marks.fill_(0xFF)  # the plan holds the marks: the buffer is free to change
    torch.cuda.synchronize()
    # a second batch with the same losses: the same groups, other damage
    rng = np.random.default_rng(11)
    hd2, hp2 = encoded("cauchy", k, m, B, pitch, G)[1:]
    hd2, hp2 = hd2.cpu().numpy(), hp2.cpu().numpy()
    for g in range(G):
        left = [i for i in range(n) if not gm[g, i]]
        for c in np.nonzero(gm[g])[0]:
            row_of(hd2, hp2, g, c)[:] = 0x77
        if g % 3 and len(left) >= k:
            hurt(rng, row_of(hd2, hp2, g, left[(5 * g) % len(left)]), B, g % 3)
    for a, b in ((hd, hp), (hd2, hp2)):
        out = torch.full((G * n,), 0xEE, dtype=torch.uint8, device=DEV)
        counts = torch.zeros(5, dtype=torch.int32, device=DEV)
        culprit = code.check_apply(to_dev(a), to_dev(b), plans, B, marks_out=out, counts=counts)
        torch.cuda.synchronize()
        want = model(code, a, b, gm, B)
        assert np.array_equal(culprit.cpu().numpy(), want[0])
        assert np.array_equal(out.cpu().numpy(), want[1]) and list(counts.cpu().numpy()) == list(want[2])


def test_more_than_one_chunk_of_plans():
    """The one-shot keeps one chunk's plans under 64 MiB: at 22 112 B per group (200,55) goes in chunks
    of 3 034 groups.  Damage on both sides of the first boundary and in the last group, beside a lost
    shard each; the model judges those groups, every other group is complete and consistent."""
    k, m, B, pitch = 200, 55, 16, 16
    n = k + m
    per = (64 << 20) // qa.Code.cauchy(k, m).check_stride()
    G = per + 40
    assert per == 3034
    code, hd, hp = host_batch("cauchy", k, m, B, pitch, G)
    rng = np.random.default_rng(3)
    gm = np.zeros((G, n), np.uint8)
    expect = np.full(G, CLEAN, np.int32)
    hit = [0, per - 1, per, per + 1, G - 1]
    for i, g in enumerate(hit):
        left = lose(rng, hd, hp, gm, g, 1 + i)
        c = left[(37 * i) % len(left)]
        hurt(rng, row_of(hd, hp, g, c), B, i % 3)
        expect[g] = c
    lose(rng, hd, hp, gm, per + 2, m)
    expect[per + 2] = UNCHECKED
    sub = hit + [per + 2]
    want = model(code, hd[sub], hp[sub], gm[sub], B)
    assert np.array_equal(want[0], expect[sub])
    culprit, marks_out, counts = run_locate(code, hd, hp, gm, B)
    assert np.array_equal(culprit, expect)
    marked = (gm != 0).astype(np.uint8)
    marked[hit, expect[hit]] = 1
    assert np.array_equal(marks_out, marks_to_rs_layout(marked, k))
    assert list(counts) == [len(hit), 0, 0, 1, 0]


# ---------------------------------------------------------------- 5. scrub_wide
def random_loss_and_damage(rng, hd, hp, B):
    """In place -> gm [G, n].  Per group t lost shards (junk rows) and 0, 1 or 2 corrupted survivors:
    mostly t <= m - 2 with one corrupted survivor; some intact; two corrupted survivors only where
    three spares remain; t = m - 1 with and without damage; t = m; t = m + 1."""
    G, k, pitch = hd.shape
    m = hp.shape[1]
    n = k + m
    gm = np.zeros((G, n), np.uint8)
    for g in range(G):
        r = rng.random()
        if r < 0.55:
            t, nc = int(rng.integers(0, m - 1)), 1
        elif r < 0.65:
            t, nc = int(rng.integers(0, m - 1)), 0
        elif r < 0.75:
            t, nc = int(rng.integers(0, m - 2)), 2
        elif r < 0.85:
            t, nc = m - 1, int(rng.integers(0, 2))
        elif r < 0.92:
            t, nc = m, 0
        else:
            t, nc = m + 1, 0
        left = lose(rng, hd, hp, gm, g, t)
        for c in rng.choice(left, size=nc, replace=False):
            hurt(rng, row_of(hd, hp, g, c), B, int(rng.integers(0, 3)))
    return gm


@pytest.mark.parametrize("flavour,k,m,G", [("cauchy", 32, 8, 80), ("vandermonde", 64, 16, 60), ("cauchy", 200, 55, 64)])
def test_scrub_wide(flavour, k, m, G):
    B, pitch = 100, 112
    code, d0, p0 = host_batch(flavour, k, m, B, pitch, G)
    hd, hp = d0.copy(), p0.copy()
    gm = random_loss_and_damage(np.random.default_rng(k + m), hd, hp, B)
    expect, _, want_counts = model(code, hd, hp, gm, B)
    left_alone = np.isin(expect, (MULTI, AMBIGUOUS, LOST))
    assert (expect >= 0).sum() >= G // 3 and all((expect == v).any() for v in (CLEAN, MULTI, AMBIGUOUS, UNCHECKED, LOST))
    d, p = Guarded.of(hd), Guarded.of(hp)
    marks = Guarded.of(marks_to_rs_layout(gm, k))
    counts = torch.zeros(5, dtype=torch.int32, device=DEV)
    failed = torch.zeros(1, dtype=torch.int32, device=DEV)
    culprit = code.scrub_wide(d.t, p.t, marks.t, B, counts=counts, failed=failed)
    torch.cuda.synchronize()
    assert np.array_equal(culprit.cpu().numpy(), expect)
    assert list(counts.cpu().numpy()) == list(want_counts)
    assert int(failed.item()) == (expect == LOST).sum()
    assert np.array_equal(marks.t.cpu().numpy(), marks_to_rs_layout(gm, k))  # the caller's marks are not written
    assert d.intact() and p.intact() and marks.intact()
    rd, rp = d.t.cpu().numpy(), p.t.cpu().numpy()
    healed = ~left_alone
    assert np.array_equal(rd[healed][..., :B], d0[healed][..., :B])
    assert np.array_equal(rp[healed][..., :B], p0[healed][..., :B])
    assert np.array_equal(rd[left_alone], hd[left_alone]) and np.array_equal(rp[left_alone], hp[left_alone])
    # the verdicts and counters are optional, and so are the marks of a complete batch
    d2, p2 = to_dev(hd), to_dev(hp)
    assert qa.lib().qfec_scrub_wide(code._h, d2.data_ptr(), p2.data_ptr(), marks.t.data_ptr(), G, B, pitch,
                                    None, None, None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(d2, d.t) and torch.equal(p2, p.t)
    whole = np.nonzero(~gm.any(axis=1) & (expect >= 0))[0]
    if len(whole):
        d3, p3 = to_dev(hd[whole]), to_dev(hp[whole])
        code.scrub_wide(d3, p3, None, B)
        torch.cuda.synchronize()
        assert np.array_equal(d3.cpu().numpy()[..., :B], d0[whole][..., :B])
        assert np.array_equal(p3.cpu().numpy()[..., :B], p0[whole][..., :B])


@pytest.mark.parametrize("B", [96, 100])
def test_scrub_wide_is_scrub_erased_on_a_narrow_code(B):
    """The same verdicts, counts and bytes.  Both repairs treat [block_size, round_up(block_size, 16))
    as scratch, and they write it differently (8-byte lanes there, 16-byte lanes here): with
    block_size 96 there is no such scratch and the whole pitch is identical, padding included; with
    block_size 100 everything in [0, block_size) is."""
    k, m, pitch, G = 16, 4, 112, 120
    code, hd, hp = host_batch("cauchy", k, m, B, pitch, G)
    gm = random_loss_and_damage(np.random.default_rng(164), hd, hp, B)
    marks = to_dev(marks_to_rs_layout(gm, k))
    res = []
    for name in ("scrub_erased", "scrub_wide"):
        d, p = to_dev(hd), to_dev(hp)
        counts = torch.zeros(5, dtype=torch.int32, device=DEV)
        failed = torch.zeros(1, dtype=torch.int32, device=DEV)
        culprit = getattr(code, name)(d, p, marks, B, counts=counts, failed=failed)
        torch.cuda.synchronize()
        res.append([x.cpu().numpy() for x in (culprit, d, p, counts, failed)])
    same = B if B % 16 else pitch
    for i, (a, b) in enumerate(zip(*res)):
        assert np.array_equal(a[..., :same], b[..., :same]) if i in (1, 2) else np.array_equal(a, b)
    assert all((res[0][0] == v).any() for v in (CLEAN, MULTI, AMBIGUOUS, UNCHECKED, LOST)) and (res[0][0] >= 0).sum() >= 40
    assert not np.array_equal(res[0][1], hd)  # something was repaired


# ---------------------------------------------------------------- 6. refusals
def changed_rows():
    rows = qa.Code.cauchy(32, 8).rows.copy()
    rows[5, 17] ^= 0x01 if rows[5, 17] != 1 else 0x02
    return qa.Code.from_rows(rows)


@pytest.mark.parametrize("make,why", [(lambda: qa.Code.cauchy(40, 1), "m = 1"), (changed_rows, "not those qfec_code_new generates")])
def test_refused_codes(make, why):
    """QFEC_EUNSUP from every call; nothing is launched: every buffer is as it was."""
    code = make()
    n, stride = code.k + code.m, code.check_stride()
    d = torch.full((2, code.k, 64), 3, dtype=torch.uint8, device=DEV)
    p = torch.full((2, code.m, 64), 5, dtype=torch.uint8, device=DEV)
    marks = torch.zeros(2 * n, dtype=torch.uint8, device=DEV)
    marks[0] = 1
    culprit = torch.full((2,), 1234, dtype=torch.int32, device=DEV)
    counts = torch.full((5,), 7, dtype=torch.int32, device=DEV)
    out = torch.full((2 * n,), 0xEE, dtype=torch.uint8, device=DEV)
    plans = torch.full((2, stride), 0xEE, dtype=torch.uint8, device=DEV)
    with pytest.raises(qa.QfecError, match=why):
        code.locate_wide(d, p, marks, culprit=culprit, marks_out=out, counts=counts)
    with pytest.raises(qa.QfecError, match=why):
        code.scrub_wide(d, p, marks, culprit=culprit, counts=counts)
    with pytest.raises(qa.QfecError, match=why):
        code.check_build(marks, check_plan=plans)
    with pytest.raises(qa.QfecError, match=why):
        code.check_apply(d, p, plans, culprit=culprit, marks_out=out, counts=counts)
    torch.cuda.synchronize()
    assert bool((d == 3).all()) and bool((p == 5).all()) and bool((out == 0xEE).all()) and bool((plans == 0xEE).all())
    assert bool((culprit == 1234).all()) and bool((counts == 7).all()) and int(marks.sum()) == 1


def test_misaligned_check_plan_is_refused():
    """A slice of a tensor that starts off the 16-byte grid, in both calls; nothing is written."""
    code = qa.Code.cauchy(32, 8)
    stride = code.check_stride()
    flat = torch.full((2 * stride + 16,), 0xEE, dtype=torch.uint8, device=DEV)
    d = torch.full((2, 32, 64), 3, dtype=torch.uint8, device=DEV)
    p = torch.full((2, 8, 64), 5, dtype=torch.uint8, device=DEV)
    marks = torch.zeros(2 * 40, dtype=torch.uint8, device=DEV)
    culprit = torch.full((2,), 1234, dtype=torch.int32, device=DEV)
    for off in (1, 4, 8):
        plans = flat[off:off + 2 * stride].view(2, stride)
        with pytest.raises(qa.QfecError, match="d_check not 16-byte aligned"):
            code.check_build(marks, check_plan=plans)
        with pytest.raises(qa.QfecError, match="d_check not 16-byte aligned"):
            code.check_apply(d, p, plans, culprit=culprit)
    torch.cuda.synchronize()
    assert bool((flat == 0xEE).all()) and bool((culprit == 1234).all())
