"""CPU tests of single-shard error location with per-shard lengths at any k + m on shard pointer tables
(qfec_check_apply_ptrs_var, qfec_locate_ptrs_wide_var, qfec_scrub_ptrs_wide_var, include/qfec.h): the
symbols are exported; every argument they refuse is refused on the host, with its cause in
qfec_last_error after the call's name, with stand-in pointers that are never dereferenced; every code
they refuse is refused before a device is asked for, also with zero groups and null buffers; what needs
no device needs none; the Python face's count and dtype checks; the numpy model of the definition
against the models it must agree with; and that the batches of the GPU tests hold every verdict class.
No kernel is launched here."""
import re

import numpy as np
import pytest

import integrity_ptrs_var_common as iv
import locate_ptrs_wide_var_common as lv
import locate_wide_common as lw
import quicknet_amd as qa
from quicknet_amd._lib import EXPORTS

QFEC_OK, QFEC_EINVAL, QFEC_ENODEV, QFEC_EUNSUP = 0, -1, -2, -5
# stand-ins for device pointers
T, LN, GL, CK, M, C, MO, CN, F, IV = 4096, 8192, 12288, 16384, 20480, 24576, 28672, 32768, 36864, 40960
CALLS = ["qfec_check_apply_ptrs_var", "qfec_locate_ptrs_wide_var", "qfec_scrub_ptrs_wide_var"]
LOCATES = CALLS[:2]


def last_error():
    return qa.lib().qfec_last_error().decode()


def call(name, code, table=T, lens=LN, glen=GL, groups=1, max_len=16, check=CK, culprit=C):
    """The call with stand-in buffers; `check` is d_check (qfec_check_apply_ptrs_var only)."""
    L = qa.lib()
    h = code._h if code is not None else None
    if name == "qfec_check_apply_ptrs_var":
        return L.qfec_check_apply_ptrs_var(h, table, lens, glen, check, groups, max_len, culprit, MO, CN, IV, None)
    if name == "qfec_locate_ptrs_wide_var":
        return L.qfec_locate_ptrs_wide_var(h, table, lens, glen, M, groups, max_len, culprit, MO, CN, IV, None)
    return L.qfec_scrub_ptrs_wide_var(h, table, lens, glen, M, groups, max_len, culprit, CN, F, IV, None)


def empty(name, code):
    """Zero groups and null buffers."""
    return getattr(qa.lib(), name)(code._h, None, None, None, None, 0, 16, None, None, None, None, None)


def test_the_three_symbols_are_exported():
    L = qa.lib()
    for name in CALLS:
        assert name in EXPORTS["qfec.h"] and hasattr(L, name)


REFUSED = [(dict(groups=-1), "groups < 0"), (dict(max_len=0), "max_len < 1"), (dict(max_len=-7), "max_len < 1"),
           (dict(table=None), "null d_shards"), (dict(lens=None), "null d_lens"), (dict(glen=None), "null d_group_len")]


@pytest.mark.parametrize("name", CALLS)
@pytest.mark.parametrize("args,why", REFUSED)
def test_bad_arguments_are_refused_on_the_host(name, args, why):
    code = qa.Code.cauchy(70, 10)
    assert call(name, code, **args) == QFEC_EINVAL
    assert last_error().startswith(name + ":") and why in last_error(), last_error()


@pytest.mark.parametrize("name", CALLS)
def test_null_code_is_named(name):
    assert call(name, None) == QFEC_EINVAL
    assert last_error().startswith(name + ":") and "null code" in last_error(), last_error()


@pytest.mark.parametrize("name", LOCATES)
def test_the_locates_need_their_culprits(name):
    code = qa.Code.cauchy(32, 8)
    assert call(name, code, culprit=None) == QFEC_EINVAL
    assert last_error().startswith(name + ":") and "null d_culprit" in last_error(), last_error()
    assert call(name, code, groups=0, culprit=None) == QFEC_OK  # nothing to write


def test_the_apply_needs_an_aligned_check_plan():
    code = qa.Code.cauchy(32, 8)
    name = "qfec_check_apply_ptrs_var"
    assert call(name, code, check=None) == QFEC_EINVAL
    assert last_error().startswith(name + ":") and "null d_check" in last_error(), last_error()
    for off in (1, 4, 8, 15):
        for groups in (0, 1):
            assert call(name, code, groups=groups, check=CK + off) == QFEC_EINVAL
            assert last_error().startswith(name + ":") and "d_check not 16-byte aligned" in last_error(), last_error()
    assert call(name, code, groups=0, check=None) == QFEC_OK


def assert_refused(code, why):
    for name in CALLS:
        for rc in (call(name, code), empty(name, code)):
            assert rc == QFEC_EUNSUP, name
            assert last_error().startswith(name + ":") and re.search(why, last_error()), last_error()


@pytest.mark.parametrize("k,m", [(4, 1), (254, 1)])
def test_one_parity_row_is_refused(k, m):
    assert_refused(qa.Code.cauchy(k, m), "m = 1 < 2")


@pytest.mark.parametrize("k,m,row,col", [(4, 2, 0, 0), (32, 8, 7, 31), (200, 55, 54, 199)])
def test_one_changed_byte_is_refused(k, m, row, col):
    for flavour in ("cauchy", "vandermonde"):
        rows = getattr(qa.Code, flavour)(k, m).rows.copy()
        rows[row, col] ^= 0x01 if rows[row, col] != 1 else 0x02  # still non-zero
        assert_refused(qa.Code.from_rows(rows), "not those qfec_code_new generates")


def test_rs_handle_is_accepted_until_edited():
    rs = qa.ReedSolomon(6, 3)
    for name in CALLS:
        assert empty(name, rs.code()) == QFEC_OK
    rs.m_matrix[7, 2] ^= 0x21
    assert_refused(rs.code(), "decode matrix|not those qfec_code_new generates")
    rs.m_matrix[7, 2] ^= 0x21
    for name in CALLS:
        assert empty(name, rs.code()) == QFEC_OK
    rs.close()


@pytest.mark.parametrize("k,m", [(4, 2), (10, 3), (64, 16), (200, 55), (128, 127)])
@pytest.mark.parametrize("name", CALLS)
def test_nothing_to_do_is_ok_without_a_device(name, k, m):
    """groups = 0: QFEC_OK with null buffers, narrow codes included; a bad argument still wins."""
    for flavour in ("cauchy", "vandermonde"):
        code = getattr(qa.Code, flavour)(k, m)
        assert empty(name, code) == QFEC_OK
        assert call(name, code, table=None, lens=None, glen=None, groups=0, max_len=0, culprit=None) == QFEC_EINVAL
        assert "max_len < 1" in last_error()


@pytest.mark.parametrize("name", CALLS)
@pytest.mark.parametrize("k,m", [(10, 3), (64, 16), (200, 55)])
def test_a_well_formed_call_asks_for_a_device(name, k, m):
    if qa.device_count() > 0:
        pytest.skip("a GPU is present: the calls would run on the stand-in pointers")
    assert call(name, qa.Code.cauchy(k, m), groups=3, max_len=1400) == QFEC_ENODEV


class _Fake:
    """What the Python face looks at before it reaches for a device pointer."""

    def __init__(self, n, dtype=None):
        self._n = n
        self.shape = (n,)
        self.dtype = dtype

    def dim(self):
        return 1

    def numel(self):
        return self._n


def test_python_face_checks_counts_and_dtypes():
    torch = pytest.importorskip("torch")
    code = qa.Code.cauchy(32, 8)
    stride = code.check_stride()
    ok = _Fake(2, torch.int32)
    lens, glen = _Fake(64, torch.int32), _Fake(2, torch.int32)
    faces = {"check_apply_ptrs_var": lambda p, lens=lens, glen=glen, **kw:
             code.check_apply_ptrs_var(p, lens, glen, _Fake(2 * stride), 16, **kw),
             "locate_ptrs_wide_var": lambda p, lens=lens, glen=glen, **kw: code.locate_ptrs_wide_var(p, lens, glen, 16, **kw),
             "scrub_ptrs_wide_var": lambda p, lens=lens, glen=glen, **kw: code.scrub_ptrs_wide_var(p, lens, glen, 16, **kw)}
    for what, fn in faces.items():
        with pytest.raises(qa.QfecError, match=r"not groups \* \(k \+ m\)"):
            fn(_Fake(81))
        with pytest.raises(qa.QfecError, match=f"{what}: culprit has 3 elements for 2 groups"):
            fn(_Fake(80), culprit=_Fake(3, torch.int32))
        with pytest.raises(qa.QfecError, match=f"{what}: culprit has dtype"):
            fn(_Fake(80), culprit=_Fake(2, torch.int64))
        with pytest.raises(qa.QfecError, match=f"{what}: counts has 3 elements, not 5"):
            fn(_Fake(80), culprit=ok, counts=_Fake(3))
        with pytest.raises(qa.QfecError, match=f"{what}: lens"):
            fn(_Fake(80), culprit=ok, lens=_Fake(63, torch.int32))
        with pytest.raises(qa.QfecError, match=f"{what}: lens"):
            fn(_Fake(80), culprit=ok, lens=_Fake(64, torch.int64))
        with pytest.raises(qa.QfecError, match=f"{what}: group_len"):
            fn(_Fake(80), culprit=ok, glen=_Fake(3, torch.int32))
    for what in ("locate_ptrs_wide_var", "scrub_ptrs_wide_var"):
        with pytest.raises(qa.QfecError, match=f"{what}: marks has 79 elements for 2 groups of 40"):
            faces[what](_Fake(80), culprit=ok, marks=_Fake(79))
    for what in ("check_apply_ptrs_var", "locate_ptrs_wide_var"):
        with pytest.raises(qa.QfecError, match=f"{what}: marks_out has 81 elements for 2 groups of 40"):
            faces[what](_Fake(80), culprit=ok, marks_out=_Fake(81))
    with pytest.raises(qa.QfecError, match=f"check_apply_ptrs_var: check_plan has {stride} bytes for 2 groups of {stride}"):
        code.check_apply_ptrs_var(_Fake(80), lens, glen, _Fake(stride), 16, culprit=ok)


# ---------------------------------------------------------------- the model against its neighbours
@pytest.mark.parametrize("k,m,max_len", [(10, 3, 17), (32, 8, 1025), (70, 10, 17)])
def test_with_all_lengths_equal_the_model_is_the_fixed_length_model(k, m, max_len):
    """The valid groups of the family batch, every data row taken as max_len bytes long (the bytes are the
    same: the rows are zero from their own end on)."""
    case = lv.family(k, m, max_len)
    keep = np.flatnonzero(~case.bad & (case.glen > 0))
    lens = np.full((len(keep), k), max_len, np.int64)
    glen = np.full(len(keep), max_len, np.int64)
    got = lv.model(case.code, case.hd[keep], case.hp[keep], case.gm[keep], lens, glen, max_len)
    want = lw.model(case.code, case.hd[keep], case.hp[keep], case.gm[keep], max_len)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and list(got[2]) == list(want[2])
    assert got[3] == 0 and (got[0] >= 0).sum() > 5


@pytest.mark.parametrize("k,m", [(10, 3), (16, 4)])
@pytest.mark.parametrize("max_len", [17, 1025])
def test_without_marks_the_model_is_the_narrow_model(k, m, max_len):
    """integrity_ptrs_var_common's batches (complete groups, cycling lengths, invalid groups among them)
    under its damage kinds, the length condition included: the same verdicts from both models."""
    code = qa.Code.cauchy(k, m)
    b, img = iv.batch(code, max_len, "aligned")
    lens, glen = b.lens.copy(), b.glen.copy()
    rng = np.random.default_rng(k + max_len)
    for g in range(b.G):
        live = [c for c in range(k + m) if b.span(g, c)[1] > 0]
        if g % 3 == 0 or not live:
            continue
        for c in rng.choice(live, size=1 + (g % 5 == 1), replace=False):
            n = b.span(g, int(c))[1]
            b.hit(img, g, int(c), [int(rng.integers(0, n))], g)
    # a parity byte past a short shard's end that the shard alone would explain elsewhere: wrong past its end
    d, p = iv.padded_rows(b, img)
    want, wcounts, winv = iv.model_locate(b, img)
    gm = np.zeros((b.G, k + m), np.uint8)
    got = lv.model(code, d, p, gm, lens, glen, max_len)
    assert np.array_equal(got[0], want), np.nonzero(got[0] != want)[0]
    assert list(got[2][:3]) == wcounts and not got[2][3:].any() and got[3] == winv
    assert (want >= 0).any() and (want == lv.MULTI).any() and (want == lv.CLEAN).any()


def test_wrong_past_its_own_end_in_both_models():
    """One group of (10,3): the parity says data shard 4 holds a byte at its own end.  Padded, the fixed
    model names shard 4; both models with lengths say MULTI."""
    k, m, max_len = 10, 3, 40
    code = qa.Code.cauchy(k, m)
    lens = np.full(k, max_len, np.int64)
    lens[4] = 21
    spec = dict(lens=lens, L=max_len, marks=np.zeros(k + m, np.uint8), phantom=[(4, 21, 0x6C)])
    case = lv.make(code, [spec], max_len, "aligned", 3)
    padded = case.hd.copy()
    padded[0, 4, 21] = 0x6C
    assert lw.model(code, padded, case.hp, case.gm, max_len)[0][0] == lv.CLEAN
    assert lw.model(code, case.hd, case.hp, case.gm, max_len)[0][0] == 4
    assert case.expect()[0][0] == lv.MULTI


# ---------------------------------------------------------------- what the GPU batches hold
@pytest.mark.parametrize("k,m,max_len", lv.FAMILY)
def test_the_gpu_batches_hold_every_verdict_class(k, m, max_len):
    lv.assert_family_covers(lv.family(k, m, max_len))
