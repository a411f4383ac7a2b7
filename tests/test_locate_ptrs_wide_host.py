"""CPU tests of single-shard error location at any k + m on shard pointer tables
(qfec_check_apply_ptrs, qfec_locate_ptrs_wide, qfec_scrub_ptrs_wide, include/qfec.h): the symbols are
exported; every argument they refuse is refused on the host, with its cause in qfec_last_error after
the call's name, with stand-in pointers that are never dereferenced; every code they refuse is refused
before a device is asked for, also with zero groups and null buffers; what needs no device needs
none; the Python face's count and dtype checks.  No kernel is launched here."""
import re

import numpy as np
import pytest

import quicknet_amd as qa
from quicknet_amd._lib import EXPORTS

QFEC_OK, QFEC_EINVAL, QFEC_ENODEV, QFEC_EUNSUP = 0, -1, -2, -5
T, CK, M, C, MO, CN, F = 4096, 8192, 12288, 16384, 20480, 24576, 28672  # stand-ins for device pointers
CALLS = ["qfec_check_apply_ptrs", "qfec_locate_ptrs_wide", "qfec_scrub_ptrs_wide"]
LOCATES = CALLS[:2]


def last_error():
    return qa.lib().qfec_last_error().decode()


def call(name, code, table=T, groups=1, block=16, check=CK, culprit=C):
    """The call with stand-in buffers; `check` is d_check (qfec_check_apply_ptrs only)."""
    L = qa.lib()
    h = code._h if code is not None else None
    if name == "qfec_check_apply_ptrs":
        return L.qfec_check_apply_ptrs(h, table, check, groups, block, culprit, MO, CN, None)
    if name == "qfec_locate_ptrs_wide":
        return L.qfec_locate_ptrs_wide(h, table, M, groups, block, culprit, MO, CN, None)
    return L.qfec_scrub_ptrs_wide(h, table, M, groups, block, culprit, CN, F, None)


def empty(name, code):
    """Zero groups and null buffers."""
    L, h = qa.lib(), code._h
    if name == "qfec_scrub_ptrs_wide":
        return L.qfec_scrub_ptrs_wide(h, None, None, 0, 16, None, None, None, None)
    return getattr(L, name)(h, None, None, 0, 16, None, None, None, None)


def test_the_three_symbols_are_exported():
    L = qa.lib()
    for name in CALLS:
        assert name in EXPORTS["qfec.h"] and hasattr(L, name)


REFUSED = [(dict(groups=-1), "groups < 0"), (dict(block=0), "block_size < 1"), (dict(block=-7), "block_size < 1"),
           (dict(table=None), "null d_shards")]


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
    name = "qfec_check_apply_ptrs"
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
        assert call(name, code, table=None, groups=0, block=0, culprit=None) == QFEC_EINVAL
        assert "block_size < 1" in last_error()


@pytest.mark.parametrize("name", CALLS)
@pytest.mark.parametrize("k,m", [(10, 3), (64, 16), (200, 55)])
def test_a_well_formed_call_asks_for_a_device(name, k, m):
    if qa.device_count() > 0:
        pytest.skip("a GPU is present: the calls would run on the stand-in pointers")
    assert call(name, qa.Code.cauchy(k, m), groups=3, block=1400) == QFEC_ENODEV


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
    faces = {"check_apply_ptrs": lambda p, **kw: code.check_apply_ptrs(p, _Fake(2 * stride), 16, **kw),
             "locate_ptrs_wide": lambda p, **kw: code.locate_ptrs_wide(p, 16, **kw),
             "scrub_ptrs_wide": lambda p, **kw: code.scrub_ptrs_wide(p, 16, **kw)}
    for what, fn in faces.items():
        with pytest.raises(qa.QfecError, match=r"not groups \* \(k \+ m\)"):
            fn(_Fake(81))
        with pytest.raises(qa.QfecError, match=f"{what}: culprit has 3 elements for 2 groups"):
            fn(_Fake(80), culprit=_Fake(3, torch.int32))
        with pytest.raises(qa.QfecError, match=f"{what}: culprit has dtype"):
            fn(_Fake(80), culprit=_Fake(2, torch.int64))
        with pytest.raises(qa.QfecError, match=f"{what}: counts has 3 elements, not 5"):
            fn(_Fake(80), culprit=ok, counts=_Fake(3))
    for what in ("locate_ptrs_wide", "scrub_ptrs_wide"):
        with pytest.raises(qa.QfecError, match=f"{what}: marks has 79 elements for 2 groups of 40"):
            faces[what](_Fake(80), culprit=ok, marks=_Fake(79))
    for what in ("check_apply_ptrs", "locate_ptrs_wide"):
        with pytest.raises(qa.QfecError, match=f"{what}: marks_out has 81 elements for 2 groups of 40"):
            faces[what](_Fake(80), culprit=ok, marks_out=_Fake(81))
    with pytest.raises(qa.QfecError, match=f"check_apply_ptrs: check_plan has {stride} bytes for 2 groups of {stride}"):
        code.check_apply_ptrs(_Fake(80), _Fake(stride), 16, culprit=ok)
