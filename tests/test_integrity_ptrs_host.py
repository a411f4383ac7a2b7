"""CPU tests of the integrity family on pointer tables (qfec_verify_ptrs, qfec_locate_ptrs,
qfec_scrub_ptrs, include/qfec.h): every argument they refuse is refused on the host, with its cause in
qfec_last_error after the call's name, with stand-in pointers that are never dereferenced; every code
they refuse is refused before a device is asked for; what needs no device needs none; the Python
face's count and dtype checks; the coverage the GPU tests' shapes promise.  No kernel is launched here."""
import numpy as np
import pytest

import integrity_ptrs_common as ic
import quicknet_amd as qa

QFEC_OK, QFEC_EINVAL, QFEC_ENODEV, QFEC_EUNSUP = 0, -1, -2, -5
T, R, M, CN, F = 4096, 8192, 12288, 16384, 20480  # stand-ins for device pointers (never dereferenced)


def last_error():
    return qa.lib().qfec_last_error().decode()


def call(name, code, table, groups, block, out=R):
    """The call with stand-in outputs; `out` is d_bad_rows / d_culprit."""
    L = qa.lib()
    h = code._h if code is not None else None
    if name == "qfec_verify_ptrs":
        return L.qfec_verify_ptrs(h, table, groups, block, out, CN, None)
    if name == "qfec_locate_ptrs":
        return L.qfec_locate_ptrs(h, table, groups, block, out, M, CN, None)
    return L.qfec_scrub_ptrs(h, table, groups, block, out, CN, F, None)


CALLS = ["qfec_verify_ptrs", "qfec_locate_ptrs", "qfec_scrub_ptrs"]
REFUSED = [((T, -1, 16), "groups < 0"), ((T, 1, 0), "block_size < 1"), ((T, 1, -7), "block_size < 1"),
           ((None, 1, 16), "null d_shards")]


@pytest.mark.parametrize("name", CALLS)
@pytest.mark.parametrize("args,why", REFUSED)
def test_bad_arguments_are_refused_on_the_host(name, args, why):
    code = qa.Code.cauchy(10, 3)
    assert call(name, code, *args) == QFEC_EINVAL
    assert last_error().startswith(name + ":") and why in last_error(), last_error()


@pytest.mark.parametrize("name", CALLS)
def test_null_code_is_named(name):
    assert call(name, None, T, 1, 16) == QFEC_EINVAL
    assert last_error().startswith(name + ":") and "null code" in last_error(), last_error()


def test_locate_needs_its_culprits():
    code = qa.Code.cauchy(10, 3)
    assert call("qfec_locate_ptrs", code, T, 1, 16, out=None) == QFEC_EINVAL
    assert last_error().startswith("qfec_locate_ptrs:") and "null d_culprit" in last_error(), last_error()
    assert call("qfec_locate_ptrs", code, T, 0, 16, out=None) == QFEC_OK  # nothing to write


@pytest.mark.parametrize("k,m", [(4, 2), (20, 8), (32, 32)])
@pytest.mark.parametrize("name", CALLS)
def test_nothing_to_do_is_ok_without_a_device(name, k, m):
    """groups = 0: QFEC_OK with null buffers; a bad argument still wins."""
    code = qa.Code.cauchy(k, m)
    assert call(name, code, None, 0, 16, out=None) == QFEC_OK
    assert call(name, code, None, 0, 0, out=None) == QFEC_EINVAL
    assert "block_size < 1" in last_error()


def test_verify_without_outputs_needs_no_device():
    code = qa.Code.cauchy(60, 8)
    assert qa.lib().qfec_verify_ptrs(code._h, T, 5, 1400, None, None, None) == QFEC_OK


def test_verify_refuses_33_rows():
    code = qa.Code.cauchy(4, 33)
    for groups in (0, 1):
        assert call("qfec_verify_ptrs", code, T, groups, 16) == QFEC_EUNSUP
        assert last_error().startswith("qfec_verify_ptrs:") and "m = 33" in last_error(), last_error()


@pytest.mark.parametrize("name", ["qfec_locate_ptrs", "qfec_scrub_ptrs"])
@pytest.mark.parametrize("make,why", [(lambda: qa.Code.cauchy(4, 1), "m = 1"), (lambda: qa.Code.cauchy(33, 2), "k = 33"),
                                      (lambda: qa.Code.from_rows([[1, 2, 3], [1, 0, 5]]), "zero coefficient")])
def test_refused_codes(name, make, why):
    code = make()
    for groups in (0, 1):
        assert call(name, code, T, groups, 16) == QFEC_EUNSUP
        assert last_error().startswith(name + ":") and why in last_error(), last_error()


def test_scrub_refuses_an_edited_rs_handle():
    """One edit of rs->m: the scrub answers QFEC_EUNSUP on the host (the plan calls' refusal), the
    locate, which builds no plan, does not; the edit undone, the scrub accepts the code again."""
    rs = qa.ReedSolomon(6, 3)
    rs.m_matrix[7, 2] ^= 0x21
    code = rs.code()
    for groups in (0, 1):
        assert call("qfec_scrub_ptrs", code, T, groups, 16) == QFEC_EUNSUP
        assert last_error().startswith("qfec_scrub_ptrs:") and "edited handle" in last_error(), last_error()
    assert call("qfec_locate_ptrs", code, T, 0, 16) == QFEC_OK
    rs.m_matrix[7, 2] ^= 0x21
    assert call("qfec_scrub_ptrs", rs.code(), T, 0, 16) == QFEC_OK
    rs.close()


def no_gpu():
    if qa.device_count() > 0:
        pytest.skip("a GPU is present: the calls would run on the stand-in pointers")


def test_scrub_accepts_a_code_beyond_24_shards():
    """Code.cauchy(20, 8): qfec_scrub answers QFEC_EUNSUP (k + m > 24); qfec_scrub_ptrs accepts the code
    and gets as far as asking for a device."""
    no_gpu()
    code = qa.Code.cauchy(20, 8)
    assert qa.lib().qfec_scrub(code._h, T, R, 1, 16, 16, None, None, None) == QFEC_EUNSUP
    assert call("qfec_scrub_ptrs", code, T, 1, 16) == QFEC_ENODEV
    assert call("qfec_scrub_ptrs", code, T, 1, 16, out=None) == QFEC_ENODEV


@pytest.mark.parametrize("name,k,m", [("qfec_verify_ptrs", 10, 3), ("qfec_verify_ptrs", 60, 8), ("qfec_verify_ptrs", 200, 32),
                                      ("qfec_locate_ptrs", 10, 3), ("qfec_locate_ptrs", 32, 32),
                                      ("qfec_scrub_ptrs", 10, 3), ("qfec_scrub_ptrs", 32, 32)])
def test_a_well_formed_call_asks_for_a_device(name, k, m):
    no_gpu()
    assert call(name, qa.Code.cauchy(k, m), T, 3, 1400) == QFEC_ENODEV


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
    code = qa.Code.cauchy(10, 3)
    calls = {"verify_ptrs": (code.verify_ptrs, "bad_rows"), "locate_ptrs": (code.locate_ptrs, "culprit"),
             "scrub_ptrs": (code.scrub_ptrs, "culprit")}
    for what, (fn, out) in calls.items():
        with pytest.raises(qa.QfecError, match=r"not groups \* \(k \+ m\)"):
            fn(_Fake(27), 16)
        with pytest.raises(qa.QfecError, match=f"{what}: {out} has 3 elements for 2 groups"):
            fn(_Fake(26), 16, **{out: _Fake(3, torch.int32)})
        with pytest.raises(qa.QfecError, match=f"{what}: {out} has dtype"):
            fn(_Fake(26), 16, **{out: _Fake(2, torch.int64)})
    for fn in (code.locate_ptrs, code.scrub_ptrs):
        with pytest.raises(qa.QfecError, match="counts has 2 elements, not 3"):
            fn(_Fake(26), 16, culprit=_Fake(2, torch.int32), counts=_Fake(2))
    with pytest.raises(qa.QfecError, match="marks has 25 elements for 2 groups of 13"):
        code.locate_ptrs(_Fake(26), 16, culprit=_Fake(2, torch.int32), marks=_Fake(25))


def test_shapes_cover_what_the_gpu_tests_promise():
    """Every code at B = 17, 1025 and 1400, every alignment mode at (10,3) and (9,5), every block size,
    both group counts; the draw is seeded, so the GPU run walks these cells."""
    cells = ic.cells()
    ic.assert_coverage(cells)
    assert cells == ic.cells() and len(cells) == len(set(cells))
    assert all(k + m > 64 for k, m in ic.VERIFY_ONLY) and all(k + m == 64 for k, m in ic.LOCATE_ONLY)
    for B in ic.BLOCKS:
        s = ic.spots(B)
        assert all(0 <= b < B for where in s.values() for b in where)
        assert ("tail" in s) == (B % 16 != 0) and ("col-end" in s) == (B >= 16) and ("two-slabs" in s) == (B > 1024)
        if "two-slabs" in s:
            assert s["two-slabs"][0] < 1024 <= s["two-slabs"][1]


def test_expected_bits_follow_the_damage():
    """The CPU expectation itself: a parity row names its own bit, a data shard every bit."""
    code = qa.Code.cauchy(9, 5)
    G, B = 7, 33
    pool, img = ic.batch(code, B, "residues", G)
    assert not ic.expected_bits(code, pool, img, G).any()
    ic.hit(pool, img, ic.row_id(G, 9, 5, 2, 9 + 3), [B - 1], 1)
    ic.hit(pool, img, ic.row_id(G, 9, 5, 5, 4), [0], 2)
    assert list(ic.expected_bits(code, pool, img, G)) == [0, 0, 8, 0, 0, 31, 0]
    assert np.array_equal(img[pool.start[0] - 1:pool.start[0]], [0xC3])  # the guards are where they were
