"""CPU tests of the integrity family on pointer tables with per-shard lengths (qfec_verify_ptrs_var,
qfec_locate_ptrs_var, qfec_scrub_ptrs_var, include/qfec.h): every argument they refuse is refused on the
host, with its cause in qfec_last_error after the call's name, with stand-in pointers that are never
dereferenced; every code they refuse is refused before a device is asked for; what needs no device
needs none; the scrub accepts what qfec_scrub_ptrs' plan half refuses; the Python face's count and
dtype checks; the CPU model the GPU tests expect against, held to the fixed-length expectation and to a
hand-built beyond-length group; the coverage the GPU tests' shapes promise.  No kernel is launched here."""
import numpy as np
import pytest

import integrity_ptrs_common as ic
import integrity_ptrs_var_common as iv
import quicknet_amd as qa
from locate2_common import mul_table

QFEC_OK, QFEC_EINVAL, QFEC_ENODEV, QFEC_EUNSUP = 0, -1, -2, -5
T, LN, GL, R, M, CN, IV = 4096, 8192, 12288, 16384, 20480, 24576, 28672  # stand-ins for device pointers


def last_error():
    return qa.lib().qfec_last_error().decode()


def call(name, code, table, lens, glen, groups, max_len, out=R):
    """The call with stand-in outputs; `out` is d_bad_rows / d_culprit."""
    L = qa.lib()
    h = code._h if code is not None else None
    if name == "qfec_verify_ptrs_var":
        return L.qfec_verify_ptrs_var(h, table, lens, glen, groups, max_len, out, CN, IV, None)
    if name == "qfec_locate_ptrs_var":
        return L.qfec_locate_ptrs_var(h, table, lens, glen, groups, max_len, out, M, CN, IV, None)
    return L.qfec_scrub_ptrs_var(h, table, lens, glen, groups, max_len, out, CN, IV, None)


CALLS = ["qfec_verify_ptrs_var", "qfec_locate_ptrs_var", "qfec_scrub_ptrs_var"]
REFUSED = [((T, LN, GL, -1, 16), "groups < 0"), ((T, LN, GL, 1, 0), "max_len < 1"), ((T, LN, GL, 1, -7), "max_len < 1"),
           ((None, LN, GL, 1, 16), "null d_shards"), ((T, None, GL, 1, 16), "null d_lens"),
           ((T, LN, None, 1, 16), "null d_group_len")]


def test_the_constant():
    assert qa.LOC_INVALID == qa.QFEC_LOC_INVALID == iv.INVALID == -6
    assert len({qa.QFEC_LOC_CLEAN, qa.QFEC_LOC_MULTI, qa.QFEC_LOC_AMBIGUOUS, qa.QFEC_LOC_UNCHECKED, qa.QFEC_LOC_LOST,
                qa.LOC_INVALID}) == 6


@pytest.mark.parametrize("name", CALLS)
@pytest.mark.parametrize("args,why", REFUSED)
def test_bad_arguments_are_refused_on_the_host(name, args, why):
    code = qa.Code.cauchy(10, 3)
    assert call(name, code, *args) == QFEC_EINVAL
    assert last_error().startswith(name + ":") and why in last_error(), last_error()


@pytest.mark.parametrize("name", CALLS)
def test_null_code_is_named(name):
    assert call(name, None, T, LN, GL, 1, 16) == QFEC_EINVAL
    assert last_error().startswith(name + ":") and "null code" in last_error(), last_error()


def test_locate_needs_its_culprits():
    code = qa.Code.cauchy(10, 3)
    assert call("qfec_locate_ptrs_var", code, T, LN, GL, 1, 16, out=None) == QFEC_EINVAL
    assert last_error().startswith("qfec_locate_ptrs_var:") and "null d_culprit" in last_error(), last_error()
    assert call("qfec_locate_ptrs_var", code, T, LN, GL, 0, 16, out=None) == QFEC_OK  # nothing to write


@pytest.mark.parametrize("k,m", [(4, 2), (20, 8), (32, 32)])
@pytest.mark.parametrize("name", CALLS)
def test_nothing_to_do_is_ok_without_a_device(name, k, m):
    """groups = 0: QFEC_OK with null buffers; a bad argument still wins."""
    code = qa.Code.cauchy(k, m)
    assert call(name, code, None, None, None, 0, 16, out=None) == QFEC_OK
    assert call(name, code, None, None, None, 0, 0, out=None) == QFEC_EINVAL
    assert "max_len < 1" in last_error()
    assert call(name, code, None, None, None, -1, 16, out=None) == QFEC_EINVAL


def test_verify_without_outputs_needs_no_device():
    code = qa.Code.cauchy(60, 8)
    assert qa.lib().qfec_verify_ptrs_var(code._h, T, LN, GL, 5, 1400, None, None, None, None) == QFEC_OK


def test_verify_refuses_33_rows():
    code = qa.Code.cauchy(4, 33)
    for groups in (0, 1):
        assert call("qfec_verify_ptrs_var", code, T, LN, GL, groups, 16) == QFEC_EUNSUP
        assert last_error().startswith("qfec_verify_ptrs_var:") and "m = 33" in last_error(), last_error()


@pytest.mark.parametrize("name", ["qfec_locate_ptrs_var", "qfec_scrub_ptrs_var"])
@pytest.mark.parametrize("make,why", [(lambda: qa.Code.cauchy(4, 1), "m = 1"), (lambda: qa.Code.cauchy(33, 2), "k = 33"),
                                      (lambda: qa.Code.from_rows([[1, 2, 3], [1, 0, 5]]), "zero coefficient")])
def test_refused_codes(name, make, why):
    code = make()
    for groups in (0, 1):
        assert call(name, code, T, LN, GL, groups, 16) == QFEC_EUNSUP
        assert last_error().startswith(name + ":") and why in last_error(), last_error()


def no_gpu():
    if qa.device_count() > 0:
        pytest.skip("a GPU is present: the calls would run on the stand-in pointers")


def test_scrub_accepts_an_edited_rs_handle():
    """One edit of rs->m: qfec_scrub_ptrs answers QFEC_EUNSUP (its plan half), qfec_scrub_ptrs_var builds
    no plan and accepts the code: QFEC_OK with nothing to do, and with work as far as asking for a device."""
    rs = qa.ReedSolomon(6, 3)
    rs.m_matrix[7, 2] ^= 0x21
    code = rs.code()
    assert qa.lib().qfec_scrub_ptrs(code._h, T, 0, 16, None, None, None, None) == QFEC_EUNSUP
    assert call("qfec_scrub_ptrs_var", code, T, LN, GL, 0, 16) == QFEC_OK
    if qa.device_count() == 0:
        assert call("qfec_scrub_ptrs_var", code, T, LN, GL, 1, 16) == QFEC_ENODEV
    rs.close()


def test_scrub_accepts_a_code_beyond_24_shards():
    no_gpu()
    code = qa.Code.cauchy(20, 8)
    assert qa.lib().qfec_scrub(code._h, T, R, 1, 16, 16, None, None, None) == QFEC_EUNSUP
    assert call("qfec_scrub_ptrs_var", code, T, LN, GL, 1, 16) == QFEC_ENODEV
    assert call("qfec_scrub_ptrs_var", code, T, LN, GL, 1, 16, out=None) == QFEC_ENODEV


@pytest.mark.parametrize("name,k,m", [("qfec_verify_ptrs_var", 10, 3), ("qfec_verify_ptrs_var", 60, 8),
                                      ("qfec_verify_ptrs_var", 200, 32), ("qfec_locate_ptrs_var", 10, 3),
                                      ("qfec_locate_ptrs_var", 32, 32), ("qfec_scrub_ptrs_var", 10, 3),
                                      ("qfec_scrub_ptrs_var", 32, 32)])
def test_a_well_formed_call_asks_for_a_device(name, k, m):
    no_gpu()
    assert call(name, qa.Code.cauchy(k, m), T, LN, GL, 3, 1400) == QFEC_ENODEV


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
    i32 = torch.int32
    lens, glen = _Fake(20, i32), _Fake(2, i32)
    calls = {"verify_ptrs_var": (code.verify_ptrs_var, "bad_rows"), "locate_ptrs_var": (code.locate_ptrs_var, "culprit"),
             "scrub_ptrs_var": (code.scrub_ptrs_var, "culprit")}
    for what, (fn, out) in calls.items():
        with pytest.raises(qa.QfecError, match=r"not groups \* \(k \+ m\)"):
            fn(_Fake(27), lens, glen, 16)
        with pytest.raises(qa.QfecError, match=f"{what}: {out} has 3 elements for 2 groups"):
            fn(_Fake(26), lens, glen, 16, **{out: _Fake(3, i32)})
        with pytest.raises(qa.QfecError, match=f"{what}: {out} has dtype"):
            fn(_Fake(26), lens, glen, 16, **{out: _Fake(2, torch.int64)})
        with pytest.raises(qa.QfecError, match=f"{what}: lens has 19 elements, 20 expected"):
            fn(_Fake(26), _Fake(19, i32), glen, 16, **{out: _Fake(2, i32)})
        with pytest.raises(qa.QfecError, match=f"{what}: lens has dtype"):
            fn(_Fake(26), _Fake(20, torch.int64), glen, 16, **{out: _Fake(2, i32)})
        with pytest.raises(qa.QfecError, match=f"{what}: group_len has 3 elements, 2 expected"):
            fn(_Fake(26), lens, _Fake(3, i32), 16, **{out: _Fake(2, i32)})
        with pytest.raises(qa.QfecError, match=f"{what}: group_len has dtype"):
            fn(_Fake(26), lens, _Fake(2, torch.int16), 16, **{out: _Fake(2, i32)})
    for fn in (code.locate_ptrs_var, code.scrub_ptrs_var):
        with pytest.raises(qa.QfecError, match="counts has 2 elements, not 3"):
            fn(_Fake(26), lens, glen, 16, culprit=_Fake(2, i32), counts=_Fake(2))
    with pytest.raises(qa.QfecError, match="marks has 25 elements for 2 groups of 13"):
        code.locate_ptrs_var(_Fake(26), lens, glen, 16, culprit=_Fake(2, i32), marks=_Fake(25))


# ---------------------------------------------------------------- the shapes and the CPU model

def test_shapes_cover_what_the_gpu_tests_promise():
    cells = iv.cells()
    iv.assert_coverage(cells)
    assert cells == iv.cells() and len(cells) == len(set(cells))
    for k, m in iv.TEMPLATED + iv.RUNTIME + iv.SCRUB_ONLY:
        for ml in iv.MAX_LENS:
            lens, glen = iv.cycle_lengths(k, ml)
            assert len(iv.patterns(k, ml)) <= iv.G, "every pattern occurs in a batch"
            assert not iv.invalid_groups(lens, glen, ml).any()
    for n in (1, 15, 16, 17, 1024, 1025, 1400):
        s = iv.spots(n)
        assert all(0 <= b < n for where in s.values() for b in where)
        assert ("part" in s) == (n % 16 != 0) and ("col-end" in s) == (n >= 16) and ("two-slabs" in s) == (n > 1024)


def test_invalid_groups_are_judged_on_every_length():
    lens = np.array([[5, 5], [5, 6], [5, -1], [0, 0], [0, 0], [3, 3], [iv.INT_MAX, 1], [1, iv.INT_MIN]])
    glen = np.array([5, 5, 5, 0, -1, 9, 8, 8])
    assert list(iv.invalid_groups(lens, glen, 8)) == [False, True, True, False, True, True, True, True]


@pytest.mark.parametrize("k,m,ml", [(9, 5, 33), (10, 3, 1025)])
def test_the_model_on_equal_lengths_is_the_fixed_length_expectation(k, m, ml):
    """All lengths = max_len: the model's verify bits are integrity_ptrs_common.expected_bits of the same
    rows, its verdicts follow the damage, and its scrub gives the undamaged image back."""
    code = qa.Code.cauchy(k, m)
    Gn = 9
    b = iv.Batch(code.rows, ml, "residues", np.full((Gn, k), ml), np.full(Gn, ml), seed=5)
    pool = b.vp.pool
    img = b.host.copy()
    assert not ic.expected_bits(code, pool, img, Gn).any()
    b.hit(img, 2, k + m - 1, [ml - 1], 1)
    b.hit(img, 5, 4, [0, ml // 2], 2)
    b.hit(img, 7, 1, [3], 3)
    b.hit(img, 7, k, [3], 4)
    rows, bad, inv = iv.model_verify(b, img)
    assert np.array_equal(rows, ic.expected_bits(code, pool, img, Gn)) and bad == 3 and inv == 0
    assert list(rows) == [0, 0, 1 << (m - 1), 0, 0, (1 << m) - 1, 0, (1 << m) - 1, 0]
    culprit, counts, inv = iv.model_locate(b, img)
    assert list(culprit) == [-1, -1, k + m - 1, -1, -1, 4, -1, iv.MULTI, -1] and counts == [2, 1, 0] and inv == 0
    want = b.host.copy()
    for c in range(k + m):
        s, n = b.span(7, c)
        want[s:s + n] = img[s:s + n]
    assert np.array_equal(iv.model_scrub(b, img)[3], want)


def test_the_model_on_a_hand_built_beyond_length_group():
    """rows [[1, 2, 3], [1, 4, 5]] (not the oracle's: plain products by hand), max_len 8, shard 1 three
    bytes long.  e x column 1 XORed into the parity at byte 5 is what a corrupted byte 5 of shard 1
    would look like on padded rows, but shard 1 has no byte 5: MULTI.  The same at byte 2: shard 1."""
    mul = mul_table()
    code = qa.Code.from_rows([[1, 2, 3], [1, 4, 5]])
    lens, glen = np.array([[8, 3, 6]] * 4), np.array([8] * 4)
    b = iv.Batch(code.rows, 8, "aligned", lens, glen, seed=9)
    img = b.host.copy()
    assert list(iv.model_locate(b, img)[0]) == [iv.CLEAN] * 4
    e = 0x5D
    for g, byte in ((1, 5), (2, 2)):
        for j in range(2):
            img[b.span(g, 3 + j)[0] + byte] ^= mul[int(code.rows[j, 1]), e]
    img[b.span(3, 1)[0] + 3] ^= 0xFF  # a byte past the end of shard 1: read by nobody
    culprit, counts, inv = iv.model_locate(b, img)
    assert list(culprit) == [iv.CLEAN, iv.MULTI, 1, iv.CLEAN] and counts == [1, 1, 0] and inv == 0
    assert list(iv.model_verify(b, img)[0]) == [0, 3, 3, 0]
    _, _, _, after = iv.model_scrub(b, img)
    want = img.copy()
    s, _ = b.span(2, 1)
    want[s + 2] ^= e  # the correction of group 2 writes e into byte 2 of shard 1, and nothing else
    assert np.array_equal(after, want)
    # the padded-rows locate alone (no beyond-length rule) would have named shard 1 in group 1
    b2 = iv.Batch(code.rows, 8, "aligned", np.array([[8, 8, 8]] * 4), glen, seed=9)
    img2 = b2.host.copy()
    for j in range(2):
        img2[b2.span(1, 3 + j)[0] + 5] ^= mul[int(code.rows[j, 1]), e]
    assert iv.model_locate(b2, img2)[0][1] == 1
