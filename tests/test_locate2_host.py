"""CPU tests of the host half of qfec_locate2: the distance facts the design rests on, checked with
the oracle's GF arithmetic; the pair constants F_ab (qfec_locate2_checks) against the oracle's
multiply; and the codes that two-shard location refuses, decided before any device is touched.  No
kernel is launched here."""
import itertools

import numpy as np
import pytest

import quicknet_amd as qa
from locate2_common import columns, every_subset_independent, left_null, mul_table, rank

CODES = [("cauchy", 4, 4), ("cauchy", 16, 4), ("cauchy", 5, 5), ("cauchy", 3, 6), ("vandermonde", 10, 4)]
QFEC_EINVAL, QFEC_EUNSUP = -1, -5
DEPENDENT_ROWS = [[1, 3, 2], [2, 1, 3], [4, 7, 3], [8, 5, 13]]   # columns 0, 1, 2 are dependent
DISTANCE4_ROWS = [[1, 3, 3], [2, 1, 3], [4, 7, 3], [8, 5, 13]]   # h_0 ^ h_1 ^ h_2 ^ e_0 = 0


@pytest.mark.parametrize("flavour,k,m", [("cauchy", 4, 4), ("cauchy", 8, 4), ("cauchy", 16, 4), ("cauchy", 3, 4),
                                         ("vandermonde", 4, 4), ("vandermonde", 10, 4)])
def test_every_four_columns_are_independent(flavour, k, m):
    """Distance 5: two corrupted shards are determined uniquely."""
    assert every_subset_independent(getattr(qa.Code, flavour)(k, m).rows, 4)


@pytest.mark.parametrize("flavour,k,m", [("cauchy", 5, 5), ("cauchy", 6, 5), ("vandermonde", 5, 5)])
def test_every_five_columns_are_independent(flavour, k, m):
    """Distance 6: three corrupted shards are never taken for two."""
    assert every_subset_independent(getattr(qa.Code, flavour)(k, m).rows, 5)


def test_dependent_rows_pass_locate_and_fail_locate2():
    rows = np.array(DEPENDENT_ROWS, np.uint8)
    h = columns(rows)
    assert rows.all()
    assert all(rank([h[a], h[b]]) == 2 for a, b in itertools.combinations(range(7), 2))  # no two proportional
    assert rank([h[0], h[1], h[2]]) == 2
    code = qa.Code.from_rows(DEPENDENT_ROWS)
    assert code.locate_ratios().shape == (3, 3)  # qfec_locate takes the code
    with pytest.raises(qa.QfecError, match="columns 0, 1 and 2"):
        code.locate2_checks(0, 1)


def test_distance4_rows_are_accepted():
    rows = np.array(DISTANCE4_ROWS, np.uint8)
    h = columns(rows)
    assert every_subset_independent(rows, 3)
    assert not any(np.bitwise_xor.reduce(np.array([h[0], h[1], h[2], h[3]]), axis=0))  # 3 = parity row 0
    # so the same value XORed into shards 0 and 1 at one byte is explained by {0,1} and by {2,3}
    s = np.array(h[0])[:, None] ^ np.array(h[1])[:, None]
    for pair in ((0, 1), (2, 3)):
        f = left_null([h[pair[0]], h[pair[1]]])
        assert not any(np.bitwise_xor.reduce([mul_table()[c, s[j]] for j, c in enumerate(row)])[0] for row in f)
    assert qa.Code.from_rows(DISTANCE4_ROWS).locate2_checks(0, 1).shape == (2, 4)


def gf_dot(row, col):
    mul = mul_table()
    return int(np.bitwise_xor.reduce([mul[int(r), int(c)] for r, c in zip(row, col)]))


@pytest.mark.parametrize("flavour,k,m", CODES)
def test_checks_annihilate_their_pair_and_nothing_else(oracle, flavour, k, m):
    """All pairs: F . h_a = 0 and F . h_b = 0, rank m - 2, and F . h_c != 0 for every third column
    (no three columns dependent).  The products by the table built from the oracle's multiply; one
    pair per code also by oracle.mul directly."""
    code = getattr(qa.Code, flavour)(k, m)
    h = columns(code.rows)
    n = k + m
    for a, b in itertools.combinations(range(n), 2):
        f = code.locate2_checks(a, b)
        assert f.shape == (m - 2, m) and f.dtype == np.uint8
        assert np.array_equal(f, code.locate2_checks(b, a))
        for x in (a, b):
            assert not any(gf_dot(row, h[x]) for row in f), (a, b, x)
        assert rank([tuple(int(v) for v in f[:, j]) for j in range(m)]) == m - 2
        for c in range(n):
            if c not in (a, b):
                assert any(gf_dot(row, h[c]) for row in f), (a, b, c)
    f = code.locate2_checks(0, n - 1)
    for row in f:
        for x in (0, n - 1):
            acc = 0
            for j in range(m):
                acc ^= oracle.mul(int(row[j]), h[x][j])
            assert acc == 0


def refused_codes():
    """(code, a word of the error text): every case that two-shard location cannot work on."""
    return [(qa.Code.cauchy(4, 3), "m = 3"),
            (qa.Code.cauchy(21, 4), "k \\+ m = 25"),
            (qa.Code.from_rows(DEPENDENT_ROWS), "columns 0, 1 and 2 of \\[rows \\| I\\] are linearly dependent"),
            (qa.Code.from_rows([[1, 2, 3], [1, 0, 5], [1, 4, 6], [1, 8, 9]]), "zero coefficient")]


def test_unsupported_codes_are_refused_on_the_host():
    """QFEC_EUNSUP with the cause in qfec_last_error from all three entry points; the device calls
    get null buffers and zero groups, so the refusal comes before any device is looked for."""
    import re

    L = qa.lib()
    for code, why in refused_codes():
        with pytest.raises(qa.QfecError, match=why):
            code.locate2_checks(0, 1)
        out = np.zeros(1024, np.uint8)
        assert L.qfec_locate2_checks(code._h, 0, 1, out.ctypes.data) == QFEC_EUNSUP
        assert L.qfec_locate2(code._h, None, None, 0, 16, 16, None, None, None, None) == QFEC_EUNSUP
        assert re.search(why, L.qfec_last_error().decode()) and "qfec_locate2:" in L.qfec_last_error().decode()
        assert L.qfec_scrub2(code._h, None, None, 0, 16, 16, None, None, None) == QFEC_EUNSUP
        assert re.search(why, L.qfec_last_error().decode()) and "qfec_scrub2:" in L.qfec_last_error().decode()
        # with groups to look at and a (never dereferenced) pointer each, still before the device
        assert L.qfec_locate2(code._h, 64, 128, 1, 16, 16, 192, None, None, None) == QFEC_EUNSUP
        assert L.qfec_scrub2(code._h, 64, 128, 1, 16, 16, None, None, None) == QFEC_EUNSUP


def test_accepted_code_with_nothing_to_do():
    L = qa.lib()
    code = qa.Code.cauchy(20, 4)  # k + m = 24, the widest
    assert L.qfec_locate2(code._h, None, None, 0, 16, 16, None, None, None, None) == 0
    assert L.qfec_scrub2(code._h, None, None, 0, 16, 16, None, None, None) == 0


def test_argument_checks():
    L = qa.lib()
    code = qa.Code.cauchy(4, 4)
    out = np.zeros(8, np.uint8)
    assert L.qfec_locate2(code._h, None, None, 1, 16, 16, None, None, None, None) == QFEC_EINVAL   # null buffers
    assert L.qfec_locate2(code._h, 64, 128, 1, 16, 16, None, None, None, None) == QFEC_EINVAL     # null culprit
    assert L.qfec_locate2(code._h, 64, 128, 1, 32, 16, 192, None, None, None) == QFEC_EINVAL      # pitch < block_size
    assert L.qfec_locate2(code._h, 64, 128, -1, 16, 16, 192, None, None, None) == QFEC_EINVAL
    assert L.qfec_locate2(None, 64, 128, 1, 16, 16, 192, None, None, None) == QFEC_EINVAL
    assert L.qfec_scrub2(code._h, None, None, 1, 16, 16, None, None, None) == QFEC_EINVAL
    assert L.qfec_locate2_checks(code._h, 0, 1, None) == QFEC_EINVAL
    assert L.qfec_locate2_checks(None, 0, 1, out.ctypes.data) == QFEC_EINVAL
    for a, b in ((0, 0), (-1, 2), (0, 8), (8, 0)):
        assert L.qfec_locate2_checks(code._h, a, b, out.ctypes.data) == QFEC_EINVAL
    assert L.qfec_locate2_checks(code._h, 7, 0, out.ctypes.data) == 2
