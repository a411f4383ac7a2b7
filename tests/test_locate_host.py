"""CPU tests of the host half of qfec_locate: the ratio constants r_{j,i} = rows[j][i] / rows[0][i]
(qfec_locate_ratios) against the oracle's multiply, and the codes that single-shard location
refuses, decided before any device is touched.  No kernel is launched here."""
import numpy as np
import pytest

import quicknet_amd as qa

CODES = [("cauchy", 10, 3), ("cauchy", 16, 4), ("cauchy", 4, 2), ("cauchy", 9, 5), ("vandermonde", 10, 3)]
QFEC_EUNSUP = -5


@pytest.mark.parametrize("flavour,k,m", CODES)
def test_ratio_times_first_row_is_the_row(oracle, flavour, k, m):
    code = getattr(qa.Code, flavour)(k, m)
    rows, ratio = code.rows, code.locate_ratios()
    assert ratio.shape == (k, m - 1) and ratio.dtype == np.uint8
    assert rows.all()  # every coefficient non-zero: an error in any shard shows in every row
    for i in range(k):
        for j in range(1, m):
            assert oracle.mul(int(ratio[i][j - 1]), int(rows[0][i])) == int(rows[j][i]), (i, j)


def refused_codes():
    """(code, a word of the error text): every case that location cannot work on."""
    return [(qa.Code.cauchy(4, 1), "m = 1"),
            (qa.Code.cauchy(33, 2), "k = 33"),
            (qa.Code.from_rows([[1, 2, 3], [1, 0, 5]]), "zero coefficient")]


def test_unsupported_codes_are_refused_on_the_host():
    """QFEC_EUNSUP with the cause in qfec_last_error from all three entry points; the device calls
    get null buffers and zero groups, so the refusal comes before any device is looked for (without
    one, a call that got further would return QFEC_ENODEV)."""
    L = qa.lib()
    for code, why in refused_codes():
        with pytest.raises(qa.QfecError, match=why):
            code.locate_ratios()
        out = np.zeros(64, np.uint8)
        assert L.qfec_locate_ratios(code._h, out.ctypes.data) == QFEC_EUNSUP
        assert L.qfec_locate(code._h, None, None, 0, 16, 16, None, None, None, None) == QFEC_EUNSUP
        assert why in L.qfec_last_error().decode()
        assert L.qfec_scrub(code._h, None, None, 0, 16, 16, None, None, None) == QFEC_EUNSUP
        assert why in L.qfec_last_error().decode()
        # with groups to look at and a (never dereferenced) pointer each, still before the device
        assert L.qfec_locate(code._h, 64, 128, 1, 16, 16, 192, None, None, None) == QFEC_EUNSUP


def test_scrub_has_repairs_shard_limit():
    """k + m > 24: qfec_scrub refuses as qfec_repair does, qfec_locate and the ratios do not."""
    L = qa.lib()
    code = qa.Code.cauchy(20, 10)
    assert code.locate_ratios().shape == (20, 9)
    assert L.qfec_scrub(code._h, 64, 128, 1, 16, 16, None, None, None) == QFEC_EUNSUP
    assert "k + m = 30" in L.qfec_last_error().decode()
    assert L.qfec_locate(code._h, None, None, 0, 16, 16, None, None, None, None) == 0


def test_argument_checks():
    L = qa.lib()
    code = qa.Code.cauchy(4, 2)
    assert L.qfec_locate(code._h, None, None, 1, 16, 16, None, None, None, None) == -1   # null buffers
    assert L.qfec_locate(code._h, 64, 128, 1, 32, 16, 192, None, None, None) == -1       # pitch < block_size
    assert L.qfec_scrub(code._h, None, None, 1, 16, 16, None, None, None) == -1
    assert L.qfec_locate_ratios(code._h, None) == -1
