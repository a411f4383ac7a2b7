"""CPU tests of the host half of qfec_locate_erased: the per-mask plan (survivors K, spares R, the
rows A that predict each spare from K, the ratios A_x[i] / A_x0[i]) against qfec_repair_rows and,
independently, against the oracle's GF multiply on encoded data; and the codes the call refuses,
decided before any device is touched.  No kernel is launched here."""
import functools

import numpy as np
import pytest

import quicknet_amd as qa

CODES = [("cauchy", 10, 3), ("cauchy", 16, 4), ("cauchy", 9, 5), ("cauchy", 5, 4), ("vandermonde", 10, 3)]
QFEC_EINVAL, QFEC_EUNSUP = -1, -5
B = 24  # bytes per shard in the syndrome checks


@functools.lru_cache(maxsize=None)
def mul_table(oracle):
    """The oracle's 256 x 256 product table, built once from its multiply."""
    return np.array([[oracle.mul(a, b) for b in range(256)] for a in range(256)], np.uint8)


def gf_dot(MUL, coeffs, shards):
    """sum_i coeffs[i] x shards[i] over GF(2^8); shards [len(coeffs), B]."""
    acc = np.zeros(shards.shape[1], np.uint8)
    for c, s in zip(coeffs, shards):
        acc ^= MUL[int(c)][s]
    return acc


def random_marks(rng, n, t):
    marks = np.zeros(n, np.uint8)
    marks[rng.choice(n, size=t, replace=False)] = rng.integers(1, 256, size=t)  # any non-zero byte marks
    return marks


def encoded_group(oracle, code, flavour, seed):
    """One group [n, B] encoded by the oracle."""
    k, m = code.k, code.m
    data = np.random.default_rng(seed).integers(0, 256, size=(1, k, B), dtype=np.uint8)
    par = np.zeros((1, m, B), np.uint8)
    (oracle.rs_encode if flavour == "cauchy" else oracle.fec_encode)(code.rows, data, par, B)
    return np.concatenate([data[0], par[0]])


@pytest.mark.parametrize("flavour,k,m", CODES)
def test_plan_against_repair_rows_and_the_oracle(oracle, flavour, k, m):
    """Random masks of every t <= m (three per t, plus the empty mask once)."""
    code = getattr(qa.Code, flavour)(k, m)
    MUL = mul_table(oracle)
    n = k + m
    rng = np.random.default_rng(100 * k + m)
    shards = encoded_group(oracle, code, flavour, 7 * k + m)
    for t in range(m + 1):
        for rep in range(1 if t == 0 else 3):
            marks = random_marks(rng, n, t)
            S, surv, spares, rows, ratios = code.locate_erased_plan(marks)
            unmarked = [i for i in range(n) if not marks[i]]
            assert list(surv) == unmarked[:k], (t, marks)
            if t == m:
                assert S == 0 and spares is None and rows is None
                continue
            assert S == m - t and list(spares) == unmarked[k:] and all(x >= k for x in spares)
            assert rows.shape == (S, k) and ratios.shape == (k, S - 1)
            # the rows qfec_repair_rows returns for the spares under the mask E + R (m bits set, K unchanged)
            full = np.ones(n, np.uint8)
            full[unmarked[:k]] = 0
            tt, rrows, rsurv, rlost = code.repair_rows(full)
            assert tt == m and list(rsurv) == list(surv)
            for x, sp in enumerate(spares):
                assert np.array_equal(rows[x], rrows[list(rlost).index(sp)]), (marks, sp)
            if t == 0:  # reduces to qfec_locate: K the data, R the parity, A the parity rows
                assert list(surv) == list(range(k)) and np.array_equal(rows, code.rows)
                assert np.array_equal(ratios, code.locate_ratios())
            # independently: on encoded data with the marked shards dropped every syndrome is zero
            got = shards.copy()
            got[marks != 0] = 0xA5  # never read
            syn = lambda g: [g[sp] ^ gf_dot(MUL, rows[x], g[list(surv)]) for x, sp in enumerate(spares)]
            assert not np.any(syn(got)), marks
            # a byte XORed into survivor i: s_x = ratio x s_x0 holds for i and for no other shard
            for pos in rng.choice(k, size=min(k, 4), replace=False):
                hit = got.copy()
                hit[surv[pos], 5] ^= int(rng.integers(1, 256))
                s = syn(hit)
                assert s[0].any()  # A has no zero: the error shows in the first spare
                explains = [all(np.array_equal(MUL[int(ratios[i][x - 1])][s[0]], s[x]) for x in range(1, S))
                            for i in range(k)]
                if S >= 2:
                    assert explains == [i == pos for i in range(k)], (marks, pos)
                    assert sum(1 for x in s if x.any()) >= 2  # and no spare alone explains it
    over = random_marks(rng, n, m + 1)
    assert code.locate_erased_plan(over)[0] == -1
    assert qa.lib().qfec_locate_erased_plan(code._h, over.ctypes.data, None, None, None, None) == -1
    assert qa.lib().qfec_locate_erased_plan(code._h, random_marks(rng, n, m).ctypes.data, None, None, None, None) == 0


# rows that qfec_locate accepts (no zero coefficient) but whose punctured code is not MDS: the 2 x 2
# minor of rows 0, 2 and columns 0, 1 is 1 x 2 ^ 1 x 2 = 0.  With data shard 0 lost, d0 = p0 ^ d1 ^ d2,
# so p2 = 2 d0 ^ 2 d1 ^ 7 d2 = 2 p0 ^ 0 d1 ^ 5 d2: spare row p2 has a zero at survivor d1
NOT_MDS = [[1, 1, 1], [1, 2, 3], [2, 2, 7]]


def refused_codes():
    """(code, a word of the error text): every case qfec_locate_erased cannot work on."""
    return [(qa.Code.cauchy(4, 1), "m = 1"),
            (qa.Code.cauchy(20, 10), "k \\+ m = 30"),
            (qa.Code.from_rows([[1, 2, 3], [1, 0, 5], [1, 4, 6]]), "zero coefficient"),
            (qa.Code.from_rows(NOT_MDS), "mask 0x1 lost, spare row 5 has a zero coefficient at survivor 1.*not MDS"),
            (qa.Code.cauchy(12, 12), "k = 12, m = 12 needs 7036530 pattern records")]  # sum_{t < 12} C(24, t)


def test_unsupported_codes_are_refused_on_the_host():
    """QFEC_EUNSUP with the cause in qfec_last_error from every device entry point; the calls get null
    buffers and zero groups, or never-dereferenced pointers, so the refusal comes before any device
    is looked for (without one, a call that got further would return QFEC_ENODEV)."""
    import re
    L = qa.lib()
    for code, why in refused_codes():
        assert L.qfec_locate_erased(code._h, None, None, None, 0, 16, 16, None, None, None, None) == QFEC_EUNSUP
        assert re.search(why, L.qfec_last_error().decode()), L.qfec_last_error().decode()
        assert L.qfec_scrub_erased(code._h, None, None, None, 0, 16, 16, None, None, None, None) == QFEC_EUNSUP
        assert re.search(why, L.qfec_last_error().decode())
        assert L.qfec_prepare_locate_erased(code._h) == QFEC_EUNSUP
        assert L.qfec_locate_erased(code._h, 64, 128, 256, 1, 16, 16, 192, None, None, None) == QFEC_EUNSUP
        assert L.qfec_locate_erased(code._h, 64, 128, 256, 1, 16, 16, 192, None, None, None) == QFEC_EUNSUP  # cached


def test_not_mds_rows_are_fine_for_qfec_locate_and_the_plan_shows_the_zero():
    code = qa.Code.from_rows(NOT_MDS)
    assert code.rows.all() and code.locate_ratios().shape == (3, 2)
    assert qa.lib().qfec_locate(code._h, None, None, 0, 16, 16, None, None, None, None) == 0
    S, surv, spares, rows, _ = code.locate_erased_plan([1, 0, 0, 0, 0, 0])
    assert S == 2 and list(surv) == [1, 2, 3] and list(spares) == [4, 5]
    assert list(rows[1]) == [0, 5, 2]


def test_argument_checks():
    L = qa.lib()
    code = qa.Code.cauchy(4, 2)
    assert L.qfec_locate_erased(code._h, 64, 128, 256, 1, 16, 16, None, None, None, None) == QFEC_EINVAL  # null d_culprit
    assert "invalid argument" in L.qfec_last_error().decode()
    assert L.qfec_locate_erased(code._h, 64, 128, None, 1, 16, 16, 192, None, None, None) == QFEC_EINVAL   # null marks
    assert L.qfec_locate_erased(code._h, 64, 128, 256, 1, 32, 16, 192, None, None, None) == QFEC_EINVAL    # pitch < block_size
    assert L.qfec_scrub_erased(code._h, None, None, None, 1, 16, 16, None, None, None, None) == QFEC_EINVAL
    assert L.qfec_locate_erased_plan(code._h, None, None, None, None, None) == QFEC_EINVAL
    # zero groups: OK without a device, from both calls
    assert L.qfec_locate_erased(code._h, None, None, None, 0, 16, 16, None, None, None, None) == 0
    assert L.qfec_scrub_erased(code._h, None, None, None, 0, 16, 16, None, None, None, None) == 0
    assert (qa.QFEC_LOC_UNCHECKED, qa.QFEC_LOC_LOST) == (-4, -5)
