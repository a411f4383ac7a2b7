"""CPU tests of the repair matrix (qfec_repair_rows, gf256.cpp repair_rows): for an erasure pattern
over all n shards, the rows it returns, applied to the survivors' bytes, give what the oracle's
reconstruct followed by its encode gives -- for the marked data rows and the marked parity rows.
No kernel is launched here."""
import numpy as np
import pytest

import quicknet_amd as qa
from repair_common import damage, expected_repair, masks_up_to

BT = 48  # bytes per row: a few dozen are enough for a GF identity

_MUL = []


def mul_table(oracle):
    """256 x 256 GF(2^8) products, from the oracle's multiply."""
    if not _MUL:
        _MUL.append(np.array([[oracle.mul(a, b) for b in range(256)] for a in range(256)], np.uint8))
    return _MUL[0]


def check_masks(oracle, flavour, k, m, gm, seed):
    code = getattr(qa.Code, flavour)(k, m)
    n = k + m
    G = gm.shape[0]
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, (G, k, BT), dtype=np.uint8)
    par = rng.integers(0, 256, (G, m, BT), dtype=np.uint8)  # random, inconsistent parity
    data, par = damage(data, par, gm)
    exp_d, exp_p, _ = expected_repair(oracle, code, flavour, data, par, gm, BT)
    mul = mul_table(oracle)
    seen = {"none": 0, "fail": 0, "rows": 0}
    for g in range(G):
        marks = gm[g]
        t_ref = int(marks.sum())
        t, rows, surv, lost = code.repair_rows(marks)
        if t_ref == 0:
            assert t == 0, marks
            seen["none"] += 1
            continue
        if t_ref > m:
            assert t == -1, marks
            seen["fail"] += 1
            continue
        assert t == t_ref, marks
        assert list(surv) == [i for i in range(n) if not marks[i]][:k], marks
        assert list(lost) == [i for i in range(n) if marks[i]], marks
        shards = np.concatenate([data[g], par[g]])  # [n, BT]
        expect = np.concatenate([exp_d[g], exp_p[g]])
        s = shards[list(surv)]  # [k, BT]
        out = np.zeros((t, BT), np.uint8)
        for j in range(t):
            for c in range(k):
                out[j] ^= mul[rows[j, c]][s[c]]
        assert np.array_equal(out, expect[list(lost)]), marks
        seen["rows"] += 1
    return seen


@pytest.mark.parametrize("flavour", ["cauchy", "vandermonde"])
def test_repair_rows_42_all_masks(oracle, flavour):
    seen = check_masks(oracle, flavour, 4, 2, masks_up_to(6, 6), 42)
    assert seen == {"none": 1, "fail": 64 - 1 - 6 - 15, "rows": 6 + 15}


def test_repair_rows_103_up_to_4_bits(oracle):
    gm = masks_up_to(13, 4)
    assert gm.shape[0] == 1093
    seen = check_masks(oracle, "cauchy", 10, 3, gm, 103)
    assert seen == {"none": 1, "fail": 715, "rows": 13 + 78 + 286}


def test_repair_rows_164_random(oracle):
    rng = np.random.default_rng(164)
    gm = np.zeros((200, 20), np.uint8)
    for g in range(200):
        gm[g, rng.choice(20, size=int(rng.integers(0, 6)), replace=False)] = 1
    seen = check_masks(oracle, "cauchy", 16, 4, gm, 164)
    assert seen["rows"] > 100 and seen["fail"] > 10 and seen["none"] > 10


def test_repair_rows_wide_code_on_host():
    """The host query has no LUT and so no k + m limit; the device call refuses k + m > 24 before
    it touches a device."""
    code = qa.Code.cauchy(32, 8)
    marks = np.zeros(40, np.uint8)
    marks[[0, 5, 33]] = 1
    t, rows, surv, lost = code.repair_rows(marks)
    assert t == 3 and list(lost) == [0, 5, 33] and rows.shape == (3, 32)
    assert list(surv) == [i for i in range(40) if not marks[i]][:32]
    L = qa.lib()
    assert L.qfec_prepare_repair(code._h) == -5  # QFEC_EUNSUP
    assert "k + m = 40" in L.qfec_last_error().decode()
