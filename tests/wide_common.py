"""Shared by test_wide_host.py and test_gpu_wide.py: the public layout of a decode plan
(include/qfec.h, qfec_plan_build), read and written from Python; the plan a group must get, built
from the existing host queries qfec_repair_rows / qfec_decode_rows; and the odd codes both suites
use (a stale-row code, a singular one)."""
import functools

import numpy as np

import quicknet_amd as qa

RECONSTRUCT, REPAIR = qa.QFEC_PLAN_RECONSTRUCT, qa.QFEC_PLAN_REPAIR
NONE, WORK, FAILED = 0, 1, 2


def layout(k, m):
    """(surv_off, lost_off, stale_off, coef_off, stride): a 16-byte header, k survivor ids, m lost
    ids, m stale flags, then from the next 16-byte boundary m x k coefficients, padded to 16."""
    surv = 16
    lost = surv + k
    stale = lost + m
    coef = (stale + m + 15) // 16 * 16
    return surv, lost, stale, coef, (coef + m * k + 15) // 16 * 16


def make_plan(k, m, t, e, status, surv=(), lost=(), stale=(), rows=None):
    """A plan in the public layout; every byte not given is zero."""
    so, lo, fo, co, stride = layout(k, m)
    p = np.zeros(stride, np.uint8)
    p[0], p[1], p[2], p[3], p[4] = t & 255, t >> 8, e & 255, e >> 8, status
    p[so:so + len(surv)] = surv
    p[lo:lo + len(lost)] = lost
    p[fo:fo + len(stale)] = stale
    if rows is not None:
        p[co:co + rows.size] = rows.reshape(-1)
    return p


def status_of(plan):
    return plan[..., 4]


def stale_flags(plan, k, m):
    _, _, fo, _, _ = layout(k, m)
    return plan[fo:fo + m]


def gf_tables():
    exp = np.zeros(512, np.int64)
    log = np.zeros(256, np.int64)
    x = 1
    for i in range(255):
        exp[i] = exp[i + 255] = x
        log[x] = i
        x <<= 1
        if x & 0x100:
            x ^= 0x11D
    return exp, log


def expected_plan(code, marks_n, mode, quirk):
    """The plan of one group from the host queries that exist: qfec_repair_rows (mode REPAIR) or
    qfec_decode_rows (mode RECONSTRUCT).  A refused or empty group carries t, e and the status only;
    the stale flag of a data row is quirk and a zero column-0 coefficient."""
    k, m = code.k, code.m
    marks_n = np.asarray(marks_n, np.uint8)
    e = int(marks_n[:k].sum())
    if mode == REPAIR:
        t = int(marks_n.sum())
        rt, rows, surv, lost = code.repair_rows(marks_n)
    else:
        t = e
        rt, rows, surv, lost = code.decode_rows(marks_n)
    if t == 0:
        assert rt == 0
        return make_plan(k, m, 0, e, NONE)
    if rt < 0:
        return make_plan(k, m, t, e, FAILED)
    assert rt == t
    stale = [int(quirk and j < e and rows[j, 0] == 0) for j in range(t)]
    return make_plan(k, m, t, e, WORK, surv, lost, stale, rows)


def random_masks(seed, n, m, count):
    """[count, n] uint8: 0..m+1 marks each; the first three are empty, one mark, m + 1 marks."""
    rng = np.random.default_rng(seed)
    gm = np.zeros((count, n), np.uint8)
    for g in range(count):
        t = (0, 1, min(m + 1, n))[g] if g < 3 else int(rng.integers(0, min(m + 1, n) + 1))
        gm[g, rng.choice(n, size=t, replace=False)] = 1
    return gm


def cauchy_rows(k, m):
    """module/rs.c's parity rows, rows[j][i] = 1 / ((m + i) ^ j)."""
    exp, log = gf_tables()
    return np.array([[exp[255 - log[(m + i) ^ j]] for i in range(k)] for j in range(m)], np.uint8)


@functools.lru_cache(maxsize=None)
def stale_code(quirk):
    """(30,4) from explicit Cauchy rows with rows[0][0] = 0: losing only data shard 5 decodes from
    parity row 0, and the decode row's column-0 coefficient is rows[0][0] / rows[0][5] = 0."""
    rows = cauchy_rows(30, 4)
    rows[0, 0] = 0
    return qa.Code.from_rows(rows, rs_stale_quirk=bool(quirk)), rows


def stale_marks():
    mk = np.zeros(34, np.uint8)
    mk[5] = 1
    return mk


@functools.lru_cache(maxsize=None)
def singular_code():
    """(26,2) whose two parity rows are equal: any two lost data shards give a singular matrix."""
    rows = cauchy_rows(26, 2)
    rows[1] = rows[0]
    return qa.Code.from_rows(rows), rows


def singular_marks():
    mk = np.zeros(28, np.uint8)
    mk[[3, 17]] = 1
    return mk
