"""CPU tests of the plan calls on pointer tables with per-shard lengths (qfec_plan_apply_ptrs_var,
qfec_reconstruct_ptrs_wide_var, qfec_repair_ptrs_wide_var, include/qfec.h): every argument they refuse
is refused on the host, with its cause in qfec_last_error after the call's name, with stand-in
pointers that are never dereferenced; what needs no device needs none; the Python face's count and
dtype checks; and the rule by which the apply takes "unmarked" from a plan, held against the marks the
plan was built from.  No kernel is launched here."""
import numpy as np
import pytest

import quicknet_amd as qa
import ptrs_common as pc
from wide_common import FAILED, NONE, RECONSTRUCT, REPAIR, WORK, layout, status_of

QFEC_OK, QFEC_EINVAL, QFEC_ENODEV, QFEC_EUNSUP = 0, -1, -2, -5
T, N, GL, M, PL, F, V = 4096, 8192, 12288, 16384, 20480, 24576, 28672  # stand-ins for device pointers
APPLY = "qfec_plan_apply_ptrs_var"
ONE_SHOTS = ("qfec_reconstruct_ptrs_wide_var", "qfec_repair_ptrs_wide_var")


def last_error():
    return qa.lib().qfec_last_error().decode()


def call(name, h, table, lens, glen, marks_or_plan, groups, max_len):
    """The C call with stand-in counters (the one-shots take two, the apply one) and a null stream."""
    fn = getattr(qa.lib(), name)
    if name == APPLY:
        return fn(h, table, lens, glen, marks_or_plan, groups, max_len, V, None)
    return fn(h, table, lens, glen, marks_or_plan, groups, max_len, F, V, None)


# (table, lens, group_len, marks or plan, groups, max_len) -> the cause named
COMMON_REFUSED = [
    ((T, N, GL, M, -1, 16), "groups < 0"),
    ((T, N, GL, M, 1, 0), "max_len < 1"),
    ((T, N, GL, M, 1, -7), "max_len < 1"),
    ((None, N, GL, M, 1, 16), "null d_shards"),
    ((T, None, GL, M, 1, 16), "null d_lens"),
    ((T, N, None, M, 1, 16), "null d_group_len"),
]


@pytest.mark.parametrize("args,why", COMMON_REFUSED + [((T, N, GL, None, 1, 16), "null d_marks")])
def test_one_shots_refuse_on_the_host(args, why):
    code = qa.Code.cauchy(32, 8)
    for name in ONE_SHOTS:
        assert call(name, code._h, *args) == QFEC_EINVAL
        assert last_error().startswith(name + ":") and why in last_error(), last_error()


@pytest.mark.parametrize("args,why", COMMON_REFUSED + [
    ((T, N, GL, None, 1, 16), "null d_plan"),
    ((T, N, GL, PL + 1, 1, 16), "d_plan not 16-byte aligned"),
    ((T, N, GL, PL + 4, 1, 16), "d_plan not 16-byte aligned"),
    ((T + 1, N, GL, PL + 8, 1, 16), "d_plan not 16-byte aligned"),
])
def test_plan_apply_ptrs_var_refuses_on_the_host(args, why):
    code = qa.Code.cauchy(32, 8)
    assert call(APPLY, code._h, *args) == QFEC_EINVAL
    assert last_error().startswith(APPLY + ":") and why in last_error(), last_error()


def test_null_code_is_named():
    for name in (APPLY,) + ONE_SHOTS:
        assert call(name, None, T, N, GL, PL, 1, 16) == QFEC_EINVAL
        assert last_error().startswith(name + ":") and "null code" in last_error(), last_error()


@pytest.mark.parametrize("k,m", [(4, 2), (20, 5), (200, 55)])
def test_nothing_to_do_is_ok_without_a_device(k, m):
    """groups = 0: QFEC_OK with null buffers at any k + m; a bad argument still wins."""
    code = qa.Code.cauchy(k, m)
    for name in (APPLY,) + ONE_SHOTS:
        assert call(name, code._h, None, None, None, None, 0, 16) == QFEC_OK
        assert call(name, code._h, None, None, None, None, 0, 0) == QFEC_EINVAL
        assert last_error().startswith(name + ":") and "max_len < 1" in last_error()
        assert call(name, code._h, None, None, None, None, -1, 16) == QFEC_EINVAL
        assert "groups < 0" in last_error()
    assert call(APPLY, code._h, None, None, None, PL + 4, 0, 16) == QFEC_EINVAL
    assert "d_plan not 16-byte aligned" in last_error()


def test_a_wide_code_is_accepted():
    """k + m = 25, where qfec_reconstruct_ptrs_var answers QFEC_EUNSUP: the arguments pass, the code
    passes, and the calls get as far as asking for a device."""
    if qa.device_count() > 0:
        pytest.skip("a GPU is present: the calls would run on the stand-in pointers")
    code = qa.Code.cauchy(20, 5)
    assert qa.lib().qfec_reconstruct_ptrs_var(code._h, T, N, GL, M, 1, 16, None, None, None) == QFEC_EUNSUP
    assert call(APPLY, code._h, T, N, GL, PL, 1, 16) == QFEC_ENODEV
    for name in ONE_SHOTS:
        assert call(name, code._h, T, N, GL, M, 1, 16) == QFEC_ENODEV


def test_edited_rs_handle_is_unsupported():
    rs = qa.ReedSolomon(6, 3)
    rs.m_matrix[7, 2] ^= 0x21
    code = rs.code()
    for groups in (0, 1):
        for name in (APPLY,) + ONE_SHOTS:
            assert call(name, code._h, T, N, GL, PL, groups, 16) == QFEC_EUNSUP
            assert last_error().startswith(name + ":") and "edited handle" in last_error(), last_error()
    rs.m_matrix[7, 2] ^= 0x21
    code = rs.code()
    for name in (APPLY,) + ONE_SHOTS:
        assert call(name, code._h, T, N, GL, PL, 0, 16) == QFEC_OK
    rs.close()


def test_python_face_checks_counts_and_dtypes():
    import torch

    code = qa.Code.cauchy(4, 2)  # 12 pointers = 2 groups: 8 lengths, 2 group lengths, 12 marks, 2 plans
    ptrs = torch.zeros(12, dtype=torch.int64)
    lens, glen = torch.zeros(8, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    marks = torch.zeros(12, dtype=torch.uint8)
    plan = torch.zeros(2 * code.plan_stride(), dtype=torch.uint8)
    one_shots = (code.reconstruct_ptrs_wide_var, code.repair_ptrs_wide_var)
    for n in (5, 7, 13):
        bad = torch.zeros(n, dtype=torch.int64)
        with pytest.raises(qa.QfecError, match="groups \\* \\(k \\+ m\\)"):
            code.plan_apply_ptrs_var(bad, lens, glen, plan, 16)
        for fn in one_shots:
            with pytest.raises(qa.QfecError, match="groups \\* \\(k \\+ m\\)"):
                fn(bad, lens, glen, marks, 16)
    with pytest.raises(qa.QfecError, match="plan has"):
        code.plan_apply_ptrs_var(ptrs, lens, glen, plan[:-16], 16)
    for fn, last in [(code.plan_apply_ptrs_var, plan)] + [(f, marks) for f in one_shots]:
        with pytest.raises(qa.QfecError, match="lens has 9 elements, 8 expected"):
            fn(ptrs, torch.zeros(9, dtype=torch.int32), glen, last, 16)
        with pytest.raises(qa.QfecError, match="lens has dtype torch.int64"):
            fn(ptrs, torch.zeros(8, dtype=torch.int64), glen, last, 16)
        with pytest.raises(qa.QfecError, match="group_len has 1 elements, 2 expected"):
            fn(ptrs, lens, torch.zeros(1, dtype=torch.int32), last, 16)
        with pytest.raises(qa.QfecError, match="group_len has dtype torch.int16"):
            fn(ptrs, lens, torch.zeros(2, dtype=torch.int16), last, 16)
        with pytest.raises(qa.QfecError, match="expected a device tensor"):
            fn(ptrs, lens, glen, last, 16)
    for fn in one_shots:
        with pytest.raises(qa.QfecError, match="11 marks"):
            fn(ptrs, lens, glen, torch.zeros(11, dtype=torch.uint8), 16)


@pytest.mark.parametrize("mode", [RECONSTRUCT, REPAIR], ids=["reconstruct", "repair"])
@pytest.mark.parametrize("k,m", [(10, 3), (32, 8), (60, 5)], ids=["10-3", "32-8", "60-5"])
def test_unmarked_data_shards_are_those_outside_the_lost_list(k, m, mode):
    """What the header claims of a plan: for status 0 and 1, in both modes, the data ids outside the
    first t entries of the lost list are exactly the unmarked data ids of the marks the plan was built
    from (a status-0 plan has t = 0); a failed plan carries no lists."""
    code = qa.Code.cauchy(k, m)
    gm = pc.recon_marks(k, m)
    pc.assert_marks_cover(gm, k, m)
    so, lo, _, co, _ = layout(k, m)
    seen = set()
    for mk in gm:
        plan = code.plan_host(mk, mode)
        status, t = int(status_of(plan)), int(plan[0]) | int(plan[1]) << 8
        seen.add(status)
        if status == FAILED:
            assert not plan[16:].any()
            continue
        assert status in (NONE, WORK) and t <= m
        if status == NONE:
            assert t == 0
        listed = set(plan[lo:lo + t].tolist())
        assert set(range(k)) - listed == set(np.flatnonzero(mk[:k] == 0).tolist())
        if status == WORK:  # the parity survivors the apply adds: the last e entries of the survivor list
            e = int(plan[2]) | int(plan[3]) << 8
            surv = plan[so:so + k].tolist()
            assert surv[:k - e] == sorted(set(range(k)) - listed) and all(s >= k for s in surv[k - e:])
    assert seen == {NONE, WORK, FAILED}
