"""CPU tests of edits to a LIVE reed_solomon handle (handle_edits_common): the host half.

* CACHES is held to the source: every `uint64_t ...version` stamp of DevLut, DevTables and qfec_code
  in quicknet_amd/csrc/qfec_rt.hpp must be a key, and every test it names must exist, so a cache
  added later without a warm-edit case fails here.
* Every host query is asked warm on the original matrices, after an edit, and after the original
  matrices are written back: each answer equals a cold Code.from_rows twin's (and the expectation of
  wide_common / locate_wide_common where one exists), changes with the edit and returns with the
  restore.  No device is involved: only the stamps kept on the code itself are exercised."""
import ast
import os
import re

import numpy as np
import pytest

import handle_edits_common as he
import quicknet_amd as qa
from locate_wide_common import expected_check
from wide_common import RECONSTRUCT, REPAIR, expected_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_HPP = os.path.join(ROOT, "quicknet_amd", "csrc", "qfec_rt.hpp")
SHAPES = [(6, 4), (8, 4), (26, 4)]  # generic and instanced with n <= 24; n > 24: no locate2, no mask-keyed family
QFEC_EUNSUP = -5


# ------------------------------------------------------------------ the source table

def struct_body(text, name):
    m = re.search(rf"^struct {name} \{{\n(.*?)^\}};", text, re.M | re.S)
    assert m, f"struct {name} not found in qfec_rt.hpp"
    return m.group(1)


def source_stamps():
    """Every version stamp a cache carries, named as CACHES names them: the uint64_t ...version
    members of DevTables and qfec_code (less the code's own counter), and `<member>.version` for
    every DevLut member of DevTables."""
    with open(RT_HPP) as f:
        text = f.read()
    stamp = r"^\s*uint64_t (\w*version)\b"
    assert re.findall(stamp, struct_body(text, "DevLut"), re.M) == ["version"]
    out = re.findall(stamp, struct_body(text, "DevTables"), re.M)
    out += [f"{name}.version" for name in re.findall(r"^\s*DevLut (\w+);", struct_body(text, "DevTables"), re.M)]
    code = re.findall(stamp, struct_body(text, "qfec_code"), re.M)
    assert "version" in code, "qfec_code::version, the counter the stamps are compared with"
    return sorted(out + [s for s in code if s != "version"])


def test_caches_are_the_source_stamps():
    src = source_stamps()
    assert len(src) == len(set(src)) >= 12
    assert sorted(he.CACHES) == src, (
        f"handle_edits_common.CACHES and the version stamps of qfec_rt.hpp differ: only in the source "
        f"{sorted(set(src) - set(he.CACHES))}, only in CACHES {sorted(set(he.CACHES) - set(src))}")


def test_caches_name_existing_tests():
    seen = {}
    for stamp, ids in he.CACHES.items():
        assert ids, f"{stamp}: no warm-edit test"
        for tid in ids:
            path, name = tid.split("::")
            if path not in seen:
                with open(os.path.join(ROOT, path)) as f:
                    seen[path] = {n.name for n in ast.parse(f.read()).body if isinstance(n, ast.FunctionDef)}
            assert name.startswith("test_") and name in seen[path], f"{stamp}: {tid} does not exist"


# ------------------------------------------------------------------ the host queries

def marks_for(k, m):
    """Group-order mark vectors: one data and one parity shard (the probe of the issue), one data
    shard, m - 1 shards over both halves, nothing."""
    n = k + m
    out = []
    for ids in ([1, k], [k - 1], [0, 2, n - 1][:m - 1], []):
        v = np.zeros(n, np.uint8)
        v[ids] = 1
        out.append(v)
    return out


def queries(k, m):
    mk = marks_for(k, m)
    q = {"rows": lambda c: c.rows, "locate_ratios": lambda c: c.locate_ratios(),
         "locate2_checks": lambda c: [c.locate2_checks(0, k), c.locate2_checks(1, 2), c.locate2_checks(k, k + m - 1)]}
    for i, v in enumerate(mk):
        q[f"decode_rows-{i}"] = lambda c, v=v: c.decode_rows(v)
        q[f"repair_rows-{i}"] = lambda c, v=v: c.repair_rows(v)
        q[f"locate_erased_plan-{i}"] = lambda c, v=v: c.locate_erased_plan(v)
        q[f"plan_host-repair-{i}"] = lambda c, v=v: c.plan_host(v, REPAIR)
        q[f"plan_host-reconstruct-{i}"] = lambda c, v=v: c.plan_host(v, RECONSTRUCT)
        q[f"check_host-{i}"] = lambda c, v=v: c.check_host(v)
    return q


def snap(code):
    """{query: answer, or 'ERR <the whole error text>'}"""
    out = {}
    for name, fn in queries(code.k, code.m).items():
        try:
            out[name] = fn(code)
        except qa.QfecError as e:
            out[name] = "ERR " + str(e)
    return out


def same(a, b):
    if isinstance(a, str) or isinstance(b, str):
        return isinstance(a, str) and isinstance(b, str) and a == b
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def differing(a, b):
    return sorted(name for name in a if not same(a[name], b[name]))


def check_expectations(code, got, what):
    """plan_host against wide_common.expected_plan, check_host against locate_wide_common.expected_check,
    both built from the code's other host queries (which the twin holds to the rows)."""
    for i, v in enumerate(marks_for(code.k, code.m)):
        for mode, name in ((REPAIR, "repair"), (RECONSTRUCT, "reconstruct")):
            g = got[f"plan_host-{name}-{i}"]
            if not isinstance(g, str):
                assert np.array_equal(g, expected_plan(code, v, mode, True)), f"{what}: plan_host-{name}-{i}"
        g = got[f"check_host-{i}"]
        if not isinstance(g, str):
            assert np.array_equal(g, expected_check(code, v)), f"{what}: check_host-{i}"


@pytest.fixture
def handle():
    made = []

    def new(k, m):
        rs = qa.ReedSolomon(k, m)
        made.append(rs)
        return rs, rs.parity.copy(), rs.m_matrix.copy()

    yield new
    for rs in made:
        rs.close()


def twin_of(rows):
    return qa.Code.from_rows(rows, rs_stale_quirk=True)


@pytest.mark.parametrize("k,m", SHAPES)
def test_host_queries_follow_edits(handle, k, m):
    """Warm on the original matrices, after `scaled`, after `restore`: every answer is the cold
    twin's; every answer that is not a refusal changes with the edit; all return with the restore.
    At (26,4) the constants of the families keyed by an n-bit mask or a pair (locate2_checks) keep
    refusing with one text at every step; decode / repair rows, plans, check plans and the two plain
    row queries (locate_ratios, locate_erased_plan) answer at any width."""
    rs, p0, m0 = handle(k, m)
    s0 = snap(he.step(rs))
    assert not differing(s0, snap(twin_of(p0)))
    check_expectations(he.step(rs), s0, "original")
    answered = {name for name, v in s0.items() if not isinstance(v, str)}
    want = {"rows"} | {n for n in s0 if n.split("-")[0] in ("decode_rows", "repair_rows", "plan_host", "check_host")}
    if k + m <= 24:
        want = set(s0)
    else:  # the erased plan is a host query of any width; the ratios need k <= 32
        want |= {n for n in s0 if n.startswith("locate_erased_plan")} | {"locate_ratios"}
    assert answered == want, sorted(answered ^ want)

    code, rows, full = he.apply(rs, "scaled", p0, m0)
    assert he.consistent(k, rows, full) and np.array_equal(rows, he.scaled_rows(p0))
    s1 = snap(code)
    assert not differing(s1, snap(twin_of(rows))), differing(s1, snap(twin_of(rows)))
    check_expectations(code, s1, "scaled")
    # every check plan is refused now (the rows are not generated ones), with the existing text
    for name in s1:
        if name.startswith("check_host"):
            assert isinstance(s1[name], str) and he.EUNSUP_NOT_GENERATED in s1[name] and f"({QFEC_EUNSUP})" in s1[name]
    # everything else that answered still answers, and differently -- but for what holds no coefficient:
    # a group with nothing marked has no rows, and a refusal for the width keeps its text
    unchanged = set(n for n in s0 if not differing({n: s0[n]}, {n: s1[n]}))
    empty = {n for n in s0 if n.endswith("-3") and not n.startswith(("check_host", "locate_erased_plan"))}
    refusals = {n for n in s0 if isinstance(s0[n], str)}
    assert unchanged == empty | refusals, sorted(unchanged ^ (empty | refusals))
    for name in answered - {n for n in s0 if n.startswith("check_host")}:
        assert not isinstance(s1[name], str), f"{name}: refused after the scaled edit: {s1[name]}"

    code, rows, full = he.apply(rs, "restore", p0, m0)
    s2 = snap(code)
    assert not differing(s2, s0), differing(s2, s0)
    check_expectations(code, s2, "restored")


@pytest.mark.parametrize("k,m", SHAPES)
def test_parity_only_refuses_plans(handle, k, m):
    """rs->parity scaled, rs->m left alone: every plan and check query refuses the handle with the
    existing text; the encode-side constants follow the new rows; decode_rows keeps answering from
    the unchanged rs->m; the restore brings every answer back."""
    rs, p0, m0 = handle(k, m)
    s0 = snap(he.step(rs))
    code, rows, full = he.apply(rs, "parity_only", p0, m0)
    assert not he.consistent(k, rows, full)
    s1 = snap(code)
    for name in s1:
        if name.startswith(("plan_host", "check_host")):
            assert isinstance(s1[name], str) and he.EUNSUP_EDITED in s1[name] and f"({QFEC_EUNSUP})" in s1[name], name
        elif name.startswith("decode_rows"):
            assert same(s1[name], s0[name]), name
    assert np.array_equal(s1["rows"], he.scaled_rows(p0))
    tw = snap(twin_of(rows))
    assert same(s1["locate_ratios"], tw["locate_ratios"]) and not same(s1["locate_ratios"], s0["locate_ratios"])
    assert same(s1["locate2_checks"], tw["locate2_checks"])
    if k + m <= 24:
        assert not same(s1["locate2_checks"], s0["locate2_checks"])
    s2 = snap(he.apply(rs, "restore", p0, m0)[0])
    assert not differing(s2, s0), differing(s2, s0)


@pytest.mark.parametrize("k,m", SHAPES)
def test_zero_col0_refuses_locate(handle, k, m):
    """A zero coefficient at data shard 0: locate_ratios, locate2_checks refuse with the existing text
    (locate_code_check); the erased plan, which only reports rows, follows the edit like the twin's;
    the restore brings every answer back."""
    rs, p0, m0 = handle(k, m)
    s0 = snap(he.step(rs))
    code, rows, full = he.apply(rs, "zero_col0", p0, m0)
    assert rows[he.ZERO_ROW, 0] == 0 and he.consistent(k, rows, full)
    s1 = snap(code)
    for name in ("locate_ratios", "locate2_checks"):
        assert isinstance(s1[name], str) and he.EUNSUP_ZERO in s1[name] and f"({QFEC_EUNSUP})" in s1[name], s1[name]
    assert not differing(s1, snap(twin_of(rows)))
    for entry in ("qfec_locate_erased", "qfec_locate", "qfec_locate2"):
        rc, text = empty_call(entry, code)
        assert rc == QFEC_EUNSUP and he.EUNSUP_ZERO in text, (entry, rc, text)
    s2 = snap(he.apply(rs, "restore", p0, m0)[0])
    assert not differing(s2, s0), differing(s2, s0)


# ------------------------------------------------------------------ the acceptance checks behind the device calls

def empty_call(entry, code):
    """A batched locate entry with groups = 0: the code is judged on the host (batch_begin) and no
    device is asked for.  -> (rc, error text)"""
    L = qa.lib()
    args = [code._h, None, None] + ([None] if entry == "qfec_locate_erased" else []) + [0, 16, 16, None, None, None, None]
    rc = getattr(L, entry)(*args)
    return rc, L.qfec_last_error().decode() if rc else ""


@pytest.mark.parametrize("k,m", [(6, 4), (8, 4)])
def test_erased_host_tables_follow_edits(handle, k, m):
    """The locate-erased host tables (le_host_version) are also the acceptance check of their family.
    Warm and accepted; `scaled` stays accepted; parity row 1 := row 0 keeps every coefficient non-zero
    (locate_code_check passes) but makes a punctured code singular, which only a rebuild of the tables
    finds: the call must refuse with the text a cold twin gets; accepted again after the restore."""
    rs, p0, m0 = handle(k, m)
    assert empty_call("qfec_locate_erased", he.step(rs)) == (0, "")
    assert empty_call("qfec_locate_erased", he.apply(rs, "scaled", p0, m0)[0]) == (0, "")
    code, rows, _ = he.apply(rs, "dup_row1", p0, m0)
    got = empty_call("qfec_locate_erased", code)
    assert got[0] == QFEC_EUNSUP and "the punctured code is not MDS" in got[1], got
    assert got == empty_call("qfec_locate_erased", twin_of(rows))
    assert empty_call("qfec_locate_erased", he.apply(rs, "restore", p0, m0)[0]) == (0, "")
