"""CPU tests that hold dispatch_common's shape sets to the source: INSTANCES must list exactly the
(k, m) pairs of every QFEC_*_CASE list in quicknet_amd/csrc/*.hip and the a.m == 1..4 ladder of
qfec_update.hip, so an instance added later without a GPU case in test_gpu_dispatch.py fails here.
Only the (k, m) numbers of the source are read.  Also: the rules the shapes promise (group counts,
part-empty last blocks, unique ids) and the host-side models on a batch small enough to reason about."""
import glob
import os
import re

import numpy as np
import pytest

import dispatch_common as dc
from locate2_common import AMBIGUOUS, CLEAN, MULTI, expected_locate2

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quicknet_amd", "csrc")
MACRO = {"verify": "VER", "locate": "LOC", "locate2": "LOC2", "locate_erased": "LE", "repair": "REP"}


def source_cases(macro):
    """The (k, m) of every QFEC_<macro>_CASE(k, m) line with literal numbers, over all .hip files."""
    out = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        with open(path) as f:
            out += [(int(k), int(m)) for k, m in re.findall(rf"^\s*QFEC_{macro}_CASE\((\d+),\s*(\d+)\)", f.read(), re.M)]
    return out


@pytest.mark.parametrize("family", sorted(MACRO))
def test_instances_are_the_source_lists(family):
    src = source_cases(MACRO[family])
    assert src, f"no QFEC_{MACRO[family]}_CASE line found"
    assert len(set(src)) == len(src)
    listed = dc.INSTANCES[family]
    assert len(set(listed)) == len(listed)
    assert sorted(listed) == sorted(src), (
        f"{family}: dispatch_common.INSTANCES and the QFEC_{MACRO[family]}_CASE list differ: "
        f"only in the source {sorted(set(src) - set(listed))}, only in INSTANCES {sorted(set(listed) - set(src))}")


def test_update_instances_are_the_ladder():
    with open(os.path.join(CSRC, "qfec_update.hip")) as f:
        text = f.read()
    want = sorted(m for _, m in dc.INSTANCES["update"])
    for kernel in ("k_update_perm", "k_encupd_perm"):
        rungs = re.findall(rf"a\.m == (\d+)\) hipLaunchKernelGGL\({kernel}<(\d+)>", text)
        assert rungs and all(a == b for a, b in rungs)
        assert sorted(int(a) for a, _ in rungs) == want, f"{kernel}: rungs {rungs} against INSTANCES['update'] {want}"


def test_encode_extras_are_instances():
    assert set(dc.ENCODE_EXTRA) <= set(source_cases("ENC"))


@pytest.mark.parametrize("family", sorted(dc.INSTANCES))
def test_every_branch_has_a_case(family):
    got = set(dc.cases(family))
    ids = dc.case_ids(family)
    assert len(set(ids)) == len(ids) == len(dc.cases(family))
    instances = set(dc.INSTANCES[family])
    for km in dc.INSTANCES[family]:
        assert km + ("fast",) in got
    for km in dc.GENERIC[family]:
        assert km not in instances
        assert all(km + (l,) in got for l in ("fast",) + dc.WIDE)
    assert all((20, 4, l) in got for l in ("fast",) + dc.WIDE)
    for km in dc.LIMITS[family]:
        assert km + ("fast",) in got and km + ("bytes-data-off",) in got
    # the generic shapes: one row chunk of four, and two
    assert sorted((m + 3) // 4 for _, m in dc.GENERIC[family]) == [1, 2]


def test_group_counts():
    for family in dc.INSTANCES:
        for k, m, lname in dc.cases(family):
            G, n, layout = dc.groups_for(k, m), k + m, dc.LAYOUTS[lname]
            assert G in (3 * n + 2, 3 * n + 3) and G % 2 == 1 and G % 4
            assert (G * dc.lanes(layout)) % 256, (k, m, lname)
            assert dc.byte_path(layout) == (lname.startswith("bytes"))
            assert layout.B <= layout.pitch and max(dc.second_pass(layout.B)) < layout.B - 2


def test_layouts_reach_what_they_claim():
    L = dc.LAYOUTS
    assert dc.lanes(L["fast"]) == 7 and L["fast"].B % 16 == 4
    assert dc.lanes(L["fast-wide"]) == 69 and (69 + 63) // 64 == 2 and (2 * 69 + 63) // 64 == 3
    assert L["bytes-pitch"].pitch % 16 and L["bytes-pitch"].B > 256 and (L["bytes-pitch"].B + 63) // 64 == 5
    for name in dc.OFF_BASE:
        offs = (L[name].data_off, L[name].parity_off, L[name].rows_off)
        assert sum(o != 0 for o in offs) == 1 and L[name].pitch % 16 == 0 and (L[name].B, L[name].pitch) == (100, 128)
    assert dc.written_from(L["fast"]) == 112 and dc.written_from(L["bytes-data-off"]) == 100


def test_damage_kinds_cover_the_passes():
    for B, firsts in ((100, [64]), (300, [64, 256]), (1100, [1024])):
        kinds = dict(dc.damage_kinds(B))
        assert kinds["b0"] == [(0, 0x01)] and kinds["last"][0][0] == B - 1 and kinds["row"] is None
        assert [kinds[f"b{p}"][0][0] for p in firsts] == firsts
        (lo, _), (hi, _) = kinds["two"]
        assert lo < 64 and hi >= max(firsts)


def test_models_on_a_small_batch(oracle):
    """(4,4), 100 bytes: the single-shard model agrees with the first stage of expected_locate2 on
    clean, one-shard, two-shard and same-byte two-shard groups, and the verify model names the rows
    by construction."""
    k, m, B = 4, 4, 100
    layout = dc.Layout("", B, 128, 0, 0, 0)
    rows, d, p = dc.batch(oracle, k, m, layout)
    assert not dc.bad_rows_model(oracle, rows, d, p, B).any()
    assert (dc.expected_locate1(oracle, rows, d, p, B) == CLEAN).all()
    made = dc.damage_every_shard(d, p, B)
    d[0, 0, 3] ^= 0x10            # two shards, different bytes
    p[0, 1, B - 2] ^= 0x04
    d[3, 1, 5] ^= 0x21            # two shards, the same byte
    d[3, 2, 5] ^= 0x9E
    p[6, 2, B] ^= 0xFF            # beyond the block: not damage
    made[[0, 3]] = MULTI
    one = dc.expected_locate1(oracle, rows, d, p, B)
    two = expected_locate2(oracle, rows, "cauchy", d, p, B)
    assert np.array_equal(one, made)
    single = two[:, 1] == CLEAN
    assert np.array_equal(two[single, 0], one[single])
    assert [tuple(two[g]) for g in (0, 3)] == [(0, k + 1), (1, 2)]
    assert dc.counts_of1(one) == [k + m, 2, 0] and AMBIGUOUS not in one
    bits = dc.bad_rows_model(oracle, rows, d, p, B)
    assert bits.dtype == np.uint32
    assert [int(bits[3 * (k + j) + 1]) for j in range(m)] == [1, 2, 4, 8]
    assert bits[0] == 0b1111 and bits[1] == 0b1111 and bits[2] == 0 and bits[6] == 0
    gm = dc.marks_n(two, k + m)
    assert gm[0].tolist() == [1, 0, 0, 0, 0, 1, 0, 0] and gm.sum() == k + m + 4


def test_bad_rows_model_reaches_bit_31(oracle):
    k, m, B = 2, 32, 20
    rows, d, p = dc.batch(oracle, k, m, dc.Layout("", B, 32, 0, 0, 0))
    p[4, 31, B - 1] ^= 1
    bits = dc.bad_rows_model(oracle, rows, d, p, B)
    assert bits[4] == 0x80000000 and bits.view(np.int32)[4] < 0 and not np.delete(bits, 4).any()
