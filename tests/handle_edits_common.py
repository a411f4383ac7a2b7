"""Shared by test_handle_edits_host.py and test_gpu_handle_edits.py: edits of a LIVE reed_solomon handle.

module/rs.h lets a caller write into rs->parity and rs->m between calls.  sync_rows
(qfec_rs_abi.cpp) notices on the next ABI entry and in qfec_rs_code, and bumps qfec_code::version;
everything the library derives from a code carries a stamp of the version it was built from
(qfec_rt.hpp).  The tests here use a handle, edit it, and use it again: a cache whose stamp is not
compared then answers from the previous matrices.

torch is not imported here, so the CPU suite can import this module."""
import numpy as np

from wide_common import gf_tables

_EXP, _LOG = gf_tables()


def gf_mul(a, b):
    """GF(2^8) product, polynomial 0x11D (wide_common.gf_tables)."""
    return 0 if a == 0 or b == 0 else int(_EXP[_LOG[a] + _LOG[b]])


def scaled_rows(parity):
    """Parity row j multiplied by the constant j + 2.  Every minor of [I; D.P] is a non-zero multiple
    of the same minor of [I; P], so the code stays MDS under every puncturing and no coefficient
    becomes zero; every coefficient, every ratio P[j][i] / P[0][i] (j >= 1), every decode row and
    every repair row changes."""
    out = np.array(parity, np.uint8)
    for j in range(out.shape[0]):
        for i in range(out.shape[1]):
            out[j, i] = gf_mul(int(parity[j, i]), j + 2)
    return out


ZERO_ROW = 1  # the parity row zero_col0 edits


def _write(rs, parity, full):
    rs.parity[:] = parity
    rs.m_matrix[:] = full


def scaled(rs, parity0, m0):
    """rs->parity and rows k.. of rs->m scaled: rs->m is [I; rows] again."""
    full = m0.copy()
    full[rs.k:] = scaled_rows(parity0)
    _write(rs, scaled_rows(parity0), full)


def parity_only(rs, parity0, m0):
    """The same scaling in rs->parity alone: the encode side follows the new rows, reconstruct keeps
    decoding from the unchanged rs->m, and every plan and check entry refuses the handle."""
    _write(rs, scaled_rows(parity0), m0)


def zero_col0(rs, parity0, m0):
    """rs->parity[ZERO_ROW][0] = 0, mirrored into rs->m: the rs.c stale-row quirk for the encode and
    the reconstruct, a refusal for the locate families."""
    p, full = parity0.copy(), m0.copy()
    p[ZERO_ROW, 0] = 0
    full[rs.k + ZERO_ROW, 0] = 0
    _write(rs, p, full)


def dup_row1(rs, parity0, m0):
    """Parity row 1 := parity row 0 in both matrices.  No coefficient is zero, so locate_code_check
    passes, but with one data shard lost the second spare row is the first one over again: the
    punctured code is not MDS, which only a rebuild of the locate-erased host tables (le_host_version)
    finds out."""
    p, full = parity0.copy(), m0.copy()
    p[1] = p[0]
    full[rs.k + 1] = p[0]
    _write(rs, p, full)


def restore(rs, parity0, m0):
    _write(rs, parity0, m0)


EDITS = {"scaled": scaled, "parity_only": parity_only, "zero_col0": zero_col0, "dup_row1": dup_row1, "restore": restore}


def step(rs):
    """The code of the handle's CURRENT matrices.  qfec_rs_code is what syncs, so it is fetched again
    after every edit; a Code object from before an edit is not the subject of these tests."""
    return rs.code()


def apply(rs, name, parity0, m0):
    """Edit the handle, then -> (code, parity rows, rs->m) of the step."""
    EDITS[name](rs, parity0, m0)
    return step(rs), rs.parity.copy(), rs.m_matrix.copy()


def consistent(k, rows, full):
    """Is rs->m equal to [I; rows]?  Only then does a Code.from_rows twin model the handle."""
    return np.array_equal(full[:k], np.eye(k, dtype=np.uint8)) and np.array_equal(full[k:], rows)


EUNSUP_EDITED = "the code's rs.c decode matrix is not [I; rows] (edited handle)"
EUNSUP_NOT_GENERATED = "the parity rows are not those qfec_code_new generates"
EUNSUP_ZERO = f"parity row {ZERO_ROW} has a zero coefficient at data shard 0"

_GPU = "tests/test_gpu_handle_edits.py::"
_CPU = "tests/test_handle_edits_host.py::"

# every version stamp of qfec_rt.hpp -> the tests that warm that cache, edit the handle and read the
# cache again (test_handle_edits_host.py holds the keys to the source and the ids to the two files)
CACHES = {
    "enc_version": [_GPU + "test_encode_side", _GPU + "test_locate", _GPU + "test_plans_wide", _GPU + "test_order"],
    "dec.version": [_GPU + "test_reconstruct", _GPU + "test_abi", _GPU + "test_order"],
    "rep.version": [_GPU + "test_repair", _GPU + "test_locate", _GPU + "test_order"],
    "le.version": [_GPU + "test_locate_erased", _GPU + "test_order"],
    "loc_version": [_GPU + "test_locate", _GPU + "test_order"],
    "loc2_version": [_GPU + "test_locate2", _GPU + "test_order"],
    "rec_cache_version": [_GPU + "test_reconstruct"],
    "lut_seed_version": [_GPU + "test_abi"],
    "le_host_version": [_CPU + "test_erased_host_tables_follow_edits", _GPU + "test_locate_erased"],
    "l2_host_version": [_CPU + "test_host_queries_follow_edits", _GPU + "test_locate2"],
    "plan_chk_version": [_CPU + "test_parity_only_refuses_plans", _GPU + "test_plans_wide", _GPU + "test_abi"],
    "check_chk_version": [_CPU + "test_host_queries_follow_edits", _GPU + "test_check_plans"],
}
