"""CPU: the send model and case table of tests/tx_common.py held to what they stand on, and the
coverage they owe the GPU test (tests/test_gpu_tx_model.py).

* tx_common.send_form against send_form of quicknet_amd/csrc/qfec_geom.hpp -- the function the
  launchers of qfec_wire.hip follow -- for every case of the table; every form name occurs; every
  QFEC_PACK_CASE / QFEC_PFC shape of the source is in the table under every form it can take.
  tests/send_geom_host/shim.cpp is compiled here with g++;
* the partial sums the checksummed body forms leave in d_shards fit in it at every legal shard pitch;
* at 2^31 groups the launches cover the batch in order, each within its limits;
* the model against the datagrams network/FecCodecBuf.cpp itself produced (tests/golden/wire_c*.npz);
* every batch holds every scenario it promises, twice, at group indices of opposite parity."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tx_common as tc
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "send_geom_host", "shim.cpp")
HDR = os.path.join(ROOT, "quicknet_amd", "csrc", "qfec_geom.hpp")
OUT = os.path.join(ROOT, "tests", "send_geom_host", "_build", "libsend_geom_shim.so")
CSRC = os.path.join(ROOT, "quicknet_amd", "csrc")

# SendKind of qfec_geom.hpp, in order
KINDS = ("staged", "wave1", "wave2", "wave8x3", "wave16x2", "body+line0", "body+head", "body11-line", "body11", "two-call")
WIRE = [(4, 5), (4, 6), (3, 5), (5, 8), (7, 8), (10, 13), (2, 4), (3, 4), (14, 15), (1, 2)]  # the golden (k, n)


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", OUT, SRC], check=True)
    L = C.CDLL(OUT)
    L.send_form.restype = C.c_int
    L.send_form.argtypes = [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.POINTER(C.c_uint),
                            C.POINTER(C.c_longlong)]
    L.send_part_words.restype = C.c_ulonglong
    L.send_part_words.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_ulonglong]
    L.send_chunks.restype = C.c_longlong
    L.send_chunks.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong, C.POINTER(C.c_longlong)]
    return L


Form = collections.namedtuple("Form", "name line gpw ts tn lpg rec_words per")


def host_form(L, instance, n, checksum, pitch, row_pitch, prefix):
    out = (C.c_uint * 6)()
    per = C.c_longlong(0)
    kind = L.send_form(int(instance), n, checksum, pitch, row_pitch, prefix, out, C.byref(per))
    return Form(KINDS[kind], *out, per.value)


def library_form(L, c):
    """What the library does with a case: the launchers ask send_form only where the fused send is on
    and an instance exists; otherwise the datagram call is staged and the frame call two calls."""
    inst = (c.k, c.m) in tc.PACK_SHAPES
    if not (c.fused and inst):
        return "two-call" if c.prefix else "staged"
    return host_form(L, True, c.k + c.m, c.checksum, c.shard_pitch, c.row_pitch, c.prefix).name


def source_shapes(macro):
    with open(os.path.join(CSRC, "qfec_wire.hip")) as f:
        return [(int(k), int(m)) for k, m in re.findall(rf"^\s*{macro}\((\d+),\s*(\d+)\)", f.read(), re.M)]


# ------------------------------------------------------------------ the case table

def test_send_form_is_the_librarys(shim):
    cases = tc.datagram_cases() + tc.frame_cases()
    assert len({tc.case_id(c) for c in cases}) == len(cases)
    for c in cases:
        assert c.form == tc.send_form(c.k, c.m, c.checksum, c.shard_pitch, c.row_pitch, c.prefix, c.fused)
        assert c.form == library_form(shim, c), tc.case_id(c)
        # the arguments are ones the entry points accept
        assert c.shard_pitch % 16 == 0 and c.row_pitch % 16 == 0 and c.k + c.m <= 15
        assert c.row_pitch >= (c.shard_pitch + 13 + 15) // 16 * 16 and c.row_pitch >= c.shard_pitch + 13 + c.prefix
    assert {c.form for c in cases} == set(tc.FORMS) == set(KINDS)
    assert {c.form for c in tc.single_group_cases()} == set(tc.FORMS)
    # without an instance the host function says so itself
    assert host_form(shim, False, 8, 1, 1040, 1088, 0).name == "staged"
    assert host_form(shim, False, 8, 1, 1040, 1088, 4).name == "two-call"


def test_send_form_over_every_pitch(shim):
    """The Python restatement against the host function well beyond the table: every shard pitch, every
    row pitch from the smallest legal one to three lines above it, every prefix, both checksum modes."""
    for sp in range(16, 2065, 16):
        for c in (1, 0):
            for fp in (0, 4, 12):
                lo = (sp + 13 + fp + 15) // 16 * 16
                for rp in range(lo, lo + 208, 16):
                    assert tc.send_form(10, 3, c, sp, rp, fp) == host_form(shim, True, 13, c, sp, rp, fp).name, (sp, rp, c, fp)


def test_the_table_names_every_instance():
    for macro in ("QFEC_PACK_CASE", "QFEC_PFC"):
        src = source_shapes(macro)
        assert src and len(set(src)) == len(src)
        assert sorted(src) == sorted(tc.PACK_SHAPES), macro
    assert not set(tc.STAGED_SHAPES) & set(tc.PACK_SHAPES)
    dg, fr = tc.datagram_cases(), tc.frame_cases()
    for km in tc.PACK_SHAPES:
        forms = {c.form for c in dg if (c.k, c.m) == km}
        assert {"wave1", "wave2", "body+head", "body+line0", "body11-line", "body11", "staged"} <= forms, km
        for fp in (4, 12):
            assert {"wave1", "wave2"} <= {c.form for c in fr if (c.k, c.m) == km and c.prefix == fp}, (km, fp)
    for km in tc.THREE:
        assert "wave8x3" in {c.form for c in dg if (c.k, c.m) == km}
        for fp in (4, 12):
            assert {"wave8x3", "wave16x2", "two-call"} <= {c.form for c in fr if (c.k, c.m) == km and c.prefix == fp}
    for km in tc.STAGED_SHAPES:
        assert {c.form for c in dg if (c.k, c.m) == km} == {"staged"}
        assert {c.fused for c in dg if (c.k, c.m) == km} == {0, 1}
    # every fused datagram case runs staged as well
    for c in dg:
        if c.fused and c.form != "staged":
            assert c._replace(form="staged", fused=0) in dg


def test_body_geometry(shim):
    """The geometry the case table leans on: the lpg clamp at the smallest pitches, the smallest line
    form, a line pitch too short for one, the one-wave forms' fixed split."""
    f = host_form(shim, True, 13, 1, 16, 32, 0)
    assert (f.name, f.ts, f.tn, f.lpg) == ("body+head", 1, 2, 16)      # one live lane of 16
    f = host_form(shim, True, 13, 0, 16, 32, 0)
    assert (f.name, f.ts, f.tn, f.lpg) == ("body11", 0, 2, 16)
    f = host_form(shim, True, 13, 1, 304, 320, 0)
    assert (f.name, f.line, f.ts, f.tn, f.lpg) == ("body+line0", 1, 4, 20, 16)
    f = host_form(shim, True, 13, 0, 304, 320, 0)
    assert (f.name, f.line, f.ts, f.tn, f.lpg) == ("body11-line", 1, 0, 20, 20)
    f = host_form(shim, True, 13, 1, 240, 256, 0)                       # a line pitch under 20 chunks
    assert (f.name, f.line, f.lpg) == ("body+head", 0, 16)
    f = host_form(shim, True, 13, 1, 1616, 1664, 0)
    assert (f.name, f.lpg, f.rec_words) == ("body+line0", 100, 14)
    for name, rp, gpw in (("wave1", 1088, 1), ("wave2", 576, 2), ("wave8x3", 1152, 1)):
        f = host_form(shim, True, 13, 1, rp - 48, rp, 0)
        assert (f.name, f.gpw, f.lpg, f.rec_words, f.per) == (name, gpw, 0, 0, 1 << 28)


def test_partial_sums_fit_in_d_shards(shim):
    """The checksummed body forms write one record per 16-lane row of the body into d_shards, groups
    back to back: never more than the groups * n * shard_pitch bytes the caller gave, G = 1 included."""
    ns = sorted({k + m for k, m in tc.PACK_SHAPES})
    most = 0.0
    for sp in range(16, 2065, 16):
        lo = (sp + 13 + 15) // 16 * 16
        for rp in sorted({lo, lo + 16, tc.line_above(13 + sp), tc.line_above(13 + sp) + 64, 2 * lo}):
            for n in ns:
                f = host_form(shim, True, n, 1, sp, rp, 0)
                if f.name not in ("body+line0", "body+head"):
                    assert f.rec_words == 0 and shim.send_part_words(n, 1, sp, rp, 1000) == 0
                    continue
                assert f.rec_words == 2 * ((n + 1) // 2) and f.lpg >= 16 and f.lpg == max(16, f.tn - f.ts)
                for G in (1, 2, 3, 15, 16, 17, 77, 4096):
                    words = shim.send_part_words(n, 1, sp, rp, G)
                    assert words == -(-G * f.lpg // 16) * f.rec_words
                    assert 4 * words <= G * n * sp, (sp, rp, n, G)
                    most = max(most, 4 * words / (G * n * sp))
    assert 0.25 < most <= 1.0   # the tightest case is the 16-B pitch, not a vacuous bound
    # without checksums the body keeps no sums
    assert host_form(shim, True, 13, 0, 304, 320, 0).rec_words == 0


@pytest.mark.parametrize("sp,rp,fp", [(1040, 1088, 0), (528, 576, 0), (1104, 1152, 0), (16, 32, 0), (304, 320, 0),
                                      (1616, 1664, 0), (2048, 2064, 0), (2064, 2112, 12)])
def test_launches_beyond_2_31_groups(shim, sp, rp, fp):
    f = host_form(shim, True, 13, 1, sp, rp, fp)
    most = C.c_longlong(0)
    G = (1 << 31) + 5
    if f.gpw:  # whole waves per group: 2^28 groups a launch, a grid of 2^26 blocks at the most
        n = shim.send_chunks(G, f.per, 1, C.byref(most))
        assert n == -(-G // f.per) == 9 and most.value == 1 << 28
        assert -(-most.value // (4 * f.gpw)) <= 0x7FFFFFFF
    else:  # the body's lanes are a u32, and every launch starts on a whole 16-lane row
        assert f.per % 16 == 0 and f.per >= 16
        n = shim.send_chunks(G, f.per, 16, C.byref(most))
        assert n == -(-G // f.per) and n > 1 and most.value == f.per
        assert most.value * f.lpg <= 1 << 30 and (most.value + 16) * f.lpg > 1 << 30
        assert (most.value * f.lpg + 255) // 256 * 256 < 1 << 32
    assert shim.send_chunks(0, f.per, 1, C.byref(most)) == 0
    assert shim.send_chunks(f.per + 1, f.per, 1, C.byref(most)) == 2


# ------------------------------------------------------------------ the model

@pytest.mark.parametrize("k,n", WIRE)
@pytest.mark.parametrize("checksum", [1, 0])
def test_model_vs_golden(oracle, golden, k, n, checksum):
    """tx_model over the reference's own inputs reproduces its datagrams and lengths, for every key."""
    z = golden(f"wire_c{checksum}.npz")
    key = f"{k}_{n}_{checksum}"
    sizes, payload, seq = z[f"sizes_{key}"], z[f"payload_{key}"], z[f"seq_{key}"]
    dg, dl = z[f"dgrams_{key}"], z[f"dlen_{key}"]
    G = dg.shape[0]
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64).reshape(G, k)
    sp = (int(sizes.max()) + (4 if checksum else 2) + 15) // 16 * 16
    mod = tc.tx_model(oracle, k, n - k, checksum, sp, dg.shape[2], 0, sizes.reshape(G, k).astype(np.int32), offs,
                      seq.astype(np.uint32), payload)
    assert not mod.void.any()
    assert np.array_equal(mod.lens, dl)
    assert np.array_equal(mod.rows, dg)
    tc.check_output(tuple(f"golden-{g}" for g in range(G)), mod, dg, dl.astype(np.int32), "zero", key)


def test_every_golden_key_is_covered(golden):
    for c in (0, 1):
        keys = {k_[len("dgrams_"):] for k_ in golden(f"wire_c{c}.npz").files if k_.startswith("dgrams_")}
        assert keys == {f"{k}_{n}_{c}" for k, n in WIRE}


def test_void_rule_and_frames(oracle):
    """Sizes at the bounds: 0 and M are packed, -1, M + 1, INT_MIN, INT_MAX and INT_MAX - 3 void the
    whole group; a frame is oracle.frame_udp of the datagram and unframes to it."""
    k, m, sp = 3, 2, 48
    M = tc.max_size(sp, 1)
    sizes = np.array([[0, M, 5], [-1, 1, 1], [1, M + 1, 1], [tc.INT_MIN, 0, 0], [0, 0, tc.INT_MAX], [tc.INT_MAX - 3, 0, 0]],
                     np.int32)
    G = len(sizes)
    offs = np.tile(np.arange(k, dtype=np.int64) * 50, (G, 1))
    payload = (np.arange(400) * 7 + 1).astype(np.uint8)
    seq = np.tile(np.array([[0xFFFFFFFE, 0xFFFFFFFF]], np.uint32), (G, 1))
    masks = np.full((G, k + m), 0x3C, np.uint8)
    ch = np.full((G, k + m, 2), 0xFFFFFFFF, np.uint32)
    dgm = tc.tx_model(oracle, k, m, 1, sp, 64, 0, sizes, offs, seq, payload)
    assert dgm.void.tolist() == [False] + [True] * 5 and (dgm.lens[1:] == -1).all() and not dgm.rows[1:].any()
    assert dgm.lens[0].tolist() == [17, 17 + M, 22, 17 + M, 17 + M]
    sent = [int.from_bytes(bytes(dgm.rows[0, j, 1:5]), "little") for j in range(k + m)]
    src = [int.from_bytes(bytes(dgm.rows[0, j, 5:9]), "little") for j in range(k + m)]
    assert sent == [0xFFFFFFFE, 0xFFFFFFFF, 0, 1, 2] and src == [0xFFFFFFFF, 0, 1, 1, 1]  # both wrap past 2^32
    for fp in (4, 12):
        fm = tc.tx_model(oracle, k, m, 1, sp, 128, fp, sizes, offs, seq, payload, masks, ch, cmd=0xFF, protocol=0x00)
        assert np.array_equal(fm.lens[0], dgm.lens[0] + fp) and (fm.lens[1:] == -1).all()
        for j in range(k + m):
            st, work, _ = oracle.unframe_udp(fm.rows[0, j, :fm.lens[0, j]], gmask=tc.GMASK, session=fp == 12)
            assert st == 0 and np.array_equal(work[fp:], dgm.rows[0, j, :dgm.lens[0, j]])
            assert work[2] == 0xBF and work[3] == 0x00
    # check_output: the model's own rows pass; one changed byte, one byte past the end, a written void row fail
    names = tuple("abcdef")
    got = np.where(np.arange(64) < dgm.lens[:, :, None], dgm.rows, tc.SENTINEL).astype(np.uint8)
    tc.check_output(names, dgm, got, dgm.lens, "zero-or-sentinel", "self")
    with pytest.raises(AssertionError, match="past a row's end"):
        tc.check_output(names, dgm, got, dgm.lens, "zero", "self")
    for g, j, at, why in ((0, 4, 3, "row bytes"), (0, 2, 40, "past a row's end"), (3, 1, 0, "void group")):
        bad = got.copy()
        bad[g, j, at] ^= 0x10
        with pytest.raises(AssertionError, match=why):
            tc.check_output(names, dgm, bad, dgm.lens, "zero-or-sentinel", "self")
    bad_len = dgm.lens.copy()
    bad_len[2, 1] = 17
    with pytest.raises(AssertionError, match=r"lengths, 1 groups, first 2 \(c\)"):
        tc.check_output(names, dgm, got, bad_len, "zero-or-sentinel", "self")


# ------------------------------------------------------------------ coverage the GPU test relies on

def expected_names(k, m, checksum, prefix):
    """The scenario list as the test plan states it, written out here and not taken from the builder."""
    out = ["zero", "one", "max", "max-1", "single-first", "single-last", "ff-max", "zero-bytes-max", "line0-0",
           "pass-edges-0", "ramp", "random", "alias", "seq-wrap", "seq-high", "neg", "int-min", "over", "over-int-max",
           "over-int-max-3"]
    if prefix:
        out += ["mask-00", "mask-ff", "mask-cancel", "conv-0", "conv-ff"]
    return out


BATCHES = sorted({(c.k, c.m, c.checksum, c.shard_pitch, c.row_pitch, c.prefix) for c in tc.datagram_cases() + tc.frame_cases()})


@pytest.mark.parametrize("k,m,checksum,sp,rp,fp", BATCHES, ids=[f"{k}-{m}-c{c}-{sp}-{rp}-fp{fp}" for k, m, c, sp, rp, fp in BATCHES])
def test_scenarios_cover(k, m, checksum, sp, rp, fp):
    b = tc.batch(k, m, checksum, sp, rp, fp)
    names, skipped = tc.promised(k, m, checksum, sp, rp, fp)
    G, n, M = len(b.names), k + m, tc.max_size(sp, checksum)
    assert G <= 100 and G % 2 == 1
    for want in expected_names(k, m, checksum, fp):
        assert want in names or skipped.get(want), f"{want} neither built nor excused"
    for name in names:  # each promised scenario: twice, at group indices of opposite parity
        at = [g for g in range(G) if b.names[g] == name]
        assert len(at) == 2 and (at[0] + at[1]) % 2 == 1, (name, at)
    assert "ordinary" in b.names
    at = {name: [g for g in range(G) if b.names[g] == name] for name in names}
    head = 4 if checksum else 2
    over = fp + (13 if checksum else 11) + head
    # the sizes the names stand for
    for name, val in (("zero", 0), ("one", 1), ("max", M), ("max-1", M - 1), ("ff-max", M), ("zero-bytes-max", M)):
        for g in at[name]:
            assert (b.sizes[g] == val).all(), name
    for g in at["ff-max"] + at["zero-bytes-max"]:
        want = 0xFF if b.names[g] == "ff-max" else 0
        for i in range(k):
            assert (b.payload[b.offs[g, i]:b.offs[g, i] + M + 16] == want).all()
    # every edge: rows ending one byte before, on and after the 64-B line the passes start from
    ends = {int(s) + over for g in range(G) if not b.void[g] for s in b.sizes[g]}
    for cut in range(0, rp, 512):
        for d in (-1, 0, 1):
            if over <= 64 + cut + d <= over + M:
                assert 64 + cut + d in ends, (cut, d)
    for L in (15, 16, 17, 63, 64, 65):
        if over <= L <= over + M:
            assert L in ends
    if rp == 576:
        assert {319, 320, 321} <= ends
    # void groups by the stated rule, with the stated values, at valid offsets with room behind them
    assert b.void.sum() == 10
    vals = {"neg": -1, "int-min": tc.INT_MIN, "over": M + 1, "over-int-max": tc.INT_MAX, "over-int-max-3": tc.INT_MAX - 3}
    for name, v in vals.items():
        for g in at[name]:
            assert b.void[g] and (b.sizes[g] == v).sum() == 1 and ((b.sizes[g] < 0) | (b.sizes[g] > M)).sum() == 1
            assert b.offs[g].min() >= 0 and b.offs[g].max() + sp + 16 <= len(b.payload)
    assert b.sizes[at["neg"][0], 0] == -1 and b.sizes[at["over"][1], k - 1] == M + 1
    # a void group beside a live one on either side of a wave of two
    for name in vals:
        assert sorted(g % 2 for g in at[name]) == [0, 1]
        assert all((g ^ 1) < G and not b.void[g ^ 1] for g in at[name]), name
    # live rows: offsets and sizes inside the buffer with the 16 readable bytes the call asks for
    for g in range(G):
        if not b.void[g]:
            assert b.offs[g].min() >= 0 and int((b.offs[g] + b.sizes[g]).max()) + 16 <= len(b.payload)
    eq, desc = at["alias"]
    assert len(set(b.offs[eq].tolist())) == 1 and b.offs[eq, 0] % 2 == 1
    assert (np.diff(b.offs[desc]) < 0).all() and (b.offs[desc] % 2 == 1).all()
    assert [tuple(b.seq[g]) for g in at["seq-wrap"]] == [(0xFFFFFFFD, 0xFFFFFFFE)] * 2
    assert [tuple(b.seq[g]) for g in at["seq-high"]] == [(0x89ABCDEF, 0x7654321F)] * 2
    assert (b.seq[b.names.index("ordinary")] > 0xFFFF).all()  # ordinary groups: header bytes above the low one non-zero
    if fp:
        for name, v in (("mask-00", 0), ("mask-ff", 0xFF), ("mask-cancel", tc.GMASK ^ 0x5A)):
            for g in at[name]:
                assert (b.masks[g] == v).all()
        assert (tc.GMASK ^ 0x5A) ^ tc.GMASK ^ 0x5A == 0
        if fp == 12:
            assert all((b.conv_hid[g] == 0).all() for g in at["conv-0"])
            assert all((b.conv_hid[g] == 0xFFFFFFFF).all() for g in at["conv-ff"])
        else:
            assert skipped["conv-0"] and skipped["conv-ff"]


def test_single_group_batches():
    for c in tc.single_group_cases():
        b = tc.batch(c.k, c.m, c.checksum, c.shard_pitch, c.row_pitch, c.prefix, "max")
        assert b.names == ("max",) and (b.sizes == tc.max_size(c.shard_pitch, c.checksum)).all()


def test_ff_max_reaches_the_checksum_bounds(oracle):
    """ff-max at a 1040-B shard pitch: a data row's payload sum passes 2^16 many times over (the head's
    fold), its datagram sum too, and a 16-lane row of the body sums to the stated bound of 65280."""
    b, mod = tc.batch_model(oracle, 10, 3, 1, 1040, 1088, 0)
    g = b.names.index("ff-max")
    assert int(b.payload[b.offs[g, 0]:b.offs[g, 0] + 1036].astype(np.int64).sum()) == 1036 * 255 > 4 * 65536
    assert 16 * 16 * 255 == 65280
    row = mod.rows[g, 0]
    assert (row[17:17 + 1036] == 0xFF).all() and mod.lens[g, 0] == 1053
    assert int(row[11]) | int(row[12]) << 8 == int(row[13:1053].astype(np.int64).sum()) & 0xFFFF
