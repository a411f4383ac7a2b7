"""GPU: every receive path -- the four compiled forms of the fused k_rx under the five wire_rx
settings that reach them, the staged path (k_parse_wire -> reconstruct -> k_check_payloads) and the
two-call frame fallback -- held bit for bit to the CPU model of tests/rx_common.py on hostile input:
multi-round retries, header rejects, mixed tags, bytes after the payload, dec_pkt_size, damaged
frames.  qfec_unpack_datagrams / qfec_unpack_frames / qfec_gather_rows are called through lib() on
guarded, sentinel-filled buffers; every group, every data row byte and every verdict is compared."""
import numpy as np
import pytest

import quicknet_amd as qa
import rx_common as rc
from dispatch_common import Guarded, check_all
from quicknet_amd._lib import lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)


def i32(a):
    return np.array(a, np.int32).view(np.uint8)  # a copy: the cached batches are read-only


def ptr(buf):
    return buf.t.data_ptr()


def as_i32(buf):
    return buf.host().reshape(-1).view(np.int32)


def first_diff(names, got, want):
    """Which scenario the first differing group is, for the assertion message."""
    G = len(names)
    d = np.nonzero((got.reshape(G, -1) != want.reshape(G, -1)).any(axis=1))[0]
    return f"{len(d)} groups differ, first {d[0]} ({names[d[0]]})" if len(d) else ""


def outputs(G, n, k, P, shards_off):
    return {"shards": rc.guarded64(rc.sentinel(G, n, P), shards_off), "marks": Guarded(rc.sentinel(G * n)),
            "rx_size": Guarded(rc.sentinel(G * n * 4)), "status": Guarded(rc.sentinel(G * k * 4)),
            "psize": Guarded(rc.sentinel(G * k * 4))}


def check_rx(o, mod, names, k, what):
    """Guards intact, every verdict written, every output equal to the model's."""
    check_all(o, what)
    G, n = mod.valid.shape
    status, psize, rx = (as_i32(o[x]) for x in ("status", "psize", "rx_size"))
    for name, a in (("status", status), ("psize", psize), ("rx_size", rx)):
        assert (a != rc.SENTINEL32).all(), f"{what}: {name} entries left unwritten"
    marks = o["marks"].host().reshape(-1)
    assert np.array_equal(marks, rc.marks_layout(mod.valid, k)), f"{what}: marks"
    assert np.array_equal(rx, mod.rx_size.reshape(-1)), f"{what}: rx_size, {first_diff(names, rx, mod.rx_size)}"
    assert np.array_equal(status, mod.status.reshape(-1)), f"{what}: status, {first_diff(names, status, mod.status)}"
    assert np.array_equal(psize, mod.psize.reshape(-1)), f"{what}: psize, {first_diff(names, psize, mod.psize)}"
    data = o["shards"].host()[:, :k]
    assert np.array_equal(data, mod.data), f"{what}: data rows, {first_diff(names, data, mod.data)}"


def unpack_datagrams(code, b, mod, k, m, P, checksum, wire_off, shards_off, what):
    G, n, wp = b.wire.shape
    ins = {"wire": rc.guarded64(b.wire, wire_off), "wire_len": Guarded(i32(b.wire_len))}
    o = outputs(G, n, k, P, shards_off)
    rcode = lib().qfec_unpack_datagrams(code._h, ptr(ins["wire"]), wp, ptr(ins["wire_len"]), G, checksum,
                                        b.dec_pkt_size, ptr(o["shards"]), P, ptr(o["marks"]),
                                        ptr(o["rx_size"]), ptr(o["status"]), ptr(o["psize"]), None)
    assert rcode == 0, lib().qfec_last_error().decode()
    torch.cuda.synchronize()
    check_all(ins, what)
    assert np.array_equal(ins["wire"].host(), b.wire), f"{what}: the input was written"
    check_rx(o, mod, b.names, k, what)


DCASES = [(f, k, m, p, c) for k, m in rc.FUSED_SHAPES + rc.STAGED_SHAPES for f in rc.forms_for(k, m)
          for p in rc.pitches_for(k, m) for c in (1, 0)]


@pytest.mark.parametrize("form,k,m,pitch,checksum", DCASES, ids=[f"{f}-{k}-{m}-{p}-c{c}" for f, k, m, p, c in DCASES])
def test_unpack_datagrams_vs_model(oracle, form, k, m, pitch, checksum):
    """The main scenario batch with d_wire and d_shards at a 64-B boundary and 16 B past one, and the
    dec_src batch (dec_pkt_size 600) with the two bases apart, under one wire_rx setting."""
    seed = rc.seed_for(k, m, pitch, checksum)
    main = rc.batch_model(oracle, k, m, pitch, checksum, seed, "main")
    dec = rc.batch_model(oracle, k, m, pitch, checksum, seed, "dec")
    code = qa.Code.vandermonde(k, m)
    saved = qa.tune_get("wire_rx")
    qa.tune("wire_rx", form)
    try:
        unpack_datagrams(code, *main, k, m, pitch, checksum, 0, 0, "main at +0")
        unpack_datagrams(code, *main, k, m, pitch, checksum, 16, 16, "main at +16")
        unpack_datagrams(code, *dec, k, m, pitch, checksum, 16, 0, "dec_src batch")
    finally:
        qa.tune("wire_rx", saved)


FCASES = [(f, k, m, p, c, s) for k, m in rc.FRAME_SHAPES for f in (0, 1, 3, 4) if f in rc.forms_for(k, m)
          for p in rc.pitches_for(k, m) for c in (1, 0) for s in (0, 1)]


@pytest.mark.parametrize("form,k,m,pitch,checksum,session", FCASES,
                         ids=[f"{f}-{k}-{m}-{p}-c{c}-s{s}" for f, k, m, p, c, s in FCASES])
def test_unpack_frames_vs_model(oracle, form, k, m, pitch, checksum, session):
    """The same scenarios framed row by row, plus frame-level damage (checksum, cmd, both, short, too
    long, and two successive first-k candidates with a bad frame checksum), one pass and two calls."""
    fb, mod = rc.frames_batch_model(oracle, k, m, pitch, checksum, bool(session), rc.seed_for(k, m, pitch, checksum))
    G, n, fpitch = fb.frames.shape
    code = qa.Code.vandermonde(k, m)
    saved = qa.tune_get("wire_rx")
    qa.tune("wire_rx", form)
    try:
        for off in (0, 16):
            what = f"frames at +{off}"
            ins = {"frames": rc.guarded64(fb.frames, off), "frame_len": Guarded(i32(fb.frame_len))}
            o = outputs(G, n, k, pitch, off)
            fo = {"frame_status": Guarded(rc.sentinel(G * n * 4)), "conv_hid": Guarded(rc.sentinel(G * n * 8))}
            rcode = lib().qfec_unpack_frames(code._h, ptr(ins["frames"]), fpitch, ptr(ins["frame_len"]), G,
                                             rc.GMASK, session, checksum, rc.BIG_DEC, ptr(o["shards"]), pitch,
                                             ptr(o["marks"]), ptr(o["rx_size"]), ptr(o["status"]),
                                             ptr(o["psize"]), ptr(fo["frame_status"]),
                                             ptr(fo["conv_hid"]), None)
            assert rcode == 0, lib().qfec_last_error().decode()
            torch.cuda.synchronize()
            check_all(ins, what)
            check_all(fo, what)
            assert np.array_equal(ins["frames"].host(), fb.frames), f"{what}: the input was written"
            fst = as_i32(fo["frame_status"]).reshape(G, n)
            assert (fst != rc.SENTINEL32).all(), f"{what}: frame_status entries left unwritten"
            names = fb.batch.names
            assert np.array_equal(fst, mod.frame_status), f"{what}: frame_status, {first_diff(names, fst, mod.frame_status)}"
            ch = fo["conv_hid"].host().reshape(-1).view(np.uint32).reshape(G, n, 2)
            if session:
                ok = mod.frame_status == 0
                assert np.array_equal(ch[ok], mod.conv_hid[ok]), f"{what}: conv_hid"
            else:  # no Session prefix: the buffer is not the call's to write
                assert (fo["conv_hid"].host() == rc.SENTINEL).all(), f"{what}: conv_hid written without a session"
            check_rx(o, mod.rx, fb.batch.names, k, what)
    finally:
        qa.tune("wire_rx", saved)


# ------------------------------------------------------------------ qfec_gather_rows

GATHER_PITCH = 64
GATHER_ROWS = 96  # 16 groups of 6; the first 80 rows pair every length with every source residue mod 16


def gather_case():
    """Rows at scattered source offsets of every residue mod 16, lengths 0, -3, 1, 5, 15, 16, 17,
    pitch - 11 (the longest a wrapped row holds), pitch - 10, pitch; 16 readable bytes past the last."""
    p = GATHER_PITCH
    lens = np.array([[0, -3, 1, 5, 15, 16, 17, p - 11, p - 10, p][r % 10] for r in range(GATHER_ROWS)], np.int32)
    off = np.array([r * (p + 48) + 16 * (r % 3) + r % 16 for r in range(GATHER_ROWS)], np.uint64)
    rng = np.random.default_rng(64)
    src = rng.integers(0, 256, size=int(off[-1]) + p + 16, dtype=np.uint8)
    for r in range(GATHER_ROWS):  # as shards without checksums: a size field the row holds
        if lens[r] >= 2:
            src[int(off[r])], src[int(off[r]) + 1] = (lens[r] - 2) & 0xFF, 0
    return src, off, lens


def gather_expected(src, off, lens, wrap_n, wrap_k):
    p = GATHER_PITCH
    H = 11 if wrap_n else 0
    out = rc.sentinel(GATHER_ROWS, p)
    out_len = np.zeros(GATHER_ROWS, np.int32)
    for r in range(GATHER_ROWS):
        n = int(lens[r])
        if n <= 0:
            continue  # out_len 0, the row untouched
        if H + n > p:
            # the kernel leaves before its first store: a row that does not fit keeps the caller's
            # bytes (here the sentinel), only its out_len says -1
            out_len[r] = -1
            continue
        row = np.zeros(p, np.uint8)
        if H:  # [0xEC][sent 0][src 0][n | k << 4 | ik << 8]
            row[0] = 0xEC
            ikn = wrap_n | wrap_k << 4 | (r % wrap_n) << 8
            row[9], row[10] = ikn & 0xFF, ikn >> 8
        row[H:H + n] = src[int(off[r]):int(off[r]) + n]
        out[r] = row
        out_len[r] = H + n
    return out, out_len


@pytest.mark.parametrize("wrap_n,wrap_k", [(0, 0), (6, 4), (15, 14)], ids=["plain", "wrap-6-4", "wrap-15-14"])
def test_gather_rows(oracle, wrap_n, wrap_k):
    src, off, lens = gather_case()
    want, want_len = gather_expected(src, off, lens, wrap_n, wrap_k)
    ins = {"src": Guarded(src, off=5), "off": Guarded(off.view(np.uint8)), "len": Guarded(i32(lens))}
    o = {"out": Guarded(rc.sentinel(GATHER_ROWS, GATHER_PITCH)), "out_len": Guarded(rc.sentinel(GATHER_ROWS * 4))}
    rcode = lib().qfec_gather_rows(ptr(ins["src"]), ptr(ins["off"]), ptr(ins["len"]), GATHER_ROWS,
                                   wrap_n, wrap_k, ptr(o["out"]), GATHER_PITCH, ptr(o["out_len"]), None)
    assert rcode == 0, lib().qfec_last_error().decode()
    torch.cuda.synchronize()
    check_all(ins, "gather inputs")
    check_all(o, "gather outputs")
    got_len = as_i32(o["out_len"])
    assert (got_len != rc.SENTINEL32).all()
    assert np.array_equal(got_len, want_len)
    assert {0, -1} <= set(want_len.tolist()) if wrap_n else -1 not in want_len
    got = o["out"].host()
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), f"rows {bad[:8]} (len {lens[bad[:8]]}, source residue {off[bad[:8]] % 16 + 5})"
    if (wrap_n, wrap_k) != (6, 4):
        return
    # the wrapped rows are 0xEC datagrams of groups of 6: straight into the receive, against the model
    k, m, P = 4, 2, 48
    assert rc.min_wire_pitch(P) == GATHER_PITCH
    G = GATHER_ROWS // 6
    wire, wlen = got.reshape(G, 6, GATHER_PITCH), got_len.reshape(G, 6)
    mod = rc.rx_model(oracle, rc.full_matrix(oracle, k, m), k, m, wire, wlen, 0, rc.BIG_DEC, P)
    assert mod.valid.any() and not mod.valid.all() and {2, -1, -2} <= set(mod.status.reshape(-1).tolist())
    b = rc.Batch(wire, wlen, tuple(f"gathered-{g}" for g in range(G)), None, GATHER_PITCH, rc.BIG_DEC, {})
    unpack_datagrams(qa.Code.vandermonde(k, m), b, mod, k, m, P, 0, 16, 16, "gathered rows")
