"""GPU: every send path -- the one-wave forms of k_pack_wave64 (1088 B, 576 B two groups per wave,
8-B lanes in three passes, 16-B lanes in two), k_pack_body with k_pack_line0 or k_pack_head, the
body alone without checksums, the staged build -> encode -> emit and the two-call frame fallback,
for every compiled (k, m) -- held byte for byte to the CPU model of tests/tx_common.py on batches in
which every group is a named scenario: sizes at every edge of a row, all-0xFF payloads at full size,
aliased payloads, sequence numbers that wrap, sizes of -1, INT_MIN, M + 1 and INT_MAX (void groups).
qfec_pack_datagrams / qfec_pack_frames are called through lib() on guarded, sentinel-filled buffers
at several base offsets; every length and every row byte of every group is compared, every input
must come back unwritten."""
import numpy as np
import pytest

import quicknet_amd as qa
import rx_common as rc
import tx_common as tc
from dispatch_common import Guarded, check_all
from quicknet_amd._lib import lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

QFEC_EINVAL, QFEC_EUNSUP = -1, -5


def ptr(buf):
    return buf.t.data_ptr()


def u8(a):
    return np.array(a).view(np.uint8).reshape(-1)  # a copy: the cached batches are read-only


def inputs(b, prefix, payload_off, mask_off):
    """Guarded copies of the call's inputs: d_payload (its 16 readable bytes past the last payload
    included) `payload_off` bytes and d_mask `mask_off` bytes past a 16-B boundary, the typed arrays
    on one."""
    ins = {"payload": Guarded(u8(b.payload), off=payload_off), "offsets": Guarded(u8(b.offs)), "sizes": Guarded(u8(b.sizes)),
           "seq": Guarded(u8(b.seq))}
    if prefix:
        ins["mask"] = Guarded(u8(b.masks), off=mask_off)
    if prefix == 12:
        ins["conv_hid"] = Guarded(u8(b.conv_hid))
    return ins


def inputs_unwritten(ins, b, prefix, what):
    check_all(ins, what)
    want = {"payload": b.payload, "offsets": u8(b.offs), "sizes": u8(b.sizes), "seq": u8(b.seq),
            "mask": b.masks.reshape(-1), "conv_hid": u8(b.conv_hid)}
    for name, buf in ins.items():
        assert np.array_equal(buf.host().reshape(-1), want[name]), f"{what}: input {name} was written"


def send(code, c, b, wire_off, shards_off, payload_off, mask_off, cmd=tc.CMD, protocol=tc.PROTOCOL):
    """One call on fresh buffers -> (return code, inputs, outputs); nothing is checked here."""
    G, n = len(b.names), c.k + c.m
    ins = inputs(b, c.prefix, payload_off, mask_off)
    o = {"rows": rc.guarded64(tc.sentinel(G, n, c.row_pitch), wire_off), "len": Guarded(tc.sentinel(G * n * 4)),
         "shards": rc.guarded64(tc.sentinel(G, n, c.shard_pitch), shards_off)}
    if c.prefix:
        rcode = lib().qfec_pack_frames(code._h, ptr(ins["payload"]), ptr(ins["offsets"]), ptr(ins["sizes"]), ptr(ins["seq"]),
                                       G, c.checksum, ptr(o["shards"]), c.shard_pitch, ptr(ins["mask"]),
                                       ptr(ins["conv_hid"]) if c.prefix == 12 else None, tc.GMASK, cmd, protocol,
                                       ptr(o["rows"]), c.row_pitch, ptr(o["len"]), None)
    else:
        rcode = lib().qfec_pack_datagrams(code._h, ptr(ins["payload"]), ptr(ins["offsets"]), ptr(ins["sizes"]),
                                          ptr(ins["seq"]), G, c.checksum, ptr(o["shards"]), c.shard_pitch, ptr(o["rows"]),
                                          c.row_pitch, ptr(o["len"]), None)
    torch.cuda.synchronize()
    return rcode, ins, o


def send_and_check(oracle, code, c, b, mod, wire_off, shards_off, payload_off, mask_off, unframe=False, **kw):
    what = f"{tc.case_id(c)} rows +{wire_off} shards +{shards_off} payload +{payload_off} mask +{mask_off}"
    rcode, ins, o = send(code, c, b, wire_off, shards_off, payload_off, mask_off, **kw)
    assert rcode == 0, f"{what}: {lib().qfec_last_error().decode()}"
    check_all(o, what)
    inputs_unwritten(ins, b, c.prefix, what)
    G, n = mod.lens.shape
    got = o["rows"].host()
    got_len = o["len"].host().reshape(-1).view(np.int32).reshape(G, n)
    tc.check_output(b.names, mod, got, got_len, tc.tail_rule(c), what)
    if unframe:  # the frames as a receiver sees them
        for g in np.nonzero(~mod.void)[0]:
            for j in range(n):
                st, work, _ = oracle.unframe_udp(got[g, j, :got_len[g, j]], gmask=tc.GMASK, session=c.prefix == 12)
                assert st == 0, f"{what}: unframe_udp says {st} for group {g} ({b.names[g]}) row {j}"


class fused_setting:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.saved = qa.tune_get("wire_fused")
        qa.tune("wire_fused", self.v)

    def __exit__(self, *exc):
        qa.tune("wire_fused", self.saved)


@pytest.mark.parametrize("c", tc.datagram_cases(), ids=tc.case_id)
def test_pack_datagrams_vs_model(oracle, c):
    """d_wire at +0, +16 and +48 from a 64-B boundary, d_shards at +0 and +16, d_payload at +0 and +5."""
    b, mod = tc.batch_model(oracle, c.k, c.m, c.checksum, c.shard_pitch, c.row_pitch, 0)
    code = qa.Code.vandermonde(c.k, c.m)
    with fused_setting(c.fused):
        for wire_off, shards_off, payload_off in ((0, 0, 0), (16, 16, 5), (48, 0, 5)):
            send_and_check(oracle, code, c, b, mod, wire_off, shards_off, payload_off, 0)


@pytest.mark.parametrize("c", tc.frame_cases(), ids=tc.case_id)
def test_pack_frames_vs_model(oracle, c):
    """The same with d_mask at +0, +1, +2 and +3 from a 16-B boundary; the frames of the first call are
    also handed to oracle.unframe_udp row by row."""
    b, mod = tc.batch_model(oracle, c.k, c.m, c.checksum, c.shard_pitch, c.row_pitch, c.prefix)
    code = qa.Code.vandermonde(c.k, c.m)
    with fused_setting(c.fused):
        for x, (wire_off, shards_off, payload_off, mask_off) in enumerate(((0, 0, 0, 0), (16, 16, 5, 1), (48, 0, 5, 2),
                                                                           (0, 16, 0, 3))):
            send_and_check(oracle, code, c, b, mod, wire_off, shards_off, payload_off, mask_off, unframe=x == 0)


CMD_CASES = [c for c in tc.frame_cases() if (c.k, c.m) == (5, 3) and c.prefix == 12 and c.checksum and c.fused and
             c.row_pitch in (1088, 576, 1152, 2112, 1072)]


@pytest.mark.parametrize("c", CMD_CASES, ids=tc.case_id)
def test_pack_frames_cmd_and_protocol(oracle, c):
    """cmd = 0xFF (only its low five bits travel, under 0xA0) and protocol = 0x00, on every frame form."""
    assert {x.form for x in CMD_CASES} == {"wave1", "wave2", "wave8x3", "wave16x2", "two-call"}
    b, mod = tc.batch_model(oracle, c.k, c.m, c.checksum, c.shard_pitch, c.row_pitch, c.prefix, None, 0xFF, 0x00)
    send_and_check(oracle, qa.Code.vandermonde(c.k, c.m), c, b, mod, 16, 0, 5, 3, unframe=True, cmd=0xFF, protocol=0x00)


@pytest.mark.parametrize("c", tc.single_group_cases(), ids=tc.case_id)
def test_single_group(oracle, c):
    """G = 1, every row at its largest: a launch of one group, one part-filled block or wave."""
    b, mod = tc.batch_model(oracle, c.k, c.m, c.checksum, c.shard_pitch, c.row_pitch, c.prefix, "max")
    assert len(b.names) == 1 and not mod.void.any()
    with fused_setting(c.fused):
        send_and_check(oracle, qa.Code.vandermonde(c.k, c.m), c, b, mod, 48, 16, 5, 3, unframe=bool(c.prefix))


# ------------------------------------------------------------------ argument checks

ARG_CASES = [
    # name, frames?, (k, m), checksum, shard pitch, row pitch, rows base offset, the documented code
    ("wire-base-8", 0, (4, 2), 1, 48, 64, 8, QFEC_EINVAL),
    ("frames-base-8", 12, (4, 2), 1, 48, 80, 8, QFEC_EINVAL),
    ("shard-pitch-24", 0, (4, 2), 1, 24, 64, 0, QFEC_EINVAL),
    ("frames-shard-pitch-24", 4, (4, 2), 1, 24, 64, 0, QFEC_EINVAL),
    ("wire-pitch-below-round16", 0, (4, 2), 1, 48, 48, 0, QFEC_EINVAL),   # round16(48 + 13) = 64
    ("frame-pitch-below-prefix", 12, (4, 2), 1, 48, 64, 0, QFEC_EINVAL),  # 48 + 13 + 12 = 73
    ("frame-pitch-below-prefix-4", 4, (4, 2), 1, 64, 80, 0, QFEC_EINVAL),  # 64 + 13 + 4 = 81
    ("n-16", 0, (12, 4), 1, 48, 64, 0, QFEC_EUNSUP),
    ("frames-n-16", 4, (12, 4), 1, 48, 80, 0, QFEC_EUNSUP),
    ("checksum-2", 0, (4, 2), 2, 48, 64, 0, QFEC_EINVAL),
    ("frames-checksum-2", 12, (4, 2), 2, 48, 80, 0, QFEC_EINVAL),
]


@pytest.mark.parametrize("name,prefix,km,checksum,sp,rp,base,want", ARG_CASES, ids=[a[0] for a in ARG_CASES])
def test_argument_checks(name, prefix, km, checksum, sp, rp, base, want):
    """wire_check / frame_check: the documented code, and not one output byte touched."""
    k, m = km
    n = k + m
    G = 3
    code = qa.Code.vandermonde(k, m)
    payload = Guarded(np.arange(G * k * 64 + 16, dtype=np.int64).astype(np.uint8))
    offs = Guarded(u8(np.arange(G * k, dtype=np.int64) * 64))
    sizes = Guarded(u8(np.full(G * k, 9, np.int32)))
    seq = Guarded(u8(np.arange(2 * G, dtype=np.uint32)))
    mask = Guarded(np.zeros(G * n, np.uint8))
    ch = Guarded(u8(np.zeros(2 * G * n, np.uint32)))
    o = {"rows": Guarded(tc.sentinel(G * n * (rp + 16)), off=base), "len": Guarded(tc.sentinel(G * n * 4)),
         "shards": Guarded(tc.sentinel(G * n * (sp + 16)))}
    if prefix:
        rcode = lib().qfec_pack_frames(code._h, ptr(payload), ptr(offs), ptr(sizes), ptr(seq), G, checksum, ptr(o["shards"]),
                                       sp, ptr(mask), ptr(ch) if prefix == 12 else None, tc.GMASK, tc.CMD, tc.PROTOCOL,
                                       ptr(o["rows"]), rp, ptr(o["len"]), None)
    else:
        rcode = lib().qfec_pack_datagrams(code._h, ptr(payload), ptr(offs), ptr(sizes), ptr(seq), G, checksum,
                                          ptr(o["shards"]), sp, ptr(o["rows"]), rp, ptr(o["len"]), None)
    torch.cuda.synchronize()
    assert rcode == want, lib().qfec_last_error().decode()
    check_all(o, name)
    for what, buf in o.items():
        assert (buf.host() == tc.SENTINEL).all(), f"{name}: {what} written by a rejected call"
