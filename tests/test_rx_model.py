"""CPU: the receive model of tests/rx_common.py held to the reference's own outputs, and the
coverage the scenario builder owes the GPU test (tests/test_gpu_rx_model.py).

* the per-datagram half of the model (valid, rx_size, shard rows, dec_src verdicts) against the
  vectors network/FecCodecBuf.cpp itself produced (tests/golden/wire_c{0,1}.npz);
* the survivor rule (first k valid datagrams in group order) against fec_decode_pkts of the compiled
  reference, where oracle/_ref was built;
* every (shape, pitch, checksum) the GPU test uses yields every scenario it promises, twice, at
  group indices of different parity, and the model's outputs reach every verdict and retry depth."""
import ctypes as C
import os

import numpy as np
import pytest

import rx_common as rc
from conftest import ROOT

WIRE = [(4, 5), (4, 6), (3, 5), (5, 8), (7, 8), (10, 13), (2, 4), (3, 4), (14, 15), (1, 2)]  # the golden (k, n)
REF = os.path.join(ROOT, "oracle", "_ref", "libref_feccodec_ref.so")


def golden_batch(z, k, n, checksum, var):
    key = f"{k}_{n}_{checksum}"
    dg, dl = z[f"dgrams_{key}"], z[f"dlen_{key}"].astype(np.int32)
    w = np.zeros(dg.shape[:2] + (2080,), np.uint8)
    w[..., :dg.shape[2]] = dg
    if var == 1:  # the corrupted copy the generator parsed: byte 14 flipped
        for g in range(w.shape[0]):
            for j in range(n):
                if dl[g, j] > 14:
                    w[g, j, 14] ^= 0x40
    return w, dl


@pytest.mark.parametrize("k,n", WIRE)
@pytest.mark.parametrize("checksum", [1, 0])
def test_model_vs_golden(oracle, golden, k, n, checksum):
    z = golden(f"wire_c{checksum}.npz")
    key = f"{k}_{n}_{checksum}"
    parsed, shards_ref, srcinfo = z[f"parsed_{key}"], z[f"shards_{key}"], z[f"srcinfo_{key}"]
    full = rc.full_matrix(oracle, k, n - k)
    for var in range(2):
        w, dl = golden_batch(z, k, n, checksum, var)
        mod = rc.rx_model(oracle, full, k, n - k, w, dl, checksum, rc.BIG_DEC, 2064)
        assert np.array_equal(mod.valid, parsed[:, :, var, 0] != 0)
        assert np.array_equal(mod.rx_size[mod.valid], parsed[:, :, var, 6][mod.valid])
        assert (mod.rx_size[~mod.valid] == -1).all()
        if var == 0:
            assert mod.valid.all() and not mod.rounds.any()
            for g in range(w.shape[0]):
                for j in range(n):
                    _, _, body = rc.parse_row(oracle, w[g, j], int(dl[g, j]), j, k, n, 2080, 2064)
                    assert np.array_equal(body, shards_ref[g, j, :len(body)]) and not shards_ref[g, j, len(body):].any()
            assert np.array_equal(mod.data, shards_ref[:, :k, :2064])
            assert np.array_equal(mod.status, srcinfo[:, :, 0])
            assert np.array_equal(mod.psize, srcinfo[:, :, 1])


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref caller builds absent (built only beside the reference tree)")
@pytest.mark.parametrize("k,n", WIRE)
@pytest.mark.parametrize("checksum", [1, 0])
def test_survivor_rule_vs_compiled_reference(oracle, golden, k, n, checksum):
    """One lossy group per golden shape: data row 0 lost and, without checksums, a used survivor and
    the last check row silently wrong.  The model's decoded row equals fec_decode_pkts fed the first k
    valid datagrams in group order (zfec_unpack_input, NetFecCodec.cpp:504-528) -- garbage included."""
    from oracle.oracle import FecCodecBufS, FecCodecHead, load_callers

    z = golden(f"wire_c{checksum}.npz")
    w, dl = golden_batch(z, k, n, checksum, 0)
    w, dl = w[:1].copy(), dl[:1].copy()
    dl[0, 0] = 0
    if not checksum:
        if k >= 2:
            w[0, 1, dl[0, 1] - 1] ^= 0x5A
        if n - k >= 2:
            w[0, n - 1, 12] ^= 0x21
    mod = rc.rx_model(oracle, rc.full_matrix(oracle, k, n - k), k, n - k, w, dl, checksum, rc.BIG_DEC, 2064)
    assert mod.valid[0].sum() == n - 1
    L = load_callers(REF)
    L.fec_new.restype = C.c_void_p
    L.fec_new.argtypes = [C.c_int, C.c_int]
    L.fec_free.argtypes = [C.c_void_p]
    R = FecCodecBufS()
    L.init_fec_buf(C.byref(R), 2048, 16)
    codec = L.fec_new(k, n)
    L.reset_fec_dec_buf(C.byref(R))
    v = max_size = 0
    keep = []
    for j in range(n):
        if dl[0, j] <= 0 or v == k:
            continue
        h, un = FecCodecHead(), C.c_int()
        buf = w[0, j, :dl[0, j]].copy()
        keep.append(buf)
        q = L.unpack_fec_head(C.byref(R), C.byref(h), buf.ctypes.data, len(buf), C.byref(un))
        assert q and h.ik == j
        shard = np.frombuffer(C.string_at(q, un.value), np.uint8).copy()
        keep.append(shard)
        assert L.set_fec_dec_buf(C.byref(R), v, shard.ctypes.data, len(shard), j)
        max_size = max(max_size, len(shard))
        v += 1
    assert v == k and L.fec_decode_pkts(C.byref(R), codec, max_size) == 0
    got = np.frombuffer(C.string_at(L.get_fec_decoded_pkt(C.byref(R), 0), max_size), np.uint8)
    L.fec_free(codec)
    L.release_fec_buf(C.byref(R))
    assert np.array_equal(mod.data[0, 0, :max_size], got)
    assert not mod.data[0, 0, max_size:].any()


# ------------------------------------------------------------------ coverage the GPU test relies on

REJECTS = ["tag-00", "tag-EE", "n-field", "k-field", "ik-swap", "len-neg", "len-1", "len-10", "ED-len-11", "ED-len-12",
           "len-eq-hdr", "len-over-pitch", "shard-over-pitch"]


def expected_names(k, m, checksum, kind):
    """The scenario list as the test plan states it, written out here and not taken from the builder."""
    if kind == "dec":
        return ([f"size-{s}-{h}" for s in (598, 599, 600, 601) for h in ("rx", "dec")] +
                [f"inner-sum-{h}" for h in ("rx", "dec")] + [f"size-field-over-pitch-{h}" for h in ("rx", "dec")])
    retry = "retry" if checksum else "silent-corrupt"
    out = ["clean", f"lost-{m + 1}", f"{retry}-unrecoverable", "bad-extra-only" if checksum else "silent-corrupt-extra",
           "tag-mix-survivor", "tag-mix-extra", "size-field-over-pitch-rx", "size-field-over-pitch-dec"]
    out += [f"lost-{t}-{w}" for t in range(1, m + 1) for w in ("data", "parity", "mixed")]
    out += [f"{retry}-{r}" for r in range(1, m + 1)]
    out += [f"reject-{r}" for r in REJECTS]
    out += [f"trailing-{h}-{e}" for h in ("rx", "dec") for e in (1, 7, 40)]
    return out


CASES = [(k, m, p, c) for k, m in rc.FUSED_SHAPES + rc.STAGED_SHAPES for p in rc.pitches_for(k, m) for c in (1, 0)]


@pytest.mark.parametrize("k,m,pitch,checksum", CASES, ids=[f"{k}-{m}-{p}-c{c}" for k, m, p, c in CASES])
def test_scenarios_cover(oracle, k, m, pitch, checksum):
    head = 4 if checksum else 2
    seed = rc.seed_for(k, m, pitch, checksum)
    for kind in ("main", "dec"):
        b, mod = rc.batch_model(oracle, k, m, pitch, checksum, seed, kind)
        names, skipped = rc.promised(k, m, pitch, checksum, kind)
        G = len(b.names)
        assert G <= 100
        for want in expected_names(k, m, checksum, kind):
            assert want in names or skipped.get(want), f"{kind}: {want} neither built nor excused"
        for name in names:  # each promised scenario: twice, at group indices of different parity
            at = [g for g in range(G) if b.names[g] == name]
            assert len(at) == 2 and (at[0] + at[1]) % 2 == 1, (kind, name, at)
        assert b.wire_pitch == rc.min_wire_pitch(pitch) + (32 if kind == "main" else 0)
        lens = b.wire_len[b.names.index("clean")]
        assert len(set(lens[:k].tolist())) > 1  # datagram lengths differ inside a group
        if kind == "main":
            want_rounds = {1, min(m, 2), min(m, 3)} if checksum else {0}
            assert want_rounds <= set(mod.rounds.tolist()), (want_rounds, set(mod.rounds.tolist()))
            assert {head, -1, -2} <= set(mod.status.reshape(-1).tolist())
            assert (mod.valid & (mod.rx_size == 0)).any()
            # the retry scenarios end where the plan says: k valid rows or more, or k - 1
            for g, name in enumerate(b.names):
                if name.startswith("retry-") and name != "retry-unrecoverable":
                    assert mod.valid[g].sum() >= k and mod.rounds[g] >= 1, name
                if name == "retry-unrecoverable":
                    assert mod.valid[g].sum() == k - 1
                if name == "bad-extra-only":
                    assert mod.rounds[g] == 0 and mod.valid[g].sum() == k + m - 1
                if name.startswith("reject-") and name not in ("reject-len-eq-hdr",):
                    assert not mod.valid[g].all(), name
                if name.startswith("trailing-rx"):
                    j = 1 % k
                    assert mod.valid[g].all() and mod.rx_size[g, j] > head + mod.psize[g, j] and mod.status[g, j] == head
                if name.startswith("trailing-dec"):
                    j = 1 % k
                    assert not mod.valid[g, j] and mod.status[g, j] == head
                    assert mod.data[g, j, head + mod.psize[g, j]] != 0  # the decoded row carries the trailing bytes
            if not checksum:  # silent corruption reaches the decoded rows
                differ = False
                for g, name in enumerate(b.names):
                    if name.startswith("silent-corrupt"):
                        for i in np.nonzero(~mod.valid[g, :k])[0]:
                            pl = b.payloads[g][i]
                            differ |= mod.psize[g, i] != len(pl)  # (a corrupted byte 0 lands in the size field)
                            differ |= not np.array_equal(mod.data[g, i, head:head + len(pl)], pl)
                assert differ
        else:
            for g, name in enumerate(b.names):
                j = 1 % k
                if name.startswith("size-"):
                    assert mod.valid[g, j] == name.endswith("-rx")
                if name.startswith(("size-598", "size-599")):
                    assert mod.status[g, j] == head and mod.psize[g, j] == int(name.split("-")[1])
                if name.startswith(("size-600", "size-601", "inner-sum", "size-field")):
                    assert mod.status[g, j] == -1, name
                if name.startswith("inner-sum"):  # the others decode from it or with it, and are good
                    assert (np.delete(mod.status[g], j) == head).all()


FCASES = [(k, m, p, c, s) for k, m in rc.FRAME_SHAPES for p in rc.pitches_for(k, m) for c in (1, 0) for s in (0, 1)]


@pytest.mark.parametrize("k,m,pitch,checksum,session", FCASES, ids=[f"{k}-{m}-{p}-c{c}-s{s}" for k, m, p, c, s in FCASES])
def test_frame_scenarios_cover(oracle, k, m, pitch, checksum, session):
    fb, mod = rc.frames_batch_model(oracle, k, m, pitch, checksum, bool(session), rc.seed_for(k, m, pitch, checksum))
    names = fb.batch.names
    assert len(names) <= 110
    for f in rc.FRAME_DAMAGE:
        assert names.count(f) == 2
    want = {"frame-sum": 2, "frame-cmd": 3, "frame-both": 2, "frame-short": 1, "frame-long": 4}
    for g, name in enumerate(names):
        if name in want:
            bad = np.nonzero(mod.frame_status[g])[0]
            assert len(bad) == 1 and mod.frame_status[g, bad[0]] == want[name], name
        if name == "frame-sum-chain":  # the frame checksum alone drives the retry loop past round 1
            assert mod.frame_status[g].tolist().count(2) == 2 and mod.rx.rounds[g] == 2
    assert {0, 1, 2, 3, 4} <= set(mod.frame_status.reshape(-1).tolist())
    if checksum:
        assert mod.rx.rounds.max() >= min(m, 3)
