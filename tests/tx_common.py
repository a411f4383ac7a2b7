"""Shared by test_tx_model.py (CPU) and test_gpu_tx_model.py (GPU): a CPU model of the whole
datagram / frame send (qfec_pack_datagrams, qfec_pack_frames) composed from the oracle's pack_group
(pinned to network/FecCodecBuf.cpp by tests/golden/wire_c*.npz) and frame_udp, a deterministic
builder of batches in which every group is one named scenario, send_form() -- which kernels a call
takes, restated from the rules of quicknet_amd/csrc/qfec_geom.hpp and held to them by
test_tx_model.py -- and the case table of the GPU test.

The rules are those of include/qfec.h; nothing here comes from device output.  torch is not needed."""
import collections
import functools

import numpy as np

SENTINEL = 0xA5                      # every output buffer is pre-filled with this byte
SENTINEL32 = int(np.frombuffer(bytes([SENTINEL] * 4), np.int32)[0])
GMASK = 0xA7
INT_MAX, INT_MIN = 2**31 - 1, -2**31
CMD, PROTOCOL = 0x11, 0xFF           # qfec_pack_frames' defaults in quicknet_amd/codec.py

# every QFEC_PACK_CASE / QFEC_PFC shape of quicknet_amd/csrc/qfec_wire.hip, and shapes without an instance
PACK_SHAPES = [(10, 3), (4, 1), (4, 2), (2, 2), (3, 1), (3, 2), (5, 1), (5, 3), (7, 1), (8, 4)]
STAGED_SHAPES = [(6, 2), (14, 1), (1, 14)]
THREE = [(10, 3), (5, 3), (2, 2)]    # the shapes that also run the rarer pitches

FORMS = ("wave1", "wave2", "wave8x3", "wave16x2", "body+line0", "body+head", "body11-line", "body11", "staged",
         "two-call")
# forms that store every 64-B line of a row whole: bytes past a datagram, up to the pitch, are zero
LINE_FORMS = ("wave1", "wave2", "wave8x3", "wave16x2", "body+line0", "body11-line")


def full_matrix(oracle, k, m):
    """The n x k fec.c matrix: identity on top of the Vandermonde parity rows."""
    return np.concatenate([np.eye(k, dtype=np.uint8), oracle.vandermonde(k, k + m)])


def line_above(nbytes):
    return (nbytes + 63) // 64 * 64


# ------------------------------------------------------------------ which kernels a call takes

def _wave(row_pitch):
    if 1088 < row_pitch <= 1600:
        return "wave8x3"
    return {576: "wave2", 1088: "wave1"}.get(row_pitch)


def send_form(k, m, checksum, shard_pitch, row_pitch, prefix, fused=1):
    """The form qfec_pack_datagrams (prefix 0) or qfec_pack_frames (prefix 4 / 12) takes.  One wave per
    group: wave1 (1088 B), wave2 (576 B, two groups per wave), wave8x3 (1104..1600 B, 8-B lanes, three
    passes), wave16x2 (frames only, 1664..2112 B, 16-B lanes, two passes); body + a second launch:
    body+line0, body+head; without checksums the body alone: body11-line, body11; staged: build ->
    encode -> emit; two-call: frames as qfec_pack_datagrams + qfec_frame_udp."""
    inst = (k, m) in PACK_SHAPES
    if prefix:
        if not (fused and inst and checksum) or row_pitch != line_above(prefix + 13 + shard_pitch):
            return "two-call"
        return _wave(row_pitch) or ("wave16x2" if 1088 < row_pitch <= 2112 else "two-call")
    if not (fused and inst):
        return "staged"
    hdr = 13 if checksum else 11
    line = row_pitch % 64 == 0 and row_pitch == line_above(hdr + shard_pitch) and row_pitch // 16 >= (20 if checksum else 16)
    if not checksum:
        return "body11-line" if line else "body11"
    if line and _wave(row_pitch):
        return _wave(row_pitch)
    return "body+line0" if line else "body+head"


Case = collections.namedtuple("Case", "form k m checksum shard_pitch row_pitch prefix fused")


def _case(k, m, c, sp, rp, fp, fused):
    return Case(send_form(k, m, c, sp, rp, fp, fused), k, m, c, sp, rp, fp, fused)


@functools.lru_cache(maxsize=None)
def datagram_cases():
    fused = [(k, m, 1, sp, rp) for k, m in PACK_SHAPES for sp, rp in ((1040, 1088), (528, 576), (16, 32), (304, 320))]
    fused += [(k, m, 0, sp, rp) for k, m in PACK_SHAPES for sp, rp in ((304, 320), (16, 32))]
    fused += [(k, m, 1, sp, rp) for k, m in THREE
              for sp, rp in ((1072, 1088), (1104, 1152), (1584, 1600), (1616, 1664), (240, 256), (1040, 1056), (528, 1088))]
    out = [_case(*c, 0, f) for f in (1, 0) for c in fused]
    # no instance: staged under either setting
    out += [_case(k, m, c, sp, rp, 0, f) for k, m in STAGED_SHAPES for c, sp, rp in ((1, 1040, 1088), (0, 304, 320))
            for f in (1, 0)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def frame_cases():
    out = []
    for fp in (4, 12):
        out += [_case(k, m, 1, rp - 48, rp, fp, 1) for k, m in PACK_SHAPES for rp in (1088, 576)]
        out += [_case(k, m, 1, rp - 48, rp, fp, 1) for k, m in THREE for rp in (1152, 1600, 1664, 2112)]
        out += [_case(k, m, 1, 1040, 1072, fp, 1) for k, m in THREE]   # a 16-B multiple, not the line above
        out += [_case(k, m, 0, 1040, 1088, fp, 1) for k, m in THREE]   # checksum off
        out += [_case(k, m, 1, 1040, 1088, fp, 0) for k, m in THREE]   # wire_fused 0
    return tuple(out)


def case_id(c):
    return f"{c.form}-{c.k}-{c.m}-c{c.checksum}-{c.shard_pitch}-{c.row_pitch}" + (f"-fp{c.prefix}" if c.prefix else "") + f"-f{c.fused}"


def single_group_cases():
    """One case per form for the G = 1 run of `max`."""
    seen = {}
    for c in datagram_cases() + frame_cases():
        seen.setdefault(c.form, c)
    return [seen[f] for f in FORMS]


def tail_rule(c):
    """Bytes [len, pitch) of a live row: frames promise zero on every path, datagrams where a line
    form runs; elsewhere every such byte is zero or was never written."""
    return "zero" if c.prefix or c.form in LINE_FORMS else "zero-or-sentinel"


# ------------------------------------------------------------------ scenarios

def max_size(shard_pitch, checksum):
    return shard_pitch - (4 if checksum else 2)


def _ends(k, m, checksum, shard_pitch, row_pitch, prefix):
    """Payload sizes that put a row's end at the edges the kernels care about -> {family: [sizes]}."""
    M = max_size(shard_pitch, checksum)
    over = prefix + (13 if checksum else 11) + (4 if checksum else 2)  # row length at size 0
    dg_over = over - prefix
    line0 = [L - o for L in (15, 16, 17, 63, 64, 65) for o in {over, dg_over}] + [46, 47, 48, 49]
    cuts = list(range(0, row_pitch, 512)) + ([256] if row_pitch == 576 else [])  # 576: the end of a 32-lane half's first row
    edges = [64 + c + d - over for c in cuts for d in (-1, 0, 1)]
    keep = lambda v: sorted({s for s in v if 0 <= s <= M})
    return {"line0": keep(line0), "pass-edges": keep(edges)}


def _families(k, m, checksum, shard_pitch, row_pitch, prefix):
    """[(name, k sizes)]: the edge sizes three to a group (two for k = 2, one for k = 1), the other rows
    repeating them, so the check rows' length (the group's largest shard) visits every edge too."""
    out = []
    per = min(k, 3)
    for fam, vals in _ends(k, m, checksum, shard_pitch, row_pitch, prefix).items():
        for x in range(0, len(vals), per):
            part = vals[x:x + per]
            out.append((f"{fam}-{x // per}", [part[i % len(part)] for i in range(k)]))
    return out


def _ordinary(k, M, g, rng):
    pool = [0, 1, M, max(M - 13, 0), min(37, M), min(200, M), int(rng.integers(0, M + 1)), int(rng.integers(0, M + 1))]
    return [pool[(g + i) % len(pool)] for i in range(k)]


def _scenarios(k, m, checksum, shard_pitch, row_pitch, prefix):
    """[(name, spec)] and {name: why this case cannot express it}.  spec: sizes(inst, g, rng) -> k sizes,
    and optionally fill (every payload byte of the group), offs ("equal" / "desc"), seq, mask, ch."""
    M = max_size(shard_pitch, checksum)
    S, skipped = [], {}

    def add(name, sizes, **kw):
        S.append((name, dict(sizes=sizes if callable(sizes) else (lambda inst, g, rng, v=list(sizes): list(v)), **kw)))

    def one_row(row, val):  # an ordinary group with one row's size replaced; row < 0 counts from the last
        def f(inst, g, rng):
            s = _ordinary(k, M, g, rng)
            s[row(inst) % k] = val
            return s
        return f

    add("zero", [0] * k)
    add("one", [min(1, M)] * k)
    add("max", [M] * k)
    add("max-1", [M - 1] * k)
    add("single-first", [M] + [0] * (k - 1))
    add("single-last", [0] * (k - 1) + [M])
    add("ff-max", [M] * k, fill=0xFF)
    add("zero-bytes-max", [M] * k, fill=0x00)
    for name, sizes in _families(k, m, checksum, shard_pitch, row_pitch, prefix):
        add(name, sizes)
    assert any(n.startswith("line0") for n, _ in S)
    if not any(n.startswith("pass-edges") for n, _ in S):
        assert row_pitch < 64
        skipped["pass-edges-0"] = "no row reaches byte 63"
    add("ramp", [i * M // k for i in range(k)])
    add("random", lambda inst, g, rng: [int(x) for x in rng.integers(0, M + 1, size=k)])
    add("alias", lambda inst, g, rng: [int(x) for x in rng.integers(M // 2, M + 1, size=k)], offs=("equal", "desc"))
    add("seq-wrap", lambda inst, g, rng: _ordinary(k, M, g, rng), seq=(0xFFFFFFFF - 2, 0xFFFFFFFE))
    add("seq-high", lambda inst, g, rng: _ordinary(k, M, g, rng), seq=(0x89ABCDEF, 0x7654321F))
    # void groups: one size outside [0, M]; instance 0 in row 0, instance 1 in the last row (over: always the last)
    first_last = lambda inst: 0 if inst == 0 else -1
    add("neg", one_row(lambda inst: 0, -1), void=True)
    add("int-min", one_row(first_last, INT_MIN), void=True)
    add("over", one_row(lambda inst: -1, M + 1), void=True)
    add("over-int-max", one_row(first_last, INT_MAX), void=True)
    add("over-int-max-3", one_row(first_last, INT_MAX - 3), void=True)
    # a void group between two live ones: in a wave of two (576 B) it shares the cross-lane sums with a
    # live group, as the first of the pair in one instance and as the second in the other
    live = [s for s in S if not s[1].get("void")]
    for x, v in enumerate(s for s in list(S) if s[1].get("void")):
        live.insert(3 * x + 2, v)
    S[:] = live
    if prefix:
        ordinary = lambda inst, g, rng: _ordinary(k, M, g, rng)
        add("mask-00", ordinary, mask=0x00)
        add("mask-ff", ordinary, mask=0xFF)
        add("mask-cancel", ordinary, mask=GMASK ^ 0x5A)  # mask ^ gmask ^ 0x5a == 0: the frame goes out in clear
        if prefix == 12:
            add("conv-0", ordinary, ch=0)
            add("conv-ff", ordinary, ch=0xFFFFFFFF)
        else:
            skipped["conv-0"] = skipped["conv-ff"] = "no Session prefix"
    return S, skipped


def promised(k, m, checksum, shard_pitch, row_pitch, prefix):
    """The scenario names batch() must yield for this case, and the reasons for those it skips."""
    S, skipped = _scenarios(k, m, checksum, shard_pitch, row_pitch, prefix)
    return [s[0] for s in S], skipped


Batch = collections.namedtuple("Batch", "names sizes offs seq payload masks conv_hid void")


@functools.lru_cache(maxsize=None)
def batch(k, m, checksum, shard_pitch, row_pitch, prefix, only=None):
    """A batch in which group g is the scenario names[g]: the scenarios in order, one ordinary group,
    the scenarios again (instance 1) -- so every scenario sits at two group indices of opposite
    parity and G is odd.  Every group owns a region of the payload buffer; offsets of void rows stay
    inside it with more than shard_pitch + 16 readable bytes behind them.  only: a batch of that one
    scenario (G = 1).  Deterministic; arrays are read-only."""
    n = k + m
    M = max_size(shard_pitch, checksum)
    S, _ = _scenarios(k, m, checksum, shard_pitch, row_pitch, prefix)
    if only is not None:
        order = [(s, 0) for s in S if s[0] == only]
        assert len(order) == 1
    else:
        if len(S) % 2:
            S = S + [("ordinary", dict(sizes=lambda inst, g, rng: _ordinary(k, M, g, rng)))]
        mid = ("ordinary", dict(sizes=lambda inst, g, rng: _ordinary(k, M, g, rng)))
        order = [(s, 0) for s in S] + [(mid, 0)] + [(s, 1) for s in S]
    G = len(order)
    rng = np.random.default_rng(k * 100003 + m * 10007 + checksum * 1009 + shard_pitch * 7 + row_pitch * 3 + prefix)
    region = (k * max(M, 1) + shard_pitch + 192) | 1   # odd: the groups' bases alternate in parity
    payload = rng.integers(0, 256, size=G * region + 16, dtype=np.uint8)
    sizes = np.zeros((G, k), np.int32)
    offs = np.zeros((G, k), np.int64)
    seq = rng.integers(0, 2**32, size=(G, 2), dtype=np.uint64).astype(np.uint32)
    masks = rng.integers(0, 256, size=(G, n), dtype=np.uint8)
    conv_hid = rng.integers(0, 2**32, size=(G, n, 2), dtype=np.uint64).astype(np.uint32)
    void = np.zeros(G, bool)
    names = []
    for g, ((name, spec), inst) in enumerate(order):
        base = g * region
        sz = [int(s) for s in spec["sizes"](inst, g, rng)]
        assert len(sz) == k
        sizes[g] = sz
        void[g] = bool(spec.get("void"))
        assert void[g] == any(s < 0 or s > M for s in sz), name
        how = spec.get("offs", ("packed", "packed"))[inst]
        if void[g]:
            offs[g] = base + 3 + 5 * np.arange(k)
            assert region - 3 - 5 * k >= shard_pitch + 128
        elif how == "equal":
            offs[g] = base | 1
        elif how == "desc":
            offs[g] = (base | 1) + 2 * (k - 1 - np.arange(k))
        else:
            offs[g] = base + np.concatenate([[0], np.cumsum(sz)[:-1]])
        if not void[g]:
            assert int((offs[g] + sizes[g]).max()) + 16 <= base + region
        if spec.get("fill") is not None:
            payload[base:base + region] = spec["fill"]
        if spec.get("seq") is not None:
            seq[g] = spec["seq"]
        if spec.get("mask") is not None:
            masks[g] = spec["mask"]
        if spec.get("ch") is not None:
            conv_hid[g] = spec["ch"]
        names.append(name)
    for a in (sizes, offs, seq, payload, masks, conv_hid, void):
        a.setflags(write=False)
    return Batch(tuple(names), sizes, offs, seq, payload, masks, conv_hid, void)


# ------------------------------------------------------------------ the model

Model = collections.namedtuple("Model", "lens rows void")


def tx_model(oracle, k, m, checksum, shard_pitch, row_pitch, prefix, sizes, offs, seq, payload, masks=None,
             conv_hid=None, cmd=CMD, protocol=PROTOCOL):
    """The send of a batch -> Model: lens [G, n] (-1 in every row of a void group: one with a size < 0 or
    > shard_pitch - head), rows [G, n, row_pitch] = the datagram (prefix 0: oracle.pack_group) or its
    frame (oracle.frame_udp over it; conv_hid only with prefix 12) in [0, len), zero past it."""
    G, n = len(sizes), k + m
    M = max_size(shard_pitch, checksum)
    full = full_matrix(oracle, k, m)
    lens = np.full((G, n), -1, np.int32)
    rows = np.zeros((G, n, row_pitch), np.uint8)
    void = ((sizes < 0) | (sizes > M)).any(axis=1)
    dpitch = shard_pitch + 16
    for g in np.nonzero(~void)[0]:
        dg, ln, _ = oracle.pack_group(k, n, full, payload, offs[g], sizes[g], int(seq[g, 0]), int(seq[g, 1]), checksum,
                                      shard_cap=max(2052, shard_pitch), pitch=dpitch)
        for j in range(n):
            row = dg[j, :ln[j]]
            if prefix:
                row = oracle.frame_udp(row, masks[g, j], gmask=GMASK, cmd=cmd, protocol=protocol,
                                       conv_hid=conv_hid[g, j] if prefix == 12 else None)
            assert len(row) <= row_pitch
            rows[g, j, :len(row)] = row
            lens[g, j] = len(row)
    return Model(lens, rows, void)


@functools.lru_cache(maxsize=None)
def batch_model(oracle, k, m, checksum, shard_pitch, row_pitch, prefix, only=None, cmd=CMD, protocol=PROTOCOL):
    b = batch(k, m, checksum, shard_pitch, row_pitch, prefix, only)
    mod = tx_model(oracle, k, m, checksum, shard_pitch, row_pitch, prefix, b.sizes, b.offs, b.seq, b.payload, b.masks,
                   b.conv_hid, cmd, protocol)
    assert np.array_equal(mod.void, b.void)
    for a in mod:
        a.setflags(write=False)
    return b, mod


# ------------------------------------------------------------------ holding an output to the model

def _first(names, bad):
    """Which scenario the first offending group is, for the assertion message."""
    d = np.nonzero(bad)[0]
    return f"{len(d)} groups, first {d[0]} ({names[d[0]]})"


def check_output(names, mod, got_rows, got_len, tail, what):
    """got_rows [G, n, pitch], got_len [G, n] of buffers pre-filled with SENTINEL against the model: no
    length left unwritten, every length and every byte of [0, len) equal, bytes of [len, pitch) zero
    (tail "zero") or each zero or SENTINEL ("zero-or-sentinel"), every row of a void group entirely
    SENTINEL or entirely zero."""
    G, n, pitch = got_rows.shape
    assert got_len.shape == (G, n) and mod.rows.shape == got_rows.shape
    unset = (got_len == SENTINEL32).any(axis=1)
    assert not unset.any(), f"{what}: length entries left unwritten, {_first(names, unset)}"
    bad = (got_len != mod.lens).any(axis=1)
    assert not bad.any(), f"{what}: lengths, {_first(names, bad)}: got {got_len[bad][0].tolist()} want {mod.lens[bad][0].tolist()}"
    live = ~mod.void
    inside = np.arange(pitch)[None, None, :] < mod.lens[:, :, None]   # all False in a void group
    bad = (np.where(inside, got_rows, 0) != mod.rows).any(axis=(1, 2))
    if bad.any():
        g = int(np.nonzero(bad)[0][0])
        j, at = np.argwhere(np.where(inside[g], got_rows[g], 0) != mod.rows[g])[0]
        raise AssertionError(f"{what}: row bytes, {_first(names, bad)}: row {j} byte {at} of {mod.lens[g, j]}: "
                             f"got {got_rows[g, j, at]:#04x} want {mod.rows[g, j, at]:#04x}")
    past = ~inside & live[:, None, None]
    if tail == "zero":
        bad = (past & (got_rows != 0)).any(axis=(1, 2))
    else:
        assert tail == "zero-or-sentinel"
        bad = (past & (got_rows != 0) & (got_rows != SENTINEL)).any(axis=(1, 2))
    assert not bad.any(), f"{what}: bytes past a row's end ({tail}), {_first(names, bad)}"
    vr = got_rows[mod.void].reshape(-1, pitch)
    ok = (vr == SENTINEL).all(axis=1) | (vr == 0).all(axis=1)
    bad = np.zeros(G, bool)
    bad[np.nonzero(mod.void)[0]] = ~ok.reshape(-1, n).all(axis=1)
    assert not bad.any(), f"{what}: a void group's row neither untouched nor all zero, {_first(names, bad)}"


def sentinel(*shape):
    return np.full(shape, SENTINEL, np.uint8)
