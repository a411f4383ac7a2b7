"""Shared by test_rx_model.py (CPU) and test_gpu_rx_model.py (GPU): a CPU model of the whole
datagram / frame receive (qfec_unpack_datagrams, qfec_unpack_frames) composed from the oracle's
per-datagram restatements of the reference (unpack_head, dec_src, fec_reconstruct, unframe_udp),
and a deterministic builder of hostile batches in which every group is one named scenario.

The rules are those of include/qfec.h and of network/FecCodecBuf.cpp:109-133, 334-411 and
network/NetFecCodec.cpp:200-213, 504-528; nothing here comes from device output.  torch is imported
inside the helpers that need it, so the CPU suite can import this module."""
import collections
import functools

import numpy as np

SENTINEL = 0xA5                      # every output buffer is pre-filled with this byte
SENTINEL32 = int(np.frombuffer(bytes([SENTINEL] * 4), np.int32)[0])
GMASK = 0xA7
BIG_DEC = 2068                       # the library's default dec_pkt_size
SMALL_DEC = 600                      # the dec_src batches' dec_pkt_size

# every QFEC_RX_CASE shape of quicknet_amd/csrc/qfec_rx.hip, and two shapes without an instance
FUSED_SHAPES = [(10, 3), (4, 1), (4, 2), (2, 2), (3, 1), (3, 2), (5, 1), (5, 3), (7, 1), (8, 4)]
STAGED_SHAPES = [(6, 2), (14, 1)]
ALL_PITCHES = (304, 528, 1040, 1296)
FRAME_SHAPES = [(10, 3), (4, 2), (8, 4), (6, 2)]


def pitches_for(k, m):
    """304: one partial pass on either lane width; 528: 8-B lanes + lane-mapped tail, on 16-B lanes a
    single partial pass; 1040: 16-B lanes + tail + the row-0 bypass, on 8-B lanes two passes + tail;
    1296: a partial last pass."""
    return ALL_PITCHES if (k, m) in ((10, 3), (4, 2)) else (304, 1040)


def forms_for(k, m):
    """wire_rx settings: 0 staged, 1 auto, 2 / 3 16-B lanes with / without the LDS stage, 4 / 5 8-B
    lanes likewise.  A shape without a k_rx instance takes the staged path under every setting."""
    return (0, 1, 2, 3, 4, 5) if (k, m) in FUSED_SHAPES else (0, 1)


def full_matrix(oracle, k, m):
    """The n x k fec.c matrix: identity on top of the Vandermonde parity rows."""
    return np.concatenate([np.eye(k, dtype=np.uint8), oracle.vandermonde(k, k + m)])


def min_wire_pitch(shard_pitch):
    return (shard_pitch + 13 + 15) // 16 * 16


def _sum16(b):
    return int(np.asarray(b, np.int64).sum()) & 0xFFFF


# ------------------------------------------------------------------ the model

Model = collections.namedtuple("Model", "valid rx_size status psize data rounds")
FramesModel = collections.namedtuple("FramesModel", "frame_status conv_hid rx")


def parse_row(oracle, row, ln, slot, k, n, wire_pitch, shard_pitch):
    """unpack_fec_head (FecCodecBuf.cpp:334-411) and the slot tests of NetFecCodec.cpp:200-213 on one
    received row -> (header accepted, shard checksum right, shard bytes).  The length tests come
    before oracle.unpack_head, which reads the checksum field without checking len >= 13."""
    if not 11 <= ln <= wire_pitch:
        return False, False, None
    tag = int(row[0])
    if tag not in (0xEC, 0xED):
        return False, False, None
    # the TAG decides the header length and whether the datagram sum is checked, whatever the call's
    # `checksum` argument says (that one only decides `head` and dec_src's payload check)
    hdr = 13 if tag == 0xED else 11
    if ln < hdr or ln - hdr > shard_pitch:
        return False, False, None
    rc, _, _, hn, hk, ik, _, body = oracle.unpack_head(row[:ln])
    if (hn, hk, ik) != (n, k, slot):
        return False, False, None
    return True, rc == 1, body


def _rounds(hdr_ok, ok, k):
    """How many of a group's successive first-k candidates fail their checksum and are dropped."""
    avail = [j for j in range(len(hdr_ok)) if hdr_ok[j]]
    dropped = 0
    while True:
        cand = avail[:k] if len(avail) >= k else [j for j in avail if j < k]
        bad = [j for j in cand if not ok[j]]
        if not bad:
            return dropped
        dropped += len(bad)
        avail = [j for j in avail if j not in bad]


def rx_model(oracle, rows_full, k, m, wire, wire_len, checksum, dec_pkt_size, shard_pitch, dropped=None):
    """The receive of a batch wire [G][n][wire_pitch], wire_len [G][n] -> Model.  `dropped` [G][n]
    (frames): rows a lower layer rejects by its own checksum; they are candidates like a row whose
    shard checksum fails, and count as not received."""
    G, n, wire_pitch = wire.shape
    assert n == k + m and rows_full.shape == (n, k)
    P = shard_pitch
    head = 4 if checksum else 2
    valid = np.zeros((G, n), bool)
    rx_size = np.full((G, n), -1, np.int32)
    sh = np.zeros((G, n, P), np.uint8)
    rounds = np.zeros(G, np.int32)
    for g in range(G):
        hdr_ok = np.zeros(n, bool)
        for j in range(n):
            h, s, body = parse_row(oracle, wire[g, j], int(wire_len[g, j]), j, k, n, wire_pitch, P)
            hdr_ok[j] = h
            if h and s and not (dropped is not None and dropped[g, j]):
                valid[g, j] = True
                rx_size[g, j] = len(body)
                sh[g, j, :len(body)] = body  # an invalid row stays all zero
        rounds[g] = _rounds(hdr_ok, valid[g], k)
    # lost data rows of a group with k valid rows: fec_decode over the first k valid rows in group
    # order (NetFecCodec.cpp:504-528), over the full pitch; the others stay zero
    data = np.ascontiguousarray(sh[:, :k])
    par = np.ascontiguousarray(sh[:, k:])
    marks = marks_layout(valid, k)
    oracle.fec_reconstruct(rows_full[k:], data, par, marks, P)
    status = np.zeros((G, k), np.int32)
    psize = np.zeros((G, k), np.int32)
    for g in range(G):
        recoverable = valid[g].sum() >= k
        for i in range(k):
            if not valid[g, i] and not recoverable:
                status[g, i], psize[g, i] = -2, 0
                continue
            sz = int(data[g, i, 0]) | int(data[g, i, 1]) << 8
            psize[g, i] = sz
            if head + sz > P:  # a size field the row cannot hold (before dec_src, which would read past it)
                status[g, i] = -1
            else:
                status[g, i] = oracle.dec_src(data[g, i], dec_pkt_size, checksum)[0]
    return Model(valid, rx_size, status, psize, data, rounds)


def marks_layout(valid, k):
    """~valid [G, n] in rs.c layout: every group's k data marks, then every group's m parity marks."""
    return np.concatenate([(~valid[:, :k]).reshape(-1), (~valid[:, k:]).reshape(-1)]).astype(np.uint8)


def frames_model(oracle, rows_full, k, m, frames, frame_len, session, checksum, dec_pkt_size, shard_pitch):
    """RecvPacket (ProtocolBasic.cpp:155-199, oracle.unframe_udp) on every row, rows it rejects
    counting as not received, then rx_model on the datagrams inside.  A row longer than the pitch
    is 4.  conv_hid is meaningful only where frame_status is 0."""
    G, n, fpitch = frames.shape
    fp = 12 if session else 4
    st = np.zeros((G, n), np.int32)
    conv_hid = np.zeros((G, n, 2), np.uint32)
    dg = np.zeros((G, n, fpitch), np.uint8)
    dl = np.zeros((G, n), np.int32)
    dropped = np.zeros((G, n), bool)
    for g in range(G):
        for j in range(n):
            ln = int(frame_len[g, j])
            if ln > fpitch:
                st[g, j] = 4
                continue
            s, work, _ = oracle.unframe_udp(frames[g, j, :max(ln, 0)], gmask=GMASK, session=session)
            st[g, j] = s
            if s in (0, 2):  # 2: a candidate its frame checksum drops (the retry loop sees it)
                dg[g, j, :ln - fp] = work[fp:ln]
                dl[g, j] = ln - fp
                dropped[g, j] = s == 2
                if session:
                    conv_hid[g, j] = np.frombuffer(work[4:12].tobytes(), "<u4")
    rx = rx_model(oracle, rows_full, k, m, dg, dl, checksum, dec_pkt_size, shard_pitch, dropped=dropped)
    return FramesModel(st, conv_hid, rx)


# ------------------------------------------------------------------ scenario groups

class Group:
    """One group's n datagrams as the oracle's pack_group made them, to be edited by hand."""

    def __init__(self, oracle, full, k, m, P, wp, checksum, sizes, rng, g):
        self.oracle, self.full, self.k, self.m, self.n, self.P, self.wp = oracle, full, k, m, k + m, P, wp
        self.checksum = checksum
        self.head = 4 if checksum else 2
        sizes = np.asarray(sizes, np.int32)
        payload = rng.integers(1, 256, size=int(sizes.sum()) + 1, dtype=np.uint8)  # no zero bytes
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        self.dg, self.ln, _ = oracle.pack_group(k, self.n, full, payload, offs, sizes, 7 + 31 * g, 3 + 17 * g, checksum,
                                                shard_cap=max(2052, P), pitch=wp)
        self.payloads = [payload[o:o + s].copy() for o, s in zip(offs, sizes)]

    def hdr(self, j):
        return 13 if self.dg[j, 0] == 0xED else 11

    def resum(self, j):
        """Make row j's datagram checksum right again (an edit that must stay valid)."""
        if self.dg[j, 0] == 0xED:
            s = _sum16(self.dg[j, 13:self.ln[j]])
            self.dg[j, 11], self.dg[j, 12] = s & 0xFF, s >> 8

    def lose(self, *rows):
        for j in rows:
            self.ln[j] = 0

    def corrupt(self, j, where):
        """Flip a shard byte and leave the datagram sum stale: caught under 0xED, silent under 0xEC."""
        at = self.hdr(j) if where == "first" else int(self.ln[j]) - 1
        assert at < self.ln[j]
        self.dg[j, at] ^= 0x40

    def set_shard(self, j, shard):
        h = self.hdr(j)
        assert h + len(shard) <= self.wp
        self.dg[j, h:] = 0
        self.dg[j, h:h + len(shard)] = shard
        self.ln[j] = h + len(shard)
        self.resum(j)

    def shard(self, j):
        return self.dg[j, self.hdr(j):self.ln[j]].copy()

    def reencode(self):
        """Check datagrams again from the data shards as they now are (oracle.fec_encode over the
        longest data shard, as get_fec_encoded_pkt does over groupMax)."""
        k, m = self.k, self.m
        data = np.zeros((1, k, self.P), np.uint8)
        gmax = 0
        for i in range(k):
            s = self.shard(i)
            data[0, i, :len(s)] = s
            gmax = max(gmax, len(s))
        par = np.zeros((1, m, self.P), np.uint8)
        self.oracle.fec_encode(self.full[k:], data, par, gmax)
        for j in range(m):
            self.set_shard(k + j, par[0, j, :gmax])

    def retag(self, j):
        """0xED <-> 0xEC with the same shard: the two checksum bytes leave or come (sum right)."""
        s = self.shard(j)
        self.dg[j, 0] = 0xEC if self.dg[j, 0] == 0xED else 0xED
        self.set_shard(j, s)


def base_sizes(k, P, head, g, cap=None):
    """k payload sizes, rotating with the group over 0, 1, the pitch's limit, 13 short of it, two
    values whose shards end either side of byte 1024, and fillers; `cap` bounds them (dec_src batches)."""
    top = P - head
    pool = [0, 1, top, top - 13, 37, 200]
    if P >= 1040:
        pool[4:4] = [1022 - head, 1027 - head]
    pool = [min(s, top) for s in pool]
    if cap is not None:
        pool = [min(s, cap) for s in pool]
    return [pool[(g + i) % len(pool)] for i in range(k)]


Batch = collections.namedtuple("Batch", "wire wire_len names payloads wire_pitch dec_pkt_size skipped")


def _main_scenarios(k, m, P, checksum):
    """[(name, sizes override {row: size} or None, edit(Group))], and {name: why this shape cannot
    express it}."""
    n = k + m
    head = 4 if checksum else 2
    S, skipped = [], {}
    d1 = 1 % k           # the data row most edits go to
    pl = n - 1           # and the parity row

    def add(name, fn, sizes=None):
        S.append((name, sizes, fn))

    add("clean", lambda G_: None)
    for t in range(1, m + 1):
        if t <= k:
            add(f"lost-{t}-data", lambda G_, t=t: G_.lose(*range(t)))
        else:
            skipped[f"lost-{t}-data"] = "t > k"
        add(f"lost-{t}-parity", lambda G_, t=t: G_.lose(*range(k, k + t)))
        if t >= 2:
            add(f"lost-{t}-mixed", lambda G_, t=t: G_.lose(k - 1, *range(k, k + t - 1)))
        else:
            skipped[f"lost-{t}-mixed"] = "one row cannot be both"
    add(f"lost-{m + 1}", lambda G_: G_.lose(*([0] + list(range(n - m, n)))))

    # retry rounds: with checksums the corrupted rows are dropped one round after the other; without,
    # nothing is detected and the decode of the lost row k - 1 uses the corrupted survivors as they are
    tagname = "retry" if checksum else "silent-corrupt"

    def chain(G_, r):  # row 0, then the first parity row, then the next: each the replacement of the last
        rows = [0] + list(range(k, k + r - 1))
        for x, j in enumerate(rows):
            G_.corrupt(j, "first" if x % 2 == 0 else "last")
        if not checksum:
            G_.lose(k - 1)

    for r in range(1, m + 1):
        add(f"{tagname}-{r}", lambda G_, r=r: chain(G_, r))
    add(f"{tagname}-unrecoverable", lambda G_: chain(G_, m + 1))
    if m >= 2 and k >= 2:
        def both(G_):
            G_.corrupt(0, "last")
            G_.corrupt(1, "first")
            if not checksum:
                G_.lose(k - 1)
        add(f"{tagname}-two-at-once", both)
    else:
        skipped[f"{tagname}-two-at-once"] = "needs m >= 2"

    def extra_only(G_):
        G_.corrupt(pl, "last")
        if not checksum:
            G_.lose(0)  # the corrupted row is then no survivor (m >= 2) or the only spare (m = 1)
    add("bad-extra-only" if checksum else "silent-corrupt-extra", extra_only)

    # header rejects, instance 0 on a data row and instance 1 on a parity row
    def reject(name, fn):
        S.append((name, None, fn))

    def on(fn):
        return lambda G_, inst=0: fn(G_, d1 if inst == 0 else pl)

    def set_byte(at, val):
        def f(G_, j):
            G_.dg[j, at] = val(G_, j) if callable(val) else val
        return f

    def set_len(v):
        def f(G_, j):
            G_.ln[j] = v(G_, j) if callable(v) else v
        return f

    def ed_short(v):
        def f(G_, j):
            G_.dg[j, 0] = 0xED
            G_.ln[j] = v
        return f

    def empty(G_, j):  # len == hdr: a valid empty shard (an 0xED sum over nothing is 0)
        G_.set_shard(j, np.zeros(0, np.uint8))
        G_.lose(0 if j != 0 else k)

    def swap(G_, j):
        a, b = (0, 1) if j < k and k >= 2 else ((k, k + 1) if m >= 2 else (k - 1, k))
        G_.dg[[a, b]] = G_.dg[[b, a]]
        G_.ln[[a, b]] = G_.ln[[b, a]]

    def big(G_, j):
        G_.set_shard(j, np.arange(1, P + 17, dtype=np.int64).astype(np.uint8) | 1)

    for name, fn in (("tag-00", set_byte(0, 0x00)), ("tag-EE", set_byte(0, 0xEE)),
                     ("n-field", set_byte(9, lambda G_, j: ((n - 1) & 0xF) | (k << 4))),
                     ("k-field", set_byte(9, lambda G_, j: n | (((k - 1) & 0xF) << 4))),
                     ("ik-swap", swap), ("len-neg", set_len(-1)), ("len-1", set_len(1)), ("len-10", set_len(10)),
                     ("ED-len-11", ed_short(11)), ("ED-len-12", ed_short(12)), ("len-eq-hdr", empty),
                     ("len-over-pitch", set_len(lambda G_, j: G_.wp + 1)), ("shard-over-pitch", big)):
        reject(f"reject-{name}", on(fn))

    # one row of the other tag: as a survivor of a decode, and as a row past the first k
    def mix_survivor(G_):
        G_.retag(k - 1 if k >= 2 else k)
        G_.lose(0)
    add("tag-mix-survivor", mix_survivor)
    add("tag-mix-extra", lambda G_: G_.retag(pl))

    # bytes after head + size inside the datagram, received and decoded
    for e in (1, 7, 40):
        def trail(G_, e=e, lost=False):
            s = G_.shard(d1)
            ext = (np.arange(e, dtype=np.int64) * 29 + 3 * e).astype(np.uint8) | 1
            G_.set_shard(d1, np.concatenate([s, ext]))
            if lost:
                G_.reencode()
                G_.lose(d1)
        add(f"trailing-rx-{e}", trail, sizes={d1: 90})
        add(f"trailing-dec-{e}", lambda G_, e=e, f=trail: f(G_, e, True), sizes={d1: 90})

    # a size field the row cannot hold: -1 by head + size > pitch, received and decoded
    def oversize(G_, lost=False):
        s = G_.shard(d1)
        v = P - head + 1
        s[0], s[1] = v & 0xFF, v >> 8
        G_.set_shard(d1, s)
        G_.reencode()
        if lost:
            G_.lose(d1)
    add("size-field-over-pitch-rx", oversize)
    add("size-field-over-pitch-dec", lambda G_: oversize(G_, True))
    return S, skipped


def _dec_scenarios(k, m, P, checksum):
    """The dec_src batch (dec_pkt_size = SMALL_DEC): sizes either side of the bound, a wrong payload
    checksum under a right datagram sum, a size field past the pitch; each received and decoded."""
    head = 4 if checksum else 2
    S, skipped = [], {}
    d1 = 1 % k
    S.append(("clean", None, lambda G_: None))
    for sz in (SMALL_DEC - 2, SMALL_DEC - 1, SMALL_DEC, SMALL_DEC + 1):
        for how in ("rx", "dec"):
            name = f"size-{sz}-{how}"
            if head + sz > P:
                skipped[name] = "head + size > pitch"
                continue
            S.append((name, {d1: sz}, (lambda G_: G_.lose(d1)) if how == "dec" else (lambda G_: None)))

    def inner(G_, lost=False):  # the payload checksum field wrong, the group consistent with it
        s = G_.shard(d1)
        s[2] ^= 0x01
        G_.set_shard(d1, s)
        G_.reencode()
        G_.lose(d1 if lost else (0 if d1 != 0 else k))  # received: a survivor of another row's decode
    for how in ("rx", "dec"):
        if checksum:
            S.append((f"inner-sum-{how}", None, lambda G_, how=how: inner(G_, how == "dec")))
        else:
            skipped[f"inner-sum-{how}"] = "no payload checksum without checksums"

    def oversize(G_, lost=False):
        s = G_.shard(d1)
        v = P - head + 1
        s[0], s[1] = v & 0xFF, v >> 8
        G_.set_shard(d1, s)
        G_.reencode()
        if lost:
            G_.lose(d1)
    S.append(("size-field-over-pitch-rx", None, oversize))
    S.append(("size-field-over-pitch-dec", None, lambda G_: oversize(G_, True)))
    return S, skipped


FRAME_DAMAGE = ("frame-sum", "frame-cmd", "frame-both", "frame-short", "frame-long", "frame-sum-chain")


@functools.lru_cache(maxsize=None)
def scenarios(oracle, k, m, shard_pitch, checksum, seed, kind="main", frames=False):
    """A batch in which group g is the scenario names[g]; every scenario sits at two group indices of
    different parity (instance 0 and 1: another group base mod 64, header rejects on a data row and
    on a parity row).  Deterministic; `seed` only draws payload bytes.  kind "main": wire pitch 32 B
    above the minimum, the default dec_pkt_size; "dec": the minimum pitch, dec_pkt_size 600.
    frames: clean groups are appended for the frame-level damage frames_batch applies."""
    P, n = shard_pitch, k + m
    head = 4 if checksum else 2
    full = full_matrix(oracle, k, m)
    wp = min_wire_pitch(P) + (32 if kind == "main" else 0)
    S, skipped = (_main_scenarios if kind == "main" else _dec_scenarios)(k, m, P, checksum)
    if frames:
        S = S + [(f, None, lambda G_: None) for f in FRAME_DAMAGE]
    if len(S) % 2 == 0:
        S = S + [("filler", None, lambda G_: None)]  # an odd count: instance 1 sits at the other parity
    rng = np.random.default_rng(seed)
    G = 2 * len(S)
    wire = np.zeros((G, n, wp), np.uint8)
    wire_len = np.zeros((G, n), np.int32)
    names, payloads = [], []
    for g in range(G):
        name, over, fn = S[g % len(S)]
        inst = g // len(S)
        sizes = base_sizes(k, P, head, g, cap=SMALL_DEC - 3 if kind == "dec" else None)
        for row, sz in (over or {}).items():
            sizes[row] = sz
        grp = Group(oracle, full, k, m, P, wp, checksum, sizes, rng, g)
        if name.startswith("reject-"):
            fn(grp, inst)
        else:
            fn(grp)
        # bytes of a row past its length are not the datagram's: garbage there must change nothing
        for j in range(n):
            e = max(int(grp.ln[j]), 0)
            if grp.ln[j] != 0 and e < wp:
                grp.dg[j, e:] = (np.arange(wp - e, dtype=np.int64) * 7 + g + j).astype(np.uint8) | 0x80
        wire[g], wire_len[g] = grp.dg, grp.ln
        names.append(name)
        payloads.append(grp.payloads)
    for a in (wire, wire_len):
        a.setflags(write=False)
    return Batch(wire, wire_len, tuple(names), payloads, wp, BIG_DEC if kind == "main" else SMALL_DEC, skipped)


def promised(k, m, shard_pitch, checksum, kind="main"):
    """The scenario names scenarios() must yield for this shape, and the reasons for those it skips."""
    S, skipped = (_main_scenarios if kind == "main" else _dec_scenarios)(k, m, shard_pitch, checksum)
    return [s[0] for s in S], skipped


# ------------------------------------------------------------------ frames

FrameBatch = collections.namedtuple("FrameBatch", "frames frame_len conv_hid frame_pitch batch")


def _damage_frame(row, ln, fp, kind):
    """Frame-level damage on one framed row in place -> its new length."""
    x = int(row[0]) ^ GMASK ^ 0x5A
    if kind == "sum":  # a payload byte: the frame checksum fails
        row[ln - 1] ^= 0x40
    elif kind in ("cmd", "both"):  # cmd without 0xA0, the checksum right ("cmd") or wrong too ("both")
        w = row[:ln] ^ np.uint8(x)
        w[2] = 0x11
        s = int(w[2:].astype(np.int64).sum())
        w[1] = ((~((s >> 16) + (s & 0xFFFF))) & 0xFF) ^ (0x01 if kind == "both" else 0)
        row[1:ln] = w[1:] ^ np.uint8(x)
    elif kind == "short":
        return fp - 1
    elif kind == "long":
        return len(row) + 1
    return ln


@functools.lru_cache(maxsize=None)
def frames_batch(oracle, k, m, shard_pitch, checksum, session, seed):
    """The main scenario batch framed row by row with oracle.frame_udp (a random mask per row, gmask
    0xA7), plus frame-level damage on rows of the clean groups appended for it: instance 0 on a data
    row, instance 1 on a parity row; frame-sum-chain on two successive first-k candidates (row 0 and
    its replacement, the first parity row), so the frame checksum drives the retry loop."""
    b = scenarios(oracle, k, m, shard_pitch, checksum, seed, "main", True)
    G, n, wp = b.wire.shape
    fp = 12 if session else 4
    fpitch = wp + 16
    rng = np.random.default_rng(seed + 1000)
    masks = rng.integers(0, 256, size=(G, n), dtype=np.uint8)
    ch = rng.integers(0, 2**32, size=(G, n, 2), dtype=np.uint64).astype(np.uint32)
    frames = np.zeros((G, n, fpitch), np.uint8)
    flen = np.zeros((G, n), np.int32)
    seen = collections.Counter()
    for g in range(G):
        inst = seen[b.names[g]]
        seen[b.names[g]] += 1
        for j in range(n):
            ln = int(b.wire_len[g, j])
            if ln <= 0:  # not received (0), or a length no frame can have: RecvPacket says short
                flen[g, j] = ln
                continue
            d = b.wire[g, j, :ln] if ln <= wp else np.concatenate([b.wire[g, j], np.full(ln - wp, 0x33, np.uint8)])
            f = oracle.frame_udp(d, masks[g, j], gmask=GMASK, conv_hid=ch[g, j] if session else None)
            frames[g, j, :len(f)] = f
            flen[g, j] = len(f)
        if b.names[g].startswith("frame-"):
            kind = b.names[g][len("frame-"):]
            rows = [0, k] if kind == "sum-chain" else [1 % k if inst == 0 else n - 1]
            for j in rows:
                flen[g, j] = _damage_frame(frames[g, j], int(flen[g, j]), fp, "sum" if kind == "sum-chain" else kind)
        for j in range(n):  # garbage past the frame
            e = max(int(flen[g, j]), 0)
            if flen[g, j] != 0 and e < fpitch:
                frames[g, j, e:] = (np.arange(fpitch - e, dtype=np.int64) * 5 + g + j).astype(np.uint8) | 0x80
    for a in (frames, flen, ch):
        a.setflags(write=False)
    return FrameBatch(frames, flen, ch, fpitch, b)


# ------------------------------------------------------------------ models, once per batch

@functools.lru_cache(maxsize=None)
def batch_model(oracle, k, m, shard_pitch, checksum, seed, kind="main"):
    b = scenarios(oracle, k, m, shard_pitch, checksum, seed, kind)
    mod = rx_model(oracle, full_matrix(oracle, k, m), k, m, b.wire, b.wire_len, checksum, b.dec_pkt_size, shard_pitch)
    for a in mod:
        a.setflags(write=False)
    return b, mod


@functools.lru_cache(maxsize=None)
def frames_batch_model(oracle, k, m, shard_pitch, checksum, session, seed):
    fb = frames_batch(oracle, k, m, shard_pitch, checksum, session, seed)
    mod = frames_model(oracle, full_matrix(oracle, k, m), k, m, fb.frames, fb.frame_len, session, checksum, BIG_DEC,
                       shard_pitch)
    return fb, mod


def seed_for(k, m, pitch, checksum):
    return k * 1000 + m * 100 + pitch + checksum


# ------------------------------------------------------------------ device buffers

def guarded64(host, off):
    """dispatch_common.Guarded with the base `off` (a multiple of 16 below 64) bytes past a 64-B
    boundary: the receive kernels want 16-B aligned rows, and k_rx derives its store split from the
    address of each group's first row mod 64."""
    import torch

    from dispatch_common import GUARD, Guarded, guard_pattern

    class Guarded64(Guarded):
        def __init__(self, host, off):
            host = np.array(host, order="C")  # a copy: the cached batches are read-only
            assert host.dtype == np.uint8 and off % 16 == 0 and 0 <= off < 64
            n = host.size
            self.flat = torch.empty(GUARD + n + GUARD + 128, dtype=torch.uint8, device="cuda:0")
            self.start = (-self.flat.data_ptr()) % 64 + GUARD + off
            self.n = n
            self.pattern = guard_pattern(self.flat.numel())
            self.flat.copy_(torch.from_numpy(self.pattern))
            self.t = self.flat[self.start:self.start + n].view(host.shape)
            self.t.copy_(torch.from_numpy(host))
            assert self.t.data_ptr() % 64 == off and self.t.is_contiguous()

    return Guarded64(host, off)


def sentinel(*shape):
    return np.full(shape, SENTINEL, np.uint8)
