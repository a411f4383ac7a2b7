"""Python face of libqfec: the batched device codec and the reference's per-call ABIs.

* ``Code``          -- a (k, m) code on the MI355X; ``encode`` / ``reconstruct`` run whole
                       batches of groups on device tensors (torch, uint8) on the current
                       HIP stream.  Mirrors module/rs.c's batched API (rs.h:22-49) over the
                       contiguous layout of include/qfec.h.
* ``FecParms``      -- system/fec.h's per-packet codec (fec_new / fec_encode / fec_decode),
                       the interface network/FecCodec.cpp and network/FecCodecBuf.cpp bind.
* ``ReedSolomon``   -- module/rs.h's per-call codec over shard pointer arrays.

All arithmetic runs in the HIP kernels of libqfec.so; these classes only marshal.
"""
import ctypes as C

import numpy as np

from ._lib import QFEC_CAUCHY, QFEC_LOC_INVALID, QFEC_VANDERMONDE, RSStruct, QfecError, check, lib

LOC_INVALID = QFEC_LOC_INVALID  # verify / locate / scrub _ptrs_var: a group refused for its lengths

__all__ = ["Code", "FecParms", "ReedSolomon", "QfecError", "QFEC_CAUCHY", "QFEC_VANDERMONDE",
           "set_kernel_variant", "tune", "synth_fill", "probe_stream", "probe_reconstruct", "rs_host_devices", "device_count", "frame_udp", "unframe_udp",
           "NetFec", "Pipe", "Zfec"]


def _stream_handle(stream):
    if stream is None:
        import torch
        if not torch.cuda.is_available():  # host-only calls (e.g. qfec_net's FEC-off traffic)
            return None
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if isinstance(stream, int):
        return C.c_void_p(stream)
    return C.c_void_p(stream.cuda_stream)


_U8, _I32, _I64 = "u8", "i32", "i64"


def _dev_ptr(t, kind=_U8, what="tensor"):
    """Device pointer of a contiguous tensor on the CURRENT device (the C side launches on the
    calling thread's current device and stream), with the element type the ABI reads:
    u8 = torch.uint8 bytes, i32 = 4-byte integers (int32 / uint32), i64 = int64."""
    if t is None:
        return None
    if not getattr(t, "is_cuda", False):
        raise QfecError(f"{what}: expected a device tensor")
    if not t.is_contiguous():
        raise QfecError(f"{what}: expected a contiguous tensor")
    import torch
    ok = {_U8: t.dtype == torch.uint8,
          _I32: t.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)),
          _I64: t.dtype == torch.int64}[kind]
    if not ok:
        raise QfecError(f"{what}: dtype {t.dtype} where the ABI reads {kind}")
    if t.device.index != torch.cuda.current_device():
        raise QfecError(f"{what}: on {t.device} but the current device is cuda:{torch.cuda.current_device()} "
                        "(use `with torch.cuda.device(...)`)")
    return C.c_void_p(t.data_ptr())


def device_count():
    return lib().qfec_device_count()


def set_kernel_variant(v):
    check(lib().qfec_set_kernel_variant(v), "qfec_set_kernel_variant")


def tune(key, value):
    """Experiment knob (see include/qfec.h qfec_tune); outputs are identical either way."""
    check(lib().qfec_tune(key.encode(), int(value)), f"qfec_tune({key})")


def tune_get(key):
    """The current value of a qfec_tune knob."""
    v = C.c_int(0)
    check(lib().qfec_tune_get(key.encode(), C.byref(v)), f"qfec_tune_get({key})")
    return v.value


def percall_stats():
    """The current device's resident per-call server (include/qfec.h qfec_percall_stats)."""
    out = (C.c_ulonglong * 5)()
    check(lib().qfec_percall_stats(out), "qfec_percall_stats")
    usable = out[4] if out[4] < 2**63 else out[4] - 2**64
    return {"calls": out[0], "launches": out[1], "relaunches": out[2], "running": bool(out[3]), "usable": usable}


def percall_counters():
    """qfec_percall_counters: percall_stats plus timeouts, fec_encode group-cache hits / misses, the
    current percall_idle_us and the servers abandoned after percall_stop_us."""
    out = (C.c_ulonglong * 10)()
    n = lib().qfec_percall_counters(out, 10)
    check(n if n < 0 else 0, "qfec_percall_counters")
    usable = out[4] if out[4] < 2**63 else out[4] - 2**64
    return {"calls": out[0], "launches": out[1], "relaunches": out[2], "running": bool(out[3]), "usable": usable,
            "timeouts": out[5], "group_hits": out[6], "group_misses": out[7], "idle_us": out[8],
            "abandoned": out[9]}


def synth_fill(t, seed, stream=None):
    """Fill a device uint8 tensor with quicknet_amd.synth.synth_bytes(seed, t.numel())."""
    check(lib().qfec_synth_fill(_dev_ptr(t, what="synth_fill"), t.numel(), seed & 0xFFFFFFFFFFFFFFFF, _stream_handle(stream)),
          "qfec_synth_fill")


def rs_host_devices(devices=None):
    """qfec_rs_host_devices: spread module/rs.h's host-pointer pipelines over two slots per listed
    device (repeats allowed); None or [] -> the calling thread's current device.  Returns the list
    now in force."""
    devs = list(devices or [])
    arr = (C.c_int * max(1, len(devs)))(*devs)
    check(lib().qfec_rs_host_devices(arr if devs else None, len(devs)), "qfec_rs_host_devices")
    out = (C.c_int * 64)()
    n = lib().qfec_rs_host_devices_get(out, 64)
    check(min(n, 0), "qfec_rs_host_devices_get")
    return list(out[:n])


def probe_reconstruct(data, parity, marks, block_size, lds_cap=0, stream=None):
    """Calibration only: the reconstruct's memory skeleton (RS(10,3), RS(16,4)); the erased rows
    of `data` receive garbage.  lds_cap: LDS bytes per block (0 none), a residency cap."""
    G, k, pitch = data.shape
    m = parity.shape[1]
    check(lib().qfec_probe_reconstruct(_dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"),
                                       _dev_ptr(marks, what="marks"), G, k, m, block_size, pitch, lds_cap,
                                       _stream_handle(stream)), "qfec_probe_reconstruct")


def probe_stream(data, parity, block_size, stream=None):
    """Calibration only: the encode's traffic with XOR in place of GF arithmetic."""
    G, k, pitch = data.shape
    m = parity.shape[1]
    check(lib().qfec_probe_stream(_dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"), G, k, m, block_size, pitch,
                                  _stream_handle(stream)), "qfec_probe_stream")


def frame_udp(rows, lengths, masks, gmask=0, cmd=0x11, protocol=0xFF, conv_hid=None, out_pitch=None, stream=None):
    """ProtocolUdp framing of a datagram batch (include/qfec.h qfec_frame_udp): rows uint8
    [R, pitch] device tensor, lengths int32 [R], masks uint8 [R] (per-packet Session _mask),
    conv_hid uint32/int32 [R, 2] or None.  Defaults: QUICKNET_CMD_DATA, QUICKNET_PROTOCOL_FEC
    (network/ProtocolBasic.h:82,95), as Session::TransmissionOutput sets them for FEC datagrams
    (network/SessionDesc.cpp:513-519).  Returns (framed [R, out_pitch], framed_len [R])."""
    import torch
    R, pitch = rows.shape
    P = 12 if conv_hid is not None else 4
    if out_pitch is None:
        out_pitch = (pitch + P + 15) // 16 * 16
    out = torch.empty((R, out_pitch), dtype=torch.uint8, device=rows.device)
    out_len = torch.empty(R, dtype=torch.int32, device=rows.device)
    check(lib().qfec_frame_udp(_dev_ptr(rows, what="rows"), pitch, _dev_ptr(lengths, _I32, "lengths"), R,
                               _dev_ptr(masks, what="masks"),
                               _dev_ptr(conv_hid, _I32, "conv_hid") if conv_hid is not None else None, int(gmask), int(cmd),
                               int(protocol), _dev_ptr(out), out_pitch, _dev_ptr(out_len, _I32), _stream_handle(stream)),
          "qfec_frame_udp")
    return out, out_len


def unframe_udp(frames, lengths, gmask=0, session=False, out_pitch=None, stream=None):
    """Reverse of frame_udp (qfec_unframe_udp).  Returns (data [R, out_pitch], data_len [R],
    status [R], info uint8 [R, 4], conv_hid int32 [R, 2] or None)."""
    import torch
    R, pitch = frames.shape
    if out_pitch is None:
        out_pitch = pitch
    dev = frames.device
    out = torch.empty((R, out_pitch), dtype=torch.uint8, device=dev)
    out_len = torch.empty(R, dtype=torch.int32, device=dev)
    status = torch.empty(R, dtype=torch.int32, device=dev)
    info = torch.empty((R, 4), dtype=torch.uint8, device=dev)
    ch = torch.zeros((R, 2), dtype=torch.int32, device=dev) if session else None
    check(lib().qfec_unframe_udp(_dev_ptr(frames, what="frames"), pitch, _dev_ptr(lengths, _I32, "lengths"), R, int(gmask),
                                 int(bool(session)), _dev_ptr(out), out_pitch, _dev_ptr(out_len, _I32),
                                 _dev_ptr(status, _I32), _dev_ptr(info),
                                 _dev_ptr(ch, _I32) if ch is not None else None, _stream_handle(stream)), "qfec_unframe_udp")
    return out, out_len, status, info, ch


class Code:
    """A GF(2^8) RS code with k data and m parity shards per group."""

    def __init__(self, handle, owner=True):
        if not handle:
            raise QfecError(f"invalid code: {lib().qfec_last_error().decode()}")
        self._h = C.c_void_p(handle)
        self._owner = owner
        k, m = C.c_int(), C.c_int()
        check(lib().qfec_code_shape(self._h, C.byref(k), C.byref(m)), "qfec_code_shape")
        self.k, self.m = k.value, m.value

    @classmethod
    def cauchy(cls, k, m):
        """module/rs.c's matrix (reed_solomon_new, rs.c:437-440)."""
        return cls(lib().qfec_code_new(QFEC_CAUCHY, k, m))

    @classmethod
    def vandermonde(cls, k, m):
        """module/fec.c's matrix (fec_new(k, k + m), fec.c:653-707)."""
        return cls(lib().qfec_code_new(QFEC_VANDERMONDE, k, m))

    @classmethod
    def from_rows(cls, rows, rs_stale_quirk=False):
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        m, k = rows.shape
        return cls(lib().qfec_code_from_rows(k, m, rows.ctypes.data, int(rs_stale_quirk)))

    def close(self):
        if self._h and self._owner:
            lib().qfec_code_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def rows(self):
        out = np.zeros((self.m, self.k), dtype=np.uint8)
        check(lib().qfec_code_rows(self._h, out.ctypes.data), "qfec_code_rows")
        return out

    def encode_host(self, data, parity, block_size=None):
        """qfec_encode_host: data uint8 [G, k, pitch] and parity [G, m, pitch] in HOST memory
        (numpy arrays, or CPU tensors, pinned or not); returns when parity is written."""
        G, k, pitch = data.shape
        if k != self.k or parity.shape[0] != G or parity.shape[1] != self.m or parity.shape[2] != pitch:
            raise QfecError(f"shape mismatch: data {tuple(data.shape)} parity {tuple(parity.shape)} for ({self.k},{self.m})")
        block_size = pitch if block_size is None else block_size
        ptr = (lambda a: a.ctypes.data) if isinstance(data, np.ndarray) else (lambda t: t.data_ptr())
        for a in (data, parity):
            if not (a.flags["C_CONTIGUOUS"] if isinstance(a, np.ndarray) else a.is_contiguous()):
                raise QfecError("encode_host: contiguous host buffers required")
        check(lib().qfec_encode_host(self._h, ptr(data), ptr(parity), G, block_size, pitch), "qfec_encode_host")

    def reconstruct_host(self, data, parity, marks, block_size=None):
        """qfec_reconstruct_host: data uint8 [G, k, pitch] rewritten in place from parity
        [G, m, pitch] and rs.c-layout marks [G*(k+m)], all in HOST memory (numpy arrays, or
        CPU tensors, pinned or not).  Returns the number of under-determined groups."""
        G, k, pitch = data.shape
        nmarks = marks.size if isinstance(marks, np.ndarray) else marks.numel()
        if k != self.k or tuple(parity.shape) != (G, self.m, pitch) or nmarks != G * (self.k + self.m):
            raise QfecError("reconstruct_host: shape mismatch")
        block_size = pitch if block_size is None else block_size
        nf = C.c_longlong(0)
        check(lib().qfec_reconstruct_host(self._h, _host_ptr(data, "data"), _host_ptr(parity, "parity"),
                                          _host_ptr(marks, "marks"), G, block_size, pitch, C.byref(nf)),
              "qfec_reconstruct_host")
        return int(nf.value)

    def encode(self, data, parity, block_size=None, stream=None):
        """parity[g] = P x data[g]; data uint8 [G, k, pitch], parity uint8 [G, m, pitch] on device."""
        G, k, pitch = data.shape
        if k != self.k or parity.shape[0] != G or parity.shape[1] != self.m or parity.shape[2] != pitch:
            raise QfecError(f"shape mismatch: data {tuple(data.shape)} parity {tuple(parity.shape)} for ({self.k},{self.m})")
        block_size = pitch if block_size is None else block_size
        check(lib().qfec_encode(self._h, _dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"), G, block_size, pitch,
                                _stream_handle(stream)), "qfec_encode")

    def prepare_reconstruct(self):
        check(lib().qfec_prepare_reconstruct(self._h), "qfec_prepare_reconstruct")

    def reconstruct(self, data, parity, marks, block_size=None, failed=None, stream=None):
        """Rewrite erased data shards in place.  marks: uint8 [G*k + G*m] (rs.c layout) on device;
        failed: optional device int32/uint32 [1] counter of under-determined groups."""
        G, k, pitch = data.shape
        if k != self.k or parity.shape[0] != G or parity.shape[1] != self.m or marks.numel() != G * (self.k + self.m):
            raise QfecError("shape mismatch")
        block_size = pitch if block_size is None else block_size
        check(lib().qfec_reconstruct(self._h, _dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"),
                                     _dev_ptr(marks, what="marks"), G, block_size, pitch,
                                     _dev_ptr(failed, _I32, "failed"), _stream_handle(stream)), "qfec_reconstruct")

    def _ptr_groups(self, what, ptrs):
        n = self.k + self.m
        if ptrs.dim() != 1 or ptrs.numel() % n:
            raise QfecError(f"{what}: {tuple(ptrs.shape)} pointers are not groups * (k + m) = groups * {n}")
        return ptrs.numel() // n

    def encode_ptrs(self, ptrs, block_size, stream=None):
        """qfec_encode_ptrs: encode shards scattered in device memory.  ptrs: 1-D int64 device tensor of
        groups * (k + m) device addresses in rs.c's shard order -- every group's k data shards, then
        every group's m parity shards; each shard is exactly block_size bytes, at any alignment."""
        G = self._ptr_groups("encode_ptrs", ptrs)
        check(lib().qfec_encode_ptrs(self._h, _dev_ptr(ptrs, _I64, "ptrs"), G, int(block_size),
                                     _stream_handle(stream)), "qfec_encode_ptrs")

    def reconstruct_ptrs(self, ptrs, marks, block_size, failed=None, stream=None):
        """qfec_reconstruct_ptrs: rewrite the marked data shards in place where they lie.  ptrs as for
        encode_ptrs; marks: uint8 [G*k + G*m] (rs.c layout) on device; failed: optional device
        int32/uint32 [1] counter of under-determined groups (accumulates)."""
        G = self._ptr_groups("reconstruct_ptrs", ptrs)
        if marks.numel() != G * (self.k + self.m):
            raise QfecError(f"reconstruct_ptrs: {marks.numel()} marks for {G} groups of ({self.k},{self.m})")
        check(lib().qfec_reconstruct_ptrs(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(marks, what="marks"), G,
                                          int(block_size), _dev_ptr(failed, _I32, "failed"), _stream_handle(stream)),
              "qfec_reconstruct_ptrs")

    @staticmethod
    def _int32_count(what, name, t, count):
        import torch
        if t.dtype != torch.int32:
            raise QfecError(f"{what}: {name} has dtype {t.dtype}, int32 expected")
        if t.numel() != count:
            raise QfecError(f"{what}: {name} has {t.numel()} elements, {count} expected")

    def encode_ptrs_var(self, ptrs, lens, max_len, group_len=None, invalid=None, stream=None):
        """qfec_encode_ptrs_var: encode_ptrs on shards that each have their own length.  ptrs as for
        encode_ptrs; lens: int32 [G*k] on device, the length of every data shard in table order; max_len:
        the longest length any group may have.  group_len: optional int32 [G] on device, written (-1 for
        a void group, else the group's longest length: the bytes of each parity shard that count);
        invalid: optional device int32/uint32 [1] counter of void groups (accumulates)."""
        G = self._ptr_groups("encode_ptrs_var", ptrs)
        self._int32_count("encode_ptrs_var", "lens", lens, G * self.k)
        if group_len is not None:
            self._int32_count("encode_ptrs_var", "group_len", group_len, G)
        check(lib().qfec_encode_ptrs_var(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(lens, _I32, "lens"), G,
                                         int(max_len), _dev_ptr(group_len, _I32, "group_len"),
                                         _dev_ptr(invalid, _I32, "invalid"), _stream_handle(stream)),
              "qfec_encode_ptrs_var")

    def reconstruct_ptrs_var(self, ptrs, lens, group_len, marks, max_len, failed=None, invalid=None, stream=None):
        """qfec_reconstruct_ptrs_var: reconstruct_ptrs on shards that each have their own length.  ptrs,
        marks and failed as for reconstruct_ptrs; lens: int32 [G*k] on device (the entries of marked
        shards are not looked at); group_len: int32 [G] on device, the length of every group's parity
        shards, as encode_ptrs_var reported it; invalid: optional device int32/uint32 [1] counter of
        groups refused for their lengths (accumulates)."""
        G = self._ptr_groups("reconstruct_ptrs_var", ptrs)
        if marks.numel() != G * (self.k + self.m):
            raise QfecError(f"reconstruct_ptrs_var: {marks.numel()} marks for {G} groups of ({self.k},{self.m})")
        self._int32_count("reconstruct_ptrs_var", "lens", lens, G * self.k)
        self._int32_count("reconstruct_ptrs_var", "group_len", group_len, G)
        check(lib().qfec_reconstruct_ptrs_var(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(lens, _I32, "lens"),
                                              _dev_ptr(group_len, _I32, "group_len"), _dev_ptr(marks, what="marks"), G,
                                              int(max_len), _dev_ptr(failed, _I32, "failed"),
                                              _dev_ptr(invalid, _I32, "invalid"), _stream_handle(stream)),
              "qfec_reconstruct_ptrs_var")

    def _range_args(self, what, first, count):
        first, count = int(first), int(count)
        if first < 0 or count < 1 or first + count > self.k:
            raise QfecError(f"{what}: data shards [{first}, {first + count}) are not inside [0, {self.k})")
        return first, count

    def _per_group_args(self, what, G, shard, new):
        import torch
        self._int32_count(what, "shard", shard, G)
        if new.dtype != torch.int64 or new.numel() != G:
            raise QfecError(f"{what}: new has dtype {new.dtype} and {new.numel()} elements, {G} int64 addresses expected")

    def encode_update_ptrs(self, ptrs, first, count, block_size, accumulate=True, stream=None):
        """encode_update() on shards scattered in device memory (qfec_encode_update_ptrs): parity_j (^)=
        sum_c rows[j][first + c] x data shard first + c, over [0, block_size).  ptrs as for encode_ptrs;
        only the data entries first .. first + count - 1 and the parity entries of a group are
        dereferenced, the others may hold anything.  accumulate: XOR into the parity (True) or
        overwrite it (False).  True GF products, no rs.c stale-row quirk."""
        G = self._ptr_groups("encode_update_ptrs", ptrs)
        first, count = self._range_args("encode_update_ptrs", first, count)
        check(lib().qfec_encode_update_ptrs(self._h, first, count, _dev_ptr(ptrs, _I64, "ptrs"), G, int(block_size),
                                            int(bool(accumulate)), _stream_handle(stream)), "qfec_encode_update_ptrs")

    def update_ptrs(self, ptrs, shard, new, block_size, delta_only=False, invalid=None, stream=None):
        """update() on shards scattered in device memory (qfec_update_ptrs).  ptrs as for encode_ptrs;
        shard: device int32 [G] as for update(); new: device int64 [G], the address of every group's new
        row of block_size bytes -- or, with delta_only, of its delta old ^ new: then no data entry is
        dereferenced and only the parity is written.  Nothing of a group with a negative id is read,
        its entry of `new` included.  invalid: optional device int32/uint32 [1] counter of groups with
        an id >= k (accumulates)."""
        G = self._ptr_groups("update_ptrs", ptrs)
        self._per_group_args("update_ptrs", G, shard, new)
        check(lib().qfec_update_ptrs(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(shard, _I32, "shard"),
                                     _dev_ptr(new, _I64, "new"), int(bool(delta_only)), G, int(block_size),
                                     _dev_ptr(invalid, _I32, "invalid"), _stream_handle(stream)), "qfec_update_ptrs")

    def encode_update_ptrs_var(self, ptrs, first, count, lens, group_len, max_len, accumulate=True, invalid=None,
                               stream=None):
        """encode_update_ptrs() on shards that each have their own length (qfec_encode_update_ptrs_var).
        lens: int32 [G*k] on device (only the entries of the range are read); group_len: int32 [G] on
        device, an INPUT: the extent L of every group's parity shards.  Overwriting writes exactly [0, L),
        zero past the longest part; accumulating rewrites [0, longest part of the range) only.  invalid:
        optional device int32/uint32 [1] counter of groups refused for their lengths (accumulates)."""
        G = self._ptr_groups("encode_update_ptrs_var", ptrs)
        first, count = self._range_args("encode_update_ptrs_var", first, count)
        self._int32_count("encode_update_ptrs_var", "lens", lens, G * self.k)
        self._int32_count("encode_update_ptrs_var", "group_len", group_len, G)
        check(lib().qfec_encode_update_ptrs_var(self._h, first, count, _dev_ptr(ptrs, _I64, "ptrs"),
                                                _dev_ptr(lens, _I32, "lens"), _dev_ptr(group_len, _I32, "group_len"), G,
                                                int(max_len), int(bool(accumulate)), _dev_ptr(invalid, _I32, "invalid"),
                                                _stream_handle(stream)), "qfec_encode_update_ptrs_var")

    def update_ptrs_var(self, ptrs, lens, group_len, shard, new, new_len, max_len, delta_only=False, invalid=None,
                        stream=None):
        """update_ptrs() on shards that each have their own length (qfec_update_ptrs_var).  lens: int32
        [G*k] on device, read at the replaced shard only (None allowed with delta_only); group_len: int32
        [G]; new_len: int32 [G], the length of every new row.  Exactly [0, new_len) of the replaced shard
        and [0, max(old, new length)) of the parity shards are rewritten.  lens is NOT written: store
        new_len at lens[g*k + shard[g]] afterwards, on the same stream."""
        G = self._ptr_groups("update_ptrs_var", ptrs)
        self._per_group_args("update_ptrs_var", G, shard, new)
        if lens is not None or not delta_only:
            if lens is None:
                raise QfecError("update_ptrs_var: lens may be None with delta_only alone")
            self._int32_count("update_ptrs_var", "lens", lens, G * self.k)
        self._int32_count("update_ptrs_var", "group_len", group_len, G)
        self._int32_count("update_ptrs_var", "new_len", new_len, G)
        check(lib().qfec_update_ptrs_var(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(lens, _I32, "lens"),
                                         _dev_ptr(group_len, _I32, "group_len"), _dev_ptr(shard, _I32, "shard"),
                                         _dev_ptr(new, _I64, "new"), _dev_ptr(new_len, _I32, "new_len"),
                                         int(bool(delta_only)), G, int(max_len), _dev_ptr(invalid, _I32, "invalid"),
                                         _stream_handle(stream)), "qfec_update_ptrs_var")

    def prepare_repair(self):
        check(lib().qfec_prepare_repair(self._h), "qfec_prepare_repair")

    def repair(self, data, parity, marks, block_size=None, failed=None, stream=None):
        """Rewrite every marked shard, data and parity, in place (qfec_repair).  data uint8
        [G, k, pitch], parity uint8 [G, m, pitch], marks uint8 [G*k + G*m] (rs.c layout) on device;
        failed: optional device int32/uint32 [1] counter of under-determined groups (t > m)."""
        G, k, pitch = data.shape
        if k != self.k or tuple(parity.shape) != (G, self.m, pitch) or marks.numel() != G * (self.k + self.m):
            raise QfecError(f"shape mismatch: data {tuple(data.shape)} parity {tuple(parity.shape)} "
                            f"marks {marks.numel()} for ({self.k},{self.m})")
        block_size = pitch if block_size is None else block_size
        check(lib().qfec_repair(self._h, _dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"),
                                _dev_ptr(marks, what="marks"), G, block_size, pitch,
                                _dev_ptr(failed, _I32, "failed"), _stream_handle(stream)), "qfec_repair")

    def repair_rows(self, marks_n):
        """Host-side repair matrix for one group-order mark vector over all n shards:
        (t, rows[t,k], survivors[k], lost[t]); t = 0 nothing marked, -1 under-determined."""
        marks_n = np.ascontiguousarray(marks_n, dtype=np.uint8)
        if marks_n.size != self.k + self.m:
            raise QfecError(f"repair_rows: {marks_n.size} marks for ({self.k},{self.m})")
        rows = np.zeros((max(self.m, 1), self.k), dtype=np.uint8)
        surv = np.zeros(self.k, dtype=np.int32)
        lost = np.zeros(max(self.m, 1), dtype=np.int32)
        t = lib().qfec_repair_rows(self._h, marks_n.ctypes.data, rows.ctypes.data, surv.ctypes.data, lost.ctypes.data)
        if t <= 0:
            return t, None, None, None
        return t, rows[:t].copy(), surv, lost[:t].copy()

    def _group_args(self, what, data, parity, block_size, out, out_name="culprit", counts=None, ncounts=0, marks=None,
                    slots=1):
        """The checks verify / locate / scrub, the two erased calls and the two-shard calls share ->
        (G, block_size, pitch, out): out is the call's per-group device int32 [G] result ([G, slots]
        for the two-shard calls), allocated when not given; marks (the erased calls' input) and counts
        are checked when given."""
        import torch
        G, k, pitch = data.shape
        with_marks = "" if marks is None else f"marks {marks.numel()} "
        if (k != self.k or tuple(parity.shape) != (G, self.m, pitch)
                or (marks is not None and marks.numel() != G * (self.k + self.m))):
            raise QfecError(f"shape mismatch: data {tuple(data.shape)} parity {tuple(parity.shape)} "
                            f"{with_marks}for ({self.k},{self.m})")
        if out is None:
            out = torch.empty(G if slots == 1 else (G, slots), dtype=torch.int32, device=data.device)
        elif out.numel() != G * slots:
            raise QfecError(f"{what}: {out_name} has {out.numel()} elements for {G} groups" + (f" of {slots}" if slots > 1 else ""))
        if counts is not None and counts.numel() != ncounts:
            raise QfecError(f"{what}: counts has {counts.numel()} elements, not {ncounts}")
        return G, pitch if block_size is None else block_size, pitch, out

    def verify(self, data, parity, block_size=None, bad_rows=None, bad_groups=None, stream=None):
        """Does parity[g] equal P x data[g] (qfec_verify)?  Returns bad_rows, a device int32 [G]
        tensor (allocated when not given): bit j set = parity row j of that group differs in some
        byte of [0, block_size); bad_groups: optional device int32/uint32 [1] counter that gains 1
        per inconsistent group (accumulates)."""
        G, block_size, pitch, bad_rows = self._group_args("verify", data, parity, block_size, bad_rows, "bad_rows")
        check(lib().qfec_verify(self._h, _dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"), G, block_size,
                                pitch, _dev_ptr(bad_rows, _I32, "bad_rows"), _dev_ptr(bad_groups, _I32, "bad_groups"),
                                _stream_handle(stream)), "qfec_verify")
        return bad_rows

    def encode_update(self, part, parity, first, block_size=None, accumulate=True, stream=None):
        """parity[g][j] (^)= sum_c rows[j][first + c] x part[g][c] (qfec_encode_update): part uint8
        [G, count, pitch] holds the data rows first .. first + count - 1 of every group, parity uint8
        [G, m, pitch]; accumulate: XOR into parity (True) or overwrite it (False).  True GF products,
        no rs.c stale-row quirk."""
        G, count, pitch = part.shape
        if tuple(parity.shape) != (G, self.m, pitch):
            raise QfecError(f"shape mismatch: part {tuple(part.shape)} parity {tuple(parity.shape)} for ({self.k},{self.m})")
        block_size = pitch if block_size is None else block_size
        check(lib().qfec_encode_update(self._h, int(first), count, _dev_ptr(part, what="part"),
                                       _dev_ptr(parity, what="parity"), G, block_size, pitch, int(bool(accumulate)),
                                       _stream_handle(stream)), "qfec_encode_update")

    def update(self, shard, rows, parity, data=None, block_size=None, invalid=None, stream=None):
        """Replace one data shard per group and bring the parity along (qfec_update).  shard: device
        int32 [G], the data shard id 0..k-1 group g replaces, QFEC_UPD_NONE (any id < 0) = the group is
        untouched, an id >= k = untouched and counted; rows uint8 [G, pitch]: the shard's new bytes;
        parity uint8 [G, m, pitch]; data uint8 [G, k, pitch], or None: rows holds the deltas
        old ^ new and only the parity is written.  invalid: optional device int32/uint32 [1] counter
        of groups with an id >= k (accumulates)."""
        G, pitch = rows.shape
        if (tuple(parity.shape) != (G, self.m, pitch) or shard.numel() != G
                or (data is not None and tuple(data.shape) != (G, self.k, pitch))):
            raise QfecError(f"shape mismatch: shard {shard.numel()} rows {tuple(rows.shape)} parity {tuple(parity.shape)} "
                            f"data {None if data is None else tuple(data.shape)} for ({self.k},{self.m})")
        block_size = pitch if block_size is None else block_size
        check(lib().qfec_update(self._h, _dev_ptr(shard, _I32, "shard"), _dev_ptr(data, what="data"),
                                _dev_ptr(rows, what="rows"), _dev_ptr(parity, what="parity"), G, block_size, pitch,
                                _dev_ptr(invalid, _I32, "invalid"), _stream_handle(stream)), "qfec_update")

    def plan_stride(self):
        """Bytes per group of a decode plan (qfec_plan_stride), a multiple of 16."""
        n = lib().qfec_plan_stride(self._h)
        if n < 0:
            check(int(n), "qfec_plan_stride")
        return int(n)

    def plan_build(self, marks, mode, plan=None, failed=None, stream=None):
        """The decode plan of every group from its marks, on the device, for any k + m
        (qfec_plan_build).  marks: uint8 [G*k + G*m] (rs.c layout) on device; mode:
        QFEC_PLAN_RECONSTRUCT (erased data rows) or QFEC_PLAN_REPAIR (every marked shard).  Returns
        plan, a device uint8 [G, plan_stride()] tensor (allocated when not given; one passed in must
        start on a 16-byte boundary, which a slice of a tensor may not: the call refuses it otherwise);
        failed: optional device int32/uint32 [1] counter of groups whose plan failed (accumulates)."""
        import torch
        n = self.k + self.m
        if marks.numel() % n:
            raise QfecError(f"plan_build: {marks.numel()} marks are not groups * (k + m) = groups * {n}")
        G, stride = marks.numel() // n, self.plan_stride()
        if plan is None:
            plan = torch.empty((G, stride), dtype=torch.uint8, device=marks.device)
        elif plan.numel() != G * stride:
            raise QfecError(f"plan_build: plan has {plan.numel()} bytes for {G} groups of {stride}")
        check(lib().qfec_plan_build(self._h, _dev_ptr(marks, what="marks"), G, int(mode), _dev_ptr(plan, what="plan"),
                                    _dev_ptr(failed, _I32, "failed"), _stream_handle(stream)), "qfec_plan_build")
        return plan

    def plan_apply(self, data, parity, plan, block_size=None, stream=None):
        """Execute plans on a batch (qfec_plan_apply): data uint8 [G, k, pitch], parity uint8
        [G, m, pitch], plan uint8 [G, plan_stride()] from plan_build, 16-byte aligned.  Reads no marks
        and counts nothing; parity is written only where a plan lists parity rows."""
        G, k, pitch = data.shape
        if k != self.k or tuple(parity.shape) != (G, self.m, pitch) or plan.numel() != G * self.plan_stride():
            raise QfecError(f"shape mismatch: data {tuple(data.shape)} parity {tuple(parity.shape)} "
                            f"plan {plan.numel()} for ({self.k},{self.m})")
        block_size = pitch if block_size is None else block_size
        check(lib().qfec_plan_apply(self._h, _dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"),
                                    _dev_ptr(plan, what="plan"), G, block_size, pitch, _stream_handle(stream)),
              "qfec_plan_apply")

    def _wide(self, name, data, parity, marks, block_size, failed, stream):
        G, k, pitch = data.shape
        if k != self.k or tuple(parity.shape) != (G, self.m, pitch) or marks.numel() != G * (self.k + self.m):
            raise QfecError(f"shape mismatch: data {tuple(data.shape)} parity {tuple(parity.shape)} "
                            f"marks {marks.numel()} for ({self.k},{self.m})")
        block_size = pitch if block_size is None else block_size
        check(getattr(lib(), name)(self._h, _dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"),
                                   _dev_ptr(marks, what="marks"), G, block_size, pitch,
                                   _dev_ptr(failed, _I32, "failed"), _stream_handle(stream)), name)

    def reconstruct_wide(self, data, parity, marks, block_size=None, failed=None, stream=None):
        """reconstruct for any k + m, asynchronous (qfec_reconstruct_wide): the decode plans are built
        on the device from the marks.  Arguments as for reconstruct."""
        self._wide("qfec_reconstruct_wide", data, parity, marks, block_size, failed, stream)

    def repair_wide(self, data, parity, marks, block_size=None, failed=None, stream=None):
        """repair for any k + m, asynchronous (qfec_repair_wide).  Arguments as for repair."""
        self._wide("qfec_repair_wide", data, parity, marks, block_size, failed, stream)

    def plan_apply_ptrs(self, ptrs, plan, block_size, stream=None):
        """Execute plans on shards scattered in device memory (qfec_plan_apply_ptrs).  ptrs as for
        encode_ptrs; plan uint8 [G, plan_stride()] from plan_build, 16-byte aligned; each shard is
        exactly block_size bytes, at any alignment.  Reads no marks and counts nothing."""
        G = self._ptr_groups("plan_apply_ptrs", ptrs)
        if plan.numel() != G * self.plan_stride():
            raise QfecError(f"plan_apply_ptrs: plan has {plan.numel()} bytes for {G} groups of {self.plan_stride()}")
        check(lib().qfec_plan_apply_ptrs(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(plan, what="plan"), G,
                                         int(block_size), _stream_handle(stream)), "qfec_plan_apply_ptrs")

    def _ptrs_wide(self, name, ptrs, marks, block_size, failed, stream):
        G = self._ptr_groups(name[5:], ptrs)
        if marks.numel() != G * (self.k + self.m):
            raise QfecError(f"{name[5:]}: {marks.numel()} marks for {G} groups of ({self.k},{self.m})")
        check(getattr(lib(), name)(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(marks, what="marks"), G,
                                   int(block_size), _dev_ptr(failed, _I32, "failed"), _stream_handle(stream)), name)

    def reconstruct_ptrs_wide(self, ptrs, marks, block_size, failed=None, stream=None):
        """reconstruct_ptrs for any k + m, through device-built plans (qfec_reconstruct_ptrs_wide).
        Arguments as for reconstruct_ptrs."""
        self._ptrs_wide("qfec_reconstruct_ptrs_wide", ptrs, marks, block_size, failed, stream)

    def repair_ptrs_wide(self, ptrs, marks, block_size, failed=None, stream=None):
        """Rewrite every marked shard, data and parity, where it lies, for any k + m
        (qfec_repair_ptrs_wide).  Arguments as for reconstruct_ptrs."""
        self._ptrs_wide("qfec_repair_ptrs_wide", ptrs, marks, block_size, failed, stream)

    def plan_apply_ptrs_var(self, ptrs, lens, group_len, plan, max_len, invalid=None, stream=None):
        """plan_apply_ptrs on shards that each have their own length (qfec_plan_apply_ptrs_var).  ptrs and
        plan as for plan_apply_ptrs; lens: int32 [G*k] on device (the entries of shards the plan lists as
        lost are not looked at); group_len: int32 [G] on device, the length of every group's parity
        shards; invalid: optional device int32/uint32 [1] counter of groups refused for their lengths
        (accumulates).  Reads no marks."""
        G = self._ptr_groups("plan_apply_ptrs_var", ptrs)
        if plan.numel() != G * self.plan_stride():
            raise QfecError(f"plan_apply_ptrs_var: plan has {plan.numel()} bytes for {G} groups of {self.plan_stride()}")
        self._int32_count("plan_apply_ptrs_var", "lens", lens, G * self.k)
        self._int32_count("plan_apply_ptrs_var", "group_len", group_len, G)
        check(lib().qfec_plan_apply_ptrs_var(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(lens, _I32, "lens"),
                                             _dev_ptr(group_len, _I32, "group_len"), _dev_ptr(plan, what="plan"), G,
                                             int(max_len), _dev_ptr(invalid, _I32, "invalid"), _stream_handle(stream)),
              "qfec_plan_apply_ptrs_var")

    def _ptrs_wide_var(self, name, ptrs, lens, group_len, marks, max_len, failed, invalid, stream):
        G = self._ptr_groups(name[5:], ptrs)
        if marks.numel() != G * (self.k + self.m):
            raise QfecError(f"{name[5:]}: {marks.numel()} marks for {G} groups of ({self.k},{self.m})")
        self._int32_count(name[5:], "lens", lens, G * self.k)
        self._int32_count(name[5:], "group_len", group_len, G)
        check(getattr(lib(), name)(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(lens, _I32, "lens"),
                                   _dev_ptr(group_len, _I32, "group_len"), _dev_ptr(marks, what="marks"), G,
                                   int(max_len), _dev_ptr(failed, _I32, "failed"), _dev_ptr(invalid, _I32, "invalid"),
                                   _stream_handle(stream)), name)

    def reconstruct_ptrs_wide_var(self, ptrs, lens, group_len, marks, max_len, failed=None, invalid=None, stream=None):
        """reconstruct_ptrs_var for any k + m, through device-built plans (qfec_reconstruct_ptrs_wide_var).
        Arguments as for reconstruct_ptrs_var.  failed counts from the marks alone, invalid from the
        lengths of the groups the marks let through: a group is never in both."""
        self._ptrs_wide_var("qfec_reconstruct_ptrs_wide_var", ptrs, lens, group_len, marks, max_len, failed, invalid,
                            stream)

    def repair_ptrs_wide_var(self, ptrs, lens, group_len, marks, max_len, failed=None, invalid=None, stream=None):
        """Rewrite every marked shard, data and parity, where it lies, on shards that each have their own
        length, for any k + m (qfec_repair_ptrs_wide_var).  Arguments as for reconstruct_ptrs_wide_var;
        every marked shard has room for group_len bytes."""
        self._ptrs_wide_var("qfec_repair_ptrs_wide_var", ptrs, lens, group_len, marks, max_len, failed, invalid, stream)

    def _ptrs_out(self, what, ptrs, out, out_name, counts=None, ncounts=3):
        """The checks verify_ptrs / locate_ptrs / scrub_ptrs and the wide locates on tables share ->
        (G, out): out is the call's per-group device int32 [G] result, allocated when not given; counts
        is checked when given."""
        import torch
        G = self._ptr_groups(what, ptrs)
        if out is None:
            out = torch.empty(G, dtype=torch.int32, device=ptrs.device)
        else:
            if out.numel() != G:
                raise QfecError(f"{what}: {out_name} has {out.numel()} elements for {G} groups")
            if out.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                raise QfecError(f"{what}: {out_name} has dtype {out.dtype}, a 4-byte integer expected")
        if counts is not None and counts.numel() != ncounts:
            raise QfecError(f"{what}: counts has {counts.numel()} elements, not {ncounts}")
        return G, out

    def verify_ptrs(self, ptrs, block_size, bad_rows=None, bad_groups=None, stream=None):
        """verify() on shards scattered in device memory (qfec_verify_ptrs).  ptrs as for encode_ptrs;
        nothing is written into a shard.  Returns bad_rows, a device int32 [G] tensor (allocated when
        not given) with verify()'s bits; bad_groups: optional device int32/uint32 [1] counter that
        gains 1 per inconsistent group (accumulates)."""
        G, bad_rows = self._ptrs_out("verify_ptrs", ptrs, bad_rows, "bad_rows")
        check(lib().qfec_verify_ptrs(self._h, _dev_ptr(ptrs, _I64, "ptrs"), G, int(block_size),
                                     _dev_ptr(bad_rows, _I32, "bad_rows"), _dev_ptr(bad_groups, _I32, "bad_groups"),
                                     _stream_handle(stream)), "qfec_verify_ptrs")
        return bad_rows

    def locate_ptrs(self, ptrs, block_size, culprit=None, marks=None, counts=None, stream=None):
        """locate() on shards scattered in device memory (qfec_locate_ptrs).  ptrs as for encode_ptrs;
        nothing is written into a shard.  Returns culprit as locate() does.  marks: optional device
        uint8 [G*k + G*m] in the table's own order, written for every group -- ready for
        repair_ptrs_wide(); counts: optional device int32/uint32 [3] located / multi / ambiguous."""
        G, culprit = self._ptrs_out("locate_ptrs", ptrs, culprit, "culprit", counts)
        if marks is not None and marks.numel() != G * (self.k + self.m):
            raise QfecError(f"locate_ptrs: marks has {marks.numel()} elements for {G} groups of {self.k + self.m}")
        check(lib().qfec_locate_ptrs(self._h, _dev_ptr(ptrs, _I64, "ptrs"), G, int(block_size),
                                     _dev_ptr(culprit, _I32, "culprit"), _dev_ptr(marks, what="marks"),
                                     _dev_ptr(counts, _I32, "counts"), _stream_handle(stream)), "qfec_locate_ptrs")
        return culprit

    def scrub_ptrs(self, ptrs, block_size, culprit=None, counts=None, failed=None, stream=None):
        """locate_ptrs() + repair_ptrs_wide() of the located shard in one call (qfec_scrub_ptrs), at any
        k + m locate() takes: a group with one corrupted shard is rewritten to its original bytes where
        it lies, MULTI / AMBIGUOUS groups are left as they are and only reported.  failed: optional
        device int32/uint32 [1] counter of located groups with a singular plan (accumulates).  Returns
        culprit as locate() does."""
        G, culprit = self._ptrs_out("scrub_ptrs", ptrs, culprit, "culprit", counts)
        check(lib().qfec_scrub_ptrs(self._h, _dev_ptr(ptrs, _I64, "ptrs"), G, int(block_size),
                                    _dev_ptr(culprit, _I32, "culprit"), _dev_ptr(counts, _I32, "counts"),
                                    _dev_ptr(failed, _I32, "failed"), _stream_handle(stream)), "qfec_scrub_ptrs")
        return culprit

    def _ptrs_var_out(self, what, ptrs, lens, group_len, out, out_name, counts=None):
        """_ptrs_out plus the count and dtype checks of lens [G*k] and group_len [G]."""
        G, out = self._ptrs_out(what, ptrs, out, out_name, counts)
        self._int32_count(what, "lens", lens, G * self.k)
        self._int32_count(what, "group_len", group_len, G)
        return G, out

    def verify_ptrs_var(self, ptrs, lens, group_len, max_len, bad_rows=None, bad_groups=None, invalid=None, stream=None):
        """verify_ptrs() on shards that each have their own length (qfec_verify_ptrs_var).  ptrs as for
        encode_ptrs; lens: int32 [G*k] on device, the length of every data shard in table order;
        group_len: int32 [G] on device, the length of every group's parity shards, as encode_ptrs_var
        reported it; max_len: the longest length any group may have.  A data shard counts as
        zero-filled up to its group's length and is read below its own length only.  Returns bad_rows
        (0 for a group refused for its lengths); bad_groups / invalid: optional device int32/uint32 [1]
        counters of inconsistent groups / of groups refused for their lengths (accumulate)."""
        G, bad_rows = self._ptrs_var_out("verify_ptrs_var", ptrs, lens, group_len, bad_rows, "bad_rows")
        check(lib().qfec_verify_ptrs_var(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(lens, _I32, "lens"),
                                         _dev_ptr(group_len, _I32, "group_len"), G, int(max_len),
                                         _dev_ptr(bad_rows, _I32, "bad_rows"), _dev_ptr(bad_groups, _I32, "bad_groups"),
                                         _dev_ptr(invalid, _I32, "invalid"), _stream_handle(stream)),
              "qfec_verify_ptrs_var")
        return bad_rows

    def locate_ptrs_var(self, ptrs, lens, group_len, max_len, culprit=None, marks=None, counts=None, invalid=None,
                        stream=None):
        """locate_ptrs() on shards that each have their own length (qfec_locate_ptrs_var).  Arguments
        as for verify_ptrs_var.  Returns culprit as locate() does, with LOC_INVALID for a group refused
        for its lengths; a data shard is a candidate only if every syndrome is zero from its own end
        on.  marks as for locate_ptrs(): ready for repair_ptrs_wide_var() only where the marked shard
        has room for group_len bytes; scrub_ptrs_var() has no such condition."""
        G, culprit = self._ptrs_var_out("locate_ptrs_var", ptrs, lens, group_len, culprit, "culprit", counts)
        if marks is not None and marks.numel() != G * (self.k + self.m):
            raise QfecError(f"locate_ptrs_var: marks has {marks.numel()} elements for {G} groups of {self.k + self.m}")
        check(lib().qfec_locate_ptrs_var(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(lens, _I32, "lens"),
                                         _dev_ptr(group_len, _I32, "group_len"), G, int(max_len),
                                         _dev_ptr(culprit, _I32, "culprit"), _dev_ptr(marks, what="marks"),
                                         _dev_ptr(counts, _I32, "counts"), _dev_ptr(invalid, _I32, "invalid"),
                                         _stream_handle(stream)), "qfec_locate_ptrs_var")
        return culprit

    def scrub_ptrs_var(self, ptrs, lens, group_len, max_len, culprit=None, counts=None, invalid=None, stream=None):
        """locate_ptrs_var() and the correction of the located shard in one call (qfec_scrub_ptrs_var): a
        located data shard has exactly its own length rewritten, a located parity shard group_len
        bytes; every other group is left as it is.  No plan is built, so any code locate() takes is
        accepted.  Returns culprit as locate_ptrs_var() does."""
        G, culprit = self._ptrs_var_out("scrub_ptrs_var", ptrs, lens, group_len, culprit, "culprit", counts)
        check(lib().qfec_scrub_ptrs_var(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(lens, _I32, "lens"),
                                        _dev_ptr(group_len, _I32, "group_len"), G, int(max_len),
                                        _dev_ptr(culprit, _I32, "culprit"), _dev_ptr(counts, _I32, "counts"),
                                        _dev_ptr(invalid, _I32, "invalid"), _stream_handle(stream)),
              "qfec_scrub_ptrs_var")
        return culprit

    def plan_host(self, marks_n, mode):
        """The plan of one group-order mark vector over all n shards, computed on the CPU
        (qfec_plan_build_host): uint8 [plan_stride()] in the layout of include/qfec.h."""
        marks_n = np.ascontiguousarray(marks_n, dtype=np.uint8)
        if marks_n.size != self.k + self.m:
            raise QfecError(f"plan_host: {marks_n.size} marks for ({self.k},{self.m})")
        out = np.zeros(self.plan_stride(), dtype=np.uint8)
        check(lib().qfec_plan_build_host(self._h, marks_n.ctypes.data, int(mode), out.ctypes.data), "qfec_plan_build_host")
        return out

    def locate(self, data, parity, block_size=None, culprit=None, marks=None, counts=None, stream=None):
        """Which single shard of each group is corrupted (qfec_locate)?  Returns culprit, a device
        int32 [G] tensor (allocated when not given): the shard id 0..k+m-1, or QFEC_LOC_CLEAN (-1),
        QFEC_LOC_MULTI (-2), QFEC_LOC_AMBIGUOUS (-3).  marks: optional device uint8 [G*k + G*m]
        (rs.c layout), written for every group: 1 at the culprit, else 0 -- ready for repair().
        counts: optional device int32/uint32 [3] located / multi / ambiguous (accumulates)."""
        G, block_size, pitch, culprit = self._group_args("locate", data, parity, block_size, culprit)
        if marks is not None and marks.numel() != G * (self.k + self.m):
            raise QfecError(f"locate: marks has {marks.numel()} elements for {G} groups of {self.k + self.m}")
        if counts is not None and counts.numel() != 3:
            raise QfecError(f"locate: counts has {counts.numel()} elements, not 3")
        check(lib().qfec_locate(self._h, _dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"), G, block_size,
                                pitch, _dev_ptr(culprit, _I32, "culprit"), _dev_ptr(marks, what="marks"),
                                _dev_ptr(counts, _I32, "counts"), _stream_handle(stream)), "qfec_locate")
        return culprit

    def scrub(self, data, parity, block_size=None, culprit=None, counts=None, stream=None):
        """locate() + repair() of the located shard in one call (qfec_scrub): a group with one
        corrupted shard is rewritten to its original bytes, MULTI / AMBIGUOUS groups are left as
        they are and only reported.  Returns culprit as locate() does."""
        G, block_size, pitch, culprit = self._group_args("scrub", data, parity, block_size, culprit, counts=counts, ncounts=3)
        check(lib().qfec_scrub(self._h, _dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"), G, block_size,
                               pitch, _dev_ptr(culprit, _I32, "culprit"), _dev_ptr(counts, _I32, "counts"),
                               _stream_handle(stream)), "qfec_scrub")
        return culprit

    def locate_ratios(self):
        """The constants of locate(): uint8 [k, m-1], r[i, j-1] = rows[j, i] / rows[0, i] (CPU only)."""
        out = np.zeros((self.k, max(self.m - 1, 0)), dtype=np.uint8)
        scratch = np.zeros(max(out.size, 1), dtype=np.uint8)
        check(lib().qfec_locate_ratios(self._h, scratch.ctypes.data), "qfec_locate_ratios")
        out[:] = scratch[:out.size].reshape(out.shape)
        return out

    def locate2(self, data, parity, block_size=None, culprit=None, marks=None, counts=None, stream=None):
        """Which one or two shards of each group are corrupted (qfec_locate2, m >= 4)?  Returns
        culprit, a device int32 [G, 2] tensor (allocated when not given): (id, CLEAN) for one
        corrupted shard, (a, b) with a < b for two, else QFEC_LOC_CLEAN / MULTI / AMBIGUOUS in both
        slots.  marks: optional device uint8 [G*k + G*m] (rs.c layout), written for every group: 1 at
        each culprit, else 0 -- ready for repair().  counts: optional device int32/uint32 [4]
        one / two / multi / ambiguous (accumulates)."""
        G, block_size, pitch, culprit = self._group_args("locate2", data, parity, block_size, culprit, counts=counts,
                                                         ncounts=4, slots=2)
        if marks is not None and marks.numel() != G * (self.k + self.m):
            raise QfecError(f"locate2: marks has {marks.numel()} elements for {G} groups of {self.k + self.m}")
        check(lib().qfec_locate2(self._h, _dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"), G, block_size,
                                 pitch, _dev_ptr(culprit, _I32, "culprit"), _dev_ptr(marks, what="marks"),
                                 _dev_ptr(counts, _I32, "counts"), _stream_handle(stream)), "qfec_locate2")
        return culprit

    def scrub2(self, data, parity, block_size=None, culprit=None, counts=None, stream=None):
        """locate2() + repair() of the located shards in one call (qfec_scrub2): a group with one or
        two corrupted shards is rewritten to its original bytes, MULTI / AMBIGUOUS groups are left as
        they are and only reported.  Returns culprit as locate2() does."""
        G, block_size, pitch, culprit = self._group_args("scrub2", data, parity, block_size, culprit, counts=counts,
                                                         ncounts=4, slots=2)
        check(lib().qfec_scrub2(self._h, _dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"), G, block_size,
                                pitch, _dev_ptr(culprit, _I32, "culprit"), _dev_ptr(counts, _I32, "counts"),
                                _stream_handle(stream)), "qfec_scrub2")
        return culprit

    def locate2_checks(self, a, b):
        """The constants of locate2() for the pair {a, b}: uint8 [m-2, m] rows F with F . h_a = 0 and
        F . h_b = 0, h_x = column x of [rows | I] (CPU only)."""
        out = np.zeros((max(self.m - 2, 1), max(self.m, 1)), dtype=np.uint8)
        r = lib().qfec_locate2_checks(self._h, int(a), int(b), out.ctypes.data)
        if r < 0:
            check(r, "qfec_locate2_checks")
        return out[:r].copy()

    def prepare_locate_erased(self):
        check(lib().qfec_prepare_locate_erased(self._h), "qfec_prepare_locate_erased")

    def locate_erased(self, data, parity, marks, block_size=None, culprit=None, marks_out=None, counts=None,
                      stream=None):
        """Which single surviving shard of each group is corrupted, when groups also have lost shards
        (qfec_locate_erased)?  marks: device uint8 [G*k + G*m] (rs.c layout, non-zero = lost).
        Returns culprit, a device int32 [G] tensor (allocated when not given): the shard id, or
        QFEC_LOC_CLEAN (-1), MULTI (-2), AMBIGUOUS (-3), UNCHECKED (-4: t = m), LOST (-5: t > m).
        marks_out: optional device uint8 like marks (may be marks itself), written for every group:
        the marks as 0 / 1 plus 1 at a located culprit -- ready for repair().  counts: optional device
        int32/uint32 [5] located / multi / ambiguous / unchecked / lost (accumulates)."""
        G, block_size, pitch, culprit = self._group_args("locate_erased", data, parity, block_size, culprit, counts=counts,
                                                         ncounts=5, marks=marks)
        if marks_out is not None and marks_out.numel() != marks.numel():
            raise QfecError(f"locate_erased: marks_out has {marks_out.numel()} elements, marks {marks.numel()}")
        check(lib().qfec_locate_erased(self._h, _dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"),
                                       _dev_ptr(marks, what="marks"), G, block_size, pitch,
                                       _dev_ptr(culprit, _I32, "culprit"), _dev_ptr(marks_out, what="marks_out"),
                                       _dev_ptr(counts, _I32, "counts"), _stream_handle(stream)), "qfec_locate_erased")
        return culprit

    def scrub_erased(self, data, parity, marks, block_size=None, culprit=None, counts=None, failed=None, stream=None):
        """locate_erased() + repair() in one call (qfec_scrub_erased): lost shards and the one
        corrupted survivor of a group are rewritten to their original bytes; MULTI, AMBIGUOUS and
        LOST groups are left as they are and only reported; UNCHECKED groups and CLEAN groups with
        lost shards are repaired as repair() would.  failed: optional device int32/uint32 [1],
        repair()'s counter (the LOST groups).  Returns culprit as locate_erased() does."""
        G, block_size, pitch, culprit = self._group_args("scrub_erased", data, parity, block_size, culprit, counts=counts,
                                                         ncounts=5, marks=marks)
        check(lib().qfec_scrub_erased(self._h, _dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"),
                                      _dev_ptr(marks, what="marks"), G, block_size, pitch,
                                      _dev_ptr(culprit, _I32, "culprit"), _dev_ptr(counts, _I32, "counts"),
                                      _dev_ptr(failed, _I32, "failed"), _stream_handle(stream)), "qfec_scrub_erased")
        return culprit

    def locate_erased_plan(self, marks_n):
        """The host constants of locate_erased() for one group-order mark vector over all n shards:
        (spares, survivors[k], spare_ids[spares], rows[spares, k], ratios[k, spares-1]); spares = 0
        when t = m (survivors only, the rest None), -1 when t > m (all None).  CPU only."""
        marks_n = np.ascontiguousarray(marks_n, dtype=np.uint8)
        if marks_n.size != self.k + self.m:
            raise QfecError(f"locate_erased_plan: {marks_n.size} marks for ({self.k},{self.m})")
        m1 = max(self.m, 1)
        surv = np.zeros(self.k, dtype=np.int32)
        spares = np.zeros(m1, dtype=np.int32)
        rows = np.zeros(m1 * self.k, dtype=np.uint8)
        ratios = np.zeros(m1 * self.k, dtype=np.uint8)
        s = lib().qfec_locate_erased_plan(self._h, marks_n.ctypes.data, surv.ctypes.data, spares.ctypes.data,
                                          rows.ctypes.data, ratios.ctypes.data)
        if s < -1:
            check(s, "qfec_locate_erased_plan")
        if s < 0:
            return s, None, None, None, None
        if s == 0:
            return 0, surv, None, None, None
        return (s, surv, spares[:s].copy(), rows[:s * self.k].reshape(s, self.k).copy(),
                ratios[:self.k * (s - 1)].reshape(self.k, s - 1).copy())

    def check_stride(self):
        """Bytes per group of a check plan (qfec_check_stride), a multiple of 16."""
        n = lib().qfec_check_stride(self._h)
        if n < 0:
            check(int(n), "qfec_check_stride")
        return int(n)

    def check_build(self, marks=None, groups=None, check_plan=None, stream=None):
        """The check plan of every group from its marks, on the device, for any k + m
        (qfec_check_build).  marks: uint8 [G*k + G*m] (rs.c layout) on device, or None with
        `groups` given: no shard of any group is marked.  Returns the plans, a device uint8
        [G, check_stride()] tensor (allocated when not given; one passed in must start on a 16-byte
        boundary: the call refuses it otherwise)."""
        import torch
        n = self.k + self.m
        if marks is None:
            if groups is None:
                raise QfecError("check_build: groups is needed when no marks are given")
            G = int(groups)
        else:
            if marks.numel() % n or (groups is not None and marks.numel() != int(groups) * n):
                raise QfecError(f"check_build: {marks.numel()} marks are not groups * (k + m) = groups * {n}")
            G = marks.numel() // n
        stride = self.check_stride()
        if check_plan is None:
            check_plan = torch.empty((G, stride), dtype=torch.uint8, device="cuda" if marks is None else marks.device)
        elif check_plan.numel() != G * stride:
            raise QfecError(f"check_build: check_plan has {check_plan.numel()} bytes for {G} groups of {stride}")
        check(lib().qfec_check_build(self._h, _dev_ptr(marks, what="marks"), G, _dev_ptr(check_plan, what="check_plan"),
                                     _stream_handle(stream)), "qfec_check_build")
        return check_plan

    def check_host(self, marks_n):
        """The check plan of one group-order mark vector over all n shards, computed on the CPU
        (qfec_check_build_host): uint8 [check_stride()] in the layout of include/qfec.h."""
        marks_n = np.ascontiguousarray(marks_n, dtype=np.uint8)
        if marks_n.size != self.k + self.m:
            raise QfecError(f"check_host: {marks_n.size} marks for ({self.k},{self.m})")
        out = np.zeros(self.check_stride(), dtype=np.uint8)
        check(lib().qfec_check_build_host(self._h, marks_n.ctypes.data, out.ctypes.data), "qfec_check_build_host")
        return out

    def check_apply(self, data, parity, check_plan, block_size=None, culprit=None, marks_out=None, counts=None,
                    stream=None):
        """Run check plans on a batch (qfec_check_apply): which single surviving shard of each group is
        corrupted?  check_plan: uint8 [G, check_stride()] from check_build, 16-byte aligned; it holds
        the marks, so no marks are read.  culprit, marks_out and counts as for locate_erased().
        Returns culprit."""
        G, block_size, pitch, culprit = self._group_args("check_apply", data, parity, block_size, culprit, counts=counts,
                                                         ncounts=5)
        if check_plan.numel() != G * self.check_stride():
            raise QfecError(f"check_apply: check_plan has {check_plan.numel()} bytes for {G} groups of {self.check_stride()}")
        if marks_out is not None and marks_out.numel() != G * (self.k + self.m):
            raise QfecError(f"check_apply: marks_out has {marks_out.numel()} elements for {G} groups of {self.k + self.m}")
        check(lib().qfec_check_apply(self._h, _dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"),
                                     _dev_ptr(check_plan, what="check_plan"), G, block_size, pitch,
                                     _dev_ptr(culprit, _I32, "culprit"), _dev_ptr(marks_out, what="marks_out"),
                                     _dev_ptr(counts, _I32, "counts"), _stream_handle(stream)), "qfec_check_apply")
        return culprit

    def locate_wide(self, data, parity, marks=None, block_size=None, culprit=None, marks_out=None, counts=None,
                    stream=None):
        """locate_erased() for any k + m, asynchronous (qfec_locate_wide): the check plans are built on
        the device from the marks.  marks may be None (complete groups); the other arguments and the
        result as for locate_erased().  Accepts the codes qfec_code_new generates."""
        G, block_size, pitch, culprit = self._group_args("locate_wide", data, parity, block_size, culprit, counts=counts,
                                                         ncounts=5, marks=marks)
        if marks_out is not None and marks_out.numel() != G * (self.k + self.m):
            raise QfecError(f"locate_wide: marks_out has {marks_out.numel()} elements for {G} groups of {self.k + self.m}")
        check(lib().qfec_locate_wide(self._h, _dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"),
                                     _dev_ptr(marks, what="marks"), G, block_size, pitch,
                                     _dev_ptr(culprit, _I32, "culprit"), _dev_ptr(marks_out, what="marks_out"),
                                     _dev_ptr(counts, _I32, "counts"), _stream_handle(stream)), "qfec_locate_wide")
        return culprit

    def scrub_wide(self, data, parity, marks=None, block_size=None, culprit=None, counts=None, failed=None, stream=None):
        """locate_wide() + repair_wide() in one call (qfec_scrub_wide), under scrub_erased()'s rules,
        for any k + m.  Returns culprit as locate_erased() does."""
        G, block_size, pitch, culprit = self._group_args("scrub_wide", data, parity, block_size, culprit, counts=counts,
                                                         ncounts=5, marks=marks)
        check(lib().qfec_scrub_wide(self._h, _dev_ptr(data, what="data"), _dev_ptr(parity, what="parity"),
                                    _dev_ptr(marks, what="marks"), G, block_size, pitch,
                                    _dev_ptr(culprit, _I32, "culprit"), _dev_ptr(counts, _I32, "counts"),
                                    _dev_ptr(failed, _I32, "failed"), _stream_handle(stream)), "qfec_scrub_wide")
        return culprit

    def _marks_count(self, what, name, marks, G):
        if marks is not None and marks.numel() != G * (self.k + self.m):
            raise QfecError(f"{what}: {name} has {marks.numel()} elements for {G} groups of {self.k + self.m}")

    def check_apply_ptrs(self, ptrs, check_plan, block_size, culprit=None, marks_out=None, counts=None, stream=None):
        """check_apply() on shards scattered in device memory (qfec_check_apply_ptrs).  ptrs as for
        encode_ptrs; the entries of shards the plans mark as lost are never dereferenced and nothing is
        written into a shard; check_plan as for check_apply(); marks_out: optional device uint8
        [G*k + G*m] in the table's own order, ready for repair_ptrs_wide(); counts: optional device
        int32/uint32 [5].  Returns culprit."""
        G, culprit = self._ptrs_out("check_apply_ptrs", ptrs, culprit, "culprit", counts, 5)
        if check_plan.numel() != G * self.check_stride():
            raise QfecError(f"check_apply_ptrs: check_plan has {check_plan.numel()} bytes for {G} groups of "
                            f"{self.check_stride()}")
        self._marks_count("check_apply_ptrs", "marks_out", marks_out, G)
        check(lib().qfec_check_apply_ptrs(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(check_plan, what="check_plan"),
                                          G, int(block_size), _dev_ptr(culprit, _I32, "culprit"),
                                          _dev_ptr(marks_out, what="marks_out"), _dev_ptr(counts, _I32, "counts"),
                                          _stream_handle(stream)), "qfec_check_apply_ptrs")
        return culprit

    def locate_ptrs_wide(self, ptrs, block_size, marks=None, culprit=None, marks_out=None, counts=None, stream=None):
        """locate_wide() on shards scattered in device memory (qfec_locate_ptrs_wide), at any k + m,
        beside lost shards or not.  ptrs as for encode_ptrs; marks: uint8 [G*k + G*m] (rs.c layout, the
        table's own order) or None (complete groups); the entries of marked shards are never
        dereferenced and nothing is written into a shard.  The other arguments and the result as for
        locate_wide(); marks_out may be marks itself."""
        G, culprit = self._ptrs_out("locate_ptrs_wide", ptrs, culprit, "culprit", counts, 5)
        self._marks_count("locate_ptrs_wide", "marks", marks, G)
        self._marks_count("locate_ptrs_wide", "marks_out", marks_out, G)
        check(lib().qfec_locate_ptrs_wide(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(marks, what="marks"), G,
                                          int(block_size), _dev_ptr(culprit, _I32, "culprit"),
                                          _dev_ptr(marks_out, what="marks_out"), _dev_ptr(counts, _I32, "counts"),
                                          _stream_handle(stream)), "qfec_locate_ptrs_wide")
        return culprit

    def scrub_ptrs_wide(self, ptrs, block_size, marks=None, culprit=None, counts=None, failed=None, stream=None):
        """locate_ptrs_wide() + repair_ptrs_wide() in one call (qfec_scrub_ptrs_wide), under scrub_wide()'s
        rules: the located shard and the marked shards of its group are rewritten where they lie, so
        their entries must be real buffers.  Returns culprit as locate_wide() does."""
        G, culprit = self._ptrs_out("scrub_ptrs_wide", ptrs, culprit, "culprit", counts, 5)
        self._marks_count("scrub_ptrs_wide", "marks", marks, G)
        check(lib().qfec_scrub_ptrs_wide(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(marks, what="marks"), G,
                                         int(block_size), _dev_ptr(culprit, _I32, "culprit"),
                                         _dev_ptr(counts, _I32, "counts"), _dev_ptr(failed, _I32, "failed"),
                                         _stream_handle(stream)), "qfec_scrub_ptrs_wide")
        return culprit

    def _wide_var_out(self, what, ptrs, lens, group_len, culprit, counts):
        """_ptrs_out with five counts plus the count and dtype checks of lens [G*k] and group_len [G]."""
        G, culprit = self._ptrs_out(what, ptrs, culprit, "culprit", counts, 5)
        self._int32_count(what, "lens", lens, G * self.k)
        self._int32_count(what, "group_len", group_len, G)
        return G, culprit

    def check_apply_ptrs_var(self, ptrs, lens, group_len, check_plan, max_len, culprit=None, marks_out=None, counts=None,
                             invalid=None, stream=None):
        """check_apply_ptrs() on shards that each have their own length (qfec_check_apply_ptrs_var).  ptrs
        and check_plan as for check_apply_ptrs(); lens: int32 [G*k] on device (the entries of shards the
        plans mark are not looked at); group_len: int32 [G] on device, the length of every group's parity
        shards; max_len only sizes the launch.  A surviving data shard is read below its own length only
        and counts as zero up to group_len; a group refused for its lengths gets LOC_INVALID.  invalid:
        optional device int32/uint32 [1] counter of such groups (accumulates).  Returns culprit."""
        G, culprit = self._wide_var_out("check_apply_ptrs_var", ptrs, lens, group_len, culprit, counts)
        if check_plan.numel() != G * self.check_stride():
            raise QfecError(f"check_apply_ptrs_var: check_plan has {check_plan.numel()} bytes for {G} groups of "
                            f"{self.check_stride()}")
        self._marks_count("check_apply_ptrs_var", "marks_out", marks_out, G)
        check(lib().qfec_check_apply_ptrs_var(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(lens, _I32, "lens"),
                                              _dev_ptr(group_len, _I32, "group_len"),
                                              _dev_ptr(check_plan, what="check_plan"), G, int(max_len),
                                              _dev_ptr(culprit, _I32, "culprit"), _dev_ptr(marks_out, what="marks_out"),
                                              _dev_ptr(counts, _I32, "counts"), _dev_ptr(invalid, _I32, "invalid"),
                                              _stream_handle(stream)), "qfec_check_apply_ptrs_var")
        return culprit

    def locate_ptrs_wide_var(self, ptrs, lens, group_len, max_len, marks=None, culprit=None, marks_out=None, counts=None,
                             invalid=None, stream=None):
        """locate_ptrs_wide() on shards that each have their own length (qfec_locate_ptrs_wide_var), at
        any k + m, beside lost shards or not.  lens, group_len, max_len and invalid as for
        check_apply_ptrs_var(); marks, marks_out and counts as for locate_ptrs_wide().  marks_out is
        ready for repair_ptrs_wide_var() only where the marked culprit has room for group_len bytes;
        scrub_ptrs_wide_var() has no such condition.  Returns culprit."""
        G, culprit = self._wide_var_out("locate_ptrs_wide_var", ptrs, lens, group_len, culprit, counts)
        self._marks_count("locate_ptrs_wide_var", "marks", marks, G)
        self._marks_count("locate_ptrs_wide_var", "marks_out", marks_out, G)
        check(lib().qfec_locate_ptrs_wide_var(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(lens, _I32, "lens"),
                                              _dev_ptr(group_len, _I32, "group_len"), _dev_ptr(marks, what="marks"), G,
                                              int(max_len), _dev_ptr(culprit, _I32, "culprit"),
                                              _dev_ptr(marks_out, what="marks_out"), _dev_ptr(counts, _I32, "counts"),
                                              _dev_ptr(invalid, _I32, "invalid"), _stream_handle(stream)),
              "qfec_locate_ptrs_wide_var")
        return culprit

    def scrub_ptrs_wide_var(self, ptrs, lens, group_len, max_len, marks=None, culprit=None, counts=None, failed=None,
                            invalid=None, stream=None):
        """locate_ptrs_wide_var() and the repair of repair_ptrs_wide_var() in one call
        (qfec_scrub_ptrs_wide_var): lost shards are rewritten over group_len bytes, a located data shard
        over exactly its own length, a located parity shard over group_len bytes; INVALID, MULTI,
        AMBIGUOUS and LOST groups are left as they are.  Returns culprit."""
        G, culprit = self._wide_var_out("scrub_ptrs_wide_var", ptrs, lens, group_len, culprit, counts)
        self._marks_count("scrub_ptrs_wide_var", "marks", marks, G)
        check(lib().qfec_scrub_ptrs_wide_var(self._h, _dev_ptr(ptrs, _I64, "ptrs"), _dev_ptr(lens, _I32, "lens"),
                                             _dev_ptr(group_len, _I32, "group_len"), _dev_ptr(marks, what="marks"), G,
                                             int(max_len), _dev_ptr(culprit, _I32, "culprit"),
                                             _dev_ptr(counts, _I32, "counts"), _dev_ptr(failed, _I32, "failed"),
                                             _dev_ptr(invalid, _I32, "invalid"), _stream_handle(stream)),
              "qfec_scrub_ptrs_wide_var")
        return culprit

    # -- FEC datagram batches (network/FecCodecBuf.cpp wire format); n = k + m <= 15
    def pack_datagrams(self, payload, offsets, sizes, seq, checksum=True, shard_pitch=None, wire_pitch=None,
                       stream=None):
        """payload: uint8 device tensor (16 readable bytes past the last packet); offsets int64
        [G*k]; sizes int32 [G*k]; seq uint32/int32 [G, 2] (sent, src index of each group's first
        packet).  Returns (shards [G, n, pitch], wire [G, n, wire_pitch], wire_len int32 [G, n]).
        wire_pitch defaults to the 64-B multiple above 13 + shard_pitch (1088 for 1 KiB payloads;
        round 1 used the 16-B multiple, 1056): the fused send then writes whole 64-B lines.  Pass
        wire_pitch explicitly where a consumer needs another row layout."""
        import torch
        G = sizes.numel() // self.k
        n = self.k + self.m
        head = 4 if checksum else 2
        if shard_pitch is None:
            shard_pitch = (int(sizes.max().item()) + head + 15) // 16 * 16 if G else 16
        if wire_pitch is None:  # the 64-B multiple: the fused send then writes whole lines
            wire_pitch = (shard_pitch + 13 + 63) // 64 * 64
        dev = payload.device
        shards = torch.empty((G, n, shard_pitch), dtype=torch.uint8, device=dev)
        wire = torch.empty((G, n, wire_pitch), dtype=torch.uint8, device=dev)
        wire_len = torch.empty((G, n), dtype=torch.int32, device=dev)
        check(lib().qfec_pack_datagrams(self._h, _dev_ptr(payload, what="payload"), _dev_ptr(offsets, _I64, "offsets"),
                                        _dev_ptr(sizes, _I32, "sizes"), _dev_ptr(seq, _I32, "seq"),
                                        G, int(bool(checksum)), _dev_ptr(shards), shard_pitch, _dev_ptr(wire),
                                        wire_pitch, _dev_ptr(wire_len, _I32), _stream_handle(stream)), "qfec_pack_datagrams")
        return shards, wire, wire_len

    def unpack_datagrams(self, wire, wire_len, checksum=True, dec_pkt_size=2068, shard_pitch=None, stream=None):
        """wire [G, n, wire_pitch] uint8, wire_len int32 [G, n] (0 = not received).  Returns
        (shards [G, n, pitch], status int32 [G, k], psize int32 [G, k], rx_size int32 [G, n])."""
        import torch
        G, n, wire_pitch = wire.shape
        if shard_pitch is None:
            shard_pitch = (wire_pitch - 13) // 16 * 16
        dev = wire.device
        shards = torch.empty((G, n, shard_pitch), dtype=torch.uint8, device=dev)
        marks = torch.empty(G * n, dtype=torch.uint8, device=dev)
        rx = torch.empty((G, n), dtype=torch.int32, device=dev)
        status = torch.empty((G, self.k), dtype=torch.int32, device=dev)
        psize = torch.empty((G, self.k), dtype=torch.int32, device=dev)
        check(lib().qfec_unpack_datagrams(self._h, _dev_ptr(wire, what="wire"), wire_pitch,
                                          _dev_ptr(wire_len, _I32, "wire_len"), G, int(bool(checksum)),
                                          dec_pkt_size, _dev_ptr(shards), shard_pitch, _dev_ptr(marks), _dev_ptr(rx, _I32),
                                          _dev_ptr(status, _I32), _dev_ptr(psize, _I32), _stream_handle(stream)),
              "qfec_unpack_datagrams")
        return shards, status, psize, rx

    # -- the same batches straight to / from ProtocolUdp frames (qfec_pack_frames / qfec_unpack_frames)
    def pack_frames(self, payload, offsets, sizes, seq, masks, gmask=0, cmd=0x11, protocol=0xFF, conv_hid=None,
                    checksum=True, shard_pitch=None, frame_pitch=None, stream=None):
        """pack_datagrams + frame_udp in one call: masks uint8 [G*n] (one per datagram), conv_hid
        int32/uint32 [G*n, 2] or None (no Session prefix).  frame_pitch defaults to the 64-B
        multiple above prefix + 13 + shard_pitch (the one-pass kernel's pitch for 1 KiB and
        512-B payloads).  Returns (frames [G, n, frame_pitch], frame_len int32 [G, n])."""
        import torch
        G = sizes.numel() // self.k
        n = self.k + self.m
        head = 4 if checksum else 2
        P = 12 if conv_hid is not None else 4
        if shard_pitch is None:
            shard_pitch = (int(sizes.max().item()) + head + 15) // 16 * 16 if G else 16
        if frame_pitch is None:
            frame_pitch = (shard_pitch + 13 + P + 63) // 64 * 64
        dev = payload.device
        shards = torch.empty((G, n, shard_pitch), dtype=torch.uint8, device=dev)
        frames = torch.empty((G, n, frame_pitch), dtype=torch.uint8, device=dev)
        flen = torch.empty((G, n), dtype=torch.int32, device=dev)
        check(lib().qfec_pack_frames(self._h, _dev_ptr(payload, what="payload"), _dev_ptr(offsets, _I64, "offsets"),
                                     _dev_ptr(sizes, _I32, "sizes"), _dev_ptr(seq, _I32, "seq"), G, int(bool(checksum)),
                                     _dev_ptr(shards), shard_pitch, _dev_ptr(masks, what="masks"),
                                     _dev_ptr(conv_hid, _I32, "conv_hid") if conv_hid is not None else None,
                                     int(gmask), int(cmd), int(protocol), _dev_ptr(frames), frame_pitch,
                                     _dev_ptr(flen, _I32), _stream_handle(stream)), "qfec_pack_frames")
        return frames, flen

    def unpack_frames(self, frames, frame_len, gmask=0, session=False, checksum=True, dec_pkt_size=2068,
                      shard_pitch=None, stream=None):
        """unframe_udp + unpack_datagrams in one call.  frames [G, n, frame_pitch], frame_len int32
        [G, n] (0 = not received).  Returns (shards, status, psize, rx_size, frame_status [G, n],
        conv_hid [G, n, 2] int32 or None)."""
        import torch
        G, n, fpitch = frames.shape
        P = 12 if session else 4
        if shard_pitch is None:
            shard_pitch = (fpitch - 13 - P) // 16 * 16
        dev = frames.device
        shards = torch.empty((G, n, shard_pitch), dtype=torch.uint8, device=dev)
        marks = torch.empty(G * n, dtype=torch.uint8, device=dev)
        rx = torch.empty((G, n), dtype=torch.int32, device=dev)
        status = torch.empty((G, self.k), dtype=torch.int32, device=dev)
        psize = torch.empty((G, self.k), dtype=torch.int32, device=dev)
        fst = torch.empty((G, n), dtype=torch.int32, device=dev)
        ch = torch.zeros((G, n, 2), dtype=torch.int32, device=dev) if session else None
        check(lib().qfec_unpack_frames(self._h, _dev_ptr(frames, what="frames"), fpitch,
                                       _dev_ptr(frame_len, _I32, "frame_len"), G, int(gmask), int(bool(session)),
                                       int(bool(checksum)), dec_pkt_size, _dev_ptr(shards), shard_pitch, _dev_ptr(marks),
                                       _dev_ptr(rx, _I32), _dev_ptr(status, _I32), _dev_ptr(psize, _I32),
                                       _dev_ptr(fst, _I32), _dev_ptr(ch, _I32) if ch is not None else None,
                                       _stream_handle(stream)), "qfec_unpack_frames")
        return shards, status, psize, rx, fst, ch

    def decode_rows(self, marks_n):
        """Host-side decode matrix for one group-order mark vector: (e, rows[e,k], survivors[k], erased[e])."""
        marks_n = np.ascontiguousarray(marks_n, dtype=np.uint8)
        rows = np.zeros((self.m, self.k), dtype=np.uint8)
        surv = np.zeros(self.k, dtype=np.int32)
        lost = np.zeros(max(self.m, 1), dtype=np.int32)
        e = lib().qfec_decode_rows(self._h, marks_n.ctypes.data, rows.ctypes.data, surv.ctypes.data, lost.ctypes.data)
        if e <= 0:
            return e, None, None, None
        return e, rows[:e].copy(), surv, lost[:e].copy()


class FecParms:
    """system/fec.h: fec_new(k, n) / fec_encode / fec_decode / fec_free over packet buffers."""

    def __init__(self, k, n):
        self.k, self.n = k, n
        self._h = lib().fec_new(k, n)
        if not self._h:
            raise QfecError(f"fec_new({k}, {n}) failed")
        self._h = C.c_void_p(self._h)

    def close(self):
        if self._h:
            lib().fec_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def matrix(self):
        out = np.zeros((self.n, self.k), dtype=np.uint8)
        check(lib().qfec_fec_matrix(self._h, out.ctypes.data), "qfec_fec_matrix")
        return out

    def code(self):
        """The batched Code sharing this handle's matrix (not owned)."""
        return Code(lib().qfec_fec_code(self._h), owner=False)

    def encode(self, src, dst, index, sz):
        """src: k host uint8 arrays (or one [k, >=sz] array); dst: uint8 array written in place."""
        rows = [np.ascontiguousarray(s) for s in src]
        ptrs = (C.c_void_p * len(rows))(*[r.ctypes.data for r in rows])
        lib().fec_encode(self._h, ptrs, C.c_void_p(dst.ctypes.data), index, sz)

    def decode(self, pkts, index, sz):
        """pkts: [k, >=sz] uint8 array (slots), index: k ints.  Returns (rc, pkts_after, index_after)
        with the reference's in-place pointer/index permutation applied to copies."""
        buf = np.ascontiguousarray(pkts, dtype=np.uint8).copy()
        k, stride = buf.shape
        base = buf.ctypes.data
        ptrs = (C.c_void_p * k)(*[base + s * stride for s in range(k)])
        ia = (C.c_int * k)(*[int(x) for x in index])
        rc = lib().fec_decode(self._h, ptrs, ia, sz)
        after = np.stack([buf[(ptrs[s] - base) // stride] for s in range(k)])
        return rc, after, np.array(list(ia), dtype=np.int32)


class ReedSolomon:
    """module/rs.h: reed_solomon_new / encode / reconstruct / release over shard pointers."""

    def __init__(self, k, m):
        L = lib()
        L.reed_solomon_init()
        self._h = L.reed_solomon_new(k, m)
        if not self._h:
            raise QfecError(f"reed_solomon_new({k}, {m}) failed: errno {L.reed_solomon_error()}")
        self.k, self.m = k, m

    def close(self):
        if self._h:
            lib().reed_solomon_release(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def parity(self):
        """The public parity matrix (editable, as in rs.h:12)."""
        return np.ctypeslib.as_array(self._h.contents.parity, shape=(self.m, self.k))

    @property
    def m_matrix(self):
        """The public n x k matrix rs->m (editable, as in rs.h:11): reconstruct decodes from it."""
        return np.ctypeslib.as_array(self._h.contents.m, shape=(self.k + self.m, self.k))

    def code(self):
        """The batched code behind this handle (qfec_rs_code): the handle's current matrices."""
        return Code(lib().qfec_rs_code(self._h), owner=False)

    @staticmethod
    def _ptrs(data, parity):
        G, k, pitch = data.shape
        m = parity.shape[1]
        db, pb = data.ctypes.data, parity.ctypes.data
        return (C.c_void_p * (G * (k + m)))(*([db + i * pitch for i in range(G * k)] +
                                               [pb + i * pitch for i in range(G * m)]))

    def encode(self, data, parity, block_size):
        """data [G,k,pitch], parity [G,m,pitch] host uint8 arrays (parity written)."""
        G = data.shape[0]
        return lib().reed_solomon_encode(self._h, self._ptrs(data, parity), G * (self.k + self.m), block_size)

    def reconstruct(self, data, parity, marks, block_size):
        G = data.shape[0]
        marks = np.ascontiguousarray(marks, dtype=np.uint8)
        return lib().reed_solomon_reconstruct(self._h, self._ptrs(data, parity), C.c_void_p(marks.ctypes.data),
                                              G * (self.k + self.m), block_size)


_PACK_OUT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_char), C.c_uint)
_UNPACK_OUT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_char), C.c_uint, C.c_uint)


class NetFec:
    """Batched NetFecCodec layer (include/qfec_net.h): sessions keep zfec_pack_input's
    numbering; complete groups of all sessions go out in one device launch per flush, and
    received groups come back the same way.  Callbacks get (session, bytes[, src index])."""

    def __init__(self, k, n, max_pkt_size=2048, checksum=True):
        self._h = lib().qfec_net_new(k, n, max_pkt_size, int(bool(checksum)))
        if not self._h:
            raise QfecError(f"qfec_net_new({k}, {n}, {max_pkt_size}) failed")
        self.k, self.n = k, n

    def close(self):
        if self._h:
            lib().qfec_net_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def session(self):
        """A new session; its id is also its callback peer (id + 1)."""
        self._nsess = getattr(self, "_nsess", 0)
        s = lib().qfec_net_session(self._h, C.c_void_p(self._nsess + 1))
        check(min(s, 0), "qfec_net_session")
        self._nsess += 1
        return s

    def enable(self, session, on=True):
        """enable_zfec: with FEC off a session's packets go out as [0x13][payload]."""
        check(lib().qfec_net_enable(self._h, session, int(bool(on))), "qfec_net_enable")

    def pack_input(self, session, data):
        b = bytes(data)
        check(lib().qfec_net_pack_input(self._h, session, b, len(b)), "qfec_net_pack_input")

    def flush_pack(self, stream=None):
        """-> [(session, datagram bytes)] in emission order (each session's in sent order)."""
        out = []

        def cb(peer, p, size):
            out.append((int(peer) - 1, C.string_at(p, size)))
            return 0

        f = _PACK_OUT(cb)
        rc = lib().qfec_net_flush_pack(self._h, f, _stream_handle(stream))
        check(min(rc, 0), "qfec_net_flush_pack")
        return out

    def unpack_input(self, session, datagram):
        b = bytes(datagram)
        rc = lib().qfec_net_unpack_input(self._h, session, b, len(b))
        check(min(rc, 0), "qfec_net_unpack_input")
        return rc

    def flush_unpack(self, all_groups=False, stream=None):
        """-> [(session, payload bytes, src index)] delivered, group by group in source order."""
        out = []

        def cb(peer, p, size, src):
            out.append((int(peer) - 1, C.string_at(p, size), src))
            return 0

        f = _UNPACK_OUT(cb)
        rc = lib().qfec_net_flush_unpack(self._h, f, int(bool(all_groups)), _stream_handle(stream))
        check(min(rc, 0), "qfec_net_flush_unpack")
        return out

    def stats(self):
        a = (C.c_longlong * 8)()
        check(lib().qfec_net_stats(self._h, a), "qfec_net_stats")
        keys = ["groups_packed", "datagrams_out", "groups_unpacked", "delivered", "recovered", "undecodable",
                "foreign", "late"]
        return dict(zip(keys, list(a)))


class Zfec:
    """The exact NetFecCodec layer (include/qfec_zfec.h): per-session calls are queued in call
    order and flush() runs them through the reference's zfec_pack_input / zfec_unpack_input
    state machines, all byte work in batched device launches.  flush() returns
    (datagrams, deliveries): [(session, bytes)] and [(session, payload, src index)], each
    session's in the order the reference's PackOutput / UnpackOutput would have seen them."""

    def __init__(self, _lib=None):
        self._L = _lib or lib()  # (_lib: another build of the layer, for the CPU suite)
        self._h = self._L.qfec_zfec_new()
        if not self._h:
            raise QfecError("qfec_zfec_new failed")
        self._nsess = 0

    def close(self):
        if self._h:
            self._L.qfec_zfec_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def session(self, max_pkt_size=2048, buf_items=48, kmax=10, k=4, n=5, enabled=True, is_sorted=False):
        """FecTransmission::Init (CreateFecTransmission's defaults); the callback peer is id + 1."""
        s = self._L.qfec_zfec_session(self._h, C.c_void_p(self._nsess + 1), max_pkt_size, buf_items, kmax, k, n,
                                    int(bool(enabled)), int(bool(is_sorted)))
        check(min(s, 0), "qfec_zfec_session")
        self._nsess += 1
        return s

    def set_kn(self, session, k, n, add_new=True):
        rc = self._L.qfec_zfec_set_kn(self._h, session, k, n, int(bool(add_new)))
        check(rc, f"qfec_zfec_set_kn({k}, {n})")

    def enable(self, session, on=True):
        check(self._L.qfec_zfec_enable(self._h, session, int(bool(on))), "qfec_zfec_enable")

    def sorted(self, session, on=True):
        check(self._L.qfec_zfec_sorted(self._h, session, int(bool(on))), "qfec_zfec_sorted")

    def dynkn(self, session, on=True):
        check(self._L.qfec_zfec_dynkn(self._h, session, int(bool(on))), "qfec_zfec_dynkn")

    def lost_rate(self, session, rate):
        check(self._L.qfec_zfec_lost_rate(self._h, session, float(rate)), "qfec_zfec_lost_rate")

    def pack_input(self, session, data):
        b = bytes(data)
        check(self._L.qfec_zfec_pack_input(self._h, session, b, len(b)), "qfec_zfec_pack_input")

    def unpack_input(self, session, datagram):
        b = bytes(datagram)
        check(self._L.qfec_zfec_unpack_input(self._h, session, b, len(b)), "qfec_zfec_unpack_input")

    def flush(self, stream=None):
        sent, got = [], []

        def pcb(peer, p, size):
            sent.append((int(peer) - 1, C.string_at(p, size)))
            return 0

        def ucb(peer, p, size, src):
            got.append((int(peer) - 1, C.string_at(p, size), src))
            return 0

        f, g = _PACK_OUT(pcb), _UNPACK_OUT(ucb)
        rc = self._L.qfec_zfec_flush(self._h, f, g, _stream_handle(stream))
        check(min(rc, 0), "qfec_zfec_flush")
        return sent, got

    def stats(self, session):
        a = (C.c_longlong * 8)()
        check(self._L.qfec_zfec_stats(self._h, session, a), "qfec_zfec_stats")
        keys = ["fec_src_count", "fec_restore_count", "i_sent_pkt", "i_recv_pkt", "i_expected_packet", "k", "n",
                "undefined"]
        return dict(zip(keys, list(a)))


def _host_ptr(a, what):
    """Address of a contiguous uint8 host buffer (numpy array or CPU tensor)."""
    if isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"] or a.dtype != np.uint8:
            raise QfecError(f"{what}: contiguous uint8 host array required")
        return C.c_void_p(a.ctypes.data)
    import torch
    if a.is_cuda or not a.is_contiguous() or a.dtype != torch.uint8:
        raise QfecError(f"{what}: contiguous uint8 host tensor required")
    return C.c_void_p(a.data_ptr())


class Pipe:
    """include/qfec.h qfec_pipe: batches streamed host -> device -> host over `streams` HIP
    streams per device on `devices` (None: every visible device), each stream slot holding
    `slot_bytes` of device staging.  encode / reconstruct queue a batch and return; wait()
    blocks until every queued batch is done and returns the under-determined group count.
    Buffers must be PINNED host memory (torch .pin_memory() tensors or hipHostMalloc'd) and
    are kept referenced here until wait()."""

    def __init__(self, devices=None, streams=3, slot_bytes=96 << 20):
        devs = list(devices) if devices else []
        arr = (C.c_int * len(devs))(*devs) if devs else None
        h = lib().qfec_pipe_new(arr, len(devs), streams, slot_bytes)
        if not h:
            raise QfecError(f"qfec_pipe_new: {lib().qfec_last_error().decode()}")
        self._h = C.c_void_p(h)
        self.slots = lib().qfec_pipe_slots(self._h)
        self._held = []

    def close(self):
        if self._h:
            lib().qfec_pipe_free(self._h)
            self._h = None
            self._held = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode(self, code, data, parity, block_size=None):
        G, k, pitch = data.shape
        if k != code.k or tuple(parity.shape) != (G, code.m, pitch):
            raise QfecError("pipe encode: shape mismatch")
        block_size = pitch if block_size is None else block_size
        check(lib().qfec_pipe_encode(self._h, code._h, _host_ptr(data, "data"), _host_ptr(parity, "parity"), G,
                                     block_size, pitch), "qfec_pipe_encode")
        self._held += [code, data, parity]

    def reconstruct(self, code, data, parity, marks, block_size=None):
        G, k, pitch = data.shape
        nmarks = marks.size if isinstance(marks, np.ndarray) else marks.numel()
        if k != code.k or tuple(parity.shape) != (G, code.m, pitch) or nmarks != G * (code.k + code.m):
            raise QfecError("pipe reconstruct: shape mismatch")
        block_size = pitch if block_size is None else block_size
        check(lib().qfec_pipe_reconstruct(self._h, code._h, _host_ptr(data, "data"), _host_ptr(parity, "parity"),
                                          _host_ptr(marks, "marks"), G, block_size, pitch), "qfec_pipe_reconstruct")
        self._held += [code, data, parity, marks]

    def wait(self):
        nf = C.c_longlong(0)
        rc = lib().qfec_pipe_wait(self._h, C.byref(nf))
        self._held = []
        check(rc, "qfec_pipe_wait")
        return int(nf.value)
