// qfec_geom.hpp -- launch geometry of the batched device API: how a row of block_size bytes is cut
// into lanes, and how a batch is cut into launches.  Header-only plain C++ (no HIP), so the CPU
// suite can hold the rules to shapes no GPU test reaches (tests/test_geom_host.py).
//
// Two mappings exist.  Flat (encode, verify, locate): one lane per 16-byte column, or per byte when
// the layout is not 16-B aligned, (group, column) flattened over the grid.  8-byte lanes
// (reconstruct, repair, locate_erased): a wave covers 64 8-byte columns of one group, wpg8 waves
// per group.  qfec_update has whole waves per group too, on 16-B columns (WaveGeom); the range form
// qfec_encode_update is flat; the pointer-table calls have whole waves per group as well (PtrsGeom).
// In all of them no launch has more than 2^31 - 1 lanes; a larger batch goes in several
// launches over consecutive groups (for_group_chunks).
#pragma once

#include <stdint.h>

#include <algorithm>

namespace qfec {

constexpr long long kMaxLaunchLanes = 0x7FFFFFFFll;

// 16-byte columns need both bases and the pitch 16-B aligned and the last column inside the pitch
inline bool vec16_ok(const void* a, const void* b, int block, long long pitch) {
    return ((uintptr_t)a % 16 == 0) && ((uintptr_t)b % 16 == 0) && (pitch % 16 == 0) &&
           ((long long)block + 15) / 16 * 16 <= pitch;
}

struct FlatGeom {
    bool vec16;
    uint32_t cols;  // lanes per row: 16-B columns (vec16) or bytes; also what make_div_magic takes
    long long per;  // groups per launch
};

// dgs, pgs: bytes between groups of the data and of the parity buffer
inline FlatGeom flat_geom(const void* data, const void* parity, int block, long long pitch, uint64_t dgs,
                          uint64_t pgs) {
    FlatGeom f;
    f.vec16 = vec16_ok(data, parity, block, pitch) && !((dgs | pgs) & 15);
    f.cols = f.vec16 ? (uint32_t)((block + 15) / 16) : (uint32_t)block;
    f.per = std::max<long long>(1, kMaxLaunchLanes / f.cols);
    return f;
}

struct Lane8Geom {
    uint32_t cols8, wpg8;  // 8-B columns per row, waves per group at 64 of them per wave
    long long per;         // groups per launch
};

inline Lane8Geom lane8_geom(const FlatGeom& f, int k, int block) {
    Lane8Geom g;
    // For k < 14 cover the 16-B columns' span, which the 16-B body writes anyway (it stays inside
    // the pitch): a row that ends part-way into a 64-B line costs a partial-line write
    // (B = 1400: 175 -> 176 8-B columns, rows end on 1408 = 22 lines).  It also reads the
    // extra 8 B of every survivor, and with k = 16 survivors per row written that costs
    // more than it saves: RS(16,4) B=1400 5 404 GB/s full against 5 508 partial, RS(10,3)
    // B=1024 6 009 against 5 949 (reconstruct, interleaved A/B, profiles/r03_recon/r03k_ab.txt)
    g.cols8 = f.vec16 && k < 14 ? 2u * f.cols : (uint32_t)((block + 7) / 8);
    g.wpg8 = (g.cols8 + 63) / 64;
    g.per = std::max<long long>(1, kMaxLaunchLanes / (64ll * std::max(g.wpg8, 1u)));
    return g;
}

// qfec_update on 16-B-aligned layouts: the flat mapping's 16-B columns, but whole waves per group
// (the shard a group replaces, and so its tables, are wave-uniform)
struct WaveGeom {
    uint32_t cols, wpg;  // 16-B columns per row, waves per group at 64 of them per wave
    long long per;       // groups per launch
};

inline WaveGeom wave_geom(const FlatGeom& f) {
    WaveGeom w;
    w.cols = f.cols;
    w.wpg = (w.cols + 63) / 64;
    w.per = std::max<long long>(1, kMaxLaunchLanes / (64ll * std::max(w.wpg, 1u)));
    return w;
}

// The pointer-table calls (qfec_encode_ptrs, qfec_reconstruct_ptrs): a shard is exactly `block`
// bytes with nothing usable after it.  A wave covers 64 columns of lane_bytes (16 or 8) of one group.
// The whole columns go to the vector body; the block % lane_bytes bytes after them go byte by byte
// to the first lanes of the group's last wave, which always exists: wpg counts the part column.
// A group whose pointers are not all 16-B aligned runs the same waves over the same spans byte by byte.
struct PtrsGeom {
    uint32_t vcols, wpg;    // whole columns per shard; waves per group
    uint32_t tail0, tailn;  // first byte and count of the tail (tailn < lane_bytes; tail0 + tailn = block)
    long long per;          // groups per launch
};

// 16-B lanes, except the reconstruct of k >= 10 on 8-B lanes, where the contiguous reconstruct's
// auto body runs them too (its 16-B body holds k inputs of four registers each: 4 waves per SIMD)
inline int ptrs_lane_bytes(bool reconstruct, int k) { return reconstruct && k >= 10 ? 8 : 16; }

inline PtrsGeom ptrs_geom(int block, int lane_bytes) {
    PtrsGeom p;
    p.vcols = (uint32_t)(block / lane_bytes);
    p.tail0 = p.vcols * (uint32_t)lane_bytes;
    p.tailn = (uint32_t)block - p.tail0;
    p.wpg = (p.vcols + (p.tailn ? 1u : 0u) + 63) / 64;
    p.per = std::max<long long>(1, kMaxLaunchLanes / (64ll * std::max(p.wpg, 1u)));
    return p;
}

// The pointer-table calls with per-shard lengths (qfec_encode_ptrs_var, qfec_reconstruct_ptrs_var):
// the launch has ptrs_geom(max_len, lane_bytes).wpg waves per group, and every group cuts its own
// length L <= max_len inside the kernel by this rule, which the host can call as well
// (tests/test_ptrs_var_host.py).  Waves [0, live) of the group have work; a wave whose slab starts
// at or past L (slab >= live) leaves.  The whole columns go to the vector body, the L % lane_bytes
// bytes after them byte by byte to the first lanes of wave live - 1.  L = 0: no live wave.
#ifdef __HIPCC__
#define QFEC_GEOM_HD __host__ __device__
#else
#define QFEC_GEOM_HD
#endif
struct PtrsVarGeom {
    uint32_t live;          // waves of the group with work: ceil(L / (64 * lane_bytes))
    uint32_t vcols;         // whole columns
    uint32_t tail0, tailn;  // first byte and count of the tail (tailn < lane_bytes; tail0 + tailn = L)
};

QFEC_GEOM_HD inline PtrsVarGeom ptrs_var_geom(uint32_t len, uint32_t lane_bytes) {
    PtrsVarGeom v;
    v.vcols = len / lane_bytes;
    v.tail0 = v.vcols * lane_bytes;
    v.tailn = len - v.tail0;
    v.live = (v.vcols + (v.tailn ? 1u : 0u) + 63u) / 64u;
    return v;
}

// The datagram / frame send (qfec_pack_datagrams, qfec_pack_frames; kernels in qfec_wire.hip): which
// kernels a call takes.  `row_pitch` is the wire pitch, or the frame pitch with a frame prefix (4, or
// 12 with the Session words); `instance`: a compile-time (k, m) exists and the fused send is on.
//   line          the row pitch is the 64-B multiple just above the longest row (prefix + header +
//                 shard pitch) and holds at least 20 chunks of 16 B (16 without checksums): every 64-B
//                 line of a row is then stored whole, zeros past the datagram
//   one wave per group (checksums on, line): 1088 B one pass of 16-B lanes; 576 B two groups per wave;
//                 1104..1600 B three passes of 8-B lanes; frames only, 1664..2112 B: two passes of 16-B lanes
//   body forms    flat over (group, chunk), lpg lanes per group covering chunks [ts, tn); with
//                 checksums a second launch writes line 0 (line) or chunk 0 and byte 16 (k_pack_head),
//                 from the 16-lane partial sums the body leaves in d_shards
//   frames        take one wave per group or the two calls, never a body form
enum SendKind {
    kSendStaged = 0,  // build -> encode -> emit
    kSendWave1,
    kSendWave2,
    kSendWave8x3,
    kSendWave16x2,
    kSendBodyLine0,
    kSendBodyHead,
    kSendBody11Line,
    kSendBody11,
    kSendTwoCall,  // frames: qfec_pack_datagrams into scratch, then qfec_frame_udp
};

struct SendForm {
    int kind;
    bool line;
    uint32_t gpw;        // one wave per group: groups per wave (else 0)
    uint32_t ts, tn;     // body forms: chunks [ts, tn) of a row (else 0)
    uint32_t lpg;        // body forms: lanes per group, at least 16 (else 0)
    uint32_t rec_words;  // u32 per 16-lane row of the body that it writes into d_shards (0: none)
    uint64_t per;        // groups per launch (pair); a multiple of 16 for the body forms, so that
                         // g0 * lpg % 16 == 0 and a launch's first 16-lane row is a whole one
};

inline int send_wave_kind(uint64_t row_pitch) {
    // above 1088 B: 8-B lanes in three passes (1472 B, RS(10,13) x 100k: 737 against 781 us for
    // the body + line-0 pair); at 1088 B 16-B lanes, one pass (497 against 545 us on 8-B lanes).
    // (16-B lanes in two passes above 1088 B, a retired A/B, ran 841 us against 782 for the body +
    // line-0 pair at 1472 B: profiles/r03_wire/r03n_mtu_ab.txt)
    if (row_pitch > 1088 && row_pitch <= 1600) return kSendWave8x3;
    if (row_pitch == 576) return kSendWave2;
    if (row_pitch == 1088) return kSendWave1;
    return kSendStaged;
}

inline SendForm send_form(bool instance, int n, int checksum, uint64_t pitch, uint64_t row_pitch, int prefix) {
    SendForm f{};
    f.per = 1;
    if (prefix) {
        // frames above 1088 B take the two-pass wave whenever the one-wave send is on: the other way
        // is two calls (datagrams, then frames), 1 577 against 851 us at 1472 B (r03n)
        int w = send_wave_kind(row_pitch);
        if (!w && row_pitch > 1088 && row_pitch <= 2112) w = kSendWave16x2;
        f.kind = kSendTwoCall;
        if (!instance || !checksum || !w || row_pitch != ((uint64_t)prefix + 13 + pitch + 63) / 64 * 64) return f;
        f.kind = w;
    } else {
        if (!instance) return f;
        const uint64_t hdr = checksum ? 13 : 11;
        f.line = row_pitch % 64 == 0 && row_pitch == (hdr + pitch + 63) / 64 * 64 && row_pitch / 16 >= (checksum ? 20u : 16u);
        const int w = send_wave_kind(row_pitch);
        if (checksum && f.line && w) {
            f.kind = w;
        } else {
            f.kind = checksum ? (f.line ? kSendBodyLine0 : kSendBodyHead) : (f.line ? kSendBody11Line : kSendBody11);
            // body lanes per group cover chunks [ts, tn): the longest datagram the shard pitch allows,
            // or with `line` every chunk up to the pitch; chunk 0 (line: chunks 0-3) is the second launch's
            f.ts = checksum ? (f.line ? 4u : 1u) : 0u;
            f.tn = f.line ? (uint32_t)(row_pitch / 16) : (uint32_t)((hdr + pitch + 15) / 16);
            f.lpg = std::max(16u, f.tn - f.ts);
            f.rec_words = checksum ? 2u * (uint32_t)((n + 1) / 2) : 0u;
            f.per = std::max<uint64_t>((((uint64_t)1 << 30) / f.lpg) & ~(uint64_t)15, 16);
            return f;
        }
    }
    f.line = true;
    f.gpw = f.kind == kSendWave2 ? 2u : 1u;
    f.per = (uint64_t)1 << 28;
    return f;
}

// u32 words of d_shards the body of a checksummed body form writes for a batch of `groups`: groups lie
// back to back in the flat lane space, one record of rec_words per 16-lane row (its first group's sums,
// then its last group's).  Never more than the groups * n * pitch bytes d_shards has: rec_words <= n + 1
// u32 per 16 lanes, lpg <= pitch / 16 + 2 and pitch >= 16 (tests/test_tx_model.py walks every pitch).
inline uint64_t send_part_words(const SendForm& f, uint64_t groups) {
    return (groups * f.lpg + 15) / 16 * f.rec_words;
}

// fn(g0, gn) once per launch, over [g0, g0 + gn) ascending; stops at the first non-zero return
template <class F>
inline int for_group_chunks(long long groups, long long per, F&& fn) {
    for (long long g0 = 0; g0 < groups; g0 += per) {
        const int rc = fn(g0, std::min(per, groups - g0));
        if (rc) return rc;
    }
    return 0;
}

}  // namespace qfec
