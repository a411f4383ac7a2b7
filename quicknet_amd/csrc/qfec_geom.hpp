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
