// qfec_ptrs_device.hpp -- what the kernels on tables of shard addresses share (qfec_ptrs.hip: encode,
// reconstruct; qfec_ptrs_var.hip: the same with per-shard lengths; qfec_plan.hip: k_plan_apply_ptrs,
// k_plan_apply_ptrs_var; qfec_check.hip: k_check_apply_ptrs, k_check_apply_ptrs_var): reading an address out of the lane that loaded it, saying that it is global
// memory, a wave's share of its group's shards, the encode's vector body on row addresses, and for
// the kernels with per-shard lengths a lane's length, the clipped column load and a wave's share of
// a group that has its own length, the ragged column loads of the templated bodies, and for the integrity
// kernels (qfec_integrity_ptrs.hip, qfec_integrity_ptrs_var.hip) the syndromes of a byte and of a column
// on row addresses.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "qfec_device.hpp"
#include "qfec_geom.hpp"

namespace qfec {

// v of lane l; l is wave-uniform
__device__ __forceinline__ uint64_t lane_value(uint64_t v, uint32_t l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
    return ((uint64_t)hi << 32) | lo;
}

// a table entry is an address in global memory: said so, the accesses are global_load / global_store
// and not the flat forms an address of unknown kind gets
typedef __attribute__((address_space(1))) uint8_t global_u8;
__device__ __forceinline__ const uint8_t* as_row(uint64_t p) { return (const uint8_t*)reinterpret_cast<const global_u8*>(p); }
__device__ __forceinline__ uint8_t* as_out(uint64_t p) { return (uint8_t*)reinterpret_cast<global_u8*>(p); }

// recon_column_by_e's row addresses: lane s of the wave holds the address of shard s
struct LaneRows {
    uint64_t mine;
    __device__ __forceinline__ uint8_t* operator()(uint8_t*, uint32_t l) const { return as_out(lane_value(mine, l)); }
};

// A wave's share of its group's shards.  vec(off): the lane's whole column of W bytes at byte off;
// byte(b): byte b.  Every access lies inside [0, block): a column ends at vcols * W <= block, the
// tail at tail0 + tailn = block, the byte span at min(slab end, block); the wpg slabs reach block.
// Args: PtrsArgs or PlanPtrsArgs (block, vcols, wpg, tail0, tailn of PtrsGeom).
template <int W, class Args, class Vec, class Byte>
__device__ __forceinline__ void run_slab(const Args& a, uint32_t slab, int lane, bool aligned, Vec&& vec,
                                         Byte&& byte) {
    if (aligned) {
        const uint32_t col = slab * 64u + lane;
        if (col < a.vcols) vec((uint64_t)col * W);
        if (slab + 1 == a.wpg && (uint32_t)lane < a.tailn) byte((uint64_t)a.tail0 + lane);
    } else {
        const uint32_t end = std::min((slab + 1) * 64u * W, a.block);
#pragma unroll 1
        for (uint32_t b = slab * 64u * W + lane; b < end; b += 64) byte((uint64_t)b);
    }
}

// the wave's group and slab; false past the last group
template <class Args>
__device__ __forceinline__ bool wave_item(const Args& a, uint64_t* g, uint32_t* slab) {
    const uint32_t wid = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    *g = wid / a.wpg;
    *slab = wid - (uint32_t)*g * a.wpg;
    return *g < a.groups;
}

// the M parity columns at byte `off` from the K data columns there.  For K >= 16 the inputs come in
// two halves, as in k_encode_perm_halves: half the input registers live at a time.
template <int K, int M>
__device__ __forceinline__ void encode_column(const uint8_t* const (&src)[K], uint8_t* const (&dst)[M],
                                              const uint32_t* tab, uint64_t off) {
    uint4 acc[M];
#pragma unroll
    for (int r = 0; r < M; ++r) {
        acc[r] = make_uint4(0, 0, 0, 0);
        if (tab[(r * K) * QFEC_TAB_STRIDE + 5]) acc[r] = *reinterpret_cast<const uint4*>(dst[r] + off);  // rs.c column-0 quirk
    }
    if constexpr (K >= 16) {
        constexpr int H = (K + 1) / 2;
        {
            uint4 x[H];
#pragma unroll
            for (int c = 0; c < H; ++c) x[c] = ld16(src[c] + off);
            enc_mac16<K, M, 0, H>(acc, x, tab);
        }
        __builtin_amdgcn_sched_barrier(0);  // the second half's loads stay below the first half's multiply
        {
            uint4 x[K - H];
#pragma unroll
            for (int c = 0; c < K - H; ++c) x[c] = ld16(src[H + c] + off);
            enc_mac16<K, M, H, K - H>(acc, x, tab);
        }
    } else {
        uint4 x[K];
#pragma unroll
        for (int c = 0; c < K; ++c) x[c] = ld16(src[c] + off);
        enc_mac16<K, M, 0, K>(acc, x, tab);
    }
#pragma unroll
    for (int r = 0; r < M; ++r) st16(dst[r] + off, acc[r]);
}

// ---------------------------------------------------------------- per-shard lengths
// shared by qfec_ptrs_var.hip and k_plan_apply_ptrs_var of qfec_plan.hip

// v of lane l; l is wave-uniform
__device__ __forceinline__ uint32_t lane_value32(uint32_t v, uint32_t l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l);
}

// register s >> 6 of the lane s & 63: entry s of the group's table (s wave-uniform, below 64 * NP);
// k_plan_apply_ptrs_var of qfec_plan.hip, k_check_apply_ptrs and k_check_apply_ptrs_var of qfec_check.hip
template <int NP>
__device__ __forceinline__ uint64_t entry_of(const uint64_t (&p)[NP], uint32_t s) {
    const uint32_t l = s & 63u, r = s >> 6;
    if constexpr (NP == 1) return lane_value(p[0], l);
    else if constexpr (NP == 2) return r == 0 ? lane_value(p[0], l) : lane_value(p[1], l);
    else
        return r == 0 ? lane_value(p[0], l) : r == 1 ? lane_value(p[1], l) : r == 2 ? lane_value(p[2], l) : lane_value(p[3], l);
}
template <int NP>
__device__ __forceinline__ uint32_t entry_of(const uint32_t (&v)[NP], uint32_t s) {
    const uint32_t l = s & 63u, r = s >> 6;
    if constexpr (NP == 1) return lane_value32(v[0], l);
    else if constexpr (NP == 2) return r == 0 ? lane_value32(v[0], l) : lane_value32(v[1], l);
    else
        return r == 0   ? lane_value32(v[0], l)
               : r == 1 ? lane_value32(v[1], l)
               : r == 2 ? lane_value32(v[2], l)
                        : lane_value32(v[3], l);
}

// the first n < 4 D bytes at q, zero after them: a piece of 8, 4, 2 and 1 bytes per set bit of n, each
// at the offset the larger pieces leave, which its own size divides (q is 4 D-aligned: the group is
// aligned).  Never a byte at or past n.
template <int D>
__device__ __forceinline__ void ldv_part(uint32_t (&v)[D], const uint8_t* q, uint32_t n) {
    static_assert(D == 4 || D == 2, "16-B or 8-B lanes");
    constexpr uint32_t W = 4u * D;
    uint64_t lo = 0, hi = 0;
    if constexpr (D == 4) {
        if (n & 8u) lo = *reinterpret_cast<const uint64_t*>(q);
    }
    if (n & 4u) {
        const uint32_t p = n & (W - 1u) & 8u;
        const uint64_t w = *reinterpret_cast<const uint32_t*>(q + p);
        if (p) hi |= w;
        else lo |= w;
    }
    if (n & 2u) {
        const uint32_t p = n & (W - 1u) & 12u;
        const uint64_t w = (uint64_t)*reinterpret_cast<const uint16_t*>(q + p) << (8u * (p & 7u));
        if (p & 8u) hi |= w;
        else lo |= w;
    }
    if (n & 1u) {
        const uint32_t p = n & (W - 1u) & 14u;
        const uint64_t w = (uint64_t)q[p] << (8u * (p & 7u));
        if (p & 8u) hi |= w;
        else lo |= w;
    }
    v[0] = (uint32_t)lo;
    v[1] = (uint32_t)(lo >> 32);
    if constexpr (D == 4) {
        v[2] = (uint32_t)hi;
        v[3] = (uint32_t)(hi >> 32);
    }
}

// D dwords of a row of `len` bytes at byte `off`, zero past len.  The whole column: ldv.  Nothing
// of it: no load.  Part of it: ldv_part.  One branch per source: the form of the runtime-k,m kernels.
template <int D>
__device__ __forceinline__ void ldv_clip(uint32_t (&v)[D], const uint8_t* row, uint32_t off, uint32_t len) {
    if (off + 4u * D <= len) ldv<D>(v, row + off);
    else ldv_part<D>(v, row + off, len > off ? len - off : 0u);
}

// A wave's share of a group of length len.  vec(off): the lane's whole column of W bytes at byte
// off; byte(b): byte b.  Every access lies inside [0, len): a column ends at vcols * W <= len, the
// tail at tail0 + tailn = len, the byte span at min(slab end, len).  The caller has left already
// when slab >= live.
template <int W, class Vec, class Byte>
__device__ __forceinline__ void run_slab_var(const PtrsVarGeom& v, uint32_t len, uint32_t slab, int lane, bool aligned,
                                             Vec&& vec, Byte&& byte) {
    if (aligned) {
        const uint32_t col = slab * 64u + lane;
        if (col < v.vcols) vec(col * (uint32_t)W);
        if (slab + 1 == v.live && (uint32_t)lane < v.tailn) byte(v.tail0 + lane);
    } else {
        const uint32_t end = std::min((slab + 1) * 64u * W, len);
#pragma unroll 1
        for (uint32_t b = slab * 64u * W + lane; b < end; b += 64) byte(b);
    }
}

// how far the whole columns of a wave reach: a source at least this long is read by vector loads only
template <int W>
__device__ __forceinline__ uint32_t slab_reach(const PtrsVarGeom& v, uint32_t slab) {
    return std::min((slab + 1) * 64u * W, v.tail0);
}

// ---------------------------------------------------------------- ragged columns
// (qfec_ptrs_var.hip, qfec_integrity_ptrs_var.hip: the templated bodies of a wave that is not `full`)

// ldv_clip of qfec_ptrs_device.hpp for the templated bodies, without a branch per source.  A lane whose column is not whole
// in this row loads the column of `safe` instead, a row of the group that is whole wherever a lane
// works (the group's longest data shard, a parity survivor), and drops it: the loads issue together
// as in the fixed-length body and no byte at or past len is read.  The row's part column was loaded
// before the lanes parted, by the lane that holds the row's address and length (lane_part), so the
// part columns of all rows cost the wave one round trip, at the same time as the whole columns; the
// lane whose column it is takes it from lane s with readlane.
template <int D>
__device__ __forceinline__ void ldv_ragged(uint32_t (&v)[D], const uint8_t* row, const uint8_t* safe, uint32_t off,
                                           uint32_t len, const uint32_t (&part)[D], uint32_t s) {
    constexpr uint32_t W = 4u * D;
    const bool whole = off + W <= len;
    ldv<D>(v, (whole ? row : safe) + off);
    const bool mine = len % W != 0 && off == len / W * W;
#pragma unroll
    for (int d = 0; d < D; ++d) v[d] = mine ? lane_value32(part[d], s) : whole ? v[d] : 0u;
}

// Every lane of a ragged wave calls it before the first lane-dependent branch.  source: the lane
// holds the address p and the readable length len of a row the wave reads.  A lane whose row's part
// column lies in this slab loads it: bytes [len / W * W, len) of the row, zero after them.
template <int D>
__device__ __forceinline__ void lane_part(uint32_t (&part)[D], bool source, uint64_t p, uint32_t len, uint32_t slab) {
    constexpr uint32_t W = 4u * D;
#pragma unroll
    for (int d = 0; d < D; ++d) part[d] = 0;
    const uint32_t pc = len / W, pn = len % W;
    if (source && pn && (pc >> 6) == slab) ldv_part<D>(part, as_row(p) + pc * W, pn);
}

__device__ __forceinline__ uint4 ld16_clip(const uint8_t* row, uint32_t off, uint32_t len) {
    uint32_t v[4];
    ldv_clip<4>(v, row, off, len);
    return make_uint4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ uint4 ld16_ragged(const uint8_t* row, const uint8_t* safe, uint32_t off, uint32_t len,
                                             const uint32_t (&part)[4], uint32_t s) {
    uint32_t v[4];
    ldv_ragged<4>(v, row, safe, off, len, part, s);
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// Sources per pass of the ragged column bodies: the largest divisor of K up to CAP.  The ragged bodies
// are loops rolled over the sources in such chunks, not the unrolled bodies of the fixed-length
// kernels: a kernel's registers are those of its larger path, and unrolled next to the full path the
// ragged encode of RS(16,4) holds 238 VGPRs (2 waves per SIMD) and the ragged reconstruct 101 (4 waves),
// where the full paths alone hold 93 and 94.
template <int K, int CAP>
constexpr int ragged_chunk() {
    int best = 1;
    for (int d = 2; d <= CAP && d <= K; ++d)
        if (K % d == 0) best = d;
    return best;
}

// ---------------------------------------------------------------- syndromes on row addresses
// (qfec_integrity_ptrs.hip, qfec_integrity_ptrs_var.hip)

__device__ __forceinline__ void xor16(uint4& a, const uint4& b) {
    a.x ^= b.x;
    a.y ^= b.y;
    a.z ^= b.z;
    a.w ^= b.w;
}

// Byte b of the group: its m syndromes s_r = parity_r ^ sum_c P[r][c] x data_c, row(s) = the address
// of shard s.  The non-zero rows are OR-ed into `bad`.  LOC: a data shard i stays in `cand` while
// s_r == r_{r,i} x s_0 holds in every row r >= 1 tested; rows are tested from the byte's first
// non-zero syndrome on (a row skipped before it is zero beside a zero s_0, which every candidate
// explains).  K > 0 (k == K): the K input bytes are loaded at once, as in encode_byte; the rows stay
// a rolled loop.
template <int K, bool LOC, class Row>
__device__ __forceinline__ void check_byte(int k, int m, const uint32_t* tab, const uint32_t* rtab, const Row& row,
                                           uint64_t b, uint32_t& bad, uint32_t& cand) {
    uint32_t x[K > 0 ? K : 1];
    if constexpr (K > 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) x[c] = as_row(row(c))[b];
    }
    uint32_t here = 0;
    Sel s0 = gf_sel(0u);
#pragma unroll 1
    for (int r = 0; r < m; ++r) {
        const uint32_t* tr = tab + (r * k) * QFEC_TAB_STRIDE;
        uint32_t s = as_row(row(k + r))[b];
        if constexpr (K > 0) {
#pragma unroll
            for (int c = 0; c < K; ++c) {
                const uint32_t* tc = tr + c * QFEC_TAB_STRIDE;
                s ^= gf_mul4(gf_sel(x[c]), tc[0], tc[1], tc[2], tc[3], tc[4]);
            }
        } else {
            for (int c = 0; c < k; ++c) {
                const uint32_t* tc = tr + c * QFEC_TAB_STRIDE;
                s ^= gf_mul4(gf_sel((uint32_t)as_row(row(c))[b]), tc[0], tc[1], tc[2], tc[3], tc[4]);
            }
        }
        s &= 0xFFu;
        if (s) here |= 1u << r;
        if constexpr (LOC) {
            if (r == 0) {
                s0 = gf_sel(s);
            } else if (here != 0) {
#pragma unroll 1
                for (int i = 0; i < k; ++i) {
                    const uint32_t* tc = rtab + (i * (m - 1) + r - 1) * QFEC_TAB_STRIDE;
                    if ((gf_mul4(s0, tc[0], tc[1], tc[2], tc[3], tc[4]) & 0xFFu) != s) cand &= ~(1u << i);
                }
            }
        }
    }
    bad |= here;
}

// the M syndromes of the whole column at byte `off`; p: the lanes' addresses.  Parity first, then
// the data (products16's comment has the register effect of that order); K >= 16 in two halves with
// encode_column's barrier.
template <int K, int M>
__device__ __forceinline__ void syndromes16(uint4 (&s)[M], uint64_t p, const uint32_t* tab, uint64_t off) {
    uint4 par[M];
#pragma unroll
    for (int r = 0; r < M; ++r) par[r] = ld16(as_row(lane_value(p, K + r)) + off);
#pragma unroll
    for (int r = 0; r < M; ++r) s[r] = make_uint4(0, 0, 0, 0);
    if constexpr (K >= 16) {
        constexpr int H = (K + 1) / 2;
        {
            uint4 x[H];
#pragma unroll
            for (int c = 0; c < H; ++c) x[c] = ld16(as_row(lane_value(p, c)) + off);
            enc_mac16<K, M, 0, H>(s, x, tab);
        }
        __builtin_amdgcn_sched_barrier(0);  // the second half's loads stay below the first half's multiply
        {
            uint4 x[K - H];
#pragma unroll
            for (int c = 0; c < K - H; ++c) x[c] = ld16(as_row(lane_value(p, H + c)) + off);
            enc_mac16<K, M, H, K - H>(s, x, tab);
        }
    } else {
        uint4 x[K];
#pragma unroll
        for (int c = 0; c < K; ++c) x[c] = ld16(as_row(lane_value(p, c)) + off);
        enc_mac16<K, M, 0, K>(s, x, tab);
    }
#pragma unroll
    for (int r = 0; r < M; ++r) xor16(s[r], par[r]);
}

// lane s < k + m: the address of shard s of group g; the rest zero
__device__ __forceinline__ uint64_t lane_row(const uint64_t* __restrict__ dptrs, const uint64_t* __restrict__ pptrs,
                                             uint64_t g, int k, int m, int lane) {
    uint64_t p = 0;
    if (lane < k) p = dptrs[g * (uint64_t)k + lane];
    else if (lane < k + m) p = pptrs[g * (uint64_t)m + (lane - k)];
    return p;
}

}  // namespace qfec
