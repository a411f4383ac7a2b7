// qfec_update_ptrs.hip -- incremental parity on shards scattered in device memory, for MI355X (gfx950):
// qfec_encode_update_ptrs / qfec_update_ptrs and their forms with per-shard lengths.  The arithmetic is
// that of qfec_update.hip -- parity_j ^= rows[j][i] x (old_i ^ new_i), true GF products from the
// encode's perm tables, the rs.c stale-row flag word never read -- and the table is that of
// qfec_encode_ptrs (qfec_ptrs.hip): every group's k data addresses, then every group's m parity
// addresses.
//
// Mapping: the pointer-table one for both forms -- one wave per (group, slab of 64 16-B columns), four
// waves per block, wpg waves per group from ptrs_geom(block_size or max_len, 16).  The flat mapping of
// k_encupd_perm does not carry over: a flat wave straddles groups and every lane would need its own
// addresses.
//
// Addresses: a lane loads the address (and, with lengths, the length) of ONE entry its group may
// dereference -- the range form: lanes [0, count) the data shards first .. first + count - 1, lanes
// [count, count + m) the parity shards; the per-group form: lane 0 the new row, lane 1 shard i, lanes
// [2, 2 + m) the parity shards -- and the wave reads them out with readlane.  Where those entries pass
// 64 the table is read at the point of use instead, as in k_encode_ptrs_any.  No other entry of the
// table is loaded, so it may hold anything: a sender fills the table as packets arrive.
//
// Tables stay scalar.  Range form: first .. first + count - 1 are launch-uniform, read through the
// constant address space.  Per-group form: the wave reads its id once with a scalar load, leaves
// before any other load when the id is < 0 or >= k, and then reads column i's m tables.
//
// Alignment is judged per group on the entries the group may dereference (not a part of length 0,
// not the new row of length 0): all of them 16-B aligned, the group runs 16-B lanes over its whole
// columns and the tail bytes byte by byte on the first lanes of its last live wave; any other group
// runs the same waves over the same spans byte by byte.
//
// With lengths (VAR) a group has an extent E that its waves cut with ptrs_var_geom -- range form: L
// when overwriting, the longest part of the range when accumulating; per-group form: max(o, n), or n
// in delta mode -- and nothing at or past E is read or written.  A wave whose whole columns lie below
// every length it reads runs the fixed-length column body unchanged; any other wave runs the clipped
// body, which never loads at or past a length (ld16_clip) and writes a column of the replaced shard
// that n cuts byte by byte.  The clipped body is the safe form, not a tuned one.  A group refused for a
// length or an id is counted once, by lane 0 of its first wave, through the block's sum
// (block_counts: every thread calls it, so no wave returns before it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "qfec_internal.hpp"
#include "qfec_device.hpp"
#include "qfec_geom.hpp"
#include "qfec_ptrs_device.hpp"

namespace qfec {

typedef const __attribute__((address_space(4))) int32_t* cptr_i32;

// the perm dwords of table entry `idx` (wave-uniform), read through the constant address space
__device__ __forceinline__ void tab5(uint32_t (&t)[5], const uint32_t* tab, int idx) {
    const cptr32 p = (cptr32)tab + idx * QFEC_TAB_STRIDE;
#pragma unroll
    for (int i = 0; i < 5; ++i) t[i] = p[i];
}

__device__ __forceinline__ uint32_t byte_product(uint32_t x, const uint32_t* tab, int idx) {
    uint32_t t[5];
    tab5(t, tab, idx);
    return gf_mul4(gf_sel(x), t[0], t[1], t[2], t[3], t[4]) & 0xFFu;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
    for (int o = 32; o; o >>= 1) x = std::max(x, (uint32_t)__shfl_xor((int)x, o));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
}

// the fixed-length kernels cut a group as the launch does
__device__ __forceinline__ PtrsVarGeom launch_geom(const UpdatePtrsArgs& a) {
    PtrsVarGeom v;
    v.live = a.wpg;
    v.vcols = a.vcols;
    v.tail0 = a.tail0;
    v.tailn = a.tailn;
    return v;
}

constexpr int UCH = 4;  // parity rows per pass of the runtime-m bodies, as in qfec_update.hip

// ------------------------------------------------------------------ range form

// acc[j] ^= sum_c rows[r0 + j][first + c] x column of part c at byte off, j < R (rows past m are left
// alone); the inputs two at a time, so two loads are in flight per lane.  ALL: every one of the R rows
// exists.  FULL: every part is whole in this column; else a part is loaded below its length only.
template <int R, bool ALL, bool FULL, class Row, class Len>
__device__ __forceinline__ void range_products(uint4 (&acc)[R], const UpdatePtrsArgs& a, const Row& row,
                                               const Len& len, uint32_t off, int r0) {
    const int k = a.k, m = a.m, first = a.first, count = a.count;
    const auto column = [&](int c) {
        if constexpr (FULL) return ld16(as_row(row(c)) + off);
        else return ld16_clip(as_row(row(c)), off, len(c));
    };
    int c = 0;
    for (; c + 1 < count; c += 2) {
        const uint4 xa = column(c);
        const uint4 xb = column(c + 1);
        Sel sa[4], sb[4];
        sel16(sa, xa);
        sel16(sb, xb);
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (ALL || r0 + j < m) {
                uint32_t ta[5], tb[5];
                tab5(ta, a.tab, (r0 + j) * k + first + c);
                tab5(tb, a.tab, (r0 + j) * k + first + c + 1);
                gf_mac16x2(acc[j], sa, sb, ta, tb);
            }
    }
    if (c < count) {
        Sel s[4];
        sel16(s, column(c));
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (ALL || r0 + j < m) {
                uint32_t t[5];
                tab5(t, a.tab, (r0 + j) * k + first + c);
                gf_mac16(acc[j], s, t);
            }
    }
}

// the 16-B column at byte off of the m parity shards; row(s): the address of part s < count or of
// parity shard s - count.  With accumulate the parity columns are loaded ahead of the products, as in
// k_encupd_perm.  M = 0: runtime m, rows in chunks of UCH, the parts re-read per chunk (cache hits).
template <int M, bool FULL, class Row, class Len>
__device__ __forceinline__ void range_column(const UpdatePtrsArgs& a, const Row& row, const Len& len, uint32_t off) {
    const int count = a.count;
    if constexpr (M > 0) {
        uint4 acc[M];
#pragma unroll
        for (int r = 0; r < M; ++r) acc[r] = make_uint4(0, 0, 0, 0);
        if (a.accumulate) {
#pragma unroll
            for (int r = 0; r < M; ++r) acc[r] = ld16(as_row(row(count + r)) + off);
        }
        range_products<M, true, FULL>(acc, a, row, len, off, 0);
#pragma unroll
        for (int r = 0; r < M; ++r) st16(as_out(row(count + r)) + off, acc[r]);
    } else {
        const int m = a.m;
        for (int r0 = 0; r0 < m; r0 += UCH) {
            uint4 acc[UCH];
#pragma unroll
            for (int j = 0; j < UCH; ++j) {
                acc[j] = make_uint4(0, 0, 0, 0);
                if (a.accumulate && r0 + j < m) acc[j] = ld16(as_row(row(count + r0 + j)) + off);
            }
            range_products<UCH, false, FULL>(acc, a, row, len, off, r0);
#pragma unroll
            for (int j = 0; j < UCH; ++j)
                if (r0 + j < m) st16(as_out(row(count + r0 + j)) + off, acc[j]);
        }
    }
}

// byte b of the m parity shards; a part counts as zero from its length on and is not loaded there
template <class Row, class Len>
__device__ __forceinline__ void range_byte(const UpdatePtrsArgs& a, const Row& row, const Len& len, uint32_t b) {
    const int k = a.k, m = a.m, first = a.first, count = a.count;
#pragma unroll 1
    for (int r = 0; r < m; ++r) {
        uint8_t* out = as_out(row(count + r)) + b;
        uint32_t acc = a.accumulate ? (uint32_t)*out : 0u;
#pragma unroll 1
        for (int c = 0; c < count; ++c) {
            const uint32_t x = b < len(c) ? (uint32_t)as_row(row(c))[b] : 0u;
            acc ^= byte_product(x, a.tab, r * k + first + c);
        }
        *out = (uint8_t)acc;
    }
}

// one wave of the range form; the verdict for block_counts: 0 counts the group as invalid
template <int M, bool VAR>
__device__ __forceinline__ int range_wave(const UpdatePtrsArgs& a, const uint64_t* __restrict__ dptrs,
                                          const uint64_t* __restrict__ pptrs, const int32_t* __restrict__ lens,
                                          uint64_t g, uint32_t slab, int lane) {
    const int k = a.k, m = a.m, first = a.first, count = a.count;
    const uint64_t* dp = dptrs + g * (uint64_t)k + first;
    const uint64_t* pp = pptrs + g * (uint64_t)m;
    const int32_t* ln = VAR ? lens + g * (uint64_t)k + first : nullptr;
    // entry s < count + m of the group: part s, then parity shard s - count.  Lane s holds entry s when
    // all of them fit the wave; the lanes stride over them for the judgement either way.
    const bool held = count + m <= 64;
    uint64_t p = 0;
    uint32_t len = 0;  // as unsigned: a negative length is above every L
    uint32_t low = 0, longest = 0, shortest = 0xFFFFFFFFu;
    for (int s = lane; s < count + m; s += 64) {
        uint64_t q;
        uint32_t l = a.block;
        if (s < count) {
            q = dp[s];
            if constexpr (VAR) l = (uint32_t)ln[s];
            longest = std::max(longest, l);
            shortest = std::min(shortest, l);
            if (l) low |= (uint32_t)q & 15u;  // a part of length 0 is never dereferenced
        } else {
            q = pp[s - count];
            low |= (uint32_t)q & 15u;
        }
        if (s == lane) {
            p = q;
            len = l;
        }
    }
    PtrsVarGeom v = launch_geom(a);
    uint32_t extent = a.block;
    bool full = true;
    if constexpr (VAR) {
        const uint32_t L = (uint32_t)((cptr_i32)a.group_len)[g];
        if (L > a.block || __ballot(longest > L)) return slab == 0 && lane == 0 ? 0 : -1;  // untouched, counted once
        extent = a.accumulate ? wave_max(longest) : L;
        v = ptrs_var_geom(extent, 16);
        if (slab >= v.live) return -1;  // an empty extent, or a slab at or past it
        full = ~wave_max(~shortest) >= slab_reach<16>(v, slab);
    }
    const bool aligned = __ballot(low != 0) == 0;
    const auto row = [&](int s) { return held ? lane_value(p, (uint32_t)s) : s < count ? dp[s] : pp[s - count]; };
    const auto len_of = [&](int c) { return !VAR ? a.block : held ? lane_value32(len, (uint32_t)c) : (uint32_t)ln[c]; };
    run_slab_var<16>(
        v, extent, slab, lane, aligned,
        [&](uint32_t off) {
            if (full) range_column<M, true>(a, row, len_of, off);
            else if constexpr (VAR) range_column<M, false>(a, row, len_of, off);
        },
        [&](uint32_t b) { range_byte(a, row, len_of, b); });
    return -1;
}

// __restrict__ parameters: the address table and the lengths are not written by the launch, so their
// loads need not be ordered against the stores
template <int M, bool VAR>
__global__ void __launch_bounds__(256) k_encupd_ptrs(UpdatePtrsArgs a, const uint64_t* __restrict__ dptrs,
                                                     const uint64_t* __restrict__ pptrs,
                                                     const int32_t* __restrict__ lens) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    int verdict = -1;
    if (wave_item(a, &g, &slab)) verdict = range_wave<M, VAR>(a, dptrs, pptrs, lens, g, slab, lane);
    if constexpr (VAR) {
        if (a.invalid) block_counts<1>(verdict, a.invalid);
    }
}

// ------------------------------------------------------------------ per-group form

// what a wave of the per-group form knows of its group: o, n the lengths of the old and the new row
// (the fixed-length kernels: both block_size), old = nullptr in delta mode
struct UpdateRows {
    const uint8_t* fresh;
    uint8_t* old;
    uint32_t o, n;
};

// The 16-B column at byte off of a group whose shard i (0 <= i < k, wave-uniform) is replaced;
// par(r): the address of parity shard r.  Every load is issued before the first store: the compiler
// cannot move a load above a store it cannot tell apart from it.  FULL: the column is whole in the
// old and in the new row; else either is loaded below its length only and counts as zero from there,
// and the new row's column is stored as far as n reaches.  M = 0: runtime m, parity rows in chunks of
// UCH; the data store follows the first chunk's loads.
template <int M, bool FULL, class Par>
__device__ __forceinline__ void update_column(const UpdatePtrsArgs& a, const UpdateRows& u, const Par& par, int i,
                                              uint32_t off) {
    const int k = a.k;
    uint4 x, d;
    if constexpr (FULL) x = ld16(u.fresh + off);
    else x = ld16_clip(u.fresh, off, u.n);
    d = x;  // the delta
    if (u.old) {
        uint4 o;
        if constexpr (FULL) o = ld16(u.old + off);
        else o = ld16_clip(u.old, off, u.o);
        d = make_uint4(x.x ^ o.x, x.y ^ o.y, x.z ^ o.z, x.w ^ o.w);
    }
    const auto store_new = [&]() {
        if (!u.old) return;
        if (FULL || off + 16u <= u.n) {
            st16(u.old + off, x);
        } else if (off < u.n) {  // the column n cuts: exactly [off, n)
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (uint32_t j = 0; j < 16; ++j)
                if (off + j < u.n) u.old[off + j] = (uint8_t)(w[j >> 2] >> (8u * (j & 3u)));
        }
    };
    Sel s[4];
    if constexpr (M > 0) {
        uint4 p[M];
#pragma unroll
        for (int r = 0; r < M; ++r) p[r] = ld16(as_row(par(r)) + off);
        store_new();
        sel16(s, d);
#pragma unroll
        for (int r = 0; r < M; ++r) {
            uint32_t t[5];
            tab5(t, a.tab, r * k + i);
            gf_mac16(p[r], s, t);
        }
#pragma unroll
        for (int r = 0; r < M; ++r) st16(as_out(par(r)) + off, p[r]);
    } else {
        const int m = a.m;
        sel16(s, d);
        for (int r0 = 0; r0 < m; r0 += UCH) {
            uint4 p[UCH];
#pragma unroll
            for (int j = 0; j < UCH; ++j)
                if (r0 + j < m) p[j] = ld16(as_row(par(r0 + j)) + off);
            if (r0 == 0) store_new();
#pragma unroll
            for (int j = 0; j < UCH; ++j)
                if (r0 + j < m) {
                    uint32_t t[5];
                    tab5(t, a.tab, (r0 + j) * k + i);
                    gf_mac16(p[j], s, t);
                }
#pragma unroll
            for (int j = 0; j < UCH; ++j)
                if (r0 + j < m) st16(as_out(par(r0 + j)) + off, p[j]);
        }
    }
}

// byte b of the group, b < max(o, n)
template <class Par>
__device__ __forceinline__ void update_byte(const UpdatePtrsArgs& a, const UpdateRows& u, const Par& par, int i,
                                            uint32_t b) {
    const int k = a.k, m = a.m;
    uint32_t x = b < u.n ? (uint32_t)u.fresh[b] : 0u;
    if (u.old) {
        const uint32_t o = b < u.o ? (uint32_t)u.old[b] : 0u;
        if (b < u.n) u.old[b] = (uint8_t)x;
        x ^= o;
    }
#pragma unroll 1
    for (int r = 0; r < m; ++r) {
        uint8_t* out = as_out(par(r)) + b;
        *out = (uint8_t)((uint32_t)*out ^ byte_product(x, a.tab, r * k + i));
    }
}

// one wave of the per-group form; the verdict for block_counts: 0 counts the group as invalid.  No
// table is indexed, and nothing else of the group loaded, before the id is known to lie in [0, k).
template <int M, bool VAR>
__device__ __forceinline__ int update_wave(const UpdatePtrsArgs& a, const uint64_t* __restrict__ dptrs,
                                           const uint64_t* __restrict__ pptrs, const uint64_t* __restrict__ news,
                                           uint64_t g, uint32_t slab, int lane) {
    const int k = a.k, m = a.m;
    const int i = ((cptr_i32)a.shard)[g];
    const bool leader = slab == 0 && lane == 0;
    if ((uint32_t)i >= (uint32_t)k) return i >= 0 && leader ? 0 : -1;
    const bool delta = a.delta_only != 0;
    uint32_t o = a.block, n = a.block, extent = a.block;
    PtrsVarGeom v = launch_geom(a);
    bool full = true;
    if constexpr (VAR) {
        const uint32_t L = (uint32_t)((cptr_i32)a.group_len)[g];
        n = (uint32_t)((cptr_i32)a.new_len)[g];
        o = delta ? 0u : (uint32_t)((cptr_i32)a.lens)[g * (uint64_t)k + i];
        if (L > a.block || n > L || o > L) return leader ? 0 : -1;  // untouched, counted once
        extent = std::max(o, n);
        v = ptrs_var_geom(extent, 16);
        if (slab >= v.live) return -1;  // nothing to do (o = n = 0), or a slab at or past max(o, n)
        full = (delta ? n : std::min(o, n)) >= slab_reach<16>(v, slab);
    }
    // entry s < 2 + m: the new row, shard i, parity shard s - 2.  Lane s holds entry s when all of them
    // fit the wave.  Not dereferenced, and so not loaded: the new row of length 0, shard i in delta mode.
    const uint64_t* pp = pptrs + g * (uint64_t)m;
    const bool held = M > 0 || m + 2 <= 64;  // M > 0: m == M <= 4, known here, so those instances carry one path
    uint64_t p = 0;
    uint32_t low = 0;
    for (int s = lane; s < m + 2; s += 64) {
        uint64_t q = 0;
        if (s == 0) {
            if (n) q = news[g];
        } else if (s == 1) {
            if (!delta) q = dptrs[g * (uint64_t)k + i];
        } else {
            q = pp[s - 2];
        }
        low |= (uint32_t)q & 15u;
        if (s == lane) p = q;
    }
    const bool aligned = __ballot(low != 0) == 0;
    UpdateRows u;
    u.fresh = as_row(lane_value(p, 0));
    u.old = delta ? nullptr : as_out(lane_value(p, 1));
    u.o = o;
    u.n = n;
    const auto par = [&](int r) { return held ? lane_value(p, (uint32_t)(r + 2)) : pp[r]; };
    run_slab_var<16>(
        v, extent, slab, lane, aligned,
        [&](uint32_t off) {
            if (full) update_column<M, true>(a, u, par, i, off);
            else if constexpr (VAR) update_column<M, false>(a, u, par, i, off);
        },
        [&](uint32_t b) { update_byte(a, u, par, i, b); });
    return -1;
}

template <int M, bool VAR>
__global__ void __launch_bounds__(256) k_update_ptrs(UpdatePtrsArgs a, const uint64_t* __restrict__ dptrs,
                                                     const uint64_t* __restrict__ pptrs,
                                                     const uint64_t* __restrict__ news) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    int verdict = -1;
    if (wave_item(a, &g, &slab)) verdict = update_wave<M, VAR>(a, dptrs, pptrs, news, g, slab, lane);
    if (a.invalid) block_counts<1>(verdict, a.invalid);
}

// ------------------------------------------------------------------ launchers

// blocks of four waves over groups * wpg waves; false when the caller has to chunk
static inline bool update_ptrs_grid(const UpdatePtrsArgs& a, unsigned* grid) {
    const uint64_t waves = a.groups * (uint64_t)a.wpg;
    if (a.wpg == 0 || waves * 64 > (uint64_t)kMaxLaunchLanes) return false;
    *grid = (unsigned)((waves + 3) / 4);
    return true;
}

template <bool VAR>
static hipError_t launch_range(const UpdatePtrsArgs& a, unsigned grid, hipStream_t stream) {
    const dim3 g(grid), b(256);
    if (a.m == 1) hipLaunchKernelGGL((k_encupd_ptrs<1, VAR>), g, b, 0, stream, a, a.dptrs, a.pptrs, a.lens);
    else if (a.m == 2) hipLaunchKernelGGL((k_encupd_ptrs<2, VAR>), g, b, 0, stream, a, a.dptrs, a.pptrs, a.lens);
    else if (a.m == 3) hipLaunchKernelGGL((k_encupd_ptrs<3, VAR>), g, b, 0, stream, a, a.dptrs, a.pptrs, a.lens);
    else if (a.m == 4) hipLaunchKernelGGL((k_encupd_ptrs<4, VAR>), g, b, 0, stream, a, a.dptrs, a.pptrs, a.lens);
    else hipLaunchKernelGGL((k_encupd_ptrs<0, VAR>), g, b, 0, stream, a, a.dptrs, a.pptrs, a.lens);
    return hipGetLastError();
}

template <bool VAR>
static hipError_t launch_group(const UpdatePtrsArgs& a, unsigned grid, hipStream_t stream) {
    const dim3 g(grid), b(256);
    if (a.m == 1) hipLaunchKernelGGL((k_update_ptrs<1, VAR>), g, b, 0, stream, a, a.dptrs, a.pptrs, a.news);
    else if (a.m == 2) hipLaunchKernelGGL((k_update_ptrs<2, VAR>), g, b, 0, stream, a, a.dptrs, a.pptrs, a.news);
    else if (a.m == 3) hipLaunchKernelGGL((k_update_ptrs<3, VAR>), g, b, 0, stream, a, a.dptrs, a.pptrs, a.news);
    else if (a.m == 4) hipLaunchKernelGGL((k_update_ptrs<4, VAR>), g, b, 0, stream, a, a.dptrs, a.pptrs, a.news);
    else hipLaunchKernelGGL((k_update_ptrs<0, VAR>), g, b, 0, stream, a, a.dptrs, a.pptrs, a.news);
    return hipGetLastError();
}

hipError_t launch_encode_update_ptrs(const UpdatePtrsArgs& a, bool with_lens, hipStream_t stream) {
    if (a.groups == 0 || a.m == 0) return hipSuccess;
    unsigned grid;
    if (!update_ptrs_grid(a, &grid) || a.first < 0 || a.count < 1 || a.first + a.count > a.k)
        return hipErrorInvalidValue;  // caller chunks and checks
    return with_lens ? launch_range<true>(a, grid, stream) : launch_range<false>(a, grid, stream);
}

hipError_t launch_update_ptrs(const UpdatePtrsArgs& a, bool with_lens, hipStream_t stream) {
    if (a.groups == 0 || a.m == 0) return hipSuccess;
    unsigned grid;
    if (!update_ptrs_grid(a, &grid)) return hipErrorInvalidValue;  // caller chunks
    return with_lens ? launch_group<true>(a, grid, stream) : launch_group<false>(a, grid, stream);
}

}  // namespace qfec
