// qfec_update.hip -- incremental parity for MI355X (gfx950): change part of a group that is already
// encoded without reading the rest of it.  Both forms rest on linearity,
//   parity_j ^= rows[j][i] x (old_i ^ new_i),
// and both use the encode's perm tables (entry (r*k + c) * QFEC_TAB_STRIDE, 5 dwords).  The products
// are true GF products: the rs.c stale-row flag of the encode tables is not applied.
//
// Range form (qfec_encode_update): parity[g][j] (^)= sum_c rows[j][first + c] x part[g][c].  The
// encode's flat mapping, one lane per 16-B column, (group, column) flattened over the grid.  The
// columns first .. first + count - 1 are the same for every group, so their tables are uniform over
// the launch and stay in SGPRs.
//
// Per-group form (qfec_update): group g names the one data shard it replaces.  The column differs
// from group to group, and on the flat mapping a wave can straddle two groups, which would turn the
// table reads into per-lane vector loads.  So whole waves go to a group: a wave reads shard[g] once,
// leaves at once when the group is untouched or the id invalid, and otherwise reads the m tables of
// that one column through the constant address space (scalar loads).  A lane reads its old and new
// column (or the delta alone), then the m parity columns, does m multiply-accumulates and writes the
// m parity columns and the new data column.  16-B lanes: 8-B lanes fill a group's waves better
// (B = 1400: 176/192 lanes against 88/128) and were 1-6 % faster with every group touched, but an
// untouched group then retires twice the waves, 2-9 % slower with one group in ten touched
// (profiles/update/lanes_ab.txt); sparse writes are what the call is for.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qfec_internal.hpp"
#include "qfec_device.hpp"

namespace qfec {

// the perm dwords of table entry `idx` (wave-uniform), read through the constant address space
__device__ __forceinline__ void tab5(uint32_t (&t)[5], const uint32_t* tab, int idx) {
    const cptr32 p = (cptr32)tab + idx * QFEC_TAB_STRIDE;
#pragma unroll
    for (int i = 0; i < 5; ++i) t[i] = p[i];
}

// ------------------------------------------------------------------ range form

// acc[j] ^= sum_c rows[r0 + j][first + c] x part row c, j < R (rows past m are left alone); the
// inputs two at a time, so two loads are in flight per lane.  ALL: every one of the R rows exists
template <int R, bool ALL>
__device__ __forceinline__ void range_products(uint4 (&acc)[R], const EncUpdateArgs& a, const uint8_t* src, int r0) {
    const int k = a.k, m = a.m, first = a.first, count = a.count;
    int c = 0;
    for (; c + 1 < count; c += 2) {
        const uint4 xa = ld16(src + (uint64_t)c * a.pitch);
        const uint4 xb = ld16(src + (uint64_t)(c + 1) * a.pitch);
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
        sel16(s, ld16(src + (uint64_t)c * a.pitch));
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (ALL || r0 + j < m) {
                uint32_t t[5];
                tab5(t, a.tab, (r0 + j) * k + first + c);
                gf_mac16(acc[j], s, t);
            }
    }
}

// compile-time M (a.m == M), runtime first / count.  With accumulate the M parity columns are loaded
// ahead of the products, as in k_verify_perm.
template <int M>
__global__ void __launch_bounds__(256) k_encupd_perm(EncUpdateArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= a.work) return;
    const uint64_t g = fast_div(t, a.cols_div);
    const uint32_t col = (uint32_t)(t - g * (uint64_t)a.cols);
    const uint8_t* src = a.part + g * a.sgs + (uint64_t)col * 16u;
    uint8_t* dst = a.parity + g * a.pgs + (uint64_t)col * 16u;
    uint4 acc[M];
#pragma unroll
    for (int r = 0; r < M; ++r) acc[r] = make_uint4(0, 0, 0, 0);
    if (a.accumulate) {
#pragma unroll
        for (int r = 0; r < M; ++r) acc[r] = ld16(dst + (uint64_t)r * a.pitch);
    }
    range_products<M, true>(acc, a, src, 0);
#pragma unroll
    for (int r = 0; r < M; ++r) st16(dst + (uint64_t)r * a.pitch, acc[r]);
}

// runtime m: rows in chunks of UCH; the count inputs are re-read per chunk (cache hits)
constexpr int UCH = 4;

__global__ void __launch_bounds__(256) k_encupd_any(EncUpdateArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= a.work) return;
    const uint64_t g = fast_div(t, a.cols_div);
    const uint32_t col = (uint32_t)(t - g * (uint64_t)a.cols);
    const uint8_t* src = a.part + g * a.sgs + (uint64_t)col * 16u;
    uint8_t* dst = a.parity + g * a.pgs + (uint64_t)col * 16u;
    const int m = a.m;
    for (int r0 = 0; r0 < m; r0 += UCH) {
        uint4 acc[UCH];
#pragma unroll
        for (int j = 0; j < UCH; ++j) {
            acc[j] = make_uint4(0, 0, 0, 0);
            if (a.accumulate && r0 + j < m) acc[j] = ld16(dst + (uint64_t)(r0 + j) * a.pitch);
        }
        range_products<UCH, false>(acc, a, src, r0);
#pragma unroll
        for (int j = 0; j < UCH; ++j)
            if (r0 + j < m) st16(dst + (uint64_t)(r0 + j) * a.pitch, acc[j]);
    }
}

// byte-granular fallback for pitches / pointers that are not 16-B aligned: one lane per byte of
// [0, block_size)
__global__ void __launch_bounds__(256) k_encupd_bytes(EncUpdateArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= a.work) return;
    const uint64_t g = fast_div(t, a.cols_div);
    const uint32_t b = (uint32_t)(t - g * (uint64_t)a.cols);
    const int k = a.k, m = a.m;
    const uint8_t* src = a.part + g * a.sgs + b;
    uint8_t* dst = a.parity + g * a.pgs + b;
    for (int r = 0; r < m; ++r) {
        uint32_t acc = a.accumulate ? (uint32_t)dst[(uint64_t)r * a.pitch] : 0u;
        for (int c = 0; c < a.count; ++c) {
            const uint32_t* tc = a.tab + (r * k + a.first + c) * QFEC_TAB_STRIDE;
            const Sel s = gf_sel((uint32_t)src[(uint64_t)c * a.pitch]);
            acc ^= gf_mul4(s, tc[0], tc[1], tc[2], tc[3], tc[4]);
        }
        dst[(uint64_t)r * a.pitch] = (uint8_t)acc;
    }
}

hipError_t launch_encode_update(const EncUpdateArgs& a, hipStream_t stream) {
    if (a.work == 0 || a.m == 0) return hipSuccess;
    if (a.work > 0x7FFFFFFFull || a.first < 0 || a.count < 1 || a.first + a.count > a.k)
        return hipErrorInvalidValue;  // caller chunks and checks
    const unsigned grid = (unsigned)((a.work + 255) / 256);
    if (!a.vec16) hipLaunchKernelGGL(k_encupd_bytes, dim3(grid), dim3(256), 0, stream, a);
    else if (a.m == 1) hipLaunchKernelGGL(k_encupd_perm<1>, dim3(grid), dim3(256), 0, stream, a);
    else if (a.m == 2) hipLaunchKernelGGL(k_encupd_perm<2>, dim3(grid), dim3(256), 0, stream, a);
    else if (a.m == 3) hipLaunchKernelGGL(k_encupd_perm<3>, dim3(grid), dim3(256), 0, stream, a);
    else if (a.m == 4) hipLaunchKernelGGL(k_encupd_perm<4>, dim3(grid), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_encupd_any, dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ per-group form

// The 16-B column at byte `off` of group g, whose shard i (0 <= i < k, wave-uniform) is replaced.
// Every load is issued before the first store: the compiler cannot move a load above a store it
// cannot tell apart from it.  M = 0: runtime m, parity rows in chunks of UCH.
template <int M>
__device__ __forceinline__ void update_column(const UpdateArgs& a, uint64_t g, int i, uint64_t off) {
    const int k = a.k;
    uint8_t* par = a.parity + g * a.pgs + off;
    uint8_t* old = a.data ? a.data + g * a.dgs + (uint64_t)i * a.pitch + off : nullptr;
    const uint4 x = ld16(a.rows + g * a.pitch + off);
    uint4 d = x;  // the delta
    if (old) {
        const uint4 o = ld16(old);
        d = make_uint4(x.x ^ o.x, x.y ^ o.y, x.z ^ o.z, x.w ^ o.w);
    }
    Sel s[4];
    if constexpr (M > 0) {
        uint4 p[M];
#pragma unroll
        for (int r = 0; r < M; ++r) p[r] = ld16(par + (uint64_t)r * a.pitch);
        if (old) st16(old, x);
        sel16(s, d);
#pragma unroll
        for (int r = 0; r < M; ++r) {
            uint32_t t[5];
            tab5(t, a.tab, r * k + i);
            gf_mac16(p[r], s, t);
        }
#pragma unroll
        for (int r = 0; r < M; ++r) st16(par + (uint64_t)r * a.pitch, p[r]);
    } else {
        const int m = a.m;
        if (old) st16(old, x);
        sel16(s, d);
        for (int r0 = 0; r0 < m; r0 += UCH) {
            uint4 p[UCH];
#pragma unroll
            for (int j = 0; j < UCH; ++j)
                if (r0 + j < m) p[j] = ld16(par + (uint64_t)(r0 + j) * a.pitch);
#pragma unroll
            for (int j = 0; j < UCH; ++j)
                if (r0 + j < m) {
                    uint32_t t[5];
                    tab5(t, a.tab, (r0 + j) * k + i);
                    gf_mac16(p[j], s, t);
                }
#pragma unroll
            for (int j = 0; j < UCH; ++j)
                if (r0 + j < m) st16(par + (uint64_t)(r0 + j) * a.pitch, p[j]);
        }
    }
}

// 4 waves per block over (group, 64-column slab).  An id >= k is counted once per group, by lane 0
// of the group's first wave, through the block's sum (block_counts: every thread of the block calls
// it, so no wave returns early).  No table is indexed before the id is known to lie in [0, k).
template <int M>
__global__ void __launch_bounds__(256) k_update_perm(UpdateArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t wid = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t g = wid / a.wpg;
    const uint32_t slab = wid - (uint32_t)g * a.wpg;
    int verdict = -1;
    if (g < a.groups) {
        const int i = ((const __attribute__((address_space(4))) int32_t*)a.shard)[g];
        if ((uint32_t)i >= (uint32_t)a.k) {
            if (i >= 0 && slab == 0 && lane == 0) verdict = 0;
        } else {
            const uint32_t col = slab * 64u + lane;
            if (col < a.cols) update_column<M>(a, g, i, (uint64_t)col * 16u);
        }
    }
    if (a.invalid) block_counts<1>(verdict, a.invalid);
}

// byte-granular fallback for layouts that are not 16-B aligned: the flat mapping, one lane per byte
// of [0, block_size); the shard id and the tables are read per lane
__global__ void __launch_bounds__(256) k_update_bytes(UpdateArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    int verdict = -1;
    if (t < a.work) {
        const uint64_t g = fast_div(t, a.cols_div);
        const uint32_t b = (uint32_t)(t - g * (uint64_t)a.cols);
        const int k = a.k, m = a.m;
        const int i = a.shard[g];
        if ((uint32_t)i >= (uint32_t)k) {
            if (i >= 0 && b == 0) verdict = 0;
        } else {
            uint32_t x = a.rows[g * a.pitch + b];
            if (a.data) {
                uint8_t* old = a.data + g * a.dgs + (uint64_t)i * a.pitch + b;
                const uint32_t o = *old;
                *old = (uint8_t)x;
                x ^= o;
            }
            const Sel s = gf_sel(x);
            uint8_t* par = a.parity + g * a.pgs + b;
            for (int r = 0; r < m; ++r) {
                const uint32_t* tc = a.tab + (r * k + i) * QFEC_TAB_STRIDE;
                par[(uint64_t)r * a.pitch] ^= (uint8_t)gf_mul4(s, tc[0], tc[1], tc[2], tc[3], tc[4]);
            }
        }
    }
    if (a.invalid) block_counts<1>(verdict, a.invalid);
}

hipError_t launch_update(const UpdateArgs& a, hipStream_t stream) {
    if (a.groups == 0 || a.m == 0) return hipSuccess;
    if (!a.vec16) {
        if (a.work == 0 || a.work > 0x7FFFFFFFull) return hipErrorInvalidValue;  // caller chunks
        hipLaunchKernelGGL(k_update_bytes, dim3((unsigned)((a.work + 255) / 256)), dim3(256), 0, stream, a);
        return hipGetLastError();
    }
    const uint64_t waves = a.groups * a.wpg;
    if (a.wpg == 0 || waves * 64 > 0x7FFFFFFFull) return hipErrorInvalidValue;  // caller chunks
    const unsigned grid = (unsigned)((waves + 3) / 4);
    if (a.m == 1) hipLaunchKernelGGL(k_update_perm<1>, dim3(grid), dim3(256), 0, stream, a);
    else if (a.m == 2) hipLaunchKernelGGL(k_update_perm<2>, dim3(grid), dim3(256), 0, stream, a);
    else if (a.m == 3) hipLaunchKernelGGL(k_update_perm<3>, dim3(grid), dim3(256), 0, stream, a);
    else if (a.m == 4) hipLaunchKernelGGL(k_update_perm<4>, dim3(grid), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_update_perm<0>, dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace qfec
