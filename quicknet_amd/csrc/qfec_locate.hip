// qfec_locate.hip -- which single shard of a group is corrupted?  (qfec_locate / qfec_scrub, gfx950)
//
// The hot path is qfec_verify.hip's: one lane per 16-byte column, (group, column) flattened over the
// grid, the encode's perm tables, k >= 16 inputs in two halves.  The lane keeps its m syndromes
// s_j = (parity_j ^ sum_i P[j][i] x data_i) under the column's byte mask instead of reducing them
// to a bit each.  A wave in which every lane's syndromes are zero does nothing more.
//
// Cold branch, entered wave-uniformly off a ballot: a lane with a non-zero syndrome tests every
// data shard i as the culprit.  An error e in data shard i gives s_j = P[j][i] x e, hence
// s_j = r_{j,i} x s_0 with r_{j,i} = P[j][i] / P[0][i] in every byte; the lane forms the selectors
// of s_0 once and spends m - 1 constant multiplies per candidate (ratio perm tables, wave-uniform
// loads).  A lane whose syndromes are all zero votes for every candidate.  Per group seen in the
// wave the lanes' candidate masks are AND-reduced with ballots, then one lane issues one atomic AND
// into the group's candidate word (preset to all ones) and one atomic OR into its bad-rows word
// (preset to zero): a group's columns span waves and blocks.
//
// A corrupted parity row j0 shows as bad_rows == 1 << j0 (and kills every data candidate, the
// ratios being non-zero); k_locate_finish adds it to the candidates and writes the verdict.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qfec.h"
#include "qfec_internal.hpp"
#include "qfec_device.hpp"

namespace qfec {

// same16, nonzero16 and ratio_holds are in qfec_device.hpp, shared with qfec_integrity_ptrs.hip

__device__ __forceinline__ uint4 syndrome16(const uint4& acc, const uint4& p, const uint4& mk) {
    return make_uint4((acc.x ^ p.x) & mk.x, (acc.y ^ p.y) & mk.y, (acc.z ^ p.z) & mk.z, (acc.w ^ p.w) & mk.w);
}

// compile-time K, M
template <int K, int M>
__global__ void __launch_bounds__(256) k_locate_perm(LocateArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t g32 = 0, bad = 0;
    uint4 acc[M];  // the products, then the syndromes
#pragma unroll
    for (int r = 0; r < M; ++r) acc[r] = make_uint4(0, 0, 0, 0);
    if (t < a.work) {
        const uint64_t g = fast_div(t, a.cols_div);
        const uint32_t col = (uint32_t)(t - g * (uint64_t)a.cols);
        const uint8_t* src = a.data + g * a.dgs + (uint64_t)col * 16u;
        const uint8_t* par = a.parity + g * a.pgs + (uint64_t)col * 16u;
        uint4 p[M];
#pragma unroll
        for (int r = 0; r < M; ++r) p[r] = ld16(par + (uint64_t)r * a.pitch);
        products16<K, M>(acc, src, a.pitch, a.tab);
        const uint4 mk = column_mask(a.block, col);
#pragma unroll
        for (int r = 0; r < M; ++r) {
            acc[r] = syndrome16(acc[r], p[r], mk);
            if (nonzero16(acc[r])) bad |= 1u << r;
        }
        g32 = (uint32_t)g;
    }
    if (__ballot(bad != 0) == 0) return;  // the whole wave is consistent: verify's cost
    uint32_t cand = 0xFFFFFFFFu;
    if (bad != 0) {
        const uint32_t* __restrict__ rtab = a.rtab;
        Sel s0[4];
        sel16(s0, acc[0]);
        cand = 0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            bool ok = true;
#pragma unroll
            for (int j = 1; j < M; ++j) ok = ok && ratio_holds(s0, acc[j], rtab + (i * (M - 1) + j - 1) * QFEC_TAB_STRIDE);
            if (ok) cand |= 1u << i;
        }
    }
    flat_report<true>(a.bad_rows, a.cand, nullptr, a.k, a.m, g32, bad, cand);
}

// runtime k, m: rows in chunks of LCH.
// s_0 comes with the first chunk and stays; each chunk's rows are tested against it while they
// are live.  A lane whose first non-zero syndrome turns up in a later chunk has s_0 = 0 there, and
// the test of that chunk then drops every candidate, as it must.
constexpr int LCH = 4;

__global__ void __launch_bounds__(256) k_locate_any(LocateArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t g32 = 0, bad = 0, cand = 0xFFFFFFFFu;
    const int k = a.k, m = a.m;
    uint64_t g = 0;
    uint32_t col = 0;
    const bool live = t < a.work;
    if (live) {
        g = fast_div(t, a.cols_div);
        col = (uint32_t)(t - g * (uint64_t)a.cols);
        g32 = (uint32_t)g;
    }
    const uint8_t* src = a.data + g * a.dgs + (uint64_t)col * 16u;
    const uint8_t* par = a.parity + g * a.pgs + (uint64_t)col * 16u;
    const uint4 mk = column_mask(a.block, col);
    uint4 s0 = make_uint4(0, 0, 0, 0);
    for (int r0 = 0; r0 < m; r0 += LCH) {  // wave-uniform
        uint4 s[LCH];
#pragma unroll
        for (int j = 0; j < LCH; ++j) s[j] = make_uint4(0, 0, 0, 0);
        if (live) {
            products16_rows<LCH>(s, src, a.pitch, a.tab, k, m, r0);
#pragma unroll
            for (int j = 0; j < LCH; ++j)
                if (r0 + j < m) {
                    s[j] = syndrome16(s[j], ld16(par + (uint64_t)(r0 + j) * a.pitch), mk);
                    if (nonzero16(s[j])) bad |= 1u << (r0 + j);
                }
            if (r0 == 0) s0 = s[0];
        }
        if (__ballot(bad != 0) == 0) continue;  // nothing wrong in this wave so far
        if (bad != 0) {
            Sel sl[4];
            sel16(sl, s0);
            for (int i = 0; i < k; ++i) {
                bool ok = true;
#pragma unroll
                for (int j = 0; j < LCH; ++j) {
                    const int row = r0 + j;
                    if (row >= 1 && row < m)
                        ok = ok && ratio_holds(sl, s[j], a.rtab + (i * (m - 1) + row - 1) * QFEC_TAB_STRIDE);
                }
                if (!ok) cand &= ~(1u << i);
            }
        }
    }
    if (__ballot(bad != 0) == 0) return;
    flat_report<true>(a.bad_rows, a.cand, nullptr, a.k, a.m, g32, bad, cand);
}

// byte-granular fallback for pitches / pointers that are not 16-B aligned: one lane per byte of
// [0, block_size), so there is no tail to mask
__global__ void __launch_bounds__(256) k_locate_bytes(LocateArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t g32 = 0, bad = 0, cand = 0xFFFFFFFFu;
    const int k = a.k, m = a.m;
    uint64_t g = 0;
    uint32_t b = 0;
    const bool live = t < a.work;
    if (live) {
        g = fast_div(t, a.cols_div);
        b = (uint32_t)(t - g * (uint64_t)a.cols);
        g32 = (uint32_t)g;
    }
    const uint8_t* src = a.data + g * a.dgs + b;
    const uint8_t* par = a.parity + g * a.pgs + b;
    uint32_t s0 = 0;
    for (int r = 0; r < m; ++r) {  // wave-uniform
        uint32_t s = 0;
        if (live) {
            s = (product_byte(src, a.pitch, a.tab, k, r) ^ (uint32_t)par[(uint64_t)r * a.pitch]) & 0xFFu;
            if (s) bad |= 1u << r;
            if (r == 0) s0 = s;
        }
        if (r == 0 || __ballot(bad != 0) == 0) continue;
        if (bad != 0) {
            const Sel sl = gf_sel(s0);
            for (int i = 0; i < k; ++i) {
                const uint32_t* tc = a.rtab + (i * (m - 1) + r - 1) * QFEC_TAB_STRIDE;
                if ((gf_mul4(sl, tc[0], tc[1], tc[2], tc[3], tc[4]) & 0xFFu) != s) cand &= ~(1u << i);
            }
        }
    }
    if (__ballot(bad != 0) == 0) return;
    flat_report<true>(a.bad_rows, a.cand, nullptr, a.k, a.m, g32, bad, cand);
}

// the verdict of group g from its two words: candidates = the data bits that survived every column,
// plus parity row j0 iff it is the only bad row.  Writes culprit and marks; returns the counter the
// group bumps (0 located, 1 multi, 2 ambiguous) or -1 for a clean group.
__device__ __forceinline__ int locate_verdict(const LocateFinishArgs& a, uint64_t g) {
    const int k = a.k, m = a.m;
    const uint32_t rows = a.bad_rows[g];
    const uint32_t dc = a.cand[g] & (k >= 32 ? 0xFFFFFFFFu : (1u << k) - 1u);
    const bool one_row = __builtin_popcount(rows) == 1;
    int id = QFEC_LOC_CLEAN;
    if (rows != 0) {
        const int nc = __builtin_popcount(dc) + (one_row ? 1 : 0);
        id = nc == 0 ? QFEC_LOC_MULTI : nc > 1 ? QFEC_LOC_AMBIGUOUS : dc ? __builtin_ctz(dc) : k + __builtin_ctz(rows);
    }
    a.culprit[g] = id;
    if (a.marks) write_marks_rs(a.marks, a.groups, g, k, m, id >= 0 ? 1ull << id : 0ull);
    return rows == 0 ? -1 : id >= 0 ? 0 : id == QFEC_LOC_MULTI ? 1 : 2;
}

// one lane per group, after the last chunk
__global__ void __launch_bounds__(256) k_locate_finish(LocateFinishArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    int verdict = -1;  // also for lanes past the last group
    if (g < a.groups) verdict = locate_verdict(a, g);
    if (a.counts) block_counts<3>(verdict, a.counts);  // uniform over the grid
}

#define QFEC_LOC_CASE(KK, MM)                                                                    \
    if (a.k == KK && a.m == MM) {                                                                \
        hipLaunchKernelGGL((k_locate_perm<KK, MM>), dim3(grid), dim3(256), 0, stream, a);        \
        return hipGetLastError();                                                                \
    }

hipError_t launch_locate(const LocateArgs& a, hipStream_t stream) {
    if (a.work == 0) return hipSuccess;
    if (a.work > 0x7FFFFFFFull || a.m < 2 || a.m > 32 || a.k > 32 || !a.bad_rows || !a.cand || !a.rtab)
        return hipErrorInvalidValue;  // caller chunks and checks the code
    const unsigned grid = (unsigned)((a.work + 255) / 256);
    if (!a.vec16) {
        hipLaunchKernelGGL(k_locate_bytes, dim3(grid), dim3(256), 0, stream, a);
        return hipGetLastError();
    }
    // launch_verify's instances with m >= 2
    QFEC_LOC_CASE(10, 3)
    QFEC_LOC_CASE(16, 4)
    QFEC_LOC_CASE(4, 2)
    QFEC_LOC_CASE(2, 2)
    QFEC_LOC_CASE(3, 2)
    QFEC_LOC_CASE(5, 3)
    QFEC_LOC_CASE(6, 2)
    QFEC_LOC_CASE(8, 2)
    QFEC_LOC_CASE(8, 4)
    QFEC_LOC_CASE(12, 4)
    QFEC_LOC_CASE(20, 4)
    hipLaunchKernelGGL(k_locate_any, dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_locate_finish(const LocateFinishArgs& a, hipStream_t stream) {
    if (a.groups == 0) return hipSuccess;
    if (!a.bad_rows || !a.cand || !a.culprit || a.groups > 0x7FFFFFFFull * 256u) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((a.groups + 255) / 256);
    hipLaunchKernelGGL(k_locate_finish, dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace qfec
