// qfec_integrity_ptrs.hip -- the parity check and single-shard error location on shards scattered in
// device memory, for MI355X (gfx950): qfec_verify_ptrs and qfec_locate_ptrs (and, through the latter,
// qfec_scrub_ptrs).  The caller hands over qfec_encode_ptrs' table of shard addresses; a shard is
// exactly block_size bytes, at any alignment, no byte outside it is read and nothing is written
// into a shard.
//
// Mapping and addresses: qfec_ptrs.hip's -- one wave per (group, slab of 64 columns of 16 B), four
// waves per block; lane s < k + m loads the address of shard s and the wave reads it with one
// v_readlane pair per shard.  Every lane executes its table load before the first lane-dependent
// branch and every early exit is wave-uniform (the hazard).  The runtime-k,m verify
// (k + m may pass 64) reads the table through its __restrict__ parameter instead.  Alignment is
// judged per group by one ballot of the loaded low bits: an aligned group runs the vector body on
// its whole columns and the block_size % 16 bytes after them byte by byte on the first lanes of its
// last wave; any other group runs the same waves over the same spans byte by byte.
//
// Vector body: whole columns only, so there is no column mask.  The M parity columns are loaded
// first, then the K data columns (K >= 16: in two halves, as encode_column); the product is the
// encode's multiply-accumulate from zero, a true GF product (the stale-row flag of the tables is
// not applied).  The verify compares; the locate keeps the M syndromes and, after run_slab, runs
// k_locate_perm's cold branch on them.
//
// Byte body: it runs inside a loop whose trip count differs from lane to lane (the misaligned
// path), so it holds no ballot and no shuffle.  A lane accumulates its row bits (and candidates)
// in registers; where k_locate_bytes skips the candidate test off a ballot, the test here is the
// lane's own "a syndrome of this byte is non-zero so far".
//
// Reporting: once per wave, after run_slab.  A wave without a finding leaves; otherwise
// flat_report, in which every lane carries the same group, so it runs one round and issues one
// atomic OR (and AND) per wave.  The slabs of a group are separate waves and meet only in those
// atomics; k_locate_finish turns the two words of a group into its verdict, as for qfec_locate.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "qfec_internal.hpp"
#include "qfec_device.hpp"
#include "qfec_geom.hpp"
#include "qfec_ptrs_device.hpp"

namespace qfec {

// ------------------------------------------------------------------ verify

// __restrict__ parameters: nothing the launch reads through them is written by it
template <int K, int M>
__global__ void __launch_bounds__(256) k_verify_ptrs(IntegrityPtrsArgs a, const uint64_t* __restrict__ dptrs,
                                                     const uint64_t* __restrict__ pptrs,
                                                     const uint32_t* __restrict__ tab) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a, &g, &slab)) return;
    const uint64_t p = lane_row(dptrs, pptrs, g, K, M, lane);
    const bool aligned = __ballot((p & 15u) != 0) == 0;
    uint32_t bad = 0, none = 0;
    run_slab<16>(
        a, slab, lane, aligned,
        [&](uint64_t off) {
            uint4 s[M];
            syndromes16<K, M>(s, p, tab, off);
#pragma unroll
            for (int r = 0; r < M; ++r)
                if (nonzero16(s[r])) bad |= 1u << r;
        },
        [&](uint64_t b) {
            check_byte<K, false>(K, M, tab, nullptr, [&](int s) { return lane_value(p, s); }, b, bad, none);
        });
    if (__ballot(bad != 0) == 0) return;  // the whole wave is consistent
    flat_report<false>(a.bad_rows, nullptr, a.bad_groups, K, M, (uint32_t)g, bad, 0);
}

// runtime k, m (k + m may pass 64 lanes: the addresses are read from the table where they are used);
// rows in chunks of PCH, the k inputs re-read per chunk (cache hits)
constexpr int PCH = 4;

__global__ void __launch_bounds__(256) k_verify_ptrs_any(IntegrityPtrsArgs a, const uint64_t* __restrict__ dptrs,
                                                         const uint64_t* __restrict__ pptrs,
                                                         const uint32_t* __restrict__ tab) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a, &g, &slab)) return;
    const int k = a.k, m = a.m;
    const uint64_t* dp = dptrs + g * (uint64_t)k;
    const uint64_t* pp = pptrs + g * (uint64_t)m;
    uint32_t low = 0;
    for (int i = lane; i < k + m; i += 64) low |= (uint32_t)(i < k ? dp[i] : pp[i - k]) & 15u;
    const bool aligned = __ballot(low != 0) == 0;
    uint32_t bad = 0, none = 0;
    run_slab<16>(
        a, slab, lane, aligned,
        [&](uint64_t off) {
            for (int r0 = 0; r0 < m; r0 += PCH) {
                uint4 par[PCH], acc[PCH];
#pragma unroll
                for (int j = 0; j < PCH; ++j) {
                    par[j] = acc[j] = make_uint4(0, 0, 0, 0);
                    if (r0 + j < m) par[j] = ld16(as_row(pp[r0 + j]) + off);
                }
                for (int c = 0; c < k; ++c) {
                    const uint4 v = ld16(as_row(dp[c]) + off);
                    Sel s[4];
                    sel16(s, v);
#pragma unroll
                    for (int j = 0; j < PCH; ++j)
                        if (r0 + j < m) gf_mac16(acc[j], s, tab + ((r0 + j) * k + c) * QFEC_TAB_STRIDE);
                }
#pragma unroll
                for (int j = 0; j < PCH; ++j)
                    if (r0 + j < m && !same16(acc[j], par[j])) bad |= 1u << (r0 + j);
            }
        },
        [&](uint64_t b) {
            check_byte<0, false>(k, m, tab, nullptr, [&](int s) { return s < k ? dp[s] : pp[s - k]; }, b, bad, none);
        });
    if (__ballot(bad != 0) == 0) return;
    flat_report<false>(a.bad_rows, nullptr, a.bad_groups, k, m, (uint32_t)g, bad, 0);
}

// ------------------------------------------------------------------ locate

template <int K, int M>
__global__ void __launch_bounds__(256) k_locate_ptrs(IntegrityPtrsArgs a, const uint64_t* __restrict__ dptrs,
                                                     const uint64_t* __restrict__ pptrs,
                                                     const uint32_t* __restrict__ tab,
                                                     const uint32_t* __restrict__ rtab) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a, &g, &slab)) return;
    const uint64_t p = lane_row(dptrs, pptrs, g, K, M, lane);
    const bool aligned = __ballot((p & 15u) != 0) == 0;
    uint4 s[M];  // the syndromes of the lane's whole column, if it has one
#pragma unroll
    for (int r = 0; r < M; ++r) s[r] = make_uint4(0, 0, 0, 0);
    uint32_t vbad = 0, bbad = 0, cand = 0xFFFFFFFFu;
    run_slab<16>(
        a, slab, lane, aligned,
        [&](uint64_t off) {
            syndromes16<K, M>(s, p, tab, off);
#pragma unroll
            for (int r = 0; r < M; ++r)
                if (nonzero16(s[r])) vbad |= 1u << r;
        },
        [&](uint64_t b) {
            check_byte<K, true>(K, M, tab, rtab, [&](int i) { return lane_value(p, i); }, b, bbad, cand);
        });
    const uint32_t bad = vbad | bbad;
    if (__ballot(bad != 0) == 0) return;  // the whole wave is consistent: verify's cost
    if (vbad != 0) {                      // k_locate_perm's cold branch, after every load
        Sel s0[4];
        sel16(s0, s[0]);
        uint32_t vc = 0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            bool ok = true;
#pragma unroll
            for (int j = 1; j < M; ++j) ok = ok && ratio_holds(s0, s[j], rtab + (i * (M - 1) + j - 1) * QFEC_TAB_STRIDE);
            if (ok) vc |= 1u << i;
        }
        cand &= vc;
    }
    flat_report<true>(a.bad_rows, a.cand, nullptr, K, M, (uint32_t)g, bad, cand);
}

// runtime k, m (k + m <= 64, so the lanes hold the addresses and no mask of k + m bits is formed);
// rows in chunks of LCH.  k_locate_any's rule for s_0: it comes with the first chunk and stays, and
// each chunk's rows are tested against it while they are live; a column whose first non-zero
// syndrome turns up in a later chunk has s_0 = 0 there, and that chunk's test drops every candidate.
constexpr int LCH = 4;

__global__ void __launch_bounds__(256) k_locate_ptrs_any(IntegrityPtrsArgs a, const uint64_t* __restrict__ dptrs,
                                                         const uint64_t* __restrict__ pptrs,
                                                         const uint32_t* __restrict__ tab,
                                                         const uint32_t* __restrict__ rtab) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a, &g, &slab)) return;
    const int k = a.k, m = a.m;
    const uint64_t p = lane_row(dptrs, pptrs, g, k, m, lane);
    const bool aligned = __ballot((p & 15u) != 0) == 0;
    uint32_t bad = 0, cand = 0xFFFFFFFFu;
    run_slab<16>(
        a, slab, lane, aligned,
        [&](uint64_t off) {
            uint4 s0 = make_uint4(0, 0, 0, 0);
            uint32_t vbad = 0;
            for (int r0 = 0; r0 < m; r0 += LCH) {
                uint4 par[LCH], s[LCH];
#pragma unroll
                for (int j = 0; j < LCH; ++j) {
                    par[j] = s[j] = make_uint4(0, 0, 0, 0);
                    if (r0 + j < m) par[j] = ld16(as_row(lane_value(p, k + r0 + j)) + off);
                }
                for (int c = 0; c < k; ++c) {
                    const uint4 v = ld16(as_row(lane_value(p, c)) + off);
                    Sel sl[4];
                    sel16(sl, v);
#pragma unroll
                    for (int j = 0; j < LCH; ++j)
                        if (r0 + j < m) gf_mac16(s[j], sl, tab + ((r0 + j) * k + c) * QFEC_TAB_STRIDE);
                }
#pragma unroll
                for (int j = 0; j < LCH; ++j) {
                    xor16(s[j], par[j]);
                    if (nonzero16(s[j])) vbad |= 1u << (r0 + j);  // rows past m are zero
                }
                if (r0 == 0) s0 = s[0];
                if (vbad != 0) {  // cold, after the chunk's loads
                    Sel sl[4];
                    sel16(sl, s0);
                    for (int i = 0; i < k; ++i) {
                        bool ok = true;
#pragma unroll
                        for (int j = 0; j < LCH; ++j) {
                            const int row = r0 + j;
                            if (row >= 1 && row < m)
                                ok = ok && ratio_holds(sl, s[j], rtab + (i * (m - 1) + row - 1) * QFEC_TAB_STRIDE);
                        }
                        if (!ok) cand &= ~(1u << i);
                    }
                }
            }
            bad |= vbad;
        },
        [&](uint64_t b) {
            check_byte<0, true>(k, m, tab, rtab, [&](int i) { return lane_value(p, i); }, b, bad, cand);
        });
    if (__ballot(bad != 0) == 0) return;
    flat_report<true>(a.bad_rows, a.cand, nullptr, k, m, (uint32_t)g, bad, cand);
}

// ------------------------------------------------------------------ launchers

// blocks of four waves over groups * wpg waves; false when the caller has to chunk
static inline bool integrity_grid(const IntegrityPtrsArgs& a, unsigned* grid) {
    const uint64_t waves = a.groups * (uint64_t)a.wpg;
    if (a.wpg == 0 || waves * 64 > (uint64_t)kMaxLaunchLanes) return false;
    *grid = (unsigned)((waves + 3) / 4);
    return true;
}

#define QFEC_PVER_CASE(KK, MM)                                                                                     \
    if (a.k == KK && a.m == MM) {                                                                                  \
        hipLaunchKernelGGL((k_verify_ptrs<KK, MM>), dim3(grid), dim3(256), 0, stream, a, a.dptrs, a.pptrs, a.tab); \
        return hipGetLastError();                                                                                  \
    }

hipError_t launch_verify_ptrs(const IntegrityPtrsArgs& a, hipStream_t stream) {
    if (a.groups == 0 || a.m == 0) return hipSuccess;
    unsigned grid;
    if (a.m > 32 || !a.bad_rows || !a.tab || !integrity_grid(a, &grid)) return hipErrorInvalidValue;
    // qfec_ptrs.hip's instances
    QFEC_PVER_CASE(10, 3)
    QFEC_PVER_CASE(16, 4)
    QFEC_PVER_CASE(4, 2)
    QFEC_PVER_CASE(8, 4)
    hipLaunchKernelGGL(k_verify_ptrs_any, dim3(grid), dim3(256), 0, stream, a, a.dptrs, a.pptrs, a.tab);
    return hipGetLastError();
}

#define QFEC_PLOC_CASE(KK, MM)                                                                                    \
    if (a.k == KK && a.m == MM) {                                                                                 \
        hipLaunchKernelGGL((k_locate_ptrs<KK, MM>), dim3(grid), dim3(256), 0, stream, a, a.dptrs, a.pptrs, a.tab, \
                           a.rtab);                                                                               \
        return hipGetLastError();                                                                                 \
    }

hipError_t launch_locate_ptrs(const IntegrityPtrsArgs& a, hipStream_t stream) {
    if (a.groups == 0) return hipSuccess;
    unsigned grid;
    if (a.m < 2 || a.m > 32 || a.k > 32 || !a.bad_rows || !a.cand || !a.tab || !a.rtab || !integrity_grid(a, &grid))
        return hipErrorInvalidValue;  // caller chunks and checks the code
    QFEC_PLOC_CASE(10, 3)
    QFEC_PLOC_CASE(16, 4)
    QFEC_PLOC_CASE(4, 2)
    QFEC_PLOC_CASE(8, 4)
    hipLaunchKernelGGL(k_locate_ptrs_any, dim3(grid), dim3(256), 0, stream, a, a.dptrs, a.pptrs, a.tab, a.rtab);
    return hipGetLastError();
}

}  // namespace qfec
