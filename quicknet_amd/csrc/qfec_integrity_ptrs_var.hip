// qfec_integrity_ptrs_var.hip -- the parity check, single-shard error location and correction on shards
// scattered in device memory that each have their own length, for MI355X (gfx950):
// qfec_verify_ptrs_var, qfec_locate_ptrs_var and the correction launch of qfec_scrub_ptrs_var.  Data
// shard i of a group is len_i bytes and counts as zero-filled up to the group's length L =
// d_group_len[g], the length of its parity shards.  No byte at or past len_i of a data shard or past
// L of a parity shard is read, a shard of length 0 is never dereferenced, and only the correction
// writes: [0, len_i) of a located data shard, [0, L) of a located parity shard.
//
// Mapping, loads and exits: qfec_ptrs_var.hip's.  One wave per (group, slab of 64 columns of 16 B),
// four waves per block, wpg waves per group from ptrs_geom(max_len, 16); lane s < k + m loads address
// s and lane i < k its length in the same round trip, L is a scalar load.  Every lane executes those
// loads before the first lane-dependent branch and every early exit is wave-uniform (DESIGN section
// 18, the hazard): past the last group, an invalid group (L outside [0, max_len] or any len_i outside
// [0, L]: all k are judged, there are no marks), a slab at or past L, a wave with no finding.  An
// invalid group's waves leave before they read, so its words stay as preset; k_var_invalid, one
// thread per group after k_locate_finish on the same stream, re-judges the k lengths, writes
// QFEC_LOC_INVALID over the finish's CLEAN and counts the group once.
//
// Two vector paths per wave, one ballot.  `full`: every data shard reaches the wave's whole columns;
// syndromes16 and the cold branch of k_locate_ptrs unchanged.  Any other wave is ragged: the data
// columns come through ld16_ragged / lane_part with `safe` = parity shard 0 (whole in every whole
// column below L), rolled in ragged_chunk passes so that the ragged body does not set the kernel's
// registers.  The runtime-k,m kernels clip with ld16_clip instead.
//
// The beyond-length rule (locate).  A data shard is known to be zero from len_i on, so it cannot be
// wrong there: shard i stays a candidate only if every syndrome is zero in every byte >= len_i.  Byte
// body: lane-local, a byte b with a non-zero syndrome drops every i with len_i <= b (no ballot, no
// shuffle: the body runs in loops whose trip count differs from lane to lane).  Vector cold branch:
// the lane drops i when the highest byte of its column with any non-zero syndrome lies at or past
// len_i.  A full wave never drops one: every len_i is past its columns.
//
// Alignment is judged per group on the entries the call may dereference: not the data shards of
// length 0.  The tail bytes of an aligned group and every byte of a misaligned one run the byte body,
// byte b of data shard i being b < len_i ? load : 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/qfec.h"
#include "qfec_internal.hpp"
#include "qfec_device.hpp"
#include "qfec_geom.hpp"
#include "qfec_ptrs_device.hpp"

namespace qfec {

// check_byte with lengths: len(c) = the length of data shard c.  LOC: a byte with a non-zero syndrome
// also drops every candidate that ends at or before it.
template <int K, bool LOC, class Row, class Len>
__device__ __forceinline__ void check_byte_var(int k, int m, const uint32_t* tab, const uint32_t* rtab, const Row& row,
                                               const Len& len, uint32_t b, uint32_t& bad, uint32_t& cand) {
    uint32_t x[K > 0 ? K : 1];
    if constexpr (K > 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) x[c] = b < len(c) ? (uint32_t)as_row(row(c))[b] : 0u;
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
#pragma unroll 1
            for (int c = 0; c < k; ++c) {
                const uint32_t* tc = tr + c * QFEC_TAB_STRIDE;
                const uint32_t xb = b < len(c) ? (uint32_t)as_row(row(c))[b] : 0u;
                s ^= gf_mul4(gf_sel(xb), tc[0], tc[1], tc[2], tc[3], tc[4]);
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
    if constexpr (LOC) {
        if (here != 0) {
#pragma unroll 1
            for (int i = 0; i < k; ++i)
                if (len(i) <= b) cand &= ~(1u << i);
        }
    }
    bad |= here;
}

// syndromes16 on a ragged wave: len(c) = the length of data shard c (c wave-uniform, not a
// constant), which lane c holds; safe: parity shard 0; part: lane_part's.  The parity columns are
// the accumulators' first value.
template <int K, int M, class Len>
__device__ __forceinline__ void syndromes16_ragged(uint4 (&s)[M], uint64_t p, const Len& len, const uint32_t (&part)[4],
                                                   const uint32_t* tab, uint32_t off) {
    constexpr int CH = ragged_chunk<K, 8>();
    const uint8_t* safe = as_row(lane_value(p, K));
#pragma unroll
    for (int r = 0; r < M; ++r) s[r] = ld16(as_row(lane_value(p, K + r)) + off);
#pragma unroll 1
    for (int c0 = 0; c0 < K; c0 += CH) {
        uint4 x[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) x[i] = ld16_ragged(as_row(lane_value(p, c0 + i)), safe, off, len(c0 + i), part, c0 + i);
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            Sel sl[4];
            sel16(sl, x[i]);
#pragma unroll
            for (int r = 0; r < M; ++r) gf_mac16(s[r], sl, tab + (r * K + c0 + i) * QFEC_TAB_STRIDE);
        }
    }
}

// the highest byte (0..15) of a non-zero 16-byte value that is not zero
__device__ __forceinline__ uint32_t top_byte16(const uint4& o) {
    const uint32_t w = o.w ? 3u : o.z ? 2u : o.y ? 1u : 0u;
    const uint32_t v = o.w ? o.w : o.z ? o.z : o.y ? o.y : o.x;
    return 4u * w + (31u - (uint32_t)__builtin_clz(v)) / 8u;
}

// lane s < k + m: address s of group g, lane i < k: length i as well (as unsigned: a negative length
// is above every L); the rest zero
__device__ __forceinline__ void lane_row_len(const uint64_t* __restrict__ dptrs, const uint64_t* __restrict__ pptrs,
                                             const int32_t* __restrict__ lens, uint64_t g, int k, int m, int lane,
                                             uint64_t* p, uint32_t* len) {
    *p = 0;
    *len = 0;
    if (lane < k) {
        *p = dptrs[g * (uint64_t)k + lane];
        *len = (uint32_t)lens[g * (uint64_t)k + lane];
    } else if (lane < k + m) {
        *p = pptrs[g * (uint64_t)m + (lane - k)];
    }
}

// What the lane-held kernels share once the loads are issued.  false: the wave leaves (an invalid or
// empty group, a slab at or past L); wave-uniform.
struct VarJudged {
    PtrsVarGeom v;
    uint32_t L;
    bool aligned, full;
};

__device__ __forceinline__ bool var_judge(const IntegrityPtrsVarArgs& a, uint64_t g, uint32_t slab, int lane, int k,
                                          uint64_t p, uint32_t len, const int32_t* __restrict__ glen, VarJudged* j) {
    const uint32_t L = (uint32_t)glen[g];
    if (L > a.p.block || __ballot(lane < k && len > L)) return false;  // invalid: nothing read
    j->L = L;
    j->v = ptrs_var_geom(L, 16);
    if (slab >= j->v.live) return false;  // an empty group, or a slab at or past L
    j->aligned = __ballot((p & 15u) != 0 && (lane >= k || len != 0)) == 0;
    j->full = __ballot(lane < k && len < slab_reach<16>(j->v, slab)) == 0;
    return true;
}

// ------------------------------------------------------------------ verify

template <int K, int M>
__global__ void __launch_bounds__(256) k_verify_ptrs_var(IntegrityPtrsVarArgs a, const uint64_t* __restrict__ dptrs,
                                                         const uint64_t* __restrict__ pptrs,
                                                         const int32_t* __restrict__ lens,
                                                         const int32_t* __restrict__ glen,
                                                         const uint32_t* __restrict__ tab) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a.p, &g, &slab)) return;
    uint64_t p;
    uint32_t len;
    lane_row_len(dptrs, pptrs, lens, g, K, M, lane, &p, &len);
    VarJudged j;
    if (!var_judge(a, g, slab, lane, K, p, len, glen, &j)) return;
    const auto len_of = [&](int c) { return lane_value32(len, c); };
    uint32_t part[4];
    if (j.aligned && !j.full) lane_part<4>(part, lane < K, p, len, slab);
    uint32_t bad = 0, none = 0;
    run_slab_var<16>(
        j.v, j.L, slab, lane, j.aligned,
        [&](uint32_t off) {
            uint4 s[M];
            if (j.full) {
                syndromes16<K, M>(s, p, tab, off);
#pragma unroll
                for (int r = 0; r < M; ++r)
                    if (nonzero16(s[r])) bad |= 1u << r;
            } else {
                syndromes16_ragged<K, M>(s, p, len_of, part, tab, off);
#pragma unroll
                for (int r = 0; r < M; ++r)
                    if (nonzero16(s[r])) bad |= 1u << r;
            }
        },
        [&](uint32_t b) {
            check_byte_var<K, false>(K, M, tab, nullptr, [&](int s) { return lane_value(p, s); }, len_of, b, bad, none);
        });
    if (__ballot(bad != 0) == 0) return;  // the whole wave is consistent
    flat_report<false>(a.p.bad_rows, nullptr, a.p.bad_groups, K, M, (uint32_t)g, bad, 0);
}

// runtime k, m (k + m may pass 64 lanes): addresses and lengths are read from the tables where they
// are used; the lanes stride over the group's entries for the judgement.  Rows in chunks of VCH, the
// k inputs re-read per chunk (cache hits), clipped unless the wave is full.
constexpr int VCH = 4;

__global__ void __launch_bounds__(256) k_verify_ptrs_var_any(IntegrityPtrsVarArgs a, const uint64_t* __restrict__ dptrs,
                                                             const uint64_t* __restrict__ pptrs,
                                                             const int32_t* __restrict__ lens,
                                                             const int32_t* __restrict__ glen,
                                                             const uint32_t* __restrict__ tab) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a.p, &g, &slab)) return;
    const int k = a.p.k, m = a.p.m;
    const uint64_t* dp = dptrs + g * (uint64_t)k;
    const uint64_t* pp = pptrs + g * (uint64_t)m;
    const int32_t* ln = lens + g * (uint64_t)k;
    const uint32_t L = (uint32_t)glen[g];
    uint32_t low = 0, longest = 0, shortest = 0xFFFFFFFFu;
    for (int i = lane; i < k; i += 64) {
        const uint32_t l = (uint32_t)ln[i];
        const uint32_t q = (uint32_t)dp[i] & 15u;
        longest = std::max(longest, l);
        shortest = std::min(shortest, l);
        if (l) low |= q;
    }
    for (int i = lane; i < m; i += 64) low |= (uint32_t)pp[i] & 15u;
    if (L > a.p.block || __ballot(longest > L)) return;  // invalid: nothing read
    const PtrsVarGeom v = ptrs_var_geom(L, 16);
    if (slab >= v.live) return;
    const bool aligned = __ballot(low != 0) == 0;
    const bool full = __ballot(shortest < slab_reach<16>(v, slab)) == 0;
    uint32_t bad = 0, none = 0;
    run_slab_var<16>(
        v, L, slab, lane, aligned,
        [&](uint32_t off) {
            for (int r0 = 0; r0 < m; r0 += VCH) {
                uint4 par[VCH], acc[VCH];
#pragma unroll
                for (int q = 0; q < VCH; ++q) {
                    par[q] = acc[q] = make_uint4(0, 0, 0, 0);
                    if (r0 + q < m) par[q] = ld16(as_row(pp[r0 + q]) + off);
                }
                for (int c = 0; c < k; ++c) {
                    uint4 x;
                    if (full) x = ld16(as_row(dp[c]) + off);
                    else x = ld16_clip(as_row(dp[c]), off, (uint32_t)ln[c]);
                    Sel s[4];
                    sel16(s, x);
#pragma unroll
                    for (int q = 0; q < VCH; ++q)
                        if (r0 + q < m) gf_mac16(acc[q], s, tab + ((r0 + q) * k + c) * QFEC_TAB_STRIDE);
                }
#pragma unroll
                for (int q = 0; q < VCH; ++q)
                    if (r0 + q < m && !same16(acc[q], par[q])) bad |= 1u << (r0 + q);
            }
        },
        [&](uint32_t b) {
            check_byte_var<0, false>(k, m, tab, nullptr, [&](int s) { return s < k ? dp[s] : pp[s - k]; },
                                     [&](int c) { return (uint32_t)ln[c]; }, b, bad, none);
        });
    if (__ballot(bad != 0) == 0) return;
    flat_report<false>(a.p.bad_rows, nullptr, a.p.bad_groups, k, m, (uint32_t)g, bad, 0);
}

// ------------------------------------------------------------------ locate

template <int K, int M>
__global__ void __launch_bounds__(256) k_locate_ptrs_var(IntegrityPtrsVarArgs a, const uint64_t* __restrict__ dptrs,
                                                         const uint64_t* __restrict__ pptrs,
                                                         const int32_t* __restrict__ lens,
                                                         const int32_t* __restrict__ glen,
                                                         const uint32_t* __restrict__ tab,
                                                         const uint32_t* __restrict__ rtab) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a.p, &g, &slab)) return;
    uint64_t p;
    uint32_t len;
    lane_row_len(dptrs, pptrs, lens, g, K, M, lane, &p, &len);
    VarJudged j;
    if (!var_judge(a, g, slab, lane, K, p, len, glen, &j)) return;
    const auto len_of = [&](int c) { return lane_value32(len, c); };
    uint32_t part[4];
    if (j.aligned && !j.full) lane_part<4>(part, lane < K, p, len, slab);
    uint4 s[M];  // the syndromes of the lane's whole column, if it has one
#pragma unroll
    for (int r = 0; r < M; ++r) s[r] = make_uint4(0, 0, 0, 0);
    uint32_t vbad = 0, bbad = 0, cand = 0xFFFFFFFFu;
    run_slab_var<16>(
        j.v, j.L, slab, lane, j.aligned,
        [&](uint32_t off) {
            if (j.full) syndromes16<K, M>(s, p, tab, off);
            else syndromes16_ragged<K, M>(s, p, len_of, part, tab, off);
#pragma unroll
            for (int r = 0; r < M; ++r)
                if (nonzero16(s[r])) vbad |= 1u << r;
        },
        [&](uint32_t b) {
            check_byte_var<K, true>(K, M, tab, rtab, [&](int i) { return lane_value(p, i); }, len_of, b, bbad, cand);
        });
    const uint32_t bad = vbad | bbad;
    if (__ballot(bad != 0) == 0) return;  // the whole wave is consistent: verify's cost
    if (vbad != 0) {                      // k_locate_ptrs' cold branch, after every load
        Sel s0[4];
        sel16(s0, s[0]);
        uint32_t vc = 0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            bool ok = true;
#pragma unroll
            for (int r = 1; r < M; ++r) ok = ok && ratio_holds(s0, s[r], rtab + (i * (M - 1) + r - 1) * QFEC_TAB_STRIDE);
            if (ok) vc |= 1u << i;
        }
        if (!j.full) {  // the beyond-length rule on the lane's own column
            uint4 o = s[0];
#pragma unroll
            for (int r = 1; r < M; ++r) {
                o.x |= s[r].x;
                o.y |= s[r].y;
                o.z |= s[r].z;
                o.w |= s[r].w;
            }
            const uint32_t top = (slab * 64u + lane) * 16u + top_byte16(o);
#pragma unroll 1
            for (int i = 0; i < K; ++i)
                if (len_of(i) <= top) vc &= ~(1u << i);
        }
        cand &= vc;
    }
    flat_report<true>(a.p.bad_rows, a.p.cand, nullptr, K, M, (uint32_t)g, bad, cand);
}

// runtime k, m (k + m <= 64, so the lanes hold the addresses and lengths); rows in chunks of WCH with
// k_locate_ptrs_any's rule for s_0.  The beyond-length rule runs per chunk on the chunk's own
// syndromes: what the chunks drop together is what the column's highest non-zero byte drops.
constexpr int WCH = 4;

__global__ void __launch_bounds__(256) k_locate_ptrs_var_any(IntegrityPtrsVarArgs a, const uint64_t* __restrict__ dptrs,
                                                             const uint64_t* __restrict__ pptrs,
                                                             const int32_t* __restrict__ lens,
                                                             const int32_t* __restrict__ glen,
                                                             const uint32_t* __restrict__ tab,
                                                             const uint32_t* __restrict__ rtab) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a.p, &g, &slab)) return;
    const int k = a.p.k, m = a.p.m;
    uint64_t p;
    uint32_t len;
    lane_row_len(dptrs, pptrs, lens, g, k, m, lane, &p, &len);
    VarJudged j;
    if (!var_judge(a, g, slab, lane, k, p, len, glen, &j)) return;
    const auto len_of = [&](int c) { return lane_value32(len, c); };
    uint32_t bad = 0, cand = 0xFFFFFFFFu;
    run_slab_var<16>(
        j.v, j.L, slab, lane, j.aligned,
        [&](uint32_t off) {
            uint4 s0 = make_uint4(0, 0, 0, 0);
            uint32_t vbad = 0;
            for (int r0 = 0; r0 < m; r0 += WCH) {
                uint4 par[WCH], s[WCH];
#pragma unroll
                for (int q = 0; q < WCH; ++q) {
                    par[q] = s[q] = make_uint4(0, 0, 0, 0);
                    if (r0 + q < m) par[q] = ld16(as_row(lane_value(p, k + r0 + q)) + off);
                }
                for (int c = 0; c < k; ++c) {
                    uint4 x;
                    if (j.full) x = ld16(as_row(lane_value(p, c)) + off);
                    else x = ld16_clip(as_row(lane_value(p, c)), off, len_of(c));
                    Sel sl[4];
                    sel16(sl, x);
#pragma unroll
                    for (int q = 0; q < WCH; ++q)
                        if (r0 + q < m) gf_mac16(s[q], sl, tab + ((r0 + q) * k + c) * QFEC_TAB_STRIDE);
                }
                uint4 o = make_uint4(0, 0, 0, 0);
#pragma unroll
                for (int q = 0; q < WCH; ++q) {
                    xor16(s[q], par[q]);
                    if (nonzero16(s[q])) vbad |= 1u << (r0 + q);  // rows past m are zero
                    o.x |= s[q].x;
                    o.y |= s[q].y;
                    o.z |= s[q].z;
                    o.w |= s[q].w;
                }
                if (r0 == 0) s0 = s[0];
                if (vbad != 0) {  // cold, after the chunk's loads
                    Sel sl[4];
                    sel16(sl, s0);
                    for (int i = 0; i < k; ++i) {
                        bool ok = true;
#pragma unroll
                        for (int q = 0; q < WCH; ++q) {
                            const int row = r0 + q;
                            if (row >= 1 && row < m)
                                ok = ok && ratio_holds(sl, s[q], rtab + (i * (m - 1) + row - 1) * QFEC_TAB_STRIDE);
                        }
                        if (!ok) cand &= ~(1u << i);
                    }
                    if (!j.full && nonzero16(o)) {
                        const uint32_t top = off + top_byte16(o);
                        for (int i = 0; i < k; ++i)
                            if (len_of(i) <= top) cand &= ~(1u << i);
                    }
                }
            }
            bad |= vbad;
        },
        [&](uint32_t b) {
            check_byte_var<0, true>(k, m, tab, rtab, [&](int i) { return lane_value(p, i); }, len_of, b, bad, cand);
        });
    if (__ballot(bad != 0) == 0) return;
    flat_report<true>(a.p.bad_rows, a.p.cand, nullptr, k, m, (uint32_t)g, bad, cand);
}

// ------------------------------------------------------------------ invalid groups

// One thread per group, after the finish (locate) or the main kernel (verify) on the same stream:
// the k lengths and L judged again.  An invalid group's words are still as preset (its waves left
// before they read), so its bad_rows word is 0 and the finish wrote CLEAN and zero marks; here the
// verdict becomes QFEC_LOC_INVALID and the group is counted, once.
__global__ void __launch_bounds__(256) k_var_invalid(VarInvalidArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    int verdict = -1;  // also for threads past the last group
    if (g < a.groups) {
        const uint32_t L = (uint32_t)a.group_len[g];
        bool bad = L > a.max_len;
        const int32_t* ln = a.lens + g * (uint64_t)a.k;
        for (int i = 0; i < a.k && !bad; ++i) bad = (uint32_t)ln[i] > L;
        if (bad) {
            verdict = 0;
            if (a.culprit) a.culprit[g] = QFEC_LOC_INVALID;
        }
    }
    if (a.invalid) block_counts<1>(verdict, a.invalid);  // uniform over the grid
}

// ------------------------------------------------------------------ correction

// One located shard per group, fixed from one parity row: no plan.  cul = d_culprit[g] is a scalar load,
// wave-uniform but not a constant; one body with runtime k, m covers every code the locate takes (k,
// m <= 32: the lanes hold addresses and lengths).  A data culprit i: (parity_0 ^ sum_{c != i}
// rows[0][c] x data_c) / rows[0][i], written over exactly [0, len_i); the other data are read clipped
// to their lengths, parity 0 is whole wherever a column below len_i <= L is.  A parity culprit j: sum_c
// rows[j][c] x data_c over exactly [0, L), a true product.  1 / rows[0][i]: the coefficient's log is
// dword 6 of its encode table, exp[255 - log] its inverse, whose perm table t256 holds.  The wave
// leaves, wave-uniformly, on a negative verdict or when its slab starts at or past the writable
// length; whole 16-B columns below it go by vector stores, the tail byte by byte, and a group with a
// misaligned entry among those it dereferences runs byte by byte.  No store reaches the writable length.
__global__ void __launch_bounds__(256) k_correct_ptrs_var(IntegrityPtrsVarArgs a, const uint64_t* __restrict__ dptrs,
                                                          const uint64_t* __restrict__ pptrs,
                                                          const int32_t* __restrict__ lens,
                                                          const int32_t* __restrict__ glen,
                                                          const int32_t* __restrict__ culprit,
                                                          const uint32_t* __restrict__ tab,
                                                          const uint32_t* __restrict__ t256,
                                                          const uint8_t* __restrict__ gf_exp) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a.p, &g, &slab)) return;
    const int k = a.p.k, m = a.p.m;
    uint64_t p;
    uint32_t len;
    lane_row_len(dptrs, pptrs, lens, g, k, m, lane, &p, &len);
    const uint32_t L = (uint32_t)glen[g];
    const int cul = __builtin_amdgcn_readfirstlane(culprit[g]);
    if (cul < 0 || cul >= k + m) return;  // nothing located (an invalid group has QFEC_LOC_INVALID)
    if (L > a.p.block || __ballot(lane < k && len > L)) return;  // a verdict that is not the locate's own
    const bool is_data = cul < k;
    const uint32_t wl = is_data ? lane_value32(len, cul) : L;  // the culprit's writable length
    const PtrsVarGeom v = ptrs_var_geom(wl, 16);
    if (slab >= v.live) return;
    const int row = is_data ? 0 : cul - k;   // the parity row the correction uses
    const int src = is_data ? k : cul;       // the parity shard it dereferences
    const bool aligned = __ballot((p & 15u) != 0 && (lane < k ? len != 0 : lane == src)) == 0;
    const uint32_t* tr = tab + (row * k) * QFEC_TAB_STRIDE;
    // the last multiplier: 1 / rows[0][cul] (a parity culprit: 1, the identity table)
    const uint32_t lg = is_data ? tr[cul * QFEC_TAB_STRIDE + 6] & 0xFFu : 0u;
    const uint32_t* ti = t256 + (uint32_t)gf_exp[255u - lg] * QFEC_TAB_STRIDE;
    const uint8_t* par0 = as_row(lane_value(p, k));
    uint8_t* dst = as_out(lane_value(p, cul));
    run_slab_var<16>(
        v, wl, slab, lane, aligned,
        [&](uint32_t off) {
            uint4 acc = make_uint4(0, 0, 0, 0);
            if (is_data) acc = ld16(par0 + off);
            for (int c = 0; c < k; ++c) {
                if (c == cul) continue;
                const uint4 x = ld16_clip(as_row(lane_value(p, c)), off, lane_value32(len, c));
                Sel sl[4];
                sel16(sl, x);
                gf_mac16(acc, sl, tr + c * QFEC_TAB_STRIDE);
            }
            Sel sa[4];
            sel16(sa, acc);
            uint4 out = make_uint4(0, 0, 0, 0);
            gf_mac16(out, sa, ti);
            st16(dst + off, out);
        },
        [&](uint32_t b) {
            uint32_t acc = is_data ? (uint32_t)par0[b] : 0u;
#pragma unroll 1
            for (int c = 0; c < k; ++c) {
                if (c == cul) continue;
                const uint32_t* tc = tr + c * QFEC_TAB_STRIDE;
                const uint32_t xb = b < lane_value32(len, c) ? (uint32_t)as_row(lane_value(p, c))[b] : 0u;
                acc ^= gf_mul4(gf_sel(xb), tc[0], tc[1], tc[2], tc[3], tc[4]);
            }
            dst[b] = (uint8_t)gf_mul4(gf_sel(acc & 0xFFu), ti[0], ti[1], ti[2], ti[3], ti[4]);
        });
}

// ------------------------------------------------------------------ launchers

// blocks of four waves over groups * wpg waves, wpg from ptrs_geom(max_len, 16); false when the caller
// has to chunk or the geometry is not the one the kernels are built for
static inline bool integrity_var_grid(const IntegrityPtrsArgs& a, unsigned* grid) {
    const uint64_t waves = a.groups * (uint64_t)a.wpg;
    if (a.wpg == 0 || waves * 64 > (uint64_t)kMaxLaunchLanes) return false;
    if (a.block < 1 || a.block > 0x7FFFFFFFu || a.wpg != ptrs_geom((int)a.block, 16).wpg) return false;
    *grid = (unsigned)((waves + 3) / 4);
    return true;
}

#define QFEC_VVER_CASE(KK, MM)                                                                                       \
    if (a.p.k == KK && a.p.m == MM) {                                                                                \
        hipLaunchKernelGGL((k_verify_ptrs_var<KK, MM>), dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs,   \
                           a.lens, a.group_len, a.p.tab);                                                            \
        return hipGetLastError();                                                                                    \
    }

hipError_t launch_verify_ptrs_var(const IntegrityPtrsVarArgs& a, hipStream_t stream) {
    if (a.p.groups == 0 || a.p.m == 0) return hipSuccess;
    unsigned grid;
    if (a.p.m > 32 || !a.p.bad_rows || !a.p.tab || !a.lens || !a.group_len || !integrity_var_grid(a.p, &grid))
        return hipErrorInvalidValue;
    // qfec_integrity_ptrs.hip's instances
    QFEC_VVER_CASE(10, 3)
    QFEC_VVER_CASE(16, 4)
    QFEC_VVER_CASE(4, 2)
    QFEC_VVER_CASE(8, 4)
    hipLaunchKernelGGL(k_verify_ptrs_var_any, dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs, a.lens,
                       a.group_len, a.p.tab);
    return hipGetLastError();
}

#define QFEC_VLOC_CASE(KK, MM)                                                                                       \
    if (a.p.k == KK && a.p.m == MM) {                                                                                \
        hipLaunchKernelGGL((k_locate_ptrs_var<KK, MM>), dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs,   \
                           a.lens, a.group_len, a.p.tab, a.p.rtab);                                                  \
        return hipGetLastError();                                                                                    \
    }

hipError_t launch_locate_ptrs_var(const IntegrityPtrsVarArgs& a, hipStream_t stream) {
    if (a.p.groups == 0) return hipSuccess;
    unsigned grid;
    if (a.p.m < 2 || a.p.m > 32 || a.p.k > 32 || !a.p.bad_rows || !a.p.cand || !a.p.tab || !a.p.rtab || !a.lens ||
        !a.group_len || !integrity_var_grid(a.p, &grid))
        return hipErrorInvalidValue;  // caller chunks and checks the code
    QFEC_VLOC_CASE(10, 3)
    QFEC_VLOC_CASE(16, 4)
    QFEC_VLOC_CASE(4, 2)
    QFEC_VLOC_CASE(8, 4)
    hipLaunchKernelGGL(k_locate_ptrs_var_any, dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs, a.lens,
                       a.group_len, a.p.tab, a.p.rtab);
    return hipGetLastError();
}

hipError_t launch_correct_ptrs_var(const IntegrityPtrsVarArgs& a, const int32_t* culprit, const uint32_t* t256,
                                   const uint8_t* gf_exp, hipStream_t stream) {
    if (a.p.groups == 0) return hipSuccess;
    unsigned grid;
    if (a.p.m < 1 || a.p.m > 32 || a.p.k < 1 || a.p.k > 32 || !culprit || !t256 || !gf_exp || !a.p.tab || !a.lens ||
        !a.group_len || !integrity_var_grid(a.p, &grid))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_correct_ptrs_var, dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs, a.lens, a.group_len,
                       culprit, a.p.tab, t256, gf_exp);
    return hipGetLastError();
}

hipError_t launch_var_invalid(const VarInvalidArgs& a, hipStream_t stream) {
    if (a.groups == 0 || (!a.culprit && !a.invalid)) return hipSuccess;
    if (!a.lens || !a.group_len || a.groups > 0x7FFFFFFFull * 256u) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((a.groups + 255) / 256);
    hipLaunchKernelGGL(k_var_invalid, dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace qfec
