// qfec_locate_erased.hip -- which single SURVIVING shard of a group is corrupted, when the group
// also has lost shards?  (qfec_locate_erased / qfec_scrub_erased, gfx950)
//
// A group with t marked shards has S = m - t spare parity rows beyond the k lowest unmarked shards
// K that qfec_repair decodes from.  The record of the group's mask (qfec_locate_erased.cpp) gives
// the rows A_x that predict each spare from K, so s_x = spare_x ^ A_x . K are the syndromes of the
// code punctured at the marked shards.  An error in spare x0 alone leaves only s_x0 non-zero; an
// error in the shard at position c of K gives s_x = (A_x[c] / A_0[c]) x s_0 in every byte.
//
// Mapping: the repair body's (qfec_kernels.hip), not qfec_locate's flattened one, because the record
// must be wave-uniform: 8-B lanes, one wave per 64 columns of a group, one group per block where a
// group is at most 4 waves.  The mask is a ballot over the n marks; K's and the spares' row pointers
// follow from the mask alone, so the loads issue before the record arrives; the tables come through
// the constant address space (scalar loads).  The S products are formed by a wave-uniform dispatch
// on S, as the repair dispatches on t.  A wave with no non-zero syndrome ends there.
//
// Cold branch, as qfec_locate's: a lane with a non-zero syndrome tests every position of K with
// S - 1 ratio multiplies, the other lanes vote for everyone; the wave AND-reduces with ballots and
// one lane issues one atomic AND into the group's candidate word (bit c = position c of K, preset to
// all ones) and one atomic OR into its bad-spares word (preset to zero).  With one spare there is no
// ratio to test and every position stays a candidate.  k_locate_erased_finish maps positions back to
// shard ids through the record and writes the verdicts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qfec.h"
#include "qfec_internal.hpp"
#include "qfec_device.hpp"

namespace qfec {

// the wave's verdict on its columns into the group's two words.  Every lane of the wave calls it
// (all of them belong to group g); bad = this lane's syndrome bits, cand = the positions of K that
// explain them (all ones where bad is 0).
__device__ __forceinline__ void erased_report(unsigned int* bad_w, unsigned int* cand_w, uint64_t g, int k, int S,
                                              uint32_t bad, uint32_t cand) {
    uint32_t rows = 0, keep = 0;
    for (int x = 0; x < S; ++x)
        if (__ballot((bad >> x) & 1u)) rows |= 1u << x;
    for (int c = 0; c < k; ++c)
        if (!__ballot(!((cand >> c) & 1u))) keep |= 1u << c;
    if ((threadIdx.x & 63) == 0) {
        atomicOr(bad_w + g, rows);
        atomicAnd(cand_w + g, keep);
    }
}

// the n marks of group g as a mask, wave-uniform
__device__ __forceinline__ uint32_t erased_mask(const uint8_t* __restrict__ dmarks, const uint8_t* __restrict__ pmarks,
                                                uint64_t g, int k, int m, int lane) {
    uint32_t mk = 0;
    if (lane < k) mk = dmarks[g * (uint64_t)k + lane];
    else if (lane < k + m) mk = pmarks[g * (uint64_t)m + (lane - k)];
    return (uint32_t)(__ballot(mk != 0) & ((1ull << (k + m)) - 1ull));
}

// One 8-B (D = 2) column of a group with exactly S spares.  `live` is false for the lanes past the
// row's last column: they load nothing and vote for everyone.
template <int K, int S, int D>
__device__ __forceinline__ void erased_column_s(const LocErasedArgs& a, const uint8_t* const (&src)[K],
                                                const uint8_t* par_g, uint32_t spare_bits, const uint32_t* rec,
                                                uint64_t g, uint32_t col, bool live) {
    const RTab T{rec, a.aoff, a.t256};
    uint32_t bad = 0;
    uint32_t syn[S][D];
#pragma unroll
    for (int x = 0; x < S; ++x)
#pragma unroll
        for (int d = 0; d < D; ++d) syn[x][d] = 0;
    if (live) {
        const uint64_t off = (uint64_t)col * (4u * D);
        uint32_t v[K][D], p[S][D];
#pragma unroll
        for (int c = 0; c < K; ++c) ldv<D>(v[c], src[c] + off);
#pragma unroll
        for (int x = 0; x < S; ++x) {  // the spares are parity rows: ids >= K, ascending
            const uint32_t id = (uint32_t)__builtin_ctz(spare_bits);
            spare_bits &= spare_bits - 1;
            ldv<D>(p[x], par_g + (uint64_t)(id - K) * a.pitch + off);
        }
        recon_mac_core<K, S, D>(v, syn, T);
        const int nb = (int)a.block - (int)(col * (4u * D));  // bytes of this column inside block_size (may be <= 0)
#pragma unroll
        for (int x = 0; x < S; ++x) {
            uint32_t any = 0;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                syn[x][d] = (syn[x][d] ^ p[x][d]) & head_bytes(nb - 4 * d);
                any |= syn[x][d];
            }
            if (any) bad |= 1u << x;
        }
    }
    if (__ballot(bad != 0) == 0) return;  // the whole wave is consistent
    uint32_t cand = 0xFFFFFFFFu;
    if (S > 1 && bad != 0) {
        cptr32 roffs = (cptr32)rec + a.roff;
        Sel s0[D];
#pragma unroll
        for (int d = 0; d < D; ++d) s0[d] = gf_sel(syn[0][d]);
        cand = 0;
#pragma unroll
        for (int c = 0; c < K; ++c) {
            bool ok = true;
#pragma unroll
            for (int x = 1; x < S; ++x) {
                cptr32 t = (cptr32)((cptr8)T.t256 + roffs[c * (S - 1) + (x - 1)]);
                const uint32_t t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3], t4 = t[4];
#pragma unroll
                for (int d = 0; d < D; ++d) ok = ok && gf_mul4(s0[d], t0, t1, t2, t3, t4) == syn[x][d];
            }
            if (ok) cand |= 1u << c;
        }
    }
    erased_report(a.bad, a.cand, g, K, S, bad, cand);
}

// wave-uniform dispatch on the spare count to the exact-row-count body
template <int K, int M, int D, int S = M>
__device__ __forceinline__ void erased_column_by_s(const LocErasedArgs& a, const uint8_t* const (&src)[K],
                                                   const uint8_t* par_g, uint32_t spare_bits, const uint32_t* rec,
                                                   int s, uint64_t g, uint32_t col, bool live) {
    if constexpr (S > 1) {
        if (s < S) {
            erased_column_by_s<K, M, D, S - 1>(a, src, par_g, spare_bits, rec, s, g, col, live);
            return;
        }
    }
    erased_column_s<K, S, D>(a, src, par_g, spare_bits, rec, g, col, live);
}

// ONE: one group per block of wpg8 waves (wpg8 <= 4), else 4 waves per block over (group, slab)
template <int K, int M, bool ONE>
__global__ void __launch_bounds__(256) k_locate_erased_perm(LocErasedArgs a, const uint8_t* __restrict__ data,
                                                            const uint8_t* __restrict__ parity,
                                                            const uint8_t* __restrict__ dmarks,
                                                            const uint8_t* __restrict__ pmarks,
                                                            const int32_t* __restrict__ lut,
                                                            const uint32_t* __restrict__ records) {
    constexpr int N = K + M;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint64_t g;
    uint32_t part;
    if (ONE) {
        g = blockIdx.x;
        part = wave;
    } else {
        const uint32_t wid = blockIdx.x * 4u + wave;
        g = wid / a.wpg8;
        part = wid - (uint32_t)g * a.wpg8;
    }
    if (g >= a.groups) return;
    const uint32_t mask = erased_mask(dmarks, pmarks, g, K, M, lane);
    const int t = __builtin_popcount(mask);
    if (t >= M) return;  // no spare row (UNCHECKED) or under-determined (LOST): the finish kernel says so
    const int rec = ((const __attribute__((address_space(4))) int32_t*)lut)[mask];
    if (rec < 0) return;  // not reached: the host refuses codes that lack a record for some t < m
    const uint8_t* data_g = data + g * a.dgs;
    const uint8_t* par_g = parity + g * a.pgs;
    // K = the k lowest unmarked ids, the spares = the rest: both known from the mask alone
    uint32_t avail = ~mask & ((1u << N) - 1u);
    const uint8_t* src[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        const uint32_t s = (uint32_t)__builtin_ctz(avail);
        avail &= avail - 1;
        src[c] = s < (uint32_t)K ? data_g + (uint64_t)s * a.pitch : par_g + (uint64_t)(s - K) * a.pitch;
    }
    const uint32_t col = part * 64u + lane;
    erased_column_by_s<K, M, 2>(a, src, par_g, avail, records + rec, M - t, g, col, col < a.cols8);
}

// runtime k and spare count (every shape without an instance), and the byte path for layouts that
// are not 16-B aligned (D = 1: one byte per lane in the low byte of a dword).  One wave per group,
// column loop, spares in chunks of ECH; s_0 comes with the first chunk and stays, as in k_locate_any.
constexpr int ECH = 4;

template <int D>
__device__ __forceinline__ void erased_ld(uint32_t (&v)[D], const uint8_t* p) {
    if constexpr (D == 4) ldv<4>(v, p);
    else v[0] = *p;
}

template <int D>
__global__ void __launch_bounds__(256) k_locate_erased_any(LocErasedArgs a) {
    static_assert(D == 4 || D == 1, "16-B columns or bytes");
    const int lane = threadIdx.x & 63;
    const uint64_t g = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (g >= a.groups) return;
    const int k = a.k, m = a.m;  // k + m <= QFEC_LUT_MAX_N
    const uint32_t mask = erased_mask(a.dmarks, a.pmarks, g, k, m, lane);
    if (__builtin_popcount(mask) >= m) return;
    const int rec = __builtin_amdgcn_readfirstlane(a.lut[mask]);
    if (rec < 0) return;
    const uint32_t* __restrict__ r = a.records + rec;
    const int S = (int)r[0];
    const uint32_t* ids = r + a.ids_off;
    const uint32_t* aoffs = r + a.aoff;
    const uint32_t* roffs = r + a.roff;
    const uint8_t* data_g = a.data + g * a.dgs;
    const uint8_t* par_g = a.parity + g * a.pgs;
    auto row = [&](uint32_t s) -> const uint8_t* {
        return s < (uint32_t)k ? data_g + (uint64_t)s * a.pitch : par_g + (uint64_t)(s - k) * a.pitch;
    };
    uint32_t bad = 0, cand = 0xFFFFFFFFu;
    for (uint32_t base = 0; base < a.cols; base += 64) {  // wave-uniform
        const uint32_t col = base + lane;
        const bool live = col < a.cols;
        const uint64_t off = (uint64_t)col * (D == 4 ? 16u : 1u);
        uint32_t mk[D];
        if constexpr (D == 4) {
            const uint4 q = column_mask(a.block, live ? col : 0u);
            mk[0] = q.x; mk[1] = q.y; mk[2] = q.z; mk[3] = q.w;
        } else {
            mk[0] = 0xFFu;
        }
        uint32_t cbad = 0;  // this column's syndrome bits
        uint32_t s0[D];
#pragma unroll
        for (int d = 0; d < D; ++d) s0[d] = 0;
        for (int x0 = 0; x0 < S; x0 += ECH) {
            uint32_t s[ECH][D];
#pragma unroll
            for (int j = 0; j < ECH; ++j)
#pragma unroll
                for (int d = 0; d < D; ++d) s[j][d] = 0;
            if (live) {
                for (int c = 0; c < k; ++c) {
                    uint32_t v[D];
                    erased_ld<D>(v, row(ids[c]) + off);
                    Sel sl[D];
#pragma unroll
                    for (int d = 0; d < D; ++d) sl[d] = gf_sel(v[d]);
#pragma unroll
                    for (int j = 0; j < ECH; ++j)
                        if (x0 + j < S) {
                            const uint32_t* tc = a.t256 + (aoffs[(x0 + j) * k + c] >> 2);
#pragma unroll
                            for (int d = 0; d < D; ++d) s[j][d] ^= gf_mul4(sl[d], tc[0], tc[1], tc[2], tc[3], tc[4]);
                        }
                }
#pragma unroll
                for (int j = 0; j < ECH; ++j)
                    if (x0 + j < S) {
                        uint32_t p[D], any = 0;
                        erased_ld<D>(p, row(ids[k + x0 + j]) + off);
#pragma unroll
                        for (int d = 0; d < D; ++d) {
                            s[j][d] = (s[j][d] ^ p[d]) & mk[d];
                            any |= s[j][d];
                        }
                        if (any) cbad |= 1u << (x0 + j);
                    }
                if (x0 == 0) {
#pragma unroll
                    for (int d = 0; d < D; ++d) s0[d] = s[0][d];
                }
            }
            if (__ballot(cbad != 0) == 0) continue;  // nothing wrong in this wave's columns so far
            if (cbad != 0 && S > 1) {
                Sel sl[D];
#pragma unroll
                for (int d = 0; d < D; ++d) sl[d] = gf_sel(s0[d]);
                for (int i = 0; i < k; ++i) {
                    bool ok = true;
#pragma unroll
                    for (int j = 0; j < ECH; ++j) {
                        const int x = x0 + j;
                        if (x >= 1 && x < S) {
                            const uint32_t* tc = a.t256 + (roffs[i * (S - 1) + (x - 1)] >> 2);
#pragma unroll
                            for (int d = 0; d < D; ++d)
                                ok = ok && (gf_mul4(sl[d], tc[0], tc[1], tc[2], tc[3], tc[4]) & mk[d]) == s[j][d];
                        }
                    }
                    if (!ok) cand &= ~(1u << i);
                }
            }
        }
        bad |= cbad;
    }
    if (__ballot(bad != 0) == 0) return;
    erased_report(a.bad, a.cand, g, k, S, bad, cand);
}

// the verdict of group g from its marks and its two words.  Writes culprit and marks_out; returns the
// counter the group bumps (0 located, 1 multi, 2 ambiguous, 3 unchecked, 4 lost) or -1 for a clean one.
__device__ __forceinline__ int erased_verdict(const LocErasedFinishArgs& a, uint64_t g) {
    const int k = a.k, m = a.m;
    const uint8_t* dm = a.marks + g * (uint64_t)k;  // rs.c layout: every group's data marks, then the parity marks
    const uint8_t* pm = a.marks + a.groups * (uint64_t)k + g * (uint64_t)m;
    uint32_t mask = 0;
    for (int i = 0; i < k; ++i) mask |= dm[i] ? 1u << i : 0u;
    for (int j = 0; j < m; ++j) mask |= pm[j] ? 1u << (k + j) : 0u;
    const int t = __builtin_popcount(mask);
    int id = QFEC_LOC_CLEAN;
    if (t > m) {
        id = QFEC_LOC_LOST;
    } else if (t == m) {
        id = QFEC_LOC_UNCHECKED;
    } else if (a.bad[g] != 0) {
        const uint32_t bad = a.bad[g];
        const uint32_t kc = a.cand[g] & ((1u << k) - 1u);  // k <= 23
        // the candidates: the positions of K that survived every column, plus spare x0 iff it is the only bad one
        const int nc = __builtin_popcount(kc) + (__builtin_popcount(bad) == 1 ? 1 : 0);
        if (nc == 0) {
            id = QFEC_LOC_MULTI;
        } else if (nc > 1) {
            id = QFEC_LOC_AMBIGUOUS;
        } else {
            const uint32_t* ids = a.records + a.lut[mask] + a.ids_off;
            id = (int)(kc ? ids[__builtin_ctz(kc)] : ids[k + __builtin_ctz(bad)]);
        }
    }
    if (a.culprit) a.culprit[g] = id;
    if (a.marks_out) {
        // the input marks as 0 / 1, plus the culprit; for qfec_scrub_erased nothing in a group that
        // must stay as it is (marks_out may be marks: this lane alone touches group g's bytes)
        if (a.scrub && (id == QFEC_LOC_MULTI || id == QFEC_LOC_AMBIGUOUS)) mask = 0;
        if (id >= 0) mask |= 1u << id;
        write_marks_rs(a.marks_out, a.groups, g, k, m, mask);
    }
    return id >= 0 ? 0 : id == QFEC_LOC_CLEAN ? -1 : -id - 1;  // MULTI -2 -> 1 ... LOST -5 -> 4
}

// one lane per group, after the last chunk
__global__ void __launch_bounds__(256) k_locate_erased_finish(LocErasedFinishArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    int verdict = -1;  // also for lanes past the last group
    if (g < a.groups) verdict = erased_verdict(a, g);
    if (a.counts) block_counts<5>(verdict, a.counts);  // uniform over the grid
}

// the repair's instances with m >= 2, the same launch shapes (qfec_kernels.hip, launch_repair)
#define QFEC_LE_CASE(KK, MM)                                                                                         \
    if (a.k == KK && a.m == MM) {                                                                                    \
        if (a.wpg8 <= 4)                                                                                             \
            hipLaunchKernelGGL((k_locate_erased_perm<KK, MM, true>), dim3((unsigned)a.groups), dim3(64u * a.wpg8), 0, \
                               stream, a, a.data, a.parity, a.dmarks, a.pmarks, a.lut, a.records);                   \
        else                                                                                                         \
            hipLaunchKernelGGL((k_locate_erased_perm<KK, MM, false>),                                                \
                               dim3((unsigned)((a.groups * (uint64_t)a.wpg8 + 3) / 4)), dim3(256), 0, stream, a,     \
                               a.data, a.parity, a.dmarks, a.pmarks, a.lut, a.records);                              \
        return hipGetLastError();                                                                                    \
    }

hipError_t launch_locate_erased(const LocErasedArgs& a, hipStream_t stream) {
    if (a.groups == 0) return hipSuccess;
    if (a.m < 2 || a.k < 1 || a.k + a.m > QFEC_LUT_MAX_N || a.wpg8 < 1 || !a.bad || !a.cand || !a.lut || !a.records ||
        !a.t256)
        return hipErrorInvalidValue;  // the caller checks the code
    if (a.groups * (uint64_t)a.wpg8 > 0x7FFFFFFFull) return hipErrorInvalidValue;  // the caller chunks
    const unsigned grid = (unsigned)((a.groups + 3) / 4);
    if (!a.vec16) {
        hipLaunchKernelGGL((k_locate_erased_any<1>), dim3(grid), dim3(256), 0, stream, a);
        return hipGetLastError();
    }
    QFEC_LE_CASE(10, 3)
    QFEC_LE_CASE(16, 4)
    QFEC_LE_CASE(4, 2)
    QFEC_LE_CASE(3, 2)
    QFEC_LE_CASE(8, 4)
    QFEC_LE_CASE(12, 4)
    QFEC_LE_CASE(5, 3)
    QFEC_LE_CASE(6, 2)
    QFEC_LE_CASE(8, 2)
    QFEC_LE_CASE(20, 4)
    hipLaunchKernelGGL((k_locate_erased_any<4>), dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_locate_erased_finish(const LocErasedFinishArgs& a, hipStream_t stream) {
    if (a.groups == 0) return hipSuccess;
    if (!a.marks || !a.lut || !a.records || !a.bad || !a.cand || a.groups > 0x7FFFFFFFull * 256u)
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((a.groups + 255) / 256);
    hipLaunchKernelGGL(k_locate_erased_finish, dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace qfec
