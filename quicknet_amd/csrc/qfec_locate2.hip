// qfec_locate2.hip -- which TWO shards of a group are corrupted?  (qfec_locate2 / qfec_scrub2, gfx950)
//
// Stage 1 is qfec_locate as it stands (qfec_locate.hip): it settles the consistent groups and the
// groups with one corrupted shard at qfec_verify's cost, and calls the rest MULTI.  The three
// kernels here run after it on the same stream:
//
//   k_locate2_list    one lane per group: the MULTI groups are appended to a compact list.  A block
//                     sums its hits in LDS and takes its span of the list with one atomic add.
//   k_locate2_pairs   a fixed grid of one-wave blocks strides over the list; the bound is read from
//                     the list's counter, so nothing waits on the host.  Per listed group the wave
//                     walks the group's columns 64 at a time: each lane recomputes the m syndromes of
//                     its column (the encode's perm tables, as k_locate_*), then every pair {a, b}
//                     still alive is tested: F_ab x s == 0, F_ab the (m - 2) x m left null space of
//                     [h_a h_b] with its entries as table offsets (wave-uniform loads through the
//                     constant address space; a zero entry is skipped, an entry 1 is an XOR of the
//                     syndrome itself, so a check of two data shards is two multiplies).  One ballot
//                     per pair turns the lanes' answers into one bit of a wave-uniform bitset; a dead
//                     pair is not tested again.
//   k_locate2_finish  one lane per group, every group: the two slots, the marks, the four counters.
//
// The templated instances keep the m syndromes and their selectors in registers; the runtime-(k, m)
// kernel and the byte kernel keep the syndromes in LDS, one slot per lane and row, read back by the
// lane that wrote them (no barrier), because m is not known when they are compiled.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/qfec.h"
#include "qfec_internal.hpp"
#include "qfec_device.hpp"

namespace qfec {

constexpr int L2_WORDS = (QFEC_LOC2_MAX_N * (QFEC_LOC2_MAX_N - 1) / 2 + 31) / 32;
constexpr unsigned L2_MAX_GRID = 4096;  // one-wave blocks of the pair kernel: 16 per CU
constexpr uint32_t L2_ONE = 1 * QFEC_TAB_STRIDE * 4;  // the offset of the coefficient 1: no multiply

__device__ __forceinline__ bool nonzero(const uint4& s) { return (s.x | s.y | s.z | s.w) != 0; }
__device__ __forceinline__ bool nonzero(uint32_t s) { return (s & 0xFFu) != 0; }

__device__ __forceinline__ void xor_into(uint4& v, const uint4& s) {
    v.x ^= s.x;
    v.y ^= s.y;
    v.z ^= s.z;
    v.w ^= s.w;
}
__device__ __forceinline__ void xor_into(uint32_t& v, uint32_t s) { v ^= s; }

// v ^= c x s, t = the perm table of c
__device__ __forceinline__ void mac_const(uint4& v, const Sel (&s)[4], cptr32 t) {
    const uint32_t t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3], t4 = t[4];
    v.x = xor3(v.x, pp0(s[0], t0, t1), pp1(s[0], t2, t3)) ^ pp2(s[0], t4);
    v.y = xor3(v.y, pp0(s[1], t0, t1), pp1(s[1], t2, t3)) ^ pp2(s[1], t4);
    v.z = xor3(v.z, pp0(s[2], t0, t1), pp1(s[2], t2, t3)) ^ pp2(s[2], t4);
    v.w = xor3(v.w, pp0(s[3], t0, t1), pp1(s[3], t2, t3)) ^ pp2(s[3], t4);
}
__device__ __forceinline__ void mac_const(uint4& v, const uint4& s, cptr32 t) {
    Sel sl[4];
    sel16(sl, s);
    mac_const(v, sl, t);
}
__device__ __forceinline__ void mac_const(uint32_t& v, uint32_t s, cptr32 t) {
    v ^= gf_mul4(gf_sel(s), t[0], t[1], t[2], t[3], t[4]);
}

// every pair alive: bit p of the bitset for p < pairs
template <int NW>
__device__ __forceinline__ void all_pairs(uint32_t (&alive)[NW], int pairs) {
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int left = pairs - 32 * w;
        alive[w] = left >= 32 ? 0xFFFFFFFFu : left <= 0 ? 0u : (1u << left) - 1u;
    }
}

// the verdict of one listed group from its surviving pairs
template <int NW>
__device__ __forceinline__ int pair_verdict(const uint32_t (&alive)[NW], const uint32_t* pair_ids) {
    int count = 0, first = 0;
#pragma unroll
    for (int w = NW - 1; w >= 0; --w) {
        count += __builtin_popcount(alive[w]);
        if (alive[w]) first = 32 * w + __builtin_ctz(alive[w]);
    }
    return count == 0 ? QFEC_LOC_MULTI : count > 1 ? QFEC_LOC_AMBIGUOUS : (int)pair_ids[first];
}

// compile-time K, M: the column's syndromes and their selectors stay in registers
template <int K, int M>
__global__ void __launch_bounds__(64) k_locate2_pairs(Locate2Args a) {
    constexpr int NP = (K + M) * (K + M - 1) / 2, NW = (NP + 31) / 32;
    const uint32_t lane = threadIdx.x;
    const uint32_t listed = (uint32_t)std::min<uint64_t>(*a.list_n, a.groups);
    const cptr32 chk = (cptr32)a.checks;
    const cptr8 t256 = (cptr8)a.t256;
    for (uint32_t e = blockIdx.x; e < listed; e += gridDim.x) {  // wave-uniform
        const uint64_t g = a.list[e];
        uint32_t alive[NW];
        all_pairs(alive, NP);
        for (uint32_t c0 = 0; c0 < a.cols; c0 += 64) {
            const uint32_t col = c0 + lane;
            Sel s[M][4];
            uint4 acc[M];  // the products, then the syndromes
            bool bad = false;
#pragma unroll
            for (int r = 0; r < M; ++r) acc[r] = make_uint4(0, 0, 0, 0);
            if (col < a.cols) {
                const uint8_t* src = a.data + g * a.dgs + (uint64_t)col * 16u;
                const uint8_t* par = a.parity + g * a.pgs + (uint64_t)col * 16u;
                uint4 p[M];
#pragma unroll
                for (int r = 0; r < M; ++r) p[r] = ld16(par + (uint64_t)r * a.pitch);
                products16<K, M>(acc, src, a.pitch, a.tab);
                const uint4 mk = column_mask(a.block, col);
#pragma unroll
                for (int r = 0; r < M; ++r) {
                    acc[r] = make_uint4((acc[r].x ^ p[r].x) & mk.x, (acc[r].y ^ p[r].y) & mk.y,
                                        (acc[r].z ^ p[r].z) & mk.z, (acc[r].w ^ p[r].w) & mk.w);
                    bad = bad || nonzero(acc[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < M; ++r) sel16(s[r], acc[r]);
            if (__ballot(bad) == 0) continue;  // these columns are consistent: every pair explains them
            uint32_t left = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                uint32_t todo = alive[w];
                while (todo) {  // wave-uniform
                    const int b = __builtin_ctz(todo);
                    todo &= todo - 1;
                    const cptr32 rec = chk + (32 * w + b) * ((M - 2) * M);
                    bool fail = false;
#pragma unroll
                    for (int r = 0; r < M - 2; ++r) {
                        uint4 v = make_uint4(0, 0, 0, 0);
#pragma unroll
                        for (int j = 0; j < M; ++j) {
                            const uint32_t off = rec[r * M + j];
                            if (off == L2_ONE) xor_into(v, acc[j]);
                            else if (off) mac_const(v, s[j], (cptr32)(t256 + off));
                        }
                        fail = fail || nonzero(v);
                    }
                    if (__ballot(fail)) alive[w] &= ~(1u << b);
                }
                left |= alive[w];
            }
            if (!left) break;
        }
        const int verdict = pair_verdict(alive, a.pair_ids);
        if (lane == 0) a.verdict2[g] = verdict;
    }
}

// runtime k, m.  W = uint4: one lane per 16-B column, rows in chunks of 4 as k_locate_any;
// W = uint32_t: one lane per byte of [0, block_size), for layouts that are not 16-B aligned.
// Dynamic LDS: m x 64 x sizeof(W), slot [row][lane].
template <class W>
__global__ void __launch_bounds__(64) k_locate2_pairs_any(Locate2Args a) {
    extern __shared__ uint4 l2_lds[];
    constexpr bool VEC = std::is_same<W, uint4>::value;
    W* synd = reinterpret_cast<W*>(l2_lds);
    const uint32_t lane = threadIdx.x;
    const int k = a.k, m = a.m;
    const uint32_t listed = (uint32_t)std::min<uint64_t>(*a.list_n, a.groups);
    const cptr32 chk = (cptr32)a.checks;
    const cptr8 t256 = (cptr8)a.t256;
    for (uint32_t e = blockIdx.x; e < listed; e += gridDim.x) {  // wave-uniform
        const uint64_t g = a.list[e];
        uint32_t alive[L2_WORDS];
        all_pairs(alive, a.pairs);
        for (uint32_t c0 = 0; c0 < a.cols; c0 += 64) {
            const uint32_t col = c0 + lane;
            const bool live = col < a.cols;
            bool bad = false;
            if constexpr (VEC) {
                const uint8_t* src = a.data + g * a.dgs + (uint64_t)col * 16u;
                const uint8_t* par = a.parity + g * a.pgs + (uint64_t)col * 16u;
                const uint4 mk = column_mask(a.block, live ? col : 0u);
                for (int r0 = 0; r0 < m; r0 += 4) {
                    uint4 acc[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = make_uint4(0, 0, 0, 0);
                    if (live) {
                        products16_rows<4>(acc, src, a.pitch, a.tab, k, m, r0);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (r0 + j < m) {
                                const uint4 p = ld16(par + (uint64_t)(r0 + j) * a.pitch);
                                acc[j] = make_uint4((acc[j].x ^ p.x) & mk.x, (acc[j].y ^ p.y) & mk.y,
                                                    (acc[j].z ^ p.z) & mk.z, (acc[j].w ^ p.w) & mk.w);
                                bad = bad || nonzero(acc[j]);
                            }
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (r0 + j < m) synd[(r0 + j) * 64 + lane] = acc[j];
                }
            } else {
                const uint8_t* src = a.data + g * a.dgs + col;
                const uint8_t* par = a.parity + g * a.pgs + col;
                for (int r = 0; r < m; ++r) {
                    uint32_t sy = 0;
                    if (live) sy = (product_byte(src, a.pitch, a.tab, k, r) ^ (uint32_t)par[(uint64_t)r * a.pitch]) & 0xFFu;
                    bad = bad || sy != 0;
                    synd[r * 64 + lane] = sy;
                }
            }
            if (__ballot(bad) == 0) continue;  // these columns are consistent: every pair explains them
            uint32_t left = 0;
#pragma unroll
            for (int w = 0; w < L2_WORDS; ++w) {
                uint32_t todo = alive[w];
                while (todo) {  // wave-uniform
                    const int b = __builtin_ctz(todo);
                    todo &= todo - 1;
                    const cptr32 rec = chk + (32 * w + b) * ((m - 2) * m);
                    bool fail = false;
                    for (int r = 0; r < m - 2; ++r) {
                        W v;
                        if constexpr (VEC) v = make_uint4(0, 0, 0, 0);
                        else v = 0;
                        for (int j = 0; j < m; ++j) {
                            const uint32_t off = rec[r * m + j];
                            if (off == L2_ONE) xor_into(v, synd[j * 64 + lane]);
                            else if (off) mac_const(v, synd[j * 64 + lane], (cptr32)(t256 + off));
                        }
                        fail = fail || nonzero(v);
                    }
                    if (__ballot(fail)) alive[w] &= ~(1u << b);
                }
                left |= alive[w];
            }
            if (!left) break;
        }
        const int verdict = pair_verdict(alive, a.pair_ids);
        if (lane == 0) a.verdict2[g] = verdict;
    }
}

// one lane per group: list[..] = the groups qfec_locate called MULTI.  At most `groups` entries, so
// a list of [groups] cannot overflow.
__global__ void __launch_bounds__(256) k_locate2_list(Locate2Args a) {
    __shared__ unsigned int wave_hits[4], base;
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool hit = g < a.groups && a.stage1[g] == QFEC_LOC_MULTI;
    const uint64_t hits = __ballot(hit);
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wave_hits[wave] = (unsigned)__builtin_popcountll(hits);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = wave_hits[0] + wave_hits[1] + wave_hits[2] + wave_hits[3];
        base = total ? atomicAdd(a.list_n, total) : 0u;
    }
    __syncthreads();
    if (hit) {
        unsigned at = base + (unsigned)__builtin_popcountll(hits & ((1ull << lane) - 1ull));
        for (unsigned w = 0; w < wave; ++w) at += wave_hits[w];
        if (at < a.groups) a.list[at] = (unsigned)g;
    }
}

// one lane per group, every group: the two slots, the marks, the counters
__global__ void __launch_bounds__(256) k_locate2_finish(Locate2FinishArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    int verdict = -1;  // also for lanes past the last group
    if (g < a.groups) {
        int s0 = a.stage1[g], s1 = QFEC_LOC_CLEAN;
        if (s0 == QFEC_LOC_MULTI) {
            const int v = a.verdict2[g];
            s0 = v >= 0 ? (v & 0xFF) : v;
            s1 = v >= 0 ? (v >> 8) : v;
        } else if (s0 == QFEC_LOC_AMBIGUOUS) {
            s1 = QFEC_LOC_AMBIGUOUS;
        }
        a.culprit[2 * g] = s0;
        a.culprit[2 * g + 1] = s1;
        if (a.marks)
            write_marks_rs(a.marks, a.groups, g, a.k, a.m, (s0 >= 0 ? 1ull << s0 : 0ull) | (s1 >= 0 ? 1ull << s1 : 0ull));
        verdict = s0 == QFEC_LOC_CLEAN ? -1 : s1 >= 0 ? 1 : s0 >= 0 ? 0 : s0 == QFEC_LOC_MULTI ? 2 : 3;
    }
    if (a.counts) block_counts<4>(verdict, a.counts);  // uniform over the grid
}

static bool list_args_ok(const Locate2Args& a) {
    return a.groups <= 0xFFFFFFFFull && a.stage1 && a.list && a.list_n;
}

hipError_t launch_locate2_list(const Locate2Args& a, hipStream_t stream) {
    if (a.groups == 0) return hipSuccess;
    if (!list_args_ok(a)) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((a.groups + 255) / 256);
    hipLaunchKernelGGL(k_locate2_list, dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

#define QFEC_LOC2_CASE(KK, MM)                                                                  \
    if (a.k == KK && a.m == MM) {                                                               \
        hipLaunchKernelGGL((k_locate2_pairs<KK, MM>), dim3(grid), dim3(64), 0, stream, a);      \
        return hipGetLastError();                                                               \
    }

hipError_t launch_locate2_pairs(const Locate2Args& a, hipStream_t stream) {
    if (a.groups == 0) return hipSuccess;
    const int n = a.k + a.m;
    if (!list_args_ok(a) || a.m < 4 || a.k < 1 || n > QFEC_LOC2_MAX_N || a.pairs != n * (n - 1) / 2 || !a.data ||
        !a.parity || !a.tab || !a.t256 || !a.checks || !a.pair_ids || !a.verdict2 || a.cols == 0)
        return hipErrorInvalidValue;  // the caller checks the code
    const unsigned grid = (unsigned)std::min<uint64_t>(a.groups, L2_MAX_GRID);
    if (!a.vec16) {
        hipLaunchKernelGGL(k_locate2_pairs_any<uint32_t>, dim3(grid), dim3(64), (size_t)a.m * 64 * sizeof(uint32_t), stream, a);
        return hipGetLastError();
    }
    // launch_locate's instances with m = 4
    QFEC_LOC2_CASE(16, 4)
    QFEC_LOC2_CASE(8, 4)
    QFEC_LOC2_CASE(12, 4)
    QFEC_LOC2_CASE(20, 4)
    hipLaunchKernelGGL(k_locate2_pairs_any<uint4>, dim3(grid), dim3(64), (size_t)a.m * 64 * sizeof(uint4), stream, a);
    return hipGetLastError();
}

hipError_t launch_locate2_finish(const Locate2FinishArgs& a, hipStream_t stream) {
    if (a.groups == 0) return hipSuccess;
    if (!a.stage1 || !a.verdict2 || !a.culprit || a.groups > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((a.groups + 255) / 256);
    hipLaunchKernelGGL(k_locate2_finish, dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace qfec
