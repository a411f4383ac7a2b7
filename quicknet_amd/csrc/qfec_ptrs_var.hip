// qfec_ptrs_var.hip -- qfec_encode_ptrs_var / qfec_reconstruct_ptrs_var for MI355X (gfx950): the
// pointer-table calls of qfec_ptrs.hip on shards that each have their own length.  Data shard i of a
// group is len_i bytes and counts as zero-filled up to the group's length L (the encode: the longest
// len_i; the reconstruct: d_group_len[g], the length of the group's parity shards).  No byte at or
// past len_i of a data shard is read, no byte at or past L of a shard is written, and a shard of
// length 0 is never dereferenced.
//
// Mapping, address loads, lane widths and instances are those of qfec_ptrs.hip: one wave per (group,
// slab of 64 columns), four waves per block, wpg waves per group from ptrs_geom(max_len, lane
// bytes); lane s < k + m loads address s (and mark s) of its group and the wave reads what it needs
// with readlane.  New here:
//
// Lengths.  Lane i < k loads len_i in the same round trip as its address.  The encode's L is the
// maximum over the k readlanes (the runtime-k,m kernel: a wave reduction); the reconstruct reads
// d_group_len[g] as a scalar.  A lane's length reaches the column body through readlane, like its
// address, so every lane executes its loads before the first lane-dependent branch and the only
// early exits are wave-uniform (ballots of the loaded values): a void or invalid group, an empty
// one, a wave whose slab starts at or past L.
//
// Per-group geometry, ptrs_var_geom(L, W) of qfec_geom.hpp, W the lane width: L / W whole columns,
// the L % W bytes after them byte by byte on the first lanes of the group's last live wave.  Slab 0,
// lane 0 writes d_group_len and the counters.
//
// Two vector paths, chosen per wave by one ballot.  `full`: every source the wave reads is at
// least as long as the wave's whole columns reach, min(slab end, (L / W) * W).  Such a wave runs
// the column body of the fixed-length kernels unchanged (encode_column, recon_column_by_e); with
// all lengths equal that is every wave of every group, whatever L % W.  Any other wave is ragged: a
// source's column at `off` has n = clamp(len - off, 0, W) bytes; n = W is the vector load, n = 0 is
// zero with no load of that row, in between the n bytes are loaded as pieces of 8, 4, 2 and 1 bytes, one
// per set bit of n (at most one lane per source and group): ldv_ragged, ldv_part.  Outputs are whole columns below L either way: the same non-temporal vector stores.
//
// Alignment is judged per group on the entries the call may dereference: not the data shards of
// length 0, and in the reconstruct not the shards that are neither written nor read as survivors.
// A misaligned group runs the byte body, byte b of source i being b < len_i ? load : 0; the tail
// bytes of an aligned group run the same body.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "qfec_internal.hpp"
#include "qfec_device.hpp"
#include "qfec_geom.hpp"
#include "qfec_ptrs_device.hpp"

namespace qfec {

// ldv_ragged (qfec_ptrs_device.hpp) for the reconstruct, whose registers its readlanes raise (RS(16,4): 93 -> 101
// VGPRs, 5 -> 4 waves per SIMD, and the full path of all-equal lengths pays for it: 1.14 x the
// fixed-length call against 1.04): the lane whose column the row's part column is fetches it itself,
// under a wave-uniform test of whether that column lies in this slab.  One round trip per row
// with a part column in the slab, one after the other.
template <int D>
__device__ __forceinline__ void ldv_ragged_own(uint32_t (&v)[D], const uint8_t* row, const uint8_t* safe, uint32_t off,
                                               uint32_t len, uint32_t slab) {
    constexpr uint32_t W = 4u * D;
    const bool whole = off + W <= len;
    ldv<D>(v, (whole ? row : safe) + off);
#pragma unroll
    for (int d = 0; d < D; ++d) v[d] = whole ? v[d] : 0u;
    const uint32_t pc = len / W, pn = len % W;
    if (pn && (pc >> 6) == slab) {
        if (off == pc * W) ldv_part<D>(v, row + off, pn);
    }
}

// ------------------------------------------------------------------ encode

// encode_byte of qfec_ptrs.hip with lengths: len(c) = the length of data shard c
template <int K, class Row, class Len>
__device__ __forceinline__ void encode_byte_var(int k, int m, const uint32_t* tab, const Row& row, const Len& len,
                                                uint32_t b) {
    uint32_t x[K > 0 ? K : 1];
    if constexpr (K > 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) x[c] = b < len(c) ? (uint32_t)as_row(row(c))[b] : 0u;
    }
#pragma unroll 1
    for (int r = 0; r < m; ++r) {
        const uint32_t* tr = tab + (r * k) * QFEC_TAB_STRIDE;
        uint8_t* out = as_out(row(k + r)) + b;
        uint32_t acc = tr[5] ? (uint32_t)*out : 0u;  // rs.c column-0 quirk
        if constexpr (K > 0) {
#pragma unroll
            for (int c = 0; c < K; ++c) {
                const uint32_t* tc = tr + c * QFEC_TAB_STRIDE;
                acc ^= gf_mul4(gf_sel(x[c]), tc[0], tc[1], tc[2], tc[3], tc[4]);
            }
        } else {
#pragma unroll 1
            for (int c = 0; c < k; ++c) {
                const uint32_t* tc = tr + c * QFEC_TAB_STRIDE;
                const uint32_t xb = b < len(c) ? (uint32_t)as_row(row(c))[b] : 0u;
                acc ^= gf_mul4(gf_sel(xb), tc[0], tc[1], tc[2], tc[3], tc[4]);
            }
        }
        *out = (uint8_t)acc;
    }
}

// encode_column on a ragged wave: row(c), len(c) = address and length of data shard c (c wave-uniform,
// not a constant), which lane c holds; safe: the group's longest data shard; part: lane_part's
template <int K, int M, class Row, class Len>
__device__ __forceinline__ void encode_column_var(const Row& row, const Len& len, const uint8_t* safe,
                                                  const uint32_t (&part)[4], uint8_t* const (&dst)[M],
                                                  const uint32_t* tab, uint32_t off) {
    constexpr int CH = ragged_chunk<K, 8>();
    uint4 acc[M];
#pragma unroll
    for (int r = 0; r < M; ++r) {
        acc[r] = make_uint4(0, 0, 0, 0);
        if (tab[(r * K) * QFEC_TAB_STRIDE + 5]) acc[r] = *reinterpret_cast<const uint4*>(dst[r] + off);  // rs.c column-0 quirk
    }
#pragma unroll 1
    for (int c0 = 0; c0 < K; c0 += CH) {
        uint4 x[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) x[i] = ld16_ragged(as_row(row(c0 + i)), safe, off, len(c0 + i), part, c0 + i);
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            Sel s[4];
            sel16(s, x[i]);
#pragma unroll
            for (int r = 0; r < M; ++r) gf_mac16(acc[r], s, tab + (r * K + c0 + i) * QFEC_TAB_STRIDE);
        }
    }
#pragma unroll
    for (int r = 0; r < M; ++r) st16(dst[r] + off, acc[r]);
}

// slab 0, lane 0 of a void group: -1 and the counter
__device__ __forceinline__ void report_void(const PtrsVarArgs& a, uint64_t g) {
    if (a.group_len_out) a.group_len_out[g] = -1;
    if (a.invalid) atomicAdd(a.invalid, 1u);
}

template <int K, int M>
__global__ void __launch_bounds__(256) k_encode_ptrs_var(PtrsVarArgs a, const uint64_t* __restrict__ dptrs,
                                                         const uint64_t* __restrict__ pptrs,
                                                         const int32_t* __restrict__ lens,
                                                         const uint32_t* __restrict__ tab) {
    constexpr int N = K + M;
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a.p, &g, &slab)) return;
    uint64_t p = 0;
    uint32_t len = 0;  // as unsigned: a negative length is above every max_len
    if (lane < K) {
        p = dptrs[g * K + lane];
        len = (uint32_t)lens[g * K + lane];
    } else if (lane < N) {
        p = pptrs[g * M + (lane - K)];
    }
    const bool leader = slab == 0 && lane == 0;
    if (__ballot(len > a.p.block)) {  // a void group: nothing read or written
        if (leader) report_void(a, g);
        return;
    }
    uint32_t L = 0;
#pragma unroll
    for (int c = 0; c < K; ++c) L = std::max(L, lane_value32(len, c));
    if (leader && a.group_len_out) a.group_len_out[g] = (int32_t)L;
    const PtrsVarGeom v = ptrs_var_geom(L, 16);
    if (slab >= v.live) return;  // an empty group, or a slab at or past L
    const bool aligned = __ballot((p & 15u) != 0 && (lane >= K || len != 0)) == 0;
    const uint32_t reach = slab_reach<16>(v, slab);
    const bool full = __ballot(lane < K && len < reach) == 0;
    const auto len_of = [&](int c) { return lane_value32(len, c); };
    uint32_t part[4];
    if (aligned && !full) lane_part<4>(part, lane < K, p, len, slab);
    run_slab_var<16>(
        v, L, slab, lane, aligned,
        [&](uint32_t off) {
            uint8_t* dst[M];
#pragma unroll
            for (int r = 0; r < M; ++r) dst[r] = as_out(lane_value(p, K + r));
            if (full) {
                const uint8_t* src[K];
#pragma unroll
                for (int c = 0; c < K; ++c) src[c] = as_row(lane_value(p, c));
                encode_column<K, M>(src, dst, tab, off);
            } else {
                uint64_t safe = 0;  // the longest data shard: whole in every whole column of the group
#pragma unroll
                for (int c = 0; c < K; ++c) safe = len_of(c) == L ? lane_value(p, c) : safe;
                encode_column_var<K, M>([&](int c) { return lane_value(p, c); }, len_of, as_row(safe), part, dst, tab, off);
            }
        },
        [&](uint32_t b) { encode_byte_var<K>(K, M, tab, [&](int s) { return lane_value(p, s); }, len_of, b); });
}

constexpr int PCH = 4;  // output rows per pass of the runtime-k,m bodies, as in qfec_ptrs.hip

// one column of the runtime-k,m encode: qfec_ptrs.hip's, the inputs clipped unless FULL
template <bool FULL>
__device__ __forceinline__ void encode_column_any(int k, int m, const uint64_t* dp, const uint64_t* pp, const int32_t* ln,
                                                  const uint32_t* tab, uint32_t off) {
    for (int r0 = 0; r0 < m; r0 += PCH) {
        uint4 acc[PCH];
#pragma unroll
        for (int j = 0; j < PCH; ++j) {
            acc[j] = make_uint4(0, 0, 0, 0);
            if (r0 + j < m && tab[((r0 + j) * k) * QFEC_TAB_STRIDE + 5])
                acc[j] = *reinterpret_cast<const uint4*>(as_row(pp[r0 + j]) + off);
        }
        for (int c = 0; c < k; ++c) {
            uint4 x;
            if constexpr (FULL) x = ld16(as_row(dp[c]) + off);
            else x = ld16_clip(as_row(dp[c]), off, (uint32_t)ln[c]);
            Sel s[4];
            sel16(s, x);
#pragma unroll
            for (int j = 0; j < PCH; ++j)
                if (r0 + j < m) gf_mac16(acc[j], s, tab + ((r0 + j) * k + c) * QFEC_TAB_STRIDE);
        }
#pragma unroll
        for (int j = 0; j < PCH; ++j)
            if (r0 + j < m) st16(as_out(pp[r0 + j]) + off, acc[j]);
    }
}

__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
    for (int o = 32; o; o >>= 1) x = std::max(x, (uint32_t)__shfl_xor((int)x, o));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
}

// runtime k, m (k + m may pass 64 lanes): addresses and lengths are read from the tables where they
// are used; the lanes stride over the group's entries for L, the shortest length and the alignment
__global__ void __launch_bounds__(256) k_encode_ptrs_var_any(PtrsVarArgs a, const uint64_t* __restrict__ dptrs,
                                                             const uint64_t* __restrict__ pptrs,
                                                             const int32_t* __restrict__ lens,
                                                             const uint32_t* __restrict__ tab) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a.p, &g, &slab)) return;
    const int k = a.p.k, m = a.p.m;
    const uint64_t* dp = dptrs + g * (uint64_t)k;
    const uint64_t* pp = pptrs + g * (uint64_t)m;
    const int32_t* ln = lens + g * (uint64_t)k;
    uint32_t low = 0, longest = 0, shortest = 0xFFFFFFFFu;
    for (int i = lane; i < k; i += 64) {
        const uint32_t l = (uint32_t)ln[i];
        const uint32_t q = (uint32_t)dp[i] & 15u;
        longest = std::max(longest, l);
        shortest = std::min(shortest, l);
        if (l) low |= q;
    }
    for (int i = lane; i < m; i += 64) low |= (uint32_t)pp[i] & 15u;
    const bool leader = slab == 0 && lane == 0;
    if (__ballot(longest > a.p.block)) {
        if (leader) report_void(a, g);
        return;
    }
    const uint32_t L = wave_max(longest);
    shortest = ~wave_max(~shortest);
    if (leader && a.group_len_out) a.group_len_out[g] = (int32_t)L;
    const PtrsVarGeom v = ptrs_var_geom(L, 16);
    if (slab >= v.live) return;
    const bool aligned = __ballot(low != 0) == 0;
    const bool full = shortest >= slab_reach<16>(v, slab);
    run_slab_var<16>(
        v, L, slab, lane, aligned,
        [&](uint32_t off) {
            if (full) encode_column_any<true>(k, m, dp, pp, ln, tab, off);
            else encode_column_any<false>(k, m, dp, pp, ln, tab, off);
        },
        [&](uint32_t b) {
            encode_byte_var<0>(k, m, tab, [&](int s) { return s < k ? dp[s] : pp[s - k]; },
                               [&](int c) { return (uint32_t)ln[c]; }, b);
        });
}

// ------------------------------------------------------------------ reconstruct

// What the reconstruct kernels share once a group's lengths and marks are judged.  used: the shards
// read as survivors (all surviving data, then the first e surviving parity rows); lost: the erased
// data shards.  eff: lane s holds how many bytes of shard s may be read (len_s of a data shard, L of
// a parity shard).
struct ReconJudged {
    bool aligned, full;
    uint64_t used;
};

template <int W>
__device__ __forceinline__ ReconJudged recon_judge(const PtrsVarGeom& v, uint32_t slab, int lane, int k, uint64_t p,
                                                   uint32_t eff, uint64_t avail, uint64_t lost, int e) {
    const uint64_t kmask = (1ull << k) - 1ull;
    uint64_t rest = avail >> k;
    for (int j = 0; j < e; ++j) rest &= rest - 1;
    const uint64_t used = (avail & kmask) | (((avail >> k) & ~rest) << k);
    const uint64_t deref = (used & ~__ballot(eff == 0)) | lost;
    ReconJudged r;
    r.aligned = (__ballot((p & 15u) != 0) & deref) == 0;
    r.full = (__ballot(eff < slab_reach<W>(v, slab)) & used) == 0;
    r.used = used;
    return r;
}

// recon_byte of qfec_ptrs.hip with lengths
__device__ __forceinline__ void recon_byte_var(const PtrsArgs& a, const uint32_t* r, uint64_t p, uint32_t eff, uint32_t b) {
    const int e = (int)r[0], k = a.k;
    const uint32_t* surv = r + a.surv_off;
    const uint32_t* lost = r + a.lost_off;
    const uint32_t* tab = r + a.hdr;
#pragma unroll 1
    for (int j = 0; j < e; ++j) {
        uint8_t* out = as_out(lane_value(p, lost[j])) + b;
        uint32_t acc = tab[(j * k) * QFEC_TAB_STRIDE + 5] ? (uint32_t)*out : 0u;  // rs.c column-0 quirk
#pragma unroll 1
        for (int c = 0; c < k; ++c) {
            const uint32_t* tc = tab + (j * k + c) * QFEC_TAB_STRIDE;
            const uint32_t s = surv[c];
            const uint32_t x = b < lane_value32(eff, s) ? (uint32_t)as_row(lane_value(p, s))[b] : 0u;
            acc ^= gf_mul4(gf_sel(x), tc[0], tc[1], tc[2], tc[3], tc[4]);
        }
        *out = (uint8_t)acc;
    }
}

// recon_byte_var for the templated kernels.  With per-shard lengths nearly every group has a tail, and
// recon_byte_var waits for a load per (row, survivor): at RS(16,4) 64 round trips one after the other
// in the last wave of every group.  Here a byte is loaded once per survivor, the survivors in
// chunks whose loads issue together (a survivor that ends before b reads `safe` instead and drops it,
// as in ldv_ragged), and the M rows accumulate side by side.
template <int K, int M>
__device__ __forceinline__ void recon_byte_rows(const PtrsArgs& a, const uint32_t* r, uint64_t p, uint32_t eff,
                                                uint64_t avail, uint32_t b) {
    constexpr int CH = ragged_chunk<K, 8>();
    const int e = (int)r[0];
    const uint32_t* surv = r + a.surv_off;
    const uint32_t* lost = r + a.lost_off;
    const uint32_t* tab = r + a.hdr;
    const uint8_t* safe = as_row(lane_value(p, K + (uint32_t)__builtin_ctzll(avail >> K)));
    uint32_t acc[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        acc[j] = 0;
        if (j < e && tab[(j * K) * QFEC_TAB_STRIDE + 5]) acc[j] = as_out(lane_value(p, lost[j]))[b];  // rs.c column-0 quirk
    }
#pragma unroll 1
    for (int c0 = 0; c0 < K; c0 += CH) {
        uint32_t x[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const uint32_t s = surv[c0 + i];
            const bool in = b < lane_value32(eff, s);
            x[i] = (in ? as_row(lane_value(p, s)) : safe)[b];
            x[i] = in ? x[i] : 0u;
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const Sel sl = gf_sel(x[i]);
#pragma unroll
            for (int j = 0; j < M; ++j)
                if (j < e) {
                    const uint32_t* tc = tab + (j * K + c0 + i) * QFEC_TAB_STRIDE;
                    acc[j] ^= gf_mul4(sl, tc[0], tc[1], tc[2], tc[3], tc[4]);
                }
        }
    }
#pragma unroll
    for (int j = 0; j < M; ++j)
        if (j < e) as_out(lane_value(p, lost[j]))[b] = (uint8_t)acc[j];
}

// recon_column_e / recon_column_by_e of qfec_device.hpp on a ragged wave, rolled over the survivors in
// chunks (ragged_chunk): p, eff = the lanes' addresses and readable lengths, avail = the unmarked
// shards, of which the K lowest are the survivors; safe: the first surviving parity shard, which is
// read whenever a data shard is erased and is whole in every whole column of the group
template <int K, int E, int D>
__device__ __forceinline__ void recon_column_e_var(uint64_t p, uint32_t eff, uint64_t avail, uint64_t lost_bits,
                                                   const RTab& T, uint32_t off, uint32_t slab) {
    constexpr int CH = ragged_chunk<K, 32 / (4 * D)>();
    const uint8_t* safe = as_row(lane_value(p, K + (uint32_t)__builtin_ctzll(avail >> K)));
    uint8_t* dst[E];
    uint32_t acc[E][D];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const uint32_t l = (uint32_t)__builtin_ctzll(lost_bits);
        lost_bits &= lost_bits - 1;
        dst[j] = as_out(lane_value(p, l)) + off;
#pragma unroll
        for (int d = 0; d < D; ++d) acc[j][d] = 0;
        if (T.quirk(j, K)) ldv_plain<D>(acc[j], dst[j]);  // rs.c column-0 quirk
    }
#pragma unroll 1
    for (int c0 = 0; c0 < K; c0 += CH) {
        uint32_t x[CH][D];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const uint32_t s = (uint32_t)__builtin_ctzll(avail);
            avail &= avail - 1;
            ldv_ragged_own<D>(x[i], as_row(lane_value(p, s)), safe, off, lane_value32(eff, s), slab);
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            Sel sl[D];
#pragma unroll
            for (int d = 0; d < D; ++d) sl[d] = gf_sel(x[i][d]);
#pragma unroll
            for (int j = 0; j < E; ++j) {
                uint32_t t[5];
                T.load5(j, c0 + i, K, t);
#pragma unroll
                for (int d = 0; d < D; ++d)
                    acc[j][d] = xor3(acc[j][d], pp0(sl[d], t[0], t[1]), pp1(sl[d], t[2], t[3])) ^ pp2(sl[d], t[4]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < E; ++j) stv<D>(dst[j], acc[j]);
}

template <int K, int M, int D, int E = M>
__device__ __forceinline__ void recon_column_var_by_e(uint64_t p, uint32_t eff, uint64_t avail, uint64_t lost_bits,
                                                      const RTab& T, int e, uint32_t off, uint32_t slab) {
    if constexpr (E > 1) {
        if (e < E) {
            recon_column_var_by_e<K, M, D, E - 1>(p, eff, avail, lost_bits, T, e, off, slab);
            return;
        }
    }
    recon_column_e_var<K, E, D>(p, eff, avail, lost_bits, T, off, slab);
}

// lane s < n: mark s, address s and (s < k) length s of group g, in one round trip; the rest zero
__device__ __forceinline__ void marks_rows_lens(const uint64_t* __restrict__ dptrs, const uint64_t* __restrict__ pptrs,
                                                const int32_t* __restrict__ lens, const uint8_t* __restrict__ dmarks,
                                                const uint8_t* __restrict__ pmarks, uint64_t g, int k, int m, int lane,
                                                uint32_t* mk, uint64_t* p, uint32_t* len) {
    *mk = 0;
    *p = 0;
    *len = 0;
    if (lane < k) {
        *mk = dmarks[g * (uint64_t)k + lane];
        *p = dptrs[g * (uint64_t)k + lane];
        *len = (uint32_t)lens[g * (uint64_t)k + lane];
    } else if (lane < k + m) {
        *mk = pmarks[g * (uint64_t)m + (lane - k)];
        *p = pptrs[g * (uint64_t)m + (lane - k)];
    }
}

// Lengths are judged before marks: L outside [0, max_len], or an unmarked data shard outside [0, L]
// (the entry of a marked one is not looked at).  True: the group is invalid; counted once, untouched.
__device__ __forceinline__ bool recon_invalid(const PtrsVarArgs& a, uint32_t L, int lane, int k, uint32_t mk, uint32_t len,
                                              bool leader) {
    if (L <= a.p.block && !__ballot(lane < k && mk == 0 && len > L)) return false;
    if (leader && a.invalid) atomicAdd(a.invalid, 1u);
    return true;
}

template <int K, int M, int D>
__global__ void __launch_bounds__(256) k_reconstruct_ptrs_var(PtrsVarArgs a, const uint64_t* __restrict__ dptrs,
                                                              const uint64_t* __restrict__ pptrs,
                                                              const int32_t* __restrict__ lens,
                                                              const int32_t* __restrict__ glen,
                                                              const uint8_t* __restrict__ dmarks,
                                                              const uint8_t* __restrict__ pmarks,
                                                              const int32_t* __restrict__ lut,
                                                              const uint32_t* __restrict__ records) {
    constexpr int N = K + M;
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a.p, &g, &slab)) return;
    uint32_t mk, len;
    uint64_t p;
    marks_rows_lens(dptrs, pptrs, lens, dmarks, pmarks, g, K, M, lane, &mk, &p, &len);
    const uint32_t L = (uint32_t)glen[g];
    const bool leader = slab == 0 && lane == 0;
    if (recon_invalid(a, L, lane, K, mk, len, leader)) return;
    const PtrsVarGeom v = ptrs_var_geom(L, 4 * D);
    if (slab >= v.live) return;  // an empty group, or a slab at or past L
    const uint64_t mask = __ballot(mk != 0) & ((1ull << N) - 1ull);
    const uint64_t lost_bits = mask & ((1ull << K) - 1ull);
    const int e = __builtin_popcountll(lost_bits);
    if (e == 0) return;
    const uint64_t avail = ~mask & ((1ull << N) - 1ull);
    const int rec = __builtin_popcountll(avail) < K ? QFEC_REC_FAIL
                                                    : ((const __attribute__((address_space(4))) int32_t*)lut)[mask];
    if (rec < 0) {  // under-determined (or a singular decode matrix of explicit rows): untouched, counted
        if (leader && a.p.failed) atomicAdd(a.p.failed, 1u);
        return;
    }
    const uint32_t eff = lane < K ? len : lane < N ? L : 0u;
    const ReconJudged j = recon_judge<4 * D>(v, slab, lane, K, p, eff, avail, lost_bits, e);
    run_slab_var<4 * D>(
        v, L, slab, lane, j.aligned,
        [&](uint32_t off) {
            const RTab T{records + rec, a.p.coff, a.p.t256};
            if (j.full) {
                uint64_t left = avail;
                const uint8_t* src[K];
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    const uint32_t s = (uint32_t)__builtin_ctzll(left);
                    left &= left - 1;
                    src[c] = as_row(lane_value(p, s));
                }
                recon_column_by_e<K, M, D>(src, nullptr, LaneRows{p}, lost_bits, T, e, off);
            } else {
                recon_column_var_by_e<K, M, D>(p, eff, avail, lost_bits, T, e, off, slab);
            }
        },
        [&](uint32_t b) { recon_byte_rows<K, M>(a.p, records + rec, p, eff, avail, b); });
}

// runtime k, m (k + m <= QFEC_LUT_MAX_N), e from the record, whose tables are inline; rows in chunks of PCH
template <int D>
__global__ void __launch_bounds__(256) k_reconstruct_ptrs_var_any(PtrsVarArgs a, const uint64_t* __restrict__ dptrs,
                                                                  const uint64_t* __restrict__ pptrs,
                                                                  const int32_t* __restrict__ lens,
                                                                  const int32_t* __restrict__ glen,
                                                                  const uint8_t* __restrict__ dmarks,
                                                                  const uint8_t* __restrict__ pmarks,
                                                                  const int32_t* __restrict__ lut,
                                                                  const uint32_t* __restrict__ records) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a.p, &g, &slab)) return;
    const int k = a.p.k, n = a.p.k + a.p.m;
    uint32_t mk, len;
    uint64_t p;
    marks_rows_lens(dptrs, pptrs, lens, dmarks, pmarks, g, k, a.p.m, lane, &mk, &p, &len);
    const uint32_t L = (uint32_t)glen[g];
    const bool leader = slab == 0 && lane == 0;
    if (recon_invalid(a, L, lane, k, mk, len, leader)) return;
    const PtrsVarGeom v = ptrs_var_geom(L, 4 * D);
    if (slab >= v.live) return;
    const uint32_t mask = (uint32_t)(__ballot(mk != 0) & ((1ull << n) - 1ull));
    const uint32_t lost_bits = mask & ((1u << k) - 1u);
    if (!lost_bits) return;
    const int rec = __builtin_amdgcn_readfirstlane(lut[mask]);
    if (rec < 0) {
        if (rec == QFEC_REC_FAIL && leader && a.p.failed) atomicAdd(a.p.failed, 1u);
        return;
    }
    const uint32_t* r = records + rec;
    const int e = (int)r[0];
    const uint32_t* surv = r + a.p.surv_off;
    const uint32_t* lost = r + a.p.lost_off;
    const uint32_t* tab = r + a.p.hdr;
    const uint32_t eff = lane < k ? len : lane < n ? L : 0u;
    const ReconJudged j = recon_judge<4 * D>(v, slab, lane, k, p, eff, ~mask & ((1u << n) - 1u), lost_bits,
                                             __builtin_popcount(lost_bits));
    run_slab_var<4 * D>(
        v, L, slab, lane, j.aligned,
        [&](uint32_t off) {
            for (int j0 = 0; j0 < e; j0 += PCH) {
                uint32_t acc[PCH][D];
#pragma unroll
                for (int q = 0; q < PCH; ++q) {
#pragma unroll
                    for (int d = 0; d < D; ++d) acc[q][d] = 0;
                    if (j0 + q < e && tab[((j0 + q) * k) * QFEC_TAB_STRIDE + 5])
                        ldv_plain<D>(acc[q], as_row(lane_value(p, lost[j0 + q])) + off);
                }
                for (int c = 0; c < k; ++c) {
                    uint32_t x[D];
                    const uint32_t s = surv[c];
                    if (j.full) ldv<D>(x, as_row(lane_value(p, s)) + off);
                    else ldv_clip<D>(x, as_row(lane_value(p, s)), off, lane_value32(eff, s));
#pragma unroll
                    for (int q = 0; q < PCH; ++q)
                        if (j0 + q < e) {
                            const uint32_t* tc = tab + ((j0 + q) * k + c) * QFEC_TAB_STRIDE;
#pragma unroll
                            for (int d = 0; d < D; ++d) acc[q][d] ^= gf_mul4(gf_sel(x[d]), tc[0], tc[1], tc[2], tc[3], tc[4]);
                        }
                }
#pragma unroll
                for (int q = 0; q < PCH; ++q)
                    if (j0 + q < e) stv<D>(as_out(lane_value(p, lost[j0 + q])) + off, acc[q]);
            }
        },
        [&](uint32_t b) { recon_byte_var(a.p, r, p, eff, b); });
}

// ------------------------------------------------------------------ launchers

// blocks of four waves over groups * wpg waves, wpg from ptrs_geom(max_len, lane bytes); false when
// the caller has to chunk or the geometry is not the one the kernels are built for
static inline bool ptrs_var_grid(const PtrsArgs& a, bool reconstruct, unsigned* grid) {
    const uint64_t waves = a.groups * (uint64_t)a.wpg;
    if (a.wpg == 0 || waves * 64 > (uint64_t)kMaxLaunchLanes) return false;
    if ((int)a.lane_bytes != ptrs_lane_bytes(reconstruct, a.k)) return false;
    if (a.wpg != ptrs_geom((int)a.block, (int)a.lane_bytes).wpg) return false;
    *grid = (unsigned)((waves + 3) / 4);
    return true;
}

#define QFEC_VENC_CASE(KK, MM)                                                                                   \
    if (a.p.k == KK && a.p.m == MM) {                                                                            \
        hipLaunchKernelGGL((k_encode_ptrs_var<KK, MM>), dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs, \
                           a.lens, a.p.tab);                                                                     \
        return hipGetLastError();                                                                                \
    }

hipError_t launch_encode_ptrs_var(const PtrsVarArgs& a, hipStream_t stream) {
    if (a.p.groups == 0 || a.p.m == 0) return hipSuccess;
    unsigned grid;
    if (!ptrs_var_grid(a.p, false, &grid)) return hipErrorInvalidValue;
    QFEC_VENC_CASE(10, 3)
    QFEC_VENC_CASE(16, 4)
    QFEC_VENC_CASE(4, 2)
    QFEC_VENC_CASE(8, 4)
    hipLaunchKernelGGL(k_encode_ptrs_var_any, dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs, a.lens, a.p.tab);
    return hipGetLastError();
}

// the lane width of an instance is ptrs_lane_bytes' (8 B for k >= 10)
#define QFEC_VREC_CASE(KK, MM)                                                                                        \
    if (a.p.k == KK && a.p.m == MM) {                                                                                 \
        hipLaunchKernelGGL((k_reconstruct_ptrs_var<KK, MM, (KK >= 10 ? 2 : 4)>), dim3(grid), dim3(256), 0, stream, a,  \
                           a.p.dptrs, a.p.pptrs, a.lens, a.group_len, a.p.dmarks, a.p.pmarks, a.p.lut, a.p.records); \
        return hipGetLastError();                                                                                     \
    }

hipError_t launch_reconstruct_ptrs_var(const PtrsVarArgs& a, hipStream_t stream) {
    if (a.p.groups == 0) return hipSuccess;
    unsigned grid;
    if (a.p.k + a.p.m > QFEC_LUT_MAX_N || !ptrs_var_grid(a.p, true, &grid)) return hipErrorInvalidValue;
    QFEC_VREC_CASE(10, 3)
    QFEC_VREC_CASE(16, 4)
    QFEC_VREC_CASE(4, 2)
    QFEC_VREC_CASE(8, 4)
    if (a.p.lane_bytes == 8)
        hipLaunchKernelGGL((k_reconstruct_ptrs_var_any<2>), dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs,
                           a.lens, a.group_len, a.p.dmarks, a.p.pmarks, a.p.lut, a.p.records);
    else
        hipLaunchKernelGGL((k_reconstruct_ptrs_var_any<4>), dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs,
                           a.lens, a.group_len, a.p.dmarks, a.p.pmarks, a.p.lut, a.p.records);
    return hipGetLastError();
}

}  // namespace qfec
