// qfec_device.hpp -- device helpers shared by the HIP kernels of libqfec (gfx950).
// GF(2^8) multiply by a constant four bytes per v_perm_b32 (see qfec_kernels.hip header),
// streamed loads/stores, division by a runtime constant, the bodies the integrity kernels share
// (qfec_verify.hip, qfec_locate.hip, qfec_locate_erased.hip, qfec_integrity_ptrs.hip): products,
// syndrome tests, reports, counters, marks,
// and the encode's and the reconstruct's column bodies, which the contiguous kernels
// (qfec_kernels.hip) and the pointer-table kernels (qfec_ptrs.hip) both run.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "qfec_internal.hpp"

namespace qfec {

// ------------------------------------------------------------------ GF helpers

// selector words for the three partial products of the 4 bytes in x
struct Sel {
    uint32_t a, b, c;
};

__device__ __forceinline__ Sel gf_sel(uint32_t x) {
    Sel s;
    s.a = x & 0x07070707u;
    s.b = (x >> 3) & 0x07070707u;
    s.c = (x >> 6) & 0x03030303u;
    return s;
}

// a ^ b ^ c in one VALU op (gfx950 v_bitop3_b32, truth table 0x96)
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// the three partial products of c * x (t = the 5-dword perm table of c)
__device__ __forceinline__ uint32_t pp0(const Sel& s, uint32_t t0, uint32_t t1) { return __builtin_amdgcn_perm(t1, t0, s.a); }
__device__ __forceinline__ uint32_t pp1(const Sel& s, uint32_t t2, uint32_t t3) { return __builtin_amdgcn_perm(t3, t2, s.b); }
__device__ __forceinline__ uint32_t pp2(const Sel& s, uint32_t t4) { return __builtin_amdgcn_perm(t4, t4, s.c); }

// c * x for the four bytes described by s
__device__ __forceinline__ uint32_t gf_mul4(const Sel& s, uint32_t t0, uint32_t t1, uint32_t t2,
                                            uint32_t t3, uint32_t t4) {
    return xor3(pp0(s, t0, t1), pp1(s, t2, t3), pp2(s, t4));
}

// acc ^= c * x over 16 bytes: 3 v_perm_b32 + 2 v_bitop3 per dword
__device__ __forceinline__ void gf_mac16(uint4& acc, const Sel (&s)[4], const uint32_t* __restrict__ t) {
    const uint32_t t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3], t4 = t[4];
    acc.x = xor3(acc.x, pp0(s[0], t0, t1), pp1(s[0], t2, t3)) ^ pp2(s[0], t4);
    acc.y = xor3(acc.y, pp0(s[1], t0, t1), pp1(s[1], t2, t3)) ^ pp2(s[1], t4);
    acc.z = xor3(acc.z, pp0(s[2], t0, t1), pp1(s[2], t2, t3)) ^ pp2(s[2], t4);
    acc.w = xor3(acc.w, pp0(s[3], t0, t1), pp1(s[3], t2, t3)) ^ pp2(s[3], t4);
}

// acc ^= ca * xa ^ cb * xb over 16 bytes: 6 v_perm_b32 + 3 v_bitop3 per dword
__device__ __forceinline__ uint32_t mac2(uint32_t acc, const Sel& a, const Sel& b, const uint32_t* ta,
                                         const uint32_t* tb) {
    acc = xor3(acc, pp0(a, ta[0], ta[1]), pp1(a, ta[2], ta[3]));
    acc = xor3(acc, pp2(a, ta[4]), pp0(b, tb[0], tb[1]));
    return xor3(acc, pp1(b, tb[2], tb[3]), pp2(b, tb[4]));
}

__device__ __forceinline__ void gf_mac16x2(uint4& acc, const Sel (&sa)[4], const Sel (&sb)[4],
                                           const uint32_t* __restrict__ ta, const uint32_t* __restrict__ tb) {
    uint32_t a5[5], b5[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) { a5[i] = ta[i]; b5[i] = tb[i]; }
    acc.x = mac2(acc.x, sa[0], sb[0], a5, b5);
    acc.y = mac2(acc.y, sa[1], sb[1], a5, b5);
    acc.z = mac2(acc.z, sa[2], sb[2], a5, b5);
    acc.w = mac2(acc.w, sa[3], sb[3], a5, b5);
}

// opaque register barrier: uses of v after it cannot be hoisted above it
__device__ __forceinline__ void pin16(uint4& v) {
    asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
}

__device__ __forceinline__ void sel16(Sel (&s)[4], const uint4& v) {
    s[0] = gf_sel(v.x);
    s[1] = gf_sel(v.y);
    s[2] = gf_sel(v.z);
    s[3] = gf_sel(v.w);
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// streamed once: non-temporal (the shards are not re-read by this launch)
__device__ __forceinline__ uint4 ld16(const uint8_t* p) {
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
// written once, read by a later launch or the host: non-temporal store (measured on
// MI355X: the encode traffic shape streams at 6.3 TB/s with nt loads + nt stores against
// 5.7 TB/s with plain stores, tools/membench.hip)
__device__ __forceinline__ void st16(uint8_t* p, const uint4& v) {
    const u32x4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<u32x4*>(p));
}

// D dwords per lane, streamed (the reconstruct / repair / locate-erased bodies: 16-, 12- or 8-B columns)
template <int D>
__device__ __forceinline__ void ldv(uint32_t (&v)[D], const uint8_t* p) {
    if constexpr (D == 4) {
        const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else if constexpr (D == 3) {  // merged into one global_load_dwordx3 ... nt
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        v[0] = __builtin_nontemporal_load(q);
        v[1] = __builtin_nontemporal_load(q + 1);
        v[2] = __builtin_nontemporal_load(q + 2);
    } else {
        static_assert(D == 2, "4, 3 or 2 dwords per lane");
        const u32x2 t = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
        v[0] = t.x; v[1] = t.y;
    }
}

template <int D>
__device__ __forceinline__ void stv(uint8_t* p, const uint32_t (&v)[D]) {
    if constexpr (D == 4) {
        const u32x4 t = {v[0], v[1], v[2], v[3]};
        __builtin_nontemporal_store(t, reinterpret_cast<u32x4*>(p));
    } else if constexpr (D == 3) {
        uint32_t* q = reinterpret_cast<uint32_t*>(p);
        __builtin_nontemporal_store(v[0], q);
        __builtin_nontemporal_store(v[1], q + 1);
        __builtin_nontemporal_store(v[2], q + 2);
    } else {
        const u32x2 t = {v[0], v[1]};
        __builtin_nontemporal_store(t, reinterpret_cast<u32x2*>(p));
    }
}
template <int D>
__device__ __forceinline__ void ldv_plain(uint32_t (&v)[D], const uint8_t* p) {
#pragma unroll
    for (int d = 0; d < D; ++d) v[d] = reinterpret_cast<const uint32_t*>(p)[d];
}

// where row l of a group starts, given the group's base: rows `pitch` apart (the contiguous layout)
struct RowsAt {
    uint64_t pitch;
    __device__ __forceinline__ uint8_t* operator()(uint8_t* base, uint32_t l) const { return base + (uint64_t)l * pitch; }
};

__device__ __forceinline__ uint64_t fast_div(uint64_t n, const DivMagic& d) {
    // n < 2^32 and d.mul < 2^33 (see make_div_magic); exact.
    return d.pow2 ? (n >> d.shift) : ((n * d.mul) >> (32 + d.shift));
}

// ------------------------------------------------------------------ the lanes of qfec_plan.hpp on the device
// plan_group / check_group run by one wave that is its whole block (k_plan_build, k_check_build); the
// host's counterpart is PlanHostLanes
struct PlanWaveLanes {
    static constexpr int n = 64;
    int lane;
    __device__ __forceinline__ void sync() const { __syncthreads(); }  // the block is this one wave
    __device__ __forceinline__ int uni(int x) const { return __builtin_amdgcn_readfirstlane(x); }
    __device__ __forceinline__ void store16(uint8_t* dst, const uint32_t (&w)[4]) const {
        *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    }
};

// ------------------------------------------------------------------ compact records
// where a decode record's coefficient tables are: in the 256-entry table of every coefficient
// value, at the byte offsets the record's header lists (RecordLayout::coff).  Reading only the
// record's header keeps the records of all patterns cache-resident (RS(16,4): 4 844 records of
// 2.4 KB would not fit the 4 MB L2; their headers do).  The tables are read through the
// constant address space: loads from it are scalar (SMEM) whatever stores the kernel makes.
typedef const __attribute__((address_space(4))) uint32_t* cptr32;
typedef const __attribute__((address_space(4))) uint8_t* cptr8;
struct RTab {
    cptr32 rec;  // the record: [1] quirk flags, [coff + j*K + c] table byte offsets
    cptr32 offs;
    cptr32 t256;
    __device__ RTab(const uint32_t* r, int coff, const uint32_t* t)
        : rec((cptr32)r), offs((cptr32)r + coff), t256((cptr32)t) {}
    __device__ __forceinline__ cptr32 at(int j, int c, int K) const {
        return (cptr32)((cptr8)t256 + offs[j * K + c]);
    }
    __device__ __forceinline__ bool quirk(int j, int K) const { return (rec[1] >> j) & 1u; }
    __device__ __forceinline__ void load5(int j, int c, int K, uint32_t (&t5)[5]) const {
#pragma unroll
        for (int i = 0; i < 5; ++i) t5[i] = at(j, c, K)[i];
    }
};
// acc[j] ^= sum_c coef(j, c) * x[c] over one column, exact E rows, survivors already in registers
template <int K, int E, int D>
__device__ __forceinline__ void recon_mac_core(const uint32_t (&x)[K][D], uint32_t (&acc)[E][D], const RTab& T) {
#pragma unroll
    for (int c = 0; c + 1 < K; c += 2) {
        Sel sa[D], sb[D];
#pragma unroll
        for (int d = 0; d < D; ++d) { sa[d] = gf_sel(x[c][d]); sb[d] = gf_sel(x[c + 1][d]); }
#pragma unroll
        for (int j = 0; j < E; ++j) {
            uint32_t a5[5], b5[5];
            T.load5(j, c, K, a5);
            T.load5(j, c + 1, K, b5);
#pragma unroll
            for (int d = 0; d < D; ++d) acc[j][d] = mac2(acc[j][d], sa[d], sb[d], a5, b5);
        }
    }
    if (K & 1) {
        Sel sl[D];
#pragma unroll
        for (int d = 0; d < D; ++d) sl[d] = gf_sel(x[K - 1][d]);
#pragma unroll
        for (int j = 0; j < E; ++j) {
            uint32_t t[5];
            T.load5(j, K - 1, K, t);
#pragma unroll
            for (int d = 0; d < D; ++d)
                acc[j][d] = xor3(acc[j][d], pp0(sl[d], t[0], t[1]), pp1(sl[d], t[2], t[3])) ^ pp2(sl[d], t[4]);
        }
    }
}

// One column of a group's reconstruct: the K survivors' columns at byte `off` of src[c] in, the
// group's E erased data rows (E = its erased-data count, wave-uniform) out, at byte `off` of
// row_at(l) for every set bit l of lost_bits.  All E rows at once, selectors formed once per input
// and shared by the rows, no work on the M - E rows a group does not need.  3 random erasures of 13
// give e = 1, 2, 3 with probability 0.10, 0.47, 0.42, so RS(10,3) does 77 % of the all-rows VALU
// work.  D = dwords per lane (4: 16-B columns, 2: 8-B columns for rows whose 16-B column count
// leaves a wave mostly idle, e.g. B = 1400: 88 16-B columns on 2 waves, 175 8-B on 3).  row_at(base, l): RowsAt for the contiguous layout, where `base` is the group's data
// (__restrict__: the rows written are not the inputs), or a table of row addresses that ignores it.
template <int K, int E, int D, class RowAt>
__device__ __forceinline__ void recon_column_e(const uint8_t* const (&src)[K], uint8_t* __restrict__ base,
                                               const RowAt& row_at, uint64_t lost_bits, const RTab& T, uint64_t off) {
    uint32_t x[K][D];
#pragma unroll
    for (int c = 0; c < K; ++c) ldv<D>(x[c], src[c] + off);
    uint8_t* dst[E];
    uint32_t acc[E][D];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const uint32_t l = (uint32_t)__builtin_ctzll(lost_bits);
        lost_bits &= lost_bits - 1;
        dst[j] = row_at(base, l) + off;
#pragma unroll
        for (int d = 0; d < D; ++d) acc[j][d] = 0;
        if (T.quirk(j, K)) ldv_plain<D>(acc[j], dst[j]);  // rs.c column-0 quirk
    }
    recon_mac_core<K, E, D>(x, acc, T);
#pragma unroll
    for (int j = 0; j < E; ++j) stv<D>(dst[j], acc[j]);
}

// wave-uniform dispatch on e to the exact-row-count body
template <int K, int M, int D, class RowAt, int E = M>
__device__ __forceinline__ void recon_column_by_e(const uint8_t* const (&src)[K], uint8_t* __restrict__ base,
                                                  const RowAt& row_at, uint64_t lost_bits, const RTab& T, int e,
                                                  uint64_t off) {
    if constexpr (E > 1) {
        if (e < E) {
            recon_column_by_e<K, M, D, RowAt, E - 1>(src, base, row_at, lost_bits, T, e, off);
            return;
        }
    }
    recon_column_e<K, E, D, RowAt>(src, base, row_at, lost_bits, T, off);
}

// ------------------------------------------------------------------ the encode's multiply-accumulate
// acc[r] ^= sum_{i < N} P[r][C0 + i] x x[i], r < M: N inputs in registers against columns C0 ..
// C0 + N - 1 of the [M][K] perm tables, two inputs per pass (k_encode_perm: C0 = 0, N = K)
template <int K, int M, int C0, int N>
__device__ __forceinline__ void enc_mac16(uint4 (&acc)[M], const uint4 (&x)[N], const uint32_t* tab) {
#pragma unroll
    for (int c = 0; c + 1 < N; c += 2) {
        Sel sa[4], sb[4];
        sel16(sa, x[c]);
        sel16(sb, x[c + 1]);
#pragma unroll
        for (int r = 0; r < M; ++r)
            gf_mac16x2(acc[r], sa, sb, tab + (r * K + C0 + c) * QFEC_TAB_STRIDE, tab + (r * K + C0 + c + 1) * QFEC_TAB_STRIDE);
    }
    if (N & 1) {
        Sel s[4];
        sel16(s, x[N - 1]);
#pragma unroll
        for (int r = 0; r < M; ++r) gf_mac16(acc[r], s, tab + (r * K + C0 + N - 1) * QFEC_TAB_STRIDE);
    }
}

// ------------------------------------------------------------------ compares under block_size
// (qfec_verify.hip, qfec_locate.hip, qfec_locate_erased.hip: only bytes [0, block_size) of a row count)

// mask of the first `vb` bytes of a dword (vb <= 0: none, vb >= 4: all)
__device__ __forceinline__ uint32_t head_bytes(int vb) {
    return vb >= 4 ? 0xFFFFFFFFu : vb <= 0 ? 0u : ((1u << (8 * vb)) - 1u);
}

// bytes of the 16-B column `col` that lie inside the row's block_size bytes, as four dword masks
__device__ __forceinline__ uint4 column_mask(uint32_t block, uint32_t col) {
    const int nb = (int)std::min<uint32_t>(16u, block - col * 16u);
    return make_uint4(head_bytes(nb), head_bytes(nb - 4), head_bytes(nb - 8), head_bytes(nb - 12));
}

__device__ __forceinline__ bool differs(const uint4& acc, const uint4& p, const uint4& mk) {
    return (((acc.x ^ p.x) & mk.x) | ((acc.y ^ p.y) & mk.y) | ((acc.z ^ p.z) & mk.z) | ((acc.w ^ p.w) & mk.w)) != 0;
}

// ------------------------------------------------------------------ syndromes of 16 bytes
// (qfec_locate.hip, qfec_integrity_ptrs.hip)

__device__ __forceinline__ bool same16(const uint4& a, const uint4& b) {
    return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) == 0;
}

__device__ __forceinline__ bool nonzero16(const uint4& s) { return (s.x | s.y | s.z | s.w) != 0; }

// r x s0 over 16 bytes == sj ?  (both are zero in the masked bytes)
__device__ __forceinline__ bool ratio_holds(const Sel (&s0)[4], const uint4& sj, const uint32_t* __restrict__ r) {
    uint4 pr = make_uint4(0, 0, 0, 0);
    gf_mac16(pr, s0, r);
    return same16(pr, sj);
}

// ------------------------------------------------------------------ P x data on the flat mapping
// (qfec_verify.hip, qfec_locate.hip: one lane per 16-B column or per byte, the encode's perm tables)

// compile-time K, M: acc[r] ^= sum_c P[r][c] x data row c, for the 16-B column at src.  For K >= 16
// the inputs come in two halves, as in k_encode_perm_halves: half the input registers live at a time.
// The parity loads stay with the caller, ahead of this: with them in here the RS(10,3) instances
// come out at 61 VGPRs and 8 waves per SIMD where the loop written out in the kernel has 82 and 5.
template <int K, int M>
__device__ __forceinline__ void products16(uint4 (&acc)[M], const uint8_t* src, uint64_t pitch, const uint32_t* tab) {
    constexpr int H = K >= 16 ? (K + 1) / 2 : K;
#pragma unroll
    for (int c0 = 0; c0 < K; c0 += H) {
        if (H < K) __builtin_amdgcn_sched_barrier(0);  // the second half's loads stay below the first half's multiply
        constexpr int HH = H;
        const int n = min(HH, K - c0);
        uint4 x[H];
#pragma unroll
        for (int i = 0; i < H; ++i)
            if (i < n) x[i] = ld16(src + (uint64_t)(c0 + i) * pitch);
#pragma unroll
        for (int i = 0; i + 1 < H; i += 2) {
            if (i + 1 >= n) continue;
            Sel sa[4], sb[4];
            sel16(sa, x[i]);
            sel16(sb, x[i + 1]);
#pragma unroll
            for (int r = 0; r < M; ++r)
                gf_mac16x2(acc[r], sa, sb, tab + (r * K + c0 + i) * QFEC_TAB_STRIDE,
                           tab + (r * K + c0 + i + 1) * QFEC_TAB_STRIDE);
        }
        if (n & 1) {
            Sel sl[4];
            sel16(sl, x[n - 1]);
#pragma unroll
            for (int r = 0; r < M; ++r) gf_mac16(acc[r], sl, tab + (r * K + c0 + n - 1) * QFEC_TAB_STRIDE);
        }
    }
}

// runtime k, m: acc[j] = row r0 + j of the product, j < CH (rows past m stay zero); the k inputs are
// re-read per chunk of CH rows (cache hits)
template <int CH>
__device__ __forceinline__ void products16_rows(uint4 (&acc)[CH], const uint8_t* src, uint64_t pitch,
                                                const uint32_t* tab, int k, int m, int r0) {
#pragma unroll
    for (int j = 0; j < CH; ++j) acc[j] = make_uint4(0, 0, 0, 0);
    for (int c = 0; c < k; ++c) {
        const uint4 v = ld16(src + (uint64_t)c * pitch);
        Sel s[4];
        sel16(s, v);
#pragma unroll
        for (int j = 0; j < CH; ++j)
            if (r0 + j < m) gf_mac16(acc[j], s, tab + ((r0 + j) * k + c) * QFEC_TAB_STRIDE);
    }
}

// one byte of row r of the product (in the low byte; the rest is the product of zero bytes)
__device__ __forceinline__ uint32_t product_byte(const uint8_t* src, uint64_t pitch, const uint32_t* tab, int k, int r) {
    const uint32_t* tr = tab + (r * k) * QFEC_TAB_STRIDE;
    uint32_t acc = 0;
    for (int c = 0; c < k; ++c) {
        const uint32_t* tc = tr + c * QFEC_TAB_STRIDE;
        const Sel s = gf_sel((uint32_t)src[(uint64_t)c * pitch]);
        acc ^= gf_mul4(s, tc[0], tc[1], tc[2], tc[3], tc[4]);
    }
    return acc;
}

// ------------------------------------------------------------------ reporting, off the hot path

// A wave of the flat mapping reports its lanes' findings into the per-group words; every lane of the
// wave calls it.  bad = this lane's row bits for group g (0 for idle lanes and clean columns).  Per
// group seen in the wave the row bits are OR-reduced with ballots and one lane issues one atomic OR
// into bad_rows[g] (preset to zero): a group's columns span waves and blocks.
// CAND: cand = the shards that explain this lane's rows; AND-reduced likewise into cand_w[g] (preset
// to all ones).  Without it, the OR that finds the word still zero counts the group in *bad_groups
// (nullable), so a group is counted exactly once.
template <bool CAND>
__device__ __forceinline__ void flat_report(unsigned int* bad_rows, unsigned int* cand_w, unsigned int* bad_groups,
                                            int k, int m, uint32_t g, uint32_t bad, uint32_t cand) {
    uint64_t pending = __ballot(bad != 0);
    const int lane = threadIdx.x & 63;
    while (pending) {  // wave-uniform; one round per group with a finding in this wave
        const int leader = __builtin_ctzll(pending);
        const uint32_t gl = (uint32_t)__shfl((int)g, leader);
        const bool same = bad != 0 && g == gl;
        uint32_t rows = 0, keep = 0;
        for (int j = 0; j < m; ++j)
            if (__ballot(same && ((bad >> j) & 1u))) rows |= 1u << j;
        if constexpr (CAND) {
            for (int i = 0; i < k; ++i)
                if (!__ballot(same && !((cand >> i) & 1u))) keep |= 1u << i;
        }
        if (lane == leader) {
            const unsigned old = atomicOr(bad_rows + gl, rows);
            if constexpr (CAND) atomicAnd(cand_w + gl, keep);
            else if (old == 0 && bad_groups) atomicAdd(bad_groups, 1u);
        }
        pending &= ~__ballot(same);
    }
}

// Every thread of a 256-thread block calls it with its verdict (a counter index, or -1 for none).
// One add per block and counter, summed over the block's waves in LDS: adds on one address run one
// after the other (about 10 ns each, measured), and with every group damaged an add per lane took
// longer than the main kernel.
template <int N>
__device__ __forceinline__ void block_counts(int verdict, unsigned int* counts) {
    __shared__ unsigned int sum[N];
    if (threadIdx.x < N) sum[threadIdx.x] = 0;
    __syncthreads();
    for (int c = 0; c < N; ++c) {
        const uint64_t hit = __ballot(verdict == c);
        if (hit && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(hit)) atomicAdd(&sum[c], (unsigned)__builtin_popcountll(hit));
    }
    __syncthreads();
    if (threadIdx.x < N && sum[threadIdx.x]) atomicAdd(counts + threadIdx.x, sum[threadIdx.x]);
}

// group g's marks from a mask over its k + m shards (k, m <= 32), in the rs.c layout: every group's
// data marks, then every group's parity marks
__device__ __forceinline__ void write_marks_rs(uint8_t* marks, uint64_t groups, uint64_t g, int k, int m, uint64_t mask) {
    uint8_t* dm = marks + g * (uint64_t)k;
    uint8_t* pm = marks + groups * (uint64_t)k + g * (uint64_t)m;
    const uint32_t dmask = (uint32_t)mask, pmask = (uint32_t)(mask >> k);
    // four marks per store: at the vectoriser's own width of 8 the shifted copies cost more registers
#pragma clang loop vectorize_width(4)
    for (int i = 0; i < k; ++i) dm[i] = (dmask >> i) & 1u;
#pragma clang loop vectorize_width(4)
    for (int j = 0; j < m; ++j) pm[j] = (pmask >> j) & 1u;
}

}  // namespace qfec
