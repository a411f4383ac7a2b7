// qfec_verify.hip -- batched parity check for MI355X (gfx950): does parity[g] equal P x data[g]?
//
// The encode's mapping (qfec_kernels.hip): one lane per 16-byte column, (group, column) flattened
// over the grid, the same perm tables.  The m stores are replaced by m loads and compares, so a
// launch reads (k + m) rows per group and writes nothing unless a row differs.  The product is a
// true GF product: the rs.c stale-row flag of the encode tables is not applied.
//
// Only bytes [0, block_size) of a row count.  The last 16-B column of a row is compared under a
// byte mask, so whatever lies in [block_size, pitch) of either buffer cannot set a bit; GF
// multiplication is byte-wise, so garbage input bytes there reach only the masked output bytes.
//
// Reporting is off the hot path (mismatches are rare): a wave first reduces its lanes' row bits per
// group with ballots, then one lane issues one atomic OR per group the wave saw a mismatch in.
// The OR that finds the word still zero counts the group, so a group is counted exactly once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "qfec_internal.hpp"
#include "qfec_device.hpp"

namespace qfec {

// head_bytes, column_mask and differs (the tail-byte mask and the compare under it) are in
// qfec_device.hpp, shared with qfec_locate.hip.

// bad = this lane's row bits for group g (0 for idle lanes).  Every lane of the wave calls it.
__device__ __forceinline__ void verify_report(const VerifyArgs& a, uint32_t g, uint32_t bad) {
    uint64_t pending = __ballot(bad != 0);
    const int lane = threadIdx.x & 63;
    while (pending) {  // wave-uniform; one round per group with a mismatch in this wave
        const int leader = __builtin_ctzll(pending);
        const uint32_t gl = (uint32_t)__shfl((int)g, leader);
        const bool same = bad != 0 && g == gl;
        uint32_t rows = 0;
        for (int j = 0; j < a.m; ++j)
            if (__ballot(same && ((bad >> j) & 1u))) rows |= 1u << j;
        if (lane == leader) {
            const unsigned old = atomicOr(a.bad_rows + gl, rows);
            if (old == 0 && a.bad_groups) atomicAdd(a.bad_groups, 1u);
        }
        pending &= ~__ballot(same);
    }
}

// compile-time K, M.  For K >= 16 the inputs come in two halves, as in k_encode_perm_halves: half
// the input registers live at a time.
template <int K, int M>
__global__ void __launch_bounds__(256) k_verify_perm(VerifyArgs a) {
    constexpr int H = K >= 16 ? (K + 1) / 2 : K;
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t g32 = 0, bad = 0;
    if (t < a.work) {
        const uint64_t g = fast_div(t, a.cols_div);
        const uint32_t col = (uint32_t)(t - g * (uint64_t)a.cols);
        const uint8_t* src = a.data + g * a.dgs + (uint64_t)col * 16u;
        const uint8_t* par = a.parity + g * a.pgs + (uint64_t)col * 16u;
        const uint32_t* __restrict__ tab = a.tab;
        uint4 p[M];
#pragma unroll
        for (int r = 0; r < M; ++r) p[r] = ld16(par + (uint64_t)r * a.pitch);
        uint4 acc[M];
#pragma unroll
        for (int r = 0; r < M; ++r) acc[r] = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int c0 = 0; c0 < K; c0 += H) {
            if (H < K) __builtin_amdgcn_sched_barrier(0);  // the second half's loads stay below the first half's multiply
            constexpr int HH = H;
            const int n = min(HH, K - c0);
            uint4 x[H];
#pragma unroll
            for (int i = 0; i < H; ++i)
                if (i < n) x[i] = ld16(src + (uint64_t)(c0 + i) * a.pitch);
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
        const uint4 mk = column_mask(a.block, col);
#pragma unroll
        for (int r = 0; r < M; ++r)
            if (differs(acc[r], p[r], mk)) bad |= 1u << r;
        g32 = (uint32_t)g;
    }
    verify_report(a, g32, bad);
}

// runtime k, m (m <= 32): rows in chunks of VCH, the k inputs re-read per chunk (cache hits)
constexpr int VCH = 4;

__global__ void __launch_bounds__(256) k_verify_any(VerifyArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t g32 = 0, bad = 0;
    if (t < a.work) {
        const uint64_t g = fast_div(t, a.cols_div);
        const uint32_t col = (uint32_t)(t - g * (uint64_t)a.cols);
        const int k = a.k, m = a.m;
        const uint8_t* src = a.data + g * a.dgs + (uint64_t)col * 16u;
        const uint8_t* par = a.parity + g * a.pgs + (uint64_t)col * 16u;
        const uint4 mk = column_mask(a.block, col);
        for (int r0 = 0; r0 < m; r0 += VCH) {
            uint4 acc[VCH];
#pragma unroll
            for (int j = 0; j < VCH; ++j) acc[j] = make_uint4(0, 0, 0, 0);
            for (int c = 0; c < k; ++c) {
                const uint4 v = ld16(src + (uint64_t)c * a.pitch);
                Sel s[4];
                sel16(s, v);
#pragma unroll
                for (int j = 0; j < VCH; ++j)
                    if (r0 + j < m) gf_mac16(acc[j], s, a.tab + ((r0 + j) * k + c) * QFEC_TAB_STRIDE);
            }
#pragma unroll
            for (int j = 0; j < VCH; ++j)
                if (r0 + j < m && differs(acc[j], ld16(par + (uint64_t)(r0 + j) * a.pitch), mk)) bad |= 1u << (r0 + j);
        }
        g32 = (uint32_t)g;
    }
    verify_report(a, g32, bad);
}

// byte-granular fallback for pitches / pointers that are not 16-B aligned: one lane per byte of
// [0, block_size), so there is no tail to mask
__global__ void __launch_bounds__(256) k_verify_bytes(VerifyArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t g32 = 0, bad = 0;
    if (t < a.work) {
        const uint64_t g = fast_div(t, a.cols_div);
        const uint32_t b = (uint32_t)(t - g * (uint64_t)a.cols);
        const int k = a.k, m = a.m;
        const uint8_t* src = a.data + g * a.dgs + b;
        const uint8_t* par = a.parity + g * a.pgs + b;
        for (int r = 0; r < m; ++r) {
            const uint32_t* tr = a.tab + (r * k) * QFEC_TAB_STRIDE;
            uint32_t acc = 0;
            for (int c = 0; c < k; ++c) {
                const uint32_t* tc = tr + c * QFEC_TAB_STRIDE;
                const Sel s = gf_sel((uint32_t)src[(uint64_t)c * a.pitch]);
                acc ^= gf_mul4(s, tc[0], tc[1], tc[2], tc[3], tc[4]);
            }
            if ((uint8_t)acc != par[(uint64_t)r * a.pitch]) bad |= 1u << r;
        }
        g32 = (uint32_t)g;
    }
    verify_report(a, g32, bad);
}

#define QFEC_VER_CASE(KK, MM)                                                                    \
    if (a.k == KK && a.m == MM) {                                                                \
        hipLaunchKernelGGL((k_verify_perm<KK, MM>), dim3(grid), dim3(256), 0, stream, a);        \
        return hipGetLastError();                                                                \
    }

hipError_t launch_verify(const VerifyArgs& a, hipStream_t stream) {
    if (a.work == 0) return hipSuccess;
    if (a.work > 0x7FFFFFFFull || a.m > 32 || !a.bad_rows) return hipErrorInvalidValue;  // caller chunks
    const unsigned grid = (unsigned)((a.work + 255) / 256);
    if (!a.vec16) {
        hipLaunchKernelGGL(k_verify_bytes, dim3(grid), dim3(256), 0, stream, a);
        return hipGetLastError();
    }
    // the encode's instances (qfec_kernels.hip, launch_encode)
    QFEC_VER_CASE(10, 3)
    QFEC_VER_CASE(16, 4)
    QFEC_VER_CASE(4, 2)
    QFEC_VER_CASE(2, 1)
    QFEC_VER_CASE(2, 2)
    QFEC_VER_CASE(3, 1)
    QFEC_VER_CASE(3, 2)
    QFEC_VER_CASE(4, 1)
    QFEC_VER_CASE(5, 1)
    QFEC_VER_CASE(5, 3)
    QFEC_VER_CASE(6, 2)
    QFEC_VER_CASE(7, 1)
    QFEC_VER_CASE(8, 2)
    QFEC_VER_CASE(8, 4)
    QFEC_VER_CASE(12, 4)
    QFEC_VER_CASE(20, 4)
    hipLaunchKernelGGL(k_verify_any, dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace qfec
