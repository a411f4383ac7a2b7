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

// The product bodies, the tail-byte mask and the compare under it, and the report (flat_report) are
// in qfec_device.hpp, shared with qfec_locate.hip.

// compile-time K, M
template <int K, int M>
__global__ void __launch_bounds__(256) k_verify_perm(VerifyArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t g32 = 0, bad = 0;
    if (t < a.work) {
        const uint64_t g = fast_div(t, a.cols_div);
        const uint32_t col = (uint32_t)(t - g * (uint64_t)a.cols);
        const uint8_t* src = a.data + g * a.dgs + (uint64_t)col * 16u;
        const uint8_t* par = a.parity + g * a.pgs + (uint64_t)col * 16u;
        uint4 p[M], acc[M];
#pragma unroll
        for (int r = 0; r < M; ++r) p[r] = ld16(par + (uint64_t)r * a.pitch);
#pragma unroll
        for (int r = 0; r < M; ++r) acc[r] = make_uint4(0, 0, 0, 0);
        products16<K, M>(acc, src, a.pitch, a.tab);
        const uint4 mk = column_mask(a.block, col);
#pragma unroll
        for (int r = 0; r < M; ++r)
            if (differs(acc[r], p[r], mk)) bad |= 1u << r;
        g32 = (uint32_t)g;
    }
    flat_report<false>(a.bad_rows, nullptr, a.bad_groups, a.k, a.m, g32, bad, 0);
}

// runtime k, m (m <= 32): rows in chunks of VCH
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
            products16_rows<VCH>(acc, src, a.pitch, a.tab, k, m, r0);
#pragma unroll
            for (int j = 0; j < VCH; ++j)
                if (r0 + j < m && differs(acc[j], ld16(par + (uint64_t)(r0 + j) * a.pitch), mk)) bad |= 1u << (r0 + j);
        }
        g32 = (uint32_t)g;
    }
    flat_report<false>(a.bad_rows, nullptr, a.bad_groups, a.k, a.m, g32, bad, 0);
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
        for (int r = 0; r < m; ++r)
            if ((uint8_t)product_byte(src, a.pitch, a.tab, k, r) != par[(uint64_t)r * a.pitch]) bad |= 1u << r;
        g32 = (uint32_t)g;
    }
    flat_report<false>(a.bad_rows, nullptr, a.bad_groups, a.k, a.m, g32, bad, 0);
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
