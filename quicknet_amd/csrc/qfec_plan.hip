// qfec_plan.hip -- device-built decode plans (qfec_plan_build / qfec_plan_apply of include/qfec.h):
// the decode matrix of every group from the group's marks, on the device, at any k + m.  No LUT, no
// host inversion, no read-back.
//
// k_plan_build: one wave (a 64-thread block) per group.  The marks are read in passes of 64 lanes,
// one ballot each (k + m reaches 256: four); everything else is plan_group of qfec_plan.hpp, the
// text the host query qfec_plan_build_host runs, with the wave as its lanes and LDS as its working
// memory: the GF exp / log tables (768 B), the plan's head, [M | I] and the row factors.
//
// k_plan_apply: the reconstruct's mapping, a wave per (group, 64 columns).  Status, t, ids and
// coefficients are wave-uniform and come through scalar loads from the plan; each coefficient
// indexes the 256-entry perm table.  With k in the hundreds the survivors cannot stay in registers:
// the kernel loops over the k survivors and accumulates up to PCH output rows per pass, so for
// t <= PCH every survivor byte is loaded once; above that each pass of PCH rows re-reads them.
#include "qfec_device.hpp"
#include "qfec_plan.hpp"

namespace qfec {

constexpr int PCH = 8;  // output rows per pass of k_plan_apply

__global__ void __launch_bounds__(64) k_plan_build(PlanBuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];  // [exp 512 | log 256][plan_work_bytes]
    const int lane = threadIdx.x;
    const uint64_t g = blockIdx.x;
    if (g >= a.groups) return;
    const int k = a.k, m = a.m, n = k + m;
    for (int i = lane; i < QFEC_PLAN_GF_BYTES / 4; i += 64)
        reinterpret_cast<uint32_t*>(lds)[i] = reinterpret_cast<const uint32_t*>(a.gf)[i];
    // data marks at dmarks[g*k + i], parity marks at pmarks[g*m + j]: the two ranges meet at any lane
    uint64_t mk[4] = {0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int i = p * 64 + lane;
        uint32_t v = 0;
        if (i < k) v = a.dmarks[g * (uint64_t)k + i];
        else if (i < n) v = a.pmarks[g * (uint64_t)m + (i - k)];
        mk[p] = __ballot(v != 0);
    }
    __syncthreads();
    const PlanCode C{reinterpret_cast<const uint8_t*>(a.tab + 7), QFEC_TAB_STRIDE * 4, k, m, a.quirk, lds, lds + 512};
    const int status = plan_group(C, mk, a.mode, lds + QFEC_PLAN_GF_BYTES, a.plan + g * a.stride, PlanWaveLanes{lane});
    if (status == QFEC_PLAN_FAILED && lane == 0 && a.failed) atomicAdd(a.failed, 1u);
}

// byte idx of the plan through a scalar dword load
__device__ __forceinline__ uint32_t plan_u8(cptr32 pw, int idx) { return (pw[idx >> 2] >> ((idx & 3) * 8)) & 0xFFu; }

template <bool VEC16>
__global__ void __launch_bounds__(256) k_plan_apply(PlanApplyArgs a, const uint8_t* __restrict__ plan) {
    const int lane = threadIdx.x & 63;
    const uint32_t wid = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t g = wid / a.wpg;
    const uint32_t part = wid - g * a.wpg;
    if (g >= a.groups) return;
    const int k = a.k, m = a.m, n = k + m;
    const PlanLayout PL = plan_layout(k, m);
    const cptr32 pw = (cptr32)(plan + (uint64_t)g * a.stride);
    const cptr32 t256 = (cptr32)a.t256;
    const int t = (int)(pw[0] & 0xFFFFu);
    if ((pw[1] & 0xFFu) != (uint32_t)QFEC_PLAN_WORK || t > m) return;
    const uint32_t col = part * 64u + lane;
    if (col >= a.cols) return;
    const uint64_t off = VEC16 ? (uint64_t)col * 16u : col;
    uint8_t* data_g = a.data + (uint64_t)g * a.dgs;
    uint8_t* par_g = a.parity + (uint64_t)g * a.pgs;
    auto row = [&](uint32_t s) -> uint8_t* {
        return s < (uint32_t)k ? data_g + (uint64_t)s * a.pitch : par_g + (uint64_t)(s - k) * a.pitch;
    };
    using Acc = typename std::conditional<VEC16, uint4, uint32_t>::type;

    for (int j0 = 0; j0 < t; j0 += PCH) {
        Acc acc[PCH];
#pragma unroll
        for (int j = 0; j < PCH; ++j) {
            const int jj = j0 + j;
            // a stale row starts from the destination's previous bytes (rs.c column-0 quirk)
            const bool stale = jj < t && plan_u8(pw, PL.stale_off + jj) != 0;
            if constexpr (VEC16) {
                acc[j] = make_uint4(0, 0, 0, 0);
                if (stale) acc[j] = *reinterpret_cast<const uint4*>(row(plan_u8(pw, PL.lost_off + jj)) + off);
            } else {
                acc[j] = 0;
                if (stale) acc[j] = row(plan_u8(pw, PL.lost_off + jj))[off];
            }
        }
        for (int c = 0; c < k; ++c) {
            const uint32_t s = plan_u8(pw, PL.surv_off + c);
            if (s >= (uint32_t)n) return;  // not a plan of this code
            const uint8_t* src = row(s) + off;
            if constexpr (VEC16) {
                const uint4 v = ld16(src);
                Sel sl[4];
                sel16(sl, v);
#pragma unroll
                for (int j = 0; j < PCH; ++j)
                    if (j0 + j < t) {
                        const cptr32 tc = t256 + plan_u8(pw, PL.coef_off + (j0 + j) * k + c) * QFEC_TAB_STRIDE;
                        const uint32_t t0 = tc[0], t1 = tc[1], t2 = tc[2], t3 = tc[3], t4 = tc[4];
                        acc[j].x = xor3(acc[j].x, pp0(sl[0], t0, t1), pp1(sl[0], t2, t3)) ^ pp2(sl[0], t4);
                        acc[j].y = xor3(acc[j].y, pp0(sl[1], t0, t1), pp1(sl[1], t2, t3)) ^ pp2(sl[1], t4);
                        acc[j].z = xor3(acc[j].z, pp0(sl[2], t0, t1), pp1(sl[2], t2, t3)) ^ pp2(sl[2], t4);
                        acc[j].w = xor3(acc[j].w, pp0(sl[3], t0, t1), pp1(sl[3], t2, t3)) ^ pp2(sl[3], t4);
                    }
            } else {
                const Sel sl = gf_sel((uint32_t)*src);
#pragma unroll
                for (int j = 0; j < PCH; ++j)
                    if (j0 + j < t) {
                        const cptr32 tc = t256 + plan_u8(pw, PL.coef_off + (j0 + j) * k + c) * QFEC_TAB_STRIDE;
                        acc[j] ^= gf_mul4(sl, tc[0], tc[1], tc[2], tc[3], tc[4]);
                    }
            }
        }
#pragma unroll
        for (int j = 0; j < PCH; ++j)
            if (j0 + j < t) {
                const uint32_t l = plan_u8(pw, PL.lost_off + j0 + j);
                if (l >= (uint32_t)n) continue;
                if constexpr (VEC16) st16(row(l) + off, acc[j]);
                else row(l)[off] = (uint8_t)acc[j];
            }
    }
}

hipError_t launch_plan_build(const PlanBuildArgs& a, hipStream_t stream) {
    if (a.groups == 0) return hipSuccess;
    if (a.groups > 0x7FFFFFFFull / 64u || a.lds > 65536u) return hipErrorInvalidValue;  // caller chunks
    hipLaunchKernelGGL(k_plan_build, dim3((unsigned)a.groups), dim3(64), a.lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_plan_apply(const PlanApplyArgs& a, hipStream_t stream) {
    if (a.groups == 0 || a.cols == 0) return hipSuccess;
    const uint64_t waves = a.groups * (uint64_t)a.wpg;
    if (a.wpg == 0 || waves * 64u > 0x7FFFFFFFull) return hipErrorInvalidValue;  // caller chunks
    const unsigned grid = (unsigned)((waves + 3) / 4);
    if (a.vec16) hipLaunchKernelGGL((k_plan_apply<true>), dim3(grid), dim3(256), 0, stream, a, a.plan);
    else hipLaunchKernelGGL((k_plan_apply<false>), dim3(grid), dim3(256), 0, stream, a, a.plan);
    return hipGetLastError();
}

}  // namespace qfec
