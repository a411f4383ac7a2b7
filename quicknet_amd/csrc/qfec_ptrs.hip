// qfec_ptrs.hip -- encode and reconstruct on shards scattered in device memory, for MI355X (gfx950):
// the caller hands over a device table of shard addresses (module/rs.h's `unsigned char **shards`)
// in place of the two contiguous regions of qfec_encode / qfec_reconstruct.  A shard is exactly
// block_size bytes, at any alignment, and no byte outside it is read or written.
//
// Mapping: the reconstruct's, for both calls -- one wave per (group, slab of 64 columns), four waves
// per block.  A wave then sits inside one group, so the group's addresses (and, in the reconstruct,
// its erasure pattern and decode tables) are wave-uniform.  The encode's flat (group, column)
// mapping does not carry over: at B = 1000 its waves span two groups, and every lane would need
// its own k + m addresses.
//
// How the addresses reach the wave: lane s < k + m loads the address of shard s of its group -- in
// the reconstruct in the same round trip as mark s -- and the wave reads what it needs out of that
// register with one v_readlane per shard (the lane index is wave-uniform: a constant in the encode,
// a bit position of the ballot in the reconstruct).  Nothing depends on a second load: the survivor
// loads issue right after the ballot, as in k_reconstruct_perm.  The runtime-k,m encode (k + m may
// pass 64) reads the table through its __restrict__ parameter instead.
//
// Alignment is judged per group, inside the kernel (the host cannot know it without reading the
// table): a group all of whose k + m addresses are 16-B aligned runs the vector body on its whole
// columns, and the block_size % 16 (% 8 on 8-B lanes) bytes after them go byte by byte to the first
// lanes of the group's last wave.  Any other group runs the same waves over the same spans byte by
// byte, 64 consecutive bytes per wave access: misaligned 16-B loads are free (tools/unaligned.hip),
// misaligned 16-B stores are unmeasured.
//
// Bodies: the vector bodies are those of the contiguous kernels, from qfec_device.hpp -- the
// encode's multiply-accumulate (enc_mac16) and the reconstruct's exact-e column
// (recon_column_by_e).  The byte bodies, shared by the templated and the runtime-k,m kernels, load a
// lane's k input bytes at once where k is a template constant and keep the loop over the output
// rows rolled: unrolled over the rows as well, next to the vector body, they cost it registers
// (RS(10,3) encode: 174 VGPRs against 92).  Lane width: 16 B, except the reconstruct of k >= 10 on 8 B,
// as its contiguous auto body (ptrs_lane_bytes, qfec_geom.hpp).  No residency cap and no one-wave
// blocks: those were measured for the contiguous access pattern only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "qfec_internal.hpp"
#include "qfec_device.hpp"
#include "qfec_geom.hpp"
#include "qfec_ptrs_device.hpp"

namespace qfec {

// ------------------------------------------------------------------ encode

// byte b of the m parity shards from byte b of the k data shards; row(s) = the address of shard s.
// K > 0 (k == K): the K input bytes are loaded at once and the loop over the rows has the K columns
// unrolled, so a lane waits for one round trip and not for k * m of them; the rows stay a rolled
// loop, which keeps the registers of the vector body next to it where they are.
template <int K, class Row>
__device__ __forceinline__ void encode_byte(int k, int m, const uint32_t* tab, const Row& row, uint64_t b) {
    uint32_t x[K > 0 ? K : 1];
    if constexpr (K > 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) x[c] = as_row(row(c))[b];
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
#pragma unroll 4
            for (int c = 0; c < k; ++c) {
                const uint32_t* tc = tr + c * QFEC_TAB_STRIDE;
                acc ^= gf_mul4(gf_sel((uint32_t)as_row(row(c))[b]), tc[0], tc[1], tc[2], tc[3], tc[4]);
            }
        }
        *out = (uint8_t)acc;
    }
}

// the vector body, encode_column, is in qfec_ptrs_device.hpp (qfec_ptrs_var.hip runs it too)

// __restrict__ parameters: the address table and the encode tables are not written by the launch,
// so their loads need not be ordered against the stores
template <int K, int M>
__global__ void __launch_bounds__(256) k_encode_ptrs(PtrsArgs a, const uint64_t* __restrict__ dptrs,
                                                     const uint64_t* __restrict__ pptrs,
                                                     const uint32_t* __restrict__ tab) {
    constexpr int N = K + M;
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a, &g, &slab)) return;
    uint64_t p = 0;
    if (lane < K) p = dptrs[g * K + lane];
    else if (lane < N) p = pptrs[g * M + (lane - K)];
    const bool aligned = __ballot((p & 15u) != 0) == 0;
    run_slab<16>(
        a, slab, lane, aligned,
        [&](uint64_t off) {
            const uint8_t* src[K];
            uint8_t* dst[M];
#pragma unroll
            for (int c = 0; c < K; ++c) src[c] = as_row(lane_value(p, c));
#pragma unroll
            for (int r = 0; r < M; ++r) dst[r] = as_out(lane_value(p, K + r));
            encode_column<K, M>(src, dst, tab, off);
        },
        [&](uint64_t b) { encode_byte<K>(K, M, tab, [&](int s) { return lane_value(p, s); }, b); });
}

// runtime k, m (k + m may pass 64 lanes: the addresses are read from the table where they are used);
// output rows in chunks of PCH, the k inputs re-read per chunk (cache hits)
constexpr int PCH = 4;

__global__ void __launch_bounds__(256) k_encode_ptrs_any(PtrsArgs a, const uint64_t* __restrict__ dptrs,
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
    run_slab<16>(
        a, slab, lane, aligned,
        [&](uint64_t off) {
            for (int r0 = 0; r0 < m; r0 += PCH) {
                uint4 acc[PCH];
#pragma unroll
                for (int j = 0; j < PCH; ++j) {
                    acc[j] = make_uint4(0, 0, 0, 0);
                    if (r0 + j < m && tab[((r0 + j) * k) * QFEC_TAB_STRIDE + 5])
                        acc[j] = *reinterpret_cast<const uint4*>(as_row(pp[r0 + j]) + off);
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
                    if (r0 + j < m) st16(as_out(pp[r0 + j]) + off, acc[j]);
            }
        },
        [&](uint64_t b) { encode_byte<0>(k, m, tab, [&](int s) { return s < k ? dp[s] : pp[s - k]; }, b); });
}

// ------------------------------------------------------------------ reconstruct

// lane s < n: mark s and address s of group g, in one round trip; the rest zero
__device__ __forceinline__ void marks_and_rows(const uint64_t* __restrict__ dptrs, const uint64_t* __restrict__ pptrs,
                                               const uint8_t* __restrict__ dmarks, const uint8_t* __restrict__ pmarks,
                                               uint64_t g, int k, int m, int lane, uint32_t* mk, uint64_t* p) {
    *mk = 0;
    *p = 0;
    if (lane < k) {
        *mk = dmarks[g * (uint64_t)k + lane];
        *p = dptrs[g * (uint64_t)k + lane];
    } else if (lane < k + m) {
        *mk = pmarks[g * (uint64_t)m + (lane - k)];
        *p = pptrs[g * (uint64_t)m + (lane - k)];
    }
}

// byte b of the group's erased data shards, from the whole decode record r (survivor ids, erased
// ids and its inline tables, RecordLayout); p: the lanes' addresses.  Rolled loops: with the k
// bytes loaded at once, as in encode_byte, the RS(16,4) kernel goes from 68 to 100 VGPRs.
__device__ __forceinline__ void recon_byte(const PtrsArgs& a, const uint32_t* r, uint64_t p, uint64_t b) {
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
            acc ^= gf_mul4(gf_sel((uint32_t)as_row(lane_value(p, surv[c]))[b]), tc[0], tc[1], tc[2], tc[3], tc[4]);
        }
        *out = (uint8_t)acc;
    }
}

// LUT mode, compile-time K, M; D dwords per lane.  As k_reconstruct_perm: the survivors are the K
// lowest unmarked shards, known from the ballot alone, so their loads issue while the decode record
// is still in flight.
template <int K, int M, int D>
__global__ void __launch_bounds__(256) k_reconstruct_ptrs(PtrsArgs a, const uint64_t* __restrict__ dptrs,
                                                          const uint64_t* __restrict__ pptrs,
                                                          const uint8_t* __restrict__ dmarks,
                                                          const uint8_t* __restrict__ pmarks,
                                                          const int32_t* __restrict__ lut,
                                                          const uint32_t* __restrict__ records) {
    constexpr int N = K + M;
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a, &g, &slab)) return;
    uint32_t mk;
    uint64_t p;
    marks_and_rows(dptrs, pptrs, dmarks, pmarks, g, K, M, lane, &mk, &p);
    const uint64_t mask = __ballot(mk != 0) & ((1ull << N) - 1ull);
    const uint64_t lost_bits = mask & ((1ull << K) - 1ull);
    const int e = __builtin_popcountll(lost_bits);
    if (e == 0) return;
    const uint64_t avail = ~mask & ((1ull << N) - 1ull);
    const int rec = __builtin_popcountll(avail) < K ? QFEC_REC_FAIL
                                                    : ((const __attribute__((address_space(4))) int32_t*)lut)[mask];
    if (rec < 0) {  // under-determined (or a singular decode matrix of explicit rows): untouched, counted
        if (slab == 0 && lane == 0 && a.failed) atomicAdd(a.failed, 1u);
        return;
    }
    const bool aligned = __ballot((p & 15u) != 0) == 0;
    run_slab<4 * D>(
        a, slab, lane, aligned,
        [&](uint64_t off) {
            const RTab T{records + rec, a.coff, a.t256};
            uint64_t left = avail;
            const uint8_t* src[K];
#pragma unroll
            for (int c = 0; c < K; ++c) {
                const uint32_t s = (uint32_t)__builtin_ctzll(left);
                left &= left - 1;
                src[c] = as_row(lane_value(p, s));
            }
            recon_column_by_e<K, M, D>(src, nullptr, LaneRows{p}, lost_bits, T, e, off);
        },
        [&](uint64_t b) { recon_byte(a, records + rec, p, b); });
}

// runtime k, m (k + m <= QFEC_LUT_MAX_N, so the lanes hold the addresses here too), e from the
// record, whose tables are inline; rows in chunks of PCH
template <int D>
__global__ void __launch_bounds__(256) k_reconstruct_ptrs_any(PtrsArgs a, const uint64_t* __restrict__ dptrs,
                                                              const uint64_t* __restrict__ pptrs,
                                                              const uint8_t* __restrict__ dmarks,
                                                              const uint8_t* __restrict__ pmarks,
                                                              const int32_t* __restrict__ lut,
                                                              const uint32_t* __restrict__ records) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a, &g, &slab)) return;
    const int k = a.k, n = a.k + a.m;
    uint32_t mk;
    uint64_t p;
    marks_and_rows(dptrs, pptrs, dmarks, pmarks, g, k, a.m, lane, &mk, &p);
    const uint32_t mask = (uint32_t)(__ballot(mk != 0) & ((1ull << n) - 1ull));
    if (!(mask & ((1u << k) - 1u))) return;
    const int rec = __builtin_amdgcn_readfirstlane(lut[mask]);
    if (rec < 0) {
        if (rec == QFEC_REC_FAIL && slab == 0 && lane == 0 && a.failed) atomicAdd(a.failed, 1u);
        return;
    }
    const uint32_t* r = records + rec;
    const int e = (int)r[0];
    const uint32_t* surv = r + a.surv_off;
    const uint32_t* lost = r + a.lost_off;
    const uint32_t* tab = r + a.hdr;
    const bool aligned = __ballot((p & 15u) != 0) == 0;
    run_slab<4 * D>(
        a, slab, lane, aligned,
        [&](uint64_t off) {
            for (int j0 = 0; j0 < e; j0 += PCH) {
                uint32_t acc[PCH][D];
#pragma unroll
                for (int j = 0; j < PCH; ++j) {
#pragma unroll
                    for (int d = 0; d < D; ++d) acc[j][d] = 0;
                    if (j0 + j < e && tab[((j0 + j) * k) * QFEC_TAB_STRIDE + 5])
                        ldv_plain<D>(acc[j], as_row(lane_value(p, lost[j0 + j])) + off);
                }
                for (int c = 0; c < k; ++c) {
                    uint32_t x[D];
                    ldv<D>(x, as_row(lane_value(p, surv[c])) + off);
#pragma unroll
                    for (int j = 0; j < PCH; ++j)
                        if (j0 + j < e) {
                            const uint32_t* tc = tab + ((j0 + j) * k + c) * QFEC_TAB_STRIDE;
#pragma unroll
                            for (int d = 0; d < D; ++d) acc[j][d] ^= gf_mul4(gf_sel(x[d]), tc[0], tc[1], tc[2], tc[3], tc[4]);
                        }
                }
#pragma unroll
                for (int j = 0; j < PCH; ++j)
                    if (j0 + j < e) stv<D>(as_out(lane_value(p, lost[j0 + j])) + off, acc[j]);
            }
        },
        [&](uint64_t b) { recon_byte(a, r, p, b); });
}

// ------------------------------------------------------------------ launchers

// blocks of four waves over groups * wpg waves; false when the caller has to chunk or the geometry
// is not the one the kernels are built for
static inline bool ptrs_grid(const PtrsArgs& a, bool reconstruct, unsigned* grid) {
    const uint64_t waves = a.groups * (uint64_t)a.wpg;
    if (a.wpg == 0 || waves * 64 > (uint64_t)kMaxLaunchLanes) return false;
    if ((int)a.lane_bytes != ptrs_lane_bytes(reconstruct, a.k)) return false;
    *grid = (unsigned)((waves + 3) / 4);
    return true;
}

#define QFEC_PENC_CASE(KK, MM)                                                                                     \
    if (a.k == KK && a.m == MM) {                                                                                  \
        hipLaunchKernelGGL((k_encode_ptrs<KK, MM>), dim3(grid), dim3(256), 0, stream, a, a.dptrs, a.pptrs, a.tab); \
        return hipGetLastError();                                                                                  \
    }

hipError_t launch_encode_ptrs(const PtrsArgs& a, hipStream_t stream) {
    if (a.groups == 0 || a.m == 0) return hipSuccess;
    unsigned grid;
    if (!ptrs_grid(a, false, &grid)) return hipErrorInvalidValue;
    QFEC_PENC_CASE(10, 3)
    QFEC_PENC_CASE(16, 4)
    QFEC_PENC_CASE(4, 2)
    QFEC_PENC_CASE(8, 4)
    hipLaunchKernelGGL(k_encode_ptrs_any, dim3(grid), dim3(256), 0, stream, a, a.dptrs, a.pptrs, a.tab);
    return hipGetLastError();
}

// the lane width of an instance is ptrs_lane_bytes' (8 B for k >= 10)
#define QFEC_PREC_CASE(KK, MM)                                                                                   \
    if (a.k == KK && a.m == MM) {                                                                                \
        hipLaunchKernelGGL((k_reconstruct_ptrs<KK, MM, (KK >= 10 ? 2 : 4)>), dim3(grid), dim3(256), 0, stream, a, \
                           a.dptrs, a.pptrs, a.dmarks, a.pmarks, a.lut, a.records);                              \
        return hipGetLastError();                                                                                \
    }

hipError_t launch_reconstruct_ptrs(const PtrsArgs& a, hipStream_t stream) {
    if (a.groups == 0) return hipSuccess;
    unsigned grid;
    if (a.k + a.m > QFEC_LUT_MAX_N || !ptrs_grid(a, true, &grid)) return hipErrorInvalidValue;
    QFEC_PREC_CASE(10, 3)
    QFEC_PREC_CASE(16, 4)
    QFEC_PREC_CASE(4, 2)
    QFEC_PREC_CASE(8, 4)
    if (a.lane_bytes == 8)
        hipLaunchKernelGGL((k_reconstruct_ptrs_any<2>), dim3(grid), dim3(256), 0, stream, a, a.dptrs, a.pptrs, a.dmarks,
                           a.pmarks, a.lut, a.records);
    else
        hipLaunchKernelGGL((k_reconstruct_ptrs_any<4>), dim3(grid), dim3(256), 0, stream, a, a.dptrs, a.pptrs, a.dmarks,
                           a.pmarks, a.lut, a.records);
    return hipGetLastError();
}

}  // namespace qfec
