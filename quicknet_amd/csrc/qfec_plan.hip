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
//
// k_plan_apply_ptrs: the same column body (plan_column) where the rows are given by a device table of
// shard addresses (qfec_plan_apply_ptrs), in the mapping of the pointer-table kernels of qfec_ptrs.hip.
//
// k_plan_apply_ptrs_var: the same where every data shard has its own length (qfec_plan_apply_ptrs_var),
// with the lengths, the per-group geometry and the clipped loads of qfec_ptrs_var.hip; a wave whose
// survivors all reach its columns runs plan_column unchanged, any other plan_column_var.
//
// k_plan_apply_ptrs_var_clip: the same wave where one listed data shard per group, the shard a locate
// found, is written up to its own length only (the repair of qfec_scrub_ptrs_wide_var).
#include "qfec_device.hpp"
#include "qfec_geom.hpp"
#include "qfec_plan.hpp"
#include "qfec_ptrs_device.hpp"

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

// One column of a group through its plan: byte (VEC16: the 16 bytes at) `off` of the t listed rows
// from the k survivors.  row(s) = where shard s of the group starts, s wave-uniform.  Where the ids
// are not those of a plan of this code nothing more is done for the column.
template <bool VEC16, class Row>
__device__ __forceinline__ void plan_column(cptr32 pw, const PlanLayout& PL, cptr32 t256, int k, int n, int t,
                                            const Row& row, uint64_t off) {
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
    plan_column<VEC16>(pw, PL, t256, k, n, t, row, off);
}

// The same on a table of shard addresses: the pointer-table kernels' mapping and geometry (a wave
// per (group, slab of 64 16-B columns), the block % 16 tail and the byte body of a group with a
// misaligned address: run_slab), plan_column for the work.  NP passes of 64 lanes hold the group's
// k + m <= 64 * NP addresses, entry q * 64 + lane in register q of the lane, and the address of the
// wave-uniform shard id s is a v_readlane of register s >> 6 at lane s & 63.
// Every lane loads its entries before anything depends on the lane: a lane without a column of its
// own (B = 16: all but one; the last wave of a row) still holds addresses the others read, so the
// work below is predicated (run_slab) and no lane leaves early.  The alignment ballot uses the
// loaded values, which also keeps the loads above the first lane-dependent branch.
template <int NP>
__global__ void __launch_bounds__(256) k_plan_apply_ptrs(PlanPtrsArgs a, const uint64_t* __restrict__ dptrs,
                                                         const uint64_t* __restrict__ pptrs,
                                                         const uint8_t* __restrict__ plan) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a, &g, &slab)) return;
    const int k = a.k, m = a.m, n = k + m;
    uint64_t p[NP];
    uint32_t low = 0;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int i = q * 64 + lane;
        p[q] = 0;
        if (i < k) p[q] = dptrs[g * (uint64_t)k + i];
        else if (i < n) p[q] = pptrs[g * (uint64_t)m + (i - k)];
        low |= (uint32_t)p[q] & 15u;
    }
    const bool aligned = __ballot(low != 0) == 0;
    const PlanLayout PL = plan_layout(k, m);
    const cptr32 pw = (cptr32)(plan + g * a.stride);
    const cptr32 t256 = (cptr32)a.t256;
    const int t = (int)(pw[0] & 0xFFFFu);
    if ((pw[1] & 0xFFu) != (uint32_t)QFEC_PLAN_WORK || t > m) return;  // wave-uniform
    auto row = [&](uint32_t s) -> uint8_t* {
        const uint32_t l = s & 63u;
        if constexpr (NP == 1) return as_out(lane_value(p[0], l));
        const uint32_t r = s >> 6;
        if constexpr (NP == 2) return as_out(r == 0 ? lane_value(p[0], l) : lane_value(p[1], l));
        else
            return as_out(r == 0   ? lane_value(p[0], l)
                          : r == 1 ? lane_value(p[1], l)
                          : r == 2 ? lane_value(p[NP > 2 ? 2 : 0], l)
                                   : lane_value(p[NP > 3 ? 3 : 0], l));
    };
    run_slab<16>(
        a, slab, lane, aligned, [&](uint64_t off) { plan_column<true>(pw, PL, t256, k, n, t, row, off); },
        [&](uint64_t b) { plan_column<false>(pw, PL, t256, k, n, t, row, b); });
}

// plan_column where survivor s may be read in [0, eff(s)) only and counts as zero from there on
// (qfec_plan_apply_ptrs_var): the same passes of PCH rows, the same scalar reads of the plan.  VEC16:
// a survivor's 16 bytes at `off` come through ldv_clip -- the whole column, its first bytes in pieces
// of 8, 4, 2 and 1, or nothing and then no load; else byte `off`, read when it lies below eff(s).  The
// listed rows are whole in [0, L) and `off` lies inside it: the stale loads and the stores are
// plan_column's.  Room (k_plan_apply_ptrs_var_clip only): listed row l has room(l) <= L bytes, and no
// byte at or past them is read or written.
struct WholeRoom {
    static constexpr bool clips = false;
};
template <class F>
struct ClippedRoom {
    static constexpr bool clips = true;
    F of;
};

// the first n < 16 bytes of v to q, byte by byte: one lane of one located shard per call
__device__ __forceinline__ void st16_part(uint8_t* q, const uint4& v, uint32_t n) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll 1
    for (uint32_t b = 0; b < n; ++b) q[b] = (uint8_t)(w[b >> 2] >> (8u * (b & 3u)));
}

template <bool VEC16, class Row, class Eff, class Room = WholeRoom>
__device__ __forceinline__ void plan_column_var(cptr32 pw, const PlanLayout& PL, cptr32 t256, int k, int n, int t,
                                                const Row& row, const Eff& eff, uint32_t off, const Room& room = Room{}) {
    using Acc = typename std::conditional<VEC16, uint4, uint32_t>::type;

    for (int j0 = 0; j0 < t; j0 += PCH) {
        Acc acc[PCH];
#pragma unroll
        for (int j = 0; j < PCH; ++j) {
            const int jj = j0 + j;
            const bool stale = jj < t && plan_u8(pw, PL.stale_off + jj) != 0;
            if constexpr (Room::clips) {
                const uint32_t l = plan_u8(pw, PL.lost_off + jj);
                if constexpr (VEC16) {
                    acc[j] = make_uint4(0, 0, 0, 0);
                    if (stale) acc[j] = ld16_clip(row(l), off, room.of(l));
                } else {
                    acc[j] = 0;
                    if (stale && off < room.of(l)) acc[j] = row(l)[off];
                }
            } else if constexpr (VEC16) {
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
            const uint8_t* src = row(s);
            const uint32_t len = eff(s);
            if constexpr (VEC16) {
                uint32_t x[4];
                ldv_clip<4>(x, src, off, len);
                Sel sl[4];
                sel16(sl, make_uint4(x[0], x[1], x[2], x[3]));
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
                const Sel sl = gf_sel(off < len ? (uint32_t)src[off] : 0u);
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
                if constexpr (Room::clips) {
                    const uint32_t end = room.of(l);
                    if constexpr (VEC16) {
                        if (off + 16u <= end) st16(row(l) + off, acc[j]);
                        else if (off < end) st16_part(row(l) + off, acc[j], end - off);
                    } else {
                        if (off < end) row(l)[off] = (uint8_t)acc[j];
                    }
                } else if constexpr (VEC16) st16(row(l) + off, acc[j]);
                else row(l)[off] = (uint8_t)acc[j];
            }
    }
}

// k_plan_apply_ptrs where every data shard has its own length (qfec_plan_apply_ptrs_var): data shard
// i of a group is len_i bytes and counts as zero-filled up to the group's length L = glen[g], the
// length of its parity shards.  Mapping and address loads are k_plan_apply_ptrs's, the launch has
// ptrs_geom(max_len, 16).wpg waves per group.  New here:
//
// Lengths.  Lane q * 64 + lane < k loads its length in the same round trip as its address; with L, a
// scalar load, that makes NP registers of readable length eff (len_i of a data shard, L of a parity
// shard), read where they are used with readlane, like the addresses.  Every lane executes these
// loads before the first lane-dependent branch; the early exits are wave-uniform: past the last
// group, the plan's status, an invalid group, an empty one, a slab at or past L.
//
// No marks are read.  A shard is lost when its id is among the first t entries of the plan's lost
// list, and a data shard that is not lost is a survivor (plan_group lists all of them); the parity
// survivors are the last e entries of the survivor list.  Lengths are judged after the status: L
// outside [0, max_len] or a surviving data shard outside [0, L] makes the group invalid, counted by
// slab 0, lane 0 and untouched.  The length of a lost data shard is not looked at.
//
// The group cuts its own geometry, ptrs_var_geom(L, 16).  Alignment is judged on the entries the plan
// dereferences: the survivors with eff > 0 and the lost rows.  A wave all of whose survivors reach
// slab_reach<16> runs plan_column<true> unchanged (with all lengths equal: every wave); any other
// wave runs plan_column_var<true>.  The tail of an aligned group and every byte of a misaligned one
// run plan_column_var<false>.
//
// CLIP (k_plan_apply_ptrs_var_clip, the repair of qfec_scrub_ptrs_wide_var): culprit[g] in [0, k) names a
// listed data shard that has room for its own length only, the d_lens entry the locate judged.  Its
// stale load and its stores stop there (ClippedRoom), and a wave is `full` only where that shard
// reaches the wave's columns as well.  Any other value of culprit[g] clips nothing.
template <int NP, bool CLIP>
__device__ __forceinline__ void plan_apply_ptrs_var_wave(const PlanPtrsVarArgs& a, const uint64_t* __restrict__ dptrs,
                                                         const uint64_t* __restrict__ pptrs,
                                                         const int32_t* __restrict__ lens,
                                                         const int32_t* __restrict__ glen,
                                                         const uint8_t* __restrict__ plan,
                                                         const int32_t* __restrict__ culprit) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a.p, &g, &slab)) return;
    const int k = a.p.k, m = a.p.m, n = k + m;
    uint64_t p[NP];
    uint32_t eff[NP];  // as unsigned: a negative length is above every L
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int i = q * 64 + lane;
        p[q] = 0;
        eff[q] = 0;
        if (i < k) {
            p[q] = dptrs[g * (uint64_t)k + i];
            eff[q] = (uint32_t)lens[g * (uint64_t)k + i];
        } else if (i < n) {
            p[q] = pptrs[g * (uint64_t)m + (i - k)];
        }
    }
    const uint32_t L = (uint32_t)glen[g];
    const PlanLayout PL = plan_layout(k, m);
    const cptr32 pw = (cptr32)(plan + g * a.p.stride);
    const cptr32 t256 = (cptr32)a.p.t256;
    const int t = (int)(pw[0] & 0xFFFFu), e = (int)(pw[0] >> 16);
    const uint32_t status = pw[1] & 0xFFu;
    if (status > (uint32_t)QFEC_PLAN_WORK || t > m || e > t || e > k) return;  // failed, or not a plan: wave-uniform
    // which of its entries the plan writes (lost) and reads (used), per lane
    bool lost[NP], used[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) lost[q] = false;
    for (int j = 0; j < t; ++j) {
        const uint32_t l = plan_u8(pw, PL.lost_off + j);
#pragma unroll
        for (int q = 0; q < NP; ++q) lost[q] |= l == (uint32_t)(q * 64 + lane);
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int i = q * 64 + lane;
        used[q] = i < k && !lost[q];
        if (i >= k && i < n) eff[q] = L;
    }
    bool bad = false;
#pragma unroll
    for (int q = 0; q < NP; ++q) bad |= used[q] && eff[q] > L;
    if (L > a.p.block || __ballot(bad)) {  // invalid: untouched, counted once
        if (slab == 0 && lane == 0 && a.invalid) atomicAdd(a.invalid, 1u);
        return;
    }
    const PtrsVarGeom v = ptrs_var_geom(L, 16);
    if (status != (uint32_t)QFEC_PLAN_WORK || slab >= v.live) return;  // nothing to do, an empty group, a slab at or past L
    for (int r = 0; r < e; ++r) {
        const uint32_t s = plan_u8(pw, PL.surv_off + k - e + r);
#pragma unroll
        for (int q = 0; q < NP; ++q) used[q] |= s == (uint32_t)(q * 64 + lane);
    }
    const uint32_t reach = slab_reach<16>(v, slab);
    bool low = false, cut = false;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        low |= ((used[q] && eff[q] != 0) || lost[q]) && ((uint32_t)p[q] & 15u) != 0;
        cut |= used[q] && eff[q] < reach;
    }
    const bool aligned = __ballot(low) == 0;
    auto row = [&](uint32_t s) -> uint8_t* { return as_out(entry_of<NP>(p, s)); };
    auto len_of = [&](uint32_t s) -> uint32_t { return entry_of<NP>(eff, s); };
    if constexpr (CLIP) {
        const int32_t c = culprit[g];  // a scalar load
        uint32_t cul = ~0u, own = L;
        if (c >= 0 && c < k) {
            cul = (uint32_t)c;
            own = std::min(len_of(cul), L);
        }
        const bool full = __ballot(cut) == 0 && own >= reach;
        auto of = [&](uint32_t l) -> uint32_t { return l == cul ? own : L; };
        const ClippedRoom<decltype(of)> room{of};
        run_slab_var<16>(
            v, L, slab, lane, aligned,
            [&](uint32_t off) {
                if (full) plan_column<true>(pw, PL, t256, k, n, t, row, (uint64_t)off);
                else plan_column_var<true>(pw, PL, t256, k, n, t, row, len_of, off, room);
            },
            [&](uint32_t b) { plan_column_var<false>(pw, PL, t256, k, n, t, row, len_of, b, room); });
    } else {
        const bool full = __ballot(cut) == 0;
        run_slab_var<16>(
            v, L, slab, lane, aligned,
            [&](uint32_t off) {
                if (full) plan_column<true>(pw, PL, t256, k, n, t, row, (uint64_t)off);
                else plan_column_var<true>(pw, PL, t256, k, n, t, row, len_of, off);
            },
            [&](uint32_t b) { plan_column_var<false>(pw, PL, t256, k, n, t, row, len_of, b); });
    }
}

template <int NP>
__global__ void __launch_bounds__(256) k_plan_apply_ptrs_var(PlanPtrsVarArgs a, const uint64_t* __restrict__ dptrs,
                                                             const uint64_t* __restrict__ pptrs,
                                                             const int32_t* __restrict__ lens,
                                                             const int32_t* __restrict__ glen,
                                                             const uint8_t* __restrict__ plan) {
    plan_apply_ptrs_var_wave<NP, false>(a, dptrs, pptrs, lens, glen, plan, nullptr);
}

template <int NP>
__global__ void __launch_bounds__(256) k_plan_apply_ptrs_var_clip(PlanPtrsVarArgs a, const uint64_t* __restrict__ dptrs,
                                                                  const uint64_t* __restrict__ pptrs,
                                                                  const int32_t* __restrict__ lens,
                                                                  const int32_t* __restrict__ glen,
                                                                  const uint8_t* __restrict__ plan,
                                                                  const int32_t* __restrict__ culprit) {
    plan_apply_ptrs_var_wave<NP, true>(a, dptrs, pptrs, lens, glen, plan, culprit);
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

hipError_t launch_plan_apply_ptrs(const PlanPtrsArgs& a, hipStream_t stream) {
    if (a.groups == 0) return hipSuccess;
    const uint64_t waves = a.groups * (uint64_t)a.wpg;
    const int n = a.k + a.m;
    if (a.wpg == 0 || waves * 64u > (uint64_t)kMaxLaunchLanes || n > 256) return hipErrorInvalidValue;  // caller chunks
    const unsigned grid = (unsigned)((waves + 3) / 4);
    if (n <= 64) hipLaunchKernelGGL((k_plan_apply_ptrs<1>), dim3(grid), dim3(256), 0, stream, a, a.dptrs, a.pptrs, a.plan);
    else if (n <= 128) hipLaunchKernelGGL((k_plan_apply_ptrs<2>), dim3(grid), dim3(256), 0, stream, a, a.dptrs, a.pptrs, a.plan);
    else hipLaunchKernelGGL((k_plan_apply_ptrs<4>), dim3(grid), dim3(256), 0, stream, a, a.dptrs, a.pptrs, a.plan);
    return hipGetLastError();
}

hipError_t launch_plan_apply_ptrs_var(const PlanPtrsVarArgs& a, hipStream_t stream) {
    if (a.p.groups == 0) return hipSuccess;
    const uint64_t waves = a.p.groups * (uint64_t)a.p.wpg;
    const int n = a.p.k + a.p.m;
    if (a.p.wpg != ptrs_geom((int)a.p.block, 16).wpg || waves * 64u > (uint64_t)kMaxLaunchLanes || n > 256)
        return hipErrorInvalidValue;  // caller chunks
    const unsigned grid = (unsigned)((waves + 3) / 4);
    if (n <= 64)
        hipLaunchKernelGGL((k_plan_apply_ptrs_var<1>), dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs, a.lens,
                           a.group_len, a.p.plan);
    else if (n <= 128)
        hipLaunchKernelGGL((k_plan_apply_ptrs_var<2>), dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs, a.lens,
                           a.group_len, a.p.plan);
    else
        hipLaunchKernelGGL((k_plan_apply_ptrs_var<4>), dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs, a.lens,
                           a.group_len, a.p.plan);
    return hipGetLastError();
}

// culprit: [groups] of this launch, never NULL
hipError_t launch_plan_apply_ptrs_var_clip(const PlanPtrsVarArgs& a, const int32_t* culprit, hipStream_t stream) {
    if (a.p.groups == 0) return hipSuccess;
    const uint64_t waves = a.p.groups * (uint64_t)a.p.wpg;
    const int n = a.p.k + a.p.m;
    if (a.p.wpg != ptrs_geom((int)a.p.block, 16).wpg || waves * 64u > (uint64_t)kMaxLaunchLanes || n > 256 || !culprit)
        return hipErrorInvalidValue;  // caller chunks
    const unsigned grid = (unsigned)((waves + 3) / 4);
    if (n <= 64)
        hipLaunchKernelGGL((k_plan_apply_ptrs_var_clip<1>), dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs,
                           a.lens, a.group_len, a.p.plan, culprit);
    else if (n <= 128)
        hipLaunchKernelGGL((k_plan_apply_ptrs_var_clip<2>), dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs,
                           a.lens, a.group_len, a.p.plan, culprit);
    else
        hipLaunchKernelGGL((k_plan_apply_ptrs_var_clip<4>), dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs,
                           a.lens, a.group_len, a.p.plan, culprit);
    return hipGetLastError();
}

}  // namespace qfec
