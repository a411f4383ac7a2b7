// qfec_check.hip -- single-shard error location at any k + m, beside lost shards or not
// (qfec_check_build / qfec_check_apply of include/qfec.h, and qfec_locate_wide / qfec_scrub_wide on
// top of them).  The semantics are qfec_locate_erased's; where that call takes a group's constants
// from a host-built record per mask behind a 2^(k+m)-entry LUT, here the check plan of every group is
// computed on the device from the group's marks.
//
// k_check_build: k_plan_build's frame, one wave (a 64-thread block) per group: the marks in four
// ballot passes (or none marked), the GF tables staged in LDS, then check_group of qfec_plan.hpp, the
// text the host query qfec_check_build_host runs.
//
// k_check_apply: k_plan_apply's mapping, a wave per (group, 64 columns).  Status, S, ids and
// coefficients are wave-uniform and come through scalar loads of the plan.  The wave loops over the
// k survivors and accumulates the syndromes of up to CCH spares per pass; the first spare's syndrome
// is kept across passes.  A wave whose syndromes are all zero ends there.
//
// Cold path.  For the accepted codes (MDS) a non-zero syndrome byte has at most one explanation, so
// the wave derives ONE candidate from one byte and verifies it against every lane's bytes, instead of
// keeping a candidate bit per shard (qfec_locate_erased's 32-bit words do not reach k = 254).  Per
// pass: the first lane with a non-zero byte gives that byte's syndromes z_0 (first spare) and z_x
// (the pass's spares).  z_0 = 0 and exactly one z_y != 0: spare y.  z_0 != 0 and every z_x = 0: the
// first spare.  Otherwise the position c of K with ratio[c][x1] . z_0 = z_x1, x1 the pass's first
// spare after x0: the lanes test c = lane, lane + 64, .. and one ballot picks c.  Every lane then
// tests the wave-uniform candidate on its own bytes, and lane 0 folds the result into the group's
// three words: min and max of the candidate shard id, and flags (1 some byte non-zero, 2 some byte
// unexplained).  One candidate over every wave and pass and no unexplained byte is exactly "this
// shard's relation holds in every byte, and no other's does".  With one spare only the flag is set.
// k_check_finish turns the words and the plan's head into verdicts, marks and counts.
//
// k_check_apply_ptrs: the same arithmetic and cold path (check_columns) where the rows are given by a
// device table of shard addresses (qfec_check_apply_ptrs), in the mapping of k_plan_apply_ptrs; the
// words and the finish kernel are the same.
//
// k_check_apply_ptrs_var: the same where every data shard has its own length (qfec_check_apply_ptrs_var),
// with the lengths and the per-group geometry of k_plan_apply_ptrs_var; a wave whose data survivors all
// reach the end of its span runs check_columns unchanged, any other with clipped loads and the length
// condition (RaggedRows).  k_check_finish_var is the finish kernel that knows an invalid group.
#include <type_traits>

#include "../../include/qfec.h"
#include "qfec_device.hpp"
#include "qfec_plan.hpp"
#include "qfec_ptrs_device.hpp"

namespace qfec {

constexpr int CCH = 8;  // spares per pass of k_check_apply

__global__ void __launch_bounds__(64) k_check_build(PlanBuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];  // [exp 512 | log 256][check_work_bytes]
    const int lane = threadIdx.x;
    const uint64_t g = blockIdx.x;
    if (g >= a.groups) return;
    const int k = a.k, m = a.m, n = k + m;
    for (int i = lane; i < QFEC_PLAN_GF_BYTES / 4; i += 64)
        reinterpret_cast<uint32_t*>(lds)[i] = reinterpret_cast<const uint32_t*>(a.gf)[i];
    uint64_t mk[4] = {0, 0, 0, 0};
    if (a.dmarks) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int i = p * 64 + lane;
            uint32_t v = 0;
            if (i < k) v = a.dmarks[g * (uint64_t)k + i];
            else if (i < n) v = a.pmarks[g * (uint64_t)m + (i - k)];
            mk[p] = __ballot(v != 0);
        }
    }
    __syncthreads();
    const PlanCode C{reinterpret_cast<const uint8_t*>(a.tab + 7), QFEC_TAB_STRIDE * 4, k, m, 0, lds, lds + 512};
    (void)check_group(C, mk, lds + QFEC_PLAN_GF_BYTES, a.plan + g * a.stride, PlanWaveLanes{lane});
}

// byte idx of the plan through a scalar dword load
__device__ __forceinline__ uint32_t check_u8(cptr32 pw, int idx) { return (pw[idx >> 2] >> ((idx & 3) * 8)) & 0xFFu; }

template <int D>
__device__ __forceinline__ void check_ld(uint32_t (&v)[D], const uint8_t* p) {
    if constexpr (D == 4) ldv<4>(v, p);
    else v[0] = *p;
}

// byte b of lane src's v, wave-uniform
template <int D>
__device__ __forceinline__ uint32_t check_byte_at(const uint32_t (&v)[D], int b, int src) {
    uint32_t w = v[0];
    if constexpr (D == 4) {
        const int d = b >> 2;
        w = d == 0 ? v[0] : d == 1 ? v[1] : d == 2 ? v[2] : v[3];
    }
    return ((uint32_t)__builtin_amdgcn_readlane((int)w, src) >> ((b & 3) * 8)) & 0xFFu;
}

// D = 4: 16-byte columns; D = 1: one byte per lane, in the low byte of a dword
template <int D>
__global__ void __launch_bounds__(256) k_check_apply(CheckApplyArgs a, const uint8_t* __restrict__ check) {
    static_assert(D == 4 || D == 1, "16-B columns or bytes");
    const int lane = threadIdx.x & 63;
    const uint32_t wid = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t g = wid / a.wpg;
    const uint32_t part = wid - g * a.wpg;
    if (g >= a.groups) return;
    const int k = a.k, m = a.m, n = k + m;
    const CheckLayout CL = check_layout(k, m);
    const uint8_t* chk = check + (uint64_t)g * a.stride;
    const cptr32 pw = (cptr32)chk;
    const cptr32 t256 = (cptr32)a.t256;
    const int S = (int)(pw[0] & 0xFFFFu);
    if ((pw[1] & 0xFFu) != (uint32_t)QFEC_PLAN_WORK || S < 1 || S > m) return;
    // the lanes past the row's last column stay for the ballots: they read column 0 and count no byte
    const uint32_t col = part * 64u + lane;
    const bool live = col < a.cols;
    const uint64_t off = live ? (uint64_t)col * (D == 4 ? 16u : 1u) : 0u;
    uint32_t mk[D];
    if constexpr (D == 4) {
        const uint4 q = column_mask(a.block, live ? col : 0u);
        mk[0] = live ? q.x : 0u; mk[1] = live ? q.y : 0u; mk[2] = live ? q.z : 0u; mk[3] = live ? q.w : 0u;
    } else {
        mk[0] = live ? 0xFFu : 0u;
    }
    const uint8_t* data_g = a.data + (uint64_t)g * a.dgs;
    const uint8_t* par_g = a.parity + (uint64_t)g * a.pgs;
    auto row = [&](uint32_t s) -> const uint8_t* {
        return s < (uint32_t)k ? data_g + (uint64_t)s * a.pitch : par_g + (uint64_t)(s - k) * a.pitch;
    };

    uint32_t s0[D];  // the first spare's syndrome, from pass 0
#pragma unroll
    for (int d = 0; d < D; ++d) s0[d] = 0;
    for (int x0 = 0; x0 < S; x0 += CCH) {
        uint32_t acc[CCH][D];
#pragma unroll
        for (int j = 0; j < CCH; ++j)
#pragma unroll
            for (int d = 0; d < D; ++d) acc[j][d] = 0;
        for (int c = 0; c < k; ++c) {
            const uint32_t s = check_u8(pw, QFEC_CHECK_IDS + c);
            if (s >= (uint32_t)n) return;  // not a check plan of this code
            uint32_t v[D];
            check_ld<D>(v, row(s) + off);
            Sel sl[D];
#pragma unroll
            for (int d = 0; d < D; ++d) sl[d] = gf_sel(v[d]);
#pragma unroll
            for (int j = 0; j < CCH; ++j)
                if (x0 + j < S) {
                    const cptr32 tc = t256 + check_u8(pw, CL.a_off + (x0 + j) * k + c) * QFEC_TAB_STRIDE;
                    const uint32_t t0 = tc[0], t1 = tc[1], t2 = tc[2], t3 = tc[3], t4 = tc[4];
#pragma unroll
                    for (int d = 0; d < D; ++d)
                        acc[j][d] = xor3(acc[j][d], pp0(sl[d], t0, t1), pp1(sl[d], t2, t3)) ^ pp2(sl[d], t4);
                }
        }
        uint32_t nz[D];
#pragma unroll
        for (int d = 0; d < D; ++d) nz[d] = 0;
#pragma unroll
        for (int j = 0; j < CCH; ++j)
            if (x0 + j < S) {
                const uint32_t sp = check_u8(pw, QFEC_CHECK_IDS + k + x0 + j);
                if (sp >= (uint32_t)n) return;
                uint32_t p[D];
                check_ld<D>(p, row(sp) + off);
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    acc[j][d] = (acc[j][d] ^ p[d]) & mk[d];  // bytes >= block_size never count
                    nz[d] |= acc[j][d];
                }
            }
        if (x0 == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) s0[d] = acc[0][d];
        }
        uint32_t any = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            nz[d] |= s0[d];
            any |= nz[d];
        }
        const uint64_t hot = __ballot(any != 0);
        if (!hot) continue;  // consistent so far: the common case ends with the loop

        // ---- cold: one candidate from one byte, then every lane's bytes against it
        if (S == 1) {  // no ratio to test: the finish kernel calls the group AMBIGUOUS
            if (lane == 0) atomicOr(a.flags + g, 1u);
            continue;
        }
        const int src = __builtin_ctzll(hot);
        int bsel = 0;
#pragma unroll
        for (int d = D - 1; d >= 0; --d)
            if (nz[d]) bsel = d * 4 + (__builtin_ctz(nz[d]) >> 3);
        const int b = __builtin_amdgcn_readlane(bsel, src);
        const uint32_t z0 = check_byte_at<D>(s0, b, src);
        const int jlo = x0 == 0 ? 1 : 0;  // acc[0] of pass 0 is s0 itself
        int cnt = 0, first = -1;
        uint32_t z1 = 0;
#pragma unroll
        for (int j = 0; j < CCH; ++j)
            if (j >= jlo && x0 + j < S) {
                const uint32_t zj = check_byte_at<D>(acc[j], b, src);
                if (j == jlo) z1 = zj;
                if (zj) {
                    if (!cnt) first = j;
                    ++cnt;
                }
            }
        enum { NONE = 0, KPOS, SPARE, SPARE0 };
        int kind = NONE, cpos = 0;
        if (z0 == 0) {
            kind = cnt == 1 ? SPARE : NONE;
        } else if (cnt == 0) {
            kind = SPARE0;
        } else {
            // the position c of K with ratio[c][x1] . z0 = z1: each lane multiplies its ratio by the
            // wave-uniform z0 through z0's perm table
            const cptr32 tz = t256 + z0 * QFEC_TAB_STRIDE;
            const uint32_t t0 = tz[0], t1 = tz[1], t2 = tz[2], t3 = tz[3], t4 = tz[4];
            const int x1 = x0 + jlo;
            for (int c0 = 0; c0 < k; c0 += 64) {
                const int c = c0 + lane;
                bool hit = false;
                if (c < k) {
                    const uint32_t r = chk[CL.r_off + c * (S - 1) + (x1 - 1)];
                    hit = (gf_mul4(gf_sel(r), t0, t1, t2, t3, t4) & 0xFFu) == z1;
                }
                const uint64_t hits = __ballot(hit);
                if (hits) {
                    kind = KPOS;
                    cpos = c0 + __builtin_ctzll(hits);
                    break;
                }
            }
        }
        bool ok = kind != NONE;
        if (kind == SPARE)
#pragma unroll
            for (int d = 0; d < D; ++d) ok = ok && s0[d] == 0;
#pragma unroll
        for (int j = 0; j < CCH; ++j)
            if (j >= jlo && x0 + j < S) {
                if (kind == KPOS) {
                    const cptr32 tc = t256 + check_u8(pw, CL.r_off + cpos * (S - 1) + (x0 + j - 1)) * QFEC_TAB_STRIDE;
                    const uint32_t t0 = tc[0], t1 = tc[1], t2 = tc[2], t3 = tc[3], t4 = tc[4];
#pragma unroll
                    for (int d = 0; d < D; ++d) ok = ok && gf_mul4(gf_sel(s0[d]), t0, t1, t2, t3, t4) == acc[j][d];
                } else if (kind == SPARE0 || j != first) {
#pragma unroll
                    for (int d = 0; d < D; ++d) ok = ok && acc[j][d] == 0;
                }
            }
        const bool all_ok = kind != NONE && __ballot(!ok) == 0;
        if (lane == 0) {
            atomicOr(a.flags + g, all_ok ? 1u : 3u);
            if (all_ok) {
                const uint32_t id = kind == KPOS    ? check_u8(pw, QFEC_CHECK_IDS + cpos)
                                    : kind == SPARE ? check_u8(pw, QFEC_CHECK_IDS + k + x0 + first)
                                                    : check_u8(pw, QFEC_CHECK_IDS + k);
                atomicMin(a.cmin + g, id);
                atomicMax(a.cmax + g, id);
            }
        }
    }
}

// k_check_apply's body for k_check_apply_ptrs: 64 lanes of D dwords each (D = 4: the 16 bytes, D = 1: the
// byte at `off` of every shard) through the group's check plan `chk`, S spares.  row(s): where shard s
// starts, s wave-uniform.  A lane that is not `live` has no bytes at `off`: it issues no load and
// carries zero, which every candidate explains; a live lane's bytes all count, so nothing is masked.
// The call is wave-uniform (ballots and readlane inside) and folds what it finds into the group's
// three words.  False: not a check plan of this code, nothing more to do.
// (The two bodies stay apart: as one function this text moved k_check_apply<4>'s SGPR count.)
//
// Len (k_check_apply_ptrs_var's ragged waves; WholeRows: none of this): shard s may be read in
// [0, len.of(s)) only and counts as zero from there on, so a live lane's load is clipped to it (ldv_clip:
// the whole column, its first bytes in pieces, or nothing and then no load), and a data shard is known
// to be zero from its own end on: a candidate of K that is a data shard is rejected where a byte of the
// wave at or past its length has a non-zero first syndrome, byte-exact inside a 16-B lane.  (The
// candidate passed the ratio test, so where its first syndrome is zero every syndrome is.)
struct WholeRows {
    static constexpr bool ragged = false;
};
template <class F>
struct RaggedRows {
    static constexpr bool ragged = true;
    F of;
};

template <int D, class Row, class Len = WholeRows>
__device__ __forceinline__ bool check_columns(const uint8_t* chk, const CheckLayout& CL, cptr32 t256, int k, int n, int S,
                                              int lane, unsigned int* flags, unsigned int* cmin, unsigned int* cmax,
                                              const Row& row, uint64_t off, bool live, const Len& len = Len{}) {
    static_assert(D == 4 || D == 1, "16-B columns or bytes");
    const cptr32 pw = (cptr32)chk;
    auto ld = [&](uint32_t(&v)[D], uint32_t s) {
        const uint8_t* r = row(s);  // every lane takes part in the readlane
#pragma unroll
        for (int d = 0; d < D; ++d) v[d] = 0;
        if constexpr (Len::ragged) {
            const uint32_t end = len.of(s);  // a readlane as well
            if constexpr (D == 4) {
                if (live) ldv_clip<4>(v, r, (uint32_t)off, end);
            } else {
                if (live && (uint32_t)off < end) v[0] = r[off];
            }
        } else {
            if (live) check_ld<D>(v, r + off);
        }
    };
    uint32_t s0[D];  // the first spare's syndrome, from pass 0
#pragma unroll
    for (int d = 0; d < D; ++d) s0[d] = 0;
    for (int x0 = 0; x0 < S; x0 += CCH) {
        uint32_t acc[CCH][D];
#pragma unroll
        for (int j = 0; j < CCH; ++j)
#pragma unroll
            for (int d = 0; d < D; ++d) acc[j][d] = 0;
        for (int c = 0; c < k; ++c) {
            const uint32_t s = check_u8(pw, QFEC_CHECK_IDS + c);
            if (s >= (uint32_t)n) return false;  // not a check plan of this code
            uint32_t v[D];
            ld(v, s);
            Sel sl[D];
#pragma unroll
            for (int d = 0; d < D; ++d) sl[d] = gf_sel(v[d]);
#pragma unroll
            for (int j = 0; j < CCH; ++j)
                if (x0 + j < S) {
                    const cptr32 tc = t256 + check_u8(pw, CL.a_off + (x0 + j) * k + c) * QFEC_TAB_STRIDE;
                    const uint32_t t0 = tc[0], t1 = tc[1], t2 = tc[2], t3 = tc[3], t4 = tc[4];
#pragma unroll
                    for (int d = 0; d < D; ++d)
                        acc[j][d] = xor3(acc[j][d], pp0(sl[d], t0, t1), pp1(sl[d], t2, t3)) ^ pp2(sl[d], t4);
                }
        }
        uint32_t nz[D];
#pragma unroll
        for (int d = 0; d < D; ++d) nz[d] = 0;
#pragma unroll
        for (int j = 0; j < CCH; ++j)
            if (x0 + j < S) {
                const uint32_t sp = check_u8(pw, QFEC_CHECK_IDS + k + x0 + j);
                if (sp >= (uint32_t)n) return false;
                uint32_t p[D];
                ld(p, sp);
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    acc[j][d] ^= p[d];
                    nz[d] |= acc[j][d];
                }
            }
        if (x0 == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) s0[d] = acc[0][d];
        }
        uint32_t any = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            nz[d] |= s0[d];
            any |= nz[d];
        }
        const uint64_t hot = __ballot(any != 0);
        if (!hot) continue;  // consistent so far: the common case ends with the loop

        // ---- cold: one candidate from one byte, then every lane's bytes against it
        if (S == 1) {  // no ratio to test: the finish kernel calls the group AMBIGUOUS
            if (lane == 0) atomicOr(flags, 1u);
            continue;
        }
        const int src = __builtin_ctzll(hot);
        int bsel = 0;
#pragma unroll
        for (int d = D - 1; d >= 0; --d)
            if (nz[d]) bsel = d * 4 + (__builtin_ctz(nz[d]) >> 3);
        const int b = __builtin_amdgcn_readlane(bsel, src);
        const uint32_t z0 = check_byte_at<D>(s0, b, src);
        const int jlo = x0 == 0 ? 1 : 0;  // acc[0] of pass 0 is s0 itself
        int cnt = 0, first = -1;
        uint32_t z1 = 0;
#pragma unroll
        for (int j = 0; j < CCH; ++j)
            if (j >= jlo && x0 + j < S) {
                const uint32_t zj = check_byte_at<D>(acc[j], b, src);
                if (j == jlo) z1 = zj;
                if (zj) {
                    if (!cnt) first = j;
                    ++cnt;
                }
            }
        enum { NONE = 0, KPOS, SPARE, SPARE0 };
        int kind = NONE, cpos = 0;
        if (z0 == 0) {
            kind = cnt == 1 ? SPARE : NONE;
        } else if (cnt == 0) {
            kind = SPARE0;
        } else {
            // the position c of K with ratio[c][x1] . z0 = z1: each lane multiplies its ratio by the
            // wave-uniform z0 through z0's perm table
            const cptr32 tz = t256 + z0 * QFEC_TAB_STRIDE;
            const uint32_t t0 = tz[0], t1 = tz[1], t2 = tz[2], t3 = tz[3], t4 = tz[4];
            const int x1 = x0 + jlo;
            for (int c0 = 0; c0 < k; c0 += 64) {
                const int c = c0 + lane;
                bool hit = false;
                if (c < k) {
                    const uint32_t r = chk[CL.r_off + c * (S - 1) + (x1 - 1)];
                    hit = (gf_mul4(gf_sel(r), t0, t1, t2, t3, t4) & 0xFFu) == z1;
                }
                const uint64_t hits = __ballot(hit);
                if (hits) {
                    kind = KPOS;
                    cpos = c0 + __builtin_ctzll(hits);
                    break;
                }
            }
        }
        bool ok = kind != NONE;
        if (kind == SPARE)
#pragma unroll
            for (int d = 0; d < D; ++d) ok = ok && s0[d] == 0;
#pragma unroll
        for (int j = 0; j < CCH; ++j)
            if (j >= jlo && x0 + j < S) {
                if (kind == KPOS) {
                    const cptr32 tc = t256 + check_u8(pw, CL.r_off + cpos * (S - 1) + (x0 + j - 1)) * QFEC_TAB_STRIDE;
                    const uint32_t t0 = tc[0], t1 = tc[1], t2 = tc[2], t3 = tc[3], t4 = tc[4];
#pragma unroll
                    for (int d = 0; d < D; ++d) ok = ok && gf_mul4(gf_sel(s0[d]), t0, t1, t2, t3, t4) == acc[j][d];
                } else if (kind == SPARE0 || j != first) {
#pragma unroll
                    for (int d = 0; d < D; ++d) ok = ok && acc[j][d] == 0;
                }
            }
        if constexpr (Len::ragged) {
            if (kind == KPOS) {
                const uint32_t id = check_u8(pw, QFEC_CHECK_IDS + cpos);
                if (id < (uint32_t)k) {  // wave-uniform
                    const uint32_t end = len.of(id);
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        const uint32_t at = (uint32_t)off + 4u * d;  // the bytes at or past `end` of this dword
                        const uint32_t past = D == 1 ? (at >= end ? 0xFFu : 0u)
                                              : at >= end    ? 0xFFFFFFFFu
                                              : end - at >= 4u ? 0u
                                                               : 0xFFFFFFFFu << (8u * (end - at));
                        ok = ok && (s0[d] & past) == 0;
                    }
                }
            }
        }
        const bool all_ok = kind != NONE && __ballot(!ok) == 0;
        if (lane == 0) {
            atomicOr(flags, all_ok ? 1u : 3u);
            if (all_ok) {
                const uint32_t id = kind == KPOS    ? check_u8(pw, QFEC_CHECK_IDS + cpos)
                                    : kind == SPARE ? check_u8(pw, QFEC_CHECK_IDS + k + x0 + first)
                                                    : check_u8(pw, QFEC_CHECK_IDS + k);
                atomicMin(cmin, id);
                atomicMax(cmax, id);
            }
        }
    }
    return true;
}

// The same on a table of shard addresses (qfec_check_apply_ptrs): k_plan_apply_ptrs's mapping and
// address loads -- a wave per (group, slab of 64 16-B columns), NP passes of 64 lanes hold the group's
// k + m <= 64 * NP entries, the address of the wave-uniform shard id s is a v_readlane (entry_of) --
// and check_columns for the work.  Every lane loads its entries before anything depends on the lane,
// and every exit is wave-uniform: past the last group, the plan's status, an id that is not the code's.
//
// A shard is exactly `block` bytes with nothing readable after it, so where k_check_apply lets a lane
// without a column read column 0 and masks the row's last column, here a lane that is not `live` issues
// no load and carries zero, which every candidate explains; vector work covers whole columns only and
// needs no mask.  check_columns holds ballots, so it is called by the whole wave: once on 16-B lanes
// for the slab's whole columns of an aligned group, then over a byte span in steps of 64 on byte lanes:
// the block % 16 tail on the last slab of an aligned group, the slab's whole span of any other.
//
// Aligned is judged from the entries of the unmarked shards alone: bit `lane` of the plan's mark word q
// belongs to the entry that pass q put in this lane, and a marked entry, which may hold anything and
// is never dereferenced (the plan lists survivors and spares only), stays out of the ballot.
template <int NP>
__global__ void __launch_bounds__(256) k_check_apply_ptrs(CheckPtrsArgs a, const uint64_t* __restrict__ dptrs,
                                                          const uint64_t* __restrict__ pptrs,
                                                          const uint8_t* __restrict__ check) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a, &g, &slab)) return;
    const int k = a.k, m = a.m, n = k + m;
    const uint8_t* chk = check + g * a.stride;
    const cptr32 pw = (cptr32)chk;
    uint64_t p[NP];
    uint32_t low = 0;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int i = q * 64 + lane;
        p[q] = 0;
        if (i < k) p[q] = dptrs[g * (uint64_t)k + i];
        else if (i < n) p[q] = pptrs[g * (uint64_t)m + (i - k)];
        const uint64_t marked = pw[QFEC_CHECK_MARKS / 4 + 2 * q] | (uint64_t)pw[QFEC_CHECK_MARKS / 4 + 2 * q + 1] << 32;
        if (!((marked >> lane) & 1u)) low |= (uint32_t)p[q] & 15u;
    }
    const bool aligned = __ballot(low != 0) == 0;
    const CheckLayout CL = check_layout(k, m);
    const cptr32 t256 = (cptr32)a.t256;
    const int S = (int)(pw[0] & 0xFFFFu);
    if ((pw[1] & 0xFFu) != (uint32_t)QFEC_PLAN_WORK || S < 1 || S > m) return;  // wave-uniform
    auto columns = [&](auto width, uint64_t off, bool live) {
        return check_columns<decltype(width)::value>(
            chk, CL, t256, k, n, S, lane, a.flags + g, a.cmin + g, a.cmax + g,
            [&](uint32_t s) { return as_row(entry_of<NP>(p, s)); }, off, live);
    };
    uint32_t b0 = slab * 1024u, end = std::min((slab + 1) * 1024u, a.block);  // the slab's byte span
    if (aligned) {
        const uint32_t col = slab * 64u + lane;
        if (slab * 64u < a.vcols && !columns(std::integral_constant<int, 4>{}, (uint64_t)col * 16u, col < a.vcols)) return;
        b0 = slab + 1 == a.wpg ? a.tail0 : end;  // tail0 + tailn = block = end on the last slab
    }
#pragma unroll 1
    for (; b0 < end; b0 += 64)
        if (!columns(std::integral_constant<int, 1>{}, (uint64_t)b0 + lane, b0 + lane < end)) return;
}

// k_check_apply_ptrs where every data shard has its own length (qfec_check_apply_ptrs_var): data shard i
// of a group is len_i bytes and counts as zero-filled up to the group's length L = glen[g], the length
// of its parity shards.  Mapping and address loads are k_check_apply_ptrs's; the launch has
// ptrs_geom(max_len, 16).wpg waves per group.  New here:
//
// Lengths.  A lane loads its entry's length in the same round trip as the address; with L, a scalar
// load, that makes NP registers of readable length (len_i of a data shard, L of a parity shard), read
// where they are used with readlane, like the addresses.  Every lane executes these loads before the
// first lane-dependent branch; every exit is wave-uniform: past the last group, a failed plan or none
// of this code, invalid lengths, a plan without work, an empty group, a slab at or past L, an id that
// is not the code's.
//
// Judgement.  After the plan's status (failed: nothing is judged) and for status 0 and 1 alike: L
// outside [0, max_len] or an unmarked data shard outside [0, L] makes the group invalid.  Marked is
// the plan's mark bit; the length of a marked shard is not looked at.  Every wave judges (a ballot),
// slab 0 alone reports: bit 2 of the group's flags, which k_check_finish_var turns into the verdict.
//
// Alignment is judged on the entries the wave may dereference: the unmarked shards of non-zero length
// (L > 0 here, so every unmarked parity shard).  The group cuts its own geometry, ptrs_var_geom(L, 16).
// Every unmarked data shard belongs to K (the k lowest unmarked ids), so a wave all of whose unmarked
// data shards reach the end of its span is `full` and runs k_check_apply_ptrs's body unchanged with
// block = L (all lengths equal: every wave); any other wave runs the same calls with RaggedRows.
template <int NP>
__global__ void __launch_bounds__(256) k_check_apply_ptrs_var(CheckPtrsVarArgs a, const uint64_t* __restrict__ dptrs,
                                                              const uint64_t* __restrict__ pptrs,
                                                              const int32_t* __restrict__ lens,
                                                              const int32_t* __restrict__ glen,
                                                              const uint8_t* __restrict__ check) {
    const int lane = threadIdx.x & 63;
    uint64_t g;
    uint32_t slab;
    if (!wave_item(a.p, &g, &slab)) return;
    const int k = a.p.k, m = a.p.m, n = k + m;
    const uint8_t* chk = check + g * a.p.stride;
    const cptr32 pw = (cptr32)chk;
    uint64_t p[NP];
    uint32_t eff[NP];  // as unsigned: a negative length is above every L
    bool un[NP];       // an unmarked shard of the code
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
        const uint64_t marked = pw[QFEC_CHECK_MARKS / 4 + 2 * q] | (uint64_t)pw[QFEC_CHECK_MARKS / 4 + 2 * q + 1] << 32;
        un[q] = i < n && !((marked >> lane) & 1u);
    }
    const uint32_t L = (uint32_t)glen[g];
    const CheckLayout CL = check_layout(k, m);
    const cptr32 t256 = (cptr32)a.p.t256;
    const int S = (int)(pw[0] & 0xFFFFu);
    const uint32_t status = pw[1] & 0xFFu;
    if (status > (uint32_t)QFEC_PLAN_WORK || (status == (uint32_t)QFEC_PLAN_WORK && (S < 1 || S > m))) return;  // wave-uniform
    bool bad = false;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int i = q * 64 + lane;
        bad |= un[q] && i < k && eff[q] > L;
        if (i >= k && i < n) eff[q] = L;
    }
    if (L > a.p.block || __ballot(bad)) {  // invalid: nothing dereferenced, reported once
        if (slab == 0 && lane == 0) atomicOr(a.p.flags + g, 4u);
        return;
    }
    const PtrsVarGeom v = ptrs_var_geom(L, 16);
    if (status != (uint32_t)QFEC_PLAN_WORK || slab >= v.live) return;  // unchecked, an empty group, a slab at or past L
    const uint32_t end = std::min((slab + 1) * 1024u, L);  // the slab's byte span ends here
    bool low = false, cut = false;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        low |= un[q] && eff[q] != 0 && ((uint32_t)p[q] & 15u) != 0;
        cut |= un[q] && eff[q] < end;  // a parity shard's is L
    }
    const bool aligned = __ballot(low) == 0;
    const bool full = __ballot(cut) == 0;
    auto row = [&](uint32_t s) { return as_row(entry_of<NP>(p, s)); };
    auto span = [&](const auto& rows) {
        auto columns = [&](auto width, uint64_t off, bool live) {
            return check_columns<decltype(width)::value>(chk, CL, t256, k, n, S, lane, a.p.flags + g, a.p.cmin + g,
                                                         a.p.cmax + g, row, off, live, rows);
        };
        uint32_t b0 = slab * 1024u;
        if (aligned) {
            const uint32_t col = slab * 64u + lane;
            if (slab * 64u < v.vcols && !columns(std::integral_constant<int, 4>{}, (uint64_t)col * 16u, col < v.vcols)) return;
            b0 = slab + 1 == v.live ? v.tail0 : end;  // tail0 + tailn = L = end on the last live slab
        }
#pragma unroll 1
        for (; b0 < end; b0 += 64)
            if (!columns(std::integral_constant<int, 1>{}, (uint64_t)b0 + lane, b0 + lane < end)) return;
    };
    if (full) {
        span(WholeRows{});
    } else {
        auto of = [&](uint32_t s) -> uint32_t { return entry_of<NP>(eff, s); };
        span(RaggedRows<decltype(of)>{of});
    }
}

// one lane per group
__global__ void __launch_bounds__(256) k_check_finish(CheckFinishArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    int verdict = -1;  // also for lanes past the last group
    if (g < a.groups) {
        const uint32_t* pw = reinterpret_cast<const uint32_t*>(a.check + g * a.stride);
        const int S = (int)(pw[0] & 0xFFFFu);
        const uint32_t status = pw[1] & 0xFFu;
        uint64_t mk[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) mk[w] = pw[4 + 2 * w] | (uint64_t)pw[5 + 2 * w] << 32;
        int id = QFEC_LOC_CLEAN;
        if (status == (uint32_t)QFEC_PLAN_FAILED) {
            id = QFEC_LOC_LOST;
        } else if (status == (uint32_t)QFEC_PLAN_NONE) {
            id = QFEC_LOC_UNCHECKED;
        } else if (a.flags[g] != 0) {
            if (S == 1) id = QFEC_LOC_AMBIGUOUS;
            else if ((a.flags[g] & 2u) || a.cmin[g] != a.cmax[g]) id = QFEC_LOC_MULTI;
            else id = (int)a.cmin[g];
        }
        if (a.culprit) a.culprit[g] = id;
        if (a.marks_out) {
            // the input marks as 0 / 1, plus the culprit; for the scrub nothing in a group that must
            // stay as it is.  This lane alone touches the group's bytes, and the input marks are in the plan
            const bool none = a.scrub && (id == QFEC_LOC_MULTI || id == QFEC_LOC_AMBIGUOUS);
            const int k = a.k, m = a.m;
            uint8_t* dm = a.marks_out + (a.g0 + g) * (uint64_t)k;
            uint8_t* pm = a.marks_out + a.all_groups * (uint64_t)k + (a.g0 + g) * (uint64_t)m;
            for (int i = 0; i < k; ++i) dm[i] = none ? 0 : (uint8_t)(plan_bit(mk, i) | (i == id));
            for (int j = 0; j < m; ++j) pm[j] = none ? 0 : (uint8_t)(plan_bit(mk, k + j) | (k + j == id));
        }
        verdict = id >= 0 ? 0 : id == QFEC_LOC_CLEAN ? -1 : -id - 1;  // MULTI -2 -> 1 ... LOST -5 -> 4
    }
    if (a.counts) block_counts<5>(verdict, a.counts);  // uniform over the grid
}

// k_check_finish for k_check_apply_ptrs_var, whose flags know bit 2: the group's lengths are out of range.
// Judged after a failed plan and before everything else; QFEC_LOC_INVALID counts in no entry of counts
// and once in *invalid, its marks are the input marks (scrub: none).  (A kernel of its own: as one
// body with a switch this text moved k_check_finish's SGPR count.)
__global__ void __launch_bounds__(256) k_check_finish_var(CheckFinishArgs a, unsigned int* invalid) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    int verdict = -1, bad = -1;  // also for lanes past the last group
    if (g < a.groups) {
        const uint32_t* pw = reinterpret_cast<const uint32_t*>(a.check + g * a.stride);
        const int S = (int)(pw[0] & 0xFFFFu);
        const uint32_t status = pw[1] & 0xFFu;
        uint64_t mk[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) mk[w] = pw[4 + 2 * w] | (uint64_t)pw[5 + 2 * w] << 32;
        const uint32_t flags = a.flags[g];
        int id = QFEC_LOC_CLEAN;
        if (status == (uint32_t)QFEC_PLAN_FAILED) {
            id = QFEC_LOC_LOST;
        } else if (flags & 4u) {
            id = QFEC_LOC_INVALID;
        } else if (status == (uint32_t)QFEC_PLAN_NONE) {
            id = QFEC_LOC_UNCHECKED;
        } else if (flags != 0) {
            if (S == 1) id = QFEC_LOC_AMBIGUOUS;
            else if ((flags & 2u) || a.cmin[g] != a.cmax[g]) id = QFEC_LOC_MULTI;
            else id = (int)a.cmin[g];
        }
        if (a.culprit) a.culprit[g] = id;
        if (a.marks_out) {
            const bool none = a.scrub && (id == QFEC_LOC_MULTI || id == QFEC_LOC_AMBIGUOUS || id == QFEC_LOC_INVALID);
            const int k = a.k, m = a.m;
            uint8_t* dm = a.marks_out + (a.g0 + g) * (uint64_t)k;
            uint8_t* pm = a.marks_out + a.all_groups * (uint64_t)k + (a.g0 + g) * (uint64_t)m;
            for (int i = 0; i < k; ++i) dm[i] = none ? 0 : (uint8_t)(plan_bit(mk, i) | (i == id));
            for (int j = 0; j < m; ++j) pm[j] = none ? 0 : (uint8_t)(plan_bit(mk, k + j) | (k + j == id));
        }
        bad = id == QFEC_LOC_INVALID ? 0 : -1;
        verdict = id >= 0 ? 0 : id == QFEC_LOC_CLEAN || id == QFEC_LOC_INVALID ? -1 : -id - 1;
    }
    if (a.counts) block_counts<5>(verdict, a.counts);  // uniform over the grid
    if (invalid) block_counts<1>(bad, invalid);
}

hipError_t launch_check_build(const PlanBuildArgs& a, hipStream_t stream) {
    if (a.groups == 0) return hipSuccess;
    if (a.groups > 0x7FFFFFFFull / 64u || a.lds > 65536u) return hipErrorInvalidValue;  // caller chunks
    hipLaunchKernelGGL(k_check_build, dim3((unsigned)a.groups), dim3(64), a.lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_check_apply(const CheckApplyArgs& a, hipStream_t stream) {
    if (a.groups == 0 || a.cols == 0) return hipSuccess;
    const uint64_t waves = a.groups * (uint64_t)a.wpg;
    if (a.wpg == 0 || waves * 64u > 0x7FFFFFFFull || !a.flags || !a.cmin || !a.cmax) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((waves + 3) / 4);
    if (a.vec16) hipLaunchKernelGGL((k_check_apply<4>), dim3(grid), dim3(256), 0, stream, a, a.check);
    else hipLaunchKernelGGL((k_check_apply<1>), dim3(grid), dim3(256), 0, stream, a, a.check);
    return hipGetLastError();
}

hipError_t launch_check_apply_ptrs(const CheckPtrsArgs& a, hipStream_t stream) {
    if (a.groups == 0) return hipSuccess;
    const uint64_t waves = a.groups * (uint64_t)a.wpg;
    const int n = a.k + a.m;
    if (a.wpg == 0 || waves * 64u > 0x7FFFFFFFull || n > 256 || !a.flags || !a.cmin || !a.cmax) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((waves + 3) / 4);
    if (n <= 64) hipLaunchKernelGGL((k_check_apply_ptrs<1>), dim3(grid), dim3(256), 0, stream, a, a.dptrs, a.pptrs, a.check);
    else if (n <= 128) hipLaunchKernelGGL((k_check_apply_ptrs<2>), dim3(grid), dim3(256), 0, stream, a, a.dptrs, a.pptrs, a.check);
    else hipLaunchKernelGGL((k_check_apply_ptrs<4>), dim3(grid), dim3(256), 0, stream, a, a.dptrs, a.pptrs, a.check);
    return hipGetLastError();
}

hipError_t launch_check_apply_ptrs_var(const CheckPtrsVarArgs& a, hipStream_t stream) {
    if (a.p.groups == 0) return hipSuccess;
    const uint64_t waves = a.p.groups * (uint64_t)a.p.wpg;
    const int n = a.p.k + a.p.m;
    if (a.p.wpg != ptrs_geom((int)a.p.block, 16).wpg || waves * 64u > 0x7FFFFFFFull || n > 256 || !a.p.flags || !a.p.cmin ||
        !a.p.cmax || !a.lens || !a.group_len)
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((waves + 3) / 4);
    if (n <= 64)
        hipLaunchKernelGGL((k_check_apply_ptrs_var<1>), dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs, a.lens,
                           a.group_len, a.p.check);
    else if (n <= 128)
        hipLaunchKernelGGL((k_check_apply_ptrs_var<2>), dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs, a.lens,
                           a.group_len, a.p.check);
    else
        hipLaunchKernelGGL((k_check_apply_ptrs_var<4>), dim3(grid), dim3(256), 0, stream, a, a.p.dptrs, a.p.pptrs, a.lens,
                           a.group_len, a.p.check);
    return hipGetLastError();
}

hipError_t launch_check_finish_var(const CheckFinishArgs& a, unsigned int* invalid, hipStream_t stream) {
    if (a.groups == 0) return hipSuccess;
    if (!a.check || !a.flags || !a.cmin || !a.cmax || a.groups > 0x7FFFFFFFull * 256u) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((a.groups + 255) / 256);
    hipLaunchKernelGGL(k_check_finish_var, dim3(grid), dim3(256), 0, stream, a, invalid);
    return hipGetLastError();
}

hipError_t launch_check_finish(const CheckFinishArgs& a, hipStream_t stream) {
    if (a.groups == 0) return hipSuccess;
    if (!a.check || !a.flags || !a.cmin || !a.cmax || a.groups > 0x7FFFFFFFull * 256u) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((a.groups + 255) / 256);
    hipLaunchKernelGGL(k_check_finish, dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace qfec
