// qfec_plan.hpp -- the decode plan of one group, computed from its marks alone: the layout
// (include/qfec.h, qfec_plan_build) and the arithmetic, written once for the host
// (qfec_plan_build_host, one thread) and the device (k_plan_build, one wave per group).
//
// No k x k inversion: the surviving data rows of the survivor matrix are identity rows.  With E the
// e erased data ids, Q the e parity rows the survivor rule picks (the first e unmarked ones,
// module/rs.c:620-629) and M = P[Q][E] (e x e):
//   decode row of erased shard E_j:  sum_r Minv[j][r] * P[Q_r][i] at the column of surviving data i,
//                                    Minv[j][r] at the column of parity Q_r
//   marked parity row p (repair):    with R[r] = sum_jj P[p][E_jj] * Minv[jj][r]:
//                                    P[p][i] + sum_r R[r] * P[Q_r][i] at surviving data i, R[r] at Q_r
// which is gf256.cpp's decode_rows / repair_rows restated (the inverse of an invertible matrix is
// unique, so the rows are the same bytes).  X (t x e) below holds Minv's rows, then the R rows.
#pragma once

#include <stdint.h>

#include "qfec_internal.hpp"

namespace qfec {

#define QFEC_HD __host__ __device__ __forceinline__

constexpr int QFEC_PLAN_HDR = 16;  // [u16 t][u16 e][u8 status][pad]
constexpr int QFEC_PLAN_NONE = 0, QFEC_PLAN_WORK = 1, QFEC_PLAN_FAILED = 2;
constexpr int QFEC_PLAN_GF_BYTES = 768;  // exp[512] | log[256], as DevCtx::d_gf

struct PlanLayout {
    int surv_off, lost_off, stale_off;  // k survivor ids, m lost ids, m stale flags (u8 each)
    int coef_off;                       // m x k coefficient bytes, from a 16-byte boundary
    int stride;                         // bytes per group, a multiple of 16
};

QFEC_HD PlanLayout plan_layout(int k, int m) {
    PlanLayout L;
    L.surv_off = QFEC_PLAN_HDR;
    L.lost_off = L.surv_off + k;
    L.stale_off = L.lost_off + m;
    L.coef_off = (L.stale_off + m + 15) & ~15;
    L.stride = (L.coef_off + m * k + 15) & ~15;
    return L;
}

// working memory of plan_group: the plan's first coef_off bytes, a column of e_max bytes, [M | I]
// (e_max x 2 e_max) and X (m x e_max), e_max = min(k, m)
QFEC_HD int plan_work_bytes(int k, int m) {
    const int em = k < m ? k : m;
    return plan_layout(k, m).coef_off + em + 2 * em * em + m * em;
}

// what plan_group reads of a code: P[j][i] = P[(j * k + i) * pstride]
struct PlanCode {
    const uint8_t* P;
    int pstride;
    int k, m;
    int quirk;
    const uint8_t* gexp;  // [512] (Field::exp)
    const uint8_t* glog;  // [256], log[0] = 255 (Field::log)
};

// the marks of one group as a bit per shard id, ids 0..255 in four words (selects, not an indexed
// load: on the device the words are scalar registers and i differs per lane)
QFEC_HD int plan_bit(const uint64_t (&mk)[4], int i) {
    const int w = i >> 6;
    const uint64_t v = w == 0 ? mk[0] : w == 1 ? mk[1] : w == 2 ? mk[2] : mk[3];
    return (int)((v >> (i & 63)) & 1u);
}
// marked ids below i, 0 <= i <= 256
QFEC_HD int plan_below(const uint64_t (&mk)[4], int i) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int lo = w * 64;
        if (i >= lo + 64) c += __builtin_popcountll(mk[w]);
        else if (i > lo) c += __builtin_popcountll(mk[w] & ((1ull << (i - lo)) - 1ull));
    }
    return c;
}

// b * (the value whose log is la); la < 255
QFEC_HD uint8_t plan_mul_log(const PlanCode& C, int la, uint8_t b) { return b ? C.gexp[la + C.glog[b]] : 0; }
QFEC_HD uint8_t plan_mul(const PlanCode& C, uint8_t a, uint8_t b) { return a ? plan_mul_log(C, C.glog[a], b) : 0; }

// The single thread of the host: lane 0 of 1, nothing to wait for.  The device's counterpart
// (qfec_plan.hip) is a wave: 64 lanes, a barrier, a broadcast.
struct PlanHostLanes {
    static constexpr int n = 1;
    int lane = 0;
    QFEC_HD void sync() const {}
    QFEC_HD int uni(int x) const { return x; }
    QFEC_HD void store16(uint8_t* dst, const uint32_t (&w)[4]) const { __builtin_memcpy(dst, w, 16); }
};

// coefficient (j, c) of the plan: row j (j < e: erased data shard; else a marked parity row) at
// survivor column c.  hdr = the plan's head (ids), X = t x e
QFEC_HD uint8_t plan_coef(const PlanCode& C, const PlanLayout& PL, const uint8_t* hdr, const uint8_t* X, int e, int j,
                          int c) {
    const int k = C.k;
    const int s = hdr[PL.surv_off + c];
    if (s >= k) return X[j * e + (c - (k - e))];  // the last e survivors are Q, in order
    uint8_t acc = j >= e ? C.P[(size_t)((hdr[PL.lost_off + j] - k) * k + s) * C.pstride] : 0;
    for (int r = 0; r < e; ++r) {
        const int q = hdr[PL.surv_off + k - e + r] - k;
        acc ^= plan_mul(C, X[j * e + r], C.P[(size_t)(q * k + s) * C.pstride]);
    }
    return acc;
}

// Minv of M = P[Q][E] (e x e) into the right half of A (e x 2e): Gauss-Jordan on [M | I], from the
// ids in hdr (the last e survivors are Q, the first e lost ids E).  colv: e bytes.  False for a
// singular M.  Every lane of L calls it.
template <class Lanes>
QFEC_HD bool plan_invert(const PlanCode& C, const PlanLayout& PL, const uint8_t* hdr, int e, uint8_t* colv, uint8_t* A,
                         const Lanes& L) {
    const int k = C.k;
    const int w = 2 * e;
    for (int idx = L.lane; idx < e * w; idx += L.n) {
        const int r = idx / w, c = idx - r * w;
        const int q = hdr[PL.surv_off + k - e + r] - k;
        A[idx] = c < e ? C.P[(size_t)(q * k + hdr[PL.lost_off + c]) * C.pstride] : (uint8_t)(c - e == r);
    }
    L.sync();
    // lanes across the 2e columns; any pivot order gives the same inverse
    for (int c = 0; c < e; ++c) {
        int p = c;
        while (p < e && A[p * w + c] == 0) ++p;
        p = L.uni(p);
        if (p == e) return false;
        const int ls = (255 - C.glog[A[p * w + c]]) % 255;  // log of the pivot's inverse
        L.sync();
        for (int j = L.lane; j < w; j += L.n) {
            const uint8_t a = A[p * w + j], b = A[c * w + j];
            A[c * w + j] = plan_mul_log(C, ls, a);
            if (p != c) A[p * w + j] = b;
        }
        L.sync();
        for (int r = L.lane; r < e; r += L.n) colv[r] = A[r * w + c];
        L.sync();
        for (int r = 0; r < e; ++r) {
            const uint8_t q = colv[r];
            if (r == c || !q) continue;
            const int lq = C.glog[q];
            for (int j = L.lane; j < w; j += L.n) A[r * w + j] ^= plan_mul_log(C, lq, A[c * w + j]);
        }
        L.sync();
    }
    return true;
}

// rows [j0, j1) of X (e bytes each) from the inverse plan_invert left in A: Minv's row for j < e, the
// R row of the parity shard hdr lists as lost id j above that.  The caller syncs before X is read.
template <class Lanes>
QFEC_HD void plan_factors(const PlanCode& C, const PlanLayout& PL, const uint8_t* hdr, const uint8_t* A, uint8_t* X,
                          int e, int j0, int j1, const Lanes& L) {
    const int k = C.k;
    const int w = 2 * e;
    for (int idx = j0 * e + L.lane; idx < j1 * e; idx += L.n) {
        const int j = idx / e, r = idx - j * e;
        uint8_t x;
        if (j < e) {
            x = A[j * w + e + r];
        } else {
            const int pj = hdr[PL.lost_off + j] - k;
            x = 0;
            for (int jj = 0; jj < e; ++jj)
                x ^= plan_mul(C, C.P[(size_t)(pj * k + hdr[PL.lost_off + jj]) * C.pstride], A[jj * w + e + r]);
        }
        X[idx] = x;
    }
}

// The plan of one group into out[stride] (whole 16-byte stores, unused bytes zero).  Every lane of
// L calls it with the same arguments; W = plan_work_bytes(k, m) bytes shared by the lanes.
// mode 0: the erased data rows (qfec_reconstruct's rule), 1: every marked shard (qfec_repair's).
// Returns the status.  A group with nothing to do or a failed one carries t, e and the status only.
template <class Lanes>
QFEC_HD int plan_group(const PlanCode& C, const uint64_t (&mk)[4], int mode, uint8_t* W, uint8_t* out, const Lanes& L) {
    const int k = C.k, m = C.m, n = k + m;
    const PlanLayout PL = plan_layout(k, m);
    const int em = k < m ? k : m;
    uint8_t* hdr = W;
    uint8_t* colv = W + PL.coef_off;
    uint8_t* A = colv + em;
    uint8_t* X = A + 2 * em * em;

    const int e = plan_below(mk, k);
    const int np = plan_below(mk, n) - e;
    const int t = mode ? e + np : e;
    int status = t == 0 ? QFEC_PLAN_NONE : (mode ? t > m : e > m - np) ? QFEC_PLAN_FAILED : QFEC_PLAN_WORK;

    for (int i = L.lane; i < PL.coef_off; i += L.n) hdr[i] = 0;
    L.sync();
    if (status == QFEC_PLAN_WORK) {
        // survivors: the k lowest unmarked ids; lost: the marked ids ascending (mode 0: data only)
        for (int i = L.lane; i < n; i += L.n) {
            const int below = plan_below(mk, i);
            if (!plan_bit(mk, i)) {
                if (i - below < k) hdr[PL.surv_off + i - below] = (uint8_t)i;
            } else if (i < k || mode) {
                hdr[PL.lost_off + below] = (uint8_t)i;
            }
        }
        L.sync();
        if (!plan_invert(C, PL, hdr, e, colv, A, L)) status = QFEC_PLAN_FAILED;  // singular: explicit rows that are not MDS
        if (status == QFEC_PLAN_WORK) {
            plan_factors(C, PL, hdr, A, X, e, 0, t, L);
            L.sync();
            // module/rs.c:116-117: a zero column-0 coefficient leaves the output's bytes in place (data rows only)
            if (C.quirk)
                for (int j = L.lane; j < e; j += L.n) hdr[PL.stale_off + j] = plan_coef(C, PL, hdr, X, e, j, 0) == 0;
        } else {
            for (int i = QFEC_PLAN_HDR + L.lane; i < PL.coef_off; i += L.n) hdr[i] = 0;
        }
        L.sync();
    }
    if (L.lane == 0) {
        hdr[0] = (uint8_t)t;
        hdr[1] = (uint8_t)(t >> 8);
        hdr[2] = (uint8_t)e;
        hdr[3] = (uint8_t)(e >> 8);
        hdr[4] = (uint8_t)status;
    }
    L.sync();
    const int ncoef = status == QFEC_PLAN_WORK ? t * k : 0;
    for (int pos = L.lane * 16; pos < PL.stride; pos += L.n * 16) {
        uint32_t wd[4] = {0, 0, 0, 0};
        if (pos < PL.coef_off) {
#pragma unroll
            for (int q = 0; q < 16; ++q) wd[q >> 2] |= (uint32_t)hdr[pos + q] << (8 * (q & 3));
        } else if (pos - PL.coef_off < ncoef) {
            const int i0 = pos - PL.coef_off;
            int j = i0 / k, c = i0 - j * k;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if (i0 + q < ncoef) wd[q >> 2] |= (uint32_t)plan_coef(C, PL, hdr, X, e, j, c) << (8 * (q & 3));
                if (++c == k) { c = 0; ++j; }
            }
        }
        L.store16(out + pos, wd);
    }
    return status;
}

// ---------------------------------------------------------------- check plans (qfec_check_build)
// What single-shard error location needs of one group (include/qfec.h, qfec_check_build): K, the
// spares R, the rows A_x that predict each spare from K, and the ratios A_x[i] / A_x0[i].  A_x is the
// row the repair plan above gives for x under the mask E + R (every shard outside K), so the
// elimination and the row factors are plan_invert / plan_factors over the same ids: Q, the parity
// rows inside K, and E's data ids are the same under either mask.
constexpr int QFEC_CHECK_MARKS = 16;  // after the header [u16 S][u16 t][u8 status][pad]: 32 bytes of mark bits
constexpr int QFEC_CHECK_IDS = 48;

struct CheckLayout {
    int a_off, r_off;  // m x k rows, k x (m - 1) ratios, each from a 16-byte boundary
    int stride;        // bytes per group, a multiple of 16
};

QFEC_HD CheckLayout check_layout(int k, int m) {
    CheckLayout L;
    L.a_off = (QFEC_CHECK_IDS + k + m + 15) & ~15;
    L.r_off = (L.a_off + m * k + 15) & ~15;
    L.stride = (L.r_off + k * (m > 1 ? m - 1 : 0) + 15) & ~15;
    return L;
}

// working memory of check_group: plan_group's, and the first spare's row (k bytes)
QFEC_HD int check_work_bytes(int k, int m) { return plan_work_bytes(k, m) + k; }

// The check plan of one group into out[stride] (whole 16-byte stores, unused bytes zero), called as
// plan_group is; W = check_work_bytes(k, m).  Returns the status: 0 t = m, 1 work, 2 t > m or a
// singular matrix over K.
template <class Lanes>
QFEC_HD int check_group(const PlanCode& C, const uint64_t (&mk)[4], uint8_t* W, uint8_t* out, const Lanes& L) {
    const int k = C.k, m = C.m, n = k + m;
    const PlanLayout PL = plan_layout(k, m);
    const CheckLayout CL = check_layout(k, m);
    const int em = k < m ? k : m;
    uint8_t* hdr = W;  // ids as plan_group keeps them: K, then as "lost" E's data ids and the spares
    uint8_t* row0 = W + PL.coef_off;
    uint8_t* colv = row0 + k;
    uint8_t* A = colv + em;
    uint8_t* X = A + 2 * em * em;

    const int e = plan_below(mk, k);
    const int t = plan_below(mk, n);
    const int S = t < m ? m - t : 0;
    int status = t > m ? QFEC_PLAN_FAILED : t == m ? QFEC_PLAN_NONE : QFEC_PLAN_WORK;
    if (status == QFEC_PLAN_WORK) {
        for (int i = L.lane; i < n; i += L.n) {
            const int below = plan_below(mk, i);
            if (plan_bit(mk, i)) {
                if (i < k) hdr[PL.lost_off + below] = (uint8_t)i;
            } else if (i - below < k) {
                hdr[PL.surv_off + i - below] = (uint8_t)i;
            } else {
                hdr[PL.lost_off + e + (i - below - k)] = (uint8_t)i;  // a spare: a parity row outside K
            }
        }
        L.sync();
        if (!plan_invert(C, PL, hdr, e, colv, A, L)) {
            status = QFEC_PLAN_FAILED;
        } else {
            plan_factors(C, PL, hdr, A, X, e, e, e + S, L);
            L.sync();
            for (int i = L.lane; i < k; i += L.n) row0[i] = plan_coef(C, PL, hdr, X, e, e, i);
        }
        L.sync();
    }
    const int nids = status == QFEC_PLAN_WORK ? k + S : 0;
    const int na = status == QFEC_PLAN_WORK ? S * k : 0;
    const int nr = status == QFEC_PLAN_WORK ? k * (S - 1) : 0;
    for (int pos = L.lane * 16; pos < CL.stride; pos += L.n * 16) {
        uint32_t wd[4] = {0, 0, 0, 0};
        if (pos == 0) {
            wd[0] = (uint32_t)S | (uint32_t)t << 16;
            wd[1] = (uint32_t)status;
        } else if (pos < QFEC_CHECK_IDS) {
            const uint64_t lo = pos == QFEC_CHECK_MARKS ? mk[0] : mk[2], hi = pos == QFEC_CHECK_MARKS ? mk[1] : mk[3];
            wd[0] = (uint32_t)lo;
            wd[1] = (uint32_t)(lo >> 32);
            wd[2] = (uint32_t)hi;
            wd[3] = (uint32_t)(hi >> 32);
        } else if (pos < CL.a_off) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int i = pos - QFEC_CHECK_IDS + q;
                if (i < nids)
                    wd[q >> 2] |= (uint32_t)hdr[i < k ? PL.surv_off + i : PL.lost_off + e + (i - k)] << (8 * (q & 3));
            }
        } else if (pos < CL.r_off) {
            const int i0 = pos - CL.a_off;
            if (i0 < na) {
                int x = i0 / k, c = i0 - x * k;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    if (i0 + q < na)
                        wd[q >> 2] |= (uint32_t)(x ? plan_coef(C, PL, hdr, X, e, e + x, c) : row0[c]) << (8 * (q & 3));
                    if (++c == k) { c = 0; ++x; }
                }
            }
        } else {
            const int i0 = pos - CL.r_off;
            if (i0 < nr) {
                int i = i0 / (S - 1), x = i0 - i * (S - 1);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    if (i0 + q < nr) {
                        const uint8_t a0 = row0[i], ax = plan_coef(C, PL, hdr, X, e, e + 1 + x, i);
                        const uint8_t r = a0 && ax ? C.gexp[C.glog[ax] + 255 - C.glog[a0]] : 0;
                        wd[q >> 2] |= (uint32_t)r << (8 * (q & 3));
                    }
                    if (++x == S - 1) { x = 0; ++i; }
                }
            }
        }
        L.store16(out + pos, wd);
    }
    return status;
}

#undef QFEC_HD

}  // namespace qfec
