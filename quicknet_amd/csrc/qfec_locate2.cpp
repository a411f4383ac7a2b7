// qfec_locate2.cpp -- qfec_locate2 (which two shards of a group are corrupted), qfec_scrub2 (locate2,
// then qfec_repair with the marks it wrote) and qfec_locate2_checks of the device API in
// include/qfec.h.
//
// H = [rows | I_m]; column h_x is column x of the parity rows for a data shard, the unit vector e_j
// for parity row x = k + j.  A pair {a, b} explains a byte's syndromes s iff s is in span{h_a, h_b},
// iff F_ab x s = 0 for the (m - 2) x m matrix F_ab whose rows span the left null space of [h_a h_b].
// F_ab is kept in reduced form: with p0 < p1 the first two rows on which [h_a h_b] is invertible,
// the check of every other row j reads s_j ^ alpha_j x s_p0 ^ beta_j x s_p1 = 0.  For two data
// shards of an MDS code that is p0, p1 = 0, 1 and two multiplies per check; for (data a, parity j)
// beta is zero and alpha the single-shard ratio with row j left out (against row 1 when j = 0); for
// two parity rows both are zero and the checks say that every other syndrome is zero.
// Per code the checks of all n (n - 1) / 2 pairs are built on the host once per code->version under
// code->mu, together with the acceptance check, and uploaded per device as offsets into the
// 256-entry perm table.
#include "qfec_rt.hpp"

namespace qfec {

static void h_column(const qfec_code* c, int x, uint8_t* h) {
    for (int j = 0; j < c->m; ++j) h[j] = x < c->k ? c->rows[(size_t)j * c->k + x] : (uint8_t)(x - c->k == j);
}

// rank of the m x 3 matrix [u v w] == 3 ?
static bool independent3(const uint8_t* u, const uint8_t* v, const uint8_t* w, int m) {
    const Field& f = field();
    std::vector<uint8_t> a((size_t)m * 3);
    for (int j = 0; j < m; ++j) {
        a[(size_t)j * 3] = u[j];
        a[(size_t)j * 3 + 1] = v[j];
        a[(size_t)j * 3 + 2] = w[j];
    }
    int rank = 0;
    for (int col = 0; col < 3; ++col) {
        int piv = rank;
        while (piv < m && !a[(size_t)piv * 3 + col]) ++piv;
        if (piv == m) return false;
        for (int x = 0; x < 3; ++x) std::swap(a[(size_t)piv * 3 + x], a[(size_t)rank * 3 + x]);
        const uint8_t inv = f.inv[a[(size_t)rank * 3 + col]];
        for (int j = rank + 1; j < m; ++j) {
            const uint8_t q = f.mul[a[(size_t)j * 3 + col]][inv];
            if (q)
                for (int x = 0; x < 3; ++x) a[(size_t)j * 3 + x] ^= f.mul[q][a[(size_t)rank * 3 + x]];
        }
        ++rank;
    }
    return true;
}

// F_ab ((m - 2) x m) of two independent columns; false if they are proportional
static bool pair_checks(const uint8_t* ha, const uint8_t* hb, int m, uint8_t* F) {
    const Field& f = field();
    int p0 = -1, p1 = -1;
    uint8_t det = 0;
    for (int x = 0; x < m && p0 < 0; ++x)
        for (int y = x + 1; y < m; ++y) {
            det = f.mul[ha[x]][hb[y]] ^ f.mul[ha[y]][hb[x]];
            if (det) {
                p0 = x;
                p1 = y;
                break;
            }
        }
    if (p0 < 0) return false;
    const uint8_t inv = f.inv[det];
    memset(F, 0, (size_t)(m - 2) * m);
    int r = 0;
    for (int j = 0; j < m; ++j) {
        if (j == p0 || j == p1) continue;
        uint8_t* row = F + (size_t)r++ * m;
        row[p0] = f.mul[f.mul[ha[j]][hb[p1]] ^ f.mul[ha[p1]][hb[j]]][inv];
        row[p1] = f.mul[f.mul[ha[p0]][hb[j]] ^ f.mul[hb[p0]][ha[j]]][inv];
        row[j] = 1;
    }
    return true;
}

// Can two-shard location work on this code?  Builds the checks of every pair on the way (caller
// holds c->mu).  Sets the error text on a refusal.
static int ensure_locate2_host(qfec_code* c, const char* who) {
    if (c->l2_host_version != c->version) {
        const int k = c->k, m = c->m, n = k + m;
        char why[200] = "";
        c->l2_checks.clear();
        c->l2_rc = QFEC_OK;
        if (m < 4)
            snprintf(why, sizeof why, "m = %d < 4 (two corrupted shards need a code of distance 5: four parity rows)", m);
        else if (n > QFEC_LOC2_MAX_N)
            snprintf(why, sizeof why, "k + m = %d > %d is not supported (one candidate bit per pair of shards)", n,
                     QFEC_LOC2_MAX_N);
        else {
            std::vector<uint8_t> h((size_t)n * m);
            for (int x = 0; x < n; ++x) h_column(c, x, &h[(size_t)x * m]);
            for (int x = 0; x < n && !why[0]; ++x)
                for (int y = x + 1; y < n && !why[0]; ++y)
                    for (int z = y + 1; z < n; ++z)
                        if (!independent3(&h[(size_t)x * m], &h[(size_t)y * m], &h[(size_t)z * m], m)) {
                            snprintf(why, sizeof why,
                                     "columns %d, %d and %d of [rows | I] are linearly dependent (the code's distance is "
                                     "below 4: one and two corrupted shards cannot be told apart)", x, y, z);
                            break;
                        }
            if (!why[0]) {
                const size_t per = (size_t)(m - 2) * m;
                c->l2_checks.resize((size_t)n * (n - 1) / 2 * per);
                size_t p = 0;
                for (int a = 0; a < n; ++a)
                    for (int b = a + 1; b < n; ++b, ++p)
                        pair_checks(&h[(size_t)a * m], &h[(size_t)b * m], m, &c->l2_checks[p * per]);  // independent: checked above
            }
        }
        if (why[0]) {
            c->l2_rc = QFEC_EUNSUP;
            c->l2_error = why;
        }
        c->l2_host_version = c->version;
    }
    if (c->l2_rc) set_error("%s: %s", who, c->l2_error.c_str());
    return c->l2_rc;
}

static int locate2_supported(qfec_code* c, const char* who) {
    const int rc = locate_code_check(c, who, false);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    return ensure_locate2_host(c, who);
}

// index of the pair (a, b), a < b, in the order (0,1), (0,2), .. (n-2,n-1)
static size_t pair_index(int a, int b, int n) { return (size_t)a * (2 * n - a - 1) / 2 + (size_t)(b - a - 1); }

// the checks as table offsets, then the pairs' ids, of `c` on device `dev` (caller holds c->mu;
// ensure_locate2_host passed)
static int ensure_loc2(qfec_code* c, int dev, uint32_t** out) {
    DevTables& d = c->dev[dev];
    if (d.loc2_version != c->version || !d.d_loc2) {
        const int n = c->k + c->m;
        std::vector<uint32_t> t(c->l2_checks.size() + (size_t)n * (n - 1) / 2);
        for (size_t x = 0; x < c->l2_checks.size(); ++x) t[x] = (uint32_t)c->l2_checks[x] * (QFEC_TAB_STRIDE * 4);
        size_t p = c->l2_checks.size();
        for (int a = 0; a < n; ++a)
            for (int b = a + 1; b < n; ++b) t[p++] = (uint32_t)a | (uint32_t)b << 8;
        if (d.d_loc2) HIP_TRY(hipFree(d.d_loc2));
        d.d_loc2 = nullptr;
        HIP_TRY(hipMalloc(&d.d_loc2, t.size() * 4));
        HIP_TRY(hipMemcpy(d.d_loc2, t.data(), t.size() * 4, hipMemcpyHostToDevice));
        d.loc2_version = c->version;
    }
    *out = d.d_loc2;
    return QFEC_OK;
}

// the launches of one qfec_locate2: qfec_locate's into scratch verdicts, the counter's preset, then
// the list, pair and finish kernels
static int run_locate2(DevCtx& ctx, qfec_code* code, const uint8_t* d_data, const uint8_t* d_parity, long long groups,
                       int block_size, long long pitch, int* d_culprit, uint8_t* d_marks, unsigned* d_counts,
                       hipStream_t s) {
    if (groups > 0xFFFFFFFFll) {
        set_error("qfec_locate2: %lld groups in one call (at most 2^32 - 1)", groups);
        return QFEC_EINVAL;
    }
    uint32_t *tab = nullptr, *loc2 = nullptr;
    int rc;
    {
        std::lock_guard<std::mutex> lk(code->mu);
        rc = ensure_locate2_host(code, "qfec_locate2");
        if (!rc) rc = ensure_enc(code, ctx.device, &tab);
        if (!rc) rc = ensure_loc2(code, ctx.device, &loc2);
    }
    if (rc) return rc;
    // [4] the list's counter (one word used), then [groups] each: stage-1 verdicts, list, pair verdicts
    struct Scratch {
        hipStream_t s;
        unsigned* p = nullptr;
        ~Scratch() {
            if (p) (void)hipFreeAsync(p, s);
        }
    } scratch{s};
    if (hipMallocAsync((void**)&scratch.p, (4 + 3 * (size_t)groups) * 4, s) != hipSuccess)
        return hip_fail(hipGetLastError(), "locate2 scratch");
    int* stage1 = (int*)(scratch.p + 4);
    rc = run_locate(ctx, code, d_data, d_parity, groups, block_size, pitch, stage1, nullptr, nullptr, s);
    if (rc) return rc;
    hipError_t he = hipMemsetAsync(scratch.p, 0, 16, s);
    if (he != hipSuccess) return hip_fail(he, "locate2: zeroing the list counter");
    const int n = code->k + code->m;
    Locate2Args a{};
    a.data = d_data;
    a.parity = d_parity;
    a.tab = tab;
    a.t256 = ctx.d_t256;
    a.pairs = n * (n - 1) / 2;
    a.checks = loc2;
    a.pair_ids = loc2 + (size_t)a.pairs * (code->m - 2) * code->m;
    a.stage1 = stage1;
    a.list_n = scratch.p;
    a.list = scratch.p + 4 + (size_t)groups;
    a.verdict2 = (int*)(scratch.p + 4 + 2 * (size_t)groups);
    a.groups = (uint64_t)groups;
    a.pitch = (uint64_t)pitch;
    a.block = (uint32_t)block_size;
    a.k = code->k;
    a.m = code->m;
    a.dgs = (uint64_t)code->k * pitch;
    a.pgs = (uint64_t)code->m * pitch;
    const FlatGeom fg = flat_geom(d_data, d_parity, block_size, pitch, a.dgs, a.pgs);
    a.vec16 = fg.vec16;
    a.cols = fg.cols;
    he = launch_locate2_list(a, s);
    if (he != hipSuccess) return hip_fail(he, "locate2 list kernel launch");
    he = launch_locate2_pairs(a, s);
    if (he != hipSuccess) return hip_fail(he, "locate2 pair kernel launch");
    Locate2FinishArgs f{};
    f.stage1 = stage1;
    f.verdict2 = a.verdict2;
    f.culprit = d_culprit;
    f.marks = d_marks;
    f.counts = d_counts;
    f.groups = (uint64_t)groups;
    f.k = code->k;
    f.m = code->m;
    he = launch_locate2_finish(f, s);
    return he == hipSuccess ? QFEC_OK : hip_fail(he, "locate2 finish kernel launch");
}

}  // namespace qfec

using namespace qfec;

extern "C" {

int qfec_locate2_checks(const qfec_code* code, int a, int b, unsigned char* out) {
    if (!code || !out) return QFEC_EINVAL;
    qfec_code* c = const_cast<qfec_code*>(code);  // the constants are cached in the code, under its mutex
    const int rc = locate2_supported(c, "qfec_locate2_checks");
    if (rc) return rc;
    const int n = c->k + c->m;
    if (a == b || a < 0 || b < 0 || a >= n || b >= n) {
        set_error("qfec_locate2_checks: invalid argument");
        return QFEC_EINVAL;
    }
    const size_t per = (size_t)(c->m - 2) * c->m;
    std::lock_guard<std::mutex> lk(c->mu);
    memcpy(out, &c->l2_checks[pair_index(std::min(a, b), std::max(a, b), n) * per], per);
    return c->m - 2;
}

int qfec_locate2(qfec_code* code, const unsigned char* d_data, const unsigned char* d_parity, long long groups,
                 int block_size, long long pitch, int* d_culprit, unsigned char* d_marks, unsigned int* d_counts,
                 void* stream) {
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(
        "qfec_locate2", bad_batch(code, groups, block_size, pitch) || (groups > 0 && (!d_data || !d_parity || !d_culprit)),
        [&] { return locate2_supported(code, "qfec_locate2"); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    return run_locate2(*ctx, code, d_data, d_parity, groups, block_size, pitch, d_culprit, d_marks, d_counts,
                       (hipStream_t)stream);
}

int qfec_scrub2(qfec_code* code, unsigned char* d_data, unsigned char* d_parity, long long groups, int block_size,
                long long pitch, int* d_culprit, unsigned int* d_counts, void* stream) {
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(
        "qfec_scrub2", bad_batch(code, groups, block_size, pitch) || (groups > 0 && (!d_data || !d_parity)),
        [&] { return locate2_supported(code, "qfec_scrub2"); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    hipStream_t s = (hipStream_t)stream;
    // the verdicts come from the scratch too when the caller does not want them
    return run_scrub("qfec_scrub2", code, d_data, d_parity, groups, block_size, pitch, d_culprit ? 0 : (size_t)groups * 8,
                     nullptr, s, [&](uint8_t* marks, uint8_t* extra) {
                         return run_locate2(*ctx, code, d_data, d_parity, groups, block_size, pitch,
                                            d_culprit ? d_culprit : (int*)extra, marks, d_counts, s);
                     });
}

}  // extern "C"
