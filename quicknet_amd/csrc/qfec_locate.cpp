// qfec_locate.cpp -- qfec_locate (which single shard of a group is corrupted), qfec_scrub (locate,
// then qfec_repair with the marks it wrote) and qfec_locate_ratios of the device API in
// include/qfec.h.
//
// Per code and device there is one more table set beside the encode's: the perm tables of the
// ratios r_{j,i} = P[j][i] / P[0][i] (k x (m - 1) entries), built on the host under code->mu and
// invalidated by code->version like the encode tables.
#include "qfec_rt.hpp"

namespace qfec {

// Can single-shard location work on this code at all?  Decided on the host, before any device.
static int locate_unsupported(const qfec_code* c, const char* who) {
    if (c->m < 2) {
        set_error("%s: m = %d < 2 (one parity row detects an error but cannot tell which shard holds it)", who, c->m);
        return QFEC_EUNSUP;
    }
    if (c->k > 32 || c->m > 32) {
        set_error("%s: k = %d, m = %d: more than 32 (one candidate bit per shard in a 32-bit word)", who, c->k, c->m);
        return QFEC_EUNSUP;
    }
    for (int j = 0; j < c->m; ++j)
        for (int i = 0; i < c->k; ++i)
            if (c->rows[(size_t)j * c->k + i] == 0) {
                set_error("%s: parity row %d has a zero coefficient at data shard %d (an error there would not show in that row)",
                          who, j, i);
                return QFEC_EUNSUP;
            }
    return QFEC_OK;
}

// r_{j,i} = P[j][i] / P[0][i] at [i * (m - 1) + (j - 1)], j = 1..m-1 (the code passed locate_unsupported)
static void locate_ratios(const qfec_code* c, std::vector<uint8_t>& out) {
    const Field& f = field();
    const int k = c->k, m = c->m;
    out.resize((size_t)k * (m - 1));
    for (int i = 0; i < k; ++i)
        for (int j = 1; j < m; ++j) out[(size_t)i * (m - 1) + (j - 1)] = f.mul[c->rows[(size_t)j * k + i]][f.inv[c->rows[i]]];
}

// ratio perm tables of `c` on device `dev` (caller holds c->mu)
static int ensure_loc(qfec_code* c, int dev, uint32_t** out) {
    DevTables& d = c->dev[dev];
    if (d.loc_version != c->version || !d.d_loc) {
        std::vector<uint8_t> r;
        locate_ratios(c, r);
        std::vector<uint32_t> t(r.size() * QFEC_TAB_STRIDE);
        for (size_t x = 0; x < r.size(); ++x) perm_entry(r[x], &t[x * QFEC_TAB_STRIDE]);
        if (d.d_loc) HIP_TRY(hipFree(d.d_loc));
        d.d_loc = nullptr;
        HIP_TRY(hipMalloc(&d.d_loc, std::max<size_t>(t.size(), 8) * 4));
        HIP_TRY(hipMemcpy(d.d_loc, t.data(), t.size() * 4, hipMemcpyHostToDevice));
        d.loc_version = c->version;
    }
    *out = d.d_loc;
    return QFEC_OK;
}

// the launches of one qfec_locate: two presets, the main kernel per chunk, the finish kernel
static int run_locate(DevCtx& ctx, qfec_code* code, const uint8_t* d_data, const uint8_t* d_parity, long long groups,
                      int block_size, long long pitch, int* d_culprit, uint8_t* d_marks, unsigned* d_counts,
                      hipStream_t s) {
    uint32_t *tab = nullptr, *rtab = nullptr;
    int rc;
    {
        std::lock_guard<std::mutex> lk(code->mu);
        rc = ensure_enc(code, ctx.device, &tab);
        if (!rc) rc = ensure_loc(code, ctx.device, &rtab);
    }
    if (rc) return rc;
    // per-group working words from stream-ordered scratch: [groups] bad rows, then [groups] candidates
    unsigned* words = nullptr;
    if (hipMallocAsync((void**)&words, (size_t)groups * 8, s) != hipSuccess)
        return hip_fail(hipGetLastError(), "locate scratch");
    auto done = [&](int r) {
        (void)hipFreeAsync(words, s);
        return r;
    };
    unsigned *rows = words, *cand = words + groups;
    hipError_t he = hipMemsetAsync(rows, 0, (size_t)groups * 4, s);
    if (he == hipSuccess) he = hipMemsetAsync(cand, 0xFF, (size_t)groups * 4, s);
    if (he != hipSuccess) return done(hip_fail(he, "locate: presetting the group words"));
    LocateArgs a{};
    a.tab = tab;
    a.rtab = rtab;
    a.k = code->k;
    a.m = code->m;
    a.pitch = (uint64_t)pitch;
    a.block = (uint32_t)block_size;
    a.dgs = (uint64_t)code->k * pitch;
    a.pgs = (uint64_t)code->m * pitch;
    a.vec16 = vec16_ok(d_data, d_parity, block_size, pitch) ? 1 : 0;
    a.cols = a.vec16 ? (uint32_t)((block_size + 15) / 16) : (uint32_t)block_size;
    a.cols_div = make_div_magic(a.cols);
    // batches of >= 2^31 lanes go in several launches, as qfec_verify's
    const long long per = std::max<long long>(1, (long long)(0x7FFFFFFFll / a.cols));
    for (long long g0 = 0; g0 < groups; g0 += per) {
        const long long gn = std::min(per, groups - g0);
        a.data = d_data + (size_t)g0 * a.dgs;
        a.parity = d_parity + (size_t)g0 * a.pgs;
        a.bad_rows = rows + g0;
        a.cand = cand + g0;
        a.work = (uint64_t)gn * a.cols;
        he = launch_locate(a, s);
        if (he != hipSuccess) return done(hip_fail(he, "locate kernel launch"));
    }
    LocateFinishArgs f{};
    f.bad_rows = rows;
    f.cand = cand;
    f.culprit = d_culprit;
    f.marks = d_marks;
    f.counts = d_counts;
    f.groups = (uint64_t)groups;
    f.k = code->k;
    f.m = code->m;
    he = launch_locate_finish(f, s);
    if (he != hipSuccess) return done(hip_fail(he, "locate finish kernel launch"));
    return done(QFEC_OK);
}

}  // namespace qfec

using namespace qfec;

extern "C" {

int qfec_locate_ratios(const qfec_code* code, unsigned char* out) {
    if (!code || !out) return QFEC_EINVAL;
    const int rc = locate_unsupported(code, "qfec_locate_ratios");
    if (rc) return rc;
    std::vector<uint8_t> r;
    locate_ratios(code, r);
    memcpy(out, r.data(), r.size());
    return QFEC_OK;
}

int qfec_locate(qfec_code* code, const unsigned char* d_data, const unsigned char* d_parity, long long groups,
                int block_size, long long pitch, int* d_culprit, unsigned char* d_marks, unsigned int* d_counts,
                void* stream) {
    if (!code || groups < 0 || block_size < 1 || pitch < block_size ||
        (groups > 0 && (!d_data || !d_parity || !d_culprit))) {
        set_error("qfec_locate: invalid argument");
        return QFEC_EINVAL;
    }
    int rc = locate_unsupported(code, "qfec_locate");
    if (rc) return rc;
    if (groups == 0) return QFEC_OK;
    DevCtx* ctx = nullptr;
    rc = current_ctx(&ctx);
    if (rc) return rc;
    return run_locate(*ctx, code, d_data, d_parity, groups, block_size, pitch, d_culprit, d_marks, d_counts,
                      (hipStream_t)stream);
}

int qfec_scrub(qfec_code* code, unsigned char* d_data, unsigned char* d_parity, long long groups, int block_size,
               long long pitch, int* d_culprit, unsigned int* d_counts, void* stream) {
    if (!code || groups < 0 || block_size < 1 || pitch < block_size || (groups > 0 && (!d_data || !d_parity))) {
        set_error("qfec_scrub: invalid argument");
        return QFEC_EINVAL;
    }
    int rc = locate_unsupported(code, "qfec_scrub");
    if (rc) return rc;
    if (code->k + code->m > QFEC_LUT_MAX_N) {  // qfec_repair's limit, before anything is launched
        set_error("qfec_scrub: k + m = %d > %d is not supported (qfec_repair's limit)", code->k + code->m, QFEC_LUT_MAX_N);
        return QFEC_EUNSUP;
    }
    if (groups == 0) return QFEC_OK;
    DevCtx* ctx = nullptr;
    rc = current_ctx(&ctx);
    if (rc) return rc;
    rc = qfec_prepare_repair(code);  // the repair LUT (synchronous on its first build) before the stream work
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)(code->k + code->m);
    // stream-ordered scratch: the marks, and the verdicts when the caller does not want them
    uint8_t* scratch = nullptr;
    const size_t mark_bytes = round_up((size_t)groups * n, 16);
    if (hipMallocAsync((void**)&scratch, mark_bytes + (d_culprit ? 0 : (size_t)groups * 4), s) != hipSuccess)
        return hip_fail(hipGetLastError(), "scrub scratch");
    int* culprit = d_culprit ? d_culprit : (int*)(scratch + mark_bytes);
    rc = run_locate(*ctx, code, d_data, d_parity, groups, block_size, pitch, culprit, scratch, d_counts, s);
    if (!rc) rc = qfec_repair(code, d_data, d_parity, scratch, groups, block_size, pitch, nullptr, stream);
    (void)hipFreeAsync(scratch, s);
    return rc;
}

}  // extern "C"
