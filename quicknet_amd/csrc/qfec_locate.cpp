// qfec_locate.cpp -- qfec_locate (which single shard of a group is corrupted), qfec_scrub (locate,
// then qfec_repair with the marks it wrote) and qfec_locate_ratios of the device API in
// include/qfec.h.
//
// Per code and device there is one more table set beside the encode's: the perm tables of the
// ratios r_{j,i} = P[j][i] / P[0][i] (k x (m - 1) entries), built on the host under code->mu and
// invalidated by code->version like the encode tables.
#include "qfec_rt.hpp"

namespace qfec {

int locate_code_check(const qfec_code* c, const char* who, bool need_lut) {
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
    if (need_lut && c->k + c->m > QFEC_LUT_MAX_N) {
        set_error("%s: k + m = %d > %d is not supported (the pattern LUT is keyed by the whole mask, as qfec_repair's)",
                  who, c->k + c->m, QFEC_LUT_MAX_N);
        return QFEC_EUNSUP;
    }
    return QFEC_OK;
}

void ratio_rows(const uint8_t* rows, int S, int k, std::vector<uint8_t>& out) {
    const Field& f = field();
    out.assign((size_t)k * (S - 1), 0);
    for (int i = 0; i < k; ++i)
        for (int x = 1; x < S; ++x) out[(size_t)i * (S - 1) + (x - 1)] = f.mul[rows[(size_t)x * k + i]][f.inv[rows[i]]];
}

// perm tables of r_{j,i} = P[j][i] / P[0][i] of `c` on device `dev` (caller holds c->mu; the code
// passed locate_code_check)
int ensure_loc(qfec_code* c, int dev, uint32_t** out) {
    DevTables& d = c->dev[dev];
    if (d.loc_version != c->version || !d.d_loc) {
        std::vector<uint8_t> r;
        ratio_rows(c->rows.data(), c->m, c->k, r);
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

int run_locate(DevCtx& ctx, qfec_code* code, const uint8_t* d_data, const uint8_t* d_parity, long long groups,
               int block_size, long long pitch, int* d_culprit, uint8_t* d_marks, unsigned* d_counts, hipStream_t s) {
    uint32_t *tab = nullptr, *rtab = nullptr;
    int rc;
    {
        std::lock_guard<std::mutex> lk(code->mu);
        rc = ensure_enc(code, ctx.device, &tab);
        if (!rc) rc = ensure_loc(code, ctx.device, &rtab);
    }
    if (rc) return rc;
    GroupWords words(s);  // [groups] bad rows, then [groups] candidates
    rc = words.init("locate", groups, 2);
    if (rc) return rc;
    unsigned *rows = words.at(0), *cand = words.at(1);
    LocateArgs a{};
    a.tab = tab;
    a.rtab = rtab;
    a.k = code->k;
    a.m = code->m;
    a.pitch = (uint64_t)pitch;
    a.block = (uint32_t)block_size;
    a.dgs = (uint64_t)code->k * pitch;
    a.pgs = (uint64_t)code->m * pitch;
    const FlatGeom fg = flat_geom(d_data, d_parity, block_size, pitch, a.dgs, a.pgs);
    a.vec16 = fg.vec16;
    a.cols = fg.cols;
    a.cols_div = make_div_magic(fg.cols);
    rc = for_group_chunks(groups, fg.per, [&](long long g0, long long gn) {
        a.data = d_data + (size_t)g0 * a.dgs;
        a.parity = d_parity + (size_t)g0 * a.pgs;
        a.bad_rows = rows + g0;
        a.cand = cand + g0;
        a.work = (uint64_t)gn * a.cols;
        const hipError_t he = launch_locate(a, s);
        return he == hipSuccess ? QFEC_OK : hip_fail(he, "locate kernel launch");
    });
    if (rc) return rc;
    LocateFinishArgs f{};
    f.bad_rows = rows;
    f.cand = cand;
    f.culprit = d_culprit;
    f.marks = d_marks;
    f.counts = d_counts;
    f.groups = (uint64_t)groups;
    f.k = code->k;
    f.m = code->m;
    const hipError_t he = launch_locate_finish(f, s);
    return he == hipSuccess ? QFEC_OK : hip_fail(he, "locate finish kernel launch");
}

int run_scrub(const char* who, qfec_code* code, uint8_t* d_data, uint8_t* d_parity, long long groups, int block_size,
              long long pitch, size_t extra, unsigned* d_failed, hipStream_t s,
              const std::function<int(uint8_t* marks, uint8_t* extra)>& locate) {
    int rc = qfec_prepare_repair(code);  // the repair LUT (synchronous on its first build) before the stream work
    if (rc) return rc;
    uint8_t* scratch = nullptr;
    const size_t mark_bytes = round_up((size_t)groups * (size_t)(code->k + code->m), 16);
    if (hipMallocAsync((void**)&scratch, mark_bytes + extra, s) != hipSuccess)
        return hip_fail(hipGetLastError(), (std::string(who + 5) + " scratch").c_str());  // who less "qfec_"
    rc = locate(scratch, scratch + mark_bytes);
    if (!rc) rc = qfec_repair(code, d_data, d_parity, scratch, groups, block_size, pitch, d_failed, (void*)s);
    (void)hipFreeAsync(scratch, s);
    return rc;
}

}  // namespace qfec

using namespace qfec;

extern "C" {

int qfec_locate_ratios(const qfec_code* code, unsigned char* out) {
    if (!code || !out) return QFEC_EINVAL;
    const int rc = locate_code_check(code, "qfec_locate_ratios", false);
    if (rc) return rc;
    std::vector<uint8_t> r;
    ratio_rows(code->rows.data(), code->m, code->k, r);
    memcpy(out, r.data(), r.size());
    return QFEC_OK;
}

int qfec_locate(qfec_code* code, const unsigned char* d_data, const unsigned char* d_parity, long long groups,
                int block_size, long long pitch, int* d_culprit, unsigned char* d_marks, unsigned int* d_counts,
                void* stream) {
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(
        "qfec_locate", bad_batch(code, groups, block_size, pitch) || (groups > 0 && (!d_data || !d_parity || !d_culprit)),
        [&] { return locate_code_check(code, "qfec_locate", false); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    return run_locate(*ctx, code, d_data, d_parity, groups, block_size, pitch, d_culprit, d_marks, d_counts,
                      (hipStream_t)stream);
}

int qfec_scrub(qfec_code* code, unsigned char* d_data, unsigned char* d_parity, long long groups, int block_size,
               long long pitch, int* d_culprit, unsigned int* d_counts, void* stream) {
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(
        "qfec_scrub", bad_batch(code, groups, block_size, pitch) || (groups > 0 && (!d_data || !d_parity)),
        [&] {
            const int r = locate_code_check(code, "qfec_scrub", false);
            if (r || code->k + code->m <= QFEC_LUT_MAX_N) return r;
            // qfec_repair's limit, before anything is launched
            set_error("qfec_scrub: k + m = %d > %d is not supported (qfec_repair's limit)", code->k + code->m, QFEC_LUT_MAX_N);
            return QFEC_EUNSUP;
        },
        groups == 0, &ctx);
    if (rc || !ctx) return rc;
    hipStream_t s = (hipStream_t)stream;
    // the verdicts come from the scratch too when the caller does not want them
    return run_scrub("qfec_scrub", code, d_data, d_parity, groups, block_size, pitch, d_culprit ? 0 : (size_t)groups * 4,
                     nullptr, s, [&](uint8_t* marks, uint8_t* extra) {
                         return run_locate(*ctx, code, d_data, d_parity, groups, block_size, pitch,
                                           d_culprit ? d_culprit : (int*)extra, marks, d_counts, s);
                     });
}

}  // extern "C"
