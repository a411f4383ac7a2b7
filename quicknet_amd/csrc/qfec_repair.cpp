// qfec_repair.cpp -- one-pass group repair (qfec_repair: every marked shard, data and parity) and
// the batched parity check (qfec_verify) of the device API in include/qfec.h.
//
// Repair has a LUT of its own per code and device, keyed by the full n-bit erasure mask (the
// reconstruct's LUT shares records between masks that differ only in unused parity; a repair row
// set depends on every bit).  Its records are compact: the RecordLayout header with the byte
// offsets of the coefficients' tables in the 256-entry table, no inline tables -- RS(20,4) has
// 12 950 repairable patterns of 448 B each (5.8 MB) beside the 64 MiB LUT at n = 24.
#include "qfec_rt.hpp"

namespace qfec {

// device LUT (2^n entries) + the compact repair records of `c` (caller holds c->mu)
static int ensure_repair_lut(qfec_code* c, int dev, DevTables** out) {
    DevTables& d = c->dev[dev];
    *out = &d;
    if (d.rep_version == c->version && d.d_rep_lut) return QFEC_OK;
    const int k = c->k, m = c->m, n = k + m;
    const size_t nmask = (size_t)1 << n;
    const RecordLayout L = record_layout(k, m);
    std::vector<int32_t> lut(nmask);
    std::vector<uint32_t> recs;
    std::vector<uint8_t> marks((size_t)n), rows;
    std::vector<int> surv, lost;
    for (size_t mask = 0; mask < nmask; ++mask) {
        const int t = __builtin_popcountll((unsigned long long)mask);
        if (t == 0) { lut[mask] = QFEC_REC_NONE; continue; }
        if (t > m) { lut[mask] = QFEC_REC_FAIL; continue; }
        for (int i = 0; i < n; ++i) marks[i] = (mask >> i) & 1;
        int e = 0;
        if (repair_rows(c->rows.data(), k, m, marks.data(), rows, surv, lost, full_of(c), &e) != t) {
            lut[mask] = QFEC_REC_FAIL;
            continue;
        }
        const size_t off = recs.size();
        recs.resize(off + (size_t)L.hdr);
        build_repair_record(L, k, t, e, rows.data(), surv.data(), lost.data(), c->quirk != 0, &recs[off]);
        lut[mask] = (int32_t)off;
    }
    if (d.d_rep_lut) HIP_TRY(hipFree(d.d_rep_lut));
    if (d.d_rep_rec) HIP_TRY(hipFree(d.d_rep_rec));
    d.d_rep_lut = nullptr;
    d.d_rep_rec = nullptr;
    HIP_TRY(hipMalloc(&d.d_rep_lut, nmask * 4));
    HIP_TRY(hipMalloc(&d.d_rep_rec, std::max<size_t>(recs.size(), 8) * 4));
    HIP_TRY(hipMemcpy(d.d_rep_lut, lut.data(), nmask * 4, hipMemcpyHostToDevice));
    if (!recs.empty()) HIP_TRY(hipMemcpy(d.d_rep_rec, recs.data(), recs.size() * 4, hipMemcpyHostToDevice));
    d.rep_version = c->version;
    return QFEC_OK;
}

static int repair_unsupported(const qfec_code* c) {
    set_error("qfec_repair: k + m = %d > %d is not supported (no host-record path for repair)", c->k + c->m,
              QFEC_LUT_MAX_N);
    return QFEC_EUNSUP;
}

static int run_repair(DevCtx& ctx, const qfec_code* c, const DevTables& d, uint8_t* d_data, uint8_t* d_par,
                      const uint8_t* d_marks, long long groups, int block, long long pitch, unsigned* d_failed,
                      hipStream_t s) {
    RepairArgs a{};
    const RecordLayout L = record_layout(c->k, c->m);
    a.lut = d.d_rep_lut;
    a.records = d.d_rep_rec;
    a.t256 = ctx.d_t256;
    a.failed = d_failed;
    a.pitch = (uint64_t)pitch;
    a.k = c->k;
    a.m = c->m;
    a.surv_off = L.surv_off;
    a.lost_off = L.lost_off;
    a.coff = L.coff;
    a.dgs = (uint64_t)c->k * pitch;
    a.pgs = (uint64_t)c->m * pitch;
    a.vec16 = vec16_ok(d_data, d_par, block, pitch) ? 1 : 0;
    a.cols = a.vec16 ? (uint32_t)((block + 15) / 16) : (uint32_t)block;
    // 8-B columns: the 16-B columns' span for k < 14, else just the row (as the reconstruct, whose
    // measurements this follows: qfec_runtime.cpp run_reconstruct)
    a.cols8 = a.vec16 && c->k < 14 ? 2u * a.cols : (uint32_t)((block + 7) / 8);
    a.wpg8 = (a.cols8 + 63) / 64;
    const long long per = std::max<long long>(1, 0x7FFFFFFFll / (long long)std::max(a.wpg8, 1u));
    for (long long g0 = 0; g0 < groups; g0 += per) {
        const long long gn = std::min(per, groups - g0);
        a.data = d_data + (size_t)g0 * a.dgs;
        a.parity = d_par + (size_t)g0 * a.pgs;
        a.dmarks = d_marks + (size_t)g0 * c->k;  // rs.c layout: every group's data marks, then the parity marks
        a.pmarks = d_marks + (size_t)groups * c->k + (size_t)g0 * c->m;
        a.groups = (uint64_t)gn;
        hipError_t e = launch_repair(a, s);
        if (e != hipSuccess) return hip_fail(e, "repair kernel launch");
    }
    return QFEC_OK;
}

}  // namespace qfec

using namespace qfec;

extern "C" {

int qfec_prepare_repair(qfec_code* code) {
    if (!code) return QFEC_EINVAL;
    if (code->k + code->m > QFEC_LUT_MAX_N) return repair_unsupported(code);
    DevCtx* ctx = nullptr;
    int rc = current_ctx(&ctx);
    if (rc) return rc;
    DevTables* d = nullptr;
    std::lock_guard<std::mutex> lk(code->mu);
    return ensure_repair_lut(code, ctx->device, &d);
}

int qfec_repair(qfec_code* code, unsigned char* d_data, unsigned char* d_parity, const unsigned char* d_marks,
                long long groups, int block_size, long long pitch, unsigned int* d_failed, void* stream) {
    if (!code || groups < 0 || block_size < 1 || pitch < block_size ||
        (groups > 0 && (!d_data || !d_marks || (code->m > 0 && !d_parity)))) {
        set_error("qfec_repair: invalid argument");
        return QFEC_EINVAL;
    }
    if (code->k + code->m > QFEC_LUT_MAX_N) return repair_unsupported(code);
    if (groups == 0) return QFEC_OK;
    DevCtx* ctx = nullptr;
    int rc = current_ctx(&ctx);
    if (rc) return rc;
    DevTables* d = nullptr;
    {
        std::lock_guard<std::mutex> lk(code->mu);
        rc = ensure_repair_lut(code, ctx->device, &d);
    }
    if (rc) return rc;
    return run_repair(*ctx, code, *d, d_data, d_parity, d_marks, groups, block_size, pitch, d_failed,
                      (hipStream_t)stream);
}

int qfec_repair_rows(const qfec_code* code, const unsigned char* marks_n, unsigned char* rows_out,
                     int* survivors_out, int* lost_out) {
    if (!code || !marks_n) return QFEC_EINVAL;
    std::vector<uint8_t> rows;
    std::vector<int> surv, lost;
    const int t = repair_rows(code->rows.data(), code->k, code->m, marks_n, rows, surv, lost, full_of(code));
    if (t > 0) {
        if (rows_out) memcpy(rows_out, rows.data(), rows.size());
        if (survivors_out) memcpy(survivors_out, surv.data(), surv.size() * sizeof(int));
        if (lost_out) memcpy(lost_out, lost.data(), lost.size() * sizeof(int));
    }
    return t;
}

int qfec_verify(qfec_code* code, const unsigned char* d_data, const unsigned char* d_parity, long long groups,
                int block_size, long long pitch, unsigned int* d_bad_rows, unsigned int* d_bad_groups,
                void* stream) {
    if (!code || groups < 0 || block_size < 1 || pitch < block_size ||
        (groups > 0 && (!d_data || (code->m > 0 && !d_parity)))) {
        set_error("qfec_verify: invalid argument");
        return QFEC_EINVAL;
    }
    if (code->m > 32) {
        set_error("qfec_verify: m = %d > 32 (one bit per parity row in a 32-bit word)", code->m);
        return QFEC_EUNSUP;
    }
    if (groups == 0 || (!d_bad_rows && !d_bad_groups)) return QFEC_OK;
    DevCtx* ctx = nullptr;
    int rc = current_ctx(&ctx);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    // the per-group words also decide which OR counts a group, so a call that only wants the
    // counter gets them from stream-ordered scratch
    unsigned* rows = d_bad_rows;
    if (!rows && hipMallocAsync((void**)&rows, (size_t)groups * 4, s) != hipSuccess)
        return hip_fail(hipGetLastError(), "verify scratch");
    auto done = [&](int r) {
        if (!d_bad_rows) (void)hipFreeAsync(rows, s);
        return r;
    };
    hipError_t he = hipMemsetAsync(rows, 0, (size_t)groups * 4, s);
    if (he != hipSuccess) return done(hip_fail(he, "verify: zeroing bad_rows"));
    if (code->m == 0) return done(QFEC_OK);
    uint32_t* tab = nullptr;
    {
        std::lock_guard<std::mutex> lk(code->mu);
        rc = ensure_enc(code, ctx->device, &tab);
    }
    if (rc) return done(rc);
    VerifyArgs a{};
    a.tab = tab;
    a.bad_groups = d_bad_groups;
    a.k = code->k;
    a.m = code->m;
    a.pitch = (uint64_t)pitch;
    a.block = (uint32_t)block_size;
    a.dgs = (uint64_t)code->k * pitch;
    a.pgs = (uint64_t)code->m * pitch;
    a.vec16 = vec16_ok(d_data, d_parity, block_size, pitch) ? 1 : 0;
    a.cols = a.vec16 ? (uint32_t)((block_size + 15) / 16) : (uint32_t)block_size;
    a.cols_div = make_div_magic(a.cols);
    // batches of >= 2^31 lanes go in several launches, as the encode's (run_encode)
    const long long per = std::max<long long>(1, (long long)(0x7FFFFFFFll / a.cols));
    for (long long g0 = 0; g0 < groups; g0 += per) {
        const long long gn = std::min(per, groups - g0);
        a.data = d_data + (size_t)g0 * a.dgs;
        a.parity = d_parity + (size_t)g0 * a.pgs;
        a.bad_rows = rows + g0;
        a.work = (uint64_t)gn * a.cols;
        he = launch_verify(a, s);
        if (he != hipSuccess) return done(hip_fail(he, "verify kernel launch"));
    }
    return done(QFEC_OK);
}

}  // extern "C"
