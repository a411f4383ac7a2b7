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
    if (d.rep.version == c->version && d.rep.lut) return QFEC_OK;
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
    return upload_lut(d.rep, lut, recs, c->version);
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
    a.lut = d.rep.lut;
    a.records = d.rep.rec;
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
    const FlatGeom f = flat_geom(d_data, d_par, block, pitch, a.dgs, a.pgs);
    const Lane8Geom l8 = lane8_geom(f, c->k, block);
    a.vec16 = f.vec16;
    a.cols = f.cols;
    a.cols8 = l8.cols8;
    a.wpg8 = l8.wpg8;
    return for_group_chunks(groups, l8.per, [&](long long g0, long long gn) {
        a.data = d_data + (size_t)g0 * a.dgs;
        a.parity = d_par + (size_t)g0 * a.pgs;
        a.dmarks = d_marks + (size_t)g0 * c->k;  // rs.c layout: every group's data marks, then the parity marks
        a.pmarks = d_marks + (size_t)groups * c->k + (size_t)g0 * c->m;
        a.groups = (uint64_t)gn;
        const hipError_t e = launch_repair(a, s);
        return e == hipSuccess ? QFEC_OK : hip_fail(e, "repair kernel launch");
    });
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
    DevCtx* ctx = nullptr;
    int rc = batch_begin(
        "qfec_repair",
        bad_batch(code, groups, block_size, pitch) || (groups > 0 && (!d_data || !d_marks || (code->m > 0 && !d_parity))),
        [&] { return code->k + code->m > QFEC_LUT_MAX_N ? repair_unsupported(code) : QFEC_OK; }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
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
    DevCtx* ctx = nullptr;
    int rc = batch_begin(
        "qfec_verify", bad_batch(code, groups, block_size, pitch) || (groups > 0 && (!d_data || (code->m > 0 && !d_parity))),
        [&] {
            if (code->m <= 32) return QFEC_OK;
            set_error("qfec_verify: m = %d > 32 (one bit per parity row in a 32-bit word)", code->m);
            return QFEC_EUNSUP;
        },
        groups == 0 || (!d_bad_rows && !d_bad_groups), &ctx);
    if (rc || !ctx) return rc;
    hipStream_t s = (hipStream_t)stream;
    // the per-group words also decide which OR counts a group, so a call that only wants the
    // counter gets them from stream-ordered scratch
    GroupWords words(s);
    rc = words.init("verify", groups, 1, d_bad_rows);
    if (rc || code->m == 0) return rc;
    uint32_t* tab = nullptr;
    {
        std::lock_guard<std::mutex> lk(code->mu);
        rc = ensure_enc(code, ctx->device, &tab);
    }
    if (rc) return rc;
    VerifyArgs a{};
    a.tab = tab;
    a.bad_groups = d_bad_groups;
    a.k = code->k;
    a.m = code->m;
    a.pitch = (uint64_t)pitch;
    a.block = (uint32_t)block_size;
    a.dgs = (uint64_t)code->k * pitch;
    a.pgs = (uint64_t)code->m * pitch;
    const FlatGeom f = flat_geom(d_data, d_parity, block_size, pitch, a.dgs, a.pgs);
    a.vec16 = f.vec16;
    a.cols = f.cols;
    a.cols_div = make_div_magic(f.cols);
    return for_group_chunks(groups, f.per, [&](long long g0, long long gn) {
        a.data = d_data + (size_t)g0 * a.dgs;
        a.parity = d_parity + (size_t)g0 * a.pgs;
        a.bad_rows = words.at(0) + g0;
        a.work = (uint64_t)gn * a.cols;
        const hipError_t he = launch_verify(a, s);
        return he == hipSuccess ? QFEC_OK : hip_fail(he, "verify kernel launch");
    });
}

}  // extern "C"
