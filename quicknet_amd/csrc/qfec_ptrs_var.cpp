// qfec_ptrs_var.cpp -- the pointer-table calls with per-shard lengths of include/qfec.h:
// qfec_encode_ptrs_var and qfec_reconstruct_ptrs_var (kernels: qfec_ptrs_var.hip).  Table and marks as
// in qfec_ptrs.cpp; d_lens holds a length per data shard in table order, d_group_len one per group, so
// a launch over groups [g0, g0 + gn) is handed d_lens + g0 * k and d_group_len + g0.  max_len only
// sizes the launch: the waves per group and the groups per launch are those of ptrs_geom(max_len).
// Arguments are judged on the host before a device is touched; nothing is read back.
#include "qfec_rt.hpp"

namespace qfec {

// cuts the batch into launches; launch(a) sees the chunk's parts of the table, the marks and the lengths
template <class Launch>
static int ptrs_var_chunks(const qfec_code* c, bool reconstruct, PtrsVarArgs a, const uint64_t* shards, const int32_t* lens,
                           int32_t* glen_out, const int32_t* glen, const uint8_t* marks, long long groups, int max_len,
                           const char* what, Launch&& launch) {
    a.p.k = c->k;
    a.p.m = c->m;
    a.p.block = (uint32_t)max_len;
    a.p.lane_bytes = (uint32_t)ptrs_lane_bytes(reconstruct, c->k);
    const PtrsGeom p = ptrs_geom(max_len, (int)a.p.lane_bytes);
    a.p.vcols = p.vcols;
    a.p.wpg = p.wpg;
    a.p.tail0 = p.tail0;
    a.p.tailn = p.tailn;
    const uint64_t* pptrs = shards + (size_t)groups * c->k;
    const uint8_t* pmarks = marks ? marks + (size_t)groups * c->k : nullptr;
    return for_group_chunks(groups, p.per, [&](long long g0, long long gn) {
        a.p.dptrs = shards + (size_t)g0 * c->k;
        a.p.pptrs = pptrs + (size_t)g0 * c->m;
        a.p.dmarks = marks ? marks + (size_t)g0 * c->k : nullptr;
        a.p.pmarks = pmarks ? pmarks + (size_t)g0 * c->m : nullptr;
        a.lens = lens + (size_t)g0 * c->k;
        a.group_len_out = glen_out ? glen_out + g0 : nullptr;
        a.group_len = glen ? glen + g0 : nullptr;
        a.p.groups = (uint64_t)gn;
        const hipError_t he = launch(a);
        return he == hipSuccess ? QFEC_OK : hip_fail(he, what);
    });
}

}  // namespace qfec

using namespace qfec;

extern "C" {

int qfec_encode_ptrs_var(qfec_code* code, unsigned char* const* d_shards, const int* d_lens, long long groups, int max_len,
                         int* d_group_len, unsigned int* d_invalid, void* stream) {
    const char* why = !code                     ? "null code"
                      : groups < 0              ? "groups < 0"
                      : max_len < 1             ? "max_len < 1"
                      : groups > 0 && !d_shards ? "null d_shards"
                      : groups > 0 && !d_lens   ? "null d_lens"
                                                : nullptr;
    if (why) {
        set_error("qfec_encode_ptrs_var: invalid argument (%s)", why);
        return QFEC_EINVAL;
    }
    if (groups == 0 || code->m == 0) return QFEC_OK;
    DevCtx* ctx = nullptr;
    int rc = current_ctx(&ctx);
    if (rc) return rc;
    uint32_t* tab = nullptr;
    {
        std::lock_guard<std::mutex> lk(code->mu);
        rc = ensure_enc(code, ctx->device, &tab);
    }
    if (rc) return rc;
    PtrsVarArgs a{};
    a.p.tab = tab;
    a.invalid = d_invalid;
    return ptrs_var_chunks(code, false, a, reinterpret_cast<const uint64_t*>(d_shards), d_lens, d_group_len, nullptr,
                           nullptr, groups, max_len, "encode_ptrs_var kernel launch",
                           [&](const PtrsVarArgs& x) { return launch_encode_ptrs_var(x, (hipStream_t)stream); });
}

int qfec_reconstruct_ptrs_var(qfec_code* code, unsigned char* const* d_shards, const int* d_lens, const int* d_group_len,
                              const unsigned char* d_marks, long long groups, int max_len, unsigned int* d_failed,
                              unsigned int* d_invalid, void* stream) {
    const char* why = !code                        ? "null code"
                      : groups < 0                 ? "groups < 0"
                      : max_len < 1                ? "max_len < 1"
                      : groups > 0 && !d_shards    ? "null d_shards"
                      : groups > 0 && !d_lens      ? "null d_lens"
                      : groups > 0 && !d_marks     ? "null d_marks"
                      : groups > 0 && !d_group_len ? "null d_group_len"
                                                   : nullptr;
    if (why) {
        set_error("qfec_reconstruct_ptrs_var: invalid argument (%s)", why);
        return QFEC_EINVAL;
    }
    if (groups == 0) return QFEC_OK;
    if (code->k + code->m > QFEC_LUT_MAX_N) {
        set_error("qfec_reconstruct_ptrs_var: k + m = %d > %d (no host-record path on pointer tables)", code->k + code->m,
                  QFEC_LUT_MAX_N);
        return QFEC_EUNSUP;
    }
    DevCtx* ctx = nullptr;
    int rc = current_ctx(&ctx);
    if (rc) return rc;
    DevTables* d = nullptr;
    {
        std::lock_guard<std::mutex> lk(code->mu);
        rc = ensure_lut(code, ctx->device, &d);
    }
    if (rc) return rc;
    const RecordLayout R = record_layout(code->k, code->m);
    PtrsVarArgs a{};
    a.p.lut = d->dec.lut;
    a.p.records = d->dec.rec;
    a.p.t256 = ctx->d_t256;
    a.p.failed = d_failed;
    a.p.surv_off = R.surv_off;
    a.p.lost_off = R.lost_off;
    a.p.hdr = R.hdr;
    a.p.coff = R.coff;
    a.invalid = d_invalid;
    return ptrs_var_chunks(code, true, a, reinterpret_cast<const uint64_t*>(d_shards), d_lens, nullptr, d_group_len,
                           d_marks, groups, max_len, "reconstruct_ptrs_var kernel launch",
                           [&](const PtrsVarArgs& x) { return launch_reconstruct_ptrs_var(x, (hipStream_t)stream); });
}

}  // extern "C"
