// qfec_ptrs.cpp -- the pointer-table calls of the device API in include/qfec.h: qfec_encode_ptrs and
// qfec_reconstruct_ptrs (kernels: qfec_ptrs.hip).  The table is a device array in module/rs.h's
// shard order -- every group's data shards, then every group's parity shards -- so the two halves,
// and the two halves of the marks, are what a launch over groups [g0, g0 + gn) is handed.  Arguments
// are judged on the host before a device is touched; nothing is read back.
#include "qfec_rt.hpp"

namespace qfec {

static PtrsArgs ptrs_args(const qfec_code* c, int block, bool reconstruct) {
    PtrsArgs a{};
    a.k = c->k;
    a.m = c->m;
    a.block = (uint32_t)block;
    a.lane_bytes = (uint32_t)ptrs_lane_bytes(reconstruct, c->k);
    return a;
}

// cuts the batch into launches; launch(a) sees the chunk's halves of the table (and of the marks)
template <class Launch>
static int ptrs_chunks(PtrsArgs& a, const uint64_t* dptrs, const uint64_t* pptrs, const uint8_t* dmarks,
                       const uint8_t* pmarks, long long groups, const char* what, Launch&& launch) {
    const PtrsGeom p = ptrs_geom((int)a.block, (int)a.lane_bytes);
    a.vcols = p.vcols;
    a.wpg = p.wpg;
    a.tail0 = p.tail0;
    a.tailn = p.tailn;
    return for_group_chunks(groups, p.per, [&](long long g0, long long gn) {
        a.dptrs = dptrs + (size_t)g0 * a.k;
        a.pptrs = pptrs + (size_t)g0 * a.m;
        a.dmarks = dmarks ? dmarks + (size_t)g0 * a.k : nullptr;
        a.pmarks = pmarks ? pmarks + (size_t)g0 * a.m : nullptr;
        a.groups = (uint64_t)gn;
        const hipError_t he = launch(a);
        return he == hipSuccess ? QFEC_OK : hip_fail(he, what);
    });
}

int run_encode_ptrs(const qfec_code* c, const uint32_t* tab, const uint64_t* dptrs, const uint64_t* pptrs,
                    long long groups, int block, hipStream_t s) {
    PtrsArgs a = ptrs_args(c, block, false);
    a.tab = tab;
    return ptrs_chunks(a, dptrs, pptrs, nullptr, nullptr, groups, "encode_ptrs kernel launch",
                       [&](const PtrsArgs& x) { return launch_encode_ptrs(x, s); });
}

int run_reconstruct_ptrs(DevCtx& ctx, const qfec_code* c, const DevLut& dec, const uint64_t* dptrs,
                         const uint64_t* pptrs, const uint8_t* dmarks, const uint8_t* pmarks, long long groups,
                         int block, unsigned* d_failed, hipStream_t s) {
    PtrsArgs a = ptrs_args(c, block, true);
    const RecordLayout L = record_layout(c->k, c->m);
    a.lut = dec.lut;
    a.records = dec.rec;
    a.t256 = ctx.d_t256;
    a.failed = d_failed;
    a.surv_off = L.surv_off;
    a.lost_off = L.lost_off;
    a.hdr = L.hdr;
    a.coff = L.coff;
    return ptrs_chunks(a, dptrs, pptrs, dmarks, pmarks, groups, "reconstruct_ptrs kernel launch",
                       [&](const PtrsArgs& x) { return launch_reconstruct_ptrs(x, s); });
}

}  // namespace qfec

using namespace qfec;

extern "C" {

int qfec_encode_ptrs(qfec_code* code, unsigned char* const* d_shards, long long groups, int block_size, void* stream) {
    const char* why = !code                     ? "null code"
                      : groups < 0              ? "groups < 0"
                      : block_size < 1          ? "block_size < 1"
                      : groups > 0 && !d_shards ? "null d_shards"
                                                : nullptr;
    if (why) {
        set_error("qfec_encode_ptrs: invalid argument (%s)", why);
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
    const uint64_t* t = reinterpret_cast<const uint64_t*>(d_shards);
    return run_encode_ptrs(code, tab, t, t + (size_t)groups * code->k, groups, block_size, (hipStream_t)stream);
}

int qfec_reconstruct_ptrs(qfec_code* code, unsigned char* const* d_shards, const unsigned char* d_marks,
                          long long groups, int block_size, unsigned int* d_failed, void* stream) {
    const char* why = !code                     ? "null code"
                      : groups < 0              ? "groups < 0"
                      : block_size < 1          ? "block_size < 1"
                      : groups > 0 && !d_shards ? "null d_shards"
                      : groups > 0 && !d_marks  ? "null d_marks"
                                                : nullptr;
    if (why) {
        set_error("qfec_reconstruct_ptrs: invalid argument (%s)", why);
        return QFEC_EINVAL;
    }
    if (groups == 0) return QFEC_OK;
    if (code->k + code->m > QFEC_LUT_MAX_N) {
        set_error("qfec_reconstruct_ptrs: k + m = %d > %d (no host-record path on pointer tables)", code->k + code->m,
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
    const uint64_t* t = reinterpret_cast<const uint64_t*>(d_shards);
    return run_reconstruct_ptrs(*ctx, code, d->dec, t, t + (size_t)groups * code->k, d_marks,
                                d_marks + (size_t)groups * code->k, groups, block_size, d_failed, (hipStream_t)stream);
}

}  // extern "C"
