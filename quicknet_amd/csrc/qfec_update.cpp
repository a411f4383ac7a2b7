// qfec_update.cpp -- incremental parity of the device API in include/qfec.h: qfec_encode_update (a
// range of the k columns, the same for every group) and qfec_update (one replaced data shard per
// group).  Both run on the encode's tables (ensure_enc) and need nothing else on the device: no
// LUT, no scratch, no read-back.  Arguments are judged on the host before a device is touched.
#include "qfec_rt.hpp"

namespace qfec {

// the encode tables of `code` on the calling thread's device
static int enc_tables(qfec_code* code, DevCtx** ctx, uint32_t** tab) {
    int rc = current_ctx(ctx);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(code->mu);
    return ensure_enc(code, (*ctx)->device, tab);
}

}  // namespace qfec

using namespace qfec;

extern "C" {

int qfec_encode_update(qfec_code* code, int first, int count, const unsigned char* d_part, unsigned char* d_parity,
                       long long groups, int block_size, long long pitch, int accumulate, void* stream) {
    const char* why = !code                                   ? "null code"
                      : first < 0                             ? "first < 0"
                      : count < 1                             ? "count < 1"
                      : (long long)first + count > code->k    ? "first + count > k"
                      : groups < 0                            ? "groups < 0"
                      : block_size < 1                        ? "block_size < 1"
                      : pitch < block_size                    ? "pitch < block_size"
                      : accumulate != 0 && accumulate != 1    ? "accumulate is not 0 or 1"
                      : groups > 0 && (!d_part || !d_parity)  ? "null buffer"
                                                              : nullptr;
    if (why) {
        set_error("qfec_encode_update: invalid argument (%s)", why);
        return QFEC_EINVAL;
    }
    if (groups == 0 || code->m == 0) return QFEC_OK;
    DevCtx* ctx = nullptr;
    uint32_t* tab = nullptr;
    const int rc = enc_tables(code, &ctx, &tab);
    if (rc) return rc;
    EncUpdateArgs a{};
    a.tab = tab;
    a.k = code->k;
    a.m = code->m;
    a.first = first;
    a.count = count;
    a.accumulate = accumulate;
    a.pitch = (uint64_t)pitch;
    a.sgs = (uint64_t)count * pitch;
    a.pgs = (uint64_t)code->m * pitch;
    const FlatGeom f = flat_geom(d_part, d_parity, block_size, pitch, a.sgs, a.pgs);
    a.vec16 = f.vec16;
    a.cols = f.cols;
    a.cols_div = make_div_magic(f.cols);
    return for_group_chunks(groups, f.per, [&](long long g0, long long gn) {
        a.part = d_part + (size_t)g0 * a.sgs;
        a.parity = d_parity + (size_t)g0 * a.pgs;
        a.work = (uint64_t)gn * a.cols;
        const hipError_t he = launch_encode_update(a, (hipStream_t)stream);
        return he == hipSuccess ? QFEC_OK : hip_fail(he, "encode_update kernel launch");
    });
}

int qfec_update(qfec_code* code, const int* d_shard, unsigned char* d_data, const unsigned char* d_rows,
                unsigned char* d_parity, long long groups, int block_size, long long pitch, unsigned int* d_invalid,
                void* stream) {
    const char* why = !code                                               ? "null code"
                      : groups < 0                                        ? "groups < 0"
                      : block_size < 1                                    ? "block_size < 1"
                      : pitch < block_size                                ? "pitch < block_size"
                      : groups > 0 && (!d_shard || !d_rows || !d_parity)  ? "null buffer"
                                                                          : nullptr;
    if (why) {
        set_error("qfec_update: invalid argument (%s)", why);
        return QFEC_EINVAL;
    }
    if (groups == 0 || code->m == 0) return QFEC_OK;
    DevCtx* ctx = nullptr;
    uint32_t* tab = nullptr;
    const int rc = enc_tables(code, &ctx, &tab);
    if (rc) return rc;
    UpdateArgs a{};
    a.tab = tab;
    a.invalid = d_invalid;
    a.k = code->k;
    a.m = code->m;
    a.pitch = (uint64_t)pitch;
    a.dgs = (uint64_t)code->k * pitch;
    a.pgs = (uint64_t)code->m * pitch;
    // three buffers: the data base joins the two that flat_geom looks at (an unaligned base there
    // sends the call down the byte path)
    const bool data16 = !d_data || (uintptr_t)d_data % 16 == 0;
    const FlatGeom f = flat_geom(data16 ? d_rows : d_data, d_parity, block_size, pitch, a.pitch | a.dgs, a.pgs);
    a.vec16 = f.vec16;
    long long per = f.per;
    if (f.vec16) {
        const WaveGeom w = wave_geom(f);
        a.cols = w.cols;
        a.wpg = w.wpg;
        per = w.per;
    } else {
        a.cols = f.cols;
        a.cols_div = make_div_magic(f.cols);
    }
    return for_group_chunks(groups, per, [&](long long g0, long long gn) {
        a.shard = d_shard + g0;
        a.data = d_data ? d_data + (size_t)g0 * a.dgs : nullptr;
        a.rows = d_rows + (size_t)g0 * a.pitch;
        a.parity = d_parity + (size_t)g0 * a.pgs;
        a.groups = (uint64_t)gn;
        a.work = a.vec16 ? 0 : (uint64_t)gn * a.cols;
        const hipError_t he = launch_update(a, (hipStream_t)stream);
        return he == hipSuccess ? QFEC_OK : hip_fail(he, "update kernel launch");
    });
}

}  // extern "C"
