// qfec_update_ptrs.cpp -- incremental parity on pointer tables of include/qfec.h: qfec_encode_update_ptrs,
// qfec_update_ptrs and their forms with per-shard lengths (kernels: qfec_update_ptrs.hip).  The table
// is qfec_encode_ptrs': every group's data addresses, then every group's parity addresses, so a launch
// over groups [g0, g0 + gn) is handed the two halves from g0 on, and d_lens + g0 * k, d_group_len + g0,
// d_shard + g0, d_new + g0, d_new_len + g0.  All four run on the encode's tables (ensure_enc) and need
// nothing else on the device: no LUT, no scratch, no read-back.  block_size / max_len only size the
// launch: waves per group and groups per launch are those of ptrs_geom at 16-B lanes.  Arguments are
// judged on the host before a device is touched.
#include "qfec_rt.hpp"

namespace qfec {

// the part of the argument checks the four calls share; nullptr: fine so far
static const char* common_cause(const qfec_code* code, long long groups, int size, const char* size_cause) {
    return !code        ? "null code"
           : groups < 0 ? "groups < 0"
           : size < 1   ? size_cause
                        : nullptr;
}

static const char* range_cause(const qfec_code* code, int first, int count) {
    return !code                                  ? "null code"
           : first < 0                            ? "first < 0"
           : count < 1                            ? "count < 1"
           : (long long)first + count > code->k   ? "first + count > k"
                                                  : nullptr;
}

// the encode tables on the calling thread's device, the geometry, and the launches over the batch
template <class Launch>
static int run_update_ptrs(qfec_code* code, UpdatePtrsArgs a, unsigned char* const* d_shards, long long groups,
                           int size, const char* what, Launch&& launch) {
    DevCtx* ctx = nullptr;
    int rc = current_ctx(&ctx);
    if (rc) return rc;
    uint32_t* tab = nullptr;
    {
        std::lock_guard<std::mutex> lk(code->mu);
        rc = ensure_enc(code, ctx->device, &tab);
    }
    if (rc) return rc;
    a.tab = tab;
    a.k = code->k;
    a.m = code->m;
    a.block = (uint32_t)size;
    const PtrsGeom p = ptrs_geom(size, 16);
    a.vcols = p.vcols;
    a.wpg = p.wpg;
    a.tail0 = p.tail0;
    a.tailn = p.tailn;
    const uint64_t* dptrs = reinterpret_cast<const uint64_t*>(d_shards);
    const uint64_t* pptrs = dptrs + (size_t)groups * code->k;
    const UpdatePtrsArgs all = a;
    return for_group_chunks(groups, p.per, [&](long long g0, long long gn) {
        a.dptrs = dptrs + (size_t)g0 * a.k;
        a.pptrs = pptrs + (size_t)g0 * a.m;
        a.lens = all.lens ? all.lens + (size_t)g0 * a.k : nullptr;
        a.group_len = all.group_len ? all.group_len + g0 : nullptr;
        a.shard = all.shard ? all.shard + g0 : nullptr;
        a.news = all.news ? all.news + g0 : nullptr;
        a.new_len = all.new_len ? all.new_len + g0 : nullptr;
        a.groups = (uint64_t)gn;
        const hipError_t he = launch(a);
        return he == hipSuccess ? QFEC_OK : hip_fail(he, what);
    });
}

}  // namespace qfec

using namespace qfec;

extern "C" {

int qfec_encode_update_ptrs(qfec_code* code, int first, int count, unsigned char* const* d_shards, long long groups,
                            int block_size, int accumulate, void* stream) {
    const char* why = range_cause(code, first, count);
    if (!why) why = common_cause(code, groups, block_size, "block_size < 1");
    if (!why)
        why = accumulate != 0 && accumulate != 1 ? "accumulate is not 0 or 1"
              : groups > 0 && !d_shards          ? "null d_shards"
                                                 : nullptr;
    if (why) {
        set_error("qfec_encode_update_ptrs: invalid argument (%s)", why);
        return QFEC_EINVAL;
    }
    if (groups == 0 || code->m == 0) return QFEC_OK;
    UpdatePtrsArgs a{};
    a.first = first;
    a.count = count;
    a.accumulate = accumulate;
    return run_update_ptrs(code, a, d_shards, groups, block_size, "encode_update_ptrs kernel launch",
                           [&](const UpdatePtrsArgs& x) { return launch_encode_update_ptrs(x, false, (hipStream_t)stream); });
}

int qfec_encode_update_ptrs_var(qfec_code* code, int first, int count, unsigned char* const* d_shards, const int* d_lens,
                                const int* d_group_len, long long groups, int max_len, int accumulate,
                                unsigned int* d_invalid, void* stream) {
    const char* why = range_cause(code, first, count);
    if (!why) why = common_cause(code, groups, max_len, "max_len < 1");
    if (!why)
        why = accumulate != 0 && accumulate != 1 ? "accumulate is not 0 or 1"
              : groups > 0 && !d_shards          ? "null d_shards"
              : groups > 0 && !d_lens            ? "null d_lens"
              : groups > 0 && !d_group_len       ? "null d_group_len"
                                                 : nullptr;
    if (why) {
        set_error("qfec_encode_update_ptrs_var: invalid argument (%s)", why);
        return QFEC_EINVAL;
    }
    if (groups == 0 || code->m == 0) return QFEC_OK;
    UpdatePtrsArgs a{};
    a.first = first;
    a.count = count;
    a.accumulate = accumulate;
    a.lens = d_lens;
    a.group_len = d_group_len;
    a.invalid = d_invalid;
    return run_update_ptrs(code, a, d_shards, groups, max_len, "encode_update_ptrs_var kernel launch",
                           [&](const UpdatePtrsArgs& x) { return launch_encode_update_ptrs(x, true, (hipStream_t)stream); });
}

int qfec_update_ptrs(qfec_code* code, unsigned char* const* d_shards, const int* d_shard,
                     const unsigned char* const* d_new, int delta_only, long long groups, int block_size,
                     unsigned int* d_invalid, void* stream) {
    const char* why = common_cause(code, groups, block_size, "block_size < 1");
    if (!why)
        why = delta_only != 0 && delta_only != 1 ? "delta_only is not 0 or 1"
              : groups > 0 && !d_shards          ? "null d_shards"
              : groups > 0 && !d_shard           ? "null d_shard"
              : groups > 0 && !d_new             ? "null d_new"
                                                 : nullptr;
    if (why) {
        set_error("qfec_update_ptrs: invalid argument (%s)", why);
        return QFEC_EINVAL;
    }
    if (groups == 0 || code->m == 0) return QFEC_OK;
    UpdatePtrsArgs a{};
    a.shard = d_shard;
    a.news = reinterpret_cast<const uint64_t*>(d_new);
    a.delta_only = delta_only;
    a.invalid = d_invalid;
    return run_update_ptrs(code, a, d_shards, groups, block_size, "update_ptrs kernel launch",
                           [&](const UpdatePtrsArgs& x) { return launch_update_ptrs(x, false, (hipStream_t)stream); });
}

int qfec_update_ptrs_var(qfec_code* code, unsigned char* const* d_shards, const int* d_lens, const int* d_group_len,
                         const int* d_shard, const unsigned char* const* d_new, const int* d_new_len, int delta_only,
                         long long groups, int max_len, unsigned int* d_invalid, void* stream) {
    const char* why = common_cause(code, groups, max_len, "max_len < 1");
    if (!why)
        why = delta_only != 0 && delta_only != 1        ? "delta_only is not 0 or 1"
              : groups > 0 && !d_shards                 ? "null d_shards"
              : groups > 0 && !d_shard                  ? "null d_shard"
              : groups > 0 && !d_new                    ? "null d_new"
              : groups > 0 && !d_lens && !delta_only    ? "null d_lens"
              : groups > 0 && !d_group_len              ? "null d_group_len"
              : groups > 0 && !d_new_len                ? "null d_new_len"
                                                        : nullptr;
    if (why) {
        set_error("qfec_update_ptrs_var: invalid argument (%s)", why);
        return QFEC_EINVAL;
    }
    if (groups == 0 || code->m == 0) return QFEC_OK;
    UpdatePtrsArgs a{};
    a.lens = d_lens;
    a.group_len = d_group_len;
    a.shard = d_shard;
    a.news = reinterpret_cast<const uint64_t*>(d_new);
    a.new_len = d_new_len;
    a.delta_only = delta_only;
    a.invalid = d_invalid;
    return run_update_ptrs(code, a, d_shards, groups, max_len, "update_ptrs_var kernel launch",
                           [&](const UpdatePtrsArgs& x) { return launch_update_ptrs(x, true, (hipStream_t)stream); });
}

}  // extern "C"
