// qfec_integrity_ptrs.cpp -- the integrity family on pointer tables of the device API in include/qfec.h:
// qfec_verify_ptrs, qfec_locate_ptrs (kernels: qfec_integrity_ptrs.hip, k_locate_finish) and
// qfec_scrub_ptrs (locate, then the repair of qfec_repair_ptrs_wide with the marks it wrote).  The table
// is qfec_encode_ptrs' (qfec_ptrs.cpp): every group's data shards, then every group's parity shards,
// so a launch over groups [g0, g0 + gn) is handed the two halves from g0 on and its groups' words.
// Arguments and codes are judged on the host before a device is touched; nothing is read back.
#include "qfec_rt.hpp"

namespace qfec {

const char* bad_table_args(const qfec_code* code, unsigned char* const* d_shards, long long groups, int block_size) {
    return !code                     ? "null code"
           : groups < 0              ? "groups < 0"
           : block_size < 1          ? "block_size < 1"
           : groups > 0 && !d_shards ? "null d_shards"
                                     : nullptr;
}

// cuts the batch into launches; launch(a) sees the chunk's halves of the table and its group words
template <class Launch>
static int integrity_chunks(IntegrityPtrsArgs& a, const qfec_code* c, const uint64_t* dptrs, const uint64_t* pptrs,
                            unsigned* rows, unsigned* cand, long long groups, int block, const char* what,
                            Launch&& launch) {
    const PtrsGeom p = ptrs_geom(block, ptrs_lane_bytes(false, c->k));
    a.k = c->k;
    a.m = c->m;
    a.block = (uint32_t)block;
    a.vcols = p.vcols;
    a.wpg = p.wpg;
    a.tail0 = p.tail0;
    a.tailn = p.tailn;
    return for_group_chunks(groups, p.per, [&](long long g0, long long gn) {
        a.dptrs = dptrs + (size_t)g0 * a.k;
        a.pptrs = pptrs + (size_t)g0 * a.m;
        a.bad_rows = rows + g0;
        a.cand = cand ? cand + g0 : nullptr;
        a.groups = (uint64_t)gn;
        const hipError_t he = launch(a);
        return he == hipSuccess ? QFEC_OK : hip_fail(he, what);
    });
}

// the launches of one qfec_locate_ptrs (validated arguments): run_locate's, on the table
int run_locate_ptrs(DevCtx& ctx, qfec_code* code, const uint64_t* dptrs, const uint64_t* pptrs, long long groups,
                    int block_size, int* d_culprit, uint8_t* d_marks, unsigned* d_counts, hipStream_t s) {
    uint32_t *tab = nullptr, *rtab = nullptr;
    int rc;
    {
        std::lock_guard<std::mutex> lk(code->mu);
        rc = ensure_enc(code, ctx.device, &tab);
        if (!rc) rc = ensure_loc(code, ctx.device, &rtab);
    }
    if (rc) return rc;
    GroupWords words(s);  // [groups] bad rows, then [groups] candidates
    rc = words.init("locate_ptrs", groups, 2);
    if (rc) return rc;
    IntegrityPtrsArgs a{};
    a.tab = tab;
    a.rtab = rtab;
    rc = integrity_chunks(a, code, dptrs, pptrs, words.at(0), words.at(1), groups, block_size,
                          "locate_ptrs kernel launch", [&](const IntegrityPtrsArgs& x) { return launch_locate_ptrs(x, s); });
    if (rc) return rc;
    LocateFinishArgs f{};
    f.bad_rows = words.at(0);
    f.cand = words.at(1);
    f.culprit = d_culprit;
    f.marks = d_marks;
    f.counts = d_counts;
    f.groups = (uint64_t)groups;
    f.k = code->k;
    f.m = code->m;
    const hipError_t he = launch_locate_finish(f, s);
    return he == hipSuccess ? QFEC_OK : hip_fail(he, "locate_ptrs finish kernel launch");
}

}  // namespace qfec

using namespace qfec;

extern "C" {

int qfec_verify_ptrs(qfec_code* code, unsigned char* const* d_shards, long long groups, int block_size,
                     unsigned int* d_bad_rows, unsigned int* d_bad_groups, void* stream) {
    const char* who = "qfec_verify_ptrs";
    const char* why = bad_table_args(code, d_shards, groups, block_size);
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    int rc = batch_begin(
        who, false,
        [&] {
            if (code->m <= 32) return QFEC_OK;
            set_error("qfec_verify_ptrs: m = %d > 32 (one bit per parity row in a 32-bit word)", code->m);
            return QFEC_EUNSUP;
        },
        groups == 0 || (!d_bad_rows && !d_bad_groups), &ctx);
    if (rc || !ctx) return rc;
    hipStream_t s = (hipStream_t)stream;
    // as qfec_verify: the per-group words also decide which OR counts a group, so a call that only
    // wants the counter gets them from stream-ordered scratch
    GroupWords words(s);
    rc = words.init("verify_ptrs", groups, 1, d_bad_rows);
    if (rc || code->m == 0) return rc;
    uint32_t* tab = nullptr;
    {
        std::lock_guard<std::mutex> lk(code->mu);
        rc = ensure_enc(code, ctx->device, &tab);
    }
    if (rc) return rc;
    IntegrityPtrsArgs a{};
    a.tab = tab;
    a.bad_groups = d_bad_groups;
    const uint64_t* t = reinterpret_cast<const uint64_t*>(d_shards);
    return integrity_chunks(a, code, t, t + (size_t)groups * code->k, words.at(0), nullptr, groups, block_size,
                            "verify_ptrs kernel launch", [&](const IntegrityPtrsArgs& x) { return launch_verify_ptrs(x, s); });
}

int qfec_locate_ptrs(qfec_code* code, unsigned char* const* d_shards, long long groups, int block_size, int* d_culprit,
                     unsigned char* d_marks, unsigned int* d_counts, void* stream) {
    const char* who = "qfec_locate_ptrs";
    const char* why = bad_table_args(code, d_shards, groups, block_size);
    if (!why && groups > 0 && !d_culprit) why = "null d_culprit";
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(who, false, [&] { return locate_code_check(code, who, false); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    const uint64_t* t = reinterpret_cast<const uint64_t*>(d_shards);
    return run_locate_ptrs(*ctx, code, t, t + (size_t)groups * code->k, groups, block_size, d_culprit, d_marks, d_counts,
                           (hipStream_t)stream);
}

int qfec_scrub_ptrs(qfec_code* code, unsigned char* const* d_shards, long long groups, int block_size, int* d_culprit,
                    unsigned int* d_counts, unsigned int* d_failed, void* stream) {
    const char* who = "qfec_scrub_ptrs";
    const char* why = bad_table_args(code, d_shards, groups, block_size);
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    int rc = batch_begin(
        who, false,
        [&] {
            const int r = locate_code_check(code, who, false);
            return r ? r : plan_code_check(code, who);  // both halves' limits, before anything is launched
        },
        groups == 0, &ctx);
    if (rc || !ctx) return rc;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* tab = nullptr;
    {
        std::lock_guard<std::mutex> lk(code->mu);
        rc = ensure_enc(code, ctx->device, &tab);
    }
    if (rc) return rc;
    // the marks, and the verdicts too when the caller does not want them, live in stream-ordered scratch
    const size_t nk = (size_t)groups * (size_t)code->k;
    const size_t mark_bytes = round_up(nk + (size_t)groups * (size_t)code->m, 16);
    uint8_t* scratch = nullptr;
    if (hipMallocAsync((void**)&scratch, mark_bytes + (d_culprit ? 0 : (size_t)groups * 4), s) != hipSuccess)
        return hip_fail(hipGetLastError(), "scrub_ptrs scratch");
    const uint64_t* t = reinterpret_cast<const uint64_t*>(d_shards);
    rc = run_locate_ptrs(*ctx, code, t, t + nk, groups, block_size, d_culprit ? d_culprit : (int*)(scratch + mark_bytes),
                         scratch, d_counts, s);
    // qfec_repair_ptrs_wide's path: plans built on the device from the marks, applied to the table
    if (!rc) rc = run_wide_ptrs(*ctx, code, tab, t, t + nk, scratch, scratch + nk, groups, block_size, QFEC_PLAN_REPAIR,
                                d_failed, s, who);
    (void)hipFreeAsync(scratch, s);
    return rc;
}

}  // extern "C"
