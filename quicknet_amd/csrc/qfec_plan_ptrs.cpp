// qfec_plan_ptrs.cpp -- device plans on pointer tables (include/qfec.h): qfec_plan_apply_ptrs and the
// one-shot calls qfec_reconstruct_ptrs_wide / qfec_repair_ptrs_wide; the three calls with per-shard
// lengths, qfec_plan_apply_ptrs_var / qfec_reconstruct_ptrs_wide_var / qfec_repair_ptrs_wide_var, whose
// launches are handed d_lens + g0 * k and d_group_len + g0 as well.  The plans are those of
// qfec_plan.cpp (run_plan_build: they depend on the marks alone); the rows are where a device table
// in module/rs.h's shard order says (qfec_ptrs.cpp), so a launch over groups [g0, g0 + gn) is handed
// the two halves of the table, of the marks and the plans from g0 on.  Any k + m; arguments are
// judged on the host before a device is touched; nothing is read back.
#include "qfec_plan.hpp"
#include "qfec_rt.hpp"

namespace qfec {

int run_plan_apply_ptrs(DevCtx& ctx, const qfec_code* c, const uint64_t* dptrs, const uint64_t* pptrs,
                        const uint8_t* d_plan, long long gn, int block, hipStream_t s) {
    PlanPtrsArgs a{};
    const PtrsGeom p = ptrs_geom(block, 16);
    a.t256 = ctx.d_t256;
    a.k = c->k;
    a.m = c->m;
    a.block = (uint32_t)block;
    a.stride = (uint32_t)plan_layout(c->k, c->m).stride;
    a.vcols = p.vcols;
    a.wpg = p.wpg;
    a.tail0 = p.tail0;
    a.tailn = p.tailn;
    return for_group_chunks(gn, p.per, [&](long long g0, long long n) {
        a.dptrs = dptrs + (size_t)g0 * a.k;
        a.pptrs = pptrs + (size_t)g0 * a.m;
        a.plan = d_plan + (size_t)g0 * a.stride;
        a.groups = (uint64_t)n;
        const hipError_t e = launch_plan_apply_ptrs(a, s);
        return e == hipSuccess ? QFEC_OK : hip_fail(e, "plan_apply_ptrs kernel launch");
    });
}

// build into stream-ordered scratch, apply(g0, n, plan), free: chunks of at most kPlanScratchCap of plans
template <class Apply>
static int wide_chunks(DevCtx& ctx, const qfec_code* c, const uint32_t* tab, const uint8_t* dmarks, const uint8_t* pmarks,
                       long long gn, int block, int mode, unsigned* d_failed, hipStream_t s, const char* who,
                       Apply&& apply) {
    const long long stride = plan_layout(c->k, c->m).stride;
    const long long per = std::max(1ll, std::min(ptrs_geom(block, 16).per, kPlanScratchCap / stride));
    return for_group_chunks(gn, per, [&](long long g0, long long n) {
        uint8_t* plan = nullptr;
        if (hipMallocAsync((void**)&plan, (size_t)n * stride, s) != hipSuccess)
            return hip_fail(hipGetLastError(), (std::string(who) + " scratch").c_str());
        int r = run_plan_build(ctx, c, tab, dmarks + (size_t)g0 * c->k, pmarks + (size_t)g0 * c->m, n, mode, plan,
                               d_failed, s);
        if (!r) r = apply(g0, n, plan);
        (void)hipFreeAsync(plan, s);
        return r;
    });
}

int run_wide_ptrs(DevCtx& ctx, const qfec_code* c, const uint32_t* tab, const uint64_t* dptrs, const uint64_t* pptrs,
                  const uint8_t* dmarks, const uint8_t* pmarks, long long gn, int block, int mode, unsigned* d_failed,
                  hipStream_t s, const char* who) {
    return wide_chunks(ctx, c, tab, dmarks, pmarks, gn, block, mode, d_failed, s, who,
                       [&](long long g0, long long n, const uint8_t* plan) {
                           return run_plan_apply_ptrs(ctx, c, dptrs + (size_t)g0 * c->k, pptrs + (size_t)g0 * c->m, plan, n,
                                                      block, s);
                       });
}

// the same with per-shard lengths: lens / glen are the chunk's parts of d_lens and d_group_len.  culprit
// (the scrub's repair; else NULL): [gn], a data id there is written up to its own length only
int run_plan_apply_ptrs_var(DevCtx& ctx, const qfec_code* c, const uint64_t* dptrs, const uint64_t* pptrs,
                            const int32_t* lens, const int32_t* glen, const uint8_t* d_plan, long long gn, int max_len,
                            unsigned* d_invalid, hipStream_t s, const int32_t* culprit) {
    PlanPtrsVarArgs a{};
    const PtrsGeom p = ptrs_geom(max_len, 16);
    a.p.t256 = ctx.d_t256;
    a.p.k = c->k;
    a.p.m = c->m;
    a.p.block = (uint32_t)max_len;
    a.p.stride = (uint32_t)plan_layout(c->k, c->m).stride;
    a.p.vcols = p.vcols;
    a.p.wpg = p.wpg;
    a.p.tail0 = p.tail0;
    a.p.tailn = p.tailn;
    a.invalid = d_invalid;
    return for_group_chunks(gn, p.per, [&](long long g0, long long n) {
        a.p.dptrs = dptrs + (size_t)g0 * a.p.k;
        a.p.pptrs = pptrs + (size_t)g0 * a.p.m;
        a.p.plan = d_plan + (size_t)g0 * a.p.stride;
        a.lens = lens + (size_t)g0 * a.p.k;
        a.group_len = glen + g0;
        a.p.groups = (uint64_t)n;
        const hipError_t e = culprit ? launch_plan_apply_ptrs_var_clip(a, culprit + g0, s) : launch_plan_apply_ptrs_var(a, s);
        return e == hipSuccess ? QFEC_OK : hip_fail(e, "plan_apply_ptrs_var kernel launch");
    });
}

static int run_wide_ptrs_var(DevCtx& ctx, const qfec_code* c, const uint32_t* tab, const uint64_t* dptrs,
                             const uint64_t* pptrs, const int32_t* lens, const int32_t* glen, const uint8_t* dmarks,
                             const uint8_t* pmarks, long long gn, int max_len, int mode, unsigned* d_failed,
                             unsigned* d_invalid, hipStream_t s, const char* who, const int32_t* culprit = nullptr) {
    return wide_chunks(ctx, c, tab, dmarks, pmarks, gn, max_len, mode, d_failed, s, who,
                       [&](long long g0, long long n, const uint8_t* plan) {
                           return run_plan_apply_ptrs_var(ctx, c, dptrs + (size_t)g0 * c->k, pptrs + (size_t)g0 * c->m,
                                                          lens + (size_t)g0 * c->k, glen + g0, plan, n, max_len, d_invalid, s,
                                                          culprit ? culprit + g0 : nullptr);
                       });
}

// qfec_scrub_ptrs_wide_var's repair: qfec_repair_ptrs_wide_var on the locate's marks (rs.c layout over
// `groups`), the located data shard of a group written up to its own length only, the lengths not
// counted (the locate judged them)
int run_repair_ptrs_wide_var_clip(DevCtx& ctx, qfec_code* c, const uint64_t* t, const int32_t* lens, const int32_t* glen,
                                  const uint8_t* marks, const int32_t* culprit, long long groups, int max_len,
                                  unsigned* d_failed, hipStream_t s, const char* who) {
    uint32_t* tab = nullptr;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        const int rc = ensure_enc(c, ctx.device, &tab);
        if (rc) return rc;
    }
    return run_wide_ptrs_var(ctx, c, tab, t, t + (size_t)groups * c->k, lens, glen, marks, marks + (size_t)groups * c->k,
                             groups, max_len, QFEC_PLAN_REPAIR, d_failed, nullptr, s, who, culprit);
}

static const char* bad_ptrs_args(const qfec_code* code, long long groups, int block_size) {
    return !code ? "null code" : groups < 0 ? "groups < 0" : block_size < 1 ? "block_size < 1" : nullptr;
}

// what the one-shots do once their arguments passed: the code check, the device (*ctx stays null when
// groups == 0: nothing to do), the code's encode tables on it
static int one_shot_begin(const char* who, qfec_code* code, long long groups, DevCtx** ctx, uint32_t** tab) {
    int rc = batch_begin(who, false, [&] { return plan_code_check(code, who); }, groups == 0, ctx);
    if (rc || !*ctx) return rc;
    std::lock_guard<std::mutex> lk(code->mu);
    return ensure_enc(code, (*ctx)->device, tab);
}

static int one_shot(const char* who, qfec_code* code, unsigned char* const* d_shards, const unsigned char* d_marks,
                    long long groups, int block_size, int mode, unsigned* d_failed, hipStream_t s) {
    const char* why = bad_ptrs_args(code, groups, block_size);
    if (!why && groups > 0) why = !d_shards ? "null d_shards" : !d_marks ? "null d_marks" : nullptr;
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    uint32_t* tab = nullptr;
    const int rc = one_shot_begin(who, code, groups, &ctx, &tab);
    if (rc || !ctx) return rc;
    const uint64_t* t = reinterpret_cast<const uint64_t*>(d_shards);
    // rs.c layout, table and marks alike: every group's data entries, then the parity entries
    return run_wide_ptrs(*ctx, code, tab, t, t + (size_t)groups * code->k, d_marks, d_marks + (size_t)groups * code->k,
                         groups, block_size, mode, d_failed, s, who);
}

static const char* bad_ptrs_var_args(const qfec_code* code, const void* d_shards, const int* d_lens,
                                     const int* d_group_len, long long groups, int max_len) {
    return !code                        ? "null code"
           : groups < 0                 ? "groups < 0"
           : max_len < 1                ? "max_len < 1"
           : groups > 0 && !d_shards    ? "null d_shards"
           : groups > 0 && !d_lens      ? "null d_lens"
           : groups > 0 && !d_group_len ? "null d_group_len"
                                        : nullptr;
}

static int one_shot_var(const char* who, qfec_code* code, unsigned char* const* d_shards, const int* d_lens,
                        const int* d_group_len, const unsigned char* d_marks, long long groups, int max_len, int mode,
                        unsigned* d_failed, unsigned* d_invalid, hipStream_t s) {
    const char* why = bad_ptrs_var_args(code, d_shards, d_lens, d_group_len, groups, max_len);
    if (!why && groups > 0 && !d_marks) why = "null d_marks";
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    uint32_t* tab = nullptr;
    const int rc = one_shot_begin(who, code, groups, &ctx, &tab);
    if (rc || !ctx) return rc;
    const uint64_t* t = reinterpret_cast<const uint64_t*>(d_shards);
    return run_wide_ptrs_var(*ctx, code, tab, t, t + (size_t)groups * code->k, d_lens, d_group_len, d_marks,
                             d_marks + (size_t)groups * code->k, groups, max_len, mode, d_failed, d_invalid, s, who);
}

}  // namespace qfec

using namespace qfec;

extern "C" {

int qfec_plan_apply_ptrs(qfec_code* code, unsigned char* const* d_shards, const unsigned char* d_plan, long long groups,
                         int block_size, void* stream) {
    const char* who = "qfec_plan_apply_ptrs";
    const char* why = bad_ptrs_args(code, groups, block_size);
    if (!why && groups > 0) why = !d_shards ? "null d_shards" : !d_plan ? "null d_plan" : nullptr;
    if (!why && plan_misaligned(d_plan)) why = "d_plan not 16-byte aligned";
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(who, false, [&] { return plan_code_check(code, who); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    const uint64_t* t = reinterpret_cast<const uint64_t*>(d_shards);
    return run_plan_apply_ptrs(*ctx, code, t, t + (size_t)groups * code->k, d_plan, groups, block_size,
                               (hipStream_t)stream);
}

int qfec_reconstruct_ptrs_wide(qfec_code* code, unsigned char* const* d_shards, const unsigned char* d_marks,
                               long long groups, int block_size, unsigned int* d_failed, void* stream) {
    return one_shot("qfec_reconstruct_ptrs_wide", code, d_shards, d_marks, groups, block_size, QFEC_PLAN_RECONSTRUCT,
                    d_failed, (hipStream_t)stream);
}

int qfec_repair_ptrs_wide(qfec_code* code, unsigned char* const* d_shards, const unsigned char* d_marks,
                          long long groups, int block_size, unsigned int* d_failed, void* stream) {
    return one_shot("qfec_repair_ptrs_wide", code, d_shards, d_marks, groups, block_size, QFEC_PLAN_REPAIR, d_failed,
                    (hipStream_t)stream);
}

int qfec_plan_apply_ptrs_var(qfec_code* code, unsigned char* const* d_shards, const int* d_lens, const int* d_group_len,
                             const unsigned char* d_plan, long long groups, int max_len, unsigned int* d_invalid,
                             void* stream) {
    const char* who = "qfec_plan_apply_ptrs_var";
    const char* why = bad_ptrs_var_args(code, d_shards, d_lens, d_group_len, groups, max_len);
    if (!why && groups > 0 && !d_plan) why = "null d_plan";
    if (!why && plan_misaligned(d_plan)) why = "d_plan not 16-byte aligned";
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(who, false, [&] { return plan_code_check(code, who); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    const uint64_t* t = reinterpret_cast<const uint64_t*>(d_shards);
    return run_plan_apply_ptrs_var(*ctx, code, t, t + (size_t)groups * code->k, d_lens, d_group_len, d_plan, groups,
                                   max_len, d_invalid, (hipStream_t)stream);
}

int qfec_reconstruct_ptrs_wide_var(qfec_code* code, unsigned char* const* d_shards, const int* d_lens,
                                   const int* d_group_len, const unsigned char* d_marks, long long groups, int max_len,
                                   unsigned int* d_failed, unsigned int* d_invalid, void* stream) {
    return one_shot_var("qfec_reconstruct_ptrs_wide_var", code, d_shards, d_lens, d_group_len, d_marks, groups, max_len,
                        QFEC_PLAN_RECONSTRUCT, d_failed, d_invalid, (hipStream_t)stream);
}

int qfec_repair_ptrs_wide_var(qfec_code* code, unsigned char* const* d_shards, const int* d_lens, const int* d_group_len,
                              const unsigned char* d_marks, long long groups, int max_len, unsigned int* d_failed,
                              unsigned int* d_invalid, void* stream) {
    return one_shot_var("qfec_repair_ptrs_wide_var", code, d_shards, d_lens, d_group_len, d_marks, groups, max_len,
                        QFEC_PLAN_REPAIR, d_failed, d_invalid, (hipStream_t)stream);
}

}  // extern "C"
