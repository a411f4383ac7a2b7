// qfec_integrity_ptrs_var.cpp -- the integrity family on pointer tables with per-shard lengths of
// include/qfec.h: qfec_verify_ptrs_var, qfec_locate_ptrs_var (kernels: qfec_integrity_ptrs_var.hip,
// k_locate_finish, k_var_invalid) and qfec_scrub_ptrs_var (locate, then k_correct_ptrs_var: one
// located shard is fixed from one parity row, so no plan is built).  Table as in
// qfec_integrity_ptrs.cpp; d_lens holds a length per data shard in table order, d_group_len one per
// group, so a launch over groups [g0, g0 + gn) is handed d_lens + g0 * k and d_group_len + g0.
// max_len only sizes the launch.  Arguments and codes are judged on the host before a device is
// touched; nothing is read back.
#include "qfec_rt.hpp"

namespace qfec {

static const char* bad_var_args(const qfec_code* code, unsigned char* const* d_shards, const int* d_lens,
                                const int* d_group_len, long long groups, int max_len) {
    return !code                        ? "null code"
           : groups < 0                 ? "groups < 0"
           : max_len < 1                ? "max_len < 1"
           : groups > 0 && !d_shards    ? "null d_shards"
           : groups > 0 && !d_lens      ? "null d_lens"
           : groups > 0 && !d_group_len ? "null d_group_len"
                                        : nullptr;
}

// what a call's launches share: the table's two halves, the lengths, the geometry of max_len
struct VarBatch {
    const qfec_code* c;
    const uint64_t *dptrs, *pptrs;
    const int32_t *lens, *glen;
    long long groups;
    int max_len;
};

// cuts the batch into launches; launch(a, g0) sees the chunk's parts of the table, the lengths and the words
template <class Launch>
static int var_chunks(IntegrityPtrsVarArgs a, const VarBatch& b, unsigned* rows, unsigned* cand, const char* what,
                      Launch&& launch) {
    const PtrsGeom p = ptrs_geom(b.max_len, 16);
    a.p.k = b.c->k;
    a.p.m = b.c->m;
    a.p.block = (uint32_t)b.max_len;
    a.p.vcols = p.vcols;
    a.p.wpg = p.wpg;
    a.p.tail0 = p.tail0;
    a.p.tailn = p.tailn;
    return for_group_chunks(b.groups, p.per, [&](long long g0, long long gn) {
        a.p.dptrs = b.dptrs + (size_t)g0 * a.p.k;
        a.p.pptrs = b.pptrs + (size_t)g0 * a.p.m;
        a.p.bad_rows = rows ? rows + g0 : nullptr;
        a.p.cand = cand ? cand + g0 : nullptr;
        a.lens = b.lens + (size_t)g0 * a.p.k;
        a.group_len = b.glen + g0;
        a.p.groups = (uint64_t)gn;
        const hipError_t he = launch(a, g0);
        return he == hipSuccess ? QFEC_OK : hip_fail(he, what);
    });
}

// the groups refused for their lengths: QFEC_LOC_INVALID (culprit nullable) and the counter (nullable)
static int run_var_invalid(const VarBatch& b, int* d_culprit, unsigned* d_invalid, hipStream_t s, const char* what) {
    VarInvalidArgs v{};
    v.lens = b.lens;
    v.group_len = b.glen;
    v.culprit = d_culprit;
    v.invalid = d_invalid;
    v.groups = (uint64_t)b.groups;
    v.max_len = (uint32_t)b.max_len;
    v.k = b.c->k;
    const hipError_t he = launch_var_invalid(v, s);
    return he == hipSuccess ? QFEC_OK : hip_fail(he, what);
}

// the launches of one qfec_locate_ptrs_var (validated arguments): run_locate_ptrs' with lengths, then
// the invalid groups' verdicts over the finish's
int run_locate_ptrs_var(DevCtx& ctx, qfec_code* code, const uint64_t* dptrs, const uint64_t* pptrs, const int32_t* lens,
                        const int32_t* glen, long long groups, int max_len, int* d_culprit, uint8_t* d_marks,
                        unsigned* d_counts, unsigned* d_invalid, hipStream_t s) {
    uint32_t *tab = nullptr, *rtab = nullptr;
    int rc;
    {
        std::lock_guard<std::mutex> lk(code->mu);
        rc = ensure_enc(code, ctx.device, &tab);
        if (!rc) rc = ensure_loc(code, ctx.device, &rtab);
    }
    if (rc) return rc;
    GroupWords words(s);  // [groups] bad rows, then [groups] candidates
    rc = words.init("locate_ptrs_var", groups, 2);
    if (rc) return rc;
    IntegrityPtrsVarArgs a{};
    a.p.tab = tab;
    a.p.rtab = rtab;
    const VarBatch b{code, dptrs, pptrs, lens, glen, groups, max_len};
    rc = var_chunks(a, b, words.at(0), words.at(1), "locate_ptrs_var kernel launch",
                    [&](const IntegrityPtrsVarArgs& x, long long) { return launch_locate_ptrs_var(x, s); });
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
    if (he != hipSuccess) return hip_fail(he, "locate_ptrs_var finish kernel launch");
    return run_var_invalid(b, d_culprit, d_invalid, s, "locate_ptrs_var invalid-group kernel launch");
}

}  // namespace qfec

using namespace qfec;

extern "C" {

int qfec_verify_ptrs_var(qfec_code* code, unsigned char* const* d_shards, const int* d_lens, const int* d_group_len,
                         long long groups, int max_len, unsigned int* d_bad_rows, unsigned int* d_bad_groups,
                         unsigned int* d_invalid, void* stream) {
    const char* who = "qfec_verify_ptrs_var";
    const char* why = bad_var_args(code, d_shards, d_lens, d_group_len, groups, max_len);
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    int rc = batch_begin(
        who, false,
        [&] {
            if (code->m <= 32) return QFEC_OK;
            set_error("qfec_verify_ptrs_var: m = %d > 32 (one bit per parity row in a 32-bit word)", code->m);
            return QFEC_EUNSUP;
        },
        groups == 0 || (!d_bad_rows && !d_bad_groups && !d_invalid), &ctx);
    if (rc || !ctx) return rc;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t* t = reinterpret_cast<const uint64_t*>(d_shards);
    const VarBatch b{code, t, t + (size_t)groups * code->k, d_lens, d_group_len, groups, max_len};
    // as qfec_verify_ptrs: the per-group words also decide which OR counts a group
    GroupWords words(s);
    if (d_bad_rows || d_bad_groups) rc = words.init("verify_ptrs_var", groups, 1, d_bad_rows);
    if (rc) return rc;
    if (code->m > 0 && (d_bad_rows || d_bad_groups)) {
        uint32_t* tab = nullptr;
        {
            std::lock_guard<std::mutex> lk(code->mu);
            rc = ensure_enc(code, ctx->device, &tab);
        }
        if (rc) return rc;
        IntegrityPtrsVarArgs a{};
        a.p.tab = tab;
        a.p.bad_groups = d_bad_groups;
        rc = var_chunks(a, b, words.at(0), nullptr, "verify_ptrs_var kernel launch",
                        [&](const IntegrityPtrsVarArgs& x, long long) { return launch_verify_ptrs_var(x, s); });
        if (rc) return rc;
    }
    return run_var_invalid(b, nullptr, d_invalid, s, "verify_ptrs_var invalid-group kernel launch");
}

int qfec_locate_ptrs_var(qfec_code* code, unsigned char* const* d_shards, const int* d_lens, const int* d_group_len,
                         long long groups, int max_len, int* d_culprit, unsigned char* d_marks, unsigned int* d_counts,
                         unsigned int* d_invalid, void* stream) {
    const char* who = "qfec_locate_ptrs_var";
    const char* why = bad_var_args(code, d_shards, d_lens, d_group_len, groups, max_len);
    if (!why && groups > 0 && !d_culprit) why = "null d_culprit";
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(who, false, [&] { return locate_code_check(code, who, false); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    const uint64_t* t = reinterpret_cast<const uint64_t*>(d_shards);
    return run_locate_ptrs_var(*ctx, code, t, t + (size_t)groups * code->k, d_lens, d_group_len, groups, max_len, d_culprit,
                               d_marks, d_counts, d_invalid, (hipStream_t)stream);
}

int qfec_scrub_ptrs_var(qfec_code* code, unsigned char* const* d_shards, const int* d_lens, const int* d_group_len,
                        long long groups, int max_len, int* d_culprit, unsigned int* d_counts, unsigned int* d_invalid,
                        void* stream) {
    const char* who = "qfec_scrub_ptrs_var";
    const char* why = bad_var_args(code, d_shards, d_lens, d_group_len, groups, max_len);
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    // the locate's limits alone: the correction uses only the parity rows the locate judged with
    int rc = batch_begin(who, false, [&] { return locate_code_check(code, who, false); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    hipStream_t s = (hipStream_t)stream;
    int* verdicts = d_culprit;  // stream-ordered scratch when the caller does not want them
    if (!verdicts && hipMallocAsync((void**)&verdicts, (size_t)groups * sizeof(int), s) != hipSuccess)
        return hip_fail(hipGetLastError(), "scrub_ptrs_var scratch");
    const uint64_t* t = reinterpret_cast<const uint64_t*>(d_shards);
    const VarBatch b{code, t, t + (size_t)groups * code->k, d_lens, d_group_len, groups, max_len};
    rc = run_locate_ptrs_var(*ctx, code, b.dptrs, b.pptrs, d_lens, d_group_len, groups, max_len, verdicts, nullptr, d_counts,
                             d_invalid, s);
    if (!rc) {
        uint32_t* tab = nullptr;
        {
            std::lock_guard<std::mutex> lk(code->mu);
            rc = ensure_enc(code, ctx->device, &tab);
        }
        if (!rc) {
            IntegrityPtrsVarArgs a{};
            a.p.tab = tab;
            rc = var_chunks(a, b, nullptr, nullptr, "scrub_ptrs_var correction kernel launch",
                            [&](const IntegrityPtrsVarArgs& x, long long g0) {
                                return launch_correct_ptrs_var(x, verdicts + g0, ctx->d_t256, ctx->d_gf, s);
                            });
        }
    }
    if (!d_culprit) (void)hipFreeAsync(verdicts, s);
    return rc;
}

}  // extern "C"
