// qfec_plan.cpp -- device-built decode plans of the device API in include/qfec.h: qfec_plan_build,
// qfec_plan_apply, the one-shot calls qfec_reconstruct_wide / qfec_repair_wide (build into
// stream-ordered scratch, then apply) and the host query qfec_plan_build_host.  The plan of a group
// is computed from its marks on the device (qfec_plan.hip) by the arithmetic of qfec_plan.hpp, so
// there is no LUT, no read-back and no k + m limit here.  Arguments are judged on the host before a
// device is touched.
#include "qfec_plan.hpp"
#include "qfec_rt.hpp"

namespace qfec {

// rs.c's decode with a partially inverted matrix is not reproduced here: a code that carries an
// rs.c decode matrix must have it equal to [I; rows].  Judged once per code version.
int plan_code_check(const qfec_code* cc, const char* who) {
    qfec_code* c = const_cast<qfec_code*>(cc);
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->plan_chk_version != c->version) {
        const int k = c->k, m = c->m;
        bool ok = true;
        if (!c->full.empty()) {
            for (int r = 0; r < k && ok; ++r)
                for (int i = 0; i < k && ok; ++i) ok = c->full[(size_t)r * k + i] == (r == i);
            ok = ok && memcmp(c->full.data() + (size_t)k * k, c->rows.data(), (size_t)m * k) == 0;
        }
        c->plan_chk_ok = ok;
        c->plan_chk_version = c->version;
    }
    if (c->plan_chk_ok) return QFEC_OK;
    set_error("%s: the code's rs.c decode matrix is not [I; rows] (edited handle): not supported by device plans", who);
    return QFEC_EUNSUP;
}

const char* bad_rows_args(const qfec_code* code, long long groups, int block_size, long long pitch) {
    return !code              ? "null code"
           : groups < 0       ? "groups < 0"
           : block_size < 1   ? "block_size < 1"
           : pitch < block_size ? "pitch < block_size"
                              : nullptr;
}

// the build kernel stores a plan 16 bytes at a time and the apply kernel reads it as dwords
bool plan_misaligned(const void* d_plan) { return ((uintptr_t)d_plan & 15) != 0; }

int refuse(const char* who, const char* why) {
    set_error("%s: invalid argument (%s)", who, why);
    return QFEC_EINVAL;
}

// the encode tables of `code` on the context's device (the build kernel reads the coefficients there)
static int enc_tables(qfec_code* code, DevCtx& ctx, uint32_t** tab) {
    std::lock_guard<std::mutex> lk(code->mu);
    return ensure_enc(code, ctx.device, tab);
}

// plans of `gn` groups whose marks start at dmarks / pmarks
int run_plan_build(DevCtx& ctx, const qfec_code* c, const uint32_t* tab, const uint8_t* dmarks, const uint8_t* pmarks,
                   long long gn, int mode, uint8_t* d_plan, unsigned* d_failed, hipStream_t s) {
    PlanBuildArgs a{};
    a.tab = tab;
    a.gf = ctx.d_gf;
    a.failed = d_failed;
    a.k = c->k;
    a.m = c->m;
    a.mode = mode;
    a.quirk = c->quirk;
    a.stride = (uint32_t)plan_layout(c->k, c->m).stride;
    a.lds = (uint32_t)(QFEC_PLAN_GF_BYTES + plan_work_bytes(c->k, c->m));
    return for_group_chunks(gn, kMaxLaunchLanes / 64, [&](long long g0, long long n) {
        a.dmarks = dmarks + (size_t)g0 * c->k;
        a.pmarks = pmarks + (size_t)g0 * c->m;
        a.plan = d_plan + (size_t)g0 * a.stride;
        a.groups = (uint64_t)n;
        const hipError_t e = launch_plan_build(a, s);
        return e == hipSuccess ? QFEC_OK : hip_fail(e, "plan_build kernel launch");
    });
}

struct ApplyGeom {
    PlanApplyArgs a;
    long long per;  // groups per launch
};

static ApplyGeom apply_geom(DevCtx& ctx, const qfec_code* c, const uint8_t* d_data, const uint8_t* d_par, int block,
                            long long pitch) {
    ApplyGeom G{};
    PlanApplyArgs& a = G.a;
    a.t256 = ctx.d_t256;
    a.k = c->k;
    a.m = c->m;
    a.pitch = (uint64_t)pitch;
    a.dgs = (uint64_t)c->k * pitch;
    a.pgs = (uint64_t)c->m * pitch;
    a.stride = (uint32_t)plan_layout(c->k, c->m).stride;
    const FlatGeom f = flat_geom(d_data, d_par, block, pitch, a.dgs, a.pgs);
    const WaveGeom w = wave_geom(f);  // whole waves per group, over 16-B columns or bytes
    a.vec16 = f.vec16;
    a.cols = w.cols;
    a.wpg = w.wpg;
    G.per = w.per;
    return G;
}

static int run_plan_apply(PlanApplyArgs& a, uint8_t* d_data, uint8_t* d_par, const uint8_t* d_plan, long long g0,
                          long long gn, hipStream_t s) {
    a.data = d_data + (size_t)g0 * a.dgs;
    a.parity = d_par + (size_t)g0 * a.pgs;
    a.plan = d_plan;
    a.groups = (uint64_t)gn;
    const hipError_t e = launch_plan_apply(a, s);
    return e == hipSuccess ? QFEC_OK : hip_fail(e, "plan_apply kernel launch");
}

// qfec_reconstruct_wide / qfec_repair_wide: per chunk, plans into stream-ordered scratch, apply, free
static int run_wide(const char* who, qfec_code* code, uint8_t* d_data, uint8_t* d_par, const uint8_t* d_marks,
                    long long groups, int block_size, long long pitch, int mode, unsigned* d_failed, hipStream_t s) {
    const char* why = bad_rows_args(code, groups, block_size, pitch);
    if (!why && groups > 0 && (!d_data || !d_marks || (code->m > 0 && !d_par))) why = "null buffer";
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    int rc = batch_begin(who, false, [&] { return plan_code_check(code, who); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    uint32_t* tab = nullptr;
    if ((rc = enc_tables(code, *ctx, &tab))) return rc;
    ApplyGeom G = apply_geom(*ctx, code, d_data, d_par, block_size, pitch);
    const long long per = std::max(1ll, std::min(G.per, kPlanScratchCap / G.a.stride));
    return for_group_chunks(groups, per, [&](long long g0, long long gn) {
        uint8_t* plan = nullptr;
        if (hipMallocAsync((void**)&plan, (size_t)gn * G.a.stride, s) != hipSuccess)
            return hip_fail(hipGetLastError(), (std::string(who) + " scratch").c_str());
        // rs.c layout: every group's data marks, then the parity marks
        int r = run_plan_build(*ctx, code, tab, d_marks + (size_t)g0 * code->k,
                               d_marks + (size_t)groups * code->k + (size_t)g0 * code->m, gn, mode, plan, d_failed, s);
        if (!r) r = run_plan_apply(G.a, d_data, d_par, plan, g0, gn, s);
        (void)hipFreeAsync(plan, s);
        return r;
    });
}

}  // namespace qfec

using namespace qfec;

extern "C" {

long long qfec_plan_stride(const qfec_code* code) {
    if (!code) {
        set_error("qfec_plan_stride: invalid argument (null code)");
        return QFEC_EINVAL;
    }
    return plan_layout(code->k, code->m).stride;
}

int qfec_plan_build_host(const qfec_code* code, const unsigned char* marks_n, int mode, unsigned char* out_plan) {
    const char* who = "qfec_plan_build_host";
    const char* why = !code                      ? "null code"
                      : mode != 0 && mode != 1   ? "mode is not 0 or 1"
                      : !marks_n || !out_plan    ? "null buffer"
                                                 : nullptr;
    if (why) return refuse(who, why);
    const int rc = plan_code_check(code, who);
    if (rc) return rc;
    const int k = code->k, m = code->m;
    uint64_t mk[4] = {0, 0, 0, 0};
    for (int i = 0; i < k + m; ++i)
        if (marks_n[i]) mk[i >> 6] |= 1ull << (i & 63);
    const Field& f = field();
    const PlanCode C{code->rows.data(), 1, k, m, code->quirk, f.exp, f.log};
    std::vector<uint8_t> work((size_t)plan_work_bytes(k, m));
    (void)plan_group(C, mk, mode, work.data(), out_plan, PlanHostLanes{});
    return QFEC_OK;
}

int qfec_plan_build(qfec_code* code, const unsigned char* d_marks, long long groups, int mode, unsigned char* d_plan,
                    unsigned int* d_failed, void* stream) {
    const char* who = "qfec_plan_build";
    const char* why = !code                                ? "null code"
                      : groups < 0                         ? "groups < 0"
                      : mode != 0 && mode != 1             ? "mode is not 0 or 1"
                      : groups > 0 && (!d_marks || !d_plan) ? "null buffer"
                      : plan_misaligned(d_plan)            ? "d_plan not 16-byte aligned"
                                                           : nullptr;
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    int rc = batch_begin(who, false, [&] { return plan_code_check(code, who); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    uint32_t* tab = nullptr;
    if ((rc = enc_tables(code, *ctx, &tab))) return rc;
    return run_plan_build(*ctx, code, tab, d_marks, d_marks + (size_t)groups * code->k, groups, mode, d_plan, d_failed,
                          (hipStream_t)stream);
}

int qfec_plan_apply(qfec_code* code, unsigned char* d_data, unsigned char* d_parity, const unsigned char* d_plan,
                    long long groups, int block_size, long long pitch, void* stream) {
    const char* who = "qfec_plan_apply";
    const char* why = bad_rows_args(code, groups, block_size, pitch);
    if (!why && groups > 0 && (!d_data || !d_plan || (code->m > 0 && !d_parity))) why = "null buffer";
    if (!why && plan_misaligned(d_plan)) why = "d_plan not 16-byte aligned";
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(who, false, [&] { return plan_code_check(code, who); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    ApplyGeom G = apply_geom(*ctx, code, d_data, d_parity, block_size, pitch);
    return for_group_chunks(groups, G.per, [&](long long g0, long long gn) {
        return run_plan_apply(G.a, d_data, d_parity, d_plan + (size_t)g0 * G.a.stride, g0, gn, (hipStream_t)stream);
    });
}

int qfec_reconstruct_wide(qfec_code* code, unsigned char* d_data, const unsigned char* d_parity,
                          const unsigned char* d_marks, long long groups, int block_size, long long pitch,
                          unsigned int* d_failed, void* stream) {
    // a RECONSTRUCT plan lists no parity row, so the parity is only read
    return run_wide("qfec_reconstruct_wide", code, d_data, const_cast<unsigned char*>(d_parity), d_marks, groups,
                    block_size, pitch, QFEC_PLAN_RECONSTRUCT, d_failed, (hipStream_t)stream);
}

int qfec_repair_wide(qfec_code* code, unsigned char* d_data, unsigned char* d_parity, const unsigned char* d_marks,
                     long long groups, int block_size, long long pitch, unsigned int* d_failed, void* stream) {
    return run_wide("qfec_repair_wide", code, d_data, d_parity, d_marks, groups, block_size, pitch, QFEC_PLAN_REPAIR,
                    d_failed, (hipStream_t)stream);
}

}  // extern "C"
