// qfec_check.cpp -- single-shard error location at any k + m of the device API in include/qfec.h:
// qfec_check_build, qfec_check_apply, the one-shot calls qfec_locate_wide (build into stream-ordered
// scratch, then apply) and qfec_scrub_wide (locate into scratch marks, then qfec_repair_wide), and
// the host query qfec_check_build_host; and the same on a table of shard addresses: qfec_check_apply_ptrs,
// qfec_locate_ptrs_wide and qfec_scrub_ptrs_wide (then qfec_repair_ptrs_wide); and with a length per shard:
// qfec_check_apply_ptrs_var, qfec_locate_ptrs_wide_var and qfec_scrub_ptrs_wide_var (then the repair of
// qfec_repair_ptrs_wide_var with the located shard written up to its own length).
// The check plan of a group is computed from its marks on the device (qfec_check.hip) by the arithmetic of qfec_plan.hpp: no LUT, no record per mask, no
// read-back and no k + m limit.  Arguments and the code are judged on the host before a device is
// touched.
#include "qfec_plan.hpp"
#include "qfec_rt.hpp"

namespace qfec {

// one chunk's check plans in the one-shot calls stay under this many bytes of stream-ordered scratch
constexpr long long kCheckScratchCap = 64ll << 20;

// That every punctured code is MDS cannot be checked by enumeration at these widths, so the rows
// must be the generated ones, which are.  Judged once per code version.
static int check_code_check(const qfec_code* cc, const char* who) {
    qfec_code* c = const_cast<qfec_code*>(cc);
    int rc = plan_code_check(cc, who);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->check_chk_version != c->version) {
        const int k = c->k, m = c->m;
        char why[240];
        c->check_chk_rc = QFEC_OK;
        c->check_chk_error.clear();
        if (m < 2) {
            snprintf(why, sizeof why, "m = %d < 2 (one parity row detects an error but cannot tell which shard holds it)", m);
            c->check_chk_rc = QFEC_EUNSUP;
        } else {
            std::vector<uint8_t> gen;
            const bool cauchy = cauchy_rows(k, m, gen) && gen == c->rows;
            const bool vander = !cauchy && vandermonde_rows(k, m, gen) && gen == c->rows;
            if (!cauchy && !vander) {
                snprintf(why, sizeof why,
                         "the parity rows are not those qfec_code_new generates for k = %d, m = %d (Cauchy or Vandermonde): "
                         "only generated codes are known to be MDS under every puncturing", k, m);
                c->check_chk_rc = QFEC_EUNSUP;
            }
        }
        if (c->check_chk_rc) c->check_chk_error = why;
        c->check_chk_version = c->version;
    }
    if (c->check_chk_rc) set_error("%s: %s", who, c->check_chk_error.c_str());
    return c->check_chk_rc;
}

// check plans of `gn` groups whose marks start at dmarks / pmarks (both NULL: nothing marked)
static int run_check_build(DevCtx& ctx, qfec_code* c, const uint8_t* dmarks, const uint8_t* pmarks, long long gn,
                           uint8_t* d_check, hipStream_t s) {
    uint32_t* tab = nullptr;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        const int rc = ensure_enc(c, ctx.device, &tab);
        if (rc) return rc;
    }
    PlanBuildArgs a{};
    a.tab = tab;
    a.gf = ctx.d_gf;
    a.k = c->k;
    a.m = c->m;
    a.stride = (uint32_t)check_layout(c->k, c->m).stride;
    a.lds = (uint32_t)(QFEC_PLAN_GF_BYTES + check_work_bytes(c->k, c->m));
    return for_group_chunks(gn, kMaxLaunchLanes / 64, [&](long long g0, long long n) {
        a.dmarks = dmarks ? dmarks + (size_t)g0 * c->k : nullptr;
        a.pmarks = dmarks ? pmarks + (size_t)g0 * c->m : nullptr;
        a.plan = d_check + (size_t)g0 * a.stride;
        a.groups = (uint64_t)n;
        const hipError_t e = launch_check_build(a, s);
        return e == hipSuccess ? QFEC_OK : hip_fail(e, "check_build kernel launch");
    });
}

struct CheckGeom {
    CheckApplyArgs a;
    long long per;  // groups per launch
};

static CheckGeom check_geom(DevCtx& ctx, const qfec_code* c, const uint8_t* d_data, const uint8_t* d_par, int block,
                            long long pitch) {
    CheckGeom G{};
    CheckApplyArgs& a = G.a;
    a.t256 = ctx.d_t256;
    a.k = c->k;
    a.m = c->m;
    a.pitch = (uint64_t)pitch;
    a.block = (uint32_t)block;
    a.dgs = (uint64_t)c->k * pitch;
    a.pgs = (uint64_t)c->m * pitch;
    a.stride = (uint32_t)check_layout(c->k, c->m).stride;
    const FlatGeom f = flat_geom(d_data, d_par, block, pitch, a.dgs, a.pgs);
    const WaveGeom w = wave_geom(f);  // whole waves per group, over 16-B columns or bytes
    a.vec16 = f.vec16;
    a.cols = w.cols;
    a.wpg = w.wpg;
    G.per = w.per;
    return G;
}

// the launches over groups [g0, g0 + gn) of a batch of `groups`, whose check plans start at d_check:
// three presets, the main kernel per chunk of `per` groups -- launch(c0, cn, flags, cmin, cmax), the
// words being those of group g0 -- and the finish kernel.  d_culprit is the batch's.  var: the finish
// kernel that knows an invalid group and counts it into d_invalid (nullable).
template <class Launch>
static int run_check_words(const qfec_code* c, uint32_t stride, long long per, const uint8_t* d_check, long long g0,
                           long long gn, long long groups, int* d_culprit, uint8_t* d_marks_out, unsigned* d_counts,
                           int scrub, hipStream_t s, Launch&& launch, bool var = false, unsigned* d_invalid = nullptr) {
    GroupWords words(s);  // [gn] flags, lowest candidate, highest candidate
    int rc = words.init("check_apply", gn, 3);
    if (rc) return rc;
    if (hipMemsetAsync(words.at(2), 0, (size_t)gn * 4, s) != hipSuccess)
        return hip_fail(hipGetLastError(), "check_apply: presetting the group words");
    rc = for_group_chunks(gn, per, [&](long long c0, long long cn) {
        return launch(c0, cn, words.at(0) + c0, words.at(1) + c0, words.at(2) + c0);
    });
    if (rc) return rc;
    CheckFinishArgs f{};
    f.check = d_check;
    f.flags = words.at(0);
    f.cmin = words.at(1);
    f.cmax = words.at(2);
    f.culprit = d_culprit ? d_culprit + g0 : nullptr;
    f.marks_out = d_marks_out;
    f.counts = d_counts;
    f.groups = (uint64_t)gn;
    f.g0 = (uint64_t)g0;
    f.all_groups = (uint64_t)groups;
    f.stride = stride;
    f.k = c->k;
    f.m = c->m;
    f.scrub = scrub;
    const hipError_t e = var ? launch_check_finish_var(f, d_invalid, s) : launch_check_finish(f, s);
    return e == hipSuccess ? QFEC_OK : hip_fail(e, "check_finish kernel launch");
}

static int run_check_apply(CheckGeom& G, const qfec_code* c, const uint8_t* d_data, const uint8_t* d_par,
                           const uint8_t* d_check, long long g0, long long gn, long long groups, int* d_culprit,
                           uint8_t* d_marks_out, unsigned* d_counts, int scrub, hipStream_t s) {
    CheckApplyArgs& a = G.a;
    return run_check_words(c, a.stride, G.per, d_check, g0, gn, groups, d_culprit, d_marks_out, d_counts, scrub, s,
                           [&](long long c0, long long cn, unsigned* flags, unsigned* cmin, unsigned* cmax) {
                               a.data = d_data + (size_t)(g0 + c0) * a.dgs;
                               a.parity = d_par + (size_t)(g0 + c0) * a.pgs;
                               a.check = d_check + (size_t)c0 * a.stride;
                               a.flags = flags;
                               a.cmin = cmin;
                               a.cmax = cmax;
                               a.groups = (uint64_t)cn;
                               const hipError_t e = launch_check_apply(a, s);
                               return e == hipSuccess ? QFEC_OK : hip_fail(e, "check_apply kernel launch");
                           });
}

// the same on a table of shard addresses: dptrs / pptrs are the two halves of the batch's table
static int run_check_apply_ptrs(DevCtx& ctx, const qfec_code* c, const uint64_t* dptrs, const uint64_t* pptrs,
                                const uint8_t* d_check, long long g0, long long gn, long long groups, int block,
                                int* d_culprit, uint8_t* d_marks_out, unsigned* d_counts, int scrub, hipStream_t s) {
    CheckPtrsArgs a{};
    const PtrsGeom p = ptrs_geom(block, 16);
    a.t256 = ctx.d_t256;
    a.k = c->k;
    a.m = c->m;
    a.block = (uint32_t)block;
    a.stride = (uint32_t)check_layout(c->k, c->m).stride;
    a.vcols = p.vcols;
    a.wpg = p.wpg;
    a.tail0 = p.tail0;
    a.tailn = p.tailn;
    return run_check_words(c, a.stride, p.per, d_check, g0, gn, groups, d_culprit, d_marks_out, d_counts, scrub, s,
                           [&](long long c0, long long cn, unsigned* flags, unsigned* cmin, unsigned* cmax) {
                               a.dptrs = dptrs + (size_t)(g0 + c0) * a.k;
                               a.pptrs = pptrs + (size_t)(g0 + c0) * a.m;
                               a.check = d_check + (size_t)c0 * a.stride;
                               a.flags = flags;
                               a.cmin = cmin;
                               a.cmax = cmax;
                               a.groups = (uint64_t)cn;
                               const hipError_t e = launch_check_apply_ptrs(a, s);
                               return e == hipSuccess ? QFEC_OK : hip_fail(e, "check_apply_ptrs kernel launch");
                           });
}

// the same with per-shard lengths: lens / glen are the batch's d_lens and d_group_len
static int run_check_apply_ptrs_var(DevCtx& ctx, const qfec_code* c, const uint64_t* dptrs, const uint64_t* pptrs,
                                    const int32_t* lens, const int32_t* glen, const uint8_t* d_check, long long g0,
                                    long long gn, long long groups, int max_len, int* d_culprit, uint8_t* d_marks_out,
                                    unsigned* d_counts, unsigned* d_invalid, int scrub, hipStream_t s) {
    CheckPtrsVarArgs a{};
    const PtrsGeom p = ptrs_geom(max_len, 16);
    a.p.t256 = ctx.d_t256;
    a.p.k = c->k;
    a.p.m = c->m;
    a.p.block = (uint32_t)max_len;
    a.p.stride = (uint32_t)check_layout(c->k, c->m).stride;
    a.p.vcols = p.vcols;
    a.p.wpg = p.wpg;
    a.p.tail0 = p.tail0;
    a.p.tailn = p.tailn;
    return run_check_words(
        c, a.p.stride, p.per, d_check, g0, gn, groups, d_culprit, d_marks_out, d_counts, scrub, s,
        [&](long long c0, long long cn, unsigned* flags, unsigned* cmin, unsigned* cmax) {
            a.p.dptrs = dptrs + (size_t)(g0 + c0) * a.p.k;
            a.p.pptrs = pptrs + (size_t)(g0 + c0) * a.p.m;
            a.lens = lens + (size_t)(g0 + c0) * a.p.k;
            a.group_len = glen + (g0 + c0);
            a.p.check = d_check + (size_t)c0 * a.p.stride;
            a.p.flags = flags;
            a.p.cmin = cmin;
            a.p.cmax = cmax;
            a.p.groups = (uint64_t)cn;
            const hipError_t e = launch_check_apply_ptrs_var(a, s);
            return e == hipSuccess ? QFEC_OK : hip_fail(e, "check_apply_ptrs_var kernel launch");
        },
        true, d_invalid);
}

// the one-shot locates: per chunk, check plans into stream-ordered scratch, apply(g0, gn, plans), free
template <class Apply>
static int locate_wide_chunks(const char* who, DevCtx& ctx, qfec_code* code, const uint8_t* d_marks, long long groups,
                              hipStream_t s, Apply&& apply) {
    const long long stride = check_layout(code->k, code->m).stride;
    const long long per = std::max(1ll, std::min(kMaxLaunchLanes / 64, kCheckScratchCap / stride));
    return for_group_chunks(groups, per, [&](long long g0, long long gn) {
        uint8_t* chk = nullptr;
        if (hipMallocAsync((void**)&chk, (size_t)gn * stride, s) != hipSuccess)
            return hip_fail(hipGetLastError(), (std::string(who) + " scratch").c_str());
        // rs.c layout: every group's data marks, then the parity marks
        int r = run_check_build(ctx, code, d_marks ? d_marks + (size_t)g0 * code->k : nullptr,
                                d_marks ? d_marks + (size_t)groups * code->k + (size_t)g0 * code->m : nullptr, gn, chk, s);
        if (!r) r = apply(g0, gn, chk);
        (void)hipFreeAsync(chk, s);
        return r;
    });
}

// qfec_locate_wide
static int run_locate_wide(const char* who, DevCtx& ctx, qfec_code* code, const uint8_t* d_data, const uint8_t* d_par,
                           const uint8_t* d_marks, long long groups, int block_size, long long pitch, int* d_culprit,
                           uint8_t* d_marks_out, unsigned* d_counts, int scrub, hipStream_t s) {
    CheckGeom G = check_geom(ctx, code, d_data, d_par, block_size, pitch);
    return locate_wide_chunks(who, ctx, code, d_marks, groups, s, [&](long long g0, long long gn, const uint8_t* chk) {
        return run_check_apply(G, code, d_data, d_par, chk, g0, gn, groups, d_culprit, d_marks_out, d_counts, scrub, s);
    });
}

// qfec_locate_ptrs_wide: t is the table, data entries first
static int run_locate_ptrs_wide(const char* who, DevCtx& ctx, qfec_code* code, const uint64_t* t, const uint8_t* d_marks,
                                long long groups, int block_size, int* d_culprit, uint8_t* d_marks_out,
                                unsigned* d_counts, int scrub, hipStream_t s) {
    return locate_wide_chunks(who, ctx, code, d_marks, groups, s, [&](long long g0, long long gn, const uint8_t* chk) {
        return run_check_apply_ptrs(ctx, code, t, t + (size_t)groups * code->k, chk, g0, gn, groups, block_size, d_culprit,
                                    d_marks_out, d_counts, scrub, s);
    });
}

// qfec_locate_ptrs_wide_var
static int run_locate_ptrs_wide_var(const char* who, DevCtx& ctx, qfec_code* code, const uint64_t* t, const int32_t* lens,
                                    const int32_t* glen, const uint8_t* d_marks, long long groups, int max_len,
                                    int* d_culprit, uint8_t* d_marks_out, unsigned* d_counts, unsigned* d_invalid,
                                    int scrub, hipStream_t s) {
    return locate_wide_chunks(who, ctx, code, d_marks, groups, s, [&](long long g0, long long gn, const uint8_t* chk) {
        return run_check_apply_ptrs_var(ctx, code, t, t + (size_t)groups * code->k, lens, glen, chk, g0, gn, groups,
                                        max_len, d_culprit, d_marks_out, d_counts, d_invalid, scrub, s);
    });
}

// what the three calls with per-shard lengths refuse before anything else
static const char* bad_table_var_args(const qfec_code* code, unsigned char* const* d_shards, const int* d_lens,
                                      const int* d_group_len, long long groups, int max_len) {
    return !code                        ? "null code"
           : groups < 0                 ? "groups < 0"
           : max_len < 1                ? "max_len < 1"
           : groups > 0 && !d_shards    ? "null d_shards"
           : groups > 0 && !d_lens      ? "null d_lens"
           : groups > 0 && !d_group_len ? "null d_group_len"
                                        : nullptr;
}

}  // namespace qfec

using namespace qfec;

extern "C" {

long long qfec_check_stride(const qfec_code* code) {
    if (!code) {
        set_error("qfec_check_stride: invalid argument (null code)");
        return QFEC_EINVAL;
    }
    return check_layout(code->k, code->m).stride;
}

int qfec_check_build_host(const qfec_code* code, const unsigned char* marks_n, unsigned char* out_check) {
    const char* who = "qfec_check_build_host";
    const char* why = !code ? "null code" : !marks_n || !out_check ? "null buffer" : nullptr;
    if (why) return refuse(who, why);
    const int rc = check_code_check(code, who);
    if (rc) return rc;
    const int k = code->k, m = code->m;
    uint64_t mk[4] = {0, 0, 0, 0};
    for (int i = 0; i < k + m; ++i)
        if (marks_n[i]) mk[i >> 6] |= 1ull << (i & 63);
    const Field& f = field();
    const PlanCode C{code->rows.data(), 1, k, m, 0, f.exp, f.log};
    std::vector<uint8_t> work((size_t)check_work_bytes(k, m));
    (void)check_group(C, mk, work.data(), out_check, PlanHostLanes{});
    return QFEC_OK;
}

int qfec_check_build(qfec_code* code, const unsigned char* d_marks, long long groups, unsigned char* d_check,
                     void* stream) {
    const char* who = "qfec_check_build";
    const char* why = !code                        ? "null code"
                      : groups < 0                 ? "groups < 0"
                      : groups > 0 && !d_check     ? "null buffer"
                      : plan_misaligned(d_check)  ? "d_check not 16-byte aligned"
                                                   : nullptr;
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(who, false, [&] { return check_code_check(code, who); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    return run_check_build(*ctx, code, d_marks, d_marks ? d_marks + (size_t)groups * code->k : nullptr, groups, d_check,
                           (hipStream_t)stream);
}

int qfec_check_apply(qfec_code* code, const unsigned char* d_data, const unsigned char* d_parity,
                     const unsigned char* d_check, long long groups, int block_size, long long pitch, int* d_culprit,
                     unsigned char* d_marks_out, unsigned int* d_counts, void* stream) {
    const char* who = "qfec_check_apply";
    const char* why = bad_rows_args(code, groups, block_size, pitch);
    if (!why && groups > 0 && (!d_data || !d_parity || !d_check || !d_culprit)) why = "null buffer";
    if (!why && plan_misaligned(d_check)) why = "d_check not 16-byte aligned";
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(who, false, [&] { return check_code_check(code, who); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    CheckGeom G = check_geom(*ctx, code, d_data, d_parity, block_size, pitch);
    return run_check_apply(G, code, d_data, d_parity, d_check, 0, groups, groups, d_culprit, d_marks_out, d_counts, 0,
                           (hipStream_t)stream);
}

int qfec_locate_wide(qfec_code* code, const unsigned char* d_data, const unsigned char* d_parity,
                     const unsigned char* d_marks, long long groups, int block_size, long long pitch, int* d_culprit,
                     unsigned char* d_marks_out, unsigned int* d_counts, void* stream) {
    const char* who = "qfec_locate_wide";
    const char* why = bad_rows_args(code, groups, block_size, pitch);
    if (!why && groups > 0 && (!d_data || !d_parity || !d_culprit)) why = "null buffer";
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(who, false, [&] { return check_code_check(code, who); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    return run_locate_wide(who, *ctx, code, d_data, d_parity, d_marks, groups, block_size, pitch, d_culprit, d_marks_out,
                           d_counts, 0, (hipStream_t)stream);
}

int qfec_scrub_wide(qfec_code* code, unsigned char* d_data, unsigned char* d_parity, const unsigned char* d_marks,
                    long long groups, int block_size, long long pitch, int* d_culprit, unsigned int* d_counts,
                    unsigned int* d_failed, void* stream) {
    const char* who = "qfec_scrub_wide";
    const char* why = bad_rows_args(code, groups, block_size, pitch);
    if (!why && groups > 0 && (!d_data || !d_parity)) why = "null buffer";
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    int rc = batch_begin(who, false, [&] { return check_code_check(code, who); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    hipStream_t s = (hipStream_t)stream;
    uint8_t* marks = nullptr;  // the locate's marks_out, then the repair's marks
    if (hipMallocAsync((void**)&marks, (size_t)groups * (size_t)(code->k + code->m), s) != hipSuccess)
        return hip_fail(hipGetLastError(), "scrub_wide scratch");
    rc = run_locate_wide(who, *ctx, code, d_data, d_parity, d_marks, groups, block_size, pitch, d_culprit, marks, d_counts,
                         1, s);
    if (!rc) rc = qfec_repair_wide(code, d_data, d_parity, marks, groups, block_size, pitch, d_failed, stream);
    (void)hipFreeAsync(marks, s);
    return rc;
}

int qfec_check_apply_ptrs(qfec_code* code, unsigned char* const* d_shards, const unsigned char* d_check, long long groups,
                          int block_size, int* d_culprit, unsigned char* d_marks_out, unsigned int* d_counts,
                          void* stream) {
    const char* who = "qfec_check_apply_ptrs";
    const char* why = bad_table_args(code, d_shards, groups, block_size);
    if (!why && groups > 0) why = !d_check ? "null d_check" : !d_culprit ? "null d_culprit" : nullptr;
    if (!why && plan_misaligned(d_check)) why = "d_check not 16-byte aligned";
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(who, false, [&] { return check_code_check(code, who); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    const uint64_t* t = reinterpret_cast<const uint64_t*>(d_shards);
    return run_check_apply_ptrs(*ctx, code, t, t + (size_t)groups * code->k, d_check, 0, groups, groups, block_size,
                                d_culprit, d_marks_out, d_counts, 0, (hipStream_t)stream);
}

int qfec_locate_ptrs_wide(qfec_code* code, unsigned char* const* d_shards, const unsigned char* d_marks, long long groups,
                          int block_size, int* d_culprit, unsigned char* d_marks_out, unsigned int* d_counts,
                          void* stream) {
    const char* who = "qfec_locate_ptrs_wide";
    const char* why = bad_table_args(code, d_shards, groups, block_size);
    if (!why && groups > 0 && !d_culprit) why = "null d_culprit";
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(who, false, [&] { return check_code_check(code, who); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    return run_locate_ptrs_wide(who, *ctx, code, reinterpret_cast<const uint64_t*>(d_shards), d_marks, groups, block_size,
                                d_culprit, d_marks_out, d_counts, 0, (hipStream_t)stream);
}

int qfec_scrub_ptrs_wide(qfec_code* code, unsigned char* const* d_shards, const unsigned char* d_marks, long long groups,
                         int block_size, int* d_culprit, unsigned int* d_counts, unsigned int* d_failed, void* stream) {
    const char* who = "qfec_scrub_ptrs_wide";
    const char* why = bad_table_args(code, d_shards, groups, block_size);
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    int rc = batch_begin(who, false, [&] { return check_code_check(code, who); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    hipStream_t s = (hipStream_t)stream;
    uint8_t* marks = nullptr;  // the locate's marks_out, then the repair's marks
    if (hipMallocAsync((void**)&marks, (size_t)groups * (size_t)(code->k + code->m), s) != hipSuccess)
        return hip_fail(hipGetLastError(), "scrub_ptrs_wide scratch");
    rc = run_locate_ptrs_wide(who, *ctx, code, reinterpret_cast<const uint64_t*>(d_shards), d_marks, groups, block_size,
                              d_culprit, marks, d_counts, 1, s);
    if (!rc) rc = qfec_repair_ptrs_wide(code, d_shards, marks, groups, block_size, d_failed, stream);
    (void)hipFreeAsync(marks, s);
    return rc;
}

int qfec_check_apply_ptrs_var(qfec_code* code, unsigned char* const* d_shards, const int* d_lens, const int* d_group_len,
                              const unsigned char* d_check, long long groups, int max_len, int* d_culprit,
                              unsigned char* d_marks_out, unsigned int* d_counts, unsigned int* d_invalid, void* stream) {
    const char* who = "qfec_check_apply_ptrs_var";
    const char* why = bad_table_var_args(code, d_shards, d_lens, d_group_len, groups, max_len);
    if (!why && groups > 0) why = !d_check ? "null d_check" : !d_culprit ? "null d_culprit" : nullptr;
    if (!why && plan_misaligned(d_check)) why = "d_check not 16-byte aligned";
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(who, false, [&] { return check_code_check(code, who); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    const uint64_t* t = reinterpret_cast<const uint64_t*>(d_shards);
    return run_check_apply_ptrs_var(*ctx, code, t, t + (size_t)groups * code->k, d_lens, d_group_len, d_check, 0, groups,
                                    groups, max_len, d_culprit, d_marks_out, d_counts, d_invalid, 0, (hipStream_t)stream);
}

int qfec_locate_ptrs_wide_var(qfec_code* code, unsigned char* const* d_shards, const int* d_lens, const int* d_group_len,
                              const unsigned char* d_marks, long long groups, int max_len, int* d_culprit,
                              unsigned char* d_marks_out, unsigned int* d_counts, unsigned int* d_invalid, void* stream) {
    const char* who = "qfec_locate_ptrs_wide_var";
    const char* why = bad_table_var_args(code, d_shards, d_lens, d_group_len, groups, max_len);
    if (!why && groups > 0 && !d_culprit) why = "null d_culprit";
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(who, false, [&] { return check_code_check(code, who); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    return run_locate_ptrs_wide_var(who, *ctx, code, reinterpret_cast<const uint64_t*>(d_shards), d_lens, d_group_len,
                                    d_marks, groups, max_len, d_culprit, d_marks_out, d_counts, d_invalid, 0,
                                    (hipStream_t)stream);
}

int qfec_scrub_ptrs_wide_var(qfec_code* code, unsigned char* const* d_shards, const int* d_lens, const int* d_group_len,
                             const unsigned char* d_marks, long long groups, int max_len, int* d_culprit,
                             unsigned int* d_counts, unsigned int* d_failed, unsigned int* d_invalid, void* stream) {
    const char* who = "qfec_scrub_ptrs_wide_var";
    const char* why = bad_table_var_args(code, d_shards, d_lens, d_group_len, groups, max_len);
    if (why) return refuse(who, why);
    DevCtx* ctx = nullptr;
    int rc = batch_begin(who, false, [&] { return check_code_check(code, who); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t* t = reinterpret_cast<const uint64_t*>(d_shards);
    // the locate's marks_out, then the repair's marks; behind them (4-byte aligned) the verdicts the repair's
    // write clip reads, where the caller wants none
    const size_t nmarks = ((size_t)groups * (size_t)(code->k + code->m) + 3) & ~(size_t)3;
    uint8_t* marks = nullptr;
    if (hipMallocAsync((void**)&marks, nmarks + (d_culprit ? 0 : (size_t)groups * sizeof(int)), s) != hipSuccess)
        return hip_fail(hipGetLastError(), "scrub_ptrs_wide_var scratch");
    int* culprit = d_culprit ? d_culprit : reinterpret_cast<int*>(marks + nmarks);
    rc = run_locate_ptrs_wide_var(who, *ctx, code, t, d_lens, d_group_len, d_marks, groups, max_len, culprit, marks,
                                  d_counts, d_invalid, 1, s);
    if (!rc)
        rc = run_repair_ptrs_wide_var_clip(*ctx, code, t, d_lens, d_group_len, marks, culprit, groups, max_len, d_failed, s,
                                           who);
    (void)hipFreeAsync(marks, s);
    return rc;
}

}  // extern "C"
