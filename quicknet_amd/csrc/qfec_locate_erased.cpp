// qfec_locate_erased.cpp -- qfec_locate_erased (which single surviving shard of a group is corrupted,
// when the group also has lost shards), qfec_scrub_erased (locate, then qfec_repair with the marks it
// wrote) and qfec_locate_erased_plan of the device API in include/qfec.h.
//
// Per group with marked set E (t shards): K = the k lowest unmarked ids (qfec_repair's survivors),
// R = the other m - t unmarked ids (spare parity rows).  A_x, the row that predicts spare x from K,
// is the row repair_rows gives for x under the mask E + R; the syndromes s_x = shard_x ^ A_x . K are
// those of the code punctured at E.  Per code there is one record per mask with t <= m - 1 (the ids
// of K and R, the table offsets of A and of the ratios A_x[i] / A_0[i]), built on the host once per
// code->version under code->mu -- building them is also the check that the punctured codes are MDS
// -- and a 2^n-entry LUT from the mask to its record per device (a DevLut).
#include "qfec_rt.hpp"

namespace qfec {

LocErasedLayout loc_erased_layout(int k, int m) {
    LocErasedLayout L;
    L.ids_off = 2;
    L.aoff = (2 + k + m + 7) & ~7;
    L.roff = (L.aoff + m * k + 7) & ~7;
    L.words = (L.roff + k * (m - 1) + 7) & ~7;
    return L;
}

constexpr size_t kErasedMaxTableBytes = (size_t)256 << 20;  // the records of one code

// The plan of one group-order mark vector: survivors (k) = K, spares (S) = R, rows (S x k) = A,
// ratios (k x (S - 1)) = A_x[i] / A_0[i] at [i*(S-1) + (x-1)] (0 where A_0[i] is 0).  Returns
// S = m - t >= 1, 0 when t = m, -1 when t > m, -2 when the matrix over K is singular.
static int erased_plan(const uint8_t* P, int k, int m, const uint8_t* marks, std::vector<int>& survivors,
                       std::vector<int>& spares, std::vector<uint8_t>& rows, std::vector<uint8_t>& ratios) {
    const int n = k + m;
    survivors.clear();
    spares.clear();
    rows.clear();
    ratios.clear();
    std::vector<uint8_t> full((size_t)n);  // E + R: every shard outside K
    int t = 0;
    for (int i = 0; i < n; ++i) {
        full[i] = 1;
        if (marks[i]) ++t;
        else if ((int)survivors.size() < k) { survivors.push_back(i); full[i] = 0; }
        else spares.push_back(i);
    }
    if (t > m) return -1;
    if (t == m) return 0;
    const int S = m - t;
    std::vector<uint8_t> all;
    std::vector<int> surv, lost;
    if (repair_rows(P, k, m, full.data(), all, surv, lost) != m) return -2;
    rows.assign((size_t)S * k, 0);
    for (int x = 0; x < S; ++x) {
        const size_t r = std::find(lost.begin(), lost.end(), spares[x]) - lost.begin();
        memcpy(&rows[(size_t)x * k], &all[r * k], (size_t)k);
    }
    ratio_rows(rows.data(), S, k, ratios);
    return S;
}

// the records of every mask with t <= m - 1, or the refusal (caller holds c->mu; the code passed
// locate_code_check with need_lut).  Sets the error text on a refusal.
static int ensure_erased_host(qfec_code* c, const char* who) {
    if (c->le_host_version != c->version) {
        const int k = c->k, m = c->m, n = k + m;
        const LocErasedLayout L = loc_erased_layout(k, m);
        c->le_recs.clear();
        c->le_masks.clear();
        c->le_rc = QFEC_OK;
        c->le_error.clear();
        std::vector<uint8_t> marks((size_t)n), rows, ratios;
        std::vector<int> surv, spares;
        char why[200];
        // sum_{t < m} C(n, t) records: a wide m at n near 24 would need gigabytes (and minutes)
        double nrec = 0, comb = 1;
        for (int t = 0; t < m; ++t) {
            nrec += comb;
            comb = comb * (n - t) / (t + 1);
        }
        if (nrec * L.words * 4 > (double)kErasedMaxTableBytes) {
            c->le_rc = QFEC_EUNSUP;
            snprintf(why, sizeof why, "k = %d, m = %d needs %.0f pattern records (%.0f MiB, more than %d MiB)", k, m, nrec,
                     nrec * L.words * 4 / 1048576.0, (int)(kErasedMaxTableBytes >> 20));
            c->le_error = why;
        }
        for (int t = 0; t < m && c->le_rc == QFEC_OK; ++t) {
            // every mask of t bits, ascending (Gosper's hack); t = 0 is the one empty mask
            for (uint32_t mask = t ? (1u << t) - 1u : 0u;;) {
                for (int i = 0; i < n; ++i) marks[i] = (mask >> i) & 1u;
                const int S = erased_plan(c->rows.data(), k, m, marks.data(), surv, spares, rows, ratios);
                // one spare has no ratio to test: a zero there only hides an error, as any t = m - 1 group may
                const uint8_t* zero = S >= 2 ? (const uint8_t*)memchr(rows.data(), 0, rows.size()) : nullptr;
                if (S < 0) {
                    snprintf(why, sizeof why, "with the shards of mask 0x%x lost the matrix over the %d lowest survivors is singular",
                             mask, k);
                } else if (zero) {
                    const size_t at = (size_t)(zero - rows.data());
                    snprintf(why, sizeof why,
                             "with the shards of mask 0x%x lost, spare row %d has a zero coefficient at survivor %d (an error "
                             "there would not show in that row)", mask, spares[at / k], surv[at % k]);
                }
                if (S < 0 || zero) {
                    c->le_rc = QFEC_EUNSUP;
                    c->le_error = std::string(why) + ": the punctured code is not MDS";
                    break;
                }
                const size_t off = c->le_recs.size();
                c->le_recs.resize(off + (size_t)L.words, 0);
                uint32_t* r = &c->le_recs[off];
                r[0] = (uint32_t)S;
                r[1] = (uint32_t)t;
                for (int i = 0; i < k; ++i) r[L.ids_off + i] = (uint32_t)surv[i];
                for (int x = 0; x < S; ++x) r[L.ids_off + k + x] = (uint32_t)spares[x];
                for (size_t i = 0; i < rows.size(); ++i) r[L.aoff + i] = (uint32_t)rows[i] * (QFEC_TAB_STRIDE * 4);
                for (size_t i = 0; i < ratios.size(); ++i) r[L.roff + i] = (uint32_t)ratios[i] * (QFEC_TAB_STRIDE * 4);
                c->le_masks.emplace_back(mask, (int32_t)off);
                if (t == 0) break;
                const uint32_t lo = mask & (0u - mask), rip = mask + lo;
                mask = rip | (((mask ^ rip) >> 2) / lo);
                if (mask >> n) break;
            }
        }
        if (c->le_rc) {
            c->le_recs.clear();
            c->le_masks.clear();
        }
        c->le_host_version = c->version;
    }
    if (c->le_rc) set_error("%s: %s", who, c->le_error.c_str());
    return c->le_rc;
}

static int erased_supported(qfec_code* c, const char* who) {
    const int rc = locate_code_check(c, who, true);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    return ensure_erased_host(c, who);
}

// device LUT (2^n entries) + records of `c` (caller holds c->mu; ensure_erased_host passed)
static int ensure_erased_lut(qfec_code* c, int dev, DevTables** out) {
    DevTables& d = c->dev[dev];
    *out = &d;
    if (d.le.version == c->version && d.le.lut) return QFEC_OK;
    const int m = c->m, n = c->k + c->m;
    const size_t nmask = (size_t)1 << n;
    std::vector<int32_t> lut(nmask);
    for (size_t mask = 0; mask < nmask; ++mask) {
        const int t = __builtin_popcountll((unsigned long long)mask);
        lut[mask] = t > m ? QFEC_LE_LOST : QFEC_LE_UNCHECKED;  // t < m is overwritten below
    }
    for (const auto& e : c->le_masks) lut[e.first] = e.second;
    return upload_lut(d.le, lut, c->le_recs, c->version);
}

// the launches of one qfec_locate_erased: two presets, the main kernel per chunk, the finish kernel
static int run_locate_erased(DevCtx& ctx, qfec_code* code, const uint8_t* d_data, const uint8_t* d_parity,
                             const uint8_t* d_marks, long long groups, int block_size, long long pitch, int* d_culprit,
                             uint8_t* d_marks_out, unsigned* d_counts, int scrub, hipStream_t s) {
    DevTables* d = nullptr;
    int rc;
    {
        std::lock_guard<std::mutex> lk(code->mu);
        rc = ensure_erased_host(code, "qfec_locate_erased");
        if (!rc) rc = ensure_erased_lut(code, ctx.device, &d);
    }
    if (rc) return rc;
    GroupWords words(s);  // [groups] bad spares, then [groups] candidates
    rc = words.init("locate_erased", groups, 2);
    if (rc) return rc;
    unsigned *bad = words.at(0), *cand = words.at(1);
    const LocErasedLayout L = loc_erased_layout(code->k, code->m);
    LocErasedArgs a{};
    a.lut = d->le.lut;
    a.records = d->le.rec;
    a.t256 = ctx.d_t256;
    a.pitch = (uint64_t)pitch;
    a.block = (uint32_t)block_size;
    a.k = code->k;
    a.m = code->m;
    a.ids_off = L.ids_off;
    a.aoff = L.aoff;
    a.roff = L.roff;
    a.dgs = (uint64_t)code->k * pitch;
    a.pgs = (uint64_t)code->m * pitch;
    const FlatGeom fg = flat_geom(d_data, d_parity, block_size, pitch, a.dgs, a.pgs);
    const Lane8Geom l8 = lane8_geom(fg, code->k, block_size);
    a.vec16 = fg.vec16;
    a.cols = fg.cols;
    a.cols8 = l8.cols8;
    a.wpg8 = l8.wpg8;
    rc = for_group_chunks(groups, l8.per, [&](long long g0, long long gn) {
        a.data = d_data + (size_t)g0 * a.dgs;
        a.parity = d_parity + (size_t)g0 * a.pgs;
        a.dmarks = d_marks + (size_t)g0 * code->k;  // rs.c layout: every group's data marks, then the parity marks
        a.pmarks = d_marks + (size_t)groups * code->k + (size_t)g0 * code->m;
        a.bad = bad + g0;
        a.cand = cand + g0;
        a.groups = (uint64_t)gn;
        const hipError_t he = launch_locate_erased(a, s);
        return he == hipSuccess ? QFEC_OK : hip_fail(he, "locate_erased kernel launch");
    });
    if (rc) return rc;
    LocErasedFinishArgs f{};
    f.marks = d_marks;
    f.lut = d->le.lut;
    f.records = d->le.rec;
    f.bad = bad;
    f.cand = cand;
    f.culprit = d_culprit;
    f.marks_out = d_marks_out;
    f.counts = d_counts;
    f.groups = (uint64_t)groups;
    f.k = code->k;
    f.m = code->m;
    f.ids_off = L.ids_off;
    f.scrub = scrub;
    const hipError_t he = launch_locate_erased_finish(f, s);
    return he == hipSuccess ? QFEC_OK : hip_fail(he, "locate_erased finish kernel launch");
}

}  // namespace qfec

using namespace qfec;

extern "C" {

int qfec_locate_erased_plan(const qfec_code* code, const unsigned char* marks_n, int* survivors_out, int* spares_out,
                            unsigned char* rows_out, unsigned char* ratios_out) {
    if (!code || !marks_n) return QFEC_EINVAL;
    std::vector<int> surv, spares;
    std::vector<uint8_t> rows, ratios;
    const int S = erased_plan(code->rows.data(), code->k, code->m, marks_n, surv, spares, rows, ratios);
    if (S == -2) {
        set_error("qfec_locate_erased_plan: the matrix over the %d lowest unmarked shards is singular", code->k);
        return QFEC_EUNSUP;
    }
    if (S < 0) return -1;
    if (survivors_out) memcpy(survivors_out, surv.data(), surv.size() * sizeof(int));
    if (S > 0) {
        if (spares_out) memcpy(spares_out, spares.data(), spares.size() * sizeof(int));
        if (rows_out) memcpy(rows_out, rows.data(), rows.size());
        if (ratios_out && !ratios.empty()) memcpy(ratios_out, ratios.data(), ratios.size());
    }
    return S;
}

int qfec_prepare_locate_erased(qfec_code* code) {
    if (!code) return QFEC_EINVAL;
    int rc = erased_supported(code, "qfec_prepare_locate_erased");
    if (rc) return rc;
    DevCtx* ctx = nullptr;
    rc = current_ctx(&ctx);
    if (rc) return rc;
    DevTables* d = nullptr;
    std::lock_guard<std::mutex> lk(code->mu);
    return ensure_erased_lut(code, ctx->device, &d);
}

int qfec_locate_erased(qfec_code* code, const unsigned char* d_data, const unsigned char* d_parity,
                       const unsigned char* d_marks, long long groups, int block_size, long long pitch, int* d_culprit,
                       unsigned char* d_marks_out, unsigned int* d_counts, void* stream) {
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(
        "qfec_locate_erased",
        bad_batch(code, groups, block_size, pitch) || (groups > 0 && (!d_data || !d_parity || !d_marks || !d_culprit)),
        [&] { return erased_supported(code, "qfec_locate_erased"); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    return run_locate_erased(*ctx, code, d_data, d_parity, d_marks, groups, block_size, pitch, d_culprit, d_marks_out,
                             d_counts, 0, (hipStream_t)stream);
}

int qfec_scrub_erased(qfec_code* code, unsigned char* d_data, unsigned char* d_parity, const unsigned char* d_marks,
                      long long groups, int block_size, long long pitch, int* d_culprit, unsigned int* d_counts,
                      unsigned int* d_failed, void* stream) {
    DevCtx* ctx = nullptr;
    const int rc = batch_begin(
        "qfec_scrub_erased", bad_batch(code, groups, block_size, pitch) || (groups > 0 && (!d_data || !d_parity || !d_marks)),
        [&] { return erased_supported(code, "qfec_scrub_erased"); }, groups == 0, &ctx);
    if (rc || !ctx) return rc;
    hipStream_t s = (hipStream_t)stream;
    return run_scrub("qfec_scrub_erased", code, d_data, d_parity, groups, block_size, pitch, 0, d_failed, s,
                     [&](uint8_t* marks, uint8_t*) {
                         return run_locate_erased(*ctx, code, d_data, d_parity, d_marks, groups, block_size, pitch, d_culprit,
                                                  marks, d_counts, 1, s);
                     });
}

}  // extern "C"
