// qfec_rt.hpp -- internals shared by the host runtime's translation units:
//   qfec_runtime.cpp   errors, device contexts, code objects and their device tables, the batched
//                      device API (qfec_*), knobs, calibration probes, row staging
//   qfec_fec_abi.cpp   system/fec.h (fec_new / fec_encode / fec_decode) and the resident per-call
//                      server behind it
//   qfec_rs_abi.cpp    module/rs.h (reed_solomon_*) with its host-pointer pipelines and the
//                      classification of caller shard pointers
//   qfec_pipe.cpp      qfec_pipe_* (host batches streamed over several streams and devices)
//   qfec_wire_api.cpp  the datagram / framing entry points (qfec_pack_*, qfec_unpack_*, ...)
//   qfec_repair.cpp    qfec_repair (its LUT and records) and qfec_verify
//   qfec_locate.cpp    qfec_locate (its ratio tables), qfec_scrub, and what the locate family shares:
//                      the code check, the ratio formula, the scrub driver
//   qfec_locate_erased.cpp  qfec_locate_erased (its LUT and records), qfec_scrub_erased
//   qfec_locate2.cpp   qfec_locate2 (its acceptance check and pair constants), qfec_scrub2
//   qfec_update.cpp    qfec_encode_update, qfec_update (incremental parity on the encode's tables)
//   qfec_ptrs.cpp      qfec_encode_ptrs, qfec_reconstruct_ptrs (shards given as a device table of addresses)
//   qfec_plan.cpp      qfec_plan_build / qfec_plan_apply, qfec_reconstruct_wide / qfec_repair_wide (decode plans
//                      built on the device, any k + m), qfec_plan_build_host
//   qfec_plan_ptrs.cpp qfec_plan_apply_ptrs, qfec_reconstruct_ptrs_wide / qfec_repair_ptrs_wide (the plans applied to
//                      shards given as a device table of addresses)
//   qfec_integrity_ptrs.cpp  qfec_verify_ptrs, qfec_locate_ptrs, qfec_scrub_ptrs (the parity check and single-shard
//                      error location on shards given as a device table of addresses)
//   qfec_integrity_ptrs_var.cpp  qfec_verify_ptrs_var, qfec_locate_ptrs_var, qfec_scrub_ptrs_var (the same where every
//                      data shard has its own length; the scrub corrects from one parity row, without a plan)
//   qfec_check.cpp     qfec_check_build / qfec_check_apply, qfec_locate_wide / qfec_scrub_wide (check plans built
//                      on the device: single-shard error location at any k + m), qfec_check_build_host,
//                      qfec_check_apply_ptrs, qfec_locate_ptrs_wide / qfec_scrub_ptrs_wide (the same on a table)
// Launch geometry (lanes per row, groups per launch) is qfec_geom.hpp's, for every launch site.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/qfec.h"
#include "../../include/qfec_fec.h"
#include "../../include/qfec_rs.h"
#include "qfec_geom.hpp"
#include "qfec_internal.hpp"
#include "qfec_maps.hpp"
#include "qfec_percall.hpp"
#include "qfec_pool.hpp"

namespace qfec {

// ---- errors (qfec_runtime.cpp): the thread's last error text, qfec_last_error()
extern thread_local std::string t_last_error;
void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int hip_fail(hipError_t e, const char* what);  // sets the error text, returns QFEC_EHIP

#define HIP_TRY(expr)                                       \
    do {                                                    \
        hipError_t _e = (expr);                             \
        if (_e != hipSuccess) return hip_fail(_e, #expr);   \
    } while (0)

inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- settings (qfec_tune keys outside Tuning; qfec_runtime.cpp / qfec_fec_abi.cpp)
extern std::atomic<int> g_variant;
extern std::atomic<int> g_percall_fast, g_percall_resident, g_percall_idle_us, g_percall_timeout_us,
    g_percall_fault, g_percall_group, g_percall_stop_us;
extern std::atomic<unsigned long long> g_group_hits, g_group_misses;

// ---- device contexts (qfec_runtime.cpp)
constexpr int kMaxDevices = 64;
constexpr int kMaxHostLanes = 8;  // host-buffer chunk slots per device context

struct DevCtx {
    int device = 0;
    std::mutex mu;  // serialises use of the staging buffers and the internal stream
    hipStream_t stream = nullptr;
    uint8_t* d_stage = nullptr;
    size_t d_cap = 0;
    uint8_t* h_stage = nullptr;  // pinned
    size_t h_cap = 0;
    uint8_t* d_gf = nullptr;     // exp[512] | log[256] for the LDS variant
    uint32_t* d_t256 = nullptr;  // perm tables of all 256 coefficient values (compact reconstruct)
    uint32_t* d_small = nullptr; // per-call tables (fec_encode row, fec_decode matrix)
    size_t small_cap = 0;
    uint32_t* h_small = nullptr; // pinned mirror
    unsigned* d_counter = nullptr;
    // per-packet calls (fec_encode / fec_decode): pinned, device-mapped staging the
    // k_percall kernel reads and writes directly (qfec_percall.hpp)
    uint8_t* h_pc = nullptr;
    uint8_t* d_pc = nullptr;  // the device address of h_pc
    size_t pc_cap = 0;
    uint32_t* h_pc_done = nullptr;  // k_percall's completion word (coherent pinned)
    uint32_t* d_pc_done = nullptr;
    uint32_t pc_seq = 0;
    uint32_t pc_unsynced = 0;       // spin-completed launches since the last stream query
    // the resident per-call server (qfec_percall.hpp): set up on first use
    struct PcServer {
        int usable = 0;              // 0 not tried, 1 ready, -1 unavailable on this device, -2 abandoned
                                     // (did not stop within percall_stop_us; percall_resident 1 retries)
        hipStream_t stream = nullptr;
        PcBell* bell = nullptr;      // fine-grained device memory the CPU stores into
        uint8_t* in = nullptr;       // ditto: kPcMaxCoef rows of kPcMaxChunks * 16 bytes
        uint8_t* h_out = nullptr;    // coherent pinned host memory, same shape
        uint8_t* d_out = nullptr;
        PcStatus* h_st = nullptr;    // coherent pinned host memory
        PcStatus* d_st = nullptr;
        uint32_t req = 0;            // the last request number stored into the bell word
        uint32_t tab_last[kPcTabWords];  // the tables the bell holds (tab_bytes of them)
        size_t tab_bytes = 0;
        uint32_t gen = 0;            // the last launch's generation
        bool launched = false;
        unsigned long long calls = 0, launches = 0, relaunches = 0, timeouts = 0, abandoned = 0;
        // QFEC_PERCALL_TRACE sums: loads, compute, fence (shader clocks), host wait (ns), n, clocks and
        // wall ticks over the traced span (the clock calibration)
        unsigned long long tr[7] = {0, 0, 0, 0, 0, 0, 0};
    } srv;
    int init_rc = QFEC_ENODEV;
    // host-buffer chunk slots, each with its own stream, event, device buffers and pinned staging
    // (created on first use): qfec_encode_host / qfec_reconstruct_host alternate host[0] and host[1];
    // module/rs.h's host-pointer pipelines take the first tuning "host_lanes" of them
    struct HostSlot {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        uint8_t* d_buf = nullptr;  // data chunk | parity chunk
        uint8_t* h_in = nullptr;   // pinned
        uint8_t* h_out = nullptr;  // pinned
        size_t in_cap = 0, out_cap = 0;
    } host[kMaxHostLanes];
    std::mutex host_mu;
};

extern DevCtx g_ctx[kMaxDevices];

int current_ctx(DevCtx** out);  // the calling thread's current device (created on first use)
int ensure_stage(DevCtx& c, size_t dbytes, size_t hbytes);
int ensure_pc(DevCtx& c, size_t bytes);
int ensure_small(DevCtx& c, size_t words);
bool is_device_ptr(const void* p);
bool is_pinned_host(const void* p);
bool host_dev(const void* h, uint8_t** d);
int ensure_host_slot(DevCtx::HostSlot& h, size_t in_bytes, size_t out_bytes);
void quiesce_host_slots(DevCtx& c);
// rows of caller memory to / from a device staging area (qfec_runtime.cpp)
int gather_rows(DevCtx& c, unsigned char* const* ptrs, size_t count, int len, size_t pitch, uint8_t* d_dst,
                uint8_t* h_tmp, bool dev_src);
int scatter_rows(DevCtx& c, unsigned char* const* ptrs, size_t count, int len, size_t pitch, const uint8_t* d_src,
                 uint8_t* h_tmp, bool dev_dst, const uint8_t* only);

// Per-group working words of one call, from stream-ordered scratch: `arrays` x [groups] unsigned,
// array 0 preset to zero, array 1 to all ones.  Freed on the stream when the object goes.  A call
// that needs one array may bring its own (`given`), which is then preset and not freed.
class GroupWords {
public:
    explicit GroupWords(hipStream_t s) : s_(s) {}
    ~GroupWords() {
        if (own_) (void)hipFreeAsync(own_, s_);
    }
    GroupWords(const GroupWords&) = delete;
    GroupWords& operator=(const GroupWords&) = delete;
    int init(const char* who, long long groups, int arrays, unsigned* given = nullptr);
    unsigned* at(int i) const { return w_ + (size_t)i * groups_; }

private:
    hipStream_t s_;
    unsigned *own_ = nullptr, *w_ = nullptr;
    size_t groups_ = 0;
};

// The head of a batched entry point: refuses bad arguments under the entry's name, asks the entry's
// own check of the code, and fetches the calling thread's device context.  *ctx stays null when
// there is nothing to do (`empty`) or the call is refused.
inline bool bad_batch(const qfec_code* code, long long groups, int block_size, long long pitch) {
    return !code || groups < 0 || block_size < 1 || pitch < block_size;
}
template <class Check>
int batch_begin(const char* who, bool bad_args, Check&& code_check, bool empty, DevCtx** ctx) {
    if (bad_args) {
        set_error("%s: invalid argument", who);
        return QFEC_EINVAL;
    }
    const int rc = code_check();
    return rc || empty ? rc : current_ctx(ctx);
}

// ---- the resident per-call server (qfec_fec_abi.cpp)
bool pc_server_alive(const DevCtx::PcServer& s);
hipError_t pc_server_stop(DevCtx& c, long long limit_us = -1);  // limit_us >= 0: bounded wait

}  // namespace qfec

// ---- code objects (qfec_runtime.cpp); qfec_code is the C ABI's opaque type
// a pattern LUT on one device: [2^n] mask -> record offset (dwords) or a negative code, and the records
struct DevLut {
    int32_t* lut = nullptr;
    uint32_t* rec = nullptr;
    uint64_t version = ~0ull;  // the code->version it was built from
};

struct DevTables {
    uint32_t* d_enc = nullptr;  // [m][k][8]
    uint64_t enc_version = ~0ull;
    DevLut dec;                 // reconstruct: decode records, shared between masks that differ in unused parity
    DevLut rep;                 // repair: full n-bit mask -> compact record (qfec_repair.cpp)
    uint32_t* d_loc = nullptr;  // [k][m-1][8] locate: perm tables of P[j][i] / P[0][i] (qfec_locate.cpp)
    uint64_t loc_version = ~0ull;
    DevLut le;                  // locate-erased: full n-bit mask -> LocErasedLayout record (qfec_locate_erased.cpp)
    uint32_t* d_loc2 = nullptr; // locate2: [pairs][m-2][m] check offsets, then [pairs] ids (qfec_locate2.cpp)
    uint64_t loc2_version = ~0ull;
};

struct qfec_code {
    int k = 0, m = 0;
    int quirk = 0;  // module/rs.c column-0 zero-coefficient behaviour
    std::mutex mu;
    std::vector<uint8_t> rows;  // m x k
    std::vector<uint8_t> full;  // n x k decode matrix of a reed_solomon handle (rs->m), else empty
    uint64_t version = 0;
    std::map<int, DevTables> dev;
    // host-side decode cache: pattern key -> (record words); for explicit mode
    std::unordered_map<uint64_t, std::vector<uint32_t>> rec_cache;
    uint64_t rec_cache_version = ~0ull;
    // per LUT mask: 1 if its record seeds a row from the output's old bytes (the rs.c quirk), so a
    // host-pointer reconstruct must stage the erased rows too (filled with the LUT)
    std::shared_ptr<const std::vector<uint8_t>> lut_seed;  // replaced whole on a rebuild; readers keep a reference
    uint64_t lut_seed_version = ~0ull;
    // qfec_locate_erased's host tables (qfec_locate_erased.cpp): the records of every mask with
    // t <= m - 1, or why the code is refused; built once per version under mu, uploaded per device
    uint64_t le_host_version = ~0ull;
    int le_rc = 0;
    std::string le_error;
    std::vector<uint32_t> le_recs;
    std::vector<std::pair<uint32_t, int32_t>> le_masks;  // (mask, record offset in dwords)
    // qfec_locate2's host constants (qfec_locate2.cpp): the checks of every pair, or why the code is
    // refused; built once per version under mu, uploaded per device
    uint64_t l2_host_version = ~0ull;
    int l2_rc = 0;
    std::string l2_error;
    std::vector<uint8_t> l2_checks;  // [pairs][m-2][m]: F_ab, pairs in the order (0,1), (0,2), .. (n-2,n-1)
    // device plans (qfec_plan.cpp): is `full` empty or [I; rows]?  Judged once per version under mu
    uint64_t plan_chk_version = ~0ull;
    bool plan_chk_ok = false;
    // check plans (qfec_check.cpp): are `rows` what qfec_code_new generates for (k, m), and why not?
    // Judged once per version under mu
    uint64_t check_chk_version = ~0ull;
    int check_chk_rc = 0;
    std::string check_chk_error;
};

namespace qfec {

qfec_code* make_code(int k, int m, std::vector<uint8_t>&& rows, int quirk);
void free_code(qfec_code* c);
const uint8_t* full_of(const qfec_code* c);  // module/rs.c's rs->m, or nullptr
int ensure_enc(qfec_code* c, int dev, uint32_t** out);    // caller holds c->mu
int ensure_lut(qfec_code* c, int dev, DevTables** out);   // caller holds c->mu
// replaces d's tables by (lut, recs) and stamps the version (synchronous; caller holds c->mu)
int upload_lut(DevLut& d, const std::vector<int32_t>& lut, const std::vector<uint32_t>& recs, uint64_t version);
int run_encode(DevCtx& ctx, const qfec_code* c, const uint32_t* tab, int m, const uint8_t* d_data, uint8_t* d_par,
               long long groups, int block, long long pitch, hipStream_t s, long long dgs = -1, long long pgs = -1,
               bool host_mem = false);
int run_reconstruct(DevCtx& ctx, const qfec_code* c, const int32_t* lut, const int32_t* group_rec,
                    const uint32_t* recs, uint8_t* d_data, const uint8_t* d_par, const uint8_t* d_marks,
                    long long groups, int block, long long pitch, unsigned* d_failed, hipStream_t s,
                    long long dgs = -1, long long pgs = -1);
// the pointer-table kernels (qfec_ptrs.cpp): dptrs / pptrs are device arrays of groups * k and
// groups * m shard addresses, dmarks / pmarks the two halves of rs.c-layout marks
int run_encode_ptrs(const qfec_code* c, const uint32_t* tab, const uint64_t* dptrs, const uint64_t* pptrs,
                    long long groups, int block, hipStream_t s);
int run_reconstruct_ptrs(DevCtx& ctx, const qfec_code* c, const DevLut& dec, const uint64_t* dptrs,
                         const uint64_t* pptrs, const uint8_t* dmarks, const uint8_t* pmarks, long long groups,
                         int block, unsigned* d_failed, hipStream_t s);
int host_records(qfec_code* c, const uint8_t* marks, long long groups, std::vector<int32_t>& grec,
                 std::vector<uint32_t>& recs, long long* nfail);
int reconstruct_host_records(DevCtx& ctx, qfec_code* c, uint8_t* d_data, const uint8_t* d_par,
                             const uint8_t* d_marks, long long groups, int block_size, long long pitch,
                             unsigned* d_failed, hipStream_t s);

// ---- device plans (qfec_plan.cpp)
// QFEC_EUNSUP for a code whose rs.c decode matrix is not [I; rows] (an edited handle)
int plan_code_check(const qfec_code* c, const char* who);
// what the plan calls (qfec_plan.cpp, qfec_check.cpp) refuse before a device is touched: the cause of a
// bad batch argument or nullptr; a plan base the 16-byte stores and dword loads cannot take; the
// refusal itself, its cause named in the error text (returns QFEC_EINVAL)
const char* bad_rows_args(const qfec_code* code, long long groups, int block_size, long long pitch);
// the same for the calls on a table of shard addresses (qfec_integrity_ptrs.cpp); a null table counts with groups > 0
const char* bad_table_args(const qfec_code* code, unsigned char* const* d_shards, long long groups, int block_size);
bool plan_misaligned(const void* d_plan);
int refuse(const char* who, const char* why);
// one chunk's plans in the one-shot calls stay under this many bytes of stream-ordered scratch
constexpr long long kPlanScratchCap = 64ll << 20;
// plans of `gn` groups whose marks start at dmarks / pmarks (tab: the code's encode tables on ctx's device)
int run_plan_build(DevCtx& ctx, const qfec_code* c, const uint32_t* tab, const uint8_t* dmarks, const uint8_t* pmarks,
                   long long gn, int mode, uint8_t* d_plan, unsigned* d_failed, hipStream_t s);
// ---- device plans on pointer tables (qfec_plan_ptrs.cpp): dptrs / pptrs as for run_encode_ptrs
// the plans of `gn` groups applied to the rows the table names; a launch over groups [g0, ..) of it
// is handed dptrs + g0 * k, pptrs + g0 * m, plan + g0 * stride
int run_plan_apply_ptrs(DevCtx& ctx, const qfec_code* c, const uint64_t* dptrs, const uint64_t* pptrs,
                        const uint8_t* d_plan, long long gn, int block, hipStream_t s);
// the same where every data shard has its own length: lens + g0 * k and glen + g0 go with a launch as well
int run_plan_apply_ptrs_var(DevCtx& ctx, const qfec_code* c, const uint64_t* dptrs, const uint64_t* pptrs,
                            const int32_t* lens, const int32_t* glen, const uint8_t* d_plan, long long gn, int max_len,
                            unsigned* d_invalid, hipStream_t s, const int32_t* culprit = nullptr);
// qfec_scrub_ptrs_wide_var's repair (t: the table, marks: rs.c layout, culprit: [groups], all of the batch)
int run_repair_ptrs_wide_var_clip(DevCtx& ctx, qfec_code* c, const uint64_t* t, const int32_t* lens, const int32_t* glen,
                                  const uint8_t* marks, const int32_t* culprit, long long groups, int max_len,
                                  unsigned* d_failed, hipStream_t s, const char* who);
// build into stream-ordered scratch, apply, free, in chunks of at most kPlanScratchCap of plans
int run_wide_ptrs(DevCtx& ctx, const qfec_code* c, const uint32_t* tab, const uint64_t* dptrs, const uint64_t* pptrs,
                  const uint8_t* dmarks, const uint8_t* pmarks, long long gn, int block, int mode, unsigned* d_failed,
                  hipStream_t s, const char* who);

// ---- shared by the locate family (qfec_locate.cpp)
// Can single-shard location work on this code at all?  Decided on the host, before any device.
// need_lut: also the width of a LUT keyed by the whole mask.
int locate_code_check(const qfec_code* c, const char* who, bool need_lut);
// perm tables of r_{j,i} = P[j][i] / P[0][i] of `c` on device `dev` (caller holds c->mu; the code passed
// locate_code_check)
int ensure_loc(qfec_code* c, int dev, uint32_t** out);
// out[i * (S - 1) + (x - 1)] = rows[x][i] / rows[0][i], x = 1..S-1 (0 where rows[0][i] is 0); rows is S x k
void ratio_rows(const uint8_t* rows, int S, int k, std::vector<uint8_t>& out);
// the launches of one qfec_locate (validated arguments): two presets, the main kernel per chunk, the
// finish kernel
int run_locate(DevCtx& ctx, qfec_code* code, const uint8_t* d_data, const uint8_t* d_parity, long long groups,
               int block_size, long long pitch, int* d_culprit, uint8_t* d_marks, unsigned* d_counts, hipStream_t s);
// the same on a pointer table (qfec_integrity_ptrs.cpp): dptrs / pptrs as for run_encode_ptrs, d_marks in the
// table's own order
int run_locate_ptrs(DevCtx& ctx, qfec_code* code, const uint64_t* dptrs, const uint64_t* pptrs, long long groups,
                    int block_size, int* d_culprit, uint8_t* d_marks, unsigned* d_counts, hipStream_t s);
// the same where every data shard has its own length (qfec_integrity_ptrs_var.cpp): lens [groups * k] in table
// order, glen [groups] the length of each group's parity shards; a group refused for its lengths gets
// QFEC_LOC_INVALID and is counted into d_invalid (nullable)
int run_locate_ptrs_var(DevCtx& ctx, qfec_code* code, const uint64_t* dptrs, const uint64_t* pptrs, const int32_t* lens,
                        const int32_t* glen, long long groups, int max_len, int* d_culprit, uint8_t* d_marks,
                        unsigned* d_counts, unsigned* d_invalid, hipStream_t s);
// locate(marks, extra), then qfec_repair with the marks it wrote; both from stream-ordered scratch
// (`extra` bytes follow the marks)
int run_scrub(const char* who, qfec_code* code, uint8_t* d_data, uint8_t* d_parity, long long groups, int block_size,
              long long pitch, size_t extra, unsigned* d_failed, hipStream_t s,
              const std::function<int(uint8_t* marks, uint8_t* extra)>& locate);

}  // namespace qfec
