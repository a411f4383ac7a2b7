// qfec_internal.hpp -- shared declarations of libqfec (host runtime <-> kernels).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <vector>

namespace qfec {

// dwords per coefficient in a perm table:
//   [0..4] v_perm_b32 tables (c*{0..7}, c*{0..7}<<3, c*{0..3}<<6, packed 4 bytes/dword)
//   [5]    row flag on column 0: 1 = row starts from the output's previous bytes
//   [6]    log(c) (0xFF for c == 0), for the LDS log/exp variant
//   [7]    c itself
constexpr int QFEC_TAB_STRIDE = 8;

constexpr int QFEC_REC_NONE = -1;  // LUT: nothing erased in this group
constexpr int QFEC_REC_FAIL = -2;  // LUT: more erased data than surviving parity
constexpr int QFEC_LE_UNCHECKED = -1;  // locate-erased LUT: t = m, no spare row to check with
constexpr int QFEC_LE_LOST = -2;       // locate-erased LUT: t > m
constexpr int QFEC_LUT_MAX_N = 24; // n <= 24 -> 2^n-entry pattern LUT on the device

constexpr int QFEC_VARIANT_PERM_I = 0;
constexpr int QFEC_VARIANT_LDSLOG_I = 1;

// n / d for n < 2^32 via a 33-bit magic (Granlund-Montgomery, round-up form)
struct DivMagic {
    uint64_t mul;
    uint32_t shift;
    uint32_t pow2;
};

DivMagic make_div_magic(uint32_t d);

struct EncodeArgs {
    const uint8_t* data;    // [groups][k][pitch]
    uint8_t* parity;        // [groups][m][pitch]
    const uint32_t* tab;    // [m][k][QFEC_TAB_STRIDE]
    const uint8_t* gf_exp;  // LDS variant: exp[512]
    const uint8_t* gf_log;  // LDS variant: log[256]
    uint64_t work;          // groups * cols lanes (< 2^32)
    uint64_t pitch;         // bytes between rows of a group
    uint64_t dgs, pgs;      // bytes between groups: data (k*pitch when packed), parity (m*pitch)
    DivMagic cols_div;
    uint32_t cols;          // columns per row: 16-B columns (vec16) or bytes
    int k, m;
    int vec16;
    int impl;               // tuning "encode_impl"
    int lds;                // dynamic LDS bytes per block, a residency cap: -1 auto, 0 none (tuning "encode_lds")
    int block;              // threads per block: -1 auto, 64, 256 (tuning "encode_block")
};

struct ReconArgs {
    uint8_t* data;            // [groups][k][pitch]
    const uint8_t* parity;    // [groups][m][pitch]
    const uint8_t* marks;     // rs.c layout, or NULL when group_rec is given
    const int32_t* lut;       // [2^n] pattern -> record offset (dwords) / QFEC_REC_*
    const int32_t* group_rec; // explicit mode: per-group record offset / QFEC_REC_*
    const uint32_t* records;
    unsigned int* failed;
    uint64_t groups;
    uint64_t pitch;
    uint64_t dgs, pgs;        // bytes between groups: data rows, parity rows
    uint32_t cols;            // 16-B columns (vec16) or bytes per row
    int k, m;
    int surv_off, lost_off, hdr;
    int coff;                 // record word of the coefficient-table byte offsets (RecordLayout::coff)
    const uint32_t* t256;     // [256][QFEC_TAB_STRIDE] perm tables of every coefficient value (compact mode)
    int vec16;
    int impl;                 // tuning "recon_impl": -1 auto, exact-e rows on 2 16-B lanes, 3 8-B lanes,
                              // 4 12-B lanes, 8 8-B lanes with one group per block
    uint32_t wpg;             // waves per group = ceil(cols / 64) (vec16 LUT kernels)
    uint32_t cols8, wpg8;     // the same at 8-B columns: ceil(B / 8), ceil(cols8 / 64)
    uint32_t cols12, wpg12;   // the same at 12-B columns (recon_impl 4)
    int rlds;                 // reconstruct skeleton probe: LDS bytes per block, a residency cap (0 none)
};

// group repair (qfec_kernels.hip, "repair"): every marked shard of a group, data or parity
struct RepairArgs {
    uint8_t* data;            // [groups][k][pitch]
    uint8_t* parity;          // [groups][m][pitch]
    const uint8_t* dmarks;    // [groups][k] data marks of this launch's groups
    const uint8_t* pmarks;    // [groups][m] parity marks of this launch's groups
    const int32_t* lut;       // [2^n] full n-bit mask -> record offset (dwords) / QFEC_REC_*
    const uint32_t* records;  // compact repair records (RecordLayout header only, no inline tables)
    const uint32_t* t256;     // [256][QFEC_TAB_STRIDE] perm tables of every coefficient value
    unsigned int* failed;
    uint64_t groups;
    uint64_t pitch;
    uint64_t dgs, pgs;        // bytes between groups: data rows, parity rows
    uint32_t cols;            // 16-B columns (vec16) or bytes per row
    uint32_t cols8, wpg8;     // 8-B columns per row and waves per group at 64 of them per wave
    int k, m;
    int surv_off, lost_off, coff;
    int vec16;
};

// batched parity check (qfec_verify.hip): the encode's mapping, compares in place of the stores
struct VerifyArgs {
    const uint8_t* data;      // [groups][k][pitch]
    const uint8_t* parity;    // [groups][m][pitch]
    const uint32_t* tab;      // [m][k][QFEC_TAB_STRIDE] (the encode's tables; the stale flag is not used)
    unsigned int* bad_rows;   // [groups] of this launch, zeroed before it; bit j = parity row j differs
    unsigned int* bad_groups; // counter of groups with any bad row; may be NULL
    uint64_t work;            // groups * cols lanes (< 2^31)
    uint64_t pitch;
    uint64_t dgs, pgs;
    DivMagic cols_div;
    uint32_t cols;            // 16-B columns (vec16) or bytes per row
    uint32_t block;           // block_size: bytes of a row that count
    int k, m;
    int vec16;
};

// incremental parity, range form (qfec_update.hip): the encode's mapping over `count` of the k columns
struct EncUpdateArgs {
    const uint8_t* part;      // [groups][count][pitch]: data rows first .. first + count - 1
    uint8_t* parity;          // [groups][m][pitch]
    const uint32_t* tab;      // [m][k][QFEC_TAB_STRIDE] (the encode's tables; the stale flag is not used)
    uint64_t work;            // groups * cols lanes (< 2^31)
    uint64_t pitch;
    uint64_t sgs, pgs;        // bytes between groups: part (count * pitch), parity (m * pitch)
    DivMagic cols_div;
    uint32_t cols;            // 16-B columns (vec16) or bytes per row
    int k, m;
    int first, count;         // 0 <= first, 1 <= count, first + count <= k
    int accumulate;           // 1: XOR into parity, 0: overwrite it
    int vec16;
};

// incremental parity, per-group form (qfec_update.hip): whole waves per group, so the shard id a
// group names, and with it the m tables of that column, are wave-uniform
struct UpdateArgs {
    const int32_t* shard;     // [groups] of this launch: 0..k-1 replaced, < 0 untouched, >= k invalid
    uint8_t* data;            // [groups][k][pitch], or NULL: rows holds the deltas
    const uint8_t* rows;      // [groups][pitch]: the new bytes of shard[g], or the delta
    uint8_t* parity;          // [groups][m][pitch]
    const uint32_t* tab;      // [m][k][QFEC_TAB_STRIDE] (the encode's tables; the stale flag is not used)
    unsigned int* invalid;    // counter of groups with shard >= k; may be NULL
    uint64_t groups;
    uint64_t pitch;
    uint64_t dgs, pgs;        // bytes between groups: data rows, parity rows (rows: pitch)
    uint64_t work;            // byte path: groups * cols lanes (< 2^31)
    DivMagic cols_div;        // byte path
    uint32_t cols;            // lanes per row: 16-B columns (vec16) or bytes
    uint32_t wpg;             // vec16: waves per group = ceil(cols / 64)
    int k, m;
    int vec16;
};

// encode / reconstruct on a table of shard addresses (qfec_ptrs.hip): one wave per (group, slab of 64
// columns); every shard is exactly `block` bytes and no byte outside it is touched
struct PtrsArgs {
    const uint64_t* dptrs;    // [groups][k] addresses of the data shards of this launch's groups
    const uint64_t* pptrs;    // [groups][m] addresses of their parity shards
    const uint8_t* dmarks;    // reconstruct: [groups][k] data marks of this launch's groups
    const uint8_t* pmarks;    // reconstruct: [groups][m] parity marks
    const uint32_t* tab;      // encode: [m][k][QFEC_TAB_STRIDE]
    const int32_t* lut;       // reconstruct: [2^n] pattern -> record offset (dwords) / QFEC_REC_*
    const uint32_t* records;
    const uint32_t* t256;     // [256][QFEC_TAB_STRIDE] perm tables of every coefficient value
    unsigned int* failed;
    uint64_t groups;
    uint32_t block;           // bytes per shard
    uint32_t lane_bytes;      // 16 or 8: bytes per lane of the vector body (PtrsGeom)
    uint32_t vcols, wpg;      // whole lane_bytes columns per shard; waves per group
    uint32_t tail0, tailn;    // the bytes past the last whole column: first byte, count (< lane_bytes)
    int k, m;
    int surv_off, lost_off, hdr, coff;  // RecordLayout
};

// the same with per-shard lengths (qfec_ptrs_var.hip): p is what the fixed-length kernels take, with
// block = max_len and the geometry of max_len, which only sizes the launch (wpg, lane_bytes); every
// group cuts its own length inside the kernel (ptrs_var_geom)
struct PtrsVarArgs {
    PtrsArgs p;
    const int32_t* lens;         // [groups][k] lengths of the data shards of this launch's groups
    int32_t* group_len_out;      // encode: [groups] written (-1 void, else the longest length); may be NULL
    const int32_t* group_len;    // reconstruct: [groups] length of the group's parity shards
    unsigned int* invalid;       // counter of groups refused for their lengths; may be NULL
};

// incremental parity on a table of shard addresses (qfec_update_ptrs.hip), both forms, with and without
// per-shard lengths: PtrsArgs' mapping on 16-B lanes with the geometry of `block`, which with lengths
// is max_len and only sizes the launch (every group cuts its own extent inside the kernel)
struct UpdatePtrsArgs {
    const uint64_t* dptrs;       // [groups][k] addresses of the data shards of this launch's groups
    const uint64_t* pptrs;       // [groups][m] addresses of their parity shards
    const uint32_t* tab;         // [m][k][QFEC_TAB_STRIDE] (the encode's tables; the stale flag is not used)
    const int32_t* lens;         // with lengths: [groups][k]; NULL allowed in delta mode of the per-group form
    const int32_t* group_len;    // with lengths: [groups] the extent of the group's parity shards
    const int32_t* shard;        // per-group form: [groups] 0..k-1 replaced, < 0 untouched, >= k invalid
    const uint64_t* news;        // per-group form: [groups] addresses of the new rows (or the deltas)
    const int32_t* new_len;      // per-group form with lengths: [groups]
    unsigned int* invalid;       // counter of groups refused for an id or a length; may be NULL
    uint64_t groups;
    uint32_t block;              // block_size, or max_len
    uint32_t vcols, wpg;         // whole 16-B columns per shard; waves per group (PtrsGeom at 16-B lanes)
    uint32_t tail0, tailn;       // the bytes past the last whole column: first byte, count (< 16)
    int k, m;
    int first, count;            // range form: 0 <= first, 1 <= count, first + count <= k
    int accumulate;              // range form: 1 XOR into the parity, 0 overwrite it
    int delta_only;              // per-group form: 1 the new rows are deltas and no data entry is dereferenced
};

// parity check and single-shard error location on a table of shard addresses
// (qfec_integrity_ptrs.hip): PtrsArgs' mapping on 16-B lanes, the group words of VerifyArgs / LocateArgs
struct IntegrityPtrsArgs {
    const uint64_t* dptrs;    // [groups][k] addresses of the data shards of this launch's groups
    const uint64_t* pptrs;    // [groups][m] addresses of their parity shards
    const uint32_t* tab;      // [m][k][QFEC_TAB_STRIDE] (the encode's tables; the stale flag is not used)
    const uint32_t* rtab;     // locate: [k][m-1][QFEC_TAB_STRIDE], as LocateArgs
    unsigned int* bad_rows;   // [groups] of this launch, zeroed before it
    unsigned int* cand;       // locate: [groups] of this launch, all ones before it
    unsigned int* bad_groups; // verify: counter of groups with any bad row; may be NULL
    uint64_t groups;
    uint32_t block;           // bytes per shard
    uint32_t vcols, wpg;      // whole 16-B columns per shard; waves per group (PtrsGeom)
    uint32_t tail0, tailn;    // the bytes past the last whole column: first byte, count (< 16)
    int k, m;                 // verify: m <= 32; locate: 2 <= m <= 32, k <= 32
};

// the same with per-shard lengths (qfec_integrity_ptrs_var.hip): p with block = max_len and the geometry
// of max_len, which only sizes the launch; every group cuts its own length inside the kernel (ptrs_var_geom)
struct IntegrityPtrsVarArgs {
    IntegrityPtrsArgs p;
    const int32_t* lens;         // [groups][k] lengths of the data shards of this launch's groups
    const int32_t* group_len;    // [groups] length of the group's parity shards
};

// the groups the kernels above left alone for their lengths, one thread per group (k_var_invalid)
struct VarInvalidArgs {
    const int32_t* lens;         // [groups][k]
    const int32_t* group_len;    // [groups]
    int* culprit;                // [groups]: QFEC_LOC_INVALID written for an invalid group; may be NULL
    unsigned int* invalid;       // counter of invalid groups; may be NULL
    uint64_t groups;
    uint32_t max_len;
    int k;
};

// single-shard error location (qfec_locate.hip): verify's mapping; a wave that holds a non-zero
// syndrome tests every data shard as the culprit
struct LocateArgs {
    const uint8_t* data;      // [groups][k][pitch]
    const uint8_t* parity;    // [groups][m][pitch]
    const uint32_t* tab;      // [m][k][QFEC_TAB_STRIDE] (the encode's tables; the stale flag is not used)
    const uint32_t* rtab;     // [k][m-1][QFEC_TAB_STRIDE] perm tables of r_{j,i} = P[j][i] / P[0][i], j = 1..m-1
    unsigned int* bad_rows;   // [groups] of this launch, zeroed before it; bit j = syndrome j is non-zero
    unsigned int* cand;       // [groups] of this launch, all ones before it; bit i = data shard i explains
                              // every non-zero syndrome column seen so far
    uint64_t work;            // groups * cols lanes (< 2^31)
    uint64_t pitch;
    uint64_t dgs, pgs;
    DivMagic cols_div;
    uint32_t cols;            // 16-B columns (vec16) or bytes per row
    uint32_t block;           // block_size: bytes of a row that count
    int k, m;                 // 2 <= m <= 32, k <= 32
    int vec16;
};

// the verdict per group from its two words, after the last launch_locate of a call
struct LocateFinishArgs {
    const unsigned int* bad_rows;  // [groups]
    const unsigned int* cand;      // [groups]
    int* culprit;                  // [groups] shard id or QFEC_LOC_*
    uint8_t* marks;                // rs.c layout, groups * (k + m) bytes; may be NULL
    unsigned int* counts;          // [3] located, multi, ambiguous; may be NULL
    uint64_t groups;
    int k, m;
};

// two-shard error location (qfec_locate2.hip), after qfec_locate's launches: the groups it called
// MULTI are listed, and a wave per listed group tests every pair {a, b} of shards: F_ab x s == 0 in
// every byte, F_ab = the m - 2 rows of the left null space of [h_a h_b] (columns of [rows | I])
constexpr int QFEC_LOC2_MAX_N = 24;  // C(24, 2) = 276 pair bits in nine 32-bit words
struct Locate2Args {
    const uint8_t* data;       // [groups][k][pitch], the whole batch
    const uint8_t* parity;     // [groups][m][pitch]
    const uint32_t* tab;       // [m][k][QFEC_TAB_STRIDE] (the encode's tables; the stale flag is not used)
    const uint32_t* t256;      // [256][QFEC_TAB_STRIDE] perm tables of every coefficient value
    const uint32_t* checks;    // [pairs][m-2][m] F_ab[r][j] as the byte offset of its perm table in t256
                               // (0: a zero entry); pairs in the order (0,1), (0,2), .. (n-2,n-1)
    const uint32_t* pair_ids;  // [pairs] a | b << 8
    const int* stage1;         // [groups] qfec_locate's verdicts
    unsigned int* list;        // [groups] the groups with stage1 == QFEC_LOC_MULTI, in no order
    unsigned int* list_n;      // how many; zeroed before the list kernel
    int* verdict2;             // [groups], written for listed groups only: a | b << 8, QFEC_LOC_MULTI
                               // or QFEC_LOC_AMBIGUOUS
    uint64_t groups;           // < 2^32
    uint64_t pitch;
    uint64_t dgs, pgs;
    uint32_t cols;             // 16-B columns (vec16) or bytes per row
    uint32_t block;            // block_size: bytes of a row that count
    int k, m;                  // 4 <= m, k + m <= QFEC_LOC2_MAX_N
    int pairs;                 // n (n - 1) / 2
    int vec16;
};

struct Locate2FinishArgs {
    const int* stage1;         // [groups]
    const int* verdict2;       // [groups], read where stage1 == QFEC_LOC_MULTI
    int* culprit;              // [groups][2]
    uint8_t* marks;            // rs.c layout, groups * (k + m) bytes; may be NULL
    unsigned int* counts;      // [4] one, two, multi, ambiguous; may be NULL
    uint64_t groups;
    int k, m;
};

// single-shard error location in groups that also have lost shards (qfec_locate_erased.hip): the
// repair body's mapping (a wave sits inside one group); the syndromes are those of the m - t spare
// parity rows over the k lowest unmarked shards
struct LocErasedArgs {
    const uint8_t* data;      // [groups][k][pitch]
    const uint8_t* parity;    // [groups][m][pitch]
    const uint8_t* dmarks;    // [groups][k] data marks of this launch's groups
    const uint8_t* pmarks;    // [groups][m] parity marks of this launch's groups
    const int32_t* lut;       // [2^n] full n-bit mask -> record offset (dwords) / QFEC_LE_*
    const uint32_t* records;  // LocErasedLayout records (offsets into t256, no inline tables)
    const uint32_t* t256;     // [256][QFEC_TAB_STRIDE] perm tables of every coefficient value
    unsigned int* bad;        // [groups] of this launch, zeroed before it; bit x = syndrome of spare x is non-zero
    unsigned int* cand;       // [groups] of this launch, all ones before it; bit c = the shard at position c of K
                              // explains every non-zero syndrome column seen so far
    uint64_t groups;
    uint64_t pitch;
    uint64_t dgs, pgs;        // bytes between groups: data rows, parity rows
    uint32_t cols;            // 16-B columns (vec16) or bytes per row
    uint32_t cols8, wpg8;     // 8-B columns per row and waves per group at 64 of them per wave
    uint32_t block;           // block_size: bytes of a row that count
    int k, m;                 // 2 <= m, k + m <= QFEC_LUT_MAX_N
    int ids_off, aoff, roff;  // LocErasedLayout
    int vec16;
};

// the verdict per group from its marks and its two words, after the last launch_locate_erased
struct LocErasedFinishArgs {
    const uint8_t* marks;          // rs.c layout over all groups (may be marks_out)
    const int32_t* lut;
    const uint32_t* records;
    const unsigned int* bad;       // [groups]
    const unsigned int* cand;      // [groups]
    int* culprit;                  // [groups] shard id or QFEC_LOC_*; may be NULL
    uint8_t* marks_out;            // rs.c layout; may be NULL, may be marks
    unsigned int* counts;          // [5] located, multi, ambiguous, unchecked, lost; may be NULL
    uint64_t groups;
    int k, m;
    int ids_off;
    int scrub;                     // 1: MULTI / AMBIGUOUS groups get all-zero marks_out (qfec_repair leaves them alone)
};

// device-built decode plans (qfec_plan.hip; layout and arithmetic in qfec_plan.hpp): one wave per
// group turns the group's marks into its plan, for any k + m
struct PlanBuildArgs {
    const uint8_t* dmarks;    // [groups][k] data marks of this launch's groups
    const uint8_t* pmarks;    // [groups][m] parity marks of this launch's groups
    const uint32_t* tab;      // [m][k][QFEC_TAB_STRIDE] the encode's tables: dword 7 is the coefficient itself
    const uint8_t* gf;        // exp[512] | log[256] (DevCtx::d_gf), staged into LDS
    uint8_t* plan;            // [groups][stride] of this launch
    unsigned int* failed;     // counter of groups whose plan has status 2; may be NULL
    uint64_t groups;          // one 64-thread block each (< 2^31)
    uint32_t stride;          // PlanLayout::stride
    uint32_t lds;             // dynamic LDS bytes per block: QFEC_PLAN_GF_BYTES + plan_work_bytes(k, m)
    int k, m;
    int mode;                 // QFEC_PLAN_RECONSTRUCT / QFEC_PLAN_REPAIR
    int quirk;                // the code's rs_stale_quirk
};

// a wave per (group, 64 columns) applies the group's plan: the k survivors in, the t listed rows out
struct PlanApplyArgs {
    uint8_t* data;            // [groups][k][pitch]
    uint8_t* parity;          // [groups][m][pitch]; written only where a plan lists parity rows
    const uint8_t* plan;      // [groups][stride] of this launch
    const uint32_t* t256;     // [256][QFEC_TAB_STRIDE] perm tables of every coefficient value
    uint64_t groups;
    uint64_t pitch;
    uint64_t dgs, pgs;        // bytes between groups: data rows, parity rows
    uint32_t stride;          // PlanLayout::stride
    uint32_t cols, wpg;       // lanes per row: 16-B columns (vec16) or bytes; waves per group at 64 of them
    int k, m;
    int vec16;
};

// the same on a table of shard addresses (k_plan_apply_ptrs): the mapping and the geometry of the
// pointer-table kernels (PtrsArgs), the plan of k_plan_apply
struct PlanPtrsArgs {
    const uint64_t* dptrs;    // [groups][k] addresses of the data shards of this launch's groups
    const uint64_t* pptrs;    // [groups][m] addresses of their parity shards
    const uint8_t* plan;      // [groups][stride] of this launch
    const uint32_t* t256;     // [256][QFEC_TAB_STRIDE] perm tables of every coefficient value
    uint64_t groups;
    uint32_t block;           // bytes per shard
    uint32_t stride;          // PlanLayout::stride
    uint32_t vcols, wpg;      // whole 16-B columns per shard; waves per group (PtrsGeom at 16-B lanes)
    uint32_t tail0, tailn;    // the bytes past the last whole column: first byte, count (< 16)
    int k, m;
};

// the same with per-shard lengths (k_plan_apply_ptrs_var): p with block = max_len and the geometry of
// max_len, which only sizes the launch; every group cuts its own length inside the kernel (ptrs_var_geom)
struct PlanPtrsVarArgs {
    PlanPtrsArgs p;
    const int32_t* lens;         // [groups][k] lengths of the data shards of this launch's groups
    const int32_t* group_len;    // [groups] length of the group's parity shards
    unsigned int* invalid;       // counter of groups refused for their lengths; may be NULL
};

// device-built check plans (qfec_check.hip; layout and arithmetic in qfec_plan.hpp): single-shard
// error location at any k + m.  k_check_build takes a PlanBuildArgs (dmarks NULL: nothing marked;
// mode, quirk and failed unused; lds = QFEC_PLAN_GF_BYTES + check_work_bytes(k, m)).
// A wave per (group, 64 columns) forms the group's syndromes from its check plan and folds what it
// finds into the group's three words
struct CheckApplyArgs {
    const uint8_t* data;      // [groups][k][pitch]
    const uint8_t* parity;    // [groups][m][pitch]
    const uint8_t* check;     // [groups][stride] of this launch
    const uint32_t* t256;     // [256][QFEC_TAB_STRIDE] perm tables of every coefficient value
    unsigned int* flags;      // [groups] of this launch, zero before it: 1 a non-zero syndrome byte, 2 one that no
                              // single shard explains
    unsigned int* cmin;       // [groups], all ones before it: the lowest candidate shard id of any wave
    unsigned int* cmax;       // [groups], zero before it: the highest
    uint64_t groups;
    uint64_t pitch;
    uint64_t dgs, pgs;        // bytes between groups: data rows, parity rows
    uint32_t stride;          // CheckLayout::stride
    uint32_t cols, wpg;       // lanes per row: 16-B columns (vec16) or bytes; waves per group at 64 of them
    uint32_t block;           // block_size: bytes of a row that count
    int k, m;
    int vec16;
};

// the same on a table of shard addresses (k_check_apply_ptrs): PlanPtrsArgs's mapping and geometry, the
// check plan and the three words of CheckApplyArgs
struct CheckPtrsArgs {
    const uint64_t* dptrs;    // [groups][k] addresses of the data shards of this launch's groups
    const uint64_t* pptrs;    // [groups][m] addresses of their parity shards
    const uint8_t* check;     // [groups][stride] of this launch
    const uint32_t* t256;     // [256][QFEC_TAB_STRIDE] perm tables of every coefficient value
    unsigned int* flags;      // [groups] of this launch, as in CheckApplyArgs
    unsigned int* cmin;
    unsigned int* cmax;
    uint64_t groups;
    uint32_t block;           // bytes per shard
    uint32_t stride;          // CheckLayout::stride
    uint32_t vcols, wpg;      // whole 16-B columns per shard; waves per group (PtrsGeom at 16-B lanes)
    uint32_t tail0, tailn;    // the bytes past the last whole column: first byte, count (< 16)
    int k, m;
};

// the same with per-shard lengths (k_check_apply_ptrs_var): p with block = max_len and the geometry of
// max_len, which only sizes the launch; every group cuts its own length inside the kernel (ptrs_var_geom).
// An invalid group sets bit 2 (value 4) of its flags word and nothing else
struct CheckPtrsVarArgs {
    CheckPtrsArgs p;
    const int32_t* lens;         // [groups][k] lengths of the data shards of this launch's groups
    const int32_t* group_len;    // [groups] length of the group's parity shards
};

// the verdict per group from its check plan's head and its three words
struct CheckFinishArgs {
    const uint8_t* check;          // [groups][stride] of this launch
    const unsigned int* flags;     // [groups] of this launch
    const unsigned int* cmin;
    const unsigned int* cmax;
    int* culprit;                  // [groups] of this launch: shard id or QFEC_LOC_*; may be NULL
    uint8_t* marks_out;            // rs.c layout over all_groups; may be NULL
    unsigned int* counts;          // [5] located, multi, ambiguous, unchecked, lost; may be NULL
    uint64_t groups;               // of this launch
    uint64_t g0, all_groups;       // where this launch's groups sit in marks_out
    uint32_t stride;
    int k, m;
    int scrub;                     // 1: MULTI / AMBIGUOUS groups get all-zero marks_out (the repair leaves them alone)
};

// FEC datagram batches (qfec_wire.hip): shards[G][n][pitch], wire[G][n][wire_pitch]
struct WireArgs {
    const uint8_t* payload;   // send: concatenated payloads (16 readable bytes past the last)
    const int64_t* offsets;   // send: [G*k] payload offsets
    const int32_t* sizes;     // send: [G*k] payload sizes
    const uint32_t* seq;      // send: [G][2] sent / src index of the group's first packet
    uint8_t* shards;
    uint64_t group_stride;    // n * pitch
    uint64_t pitch;
    uint8_t* wire;
    uint64_t wire_pitch;
    int32_t* wire_len;        // [G*n] datagram lengths (receive: 0 = not received)
    uint8_t* marks;           // receive: rs.c-layout erasure marks
    int32_t* rx_size;         // receive: [G*n] shard size or -1 (may be NULL)
    int32_t* status;          // receive: [G*k] payload offset (2|4), -1 dropped, -2 lost
    int32_t* psize;           // receive: [G*k] payload size field
    uint64_t groups;
    int k, m;
    int checksum;
    int dec_pkt_size;
    int store_nt;             // fused send: bit 0 body, bit 1 head use non-temporal stores
};

hipError_t launch_build_shards(const WireArgs& a, hipStream_t s);
// fused send path for templated (k, m); *launched = false when the shape has no instance
// `part` = scratch of (lpg / 16) * ((n + 1) / 2) u32 per group, lpg ~ (pitch + 13) / 16
hipError_t launch_pack_fused(const WireArgs& a, const uint32_t* tab, uint32_t* part, hipStream_t s, bool* launched);
struct FrameArgs {
    const uint8_t* in;        // [rows][in_pitch]
    const int32_t* in_len;    // [rows]
    uint8_t* out;             // [rows][out_pitch]
    int32_t* out_len;         // [rows] (frame: framed length, -1 if it does not fit)
    const uint8_t* mask;      // frame: [rows] raw mask byte (Session::PacketOutput's _mask++)
    uint32_t* conv_hid;       // [rows][2] Session prefix (frame: in, unframe: out); may be NULL
    int32_t* status;          // unframe: [rows]
    uint8_t* info;            // unframe: [rows][4] mask, check, cmd & 0x1f, protocol; may be NULL
    uint64_t rows, in_pitch, out_pitch;
    uint32_t gmask, cmd, protocol;
    int session;              // 1: the 8-byte conv/hid prefix is part of the frame
};
hipError_t launch_frame_udp(const FrameArgs& a, hipStream_t s);
// ProtocolUdp framing inside the datagram kernels (qfec_pack_frames / qfec_unpack_frames)
struct FrameSend {
    const uint8_t* mask;       // [G*n] raw mask bytes (Session::PacketOutput's _mask++)
    const uint32_t* conv_hid;  // [G*n][2] Session prefix, or NULL (4-byte prefix)
    uint32_t gmask, cmd, protocol;
};
struct FrameRecv {
    uint32_t gmask;
    int32_t* status;           // [G*n] RecvPacket verdict (0 ok, 1 short, 2 checksum, 3 cmd, 4 too long); nullable
    uint32_t* conv_hid;        // [G*n][2] Session prefix out (session frames only); nullable
};
hipError_t launch_pack_frames(const WireArgs& a, const FrameSend& fs, int fp, const uint32_t* tab, hipStream_t s,
                              bool* launched);
hipError_t launch_unpack_frames(const WireArgs& a, const FrameRecv& fr, int fp, const int32_t* lut,
                                const uint32_t* records, uint32_t rec_hdr, hipStream_t s, bool* launched);
hipError_t launch_len_by_status(int32_t* len, const int32_t* status, uint64_t rows, hipStream_t s);
hipError_t launch_gather_rows(const uint8_t* base, const uint64_t* off, const int32_t* len, uint64_t rows, int wrap_n,
                              int wrap_k, uint8_t* out, uint64_t out_pitch, int32_t* out_len, hipStream_t s);
// the datagram receive k_rx (qfec_rx.hip) for templated (k, m); *launched = false when the shape has no instance
hipError_t launch_rx(const WireArgs& a, const int32_t* lut, const uint32_t* records, uint32_t rec_hdr, hipStream_t s,
                     bool* launched);
hipError_t launch_unframe_udp(const FrameArgs& a, hipStream_t s);
hipError_t launch_emit_wire(const WireArgs& a, hipStream_t s);
hipError_t launch_parse_wire(const WireArgs& a, hipStream_t s);
hipError_t launch_check_payloads(const WireArgs& a, hipStream_t s);

// runtime tuning knobs (qfec_tune); defaults are the measured best.  Atomic: qfec_tune may
// write a knob while launches on other threads read it (each read is one atomic load)
struct Tuning {
    std::atomic<int> recon_impl{-1};  // -1 auto (per shape); 2, 3, 4: exact-e rows on 16-, 8-, 12-B lanes; 8: 3 one group per block
    std::atomic<int> encode_impl{-1};   // -1 auto (inputs in halves for k >= 16), 0 all rows, 2 halves
    std::atomic<int> wire_fused{1};     // fused datagram send where a (k, m) instance exists (0: staged)
    std::atomic<int> wire_rx{1};        // datagram receive: 1 fused k_rx, lanes and LDS staging by pitch; 2 / 3 16-B lanes
                                        // with / without LDS staging, 4 / 5 8-B lanes likewise; 0 staged (3 launches)
    std::atomic<int> host_chunk{0};     // host-buffer paths: groups per pipelined chunk (0: by bytes)
    std::atomic<int> host_threads{0};   // host copy threads for module/rs.h on host pointers (0: usable CPUs, <= 32)
    std::atomic<int> host_zero_copy{1}; // pinned host batches: kernels read/write them directly (0: staged copies)
    std::atomic<int> host_lanes{4};     // module/rs.h on host pointers: chunk slots in flight on the device (2..8)
    std::atomic<int> host_nt{2};        // module/rs.h on host pointers: streaming stores into the slots (0 / 1 / 2 sequential rows)
    std::atomic<int> encode_block{-1};  // threads per encode block: -1 auto (64 for k = 10 all-rows), 64, 256
    std::atomic<int> encode_lds{-1};    // LDS bytes per encode block, capping waves per CU (-1 auto, 0 none)
    std::atomic<int> rs_dev_ptrs{0};    // module/rs.h on scattered device shards: 1 the pointer-table kernels in place, 0 staged copies
    std::atomic<int> rs_dev_ptrs_wide{0};  // with rs_dev_ptrs 1: reconstruct of k + m > 24 through device plans on the table, 0 staged
};
Tuning& tuning();

hipError_t launch_encode(const EncodeArgs& a, int variant, hipStream_t stream);
hipError_t launch_reconstruct(const ReconArgs& a, hipStream_t stream);
hipError_t launch_repair(const RepairArgs& a, hipStream_t stream);
hipError_t launch_verify(const VerifyArgs& a, hipStream_t stream);
hipError_t launch_encode_update(const EncUpdateArgs& a, hipStream_t stream);
hipError_t launch_update(const UpdateArgs& a, hipStream_t stream);
hipError_t launch_encode_ptrs(const PtrsArgs& a, hipStream_t stream);
hipError_t launch_reconstruct_ptrs(const PtrsArgs& a, hipStream_t stream);
hipError_t launch_encode_ptrs_var(const PtrsVarArgs& a, hipStream_t stream);
hipError_t launch_reconstruct_ptrs_var(const PtrsVarArgs& a, hipStream_t stream);
// with_lens: the kernels with per-shard lengths (a.group_len, a.lens, a.new_len are read)
hipError_t launch_encode_update_ptrs(const UpdatePtrsArgs& a, bool with_lens, hipStream_t stream);
hipError_t launch_update_ptrs(const UpdatePtrsArgs& a, bool with_lens, hipStream_t stream);
hipError_t launch_verify_ptrs(const IntegrityPtrsArgs& a, hipStream_t stream);
hipError_t launch_locate_ptrs(const IntegrityPtrsArgs& a, hipStream_t stream);
hipError_t launch_verify_ptrs_var(const IntegrityPtrsVarArgs& a, hipStream_t stream);
hipError_t launch_locate_ptrs_var(const IntegrityPtrsVarArgs& a, hipStream_t stream);
// qfec_scrub_ptrs_var's correction: culprit [groups] of this launch, t256 and exp[512] of the device context
hipError_t launch_correct_ptrs_var(const IntegrityPtrsVarArgs& a, const int32_t* culprit, const uint32_t* t256,
                                   const uint8_t* gf_exp, hipStream_t stream);
hipError_t launch_var_invalid(const VarInvalidArgs& a, hipStream_t stream);
hipError_t launch_locate(const LocateArgs& a, hipStream_t stream);
hipError_t launch_locate_finish(const LocateFinishArgs& a, hipStream_t stream);
hipError_t launch_locate2_list(const Locate2Args& a, hipStream_t stream);
hipError_t launch_locate2_pairs(const Locate2Args& a, hipStream_t stream);
hipError_t launch_locate2_finish(const Locate2FinishArgs& a, hipStream_t stream);
hipError_t launch_locate_erased(const LocErasedArgs& a, hipStream_t stream);
hipError_t launch_locate_erased_finish(const LocErasedFinishArgs& a, hipStream_t stream);
hipError_t launch_plan_build(const PlanBuildArgs& a, hipStream_t stream);
hipError_t launch_plan_apply(const PlanApplyArgs& a, hipStream_t stream);
hipError_t launch_plan_apply_ptrs(const PlanPtrsArgs& a, hipStream_t stream);
hipError_t launch_plan_apply_ptrs_var(const PlanPtrsVarArgs& a, hipStream_t stream);
hipError_t launch_plan_apply_ptrs_var_clip(const PlanPtrsVarArgs& a, const int32_t* culprit, hipStream_t stream);
hipError_t launch_check_build(const PlanBuildArgs& a, hipStream_t stream);
hipError_t launch_check_apply(const CheckApplyArgs& a, hipStream_t stream);
hipError_t launch_check_apply_ptrs(const CheckPtrsArgs& a, hipStream_t stream);
hipError_t launch_check_finish(const CheckFinishArgs& a, hipStream_t stream);
hipError_t launch_check_apply_ptrs_var(const CheckPtrsVarArgs& a, hipStream_t stream);
// invalid: counter of the groups whose flags say invalid; may be NULL
hipError_t launch_check_finish_var(const CheckFinishArgs& a, unsigned int* invalid, hipStream_t stream);
hipError_t launch_synth_fill(uint8_t* p, uint64_t nbytes, uint64_t seed, hipStream_t stream);
hipError_t launch_probe_xor(const EncodeArgs& a, hipStream_t stream);
hipError_t launch_probe_recon(const ReconArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- host GF(2^8) (gf256.cpp)
struct Field {
    uint8_t exp[512];  // exp[i] = 2^i, doubled (exp[i + 255] = exp[i]) + 2 pad
    uint8_t log[256];  // log[0] = 255 sentinel
    uint8_t inv[256];  // inv[0] = 0
    uint8_t mul[256][256];
};

const Field& field();

// parity rows (m x k, row-major) of the two reference matrix flavours
bool cauchy_rows(int k, int m, std::vector<uint8_t>& out);       // module/rs.c:437-440
bool vandermonde_rows(int k, int m, std::vector<uint8_t>& out);  // module/fec.c:653-707

// in-place GF inverse of a k x k matrix; false if singular
bool gf_invert(uint8_t* a, int k);
// the same with module/rs.c invert_mat's pivot order: on a singular matrix it returns false
// and leaves `a` in the partially eliminated state rs.c then decodes with (rs.c:556)
bool gf_invert_rs(uint8_t* a, int k);

// one coefficient's 8-dword perm table
void perm_entry(uint8_t c, uint32_t* out8);

// decode record of one erasure pattern (see qfec_kernels.hip, "reconstruct").
// group-order marks over n = k + m shards.  Returns e (>= 1), 0 if nothing is erased
// or -1 if under-determined; on e >= 1 fills rows (e x k), survivors (k), lost (e).
// `full` (n x k, nullable): module/rs.c's rs->m -- the sub-matrix is taken from it, data rows
// included, and inverted with rs.c's semantics (a singular one decodes with its partial state)
int decode_rows(const uint8_t* parity_rows, int k, int m, const uint8_t* marks_n,
                std::vector<uint8_t>& rows, std::vector<int>& survivors, std::vector<int>& lost,
                const uint8_t* full = nullptr);

// Record: [0] e, [1] rs.c quirk flags (bit j: row j's column-0 coefficient is zero),
// [surv_off + c] survivor shard id, [lost_off + j] erased data row,
// [coff + j*k + c] byte offset of coefficient (j, c)'s perm table in the 256-entry table
// (value * 32), then from [hdr] the tables themselves
// ([j][c][QFEC_TAB_STRIDE]).  A kernel that reads the offsets touches only the record's
// first (coff + m*k) words, so the records of every pattern stay cache-resident.
struct RecordLayout {
    int surv_off, lost_off, coff, hdr;
    size_t words(int e, int k) const { return (size_t)hdr + (size_t)e * k * QFEC_TAB_STRIDE; }
};
RecordLayout record_layout(int k, int m);

// repair rows of one erasure pattern over all n = k + m shards (group-order marks).  Returns t =
// the number of marked shards (1..m), 0 if nothing is marked or -1 if t > m (under-determined; also
// when the decode matrix is singular).  On t >= 1: survivors (k) = the k lowest unmarked ids, lost
// (t) = the marked ids ascending (data first), rows (t x k) over the survivors: the decode rows of
// decode_rows for the e erased data shards, then for every marked parity row j
// P[j] x [identity on surviving data; those decode rows on erased data] -- a true GF product.
// *e_out (nullable) = e.  `full` as in decode_rows.
int repair_rows(const uint8_t* parity_rows, int k, int m, const uint8_t* marks_n, std::vector<uint8_t>& rows,
                std::vector<int>& survivors, std::vector<int>& lost, const uint8_t* full = nullptr,
                int* e_out = nullptr);
// compact repair record: the RecordLayout header alone (hdr words): [0] t, [1] rs.c quirk flags of
// the e data rows, [2] e, survivors, lost ids (0..n-1), coefficient-table byte offsets
void build_repair_record(const RecordLayout& L, int k, int t, int e, const uint8_t* rows, const int* survivors,
                         const int* lost, bool rs_quirk, uint32_t* out);
void build_record(const RecordLayout& L, int k, int e, const uint8_t* rows, const int* survivors,
                  const int* lost, bool rs_quirk, uint32_t* out);

// Record of one erasure pattern for qfec_locate_erased (t <= m - 1 marked shards, S = m - t spares):
// [0] S, [1] t, [ids_off + c] id of the shard at position c of K (the k lowest unmarked ids),
// [ids_off + k + x] id of spare x (a parity row), [aoff + x*k + c] byte offset in the 256-entry
// table of the perm table of A_x[c], [roff + c*(S-1) + (x-1)] the same for A_x[c] / A_0[c].
struct LocErasedLayout {
    int ids_off, aoff, roff, words;
};
LocErasedLayout loc_erased_layout(int k, int m);

}  // namespace qfec
