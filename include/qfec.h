/*
 * qfec.h -- batched, device-resident GF(2^8) Reed-Solomon API of libqfec.so (MI355X).
 *
 * This is the GPU boundary the reference does not have: the reference codecs work one
 * group (module/rs.c:574-643) or one packet (system/fec.c:714-862) at a time on the CPU.
 * Here many independent (k+m)-shard groups are encoded or reconstructed by one kernel
 * launch over device buffers, on the caller's HIP stream, with no host synchronisation.
 * The per-packet / per-call C ABIs (qfec_fec.h, qfec_rs.h) are built on top of it.
 *
 * Device layout (one contiguous region per role; `pitch` bytes between shard starts):
 *   data   [groups][k][pitch]   shard bytes [0, block_size) of each row are the payload
 *   parity [groups][m][pitch]
 *   marks  [groups*k data marks][groups*m parity marks]  (module/rs.c:609-612 layout;
 *          non-zero = erased)
 * With pitch == block_size, data followed by parity is exactly module/rs.c's shard order.
 * Bytes in [block_size, round_up(block_size, 16)) of a row may be read and written when
 * pitch allows (fast path); they are scratch.
 *
 * Arithmetic is bit-exact with module/rs.c (QFEC_CAUCHY) and module/fec.c / system/fec.c
 * (QFEC_VANDERMONDE), including rs.c's column-0 zero-coefficient behaviour when a code is
 * built with rs_stale_quirk = 1 (the default for QFEC_CAUCHY).
 *
 * All functions are thread-safe.  The device context of the calling thread's current HIP
 * device is created lazily, once.  `stream` is a hipStream_t passed as void* (NULL = the
 * null stream).  Return values: 0 or a negative QFEC_E* code.
 */
#ifndef QFEC_H
#define QFEC_H

#ifdef __cplusplus
extern "C" {
#endif

#define QFEC_CAUCHY 0      /* module/rs.c:437-440 parity rows (reed_solomon_new)   */
#define QFEC_VANDERMONDE 1 /* module/fec.c:653-707 parity rows (fec_new)          */

#define QFEC_OK 0
#define QFEC_EINVAL (-1)   /* bad argument / shape                                   */
#define QFEC_ENODEV (-2)   /* no HIP device                                          */
#define QFEC_EHIP (-3)     /* a HIP runtime call failed                              */
#define QFEC_ENOMEM (-4)   /* allocation failed                                      */
#define QFEC_EUNSUP (-5)   /* shape not supported by this entry point                */

#define QFEC_VARIANT_PERM 0    /* register byte-permute GF tables (v_perm_b32), default */
#define QFEC_VARIANT_LDSLOG 1  /* log/exp tables staged in LDS                          */

typedef struct qfec_code qfec_code;

/* A code over k data and m parity shards with the given parity-row flavour.
 * QFEC_CAUCHY: 1 <= k, 1 <= m, k + m <= 255 (rs.c:404).  QFEC_VANDERMONDE: 1 <= k,
 * 0 <= m, k + m <= 256 (fec.c:664).  NULL on error. */
qfec_code *qfec_code_new(int flavour, int k, int m);
/* A code over explicit m x k parity rows (row-major). */
qfec_code *qfec_code_from_rows(int k, int m, const unsigned char *parity_rows, int rs_stale_quirk);
void qfec_code_free(qfec_code *code);
int qfec_code_rows(const qfec_code *code, unsigned char *out_rows /* m*k */);
int qfec_code_shape(const qfec_code *code, int *k, int *m);

/* parity[g] = P x data[g] for every group g.  block_size >= 1, pitch >= block_size. */
int qfec_encode(qfec_code *code, const unsigned char *d_data, unsigned char *d_parity,
                long long groups, int block_size, long long pitch, void *stream);

/* qfec_encode on HOST buffers (the network path starts and ends in host memory).  Pinned
 * buffers the device can address (hipHostMalloc'd, or registered mapped) are read and written
 * in place by one launch over PCIe ("zero copy"); pageable ones run in ~32 MiB chunks over two
 * internal streams, staged through pinned memory, H2D -> encode -> D2H of one chunk overlapping
 * the staging of the next.  Returns after the parity is in h_parity.  Layouts as qfec_encode. */
int qfec_encode_host(qfec_code *code, const unsigned char *h_data, unsigned char *h_parity,
                     long long groups, int block_size, long long pitch);

/* qfec_reconstruct on HOST buffers: h_data is rewritten in place, h_marks is in the rs.c
 * layout over all `groups` (G*k data marks, then G*m parity marks); *failed (may be NULL) =
 * groups left under-determined.  k + m <= 24.  Pinned data and parity are worked on in place
 * (zero copy: the survivors are read and only the erased rows written, over PCIe; the marks are
 * staged); otherwise chunked and staged like qfec_encode_host. */
int qfec_reconstruct_host(qfec_code *code, unsigned char *h_data, const unsigned char *h_parity,
                          const unsigned char *h_marks, long long groups, int block_size, long long pitch,
                          long long *failed);

/* ---- host streaming pipe (BASELINE config 5: mixed (k,m) batches host -> device -> host) ----
 * A pipe owns `nstreams` slots per device (HIP stream + event + `slot_bytes` of device
 * staging), over the listed devices (devices = NULL / ndev = 0: every visible device;
 * a device may be listed more than once).  qfec_pipe_encode / qfec_pipe_reconstruct split a
 * batch into pieces that fit a slot and spread over all slots; each piece takes the next
 * slot round-robin (devices interleaved), waits for that slot's previous piece, and queues
 * its kernel on the pinned buffers in place (zero copy; only the piece's marks are staged)
 * -- or, with qfec_tune("host_zero_copy", 0) or a device that cannot address the buffers,
 * H2D -> kernel -> D2H through the slot's staging -- so the pieces overlap each other.  They return once the pieces are queued.  Host buffers must be
 * PINNED (hipHostMalloc'd or hipHostRegister'ed; DMA'd directly) and must not be touched
 * until qfec_pipe_wait returns.  Layouts as qfec_encode / qfec_reconstruct_host (marks in
 * the rs.c layout over the batch's `groups`).  Any number of codes may share a pipe.
 * qfec_pipe_wait: every queued piece has finished; *failed (may be NULL) = under-determined
 * groups since the previous wait.  On an error return the pipe has been drained. */
typedef struct qfec_pipe qfec_pipe;
qfec_pipe *qfec_pipe_new(const int *devices, int ndev, int nstreams, long long slot_bytes);
void qfec_pipe_free(qfec_pipe *pipe);
int qfec_pipe_encode(qfec_pipe *pipe, qfec_code *code, const unsigned char *h_data, unsigned char *h_parity,
                     long long groups, int block_size, long long pitch);
int qfec_pipe_reconstruct(qfec_pipe *pipe, qfec_code *code, unsigned char *h_data, const unsigned char *h_parity,
                          const unsigned char *h_marks, long long groups, int block_size, long long pitch);
int qfec_pipe_wait(qfec_pipe *pipe, long long *failed);
int qfec_pipe_slots(const qfec_pipe *pipe);

/* Rewrite every erased data shard from k survivors: the surviving data shards in
 * ascending order, then the first e surviving parity shards in ascending order
 * (module/rs.c:620-629; the same set network/NetFecCodec.cpp:504-528 hands to
 * fec_decode).  Groups with no erased data are untouched; groups with more erased data
 * than surviving parity are untouched and counted into *d_failed (device counter,
 * may be NULL; accumulated, not reset).  k + m <= 24: asynchronous on `stream`, erasure
 * pattern -> decode matrix through a device LUT.  k + m > 24: the marks are read back
 * (k + m bytes per group), decode records are built per distinct pattern on the host,
 * and the call returns after the kernel has run on `stream`. */
int qfec_reconstruct(qfec_code *code, unsigned char *d_data, const unsigned char *d_parity,
                     const unsigned char *d_marks, long long groups, int block_size,
                     long long pitch, unsigned int *d_failed, void *stream);

/* Build the per-erasure-pattern decode tables of `code` on the current device now
 * (otherwise done on the first qfec_reconstruct). */
int qfec_prepare_reconstruct(qfec_code *code);

/* qfec_encode and qfec_reconstruct on shards SCATTERED in device memory, for callers that hold one
 * buffer per packet (module/rs.h's `unsigned char **shards`).  d_shards is a DEVICE array of
 * groups * (k + m) device pointers in rs.c's shard order (rs.c:578-586, what reed_solomon_encode
 * receives): the groups * k data shards first, group-major, then the groups * m parity shards.
 * d_marks is the rs.c marks layout, as for qfec_reconstruct.  Every shard is exactly block_size
 * bytes: there is no pitch and there are NO scratch bytes -- no byte outside [0, block_size) of any
 * shard is read or written (the next byte may belong to someone else's packet).
 *   Encode results: qfec_encode_ptrs writes, into the parity shards, exactly the bytes qfec_encode
 *     writes for the same rows laid out contiguously: the same tables, the rs.c column-0 stale-row
 *     quirk included (a flagged row starts from the destination's previous bytes).
 *   Reconstruct results: qfec_reconstruct_ptrs rewrites the marked data shards exactly as
 *     qfec_reconstruct does: the same survivor rule, decode records, quirk and *d_failed accounting
 *     (nullable, accumulated).  Groups with no erased data are untouched; under-determined groups
 *     are untouched and counted.
 *   Any alignment: shards may start at any byte, block_size may be any value >= 1.  A group all of
 *     whose k + m pointers are 16-B aligned runs 16-byte (reconstruct of k >= 10: 8-byte) accesses;
 *     any other group is worked on byte by byte, much slower.
 *   Aliasing: shards that are only read may alias each other or repeat (a shared padding shard).  A
 *     shard the call writes -- the parity in encode, the marked data in reconstruct -- must not
 *     overlap any other shard of the batch, or the result is undefined.
 *   Asynchronous on `stream`: no host synchronisation, no read-back.  The pointer table and the
 *     marks must stay valid until the work has run.
 *   qfec_reconstruct_ptrs uses the device LUT qfec_reconstruct uses (built on the first call or by
 *     qfec_prepare_reconstruct).  k + m > 24 returns QFEC_EUNSUP: there is no host-record path
 *     here.  qfec_encode_ptrs takes any code qfec_code_new accepts.  Batches beyond the 32-bit
 *     index space of a launch are cut into several launches by the host, as elsewhere.
 *   QFEC_EINVAL, decided on the host before a device is touched, the cause named in
 *     qfec_last_error: a null code, groups < 0, block_size < 1, a null d_shards with groups > 0, a
 *     null d_marks with groups > 0.  groups == 0 (or m == 0 for the encode) returns QFEC_OK and
 *     launches nothing.
 *   qfec_set_kernel_variant does not apply: always the perm-table kernels. */
int qfec_encode_ptrs(qfec_code *code, unsigned char *const *d_shards,
                     long long groups, int block_size, void *stream);
int qfec_reconstruct_ptrs(qfec_code *code, unsigned char *const *d_shards,
                          const unsigned char *d_marks, long long groups, int block_size,
                          unsigned int *d_failed, void *stream);

/* The pointer-table calls on shards that each have their OWN LENGTH: the packets of a FEC group as
 * they lie, with no copy into zero-padded slots.  A data shard shorter than its group counts as
 * zero-filled up to the group's length, and parity covers the group's longest shard only -- the
 * reference's groupMaxPktSize (network/FecCodecBuf.cpp:137-156, fec_decode_pkts(.., maxSize)
 * :197-206).  d_shards and d_marks are exactly those of qfec_encode_ptrs / qfec_reconstruct_ptrs:
 * shard order, marks layout, any alignment and the aliasing rule carry over.  d_lens: DEVICE array of
 * groups * k ints, the length of every data shard in table order.  max_len >= 1 is the longest
 * length any group may have; it only sizes the launch.  Asynchronous on `stream`, no read-back; the
 * tables must stay valid until the work has run.  Codes as for the fixed-length calls: any code for
 * the encode; k + m <= 24 for the reconstruct through the same device LUT (QFEC_EUNSUP above that,
 * qfec_prepare_reconstruct applies).
 *   Encode, per group g, len_i = d_lens[g*k + i] and L = max_i len_i:
 *     Void group: any len_i < 0 or > max_len (INT_MIN and INT_MAX included).  No byte of it is read
 *       or written, d_group_len[g] = -1 and *d_invalid gains 1.
 *     Empty group, L = 0: nothing is read or written, d_group_len[g] = 0.
 *     Otherwise d_group_len[g] = L, and bytes [0, L) of every parity shard become exactly what
 *       qfec_encode_ptrs with block_size = L writes for these shards zero-padded to L: the same
 *       tables, the rs.c column-0 stale-row quirk included (a flagged row starts from the
 *       destination's previous bytes).  Bytes [L, ...) of a parity shard are never written.
 *     Data shard i is read in [0, len_i) only: no byte at or past len_i is read on any path, and
 *       none influences a result.  A shard with len_i = 0 is never dereferenced (its table entry
 *       may be anything) and takes no part in the alignment judgement.
 *     d_group_len (groups ints, written) and d_invalid (one counter, accumulated, not reset) may
 *       be NULL.  A sender transmits d_group_len[g] bytes of each parity shard of group g.
 *   Reconstruct, per group g, L = d_group_len[g]: the length of the group's parity shards -- what
 *     the encode reported, what a receiver reads off a parity packet.
 *     Lengths are judged before marks.  The group is untouched and counted into *d_invalid (not
 *       into *d_failed) when L is outside [0, max_len] or an unmarked data shard has len_i outside
 *       [0, L].  Then an empty group, L = 0, is untouched and counted nowhere.
 *     The d_lens entry of a marked data shard is not looked at.  The shard has room for L bytes
 *       and exactly its bytes [0, L) are written.
 *     Otherwise the behaviour is that of qfec_reconstruct_ptrs with block_size = L on the
 *       zero-padded rows: the same survivor rule (all surviving data, then the first e surviving
 *       parity rows), records, quirk and *d_failed accounting; groups with no erased data are
 *       untouched; under-determined groups are untouched and counted into *d_failed.
 *     Surviving data shard i is read in [0, len_i), the parity survivors used in [0, L); nothing
 *       else is dereferenced.
 *   Alignment, per group: a group runs 16-byte (reconstruct of k >= 10: 8-byte) accesses over its
 *     whole columns when all of its table entries that the call may dereference are 16-B aligned;
 *     any other group is worked on byte by byte, much slower.
 *   QFEC_EINVAL, decided on the host before a device is touched, the cause named in
 *     qfec_last_error: a null code, groups < 0, max_len < 1, and with groups > 0 a null d_shards, a
 *     null d_lens, a null d_marks or (reconstruct only) a null d_group_len.  groups == 0 (or m == 0
 *     for the encode) returns QFEC_OK and launches nothing. */
int qfec_encode_ptrs_var(qfec_code *code, unsigned char *const *d_shards,
                         const int *d_lens, long long groups, int max_len,
                         int *d_group_len, unsigned int *d_invalid, void *stream);
int qfec_reconstruct_ptrs_var(qfec_code *code, unsigned char *const *d_shards,
                              const int *d_lens, const int *d_group_len,
                              const unsigned char *d_marks, long long groups, int max_len,
                              unsigned int *d_failed, unsigned int *d_invalid, void *stream);

/* Host-side decode-matrix query for one group (group-order marks[n]).  Writes e <= m
 * rows of k coefficients over the survivors listed in survivors[k] (shard ids 0..n-1).
 * Returns e, 0 when nothing is erased, or -1 when under-determined.  CPU only. */
int qfec_decode_rows(const qfec_code *code, const unsigned char *marks_n,
                     unsigned char *rows_out, int *survivors_out, int *erased_out);

/* Bring every group back to full strength in one launch: rewrite every marked shard, data AND
 * parity, from the k lowest unmarked shards (all surviving data, then the first e surviving parity
 * rows -- the set qfec_reconstruct uses; all of the data when no data shard is marked).  Layouts,
 * marks, pitch, stream and the scratch bytes in [block_size, round_up(block_size, 16)) are exactly
 * as for qfec_reconstruct; the one difference is that d_parity is written.  Per group, with t
 * marked shards of which e are data:
 *   t = 0   untouched.
 *   t > m   under-determined (e <= surviving parity holds exactly when t <= m): untouched and
 *           counted into *d_failed (device counter, may be NULL; accumulated, not reset).
 *   else    every marked data row is rewritten byte for byte as qfec_reconstruct rewrites it (the
 *           same decode rows, rs.c's stale-row quirk included); every marked parity row j becomes
 *           rows[j] x [identity on surviving data; the decode rows on erased data] applied to the
 *           survivors -- a true GF product, no stale-row semantics.
 * A repaired parity row equals what qfec_encode writes into it from the repaired data whenever no
 * quirk-stale coefficient is involved (a zero column-0 coefficient of that parity row or of a
 * decode row, with rs_stale_quirk = 1).  Codes from qfec_code_new have none, so there it always
 * does; codes with edited or explicit rows may differ in exactly those rows.
 * No other byte of data or parity is written.  Always the perm-table kernels
 * (qfec_set_kernel_variant does not apply).  Asynchronous on `stream`; the pattern -> rows LUT
 * (2^(k+m) entries, keyed by the whole mask) is built on the first call or by qfec_prepare_repair.
 * k + m > 24 returns QFEC_EUNSUP: there is no host-record path for repair. */
int qfec_repair(qfec_code *code, unsigned char *d_data, unsigned char *d_parity,
                const unsigned char *d_marks, long long groups, int block_size,
                long long pitch, unsigned int *d_failed, void *stream);
int qfec_prepare_repair(qfec_code *code);

/* Host-side repair-matrix query for one group (group-order marks[n]): t <= m rows of k coefficients
 * over the survivors listed in survivors[k] (the k lowest unmarked ids), one row per marked shard
 * in lost[t] (ids 0..n-1 ascending: data rows first, then parity rows k + j).  Returns t, 0 when
 * nothing is marked, or -1 when under-determined.  Any k + m.  CPU only, like qfec_decode_rows. */
int qfec_repair_rows(const qfec_code *code, const unsigned char *marks_n,
                     unsigned char *rows_out /* t*k */, int *survivors_out /* k */,
                     int *lost_out /* t */);

/* Device-built decode plans: reconstruct and repair for ANY k + m, asynchronously.  The calls above
 * take a group's decode matrix from a host-built table of 2^(k+m) entries (k + m <= 24), or, in
 * qfec_reconstruct above that, from host inversions after a read-back of the marks.  Here the plan
 * of every group is computed on the device from the group's marks, on the caller's stream: no LUT,
 * no qfec_prepare_*, no read-back, no host synchronisation, no k + m limit.
 *   Codes: any code qfec_code_new or qfec_code_from_rows accepts, narrow ones (k + m <= 24) included.
 *     QFEC_EUNSUP for a code that carries an rs.c decode matrix (qfec_rs_code of a handle) which is
 *     not [I; rows], i.e. an edited handle: rs.c's decode with a partially inverted matrix is not
 *     reproduced here.  Checked on the host, once per version of the code.
 *   Marks, layouts, pitch, stream and the scratch bytes in [block_size, round_up(block_size, 16)) are
 *     exactly those of qfec_reconstruct / qfec_repair.  16-byte lanes when both bases and the pitch
 *     allow, else byte by byte.  Batches beyond the 32-bit index space of a launch are cut into
 *     several launches by the host, as elsewhere.
 *   Per group in mode QFEC_PLAN_RECONSTRUCT, with e marked data shards: e = 0 untouched; e greater
 *     than the surviving parity: untouched and counted into *d_failed (device counter, may be NULL;
 *     accumulated, not reset); else every marked data row is rewritten exactly as qfec_reconstruct
 *     rewrites it: the same survivor rule (rs.c:620-629), the same rows, and the column-0 stale-row
 *     quirk when the code has rs_stale_quirk.
 *   Per group in mode QFEC_PLAN_REPAIR, with t marked shards: t = 0 untouched; t > m untouched and
 *     counted; else data rows as above, and marked parity rows as true GF products, exactly as
 *     qfec_repair / qfec_repair_rows define them.
 *   A group whose survivor matrix is singular (explicit rows that are not MDS) is untouched and
 *     counted, in either mode.
 *   The plan of a group, qfec_plan_stride(code) bytes, public and fixed:
 *       [0]   u16 t (rows to write), u16 e (of them erased data), u8 status (0 nothing to do, 1 work,
 *             2 failed), pad to 16 bytes
 *       [16]  k survivor ids (u8: the k lowest unmarked ids)
 *             m lost ids (u8, the first t valid: data ascending, then parity as k + j; mode
 *             RECONSTRUCT lists data only)
 *             m stale flags (u8, 1: the row starts from the destination's previous bytes)
 *       from the next 16-byte boundary: m x k coefficient bytes, the first t x k valid -- row j over the
 *             survivors in the order listed
 *       padded to a multiple of 16; every unused byte is zero.  With status 0 or 2 only t, e and the
 *       status are set.
 *   qfec_plan_build writes the plans of `groups` groups and counts the failed ones into *d_failed;
 *     qfec_plan_apply executes plans on a batch and counts nothing.  It reads only the plan, never
 *     the marks, so one plan may be applied to any number of batches with the same losses.  d_parity
 *     is written only where the plan lists parity rows: under a RECONSTRUCT plan it is only read.  A
 *     buffer that qfec_plan_build did not write is not a plan, and applying it is undefined.
 *   d_plan must be 16-byte aligned (the stride is a multiple of 16, so every group's plan then is):
 *     plans are written 16 bytes at a time and read as dwords.  Unlike a misaligned data base, which
 *     only selects the byte path, a misaligned d_plan is refused with QFEC_EINVAL.
 *   qfec_reconstruct_wide / qfec_repair_wide are qfec_plan_build into stream-ordered scratch followed
 *     by qfec_plan_apply; the scratch is freed on the stream.  A batch is cut into launches so that
 *     one chunk's plans stay under 64 MiB.
 *   QFEC_EINVAL, decided on the host before a device is touched, the cause named in
 *     qfec_last_error: a null code, groups < 0, block_size < 1, pitch < block_size, mode not 0 or 1, a
 *     null buffer with groups > 0 (d_failed may be NULL), a d_plan that is not 16-byte aligned.  groups == 0 returns QFEC_OK and launches
 *     nothing.  Always the perm-table kernels (qfec_set_kernel_variant does not apply). */
#define QFEC_PLAN_RECONSTRUCT 0   /* qfec_reconstruct's rule: erased data rows only            */
#define QFEC_PLAN_REPAIR      1   /* qfec_repair's rule: every marked shard, data and parity   */
long long qfec_plan_stride(const qfec_code *code);          /* bytes per group, a multiple of 16 */
int qfec_plan_build(qfec_code *code, const unsigned char *d_marks, long long groups, int mode,
                    unsigned char *d_plan /* [groups][stride] */, unsigned int *d_failed, void *stream);
int qfec_plan_apply(qfec_code *code, unsigned char *d_data, unsigned char *d_parity,
                    const unsigned char *d_plan, long long groups, int block_size, long long pitch,
                    void *stream);
int qfec_reconstruct_wide(qfec_code *code, unsigned char *d_data, const unsigned char *d_parity,
                          const unsigned char *d_marks, long long groups, int block_size,
                          long long pitch, unsigned int *d_failed, void *stream);
int qfec_repair_wide(qfec_code *code, unsigned char *d_data, unsigned char *d_parity,
                     const unsigned char *d_marks, long long groups, int block_size,
                     long long pitch, unsigned int *d_failed, void *stream);
/* The plan of one group (group-order marks[n]) in the same layout, stride bytes.  Any k + m.  CPU
 * only, like qfec_repair_rows; QFEC_EINVAL / QFEC_EUNSUP as above. */
int qfec_plan_build_host(const qfec_code *code, const unsigned char *marks_n, int mode,
                         unsigned char *out_plan /* stride bytes */);

/* Device plans on shards SCATTERED in device memory: reconstruct AND repair on a pointer table, at
 * any k + m.  The join of the two families above: the table, the marks and the shard rules are those
 * of qfec_reconstruct_ptrs; the plans, the codes and the per-group results are those of
 * qfec_plan_build / qfec_plan_apply / qfec_reconstruct_wide / qfec_repair_wide.
 *   Table and marks: d_shards is a DEVICE array of groups * (k + m) device pointers in rs.c's shard
 *     order (all data shards group-major, then all parity shards), d_marks the rs.c marks layout.
 *   Shards: every shard is exactly block_size bytes at any alignment; no pitch, NO scratch bytes: no
 *     byte outside [0, block_size) of any shard is read or written.
 *   Codes: every code the plan calls accept, any k + m up to 256, narrow codes included.  QFEC_EUNSUP
 *     only for an edited reed_solomon handle, as there.
 *   Results: per group exactly those of qfec_plan_apply / qfec_reconstruct_wide / qfec_repair_wide on
 *     the same rows laid out contiguously: the survivor rule (the k lowest unmarked ids), the same
 *     coefficient bytes, the column-0 stale-row quirk (a flagged row starts from the destination's
 *     previous bytes); status 0 groups and failed groups untouched, a singular group untouched and
 *     counted.  qfec_plan_apply_ptrs counts nothing and never reads marks, so one plan (from
 *     qfec_plan_build, 16-byte aligned, else QFEC_EINVAL) serves any number of tables.  The one-shot
 *     calls count failed groups into *d_failed (device counter, may be NULL; accumulated, not reset).
 *   Untouched shards: a shard the plan neither reads (it is not one of the k survivors) nor writes (it
 *     is not in the lost list) is never dereferenced; its table entry still takes part in the
 *     alignment judgement.
 *   Alignment, judged per group on the device: a group all of whose k + m table entries are 16-B
 *     aligned runs 16-byte lanes over its whole columns and the block_size % 16 tail bytes byte by
 *     byte; any other group is worked on byte by byte, much slower.
 *   Aliasing: shards that are only read may alias each other or repeat.  A shard the call writes must
 *     not overlap any other shard of the batch, or the result is undefined.
 *   Asynchronous on `stream`: no host synchronisation, no read-back.  The one-shot calls are
 *     qfec_plan_build into stream-ordered scratch followed by qfec_plan_apply_ptrs, in chunks of at
 *     most 64 MiB of plans; the scratch is freed on the stream.
 *   Narrow codes (k + m <= 24): qfec_reconstruct_ptrs, which reads a prebuilt LUT and keeps the
 *     survivors in registers, is the faster call there (DESIGN section 18 has the measured ratio);
 *     qfec_reconstruct_ptrs_wide gives the same bytes and is the call for repair on pointers.
 *   QFEC_EINVAL, decided on the host before a device is touched, the cause named in
 *     qfec_last_error after the call's name: a null code, groups < 0, block_size < 1, a null d_shards /
 *     d_marks / d_plan with groups > 0, a d_plan that is not 16-byte aligned.  groups == 0 returns
 *     QFEC_OK and launches nothing. */
int qfec_plan_apply_ptrs(qfec_code *code, unsigned char *const *d_shards, const unsigned char *d_plan,
                         long long groups, int block_size, void *stream);
int qfec_reconstruct_ptrs_wide(qfec_code *code, unsigned char *const *d_shards,
                               const unsigned char *d_marks, long long groups, int block_size,
                               unsigned int *d_failed, void *stream);
int qfec_repair_ptrs_wide(qfec_code *code, unsigned char *const *d_shards,
                          const unsigned char *d_marks, long long groups, int block_size,
                          unsigned int *d_failed, void *stream);

/* The plan calls on pointer tables where every shard has its OWN LENGTH: reconstruct AND repair of
 * ragged packets where they lie, at any k + m.  d_shards and d_marks are those of
 * qfec_reconstruct_ptrs_wide (rs.c shard order, any alignment, no pitch, read-only shards may alias);
 * d_lens (groups * k ints, table order), d_group_len (groups ints: the length of each group's parity
 * shards) and max_len >= 1 are those of qfec_reconstruct_ptrs_var; d_plan is a plan of either mode
 * from qfec_plan_build, 16-byte aligned.  Codes: those the plan calls accept, any k + m up to 256,
 * narrow codes included; QFEC_EUNSUP only for an edited reed_solomon handle.  Asynchronous on
 * `stream`, no read-back.
 *   qfec_plan_apply_ptrs_var, per group g, L = d_group_len[g]:
 *     The plan's status is looked at first.  Status 2 (failed): the group is untouched, its lengths
 *       are not judged, and this call counts it nowhere -- the build counted it.
 *     Then the lengths, for status 0 and 1 alike: the group is invalid when L is outside
 *       [0, max_len] or an unmarked data shard has len_i outside [0, L] (INT_MIN and INT_MAX
 *       included).  An invalid group is untouched and *d_invalid gains 1 (device counter, may be
 *       NULL; accumulated, not reset).
 *     The apply reads no marks: a data shard is unmarked exactly when its id is not among the
 *       first t entries of the plan's lost list, which for status 0 and 1 equals the marks the plan
 *       was built from, in both modes (a status-0 plan has t = 0: every data shard is unmarked).
 *       The d_lens entry of a listed data shard is not looked at.
 *     Status 0, or L = 0: untouched, counted nowhere.
 *     Otherwise the group behaves as qfec_plan_apply_ptrs with block_size = L on the same rows with
 *       every surviving data shard zero-padded to L: the same survivors, coefficient bytes and stale
 *       flags (a stale row starts from the destination's previous bytes in [0, L)).  Each of the t
 *       listed shards, data or parity, has room for L bytes and exactly its bytes [0, L) are
 *       written.  A surviving data shard i is read in [0, len_i) only, a surviving parity shard in
 *       [0, L).  A survivor with len_i = 0, and any shard the plan neither reads nor writes, is never
 *       dereferenced: its table entry may be anything.  No byte at or past len_i of a data survivor
 *       is read on any path; no byte at or past L of any shard is written.
 *   Alignment, judged per group on the device on the entries the plan dereferences (the survivors
 *     of non-zero readable length and the listed shards): when all of them are 16-B aligned the
 *     group runs 16-byte lanes over its whole columns and the L % 16 tail byte by byte; any other
 *     group is worked on byte by byte, much slower.
 *   qfec_reconstruct_ptrs_wide_var / qfec_repair_ptrs_wide_var are qfec_plan_build (mode RECONSTRUCT /
 *     REPAIR) into stream-ordered scratch followed by qfec_plan_apply_ptrs_var, in chunks of at most
 *     64 MiB of plans; the scratch is freed on the stream.
 *   Counters: *d_failed is the build's count and comes from the marks alone (t > m, e greater than
 *     the surviving parity, a singular group); *d_invalid is the apply's.  A group is never in both.
 *     This DEVIATES from qfec_reconstruct_ptrs_var, which judges lengths before marks and leaves an
 *     empty group before it looks at the marks: a group that is both under-determined and badly
 *     sized counts as failed here and as invalid there, and an under-determined group with L = 0
 *     counts as failed here and nowhere there.  In every other case the two calls count alike.
 *   QFEC_EINVAL, decided on the host before a device is touched, the cause named in
 *     qfec_last_error after the call's name: a null code, groups < 0, max_len < 1, with groups > 0 a
 *     null d_shards, d_lens, d_group_len or d_marks / d_plan, a d_plan that is not 16-byte aligned.
 *     groups == 0 returns QFEC_OK and launches nothing; a bad argument still wins over that. */
int qfec_plan_apply_ptrs_var(qfec_code *code, unsigned char *const *d_shards,
                             const int *d_lens, const int *d_group_len,
                             const unsigned char *d_plan, long long groups, int max_len,
                             unsigned int *d_invalid, void *stream);
int qfec_reconstruct_ptrs_wide_var(qfec_code *code, unsigned char *const *d_shards,
                                   const int *d_lens, const int *d_group_len,
                                   const unsigned char *d_marks, long long groups, int max_len,
                                   unsigned int *d_failed, unsigned int *d_invalid, void *stream);
int qfec_repair_ptrs_wide_var(qfec_code *code, unsigned char *const *d_shards,
                              const int *d_lens, const int *d_group_len,
                              const unsigned char *d_marks, long long groups, int max_len,
                              unsigned int *d_failed, unsigned int *d_invalid, void *stream);

/* Does the parity match the data?  Bit j of d_bad_rows[g] is set iff parity row j of group g
 * differs from rows[j] x data[g] (a true GF product) in any byte of [0, block_size); 0 = the group
 * is consistent.  d_bad_rows ([groups], may be NULL) is written for every group; *d_bad_groups
 * (device counter, may be NULL; accumulated, not reset) gains 1 per group with any bad row.  Bytes
 * in [block_size, pitch) of either buffer never influence the result.  Reads (k + m) rows per
 * group, writes nothing else; asynchronous on `stream`.  m > 32 returns QFEC_EUNSUP. */
int qfec_verify(qfec_code *code, const unsigned char *d_data, const unsigned char *d_parity,
                long long groups, int block_size, long long pitch,
                unsigned int *d_bad_rows /* [groups], nullable */,
                unsigned int *d_bad_groups /* counter, accumulates, nullable */, void *stream);

/* Incremental parity: change part of a group that is already encoded without reading the rest of it.
 * Both calls rest on linearity, parity_j ^= rows[j][i] x (old_i ^ new_i).  All arithmetic is true
 * GF(2^8) products from the code's parity rows, as in qfec_verify and qfec_repair: there is no rs.c
 * stale-row quirk (the encode tables' flag word is ignored), so a zero coefficient contributes
 * nothing.  Layouts, pitch, stream and the 16-byte fast path against the byte path are exactly
 * qfec_encode's.  Bytes in [block_size, round_up(block_size, 16)) of a row a call writes are scratch
 * on the fast path; bytes from round_up(block_size, 16) to pitch, and every row a call does not
 * address, are never written.  Asynchronous on `stream`: no host synchronisation, no read-back, no
 * LUT, and no k + m limit (any code qfec_code_new accepts).  d_part / d_rows must not overlap d_parity
 * or d_data.
 * QFEC_EINVAL, decided on the host before a device is touched, with the cause in qfec_last_error: a
 * null code, first < 0, count < 1, first + count > k, groups < 0, block_size < 1, pitch < block_size,
 * accumulate not 0 or 1, a null buffer with groups > 0 (d_data and d_invalid may be NULL).
 * groups == 0 or m == 0 returns QFEC_OK and launches nothing.
 *
 * qfec_encode_update, the range form, for groups whose data arrives a few shards at a time:
 *   parity[g][j] (^)= sum_{c < count} rows[j][first + c] x part[g][c]   for every group g and row j
 * d_part holds only the `count` rows first .. first + count - 1 of every group.  accumulate = 1 XORs
 * into d_parity, 0 overwrites it.  first = 0, count = k, accumulate = 0 gives qfec_encode's parity for
 * any code without a quirk-stale coefficient; calling it over any partition of [0, k), the first
 * piece with accumulate = 0 (or onto zeroed parity) and the others with accumulate = 1, gives the same
 * parity in bytes [0, block_size).  Reads count (+ m with accumulate) rows per group, writes m. */
int qfec_encode_update(qfec_code *code, int first, int count,
                       const unsigned char *d_part   /* [groups][count][pitch] */,
                       unsigned char *d_parity       /* [groups][m][pitch]     */,
                       long long groups, int block_size, long long pitch,
                       int accumulate /* 1: XOR into d_parity, 0: overwrite it */, void *stream);

/* qfec_update, the per-group form, for small writes into stored groups: group g replaces ONE data
 * shard, i = d_shard[g].
 *   0 <= i < k   with delta = data[g][i] ^ rows[g] over [0, block_size), every parity row j gets
 *                parity[g][j] ^= rows[j][i] x delta, and data[g][i] becomes rows[g]: the parity is
 *                then what a fresh encode of the new data gives.
 *   i < 0        (QFEC_UPD_NONE) no byte of the group is written, and none of its rows is read.
 *   i >= k       the group is untouched and counted into *d_invalid (device counter, may be NULL;
 *                accumulated, not reset).  No table is ever indexed with such an id.
 * With d_data == NULL, d_rows[g] is the delta itself, computed elsewhere (for example on the node that
 * holds the data shard), and only the parity is written.  One shard per group per call: several
 * changed shards of a group are several stream-ordered calls.  A touched group costs 2 + m rows read
 * and 1 + m written (1 + m and m in delta mode) against the k + m of qfec_encode; an untouched group
 * costs one 4-byte read. */
#define QFEC_UPD_NONE (-1)
int qfec_update(qfec_code *code,
                const int *d_shard            /* [groups]: data shard id 0..k-1 replaced in group g; < 0 = group untouched */,
                unsigned char *d_data         /* [groups][k][pitch]; NULL: d_rows holds deltas */,
                const unsigned char *d_rows   /* [groups][pitch]: the new bytes of shard d_shard[g] (or the delta) */,
                unsigned char *d_parity       /* [groups][m][pitch] */,
                long long groups, int block_size, long long pitch,
                unsigned int *d_invalid       /* counter, accumulates, nullable */, void *stream);

/* Incremental parity on shards scattered in device memory: qfec_encode_update and qfec_update on the
 * table of qfec_encode_ptrs (groups * k data addresses, group-major, then groups * m parity addresses),
 * each with and without a length per shard.  For a sender whose packets arrive one at a time, ragged,
 * in their own buffers, and for a store that replaces one packet where it lies.  Common to all four:
 *   Arithmetic: true GF(2^8) products from the code's parity rows, as in qfec_encode_update; the rs.c
 *     stale-row quirk is never applied.  Any code qfec_code_new accepts: there is no k + m limit.
 *   Asynchronous on `stream`: no host synchronisation, no LUT, no scratch, no read-back.  A batch
 *     beyond one launch's index space goes in several launches.
 *   No byte outside a shard's stated extent is read or written on any path.
 *   A table entry a call does not address is never dereferenced, takes no part in the alignment
 *     judgement and may hold anything, so a sender can fill the table as packets arrive.
 *   Alignment, judged per group on the device on the entries the group may dereference: all of them
 *     16-B aligned, the group runs 16-byte lanes over its whole columns and the tail bytes byte by
 *     byte; any other group is worked on byte by byte, much slower.
 *   QFEC_EINVAL, decided on the host before a device is touched, the cause named in qfec_last_error
 *     after the call's name: a null code, first < 0, count < 1, first + count > k, groups < 0,
 *     block_size < 1 or max_len < 1, accumulate or delta_only not 0 or 1, and with groups > 0 a null
 *     d_shards, d_shard, d_new, d_lens, d_group_len or d_new_len where the call takes it (d_lens may be
 *     NULL in delta mode; d_invalid may always be NULL).  groups == 0 or m == 0 returns QFEC_OK and
 *     launches nothing; a bad argument still wins over that.
 *
 * qfec_encode_update_ptrs, the range form: for every group and parity row j
 *   parity_j[0, block_size) (^)= sum_{c < count} rows[j][first + c] x data_{first + c}[0, block_size)
 * It dereferences only the data entries first .. first + count - 1 and the m parity entries of a group.
 * accumulate = 1 XORs into the parity, 0 overwrites it.  Over any partition of [0, k), the first piece
 * overwriting and the others accumulating, bytes [0, block_size) of the parity are what
 * qfec_encode_ptrs writes, for codes without a quirk-stale coefficient.
 *
 * qfec_update_ptrs, the per-group form: d_new is a DEVICE array of `groups` addresses of block_size
 * bytes each, and i = d_shard[g] names the ONE data shard group g replaces.
 *   i < 0        nothing of the group is read or written: not d_new[g], not one of its table entries.
 *   i >= k       the group is untouched and counted once into *d_invalid (accumulated, not reset).  No
 *                table is indexed with such an id.
 *   otherwise    delta_only = 0: with delta = shard i ^ new, every parity shard has rows[j][i] x delta
 *                XORed in and shard i becomes new.  delta_only = 1: d_new[g] is the delta itself, no
 *                data entry is dereferenced and only the parity is written.
 * d_new[g] must not overlap a shard the call writes.
 *
 * qfec_encode_update_ptrs_var: the range form where part c of group g has d_lens[g*k + first + c] bytes
 * (d_lens holds groups * k ints; only the entries of the range are read) and L = d_group_len[g] is an
 * INPUT: the extent of the group's parity shards that the caller keeps, for example the MTU.
 *   Invalid group: L outside [0, max_len], or a length of the range outside [0, L] (INT_MIN and
 *     INT_MAX included).  It is untouched and counted once into *d_invalid.  A length outside the
 *     range is not looked at.  L = 0: nothing is dereferenced.
 *   A part is read in [0, len) only and counts as zero from there; a part of length 0 is never
 *     dereferenced.
 *   accumulate = 0: exactly [0, L) of every parity shard is written, zero past the longest part.
 *   accumulate = 1, e the longest part of the range: [0, e) is read and rewritten, [e, L) is neither
 *     read nor written.  Nothing at or past L is touched either way.
 *   Over any partition of [0, k), the first piece overwriting: [0, max_i len_i) is what
 *     qfec_encode_ptrs_var writes (codes without a quirk-stale coefficient), [max_i len_i, L) is zero,
 *     and qfec_verify_ptrs_var with this L reports 0.
 *
 * qfec_update_ptrs_var: the per-group form with i = d_shard[g], L = d_group_len[g], n = d_new_len[g]
 * the length of the new row and o = d_lens[g*k + i] the length shard i has now.  In delta mode o and
 * the data entry are not read (d_lens may be NULL) and e = n; else e = max(o, n).
 *   i < 0 and i >= k as for qfec_update_ptrs.  Invalid group, counted once: L outside [0, max_len], or
 *     n or o outside [0, L].  No other length of the group is read.
 *   Old is read in [0, o) and new in [0, n); both count as zero beyond.  [0, e) of every parity shard
 *     is read, XORed and rewritten; nothing at or past e is touched.  Exactly [0, n) of shard i is
 *     written: the shard must have room for n bytes, and its bytes [n, o) keep their old values -- they
 *     are past the new length.  n = 0: d_new[g] is never dereferenced; n = 0 and o = 0: a valid no-op.
 *   d_lens is const: other waves of the group read it during the launch.  THE CALLER stores n at
 *     d_lens[g*k + i] afterwards, stream-ordered, before the lengths are used again.
 *   If the parity equalled the encode of the zero-padded old data over [0, L), it now equals the
 *     encode of the zero-padded new data over [0, L). */
int qfec_encode_update_ptrs(qfec_code *code, int first, int count,
                            unsigned char *const *d_shards /* groups * (k + m) device addresses */,
                            long long groups, int block_size,
                            int accumulate /* 1: XOR into the parity, 0: overwrite it */, void *stream);
int qfec_update_ptrs(qfec_code *code, unsigned char *const *d_shards,
                     const int *d_shard                  /* [groups]: 0..k-1 replaced; < 0 = group untouched */,
                     const unsigned char *const *d_new   /* [groups] device addresses: the new rows (or the deltas) */,
                     int delta_only, long long groups, int block_size,
                     unsigned int *d_invalid             /* counter, accumulates, nullable */, void *stream);
int qfec_encode_update_ptrs_var(qfec_code *code, int first, int count, unsigned char *const *d_shards,
                                const int *d_lens       /* [groups * k] */,
                                const int *d_group_len  /* [groups], read */,
                                long long groups, int max_len, int accumulate,
                                unsigned int *d_invalid /* counter, accumulates, nullable */, void *stream);
int qfec_update_ptrs_var(qfec_code *code, unsigned char *const *d_shards,
                         const int *d_lens       /* [groups * k]; NULL allowed with delta_only = 1 */,
                         const int *d_group_len  /* [groups] */,
                         const int *d_shard      /* [groups] */,
                         const unsigned char *const *d_new /* [groups] device addresses */,
                         const int *d_new_len    /* [groups] */,
                         int delta_only, long long groups, int max_len,
                         unsigned int *d_invalid /* counter, accumulates, nullable */, void *stream);

/* Which shard is wrong?  qfec_verify says whether a group's parity matches its data; qfec_locate
 * names the ONE shard, data or parity, whose corruption explains the mismatch, so that it can be
 * marked for qfec_repair.  A code with m >= 2 parity rows has minimum distance m + 1 >= 3 and can
 * locate (and so correct) one corrupted shard per group.  Per byte position the syndromes are
 * s_j = parity_j ^ sum_i rows[j][i] x data_i; an error in data shard i gives
 * s_j = (rows[j][i] / rows[0][i]) x s_0 for every j, an error in parity row j0 gives s_j0 != 0 and
 * every other s_j = 0.  A shard is a candidate only if its relation holds in EVERY byte of
 * [0, block_size).  d_culprit[g] is written for every group:
 *   0 .. k+m-1          the one candidate (data shards 0..k-1, parity rows k..k+m-1)
 *   QFEC_LOC_CLEAN      every syndrome is zero: parity matches data
 *   QFEC_LOC_MULTI      inconsistent, and no single shard explains it (two or more corrupted shards)
 *   QFEC_LOC_AMBIGUOUS  more than one single shard explains it; only codes from explicit rows that
 *                       are not MDS (two proportional columns of [rows | I]) can give this
 * With m >= 3 (distance >= 4) two corrupted shards never pass for one.  With m = 2 they can: the
 * verdict for more than one corrupted shard is then undefined (a wrong id is possible), which is
 * inherent to a distance-3 code.
 * d_marks (rs.c layout, groups * (k + m) bytes, may be NULL) is written for every group: 1 at the
 * culprit, 0 everywhere else (all zero for CLEAN, MULTI and AMBIGUOUS groups), ready for
 * qfec_repair.  d_counts ([3], may be NULL; accumulated, not reset) gains 1 per located, MULTI and
 * AMBIGUOUS group.  Layouts, pitch, stream and the meaning of [block_size, pitch) are qfec_verify's:
 * bytes past block_size of either buffer never influence a result, and nothing in d_data / d_parity
 * is written.  Asynchronous on `stream`, no host synchronisation and no read-back; the per-group
 * working words come from stream-ordered scratch.  A consistent batch costs what qfec_verify costs
 * (reads (k + m) rows per group).  QFEC_EUNSUP, decided on the host before a device is touched:
 * m < 2; k > 32 or m > 32; any zero coefficient in the parity rows. */
#define QFEC_LOC_CLEAN     (-1)  /* parity matches data */
#define QFEC_LOC_MULTI     (-2)  /* inconsistent, and no single shard explains it */
#define QFEC_LOC_AMBIGUOUS (-3)  /* more than one single shard explains it (non-MDS explicit rows only) */
int qfec_locate(qfec_code *code, const unsigned char *d_data, const unsigned char *d_parity,
                long long groups, int block_size, long long pitch,
                int *d_culprit            /* [groups]: shard id 0..k+m-1, or QFEC_LOC_* */,
                unsigned char *d_marks    /* rs.c layout, groups*(k+m) bytes, nullable */,
                unsigned int *d_counts    /* [3] located, multi, ambiguous; accumulates; nullable */,
                void *stream);

/* qfec_locate into stream-ordered scratch marks, then qfec_repair with those marks, in one call: a
 * group with one corrupted shard is back to its original bytes in [0, block_size); CLEAN groups and
 * MULTI / AMBIGUOUS groups are untouched byte for byte (the latter are reported only, in d_culprit
 * ([groups], may be NULL) and d_counts ([3], may be NULL; accumulated)).  Asynchronous on `stream`
 * once the repair LUT exists (qfec_prepare_repair, or the first call).  QFEC_EUNSUP as for
 * qfec_locate, and for k + m > 24 (qfec_repair's limit), checked before anything is launched. */
int qfec_scrub(qfec_code *code, unsigned char *d_data, unsigned char *d_parity,
               long long groups, int block_size, long long pitch,
               int *d_culprit /* nullable */, unsigned int *d_counts /* [3], nullable */, void *stream);

/* The host-built constants of qfec_locate: r_{j,i} = rows[j][i] / rows[0][i] at
 * out[i*(m-1) + (j-1)], j = 1..m-1.  QFEC_EUNSUP as for qfec_locate.  CPU only, like
 * qfec_repair_rows. */
int qfec_locate_ratios(const qfec_code *code, unsigned char *out /* k*(m-1): r_{j,i} at [i*(m-1)+(j-1)] */);

/* The integrity family on pointer tables: qfec_verify, qfec_locate and a scrub on shards scattered
 * in device memory, without a copy into a contiguous batch.
 *   Table and shards: exactly qfec_encode_ptrs' -- groups * (k + m) device addresses, every group's
 *     k data shards first (group-major), then every group's m parity shards; every shard is exactly
 *     block_size bytes, at any alignment, and no byte outside [0, block_size) of a shard is read.
 *     qfec_verify_ptrs and qfec_locate_ptrs write nothing into any shard, so there shards may alias
 *     each other or repeat.  In qfec_scrub_ptrs a shard that gets rewritten must not overlap any other
 *     shard of the batch (qfec_repair_ptrs_wide's rule), or the result is undefined.
 *   Results: per group exactly those of the contiguous calls on the same rows laid out contiguously.
 *     qfec_verify_ptrs: d_bad_rows ([groups], may be NULL) holds qfec_verify's bits (a true GF
 *       product, no stale-row quirk) and is written for every group; *d_bad_groups (device counter,
 *       may be NULL; accumulated, not reset) gains 1 per inconsistent group, exactly once.  With both
 *       NULL the call returns QFEC_OK and launches nothing; with m == 0 every word is 0.
 *     qfec_locate_ptrs: d_culprit, d_marks and d_counts are what qfec_locate gives -- an id in
 *       0 .. k+m-1 or QFEC_LOC_CLEAN / QFEC_LOC_MULTI / QFEC_LOC_AMBIGUOUS, with its m = 2 caveat.
 *       d_marks (groups * (k + m) bytes, may be NULL) comes back in the table's own order and can be
 *       handed unchanged to qfec_repair_ptrs_wide.
 *     qfec_scrub_ptrs: qfec_locate_ptrs into stream-ordered scratch marks (the culprits too when
 *       d_culprit is NULL), then the repair qfec_repair_ptrs_wide runs with those marks.  A group with
 *       one corrupted shard is back to its original bytes; CLEAN, MULTI and AMBIGUOUS groups are
 *       untouched byte for byte; a located group whose plan is singular (explicit non-MDS rows only)
 *       is untouched and counted into *d_failed (device counter, may be NULL; accumulated).
 *   Codes: qfec_verify_ptrs takes any k with m <= 32, as qfec_verify (k + m may pass 64).
 *     qfec_locate_ptrs has qfec_locate's limits: m >= 2, k <= 32, m <= 32, no zero coefficient.
 *     qfec_scrub_ptrs takes the codes both its halves accept: qfec_locate's limits, and not a
 *     reed_solomon handle whose matrix was edited (the plan calls' refusal).  It has NO k + m <= 24
 *     limit, which is more than qfec_scrub offers: the repair goes through device-built plans, not
 *     the repair LUT.  QFEC_EUNSUP is decided on the host before a device is touched.
 *   Alignment, judged per group on the device: a group all of whose k + m table entries are 16-B
 *     aligned runs 16-byte lanes over its whole columns and the block_size % 16 tail bytes byte by
 *     byte; any other group is worked on byte by byte, much slower.
 *   Asynchronous on `stream`: no host synchronisation, no read-back; the per-group working words
 *     come from stream-ordered scratch.  A batch beyond one launch's index space goes in several.
 *   QFEC_EINVAL, decided on the host before a device is touched, the cause named in
 *     qfec_last_error after the call's name: a null code, groups < 0, block_size < 1, a null d_shards
 *     with groups > 0, and for qfec_locate_ptrs a null d_culprit with groups > 0.  groups == 0 returns
 *     QFEC_OK and launches nothing. */
int qfec_verify_ptrs(qfec_code *code, unsigned char *const *d_shards,
                     long long groups, int block_size,
                     unsigned int *d_bad_rows   /* [groups], nullable */,
                     unsigned int *d_bad_groups /* counter, accumulates, nullable */, void *stream);
int qfec_locate_ptrs(qfec_code *code, unsigned char *const *d_shards,
                     long long groups, int block_size,
                     int *d_culprit             /* [groups]: shard id 0..k+m-1, or QFEC_LOC_* */,
                     unsigned char *d_marks     /* rs.c layout, groups*(k+m) bytes, nullable */,
                     unsigned int *d_counts     /* [3] located, multi, ambiguous; accumulates; nullable */,
                     void *stream);
int qfec_scrub_ptrs(qfec_code *code, unsigned char *const *d_shards,
                    long long groups, int block_size,
                    int *d_culprit /* nullable */, unsigned int *d_counts /* [3], nullable */,
                    unsigned int *d_failed /* nullable, accumulates */, void *stream);

/* The integrity family on pointer tables with per-shard lengths: what a caller of
 * qfec_encode_ptrs_var asks afterwards -- does this group's parity still match, which packet is
 * corrupted, put it right -- on the packets where they lie, without a copy into padded slots.
 *   Arguments: d_shards is qfec_verify_ptrs' table.  d_lens holds groups * k ints in table order, the
 *     length of every data shard; d_group_len holds groups ints, the length L of each group's parity
 *     shards: what qfec_encode_ptrs_var reported and what a receiver reads off a parity packet.
 *     max_len >= 1 only sizes the launch.
 *   Data shard i of a group counts as zero-filled from len_i up to L.  It is read in [0, len_i) only
 *     and a parity shard in [0, L) only; no byte at or past those is read on any path and none
 *     influences a result.  A data shard with len_i == 0 is never dereferenced: its table entry may be
 *     anything and takes no part in the alignment judgement.
 *   An invalid group: L outside [0, max_len], or ANY data shard with len_i outside [0, L] (INT_MIN and
 *     INT_MAX included; all k lengths are judged, there are no marks).  No byte of it is read or
 *     written and *d_invalid (device counter, may be NULL; accumulated) gains 1, exactly once;
 *     d_bad_rows[g] = 0, d_culprit[g] = QFEC_LOC_INVALID, its marks are all zero, and it counts nowhere
 *     in d_counts or *d_bad_groups.  An empty group (L == 0) gives d_bad_rows[g] = 0 and
 *     QFEC_LOC_CLEAN with nothing dereferenced.
 *   qfec_verify_ptrs_var: d_bad_rows[g] is what qfec_verify_ptrs with block_size = L gives on the same
 *     shards with every data shard zero-padded to L (a true GF product, no stale-row quirk).  With
 *     d_bad_rows, d_bad_groups and d_invalid all NULL the call returns QFEC_OK and launches nothing.
 *   qfec_locate_ptrs_var: the verdict of qfec_locate_ptrs on the zero-padded rows, with one more
 *     condition on a data candidate.  A shorter shard is a stricter code: shard i is KNOWN to be zero
 *     in [len_i, L), so it cannot be wrong there, and it stays a candidate only if every syndrome is
 *     zero in every byte position >= len_i.  A group whose only padded-rows explanation is a data shard
 *     "wrong" beyond its own end is therefore QFEC_LOC_MULTI.  d_marks (may be NULL) comes back in the
 *     table's own order; it may go to qfec_repair_ptrs_wide_var only when the marked shard has room
 *     for L bytes (that call writes [0, L) of every listed shard) -- qfec_scrub_ptrs_var has no such
 *     condition.  d_counts and the m = 2 caveat are those of qfec_locate.
 *   qfec_scrub_ptrs_var: the locate into d_culprit (stream-ordered scratch when it is NULL), then one
 *     correction launch, which needs no plan: one located shard is fixed from one parity row.  A
 *     located data shard i has exactly its bytes [0, len_i) rewritten as (parity_0 ^ sum_{c != i}
 *     rows[0][c] x data_c) / rows[0][i], the other data read clipped to their lengths; a located parity
 *     shard j has exactly [0, L) rewritten as sum_c rows[j][c] x data_c.  No byte at or past len_i of
 *     a data culprit or past L of a parity culprit is written; CLEAN, MULTI, AMBIGUOUS, INVALID and
 *     empty groups are untouched byte for byte.  With all lengths equal this is byte for byte what
 *     qfec_scrub_ptrs writes.  A rewritten shard must not overlap any other shard of the batch.
 *   Codes: qfec_verify_ptrs_var takes any k with m <= 32.  qfec_locate_ptrs_var and
 *     qfec_scrub_ptrs_var have qfec_locate's limits (m >= 2, k <= 32, m <= 32, no zero coefficient).
 *     The scrub has NO k + m <= 24 limit and does not refuse an edited reed_solomon handle: it uses
 *     only the parity rows the locate judged with.  QFEC_EUNSUP is decided on the host before a device
 *     is touched.
 *   Alignment, judged per group on the device on the entries the call may dereference: an aligned
 *     group runs 16-byte lanes over its whole columns and the L % 16 tail bytes byte by byte; any
 *     other group is worked on byte by byte, much slower.
 *   Asynchronous on `stream`: no host synchronisation, no read-back; working words come from
 *     stream-ordered scratch.  A batch beyond one launch's index space goes in several.
 *   QFEC_EINVAL, decided on the host first, the cause named in qfec_last_error after the call's name:
 *     a null code, groups < 0, max_len < 1, with groups > 0 a null d_shards, d_lens or d_group_len,
 *     and for qfec_locate_ptrs_var a null d_culprit.  groups == 0 returns QFEC_OK and launches
 *     nothing; a bad argument still wins over that. */
#define QFEC_LOC_INVALID (-6)   /* the group's lengths are out of range: nothing of it was read */

int qfec_verify_ptrs_var(qfec_code *code, unsigned char *const *d_shards,
                         const int *d_lens, const int *d_group_len,
                         long long groups, int max_len,
                         unsigned int *d_bad_rows   /* [groups], nullable */,
                         unsigned int *d_bad_groups /* counter, accumulates, nullable */,
                         unsigned int *d_invalid    /* counter, accumulates, nullable */, void *stream);
int qfec_locate_ptrs_var(qfec_code *code, unsigned char *const *d_shards,
                         const int *d_lens, const int *d_group_len,
                         long long groups, int max_len,
                         int *d_culprit, unsigned char *d_marks /* nullable */,
                         unsigned int *d_counts /* [3], nullable */,
                         unsigned int *d_invalid /* nullable */, void *stream);
int qfec_scrub_ptrs_var(qfec_code *code, unsigned char *const *d_shards,
                        const int *d_lens, const int *d_group_len,
                        long long groups, int max_len,
                        int *d_culprit /* nullable */, unsigned int *d_counts /* [3], nullable */,
                        unsigned int *d_invalid /* nullable */, void *stream);

/* Which TWO shards are wrong?  qfec_locate stops at one corrupted shard per group and calls the rest
 * MULTI.  A code with m >= 4 parity rows has minimum distance m + 1 >= 5 and determines two corrupted
 * shards uniquely.  With H = [rows | I_m], h_x = column x of the parity rows for a data shard x < k
 * and the unit vector e_j for parity row x = k + j, and the syndromes s of qfec_locate (true GF
 * products, no rs.c stale-row quirk), a pair {a, b}, a < b, is a candidate iff s lies in
 * span{h_a, h_b} at EVERY byte of [0, block_size).  d_culprit has two slots per group:
 *   consistent                               QFEC_LOC_CLEAN, QFEC_LOC_CLEAN
 *   one corrupted shard                      its id exactly as qfec_locate gives it, QFEC_LOC_CLEAN
 *   qfec_locate says MULTI, one candidate    a, b
 *   qfec_locate says MULTI, no candidate     QFEC_LOC_MULTI, QFEC_LOC_MULTI
 *   qfec_locate says MULTI, several          QFEC_LOC_AMBIGUOUS, QFEC_LOC_AMBIGUOUS
 * Several candidate pairs can only happen for explicit rows of distance exactly 4, or for three or
 * more corrupted shards at m = 4.  With m >= 5 (distance >= 6) three corrupted shards are never taken
 * for two: the verdict is MULTI.  With m = 4 (distance 5) the verdict for three or more corrupted
 * shards is undefined (a wrong pair is possible), as for m = 2 in qfec_locate.
 * d_marks (rs.c layout, groups * (k + m) bytes, may be NULL) is written for every group: 1 at each
 * culprit, 0 everywhere else, ready for qfec_repair.  d_counts ([4], may be NULL; accumulated, not
 * reset) gains 1 per group with one culprit, with two, per MULTI and per AMBIGUOUS group.  Layouts,
 * pitch, the 16-byte fast path and the byte path, launch chunking and the stream are qfec_locate's;
 * bytes in [block_size, pitch) never count and nothing in d_data / d_parity is written.
 * Asynchronous on `stream`, no host synchronisation and no read-back; the working memory comes from
 * stream-ordered scratch.  A consistent batch costs qfec_locate's time plus four small launches;
 * only the groups qfec_locate calls MULTI are read a second time (one wave each, every pair of
 * shards tested against the recomputed syndromes).
 * QFEC_EUNSUP, decided on the host before a device is touched, with the cause in qfec_last_error:
 * everything qfec_locate refuses; m < 4; k + m > 24; some three columns of H linearly dependent (the
 * code's distance is then below 4, and one and two corrupted shards cannot be told apart).  Codes
 * from qfec_code_new never hit the last case, and a code that passes it cannot give AMBIGUOUS from
 * the single-shard stage.  At most 2^32 - 1 groups per call. */
int qfec_locate2(qfec_code *code, const unsigned char *d_data, const unsigned char *d_parity,
                 long long groups, int block_size, long long pitch,
                 int *d_culprit          /* [groups][2]: shard ids a < b, or QFEC_LOC_* */,
                 unsigned char *d_marks  /* rs.c layout, groups*(k+m) bytes, nullable */,
                 unsigned int *d_counts  /* [4] one, two, multi, ambiguous; accumulates; nullable */,
                 void *stream);

/* qfec_locate2 into stream-ordered scratch marks, then qfec_repair with those marks, in one call:
 * groups with one or two corrupted shards are back to their original bytes in [0, block_size);
 * CLEAN, MULTI and AMBIGUOUS groups are untouched byte for byte (the latter two are reported only,
 * in d_culprit ([groups][2], may be NULL) and d_counts ([4], may be NULL; accumulated)).
 * Asynchronous on `stream` once the repair LUT exists (qfec_prepare_repair, or the first call).
 * QFEC_EUNSUP as for qfec_locate2, checked before anything is launched. */
int qfec_scrub2(qfec_code *code, unsigned char *d_data, unsigned char *d_parity,
                long long groups, int block_size, long long pitch,
                int *d_culprit /* [groups][2], nullable */, unsigned int *d_counts /* [4], nullable */,
                void *stream);

/* The host-built constants of qfec_locate2 for the pair {a, b}: m - 2 rows F (out[r*m + j]) of rank
 * m - 2 with F x h_a = 0 and F x h_b = 0, the left null space of [h_a h_b] in the basis the device
 * constants are derived from: with p0 < p1 the first two rows on which [h_a h_b] is invertible, the
 * row of every other j has 1 at j and the coefficients of s_p0 and s_p1 that predict s_j.  Returns
 * m - 2.  QFEC_EINVAL for a = b or ids outside 0..k+m-1; QFEC_EUNSUP as for qfec_locate2.  CPU only,
 * like qfec_locate_ratios. */
int qfec_locate2_checks(const qfec_code *code, int a, int b, unsigned char *out /* (m-2)*m */);

/* Which SURVIVING shard is wrong, in a group that also has lost shards?  qfec_locate needs all k + m
 * shards of a group; on a lossy link that is the rare case.  A group with t <= m - 2 marked (lost)
 * shards still holds m - t >= 2 shards more than the k a decode needs, and those can name one
 * corrupted survivor exactly as the m parity rows do for a complete group.  All arithmetic is true
 * GF(2^8) products from the code's parity rows, as in qfec_verify and qfec_locate (no rs.c stale-row
 * quirk).  Per group, with E the marked shards and t = |E|:
 *   K    the k lowest unmarked shard ids: the survivors qfec_repair decodes from
 *   R    the other m - t unmarked ids, the spares; always parity rows (K holds every unmarked data shard)
 *   A_x  for each spare x, the row over K that qfec_repair_rows returns for x under the mask E + R
 *        (m bits set, K unchanged); s_x = shard_x ^ sum_{i in K} A_x[i] x shard_i is its syndrome
 * [A | I] over (K, R) is the parity check of the code punctured at E, an MDS [n - t, k] code of
 * distance m - t + 1.  An error in spare x0 alone gives s_x0 != 0 and every other s_x = 0; an error
 * in the shard at position i of K alone gives s_x = (A_x[i] / A_x0[i]) x s_x0 for the first spare x0
 * and every other x.  A shard is a candidate only if its relation holds in EVERY byte of
 * [0, block_size).  Marked shards are never read and never candidates.  d_culprit[g]:
 *   t > m                        QFEC_LOC_LOST: under-determined
 *   t = m                        QFEC_LOC_UNCHECKED: no spare, nothing can be checked
 *   t < m, all syndromes zero    QFEC_LOC_CLEAN
 *   t < m, one candidate         its shard id 0..k+m-1
 *   t < m, no candidate          QFEC_LOC_MULTI
 *   t < m, several candidates    QFEC_LOC_AMBIGUOUS
 * With ONE spare (t = m - 1) there is no ratio to test: an inconsistent group is then AMBIGUOUS,
 * because every shard of K and the spare itself explain it equally well.  That is the honest answer
 * of a distance-2 code: it detects, it cannot locate.
 * With t = 0 the definitions reduce to qfec_locate's (K is the data, R the parity, A the parity
 * rows), and the verdicts are identical to qfec_locate's.  With m - t >= 3 spares two corrupted
 * survivors are never taken for one; with exactly 2 spares the verdict for two corrupted survivors is
 * undefined (a wrong id is possible), as for m = 2 in qfec_locate.
 * d_marks is in the rs.c layout, as for qfec_repair (non-zero = lost).  d_marks_out (same layout, may
 * be NULL, may be d_marks itself) is written for every group: the input marks as 0 / 1, plus 1 at the
 * culprit when one is located -- ready for qfec_repair, since a culprit exists only when t + 1 <= m - 1.
 * d_counts ([5], may be NULL; accumulated, not reset) gains 1 per located, MULTI, AMBIGUOUS,
 * UNCHECKED and LOST group.  Layouts, pitch and the meaning of [block_size, pitch) are qfec_locate's;
 * nothing in d_data / d_parity is written.  Asynchronous on `stream` once the pattern tables exist
 * (one record per mask with t <= m - 1 and a 2^(k+m)-entry LUT, built by qfec_prepare_locate_erased
 * or on the first call); the per-group working words come from stream-ordered scratch.  Reads the
 * k + m - t unmarked rows of a group.  On complete groups qfec_locate is the faster call (16-B lanes).
 * QFEC_EUNSUP, decided on the host before anything is launched: everything qfec_locate refuses
 * (m < 2; k or m > 32; a zero coefficient in the parity rows); k + m > 24 (the LUT is keyed by the
 * whole mask, as qfec_repair's); a code from explicit rows where some mask with t <= m - 2 has a zero
 * in A, or some mask with t <= m - 1 a singular matrix over K: the punctured code is then not MDS.
 * Codes from qfec_code_new never hit the last case.  Also refused: a shape whose records (one per mask
 * with t <= m - 1) would take more than 256 MiB, which needs m >= 8 at k + m near 24. */
#define QFEC_LOC_UNCHECKED (-4)  /* t = m: no spare row, nothing can be checked */
#define QFEC_LOC_LOST      (-5)  /* t > m: under-determined */
int qfec_locate_erased(qfec_code *code, const unsigned char *d_data, const unsigned char *d_parity,
                       const unsigned char *d_marks      /* rs.c layout, as qfec_repair; non-zero = lost */,
                       long long groups, int block_size, long long pitch,
                       int *d_culprit                    /* [groups] */,
                       unsigned char *d_marks_out        /* rs.c layout, nullable, may equal d_marks */,
                       unsigned int *d_counts            /* [5] located, multi, ambiguous, unchecked, lost; accumulates; nullable */,
                       void *stream);
int qfec_prepare_locate_erased(qfec_code *code);

/* qfec_locate_erased into stream-ordered scratch marks, then qfec_repair with them, in one call: the
 * lost shards and the one corrupted survivor of a group are both rewritten to the original bytes in
 * [0, block_size).  MULTI, AMBIGUOUS and LOST groups are untouched byte for byte (MULTI / AMBIGUOUS:
 * their lost shards are NOT rebuilt, a rebuild would carry the corruption into them; they are reported
 * in d_culprit ([groups], may be NULL) and d_counts ([5], may be NULL)).  UNCHECKED groups, and CLEAN
 * groups that have lost shards, are repaired exactly as qfec_repair would repair them -- for UNCHECKED
 * ones from survivors nothing could check.  *d_failed (may be NULL) is qfec_repair's counter: it gains
 * 1 per LOST group.  QFEC_EUNSUP as for qfec_locate_erased, before anything is launched. */
int qfec_scrub_erased(qfec_code *code, unsigned char *d_data, unsigned char *d_parity,
                      const unsigned char *d_marks, long long groups, int block_size, long long pitch,
                      int *d_culprit /* nullable */, unsigned int *d_counts /* [5], nullable */,
                      unsigned int *d_failed /* qfec_repair's counter, nullable */, void *stream);

/* The host-built constants of qfec_locate_erased for one group (group-order marks[n]): survivors_out
 * (k) = K, spares_out (m - t) = R, rows_out ((m - t) x k) = A, ratios_out (nullable) = A_x[i] / A_x0[i]
 * at [i*(m-t-1) + (x-1)], x = 1..m-t-1, x0 the first spare.  Returns the number of spares m - t, 0 when
 * t = m (only survivors_out is written), -1 when t > m; QFEC_EUNSUP when the matrix over K is singular.
 * Any k + m.  CPU only, like qfec_repair_rows. */
int qfec_locate_erased_plan(const qfec_code *code, const unsigned char *marks_n,
                            int *survivors_out /* k */, int *spares_out /* m - t */,
                            unsigned char *rows_out /* (m-t)*k: A */,
                            unsigned char *ratios_out /* k*(m-t-1): A_x[i]/A_x0[i] at [i*(m-t-1)+(x-1)], nullable */);

/* Device-built check plans: single-shard error location for ANY k + m, beside lost shards or not,
 * asynchronously.  qfec_locate_erased takes K, R, A and the ratios of a group from one host-built record
 * per mask behind a 2^(k+m)-entry LUT (k + m <= 24) and keeps a candidate bit per shard in a 32-bit
 * word (k, m <= 32).  Here the check plan of every group is computed on the device from the group's
 * marks, on the caller's stream: no LUT, no qfec_prepare_*, no read-back, no host synchronisation, no
 * limit on k, m or k + m.
 *   Semantics: exactly qfec_locate_erased's, above -- K, R, A_x, the syndromes as true GF products, a
 *     candidate only if its relation holds in EVERY byte of [0, block_size), and its table of verdicts
 *     (LOST, UNCHECKED, CLEAN, a shard id, MULTI, AMBIGUOUS).  Marked shards are never read, bytes in
 *     [block_size, pitch) never count, d_data / d_parity are never written by the locate.  With two
 *     spares the verdict for two corrupted survivors is undefined, as there.
 *   Codes: that every punctured code is MDS cannot be checked by enumerating masks at these widths, so
 *     the calls accept exactly the codes whose parity rows are, byte for byte, what
 *     qfec_code_new(QFEC_CAUCHY, k, m) or qfec_code_new(QFEC_VANDERMONDE, k, m) produces: those codes,
 *     qfec_code_from_rows with those rows, and fec_new / reed_solomon_new handles that have not been
 *     edited.  They are MDS: every entry of every A is non-zero, the ratios A_x1[i] / A_x0[i] are distinct
 *     over i, a non-zero syndrome byte has at most one explanation when there are two spares or more,
 *     and AMBIGUOUS occurs only with one spare.  Everything else is QFEC_EUNSUP with the cause in
 *     qfec_last_error, m < 2 included (as qfec_locate); judged on the host once per version of the
 *     code, before a device is touched, also with zero groups and null buffers.  Narrow codes are
 *     accepted too; for them qfec_locate / qfec_locate_erased, with their compiled instances, are the
 *     faster calls.
 *   The check plan of a group, qfec_check_stride(code) bytes, public and fixed:
 *       [0]   u16 S (spares: m - t, 0 when t >= m), u16 t (marked shards), u8 status (0 t = m: nothing
 *             to check, 1 work, 2 t > m or a zero pivot, which accepted codes never have), pad to 16 bytes
 *       [16]  32 bytes: the group's marks as one bit per shard id, four little-endian u64 words; set
 *             for every status, so qfec_check_apply never needs the marks buffer
 *       [48]  k survivor ids (K, u8), then m spare ids (u8, the first S valid, ascending), padded to 16
 *       then  m x k bytes, the first S x k valid: A, row x over K in the order listed; padded to 16
 *       then  k x (m - 1) bytes, the first k x (S - 1) valid: A_x[i] / A_x0[i] at [i*(S-1) + (x-1)],
 *             x0 the first spare -- exactly qfec_locate_erased_plan's ratios_out; padded to 16
 *       every unused byte is zero.  With status 0 or 2 only the header and the marks are set.
 *   qfec_check_build writes the check plans of `groups` groups; d_marks is in the rs.c layout (non-zero
 *     = lost) and may be NULL: no shard of any group is marked.  qfec_check_apply runs them on a batch:
 *     d_culprit, d_marks_out (rs.c layout, may be NULL) and d_counts ([5], may be NULL; accumulated) as
 *     in qfec_locate_erased.  It reads only the plan, never the marks, so one plan serves every scrub
 *     pass while the same shards stay lost.  A buffer that qfec_check_build did not write is not a
 *     check plan, and applying it is undefined.
 *   d_check must be 16-byte aligned (the stride is a multiple of 16): plans are written 16 bytes at a
 *     time and read as dwords.  A misaligned d_check is refused with QFEC_EINVAL, like d_plan.
 *   qfec_locate_wide is qfec_check_build into stream-ordered scratch followed by qfec_check_apply, the
 *     batch cut so that one chunk's plans stay under 64 MiB; d_marks may be NULL (complete groups) and
 *     d_marks_out may be d_marks itself.
 *   qfec_scrub_wide is qfec_locate_wide into stream-ordered scratch marks followed by qfec_repair_wide
 *     with them, under qfec_scrub_erased's rules: a located culprit and the lost shards of its group are
 *     rewritten to the original bytes in [0, block_size); the marks of MULTI and AMBIGUOUS groups are
 *     zeroed, so nothing in those groups is rebuilt; LOST groups are untouched and counted into
 *     *d_failed (may be NULL) by the repair; UNCHECKED groups, and CLEAN groups with losses, are
 *     repaired as qfec_repair_wide repairs them.
 *   16-byte lanes when both bases and the pitch allow, else byte by byte; batches beyond the 32-bit
 *     index space of a launch are cut into several launches by the host.  The per-group working words
 *     come from stream-ordered scratch.  A consistent batch costs one read of the k + m - t unmarked
 *     rows of every group, plus the plans.
 *   QFEC_EINVAL, decided on the host before a device is touched, the cause named in qfec_last_error:
 *     a null code, groups < 0, block_size < 1, pitch < block_size, a null required buffer with
 *     groups > 0, a d_check that is not 16-byte aligned.  groups == 0 returns QFEC_OK and launches
 *     nothing. */
long long qfec_check_stride(const qfec_code *code);         /* bytes per group, a multiple of 16 */
int qfec_check_build(qfec_code *code, const unsigned char *d_marks /* rs.c layout, NULL = no shard marked */,
                     long long groups, unsigned char *d_check /* [groups][stride] */, void *stream);
int qfec_check_apply(qfec_code *code, const unsigned char *d_data, const unsigned char *d_parity,
                     const unsigned char *d_check, long long groups, int block_size, long long pitch,
                     int *d_culprit            /* [groups] */,
                     unsigned char *d_marks_out /* rs.c layout, nullable */,
                     unsigned int *d_counts    /* [5] as qfec_locate_erased, nullable */, void *stream);
int qfec_locate_wide(qfec_code *code, const unsigned char *d_data, const unsigned char *d_parity,
                     const unsigned char *d_marks /* nullable: complete groups */, long long groups,
                     int block_size, long long pitch, int *d_culprit /* [groups] */,
                     unsigned char *d_marks_out /* nullable, may equal d_marks */,
                     unsigned int *d_counts /* [5], nullable */, void *stream);
int qfec_scrub_wide(qfec_code *code, unsigned char *d_data, unsigned char *d_parity,
                    const unsigned char *d_marks /* nullable */, long long groups, int block_size,
                    long long pitch, int *d_culprit /* nullable */, unsigned int *d_counts /* [5], nullable */,
                    unsigned int *d_failed /* qfec_repair_wide's counter, nullable */, void *stream);
/* The check plan of one group (group-order marks[n]) in the same layout, stride bytes.  Any k + m.
 * CPU only, like qfec_plan_build_host; QFEC_EINVAL / QFEC_EUNSUP as above. */
int qfec_check_build_host(const qfec_code *code, const unsigned char *marks_n,
                          unsigned char *out_check /* stride bytes */);

/* The check plans on a table of shard addresses: single-shard error location for ANY k + m, beside lost
 * shards or not, on shards scattered in device memory.  qfec_locate_ptrs takes k <= 32, m <= 32 and
 * complete groups; these calls are qfec_check_apply / qfec_locate_wide / qfec_scrub_wide, above, on the
 * table, marks and shards of qfec_reconstruct_ptrs_wide.  A check plan never refers to a layout, so
 * qfec_check_build and qfec_check_build_host serve a table unchanged.
 *   Table, marks, shards: d_shards holds groups * (k + m) device addresses in rs.c order -- every
 *     group's data shards, group-major, then every group's parity shards; d_marks and d_marks_out are
 *     in the rs.c layout, in the table's own order, so d_marks_out can be handed unchanged to
 *     qfec_repair_ptrs_wide.  Every shard is exactly block_size bytes at any alignment (no pitch), and
 *     no byte outside [0, block_size) of any shard is read.  qfec_check_apply_ptrs and
 *     qfec_locate_ptrs_wide write nothing into any shard, so there shards may alias or repeat.
 *   Verdicts, counters, codes: d_culprit, d_marks_out and d_counts ([5], accumulated) are what
 *     qfec_check_apply / qfec_locate_wide / qfec_scrub_wide give for the same rows laid out contiguously;
 *     the accepted codes are theirs (QFEC_EUNSUP for anything else, m < 2 included, judged on the host
 *     before a device is touched, also with zero groups and null buffers; narrow codes are accepted).
 *     d_check follows the same 16-byte rule, and one check plan serves any number of tables while the
 *     same shards stay lost.
 *   Marked shards are never dereferenced by qfec_check_apply_ptrs and qfec_locate_ptrs_wide: the plan
 *     lists the k survivors and the S spares and only those shards are loaded, so the table entries of
 *     marked shards may hold anything; groups whose plan has status 0 or 2 read nothing.  In
 *     qfec_scrub_ptrs_wide the entries of marked shards must be real buffers of block_size bytes, for
 *     the repair writes them; a written shard must not overlap any other shard of the batch
 *     (qfec_repair_ptrs_wide's rule), or the result is undefined.
 *   Alignment is judged per group on the device, from the entries of the group's unmarked shards only:
 *     a group whose unmarked shards all start on a 16-byte boundary runs 16-byte lanes over its whole
 *     columns and its block_size % 16 tail bytes byte by byte; any other group runs byte by byte, much
 *     slower.
 *   qfec_locate_ptrs_wide is qfec_check_build into stream-ordered scratch followed by
 *     qfec_check_apply_ptrs, the batch cut so that one chunk's plans stay under 64 MiB; d_marks may be
 *     NULL (complete groups) and d_marks_out may be d_marks itself.
 *   qfec_scrub_ptrs_wide is that locate into stream-ordered scratch marks followed by
 *     qfec_repair_ptrs_wide with them, under qfec_scrub_wide's rules: a located culprit and the lost shards
 *     of its group are rewritten to the original bytes; MULTI and AMBIGUOUS groups get no marks and are
 *     untouched byte for byte; LOST groups are untouched and counted into *d_failed (may be NULL);
 *     UNCHECKED groups, and CLEAN groups with losses, are repaired as qfec_repair_ptrs_wide repairs them.
 *   QFEC_EINVAL, decided on the host before a device is touched, the cause named in qfec_last_error
 *     after the call's name: a null code, groups < 0, block_size < 1, and with groups > 0 a null
 *     d_shards, a null d_check, for qfec_check_apply_ptrs and qfec_locate_ptrs_wide a null d_culprit; a
 *     d_check that is not 16-byte aligned.  groups == 0 returns QFEC_OK and launches nothing. */
int qfec_check_apply_ptrs(qfec_code *code, unsigned char *const *d_shards, const unsigned char *d_check,
                          long long groups, int block_size, int *d_culprit /* [groups] */,
                          unsigned char *d_marks_out /* rs.c layout, nullable */,
                          unsigned int *d_counts /* [5], nullable */, void *stream);
int qfec_locate_ptrs_wide(qfec_code *code, unsigned char *const *d_shards,
                          const unsigned char *d_marks /* nullable: complete groups */, long long groups,
                          int block_size, int *d_culprit /* [groups] */,
                          unsigned char *d_marks_out /* nullable, may equal d_marks */,
                          unsigned int *d_counts /* [5], nullable */, void *stream);
int qfec_scrub_ptrs_wide(qfec_code *code, unsigned char *const *d_shards,
                         const unsigned char *d_marks /* nullable */, long long groups, int block_size,
                         int *d_culprit /* nullable */, unsigned int *d_counts /* [5], nullable */,
                         unsigned int *d_failed /* qfec_repair_ptrs_wide's counter, nullable */, void *stream);

/* The same three calls where every data shard has its own length: a receiver's ragged packets, located
 * and repaired where they lie, at any k + m, beside lost shards or not.  The check plan never refers to a
 * length, so qfec_check_build and qfec_check_build_host serve these calls unchanged.
 *   Arguments: table, marks, check plan and accepted codes are qfec_locate_ptrs_wide's (any k + m,
 *     QFEC_EUNSUP judged on the host); d_lens (groups * k ints in table order), d_group_len (the parity
 *     length L of each group) and max_len >= 1, which only sizes the launch, are
 *     qfec_plan_apply_ptrs_var's.
 *   Judgement per group, in this order.  The plan's status first: status 2 is QFEC_LOC_LOST and its
 *     lengths are not judged.  For status 0 and 1 alike the lengths come next: L outside [0, max_len],
 *     or an UNMARKED data shard with len_i outside [0, L] (INT_MIN and INT_MAX included), makes the group
 *     invalid.  Marked is the plan's mark bit; the d_lens entry of a marked shard is not looked at.  Of
 *     an invalid group nothing is dereferenced, d_culprit[g] = QFEC_LOC_INVALID, *d_invalid (nullable,
 *     accumulates) gains 1 exactly once, the group counts nowhere in d_counts and d_marks_out carries the
 *     input marks as 0 / 1.  A valid group with status 0 is QFEC_LOC_UNCHECKED; a valid group with
 *     status 1 and L = 0 is QFEC_LOC_CLEAN with nothing dereferenced.
 *   Reads: a surviving data shard is read in [0, len_i) only and counts as zero up to L; an unmarked
 *     parity shard is read in [0, L) only; a marked shard is never dereferenced, nor is an unmarked data
 *     shard with len_i = 0, whose table entry may be anything and takes no part in the alignment
 *     judgement.  qfec_check_apply_ptrs_var and qfec_locate_ptrs_wide_var write nothing into any shard.
 *   Verdict: what qfec_check_apply_ptrs gives with block_size = L on the same rows with every data
 *     survivor zero-padded to L, plus the condition of qfec_locate_ptrs_var: a data shard of K is known
 *     to be zero in [len_i, L), so it stays a candidate only if every syndrome is zero in every byte
 *     position >= len_i.  A group whose only padded-rows explanation is a data shard "wrong" past its own
 *     end is QFEC_LOC_MULTI.  Deviation: with one spare (S = 1) an inconsistent group is
 *     QFEC_LOC_AMBIGUOUS exactly as in the contiguous call; the lengths are NOT used to narrow that
 *     verdict, although a damaged byte past the end of all data shards but one could name that one.
 *   Alignment is judged per group on the device from the entries the call may dereference: the unmarked
 *     data shards of non-zero length, and the unmarked parity shards when L > 0.  An aligned group runs
 *     16-byte lanes over its whole columns and its L % 16 tail bytes byte by byte; any other group runs
 *     byte by byte, much slower.
 *   qfec_locate_ptrs_wide_var is qfec_check_build into stream-ordered scratch followed by
 *     qfec_check_apply_ptrs_var, in qfec_locate_ptrs_wide's chunks; d_marks may be NULL and d_marks_out
 *     may be d_marks itself.  Its marks may be handed to qfec_repair_ptrs_wide_var ONLY where the marked
 *     culprit has room for L bytes, for that call writes [0, L) of every marked shard.
 *   qfec_scrub_ptrs_wide_var has no such condition.  It is that locate into stream-ordered scratch marks
 *     followed by the repair of qfec_repair_ptrs_wide_var: INVALID, MULTI and AMBIGUOUS groups get no
 *     marks and are untouched byte for byte; LOST groups are untouched and counted into *d_failed;
 *     UNCHECKED groups, and CLEAN groups with losses, are repaired as qfec_repair_ptrs_wide_var repairs
 *     them.  Lost shards need room for L bytes and exactly [0, L) of each is written.  A located DATA
 *     culprit i has exactly its bytes [0, len_i) rewritten and no byte at or past len_i is read or
 *     written (the shard is known zero there, and a ragged packet buffer has no room there); a located
 *     parity culprit has [0, L) rewritten.  *d_invalid is the locate's count: once its marks are zeroed
 *     the repair would judge lengths the caller never promised, so the repair's own count is dropped.
 *     With all lengths equal to L the result is byte for byte qfec_scrub_ptrs_wide's.
 *   QFEC_EINVAL, decided on the host before a device is touched, the cause named in qfec_last_error
 *     after the call's name: a null code, groups < 0, max_len < 1, and with groups > 0 a null d_shards,
 *     d_lens or d_group_len, a null d_check, for the two locates a null d_culprit; a d_check that is not
 *     16-byte aligned.  A bad argument wins over groups == 0, which otherwise returns QFEC_OK and
 *     launches nothing. */
int qfec_check_apply_ptrs_var(qfec_code *code, unsigned char *const *d_shards,
                              const int *d_lens /* [groups * k] */, const int *d_group_len /* [groups] */,
                              const unsigned char *d_check, long long groups, int max_len,
                              int *d_culprit /* [groups] */, unsigned char *d_marks_out /* nullable */,
                              unsigned int *d_counts /* [5], nullable */,
                              unsigned int *d_invalid /* nullable, accumulates */, void *stream);
int qfec_locate_ptrs_wide_var(qfec_code *code, unsigned char *const *d_shards, const int *d_lens,
                              const int *d_group_len, const unsigned char *d_marks /* nullable */,
                              long long groups, int max_len, int *d_culprit /* [groups] */,
                              unsigned char *d_marks_out /* nullable, may equal d_marks */,
                              unsigned int *d_counts /* [5], nullable */,
                              unsigned int *d_invalid /* nullable, accumulates */, void *stream);
int qfec_scrub_ptrs_wide_var(qfec_code *code, unsigned char *const *d_shards, const int *d_lens,
                             const int *d_group_len, const unsigned char *d_marks /* nullable */,
                             long long groups, int max_len, int *d_culprit /* nullable */,
                             unsigned int *d_counts /* [5], nullable */,
                             unsigned int *d_failed /* nullable */, unsigned int *d_invalid /* nullable */,
                             void *stream);

/* The qfec_code behind a handle of the per-call ABIs, so a caller holding fec_new() /
 * reed_solomon_new() handles (e.g. network/FecCodec.cpp's codec list) can batch groups
 * through qfec_encode / qfec_reconstruct with the very same matrix. */
struct _reed_solomon;
qfec_code *qfec_fec_code(void *fec_handle);
qfec_code *qfec_rs_code(struct _reed_solomon *rs);
/* The n x k systematic matrix of a fec_new() handle (identity on top). */
int qfec_fec_matrix(void *fec_handle, unsigned char *out_full);

/* ---- FEC datagram batches: the network layer's shard + wire format ----
 * Send, for `groups` full groups of k packets (zfec_pack_input, network/NetFecCodec.cpp:96-172):
 *   shard (g, i)    = [size u16][cksum16(payload) u16 if checksum][payload], zero-filled
 *                     (set_fec_enc_buf, network/FecCodecBuf.cpp:66-103)
 *   check shards    = fec_encode(.., groupMax) (get_fec_encoded_pkt, FecCodecBuf.cpp:137-156)
 *   datagram (g, j) = [0xEC|0xED][sent u32][src u32][n | k<<4 | ik<<8 u16][cksum16 if 0xED][shard]
 *                     (pack_fec_head, FecCodecBuf.cpp:274-328); sent = seq[g][0] + j,
 *                     src = seq[g][1] + min(j, k - 1)
 * Receive reverses it: unpack_fec_head (:334-411; a failed shard checksum drops the
 * datagram), reconstruct of the missing data shards from the first k valid ones, and
 * dec_src_pkt_info (:109-133): status[g*k+i] = payload offset in the shard row (2 or 4),
 * -1 dropped (size >= dec_pkt_size or checksum mismatch), -2 lost (group unrecoverable);
 * psize = the payload size field.
 * Layout: d_shards [G][n][shard_pitch], d_wire [G][n][wire_pitch] (16-B aligned, pitches
 * multiples of 16, wire_pitch >= shard_pitch + 13), d_wire_len [G*n] (0 = not received),
 * d_marks [G*n] rs.c-layout scratch, d_rx_size [G*n] (nullable).  n = k + m <= 15 (the
 * header's 4-bit fields).  d_payload must stay readable 16 bytes past its last byte.
 * Send, what a call leaves behind (qfec_pack_datagrams; qfec_pack_frames follows it):
 *   - a group with any size < 0 or > shard_pitch - head (head = 4 with checksums, 2 without) is
 *     void: all its n d_wire_len entries are -1.  The test is size <= shard_pitch - head, so sizes
 *     up to INT_MAX are void too.  Every row of a void group is either left as the caller had it or
 *     all zero.  The offsets of a void group's rows are still dereferenced on the staged path
 *     (k_build_shards reads up to shard_pitch bytes behind them) and so must be valid.
 *   - bytes [d_wire_len, wire_pitch) of a live row are zero where the fused send stores whole 64-B
 *     lines: a templated (k, m), wire_pitch the 64-B multiple just above hdr + shard_pitch (hdr = 13
 *     with checksums, 11 without) and at least 320 B (checksums) / 256 B (none).  Elsewhere each such
 *     byte is zero or left as the caller had it; nothing else is written there.
 *   - d_shards is scratch: the staged path builds the shards in it, the fused send keeps 16-lane
 *     partial byte sums there (never more than groups * n * shard_pitch bytes), or leaves it alone.
 *   - no input is written. */
int qfec_pack_datagrams(qfec_code *code, const unsigned char *d_payload, const long long *d_offsets,
                        const int *d_sizes, const unsigned int *d_seq, long long groups, int checksum,
                        unsigned char *d_shards, long long shard_pitch, unsigned char *d_wire,
                        long long wire_pitch, int *d_wire_len, void *stream);
int qfec_unpack_datagrams(qfec_code *code, const unsigned char *d_wire, long long wire_pitch,
                          const int *d_wire_len, long long groups, int checksum, int dec_pkt_size,
                          unsigned char *d_shards, long long shard_pitch, unsigned char *d_marks,
                          int *d_rx_size, int *d_status, int *d_psize, void *stream);

/* ---- ProtocolUdp framing of datagram batches ----
 * The byte stage below FEC.  Row r of d_out = Session::PacketOutput + ProtocolUdp::SendPacket
 * (network/SessionDesc.cpp:69-77, network/ProtocolBasic.cpp:111-150) applied to d_in row r:
 *   [mask][c][(cmd & 0x1f) | 0xA0][protocol]([conv u32 LE][hid u32 LE])[d_in[r][0, len)]
 * with bytes 1.. XORed by mask ^ gmask ^ 0x5a, mask = d_mask[r] (the session's _mask++),
 * c = CheckSum(bytes 2..) & 0xff, CheckSum(x) = ~(fold16(byte sum)) (ProtocolBasic.cpp:56-87).
 * The 8-byte Session prefix is present iff d_conv_hid ([rows][2] conv, hid) is non-NULL.
 * d_out_len[r] = framed length, or -1 when it does not fit out_pitch.  Bytes of a row past its
 * frame, up to out_pitch, are zero, and a row with d_out_len -1 is all zero (every path).
 * qfec_unframe_udp reverses it (ProtocolUdp::RecvPacket, ProtocolBasic.cpp:152-210):
 * d_status[r] = 0 ok, 1 short, 2 bad checksum, 3 bad cmd, 4 too long; d_out row = the data,
 * d_out_len = len - 4 (- 8 with session = 1); d_info [rows][4] = xor mask, c, cmd & 0x1f,
 * protocol (nullable); d_conv_hid receives the Session prefix when session = 1 (nullable; its
 * entries are meaningful only for rows whose d_status is 0).
 * Pitches multiples of 16, rows 16-B aligned. */
int qfec_frame_udp(const unsigned char *d_in, long long in_pitch, const int *d_len, long long rows,
                   const unsigned char *d_mask, const unsigned int *d_conv_hid, int gmask, int cmd, int protocol,
                   unsigned char *d_out, long long out_pitch, int *d_out_len, void *stream);
int qfec_unframe_udp(const unsigned char *d_in, long long in_pitch, const int *d_len, long long rows, int gmask,
                     int session, unsigned char *d_out, long long out_pitch, int *d_out_len, int *d_status,
                     unsigned char *d_info, unsigned int *d_conv_hid, void *stream);

/* ---- FEC datagrams straight to / from ProtocolUdp frames (SURVEY 8(f) ranks 2-4 fused) ----
 * qfec_pack_frames = qfec_pack_datagrams followed by qfec_frame_udp on every datagram, with
 * cmd / protocol as Session::TransmissionOutput sets them for FEC data (QUICKNET_CMD_DATA,
 * QUICKNET_PROTOCOL_FEC, network/SessionDesc.cpp:513-519): frame row (g, j) of d_frames =
 * [mask][c][(cmd & 0x1f) | 0xA0][protocol]([conv][hid])[datagram (g, j)], bytes 1.. XORed with
 * d_mask[g*n+j] ^ gmask ^ 0x5a; d_frame_len[g*n+j] = framed length (-1 for a void group).
 * The Session prefix is present iff d_conv_hid ([G*n][2]) is non-NULL.  Bytes of a row past its
 * frame, up to frame_pitch, are zero (every path); every row of a void group is left as the caller
 * had it (one pass) or all zero (two calls).  d_mask may have any alignment (the one pass reads it
 * in dwords counted from d_mask: up to 3 bytes past the G*n masks are read, and ignored).
 * One pass (no datagram buffer in HBM) with checksums on, a templated (k, m) and frame_pitch equal to
 * the 64-B multiple above prefix + 13 + shard_pitch, where that is 576 (512-B payloads: two groups
 * per wave), 1088 (1 KiB payloads), 1152..1600 (8-B lanes, three passes: 1400-B payloads) or
 * 1664..2112 (16-B lanes, two passes); other cases run the two calls over stream-ordered scratch.
 * d_shards is scratch as in qfec_pack_datagrams; sizes, void groups and their offsets as there.
 * qfec_unpack_frames = qfec_unframe_udp (ProtocolUdp::RecvPacket, ProtocolBasic.cpp:155-199) of
 * every row, rows RecvPacket rejects counting as not received, then qfec_unpack_datagrams over
 * the datagrams inside: the same d_marks / d_rx_size / d_status / d_psize / d_shards as that
 * call.  d_frame_status [G*n] (nullable) = RecvPacket's verdict per row (0 ok, 1 short,
 * 2 checksum, 3 cmd, 4 too long, as qfec_unframe_udp; a row with both a bad checksum and a bad
 * cmd is 2, RecvPacket's order); d_conv_hid receives the Session prefix when session = 1
 * (nullable): its entries are meaningful only for rows whose d_frame_status is 0, the others are
 * unspecified.  One pass for the templated (k, m). */
int qfec_pack_frames(qfec_code *code, const unsigned char *d_payload, const long long *d_offsets,
                     const int *d_sizes, const unsigned int *d_seq, long long groups, int checksum,
                     unsigned char *d_shards, long long shard_pitch, const unsigned char *d_mask,
                     const unsigned int *d_conv_hid, int gmask, int cmd, int protocol, unsigned char *d_frames,
                     long long frame_pitch, int *d_frame_len, void *stream);
int qfec_unpack_frames(qfec_code *code, const unsigned char *d_frames, long long frame_pitch,
                       const int *d_frame_len, long long groups, int gmask, int session, int checksum,
                       int dec_pkt_size, unsigned char *d_shards, long long shard_pitch, unsigned char *d_marks,
                       int *d_rx_size, int *d_status, int *d_psize, int *d_frame_status,
                       unsigned int *d_conv_hid, void *stream);

/* Gather scattered rows (e.g. datagrams where a receive ring put them) into the pitched batch the
 * calls above take: row r of d_out = the d_len[r] bytes at d_base + d_off[r], zero-padded to
 * out_pitch, d_out_len[r] = d_len[r]; rows with d_len <= 0 get 0 and are not written, rows that
 * do not fit get -1.  wrap_n > 0: the rows are bare shards (row r = shard ik = r % wrap_n of a
 * group) and each gets the 11-byte header a 0xEC datagram of it carries ([0xEC][sent 0][src 0]
 * [wrap_n | wrap_k << 4 | ik << 8]), so qfec_unpack_datagrams decodes groups of chosen shards
 * (fec_decode_pkts, network/FecCodecBuf.cpp:181-232).  Sources stay readable 16 bytes past
 * their last byte. */
int qfec_gather_rows(const unsigned char *d_base, const unsigned long long *d_off, const int *d_len, long long rows,
                     int wrap_n, int wrap_k, unsigned char *d_out, long long out_pitch, int *d_out_len, void *stream);

/* Fill nbytes of device memory with the synthetic stream of quicknet_amd/synth.py. */
int qfec_synth_fill(unsigned char *d_ptr, long long nbytes, unsigned long long seed, void *stream);

/* module/rs.h on host shard pointers (reed_solomon_encode / reed_solomon_reconstruct with every shard
 * in host memory) pipelines its chunks over two slots on the calling thread's current device.
 * qfec_rs_host_devices spreads them over two slots per entry of `devices` instead -- each GPU has
 * its own PCIe link, and a device may be listed more than once (more chunks in flight on it); n = 0
 * goes back to the current device.  Outputs are identical either way.  Not to be called while a
 * module/rs.h call is running on another thread (it waits for it).  qfec_rs_host_devices_get
 * copies up to `cap` entries of the list and returns its length (0: the current device). */
int qfec_rs_host_devices(const int *devices, int n);
int qfec_rs_host_devices_get(int *devices, int cap);

/* Calibration probe, NOT a codec: streams the encode's traffic (k rows in, m rows out,
 * XOR only).  Its time is the memory-side ceiling the GF kernels are compared with. */
int qfec_probe_stream(const unsigned char *d_data, unsigned char *d_parity, long long groups, int k, int m,
                      int block_size, long long pitch, void *stream);

/* Calibration probe, NOT a codec: the reconstruct's memory skeleton for RS(10,3) and RS(16,4) --
 * the same mapping, marks reads, survivor rows and erased-row writes as the auto reconstruct body,
 * XOR in place of the decode (the erased rows receive garbage; no other byte is written).
 * lds_cap: LDS bytes per block (0 none), a residency cap.  QFEC_EUNSUP for other shapes. */
int qfec_probe_reconstruct(unsigned char *d_data, const unsigned char *d_parity, const unsigned char *d_marks,
                           long long groups, int k, int m, int block_size, long long pitch, int lds_cap,
                           void *stream);

/* Knobs.  Integration settings: host chunking, host copy threads, zero copy, the per-call
 * server's footprint.  Plus one A/B switch per kernel family (tools/ab.py, tools/wire_ab.py)
 * and one test hook.  Defaults are the measured best; outputs are identical either way.
 *   "host_zero_copy"   1 pinned host batches worked on in place | 0 staged copies (module/rs.h on host
 *                      pointers: the reconstruct only; its encode always stages through the device,
 *                      measured faster for a freshly gathered slot)
 *   "host_lanes"       4 (default) | 2 .. 8: module/rs.h on host pointers, chunk slots in flight on the
 *                      current device; qfec_rs_host_devices spreads them over listed devices instead
 *   "host_nt"          2 (default) | 1 | 0: module/rs.h on host pointers, streaming (non-temporal) stores
 *                      when gathering caller rows into a slot: 2 for rows that start where the previous
 *                      row ended, 1 for every row, 0 never
 *   "host_chunk"       groups per staged host chunk (0: by bytes: ~32 MiB for qfec_*_host, ~16 MiB of
 *                      caller shards for module/rs.h on host pointers)
 *   "host_threads"     host threads that gather / scatter module/rs.h host shard pointers (0: the
 *                      CPUs this process may use -- affinity and cgroup quota -- at most 32)
 *   "rs_dev_ptrs"      0 (default) | 1: module/rs.h on shard arrays that are all device memory but not
 *                      back to back: 1 sends the pointer array to the device (one copy per chunk) and
 *                      runs the qfec_*_ptrs kernels on the caller's rows in place; 0 stages every row
 *                      through one copy in and one copy out.  Results and return codes are the same.
 *                      Host or mixed arrays, contiguous arrays and k + m > 24 (reconstruct) are not
 *                      affected
 *   "rs_dev_ptrs_wide" 0 (default) | 1: with rs_dev_ptrs = 1, reed_solomon_reconstruct on such arrays with
 *                      k + m > 24 builds RECONSTRUCT plans on the device and applies them on the caller's
 *                      rows in place (qfec_reconstruct_ptrs_wide's kernels); 0 keeps the staged copies and
 *                      host inversions.  Results and return codes are the same.  An edited handle,
 *                      host or mixed arrays, k + m <= 24 and rs_dev_ptrs = 0 are not affected
 *   "percall_resident" 1 fec_encode / fec_decode of packets up to 4 KiB with k <= 16 and k * e <= 64
 *                      go to a resident one-block server that polls a request word in device memory
 *                      and exits by itself after percall_idle_us without a request | 0 one launch per
 *                      call (setting 0 stops the servers)
 *   "percall_idle_us"  how long the resident server's block stays on the device after its last
 *                      request, 0 .. 1 000 000 us (default 1 000); 0 = it exits right after each
 *                      call (every call then pays a launch).  A hipDeviceSynchronize issued while it
 *                      is resident waits for it: at most this long after the last call.
 *   "percall_timeout_us" how long a call spins for the server before it stops the block and waits
 *                      for it (the block serves the pending request first), or, if the request was
 *                      never taken, runs it through one launch (default 2 000 000)
 *   "percall_stop_us"  how long that wait for the stopped block may last (default 2 000 000).  A
 *                      block still not done then (every CU held by other persistent kernels) is
 *                      abandoned: the call fails -- fec_encode prints to stderr and leaves dst as it
 *                      was, fec_decode returns 1 (module/fec.c's own failure shapes, fec.c:730-732,
 *                      833-836) -- and the device takes the one-launch path until percall_resident
 *                      is set to 1 again (the abandoned block's buffers stay allocated)
 *   "percall_fast"     1 per-packet calls on host packets through the server / one launch on mapped
 *                      pinned staging | 0 the staged DMA path (the one device-pointer packets take)
 *   "encode_lds"       -1 auto | 0 none | N: bytes of LDS each encode block allocates (and does not
 *                      use), of the CU's 160 KiB: a cap on the encode's resident waves per CU.  Auto
 *                      caps device-resident launches of >= 8 192 256-thread blocks at 16 waves per CU,
 *                      24 for the two-half inputs on rows <= 1 KiB, and runs 6 <= k <= 10 with m <= 3
 *                      (all rows in registers, rows >= 1 KiB with 128-B-aligned pitch, strides and
 *                      bases, >= 2^21 lanes) as one-wave blocks held
 *                      at 10 per CU (fewer concurrent row streams move more bytes per second through
 *                      HBM); k <= 2
 *                      and encodes of host memory are never capped.  The XOR probe follows the same
 *                      rule for its k (on one-wave blocks at 6 per CU, where its stream runs best)
 *   "encode_block"     -1 auto (64 where the rule above says so, else 256) | 64 | 256: threads per
 *                      encode block
 * A/B, one per kernel family:
 *   "encode_impl"      -1 auto (2 for k >= 16, else 0) | 0 all rows | 2 all rows, the inputs loaded in
 *                      two halves (fewer registers, more waves per SIMD)
 *   "recon_impl"       -1 auto | exact-e rows on 2 16-B lanes | 3 8-B lanes | 4 12-B lanes | 8 = 3 with
 *                      one group per block (auto picks it for 3 where a group is <= 4 waves)
 *   "wire_fused"       1 fused datagram send where a (k, m) instance exists | 0 staged build -> encode -> emit
 *   "wire_rx"          1 fused datagram receive (k_rx, one wave per group), lanes and LDS staging by
 *                      pitch | 2 / 3 16-B lanes with / without the K rows staged in LDS | 4 / 5 8-B
 *                      lanes likewise | 0 staged parse -> reconstruct -> check (3 launches)
 *   "percall_group"    1 fec_encode of a parity index computes the group's n - k rows in one request
 *                      and serves the group's other indices from a per-handle copy while src[], sz and
 *                      every input byte are unchanged | 0 one request per index
 * Test hook:
 *   "percall_fault"    1 requests are never handed to a server, so every call takes the timeout
 *                      branch | 2 the same, and the stopped server counts as not done within
 *                      percall_stop_us (the abandon branch) */
int qfec_tune(const char *key, int value);
/* The current value of a knob of qfec_tune (*value); QFEC_EINVAL for an unknown key. */
int qfec_tune_get(const char *key, int *value);

/* The resident per-call server of the current device (qfec_tune "percall_resident"): out[0] calls
 * it served, out[1] launches, out[2] relaunches because it had exited (idle) just before a request
 * arrived, out[3] 1 while its block may still be running (it exits 1 ms after the last request),
 * out[4] 1 set up | -1 unavailable on this device (device memory not CPU-mapped) | 0 not yet used.
 * Returns QFEC_OK, or an error without a device. */
int qfec_percall_stats(unsigned long long out[5]);
/* The same counters and more, as many as `n` asks for (returns how many were written, or an error):
 * [0..4] as qfec_percall_stats, [5] requests the server did not serve within percall_timeout_us
 * (each then waited for the stopped server, or ran through one launch), [6] / [7] fec_encode calls
 * served from / computing the group cache (all handles), [8] the current percall_idle_us, [9] servers
 * abandoned after percall_stop_us (qfec_percall_stats out[4] is then -2). */
int qfec_percall_counters(unsigned long long *out, int n);

int qfec_set_kernel_variant(int variant);
int qfec_get_kernel_variant(void);
int qfec_device_count(void);
const char *qfec_strerror(int err);
const char *qfec_last_error(void);
const char *qfec_version(void);

#ifdef __cplusplus
}
#endif

#endif /* QFEC_H */
