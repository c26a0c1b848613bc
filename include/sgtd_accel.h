/*
 * sgtd_accel.h — C ABI of the MI355X (gfx950) triangle-descriptor build +
 * geometric-hash match engine.  This is the drop-in boundary for the hot path
 * of Hfx-J/SGTD: the bodies of
 *
 *   STDescManager::BuildSingleScanSTD   src/sgtd/src/STDesc.cpp:174-315
 *   STDescManager::AddSTDescs           src/sgtd/src/STDesc.cpp:149-172
 *   STDescManager::candidate_selector   src/sgtd/src/STDesc.cpp:318-460
 *
 * (class declared at src/sgtd/include/desc/STDesc.h:342-440) forward to these
 * entry points; the reference has no FFI layer of its own, the C++ class *is*
 * the operator API.  INTEGRATION.md shows the adapter.
 *
 * Conventions: every function returns 0 (SGTD_OK) or a negative sgtd_status;
 * nothing throws across the ABI; all output buffers are caller allocated and
 * sized by the documented bounds; a handle is not thread safe (neither is the
 * reference's manager).  All HIP work of a handle is issued on one stream
 * (sgtd_set_stream).  There is NO CPU fallback: without a usable gfx950 device
 * sgtd_create fails with SGTD_ERR_NO_DEVICE.
 */
#ifndef SGTD_ACCEL_H
#define SGTD_ACCEL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum sgtd_status {
  SGTD_OK = 0,
  SGTD_ERR_INVALID = -1,      /* bad argument / config                         */
  SGTD_ERR_NO_DEVICE = -2,    /* no HIP device / wrong architecture            */
  SGTD_ERR_HIP = -3,          /* a HIP runtime call failed (see sgtd_last_error)*/
  SGTD_ERR_CAPACITY = -4,     /* caller buffer too small                       */
  SGTD_ERR_FRAME_LIMIT = -5,  /* frame id >= max_frame_n (MAX_FRAME_N, STDesc.h:33:
                                 the reference indexes a fixed array there)   */
  SGTD_ERR_UNSUPPORTED = -6,  /* configuration outside the kernels' envelope   */
  SGTD_ERR_STATE = -7,        /* call order (e.g. results before a query)      */
  SGTD_ERR_IO = -8            /* a graph file could not be opened or parsed    */
} sgtd_status;

/* ConfigSetting fields the path reads (STDesc.h:38-72); defaults in
 * sgtd_default_config() are the shipped YAML (config/SG_localization.yaml:74-89) */
typedef struct sgtd_config {
  int32_t descriptor_near_num;   /* K, STDesc.cpp:179; 3 <= K <= 16            */
  int32_t candidate_num;         /* STDesc.cpp:423; <= 64                      */
  int32_t max_frame_n;           /* MAX_FRAME_N, STDesc.h:33 (runtime here)    */
  int32_t device_id;             /* HIP device ordinal                         */
  double descriptor_min_len;     /* STDesc.cpp:181                             */
  double descriptor_max_len;     /* STDesc.cpp:180; *1000 must be < 2^21       */
  double std_side_resolution;    /* STDesc.cpp:178                             */
  double rough_dis_threshold;    /* STDesc.cpp:357                             */
  uint32_t first_frame_id;       /* initial current_frame_id_ (STDesc.h:363 is 0);
                                    a table shard of a multi-GPU map starts at
                                    the first frame it owns                    */
  uint32_t reserved;
} sgtd_config;

/* One descriptor = one STDesc (STDesc.h:75-97) without the unused covariance
 * matrices, as a structure of caller-allocated arrays.  NULL members are
 * skipped on output and read as zero on input (side, label, frame are
 * mandatory on input). */
typedef struct sgtd_desc_soa {
  double *side;      /* [n*3] side_length_ (scaled, ascending)                */
  double *angle;     /* [n*3] angle_                                          */
  double *center;    /* [n*3] center_                                         */
  float *vertex;     /* [n*9] vertex_A_,B_,C_ xyz (exact: they are f32 casts) */
  int32_t *label;    /* [n*3] (int)vertex_attached_                           */
  uint32_t *frame;   /* [n]   frame_id_                                       */
  int32_t *node_id;  /* [n*3] node_id = {i, m, n}                             */
} sgtd_desc_soa;

typedef struct sgtd_stats {
  int64_t n_entries;       /* E: descriptors in the table                      */
  int64_t n_buckets;       /* U: distinct (cell,label code) keys               */
  int64_t n_frames;        /* AddSTDescs calls so far                          */
  int64_t last_queries;    /* query frames in the last batch                   */
  int64_t last_D;          /* query descriptors in the last batch              */
  int64_t last_P;          /* table entries visited (STDesc.cpp:372 iterations)*/
  int64_t last_M;          /* rough matches (STDesc.cpp:378)                   */
  int64_t last_cand_pairs; /* pairs in all candidate match lists               */
  int64_t hbm_bytes_table; /* bytes of the hot (probed) table array (16 B/entry) */
  /* per-kernel device time of the last batch, ms (only when timing is enabled
   * with sgtd_set_timing; measured with hipEvents on the handle's stream)     */
  float ms_build, ms_sort, ms_probe, ms_votes, ms_topk, ms_count, ms_scan, ms_write, ms_total;
  int32_t overflowed;      /* last batch outgrew a work buffer and was re-run  */
  int32_t select_form;     /* how the last batch's match records were turned into votes and lists
                              (STDesc.cpp:404-453): 0 = one wave per 128-descriptor block (votes, topk,
                              block_count / _scan / _write), 1 = the lists by one workgroup per query
                              (pairs_query_kernel), 2 = votes + top-k by one workgroup per query as
                              well (votes_topk_kernel)                                        */
  int64_t last_P_swept;    /* table entries the sweep really loaded: last_P minus the
                              sub-cells of the visited buckets that no match can lie in */
  double bucket_len_sq_over_E; /* sum over buckets of len^2 / E: the bucket length a table entry
                              sees on average (sizes the first batch's work buffers)        */
  int64_t tail_entries;    /* entries in the tail segment (appended after the last full build
                              of the probe layout; 0 = one segment)                         */
  float ms_finalize;       /* wall time of the last probe-layout build: proportional to the
                              appended entries while they fit the tail segment              */
  float reserved2;
  /* since the handle was created (what a caller sees over a stream of DIFFERENT batches): */
  int64_t batches_total;     /* launches of a query batch's pipeline, counted on the device (re-runs included) —
                                the count includes batches that were enqueued and overwritten by the next one
                                without a sgtd_sync / sgtd_result_* call in between                   */
  int64_t overflow_launches_total; /* ... of them, launches that raised a work-buffer flag (their results are
                                incomplete until sgtd_sync has re-run them): a caller that enqueues batch after
                                batch without synchronising checks that this did not move            */
  int64_t reruns_total;      /* launches of a whole batch beyond the first (a work buffer
                                overflowed: match records, pass pool, GroupRows, undecided queue) */
  int64_t rewrites_total;    /* re-runs of the list pass alone (candidate-pair buffer too small) */
  int64_t list_moves_total;  /* match lists that outgrew the room they were given and moved to a
                                fresh slab during the sweep (probe_kernels.hip.h make_room)      */
  int64_t last_list_moves;   /* ... of the last batch                                         */
  int64_t device_allocs_total; /* hipMalloc calls of the handle's work and table buffers so far (a buffer that grows is
                                freed and allocated again, which synchronises the device: a timed region should see none) */
  /* the last sgtd_consistent_loops call: device time of the pair pass and of the greedy passes, ms (only when timing is
   * enabled, as the ms_ fields above), and the greedy rounds it took (a clique shortcut counts as one) */
  float ms_consistency_pairs, ms_consistency_greedy;
  int32_t consistency_rounds;
  int32_t order_giveups_total; /* since the handle was created: batches whose ordering gave up a bounded wait between
                                workgroups (a scheduling surprise) and were run again by sgtd_sync with the launch train;
                                each also counts in overflow_launches_total and reruns_total. 0 in normal use       */
} sgtd_stats;

/* descriptors per tile of the batch ordering's sort passes and of its group index (the tests place their edges there) */
void sgtd_order_tiles(int *sort_tile, int *group_tile);

typedef struct sgtd_engine *sgtd_handle;

void sgtd_default_config(sgtd_config *cfg);
int sgtd_create(const sgtd_config *cfg, sgtd_handle *out);
/* One handle over several GPUs of this process: map frames are dealt to the
 * devices in blocks of 64 consecutive frames, round robin; every device holds a complete table
 * for its frames; a query batch is swept on all devices concurrently and the per-device
 * top-candidate_num tables are merged on the host with the reference's rule (votes descending,
 * ties -> lowest frame id, STDesc.cpp:423-433) — the single-table result.  Match lists, entries
 * and sgtd_verify stay with the owning device and are fetched from it; db_entry ids of such a
 * handle are opaque (owner in the upper bits) and valid for sgtd_fetch_entries only.
 * Host pointers only (device_ptrs must be 0); sgtd_add takes descriptors stamped with the
 * current frame id (what sgtd_build stamps).  Not available on it: sgtd_set_stream,
 * sgtd_export_*_dev, sgtd_result_rough, sgtd_table_dump, sgtd_save_table / sgtd_load_table
 * (SGTD_ERR_UNSUPPORTED).  n_dev == 1 gives an ordinary handle on device_ids[0];
 * cfg->device_id is ignored, cfg->first_frame_id must be a multiple of 64 * n_dev. */
int sgtd_create_multi(const sgtd_config *cfg, const int *device_ids, int n_dev, sgtd_handle *out);
/* devices behind the handle (1 for an ordinary handle) and the per-device engine k (borrowed;
 * e.g. for per-device sgtd_get_stats) */
int sgtd_device_count(sgtd_handle h);
sgtd_handle sgtd_device_handle(sgtd_handle h, int k);
int sgtd_destroy(sgtd_handle h);
const char *sgtd_strerror(int status);
/* text of the last HIP failure on this handle ("" if none) */
const char *sgtd_last_error(sgtd_handle h);

/* all work of the handle goes to this hipStream_t (NULL = the null stream) */
int sgtd_set_stream(sgtd_handle h, void *hip_stream);
/* enable per-kernel hipEvent timing (costs a few microseconds per launch) */
int sgtd_set_timing(sgtd_handle h, int enabled);

/* ---- key helpers: the pure functions the kernels derive their keys with (the same inline
 * code, instantiated on the host; no device needed) — pinned by the CPU tests against the
 * reference's own Combinatorial_Binary_Encoding (STDesc.cpp:3-16), STDesc_LOC equality
 * (STDesc.h:229-236: x, y, z, a only) and VOXEL_LOC equality (STDesc.h:133-135).
 * sgtd_table_key: cell coordinates below 65 536 and a 12-bit code; sgtd_dedup_key: millimetre
 * coordinates below 2^21 (the envelope check_cfg enforces).  Inside those envelopes two keys
 * are equal words exactly when the reference's operator== holds. */
uint32_t sgtd_label_code(int a, int b, int c);
uint64_t sgtd_table_key(uint32_t code, uint32_t x, uint32_t y, uint32_t z);
uint64_t sgtd_dedup_key(uint64_t mx, uint64_t my, uint64_t mz);

/* STDescManager::current_frame_id_ (STDesc.h:350) */
int sgtd_current_frame_id(sgtd_handle h, uint32_t *out);

/* ---- BuildSingleScanSTD (STDesc.cpp:174-315) --------------------------- */
/* One frame: keypoints xyz[n*3] f32 + label[n] (the pcl::PointXYZL fields,
 * utility.hpp:646-659), host memory.  Descriptors are stamped with the
 * current frame id.  out arrays must hold sgtd_max_descs(h, n) descriptors.
 * A frame with n < K yields 0 descriptors (the reference reads past its k-NN
 * result there).  A frame too large for the build kernel's LDS (3638 keypoints
 * at K = 10) is SGTD_ERR_UNSUPPORTED, more than 65535 SGTD_ERR_INVALID.
 * Outside the contract: labels >= 2^31 (the reference's (int) of the label as a
 * double is undefined; labels up to 2^31 - 1 are the reference's), and, with
 * descriptor_min_len = 0, coordinates so far apart that the f32 squared distance
 * of the k-NN search overflows. */
int64_t sgtd_max_descs(sgtd_handle h, int n_keypoints);
int sgtd_build(sgtd_handle h, const float *xyz, const uint32_t *label, int n,
               sgtd_desc_soa *out, int64_t capacity, int64_t *n_out);

/* ---- AddSTDescs (STDesc.cpp:149-172) ------------------------------------ */
/* Appends n host descriptors as one frame: current_frame_id_ is incremented
 * first, entries keep the frame id stored in d->frame. */
int sgtd_add(sgtd_handle h, const sgtd_desc_soa *d, int64_t n);

/* Map construction, the caller's loop semantic_graph_localization.cpp:419-458
 * for n_frames frames at once, entirely on the device: frame k (keypoints
 * kp_off[k]..kp_off[k+1]) is built with frame id current_frame_id_ and added,
 * then current_frame_id_++ .  xyz/label are host pointers unless
 * device_ptrs != 0; kp_off is always a host array of n_frames+1 offsets. */
int sgtd_add_frames(sgtd_handle h, const float *xyz, const uint32_t *label,
                    const int64_t *kp_off, int n_frames, int device_ptrs);

/* Sorts the appended entries into the probe layout (by key, sub-cells inside a bucket, bucket
 * directory + key hash).  Idempotent; called implicitly by the first query after an add.
 * Appending to a finalized table (AddSTDescs only ever appends, STDesc.cpp:149-172) sorts only
 * the appended entries, into a tail segment that every query sweeps after the main one; the
 * tail is merged into the main segment when it outgrows an eighth of it (sgtd_stats.tail_entries,
 * .ms_finalize). */
int sgtd_finalize(sgtd_handle h);

/* Takes sessions out of a built table (the reference only appends, STDesc.cpp:149-172).  Every entry whose frame id is
 * in frame_ids[0..n) is removed; duplicates and ids without entries are ignored.  Afterwards the handle answers every
 * query and inspection call as a handle would to which those frames were never added: the surviving entries keep
 * their insertion order and their insertion indices are renumbered densely (db_entry, sgtd_fetch_entries,
 * sgtd_table_dump, sgtd_save_table); frame_lo / frame_hi and the entry and bucket counts of sgtd_stats describe the
 * survivors, and n_frames loses one for every removed frame that had entries.  current_frame_id_ does not change and
 * removed ids are not reused; a table left empty behaves as a fresh handle's.  The pending batch is dropped and the
 * table version changes: views (sgtd_attach_table) return SGTD_ERR_STATE until attached again.  The next finalize
 * builds one segment over the whole table.  A call that removes nothing changes nothing.  *n_removed (may be NULL):
 * the number of entries removed.  h == NULL, n < 0 or frame_ids == NULL with n > 0: SGTD_ERR_INVALID; a view:
 * SGTD_ERR_STATE.  A multi-device handle forwards each id to the shard that owns it; group entry ids keep their form.
 * Device memory: 36 B per surviving entry beyond the table, for the duration of the call. */
int sgtd_remove_frames(sgtd_handle h, const uint32_t *frame_ids, int64_t n, int64_t *n_removed);

/* Restrict later queries to a set of frames.  Row r holds ceil(n_frames / 64) words; bit (f - frame_lo)
 * (word (f - frame_lo) >> 6, bit (f - frame_lo) & 63) set means frame f is allowed.  Frames outside
 * [frame_lo, frame_lo + n_frames) are never allowed.  n_rows == 1: one row for every query of a batch;
 * n_rows > 1: row q for query q.  rows == NULL with n_rows == 0 clears the filter. */
/* The rows are copied at the call and hold for every later sgtd_query_frames, sgtd_query_descs and sgtd_search_frame
 * until replaced or cleared (a batch keeps the rows it was enqueued with, re-runs included).  Each query is answered as
 * by a handle that holds only its allowed frames (same ids, order and current_frame_id_): candidates, votes (0 for
 * frames not allowed), match lists, per-query match count M, verification, SearchLoop's choice, the rough list.  Only
 * the visit counters (P, n_visit) still count the whole map.  Frame ids are global: sgtd_add*, sgtd_remove_frames and
 * sgtd_load_table leave the filter alone, and frames added later are outside it unless the range covers them.  A view
 * (sgtd_attach_table) has a filter of its own; a multi-device handle slices the rows into each shard's frames.  A
 * query call whose batch size differs from n_rows > 1 (sgtd_query_descs and sgtd_search_frame are batches of one):
 * SGTD_ERR_INVALID; sgtd_loop_frames with a filter set: SGTD_ERR_STATE.  h == NULL, n_rows < 0, rows == NULL with
 * n_rows > 0 or n_frames == 0 with n_rows > 0: SGTD_ERR_INVALID, before the device is touched. */
int sgtd_set_frame_filter(sgtd_handle h, uint32_t frame_lo, uint32_t n_frames, const uint64_t *rows, int n_rows);

/* Poses of map frames, keyed by global frame id: row-major 3x4 [R | t], the 12 floats of a graph file's "poses"
 * (sgtd_graphs_view hands them out in this form).  Later calls overwrite.  pose12 == NULL with n > 0 forgets the
 * poses of those ids; frame_ids == NULL with n == 0 forgets all.  Ids may name frames not (yet) added. */
/* The poses are copied at the call and are settings of the handle, like a frame filter: sgtd_add*, sgtd_remove_frames
 * and sgtd_load_table leave them alone, the table file does not hold them, and a view (sgtd_attach_table) has poses of
 * its own.  A multi-device handle hands each pose to the shard that owns its frame.  h == NULL, n < 0 or
 * frame_ids == NULL with n > 0: SGTD_ERR_INVALID; an id >= max_frame_n: SGTD_ERR_FRAME_LIMIT (nothing is stored). */
int sgtd_set_frame_poses(sgtd_handle h, const uint32_t *frame_ids, const float *pose12, int64_t n);

/* Restrict later queries to the map frames within radius[r] of center[r]: dims 2 tests (x, y) = (t[0], t[1]),
 * dims 3 tests (x, y, z).  n_rows == 1: one prior for every query of a batch; n_rows > 1: row q for query q.
 * center == NULL with n_rows == 0 clears the prior. */
/* center[r * dims + i], radius[r].  Frame f is allowed by row r iff it has a pose (sgtd_set_frame_poses), the tested
 * coordinates of its translation t are finite, and d2 <= rr, where dx = (double)t[0] - cx (dy, dz alike),
 * d2 = (dx*dx + dy*dy) + dz*dz (dims 2: no dz term) and rr = radius * radius, all in f64 without contraction.  (This is
 * evaluate.frames_near's rule for dims 2, which writes radius ** 2.)  A NaN or infinite translation is never allowed,
 * whatever the radius; radius +inf allows every frame with a pose.  The rows are built on the device, once per prior,
 * poses, filter and table span, and work as sgtd_set_frame_filter's rows do: each query is answered as under a filter
 * of the same rows, in everything that call lists.  A prior and a frame filter may be set together: a frame is then
 * allowed only if both allow it, and setting or clearing one leaves the other alone.  The prior is a setting of the
 * handle as the filter is (a batch keeps the prior it was enqueued with, re-runs included; a view has its own; a
 * multi-device handle gives it to every shard).  A query call whose batch size differs from n_rows > 1: SGTD_ERR_INVALID;
 * sgtd_loop_frames with a prior set: SGTD_ERR_STATE.  h == NULL, n_rows < 0, and with n_rows > 0: center or radius
 * NULL, dims not 2 or 3, a non-finite center coordinate, a NaN or negative radius (+inf is allowed): SGTD_ERR_INVALID,
 * before the device is touched. */
int sgtd_set_position_prior(sgtd_handle h, const double *center, const double *radius, int n_rows, int dims);

/* Two (or more) batches in flight over ONE map: `view` — a handle of the same configuration on the same device,
 * without a table of its own — borrows the finalized table of `owner` (cold entries, probe layout, entry ids) and keeps
 * its own work buffers, results and stream.  Batches enqueued alternately on the two handles' streams overlap on the
 * device: the descriptor build, home-cell sort and plan of one run beside the passes over the other's match records.
 * The owner must outlive its views (sgtd_destroy of an owner with views is SGTD_ERR_STATE); after anything that changes
 * the owner's table (sgtd_add*, sgtd_remove_frames, sgtd_load_table, a finalize that merges a tail — the owner's own fifth batch on a tail
 * does) every call of a view that would touch the table again returns SGTD_ERR_STATE until it is attached again: the next
 * query, and for a batch still pending sgtd_sync / sgtd_verify* / sgtd_search_loop / the result calls that gather entries
 * (the view's batch is dropped; nothing reads the owner's freed buffers).  A view cannot add, load or rebuild (SGTD_ERR_STATE).  Neither handle
 * is thread safe; the table itself is only read by queries, so one host thread per handle is fine. */
int sgtd_attach_table(sgtd_handle view, sgtd_handle owner);

/* ---- candidate_selector (STDesc.cpp:318-460) ---------------------------- */
/* Fused query: for every query frame BuildSingleScanSTD (frame id =
 * current_frame_id_, as semantic_graph_localization.cpp:592) followed by
 * candidate_selector.  Enqueues on the stream and returns; results stay on the
 * device until fetched with the sgtd_result_* calls (which synchronise).
 * Inputs must stay valid until the first sgtd_result_* call returns. */
int sgtd_query_frames(sgtd_handle h, const float *xyz, const uint32_t *label,
                      const int64_t *kp_off, int n_queries, int device_ptrs);

/* Sequence loop detection: the reference's per-frame loop build -> SearchLoop -> AddSTDescs
 * (STDesc.cpp:174-315, :84-147, :149-172) over n_frames frames in one batch.  Frames
 * k = 0..n_frames-1 (keypoints kp_off[k]..kp_off[k+1]) are built and added to the table as
 * sgtd_add_frames adds them: frame id c+k, where c = current_frame_id_ on entry, and
 * current_frame_id_ += n_frames.  Each frame is then queried as a batch query q = k.  Its
 * descriptors carry frame id c+k, and only table entries with frame id e such that
 * e + skip_near < c+k count.  skip_near = 0 is the reference's result for build -> SearchLoop ->
 * AddSTDescs run frame after frame (STDesc.cpp:373 under that call order); skip_near > 0 also
 * leaves out the skip_near frames just before the query (upstream STD's skip_near_num_).
 * Results are read as for sgtd_query_frames: sgtd_result_*, sgtd_verify, sgtd_search_loop,
 * sgtd_result_rough.
 * Chunking composes exactly: calls on frames 0..B-1, then B..2B-1, and so on give every frame
 * the result one call on all frames gives — each chunk is added before it is queried, and each
 * query sees only older frames.  That is how a caller stays under sgtd_max_batch, and how an
 * online system calls it every B frames.  Entries already in the table (a map, an earlier
 * session) are searched as the reference's sequential loop would search them.
 * skip_near < 0 and the usual bad arguments: SGTD_ERR_INVALID; a view (sgtd_attach_table) cannot
 * add frames: SGTD_ERR_STATE; a multi-device handle (sgtd_create_multi): SGTD_ERR_UNSUPPORTED
 * (its round-robin frame blocks make the local frame index non-monotonic in the frame id);
 * SGTD_ERR_FRAME_LIMIT as for sgtd_add_frames.  xyz/label are host pointers unless
 * device_ptrs != 0 and must stay valid until the first sgtd_result_* call returns. */
int sgtd_loop_frames(sgtd_handle h, const float *xyz, const uint32_t *label, const int64_t *kp_off,
                     int n_frames, int32_t skip_near, int device_ptrs);

/* candidate_selector on caller-provided descriptors (one query frame). */
int sgtd_query_descs(sgtd_handle h, const sgtd_desc_soa *q, int64_t nq);

/* Results of the last query batch.  For query q:
 *   n_cand[q]                      number of candidates (<= candidate_num)
 *   cand_frame/cand_votes[q*cn+k]  match_id_.second / vote count, in the
 *                                  reference's order (votes desc, frame asc)
 *   pair_off[q*(cn+1)+k]           offsets of candidate k's match_list_ into
 *                                  the pair arrays of query q
 * where cn = candidate_num.  Any pointer may be NULL. */
int sgtd_result_candidates(sgtd_handle h, int32_t *n_cand, int32_t *cand_frame,
                           int32_t *cand_votes, int64_t *pair_off);
/* Asynchronous device-to-device export of the candidate tables of the last
 * batch into caller device buffers (int32 [n_queries*candidate_num] each;
 * unused slots hold frame -1 / votes 0), enqueued on the handle's stream
 * without synchronising: the multi-GPU path all-gathers them with RCCL. */
int sgtd_export_candidates_dev(sgtd_handle h, int32_t *d_cand_frame, int32_t *d_cand_votes);
/* ---- the multi-GPU step (one process per GPU, sgtd_amd/dist.py): every rank holds the table of a
 * frame range (sgtd_config.first_frame_id), sweeps it with the query batch and takes its local top-candidate_num; the
 * local tables travel in ONE all-gather (RCCL) per table group and every rank merges them with the reference's rule
 * (the largest vote count first, ties -> the lowest frame id, >= 5 votes: STDesc.cpp:423-433) — the list a single table
 * gives.  The calls below keep that exchange off the critical path:
 *   sgtd_set_candidate_export   registers a device buffer of sgtd_candidate_export_ints(n_queries, candidate_num) int32;
 *                               from then on every batch writes its local tables there, packed [frames | votes | 4 flag
 *                               words], as soon as they are final — BEFORE its match lists are written (NULL: off)
 *   sgtd_export_wait            makes side_stream wait (on the device) for the last enqueued batch's packed table
 *   sgtd_export_release         recorded on side_stream behind the last reader of the packed table (the all-gather): the
 *                               next batch's export waits for it — neither call blocks the host
 *   sgtd_merge_candidates_dev   the merge as one kernel on `stream`: d_gathered = n_tables packed tables back to back (an
 *                               all-gather's output); outputs int32 [n_queries*candidate_num] frames / votes (unused: -1 / 0)
 *                               and src (table << 8 | slot in the owner's local list, -1 unused), n_cand [n_queries], keep
 *                               u64 [n_queries] (bit s: slot s of table my_table's local list survived; my_table -1: none)
 *                               and flags[0] (bit 0: some table came from a batch that outgrew a work buffer — sgtd_sync
 *                               every rank and exchange again; bit 1: tables of different shapes).  Equal (frame, votes)
 *                               pairs from different tables give ONE merged candidate; its src names one of their slots,
 *                               which one is unspecified, and keep has its bit on that table only (frame-range shards
 *                               never send such pairs).  The kernel holds the keys of a query in registers:
 *                               n_tables * candidate_num <= 1024, beyond that SGTD_ERR_UNSUPPORTED and nothing is written;
 *                               my_table outside [-1, n_tables) or n_tables < 1: SGTD_ERR_INVALID
 *   sgtd_set_deferred_lists /   a batch stops behind its candidate tables; sgtd_finish_lists writes the match lists — of the
 *   sgtd_finish_lists           candidates in d_keep only (NULL: all).  Repeatable (the match records stay intact).  Batches
 *                               whose lists come from the per-block passes (small batches, sgtd_stats.select_form 0) ignore
 *                               both: they always hold every local candidate's list.
 *   sgtd_verify_masked          sgtd_verify for the candidates in d_keep only (the others score -1)
 *   sgtd_gather_verified_dev    verification results of the merged candidates out of the owners' tables: d_gathered =
 *                               n_tables x [score f64 n_queries*cn | pose f64 n_queries*cn*12] (every rank's
 *                               sgtd_export_verify_dev output, all-gathered), d_src = the merge's src
 * Not available on a multi-device handle (that one merges on the host). */
int64_t sgtd_candidate_export_ints(int n_queries, int cand_num);
int sgtd_set_candidate_export(sgtd_handle h, int32_t *d_packed, int64_t capacity_ints);
int sgtd_export_wait(sgtd_handle h, void *side_stream);
int sgtd_export_release(sgtd_handle h, void *side_stream);
int sgtd_merge_candidates_dev(sgtd_handle h, void *stream, const int32_t *d_gathered, int n_tables, int my_table, int n_queries,
                              int32_t *d_frame, int32_t *d_votes, int32_t *d_n_cand, int32_t *d_src, uint64_t *d_keep,
                              int32_t *d_flags);
int sgtd_gather_verified_dev(sgtd_handle h, void *stream, const double *d_gathered, int n_tables, const int32_t *d_src,
                             int n_queries, double *d_score, double *d_pose);
int sgtd_set_deferred_lists(sgtd_handle h, int on);
int sgtd_finish_lists(sgtd_handle h, const uint64_t *d_keep);
int sgtd_verify_masked(sgtd_handle h, const uint64_t *d_keep);

/* number of query descriptors of query q (stds_vec.size()) */
int sgtd_result_query_desc_count(sgtd_handle h, int q, int64_t *n);
/* match_list_ pairs of query q, candidate after candidate, each in the
 * reference's order: q_idx = index into the query's descriptors, db_entry =
 * insertion index of the table entry (use sgtd_fetch_entries).  capacity in
 * pairs; *n_pairs receives the total. */
int sgtd_result_pairs(sgtd_handle h, int q, int32_t *q_idx, int64_t *db_entry,
                      int64_t capacity, int64_t *n_pairs);
/* the query's own descriptors (built on the device by sgtd_query_frames) */
int sgtd_result_query_descs(sgtd_handle h, int q, sgtd_desc_soa *out,
                            int64_t capacity, int64_t *n_out);
/* per-frame vote counts of query q (match_array, STDesc.cpp:323,410):
 * votes[f - frame_lo] for f in [frame_lo, frame_lo + n) */
int sgtd_result_votes(sgtd_handle h, int q, uint32_t *votes, int64_t capacity,
                      uint32_t *frame_lo, int64_t *n);
/* all rough matches of query q in the reference's (i, cell, j) order
 * (STDesc.cpp:378-384): q_idx, voxel_round index 0..26, db_entry, frame, dis.
 * Diagnostic / parity output; any pointer may be NULL.  The first call after a batch re-runs
 * the batch with the diagnostic sweep (the reference's distance test verbatim on the exact f64
 * sides, cell index and distance recorded per match); the product sweep keeps neither. */
int sgtd_result_rough(sgtd_handle h, int q, int32_t *q_idx, int32_t *cell,
                      int64_t *db_entry, uint32_t *frame, double *dis,
                      int64_t capacity, int64_t *n_rough);

/* ---- geometric verification of the candidates of the last batch ----
 * STDescManager::candidate_verify + triangle_solver (STDesc.cpp:462-571) for every
 * (query, candidate) of the batch, on the device: hypotheses = every skip_len-th pair of the
 * candidate's match_list_ (:467-468), votes with the 3.0 inlier radius (:469-505), first
 * maximum, >= 4 votes (:507-515), inliers of the best hypothesis (:516-539).
 * The 3x3 solver is a one-sided Jacobi SVD, not Eigen::JacobiSVD (not available here):
 * parity with the reference binary's SVD is unpinned (rotations agree to rounding, inlier
 * sets can differ only for pairs within rounding of the 3.0 radius). */
int sgtd_verify(sgtd_handle h);
/* verify_score (inlier count, -1 = rejected, :539-541) and relative_pose of every candidate
 * of query q: score[candidate_num], pose[candidate_num*12] = rot row-major (9) then t (3);
 * entries past the query's candidate count hold -1 / zeros.  Either pointer may be NULL. */
int sgtd_result_verify(sgtd_handle h, int q, double *score, double *pose);
/* World pose of every candidate of query q after sgtd_verify: world[k*12 .. k*12+11] = map pose of the candidate's
 * frame composed with its relative pose (3x4 row-major f32); 12 NaNs where the candidate is past n_cand, was
 * rejected (score -1), or its frame has no pose. */
/* world holds candidate_num * 12 floats.  With M the stored pose (sgtd_set_frame_poses) and R, t the relative pose of
 * sgtd_result_verify cast to f32, every operation an f32 rounding (the node's Global_SG[match].pose * loop_transform):
 *   w[i][j] = (M[i][0]*R[0][j] + M[i][1]*R[1][j]) + M[i][2]*R[2][j]
 *   w[i][3] = ((M[i][0]*t[0] + M[i][1]*t[1]) + M[i][2]*t[2]) + M[i][3]
 * Computed in the library's host code; a multi-device handle gives the single-device values bit for bit.  h == NULL,
 * world == NULL, q outside the batch or no verification yet: SGTD_ERR_INVALID. */
int sgtd_result_world_poses(sgtd_handle h, int q, float *world);

/* Least-squares refit of every verified candidate's relative pose over ALL its inlier pairs, on the device, after
 * sgtd_verify (or sgtd_verify_masked, or sgtd_search_frame with flags 0).  sgtd_verify's pose is the motion of one triangle
 * pair (three points); this one averages over the whole inlier set and reports its RMS residual.  iterations >= 1:
 * iteration i >= 2 first re-selects the inliers under the pose of iteration i - 1. */
/* The rule, for candidate k of query q.  All arithmetic is f64, every operation rounded once (no contraction).
 * Inputs: the pairs j = 0 .. n_list-1 of the candidate's match list in list order (sgtd_result_pairs).  A pair of the
 * current set contributes three correspondences (p, w) in the order A, B, C: p = the query descriptor's vertex, w = the
 * table entry's vertex, f32 values widened exactly.  Set 0 is sgtd_verify's inlier set (sgtd_result_inliers).
 * A sum over the set, written SUM below, has this fixed order: 256 accumulators acc[0..255], each starting at +0.0;
 * acc[l] takes the pairs at list positions j == l (mod 256) in ascending j, and of a pair its correspondences A, B, C in
 * that order, one addition each (acc = acc + term); a pair outside the set is skipped, not added as zero.  Then
 * acc[l] = acc[l] + acc[l + s] for all l < s, for s = 128, 64, 32, 16, 8, 4, 2, 1 in turn; SUM = acc[0].  Sums of vectors
 * and matrices are taken component by component.
 * Fit: n = pairs in the set, d = (double)(3 n); cp = SUM(p) / d, cw = SUM(w) / d;
 *   H[i][j] = SUM((p[i] - cp[i]) * (w[j] - cw[j]));
 *   R from H exactly as triangle_solver (STDesc.cpp:558-568) obtains rot from its covariance, with sgtd_verify's 3x3
 *   solver: H = U S V^T (one-sided Jacobi), R = V U^T, and R = V diag(1, 1, -1) U^T when det(V U^T) < 0;
 *   t[i] = -((R[i][0]*cp[0] + R[i][1]*cp[1]) + R[i][2]*cp[2]) + cw[i]     (:569).
 * Residual of a correspondence under a pose (R, t): x[i] = ((R[i][0]*p[0] + R[i][1]*p[1]) + R[i][2]*p[2]) + t[i],
 *   e[i] = x[i] - w[i], r2 = (e[0]*e[0] + e[1]*e[1]) + e[2]*e[2]   (candidate_verify's distance, :488-505, squared).
 * Iteration i >= 2: the next set = every pair of the list whose three correspondences all have r2 < 9.0 under the pose of
 * iteration i - 1 (sqrt(r2) < 3.0, sgtd_verify's exact test).  If it has fewer than 4 pairs, or equals the current set,
 * the loop stops and the result of iteration i - 1 stands; otherwise it becomes the current set and is fitted.
 * Results: pose = (R, t) of the last fit, n_pairs = n of its set, moments = cp, cw, H of that fit,
 *   rmse = sqrt(SUM(r2 under (R, t)) / d), rmse_verify = sqrt(SUM(r2 under sgtd_verify's pose) / d), over that same set.
 * With iterations == 1, n_pairs[k] == score[k] of sgtd_result_verify and rmse <= rmse_verify up to rounding.
 * The call adds results and changes none: sgtd_result_verify, sgtd_result_inliers, sgtd_result_inlier_*, sgtd_search_loop
 * and sgtd_result_world_poses return what they returned before (re-selected sets live in a buffer of their own).  A new
 * batch or a new sgtd_verify* drops the refined results.  A view (sgtd_attach_table) has refined results of its own; a
 * multi-device handle forwards the call to every shard and fetches each candidate's result from its owner.
 * h == NULL or iterations < 1: SGTD_ERR_INVALID, before the device is touched; no verification of the pending batch yet:
 * SGTD_ERR_STATE; a view whose owner's table changed: SGTD_ERR_STATE, as for sgtd_verify. */
int sgtd_refine_poses(sgtd_handle h, int iterations);
/* Refined results of every candidate of query q; cn = candidate_num; any pointer may be NULL.  A candidate without a
 * verification result (past n_cand, score -1, masked out by sgtd_verify_masked) gets 12 zeros, NaN rmse and rmse_verify,
 * 0 pairs and NaN moments.  h == NULL: SGTD_ERR_INVALID; before sgtd_refine_poses on this batch: SGTD_ERR_STATE; q outside
 * the batch: SGTD_ERR_INVALID. */
int sgtd_result_refined(sgtd_handle h, int q,
                        double *pose,        /* [cn*12] rot row-major (9), t (3)             */
                        double *rmse,        /* [cn] residual under the refined pose         */
                        double *rmse_verify, /* [cn] same points, sgtd_verify's pose         */
                        int32_t *n_pairs,    /* [cn] inlier pairs of the final set           */
                        double *moments);    /* [cn*15] cp(3), cw(3), H(9): parity output    */
/* sgtd_result_world_poses with the refined relative pose in place of sgtd_verify's: the same composition rule, in the
 * library's host code (a multi-device handle gives the single-device values bit for bit); 12 NaNs where the candidate
 * has no result or its frame has no pose.  world == NULL: SGTD_ERR_INVALID; otherwise as sgtd_result_refined. */
int sgtd_result_refined_world_poses(sgtd_handle h, int q, float *world);

/* Keypoints of map frames, keyed by global frame id: frame frame_ids[i] gets the keypoints kp_off[i] .. kp_off[i+1] of
 * xyz (3 floats each) / label — host arrays, the data sgtd_add_frames takes for that frame.  They feed sgtd_overlap.
 * The call behaves like sgtd_set_frame_poses: the keypoints are copied at the call and are settings of the handle;
 * later calls overwrite; xyz == NULL with n > 0 forgets the keypoints of those ids; frame_ids == NULL with n == 0 forgets
 * all; ids may name frames not (yet) added; sgtd_add*, sgtd_remove_frames and sgtd_load_table leave them alone, the table
 * file does not hold them, a view (sgtd_attach_table) has keypoints of its own, and a multi-device handle hands each
 * frame to the shard that owns it.  A frame stored with zero keypoints "has keypoints" (count 0).
 * Memory: a host copy, and a device copy built before the next sgtd_overlap and rebuilt only after the store changed:
 * 16 B a keypoint plus an 8-byte offset word per frame id up to the largest id stored.
 * h == NULL, n < 0, frame_ids == NULL with n > 0, kp_off == NULL or label == NULL with xyz != NULL and n > 0, a frame with
 * a negative count or more than 65535 keypoints: SGTD_ERR_INVALID; an id >= max_frame_n: SGTD_ERR_FRAME_LIMIT (nothing
 * is stored).  All before the device is touched. */
int sgtd_set_frame_keypoints(sgtd_handle h, const uint32_t *frame_ids, const int64_t *kp_off,
                             const float *xyz, const uint32_t *label, int64_t n);

/* Keypoint overlap of every verified candidate, on the device, after sgtd_verify (or sgtd_verify_masked, or
 * sgtd_search_frame with flags 0): under the candidate's relative pose, how many of the query's keypoints land within
 * `radius` of a keypoint of the same label of the candidate's frame (sgtd_set_frame_keypoints) — a scale-free quantity
 * to accept or reject a loop on, where verify_score is a count.
 * Pose: sgtd_result_verify's; with SGTD_OVERLAP_REFINED sgtd_result_refined's (SGTD_ERR_STATE when sgtd_refine_poses has
 * not run on this batch).
 * Query keypoints: q_xyz == NULL takes the batch's own, as given to sgtd_query_frames / sgtd_loop_frames — if those were
 * passed with device_ptrs != 0 the caller's arrays must still be valid; a batch of sgtd_query_descs or sgtd_search_frame
 * has none (SGTD_ERR_STATE).  Otherwise q_xyz, q_label and q_kp_off (n_queries + 1 offsets) are host arrays for every
 * query of the batch, used in place of the batch's own (copied before the call returns). */
/* The rule, for candidate k of query q that has a verification result and whose frame has stored keypoints.  All
 * arithmetic is f64, every operation rounded once (no contraction); f32 inputs are widened exactly.  (R, t) = the pose.
 * For query keypoint i = 0 .. n_query_kp-1 with position p and label l:
 *   x[c] = ((R[c][0]*p[0] + R[c][1]*p[1]) + R[c][2]*p[2]) + t[c];
 *   for every keypoint j of the frame whose label equals l (as u32), with position w:
 *     e = x - w, r2(i, j) = (e[0]*e[0] + e[1]*e[1]) + e[2]*e[2];
 *   m_i = the minimum of r2(i, j) over those j, +inf when no j has the label (a NaN r2 never is the minimum).
 * With rr = radius * radius: query keypoint i is a hit iff m_i <= rr; frame keypoint j is a hit iff some query keypoint
 * i of its label has r2(i, j) <= rr.  Any NaN makes a comparison false.
 *   n_hit_query, n_hit_frame = the hits; n_query_kp, n_frame_kp = the set sizes;
 *   overlap = (double)n_hit_query / (double)n_query_kp, NaN when n_query_kp == 0;
 *   rms = sqrt(SUM(m_i over the hits i) / (double)n_hit_query), NaN without hits.
 * SUM has the fixed order of sgtd_refine_poses: 256 accumulators acc[0..255] starting at +0.0; acc[l] takes the query
 * keypoints i == l (mod 256) in ascending i, one addition each; a keypoint that is no hit is skipped, not added as zero;
 * then acc[l] = acc[l] + acc[l + s] for all l < s, for s = 128, 64, 32, 16, 8, 4, 2, 1 in turn; SUM = acc[0].
 * A candidate without a verification result (past n_cand, score -1, masked out by sgtd_verify_masked): all four counts
 * -1, overlap and rms NaN.  A verified candidate whose frame has no stored keypoints: n_frame_kp = -1, both hit counts
 * 0, overlap and rms NaN; n_query_kp is still reported.
 * The call adds results and changes none: sgtd_result_verify, sgtd_result_inlier*, sgtd_result_refined*,
 * sgtd_result_world_poses and sgtd_search_loop return what they returned before.  A new batch or a new sgtd_verify* drops
 * the overlap results; a later sgtd_overlap replaces them (another radius, another pose).  A view has results of its
 * own; a multi-device handle forwards the call to every shard and fetches each candidate's result from its owner (the
 * single handle's values bit for bit).
 * h == NULL, radius NaN, negative or infinite, unknown flag bits, q_xyz set while q_label or q_kp_off is NULL, a query
 * with a negative count or more than 65535 keypoints: SGTD_ERR_INVALID, before the device is touched; no verification of
 * the pending batch yet: SGTD_ERR_STATE; a view whose owner's table changed: SGTD_ERR_STATE, as for sgtd_verify. */
#define SGTD_OVERLAP_REFINED 1   /* use sgtd_refine_poses' pose instead of sgtd_verify's */
int sgtd_overlap(sgtd_handle h, double radius, int flags,
                 const float *q_xyz, const uint32_t *q_label, const int64_t *q_kp_off);
/* Overlap results of every candidate of query q; cn = candidate_num; any pointer may be NULL.  h == NULL:
 * SGTD_ERR_INVALID; before sgtd_overlap on this batch: SGTD_ERR_STATE; q outside the batch: SGTD_ERR_INVALID. */
int sgtd_result_overlap(sgtd_handle h, int q,
                        int32_t *n_query_kp,  /* [cn] */
                        int32_t *n_frame_kp,  /* [cn] */
                        int32_t *n_hit_query, /* [cn] */
                        int32_t *n_hit_frame, /* [cn] */
                        double *overlap,      /* [cn] n_hit_query / n_query_kp */
                        double *rms);         /* [cn] */
/* sgtd_search_loop's rule over the candidates with overlap >= min_overlap (a NaN overlap leaves a candidate out): among
 * them the first candidate with the strictly largest verify_score, accepted if it exceeds icp_threshold.
 * min_overlap <= 0 disables the gate: the choice equals sgtd_search_loop's and the call needs no overlap results.  With
 * min_overlap > 0 it requires sgtd_overlap on the batch (SGTD_ERR_STATE otherwise).  Arrays of n_queries; any may be
 * NULL.  best_overlap: the chosen candidate's overlap; NaN where nothing was accepted or no overlap results exist.
 * h == NULL or no verification yet: SGTD_ERR_INVALID. */
int sgtd_search_loop_overlap(sgtd_handle h, double icp_threshold, double min_overlap,
                             int32_t *best_cand, int32_t *best_frame,
                             double *best_score, double *best_overlap);

/* Label-aware closest-keypoint alignment (ICP over the semantic keypoints) of every verified candidate, on the device,
 * after sgtd_verify (or sgtd_verify_masked, or sgtd_search_frame with flags 0).  sgtd_refine_poses sees only the vertices
 * of matched triangles and sgtd_overlap only measures; this call assigns every query keypoint to the nearest keypoint of
 * its label of the candidate's frame (sgtd_set_frame_keypoints), refits the pose over the assigned pairs and repeats.
 * It hands out the polished pose, sgtd_overlap's figures before and after (rms_after is the registration fitness to
 * re-rank candidates on) and the keypoint-to-keypoint assignment under the final pose.
 * Start pose (R0, t0): sgtd_result_verify's; with SGTD_ALIGN_REFINED sgtd_result_refined's (SGTD_ERR_STATE when
 * sgtd_refine_poses has not run on this batch).  Query keypoints: as for sgtd_overlap (NULL: the batch's own; a batch of
 * sgtd_query_descs or sgtd_search_frame has none, SGTD_ERR_STATE; otherwise host arrays, copied before the call returns). */
/* The rule, for candidate k of query q that has a verification result and whose frame has stored keypoints.  All
 * arithmetic is f64, every operation rounded once (no contraction); f32 inputs are widened exactly.
 * Query keypoints i = 0 .. n-1 with position p_i and label l_i; frame keypoints j = 0 .. m-1 with position w_j and a
 * label; rr = radius * radius; iterations >= 1.
 * Assignment under a pose (R, t): x_i and r2(i, j) are sgtd_overlap's (x[c] = ((R[c][0]*p[0] + R[c][1]*p[1]) + R[c][2]*p[2])
 *   + t[c]; e = x - w; r2 = (e[0]*e[0] + e[1]*e[1]) + e[2]*e[2]).  a(i) = the j of label l_i (as u32) with the smallest
 *   r2(i, j); an equal r2 goes to the lowest j; a NaN r2 is never chosen.  a(i) = -1 when no j has the label (or every
 *   such r2 is NaN), or when the minimum m_i is not <= rr.
 * Iteration it = 1 .. iterations, pose 0 being the start pose: A_it = the assignment under the pose of iteration it - 1.
 *   If fewer than 3 keypoints are assigned, stop: the pose of iteration it - 1 stands.  If it >= 2 and A_it equals
 *   A_(it-1) element for element, stop (converged).  Otherwise fit, with c = (double)(number assigned):
 *     cp = SUM(p_i) / c, cw = SUM(w_a(i)) / c, H[r][s] = SUM((p_i[r] - cp[r]) * (w_a(i)[s] - cw[s]));
 *     R from H exactly as in sgtd_refine_poses (H = U S V^T by sgtd_verify's one-sided Jacobi, R = V U^T, and
 *     R = V diag(1, 1, -1) U^T when det(V U^T) < 0); t[r] = -((R[r][0]*cp[0] + R[r][1]*cp[1]) + R[r][2]*cp[2]) + cw[r];
 *   that is the pose of iteration it.
 * SUM has the fixed order of sgtd_refine_poses and sgtd_overlap: 256 accumulators acc[0..255] starting at +0.0; acc[l]
 * takes the query keypoints i == l (mod 256) in ascending i, one addition each; an unassigned keypoint is skipped, not
 * added as zero; then acc[l] = acc[l] + acc[l + s] for all l < s, for s = 128, 64, 32, 16, 8, 4, 2, 1 in turn; SUM = acc[0].
 * Results: pose = the last pose that stands (the start pose itself when no fit was made); n_fits = fits made;
 *   n_corr = the assigned count of the last fit (0 with no fit); moments = cp, cw, H of the last fit (NaN with no fit);
 *   stop = 0 ran out of iterations, 1 fewer than 3 assigned, 2 converged;
 *   counts_before / overlap_before / rms_before = sgtd_overlap's n_query_kp, n_frame_kp, n_hit_query, n_hit_frame, overlap
 *   and rms, by sgtd_overlap's rule at this radius, under the start pose; *_after = the same under the final pose;
 *   assign = the assignment under the final pose, an int32 per query keypoint (sgtd_result_aligned_pairs).
 * A candidate without a verification result (past n_cand, score -1, masked out by sgtd_verify_masked): pose 12 zeros, the
 * counts -1, n_fits and n_corr 0, stop -1, every double NaN, every assign entry -1.  A verified candidate whose frame has
 * no stored keypoints: n_frame_kp = -1 (n_query_kp is reported), the pose is the start pose, n_fits = 0, stop = 1, the hit
 * counts 0, overlap, rms and moments NaN, every assign entry -1.
 * The call adds results and changes none: sgtd_result_verify, sgtd_result_inlier*, sgtd_result_refined*,
 * sgtd_result_overlap, sgtd_result_world_poses and sgtd_search_loop* return what they returned before.  A new batch or a
 * new sgtd_verify* drops the aligned results; a later sgtd_align_keypoints replaces them.  A view has results of its own;
 * a multi-device handle forwards the call to every shard and fetches each candidate's result from its owner (the single
 * handle's values bit for bit).  Memory: candidate_num int32 per query keypoint of the batch for the assignments.
 * h == NULL, radius NaN, negative or infinite, iterations < 1, unknown flag bits, q_xyz set while q_label or q_kp_off is
 * NULL, a query with a negative count or more than 65535 keypoints: SGTD_ERR_INVALID, before the device is touched; no
 * verification of the pending batch yet: SGTD_ERR_STATE; a view whose owner's table changed: SGTD_ERR_STATE. */
#define SGTD_ALIGN_REFINED 1   /* start from sgtd_refine_poses' pose instead of sgtd_verify's */
int sgtd_align_keypoints(sgtd_handle h, double radius, int iterations, int flags,
                         const float *q_xyz, const uint32_t *q_label, const int64_t *q_kp_off);
/* Aligned results of every candidate of query q; cn = candidate_num; any pointer may be NULL.  h == NULL:
 * SGTD_ERR_INVALID; before sgtd_align_keypoints on this batch: SGTD_ERR_STATE; q outside the batch: SGTD_ERR_INVALID. */
int sgtd_result_aligned(sgtd_handle h, int q,
                        double *pose,            /* [cn*12] rot row-major (9), t (3) */
                        int32_t *n_fits,         /* [cn] */
                        int32_t *n_corr,         /* [cn] */
                        int32_t *stop,           /* [cn] */
                        int32_t *counts_before,  /* [cn*4] n_query_kp, n_frame_kp, n_hit_query, n_hit_frame */
                        int32_t *counts_after,   /* [cn*4] */
                        double *overlap_before,  /* [cn] */
                        double *rms_before,      /* [cn] */
                        double *overlap_after,   /* [cn] */
                        double *rms_after,       /* [cn] */
                        double *moments);        /* [cn*15] cp(3), cw(3), H(9): parity output */
/* The assignment of (query q, candidate cand) under the final pose: frame_kp[i] = the frame keypoint query keypoint i is
 * assigned to, or -1; capacity in elements, *n = needed = the query's keypoint count.  cand outside the query's
 * candidates, q outside the batch, n == NULL: SGTD_ERR_INVALID; more than capacity: SGTD_ERR_CAPACITY (the first
 * `capacity` entries are written); before sgtd_align_keypoints: SGTD_ERR_STATE. */
int sgtd_result_aligned_pairs(sgtd_handle h, int q, int cand, int32_t *frame_kp, int64_t capacity, int64_t *n);
/* sgtd_result_world_poses with the aligned relative pose in place of sgtd_verify's: the same composition rule, in the
 * library's host code; 12 NaNs where the candidate has no result or its frame has no pose.  world == NULL:
 * SGTD_ERR_INVALID; otherwise as sgtd_result_aligned. */
int sgtd_result_aligned_world_poses(sgtd_handle h, int q, float *world);
/* The reference node's choice among registered candidates (the lowest fitness wins), for every query of the batch, in host
 * code: of the candidates with a verification result, overlap_after >= min_overlap (min_overlap <= 0: no bound) and
 * rms_after <= max_rms (max_rms <= 0 or +inf: no bound) — a NaN overlap_after under a bound, or a NaN rms_after, leaves a
 * candidate out — the one with the strictly smallest rms_after; equal rms_after goes to the larger verify_score, then to
 * the lower candidate index.  best_rms / best_overlap: its rms_after and overlap_after.  Nothing qualifies: -1, -1, NaN,
 * NaN.  Arrays of n_queries; any may be NULL.  h == NULL, min_overlap or max_rms NaN: SGTD_ERR_INVALID; without
 * sgtd_align_keypoints on the batch: SGTD_ERR_STATE. */
int sgtd_search_loop_aligned(sgtd_handle h, double min_overlap, double max_rms,
                             int32_t *best_cand, int32_t *best_frame, double *best_rms, double *best_overlap);
/* asynchronous device-to-device export of the verification results of the whole batch into
 * caller device buffers (score f64 [n_queries*candidate_num], pose f64 [n_queries*candidate_num*12]),
 * enqueued on the handle's stream without synchronising: the table-sharded multi-GPU path
 * all-gathers them with RCCL (every candidate frame is verified by the rank that owns it) */
int sgtd_export_verify_dev(sgtd_handle h, double *d_score, double *d_pose);
/* sucess_match_vec of (query q, candidate cand) as positions into that candidate's
 * match_list_ (ascending = list order); capacity in elements, *n = needed */
int sgtd_result_inliers(sgtd_handle h, int q, int cand, int32_t *idx, int64_t capacity, int64_t *n);
/* The inlier pairs of EVERY candidate of query q in one call (one device compaction, one copy):
 * candidate k's pairs are [cand_off[k], cand_off[k+1]) of q_idx / db_entry, in match-list order;
 * cand_off holds candidate_num + 1 offsets.  What SearchLoop needs to fill
 * LOOP_RESULT::loop_std_pair (STDesc.cpp:119-124) without fetching the full match lists. */
int sgtd_result_inlier_pairs(sgtd_handle h, int q, int64_t *cand_off, int32_t *q_idx, int64_t *db_entry,
                             int64_t capacity, int64_t *n_pairs);
/* The same pairs with the table side already fetched: q_idx[i] and entry i of `entries` (the fields whose
 * pointers are set) are the i-th inlier pair — the compaction, the gather of the table entries and the copies
 * run back to back on the device, no list of indices travels to the host and back.  capacity in pairs
 * (the sum of the candidates' list lengths, sgtd_result_candidates' last offset, always suffices);
 * *n_pairs = needed.  SGTD_ERR_CAPACITY leaves cand_off and *n_pairs valid. */
int sgtd_result_inlier_entries(sgtd_handle h, int q, int64_t *cand_off, int32_t *q_idx, sgtd_desc_soa *entries,
                               int64_t capacity, int64_t *n_pairs);
/* STDescManager::SearchLoop's choice (STDesc.cpp:105-146) for every query of the batch:
 * the first candidate with the strictly largest verify_score, accepted if it exceeds
 * icp_threshold; best_frame = -1 and best_score = 0 otherwise (loop_result (-1, 0)).
 * Arrays of n_queries; any may be NULL.  Requires sgtd_verify. */
int sgtd_search_loop(sgtd_handle h, double icp_threshold, int32_t *best_cand, int32_t *best_frame,
                     double *best_score);

/* Pairwise consistency over a list of n loop closures ("edges"), on the device: two loops agree when the cycle "loop i,
 * odometry, loop j back, odometry" closes within max_trans and max_rot; from the agreement graph a mutually consistent
 * set is chosen greedily (largest remaining degree first).  Every stage before this one judges a loop alone; this one
 * drops the loops that verify well against the wrong place (perceptual aliases), which agree with few others. */
/* The rule.  All arithmetic is f64, every operation rounded once (no contraction); f32 inputs are widened exactly.  A
 * pose X is (R, t); stored poses (sgtd_set_frame_poses) and pose_a rows are row-major 3x4 [R | t].
 *   inv(X):    R'[r][c] = R[c][r];  t'[r] = -((R'[r][0]*t[0] + R'[r][1]*t[1]) + R'[r][2]*t[2])
 *   mul(X, Y): R[r][c] = (Xr[r][0]*Yr[0][c] + Xr[r][1]*Yr[1][c]) + Xr[r][2]*Yr[2][c]
 *              t[r]    = ((Xr[r][0]*Yt[0] + Xr[r][1]*Yt[1]) + Xr[r][2]*Yt[2]) + Xt[r]
 * Per edge i: B_i = the stored pose of frame_b[i]; A_i = pose_a row i when pose_a is given, otherwise the stored pose of
 * frame_a[i]; T_i = rel_pose row i; P_i = mul(B_i, T_i), the query's pose in the map's world as loop i sees it (what
 * sgtd_result_world_poses reports, here in f64).  The a side and the b side may live in different world frames (odometry
 * against the map): only relative motions on each side enter.  An edge is valid when both its poses exist and all 36
 * numbers of B_i, A_i, T_i are finite; an id beyond the stored range has no pose, which is no error.
 * Per pair i < j of valid edges: U = mul(inv(P_i), P_j); V = mul(inv(A_j), A_i); Z = mul(U, V);
 *   d2 = (Zt[0]*Zt[0] + Zt[1]*Zt[1]) + Zt[2]*Zt[2];  tr = (Z[0][0] + Z[1][1]) + Z[2][2];
 *   consistent iff d2 <= tt and tr >= min_trace, with tt = max_trans*max_trans and min_trace = 1.0 + 2.0*cos(max_rot),
 *   both computed once on the host and handed back in thresholds[0], thresholds[1].  A NaN makes a comparison false.
 * adj(i, j) = adj(j, i) = the decision of the pair taken with the lower index first; adj(i, i) = 0; an invalid edge has
 * an empty row and column.
 * Choice: P = the valid edges, C empty.  While P is not empty: d(u) = |adj(u) & P| for every u in P; v = the u with the
 * largest d(u), the lowest index among equals; v is appended to C; P = P & adj(v).  C is a clique by construction; it is
 * the greedy choice, not the maximum clique.  (The library shortcuts where the outcome is the rule's: when every d(u)
 * equals |P| - 1 the rest of P joins C in ascending index order.)
 * Results: in_set[i] = 1 for members of C, else 0; degree[i] = |adj(i)|, -1 for an invalid edge; pick[i] = the position
 * at which i was appended to C (0, 1, ...), else -1; *n_set = |C|.  n == 0: nothing is done, *n_set = 0.  One valid
 * edge: C is that edge.
 * sgtd_result_consistency_rows gives rows first .. first + n_rows - 1 of the bit matrix adj, ceil(n / 64) words each:
 * bit j of row i is bit j & 63 of word j >> 6; the padding bits are 0 (parity and diagnostics).
 * The call is independent of the pending batch and of the table and changes no other result; a view (sgtd_attach_table)
 * runs on its own poses whatever state its owner's table is in; a multi-device handle runs on its first device with
 * the group handle's poses.  The work is issued on the handle's stream; the host waits once per group of greedy rounds
 * (the rounds run on the device and fall through once P is empty).  The results last until the next
 * sgtd_consistent_loops call or sgtd_destroy; a call that fails on the device, or with SGTD_ERR_UNSUPPORTED, drops them.
 * Device memory: 8 * n * ceil(n / 64) bytes for the matrix (128 MB at SGTD_MAX_LOOP_EDGES) plus O(n): about 600 bytes an edge
 * and the pose store's copy.
 * h == NULL, n < 0, n_set == NULL, with n > 0: frame_b == NULL, rel_pose == NULL, or frame_a == NULL while
 * pose_a == NULL; max_trans NaN, negative or infinite; max_rot NaN or outside [0, pi]: SGTD_ERR_INVALID, before the
 * device is touched.  n > SGTD_MAX_LOOP_EDGES: SGTD_ERR_UNSUPPORTED (sgtd_last_error says so).  The result calls before
 * a successful run: SGTD_ERR_STATE; rows outside [0, n] (or rows == NULL with n_rows > 0): SGTD_ERR_INVALID. */
#define SGTD_MAX_LOOP_EDGES 32768
int sgtd_consistent_loops(sgtd_handle h, int64_t n,
                          const uint32_t *frame_a,   /* [n] the query-side frame of loop i            */
                          const uint32_t *frame_b,   /* [n] the candidate (map-side) frame            */
                          const double *rel_pose,    /* [n*12] rot row-major (9), t (3): x_b = R p_a + t,
                                                        the layout of sgtd_result_verify / _refined / _aligned */
                          const float *pose_a,       /* NULL, or [n*12] row-major 3x4 [R|t] used in place of
                                                        the stored pose of frame_a (frame_a may then be NULL) */
                          double max_trans, double max_rot /* radians */, int32_t *n_set);
/* arrays of n; any pointer may be NULL */
int sgtd_result_consistent(sgtd_handle h, int32_t *in_set /*[n]*/, int32_t *degree /*[n]*/,
                           int32_t *pick /*[n]*/, double *thresholds /*[2]*/);
int sgtd_result_consistency_rows(sgtd_handle h, int64_t first, int64_t n_rows, uint64_t *rows);
/* The edges sgtd_consistent_loops takes, from the pending verified batch, in host code: one edge for every query q whose
 * sgtd_search_loop choice is accepted at icp_threshold, in ascending q.  query = q; frame_a = the frame id the query's
 * descriptors carry (c + q for a sgtd_loop_frames batch, current_frame_id_ otherwise); frame_b = the chosen candidate's
 * frame; rel_pose = its sgtd_result_verify pose, with SGTD_LOOP_EDGES_REFINED its sgtd_result_refined pose
 * (SGTD_ERR_STATE when sgtd_refine_poses has not run on the batch); score = its verify_score.  Arrays of `capacity`
 * edges, any may be NULL; *n_edges = the number needed; more than capacity: SGTD_ERR_CAPACITY (the first `capacity`
 * edges are written).  Works on a multi-device handle.  A session in chunks appends each chunk's edges on its side and
 * runs one sgtd_consistent_loops over all of them.  h == NULL, n_edges == NULL, capacity < 0 or unknown flag bits:
 * SGTD_ERR_INVALID; no verification of the pending batch yet: SGTD_ERR_STATE. */
#define SGTD_LOOP_EDGES_REFINED 1
int sgtd_result_loop_edges(sgtd_handle h, double icp_threshold, int flags,
                           int32_t *query, uint32_t *frame_a, uint32_t *frame_b, double *rel_pose, double *score,
                           int64_t capacity, int64_t *n_edges);

/* Consensus among the verified candidates of ONE query, for every query of a batch in one launch: a map is a trajectory,
 * so the true place is seen by several neighbouring map frames, and several of a query's up to candidate_num verified
 * candidates measure the same world pose (sgtd_result_world_poses shows them side by side), while a candidate that
 * verifies against the wrong place stands alone or in a small group.  The call groups a query's candidates by the world
 * pose they imply, chooses a mutually consistent set, counts its support and fuses one pose from it: what a caller that
 * localises from one scan against a map with poses (sgtd_set_frame_poses) needs, without odometry and without a session.
 * It is sgtd_consistent_loops' pair test taken inside one query, where the odometry term is the identity. */
/* The rule, for one query with candidates k = 0 .. cn-1 (cn = cand_num <= 64).  All arithmetic is f64, every operation
 * (+, -, *, /, sqrt) rounded once (no contraction); f32 inputs are widened exactly.  inv() and mul() are those of
 * sgtd_consistent_loops; QUAT, UNIT and ROT those of sgtd_relax_poses.
 * Validity: candidate k is valid when k < n_cand, it has a result (score >= 0: neither rejected nor masked out), its frame
 *   has a stored pose B_k (an id beyond the stored range has none, which is no error) and all 24 numbers of B_k and of its
 *   relative pose T_k are finite.  P_k = mul(B_k, T_k).  k ranges over the cand_num slots only: an n_cand above cand_num
 *   counts as cand_num, a negative one as 0.  The frame id is read as a uint32_t (a negative cand_frame names no stored
 *   pose); a score of 0.0 or -0.0 is a result, a NaN score is none.
 * Agreement, for valid k < l: Z = mul(inv(P_k), P_l); d2 = (Zt[0]*Zt[0] + Zt[1]*Zt[1]) + Zt[2]*Zt[2];
 *   tr = (Z[0][0] + Z[1][1]) + Z[2][2]; the pair agrees iff d2 <= tt and tr >= min_trace, with tt = max_trans*max_trans and
 *   min_trace = 1.0 + 2.0*cos(max_rot) computed once on the host as sgtd_consistent_loops computes them and handed back
 *   in thresholds[0], thresholds[1].  A NaN makes a comparison false.  adj(k, l) = adj(l, k) = the decision taken with the
 *   lower index first; adj(k, k) = 0; an invalid candidate has an empty row and column.  (sgtd_consistent_loops' decision
 *   for two edges that share one pose_a: mul with the identity changes no bit of what the test reads.)
 * Choice: sgtd_consistent_loops' greedy rule over the valid candidates: the largest remaining degree first, the lowest
 *   index among equals, P = P & adj(v) after each pick v (with its shortcut, whose outcome is the rule's).  The seed is the
 *   first pick; the members m_0 < m_1 < ... are taken in ascending candidate index; n_set is their count.
 * Fusion: that[c] = (P_m.t[c] added one by one in ascending m from +0.0) / (double)n_set.  q_m = QUAT(rotation of P_m);
 *   s_m = ((w*w_s + x*x_s) + y*y_s) + z*z_s against the seed's quaternion q_s; s_m < 0 negates all four components of q_m.
 *   Q = their component-wise sum in ascending m from +0.0; qhat = UNIT(Q); Rhat = ROT(qhat).  The fused pose is
 *   [Rhat | that], row-major 3x4 f64 (the layout of sgtd_relax_poses' pose0).
 * Figures per query: n_valid, n_set, seed, the member mask (bit k of a u64);
 *   support_score = the members' scores added in ascending m from +0.0;
 *   spread_t2 = the maximum over the members of (e[0]*e[0] + e[1]*e[1]) + e[2]*e[2], e = P_m.t - that;
 *   spread_trace = the minimum over the members of (r[0] + r[1]) + r[2],
 *     r[i] = (Rhat[i][0]*R_m[i][0] + Rhat[i][1]*R_m[i][1]) + Rhat[i][2]*R_m[i][2]
 *   (both start from the first member's value; then m = v > m ? v : m, respectively v < m ? v : m, in ascending m).
 *   A query without a valid candidate: n_set 0, seed -1, mask 0, NaN pose and spreads, support_score 0.
 * Per candidate (parity and diagnostics): the row adj(k) as a u64; degree = |adj(k)|, -1 when invalid; pick = the
 *   position in the greedy order, else -1.
 * sgtd_pose_consensus_rows takes caller host arrays for all queries back to back, in the layouts of
 * sgtd_result_candidates (n_cand[n_queries], cand_frame[n_queries*cand_num]) and sgtd_result_verify
 * (score[n_queries*cand_num], rel_pose[n_queries*cand_num*12]); it uses the handle's stored poses and is independent of
 * the pending batch and of the table, as sgtd_consistent_loops is; the arrays are copied before the call returns.
 * sgtd_pose_consensus is the same over the pending verified batch, on a single-device handle without a round trip
 * through the host: the kernel reads the batch's candidates, scores and poses where the earlier stages left them, and the
 * call only enqueues.  flags 0 takes sgtd_verify's pose, SGTD_CONSENSUS_REFINED sgtd_refine_poses', SGTD_CONSENSUS_ALIGNED
 * sgtd_align_keypoints'; SGTD_ERR_STATE when that stage (or sgtd_verify) has not run on the batch; both flags together or
 * unknown bits: SGTD_ERR_INVALID.
 * The results last until the next consensus call (either form) or sgtd_destroy; a new batch or a new sgtd_verify* also
 * drops the batch form's results; a failed call drops them.  The call changes no other result.  A view (sgtd_attach_table)
 * uses its own poses and has results of its own; a multi-device handle gathers each candidate's result from its owner
 * and runs the rows form on its first device with the group's poses (the single handle's values bit for bit).
 * Device memory: 140 + 16 * cand_num bytes a query, the rows form's inputs and the pose store's copy.
 * h == NULL, a negative count, a NULL array with a positive count, cand_num outside [1, 64], max_trans NaN, negative or
 * infinite, max_rot NaN or outside [0, pi], min_support < 1: SGTD_ERR_INVALID, before the device is touched.  The getters
 * before a successful run: SGTD_ERR_STATE; q or a range outside the run: SGTD_ERR_INVALID.  n_queries == 0 does nothing. */
#define SGTD_CONSENSUS_REFINED 1   /* fuse sgtd_refine_poses' poses    */
#define SGTD_CONSENSUS_ALIGNED 2   /* fuse sgtd_align_keypoints' poses */
int sgtd_pose_consensus_rows(sgtd_handle h, int64_t n_queries, int cand_num,
                             const int32_t *n_cand,      /* [n_queries]                 */
                             const int32_t *cand_frame,  /* [n_queries*cand_num]        */
                             const double *score,        /* [n_queries*cand_num]        */
                             const double *rel_pose,     /* [n_queries*cand_num*12] rot row-major (9), t (3) */
                             double max_trans, double max_rot /* radians */);
int sgtd_pose_consensus(sgtd_handle h, double max_trans, double max_rot /* radians */, int flags);
/* the per-query figures of queries first .. first + n - 1; any pointer may be NULL */
int sgtd_result_consensus(sgtd_handle h, int64_t first, int64_t n,
                          double *pose,           /* [n*12] row-major 3x4 [R | t] */
                          int32_t *n_valid, int32_t *n_set, int32_t *seed, /* [n] each */
                          uint64_t *mask,         /* [n] bit k: candidate k is a member */
                          double *support_score, double *spread_t2, double *spread_trace, /* [n] each */
                          double *thresholds);    /* [2] tt, min_trace */
/* the per-candidate outputs of query q: arrays of the run's cand_num; any pointer may be NULL */
int sgtd_result_consensus_rows(sgtd_handle h, int q, uint64_t *rows, int32_t *degree, int32_t *pick);
/* SearchLoop's choice under consensus, for every query of the batch form's results, in host code: a query is accepted
 * when n_set >= min_support (min_support >= 1); its choice is the member with the strictly largest verify_score, the
 * first among equals; otherwise -1, -1, 0.  support = n_set, accepted or not.  Arrays of n_queries; any may be NULL.
 * After sgtd_pose_consensus_rows (no batch stands behind those results): SGTD_ERR_STATE. */
int sgtd_search_loop_consensus(sgtd_handle h, int min_support, int32_t *best_cand, int32_t *best_frame,
                               double *best_score, int32_t *support);
/* One edge per accepted query, in ascending q, with the conventions of sgtd_result_loop_edges (query, frame_a, capacity,
 * *n_edges, SGTD_ERR_CAPACITY): frame_b = the chosen member's frame, with B its stored pose rel_pose = mul(inv(B), fused)
 * in the rule's f64 arithmetic (rot row-major (9), t (3)), score = support_score.  The edges feed sgtd_consistent_loops
 * and sgtd_relax_poses unchanged.  h == NULL, n_edges == NULL, capacity < 0, min_support < 1: SGTD_ERR_INVALID; state
 * errors as sgtd_search_loop_consensus. */
int sgtd_result_consensus_edges(sgtd_handle h, int min_support, int32_t *query, uint32_t *frame_a, uint32_t *frame_b,
                                double *rel_pose, double *score, int64_t capacity, int64_t *n_edges);

/* Pose-graph relaxation on the device: the trajectory that honours a set of relative-pose measurements ("edges"), the
 * last stage behind sgtd_consistent_loops.  A generic graph in caller arrays: n_nodes poses X_v (pose0 holds the start,
 * row-major 3x4 [R | t]), n_edges measurements Z_k ~ inv(X_i) X_j between nodes i = node_i[k] and j = node_j[k] in the
 * rel_pose layout (rot row-major (9), t (3)), weights w_trans[k], w_rot[k] (NULL = 1.0 each), and held nodes
 * (fixed[v] != 0; fixed == NULL holds node 0 alone).  Orientation, as for sgtd_consistent_loops: a loop edge (frame_a,
 * frame_b, T with x_b = R p_a + t) is i = frame_b's node, j = frame_a's node, Z = T; an odometry edge between
 * consecutive frames with poses A_k, A_k+1 is i = k, j = k + 1, Z = mul(inv(A_k), A_k+1).
 * The two uses:
 *   a session closed against itself: nodes = its frames, pose0 = its odometry, edges = the odometry edges and the loops
 *     sgtd_consistent_loops kept, node 0 held (fixed == NULL): the result is the odometry with its drift pulled out;
 *   a session against a fixed map: nodes = the map frames the loops name, held at their stored poses B, and the query
 *     frames, free, started from P = mul(B, T) of one loop carried along the odometry (P_k+1 = mul(P_k, mul(inv(A_k),
 *     A_k+1))); edges = the odometry edges and the loops: the result is the session's trajectory in the map's world.
 * The rule.  All arithmetic is f64, every operation (+, -, *, /, sqrt) rounded once, no contraction, nothing else is
 * used; inv() and mul() are those of sgtd_consistent_loops.
 *   QUAT(R) -> q = (w, x, y, z): tr = (R00 + R11) + R22;
 *     tr > 0:                         s = sqrt(tr + 1.0) * 2.0;                 q = (0.25*s, (R21-R12)/s, (R02-R20)/s, (R10-R01)/s)
 *     else R00 > R11 and R00 > R22:   s = sqrt(((1.0 + R00) - R11) - R22) * 2.0;  q = ((R21-R12)/s, 0.25*s, (R01+R10)/s, (R02+R20)/s)
 *     else R11 > R22:                 s = sqrt(((1.0 + R11) - R00) - R22) * 2.0;  q = ((R02-R20)/s, (R01+R10)/s, 0.25*s, (R12+R21)/s)
 *     else:                           s = sqrt(((1.0 + R22) - R00) - R11) * 2.0;  q = ((R10-R01)/s, (R02+R20)/s, (R12+R21)/s, 0.25*s)
 *     then UNIT(q): nn = ((w*w + x*x) + y*y) + z*z; every component divided by sqrt(nn).
 *   ROT(q): R00 = 1.0 - 2.0*(y*y + z*z); R01 = 2.0*(x*y - w*z); R02 = 2.0*(x*z + w*y);
 *           R10 = 2.0*(x*y + w*z); R11 = 1.0 - 2.0*(x*x + z*z); R12 = 2.0*(y*z - w*x);
 *           R20 = 2.0*(x*z - w*y); R21 = 2.0*(y*z + w*x); R22 = 1.0 - 2.0*(x*x + y*y).
 *   M v and M^T v of a 3x3 M: (M v)[r] = (M[r][0]*v[0] + M[r][1]*v[1]) + M[r][2]*v[2]; M^T v the same over M[.][r];
 *   |v|2 = (v[0]*v[0] + v[1]*v[1]) + v[2]*v[2].
 *   SUM over elements e = 0, 1, ...: SGTD_RELAX_SUM_W accumulators start at +0.0, element e is added to accumulator
 *     e mod W in ascending e, then acc[l] = acc[l] + acc[l + s] for l < s, s = W/2, W/4, ..., 1; the sum is acc[0].
 *     MAX the same with m = v > m ? v : m.  DOT(u, v) over node vectors = SUM of u[e]*v[e], e = 6*node + a.
 * State of node v: q_v = QUAT(R of pose0 row v), t_v, R_v = ROT(q_v) (what every residual uses, held nodes included).
 * Residual of edge k = (i, j): D = mul(inv(X_i), X_j) with X = (R_v, t_v); E = mul(inv(Z_k), D); r_t = E's translation;
 *   q_E = QUAT(E's rotation), its (x, y, z) negated when its w < 0; r_R = 2.0 * that (no angle is taken: monotone up to
 *   180 degrees).  ct_k = w_trans[k] * |r_t|2, cr_k = w_rot[k] * |r_R|2 (the two numbers sgtd_result_relaxed gives per
 *   edge), c_k = ct_k + cr_k, cost = SUM of c_k over the edges.
 * Linearisation at the current state, right-multiplicative (X_v <- X_v (dR, dt): t_v += R_v dt, q_v <- UNIT(q_v (x)
 * (1, dtheta/2))), with the usual first-order pose-graph blocks, exact at zero rotational residual: with A = the
 * rotation of inv(Z_k), u = D's translation, B = A [u]x (B[r][0] = A[r][1]*u[2] - A[r][2]*u[1]; B[r][1] = A[r][2]*u[0]
 * - A[r][0]*u[2]; B[r][2] = A[r][0]*u[1] - A[r][1]*u[0]), E_R and D_R the rotations of E and D:
 *   d r_t / d(dt_i) = -A;  d r_t / d(dtheta_i) = B;  d r_t / d(dt_j) = E_R;  d r_R / d(dtheta_i) = -D_R^T;
 *   d r_R / d(dtheta_j) = I; the other blocks are 0.
 *   J^T y of one edge, y = (y_t, y_R): to node i ( -(A^T y_t), (B^T y_t) - (D_R y_R) ), to node j ( E_R^T y_t, y_R ).
 *   GATHER(y) of a free node: from +0.0, its incident edges' shares added in ascending edge index; of a held node: 0.
 *   g = GATHER(w_trans r_t, w_rot r_R).  H_vv[a][b] = from +0.0, over the incident edges in ascending index and the
 *   edge's six residual rows r in ascending order, + (w_r * J[r][a]) * J[r][b], J the edge's 6x6 block for this node
 *   (rows r_t, r_R; columns dt, dtheta; zeros and the identity written out), w_r = w_trans for r < 3, else w_rot.
 * Step: (H + lambda diag-blocks(H)) x = -g by preconditioned CG.  M_v = H_vv + lambda*H_vv elementwise = L L^T, column
 *   c = 0..5: s = M[c][c] - L[c][0]^2 - ... - L[c][c-1]^2 (subtracted in that order), L[c][c] = sqrt(s), below it
 *   L[r][c] = (M[r][c] - L[r][0]*L[c][0] - ...) / L[c][c]; a node is solvable when it is free and every s > 0.
 *   z = M^-1 r: y[a] = (r[a] - L[a][0]*y[0] - ...) / L[a][a], a = 0..5; z[a] = (y[a] - L[a+1][a]*z[a+1] - ... -
 *   L[5][a]*z[5]) / L[a][a], a = 5..0; z = 0 for a node that is not solvable: it does not move (an isolated free node).
 *   The block is taken whole: a free node all of whose edges have w_rot == 0 (or all w_trans == 0) has a singular
 *   block and does not move either, not even in the part its edges do determine; give such edges a small weight.
 *   r = -g (0 for held nodes), x = 0, p = 0, z = M^-1 r, rz = rz0 = DOT(r, z), beta = 0.  rz0 > 0 fails: the solve ends
 *   "converged" at once (a zero gradient; no iteration is counted).  Up to max_inner times: p = z + beta*p;
 *   Ap: per edge e_t = ((B b_i) - (A a_i)) + (E_R a_j), e_R = b_j - (D_R^T b_i) with p_v = (a_v, b_v), y = (w_trans e_t,
 *   w_rot e_R), Ap_v = GATHER(y)_v + lambda*(H_vv p_v) ((H p)[a] summed left to right over b; 0 for held nodes);
 *   pq = DOT(p, Ap); pq > 0 fails: CG ends; alpha = rz/pq; x = x + alpha*p; r = r - alpha*Ap; z = M^-1 r; rz' = DOT(r, z);
 *   one CG iteration is counted; rz' <= (cg_tol*cg_tol)*rz0: CG ends; beta = rz'/rz; rz = rz'.
 * Trial: every solvable node moves by x_v = (dt, dtheta): t' = (R_v dt) + t_v; h = 0.5*dtheta;
 *   w' = ((w - x*h0) - y*h1) - z*h2;  x' = ((x + w*h0) + y*h2) - z*h1;  y' = ((y + w*h1) + z*h0) - x*h2;
 *   z' = ((z + w*h2) + x*h1) - y*h0;  q' = UNIT(..), R' = ROT(q'); every other node keeps its state bit for bit.
 *   cost' = the cost at the trial state; maxd = MAX of |x[e]|.  One outer iteration is counted.
 *   cost' < cost: the trial becomes the state, lambda = max(lambda/3.0, lambda_min), and maxd <= step_tol ends the solve
 *   "converged"; otherwise the state stays, lambda = 3.0*lambda, and lambda > lambda_max ends it "damping limit".
 *   Otherwise max_outer iterations end it "outer limit".  So cost_after <= cost_before always; when no step is accepted
 *   the poses are the start's state (R = ROT(QUAT(.)) of pose0, its t), cost_after = cost_before and the edge costs are
 *   the start's.  Every node held: the cost is evaluated, status "nothing free".
 * Results: pose row v = [R_v | t_v] of the final state; edge_cost[2k], [2k+1] = ct_k, cr_k there.
 * The call is a pure function of its arguments: independent of the pending batch, the table and the stored poses; a
 * view runs whatever state its owner's table is in; a multi-device handle runs on its first device.  The work is issued
 * on the handle's stream; every decision is taken on the device, the host enqueues SGTD_RELAX_GROUP outer iterations at a
 * time and reads the state once per group.  The results last until the next successful or device-failed
 * sgtd_relax_poses call or sgtd_destroy.  Device memory: about 1 KB a node and 500 bytes an edge.
 * h == NULL, a negative count, with a positive count: pose0, node_i, node_j or meas NULL; a node index outside
 * [0, n_nodes), node_i[k] == node_j[k]; a non-finite pose0, meas or weight, a negative weight; an option that is not
 * finite and > 0: SGTD_ERR_INVALID, before the device is touched and with the earlier results kept.  More than
 * SGTD_RELAX_MAX_NODES nodes or SGTD_RELAX_MAX_EDGES edges: SGTD_ERR_UNSUPPORTED.  n_nodes == 0 or n_edges == 0: nothing
 * is done, the report is "nothing free" with zero costs and lambda_init, and sgtd_result_relaxed then writes nothing
 * (with n_nodes > 0 and no edge too: no pose comes back, the caller keeps pose0).
 * sgtd_result_relaxed before a successful run: SGTD_ERR_STATE; either of its arrays may be NULL. */
#define SGTD_RELAX_SUM_W 1024
#define SGTD_RELAX_GROUP 4
#define SGTD_RELAX_MAX_NODES (1 << 22)
#define SGTD_RELAX_MAX_EDGES (1 << 22)
enum { SGTD_RELAX_CONVERGED = 0, SGTD_RELAX_OUTER_LIMIT = 1, SGTD_RELAX_DAMPING_LIMIT = 2, SGTD_RELAX_NOTHING_FREE = 3 };
typedef struct sgtd_relax_options {
  int32_t max_outer;      /* outer (Levenberg-Marquardt) iterations, default 50 */
  int32_t max_inner;      /* CG iterations per outer iteration, default 64      */
  double lambda_init;     /* 1e-4 */
  double lambda_min;      /* 1e-9 */
  double lambda_max;      /* 1e9  */
  double cg_tol;          /* 1e-4: CG ends when r^T z <= cg_tol^2 * its start   */
  double step_tol;        /* 1e-6: metres and radians                           */
} sgtd_relax_options;
typedef struct sgtd_relax_report {
  double cost_before, cost_after, lambda;      /* lambda: the damping the solve ended with */
  int32_t outer_iterations, steps_accepted, cg_iterations, status;
} sgtd_relax_report;
void sgtd_default_relax_options(sgtd_relax_options *opt);
int sgtd_relax_poses(sgtd_handle h, int64_t n_nodes, const double *pose0, const uint8_t *fixed,
                     int64_t n_edges, const int32_t *node_i, const int32_t *node_j, const double *meas,
                     const double *w_trans, const double *w_rot,
                     const sgtd_relax_options *opt /* NULL = defaults */, sgtd_relax_report *report /* may be NULL */);
int sgtd_result_relaxed(sgtd_handle h, double *pose /*[n*12]*/, double *edge_cost /*[m*2]: trans, rot*/);

/* One query frame through candidate_selector (STDesc.cpp:318-460), candidate_verify for every candidate (:462-571) and the
 * inlier pairs of every candidate with the table entries they name — what SearchLoop (:84-147) needs — in ONE call: the
 * reference's one-frame-per-call pattern (semantic_graph_localization.cpp:590-603).  Equal, value for value, to
 * sgtd_query_descs + sgtd_verify + sgtd_result_candidates + sgtd_result_verify(0) + sgtd_result_inlier_entries(0), which
 * wait for the device eight times and issue some sixty small copies between them; this call enqueues everything behind
 * the batch and waits once: the small results arrive as one packed block, the entries where the caller wants them.  Output arrays of
 * candidate_num (pair_off, inlier_off: candidate_num + 1; pose: candidate_num * 12) elements; any pointer may be NULL.
 * capacity = room (pairs) in inlier_q_idx / entries; n_inliers = needed.  SGTD_ERR_CAPACITY leaves everything but the
 * inlier pairs valid — sgtd_result_inlier_entries(h, 0, ...) with more room fetches them.  The handle afterwards is in
 * the state the five calls leave (every sgtd_result_* call works).  Not on a multi-device handle (SGTD_ERR_UNSUPPORTED).
 * inlier_q_idx and the members of `entries` are best given as sgtd_host_alloc memory (page-locked, `capacity` entries each): the
 * device then writes the inlier pairs in place and the call has one wait; ordinary arrays are filled from a page-locked block of
 * the handle's with memcpy (same results).  On SGTD_ERR_CAPACITY the first `capacity` pairs may or may not have been written.
 * flags = SGTD_FRAME_LISTS_ONLY: candidate_selector ALONE (STDesc.cpp:318-460), for a node that keeps its own candidate_verify —
 * no verification (score and pose are not written; the handle is left as sgtd_query_descs leaves it), and the pairs handed
 * back are ALL pairs of every candidate's match_list_, in the reference's order: inlier_off = pair_off, n_inliers = their
 * number, inlier_q_idx / entries = the query descriptor and the table entry of every pair.  Equal to sgtd_query_descs +
 * sgtd_result_candidates + sgtd_result_pairs + sgtd_fetch_entries, in one call and one wait.  On SGTD_ERR_CAPACITY call again
 * with room for n_inliers pairs. */
#define SGTD_FRAME_LISTS_ONLY 1   /* sgtd_frame_search.flags: candidate_selector alone (below) */
typedef struct sgtd_frame_search {
  int32_t n_cand;           /* out */
  int32_t flags;            /* in: 0, or SGTD_FRAME_LISTS_ONLY (the field was `reserved`, always 0, before)                 */
  int32_t *cand_frame;      /* out [candidate_num]: match_id_.second, votes descending / frame ascending            */
  int32_t *cand_votes;      /* out [candidate_num]                                                                  */
  int64_t *pair_off;        /* out [candidate_num + 1]: offsets of the candidates' match lists (their lengths)      */
  double *score;            /* out [candidate_num]: verify_score (-1: rejected)                                     */
  double *pose;             /* out [candidate_num * 12]: rot row-major (9), t (3)                                   */
  int64_t *inlier_off;      /* out [candidate_num + 1]: candidate k's inlier pairs are [inlier_off[k], inlier_off[k + 1]) */
  int32_t *inlier_q_idx;    /* out [capacity]: query descriptor of inlier pair i                                    */
  sgtd_desc_soa entries;    /* out: table entry of inlier pair i (arrays of capacity descriptors; NULL members skipped) */
  int64_t capacity;         /* in                                                                                   */
  int64_t n_inliers;        /* out                                                                                  */
} sgtd_frame_search;
int sgtd_search_frame(sgtd_handle h, const sgtd_desc_soa *q, int64_t nq, sgtd_frame_search *io);

/* ---- persistent table ----
 * The reference rebuilds data_base_ from the map files at every start
 * (semantic_graph_localization.cpp:419-458) and only ever appends (STDesc.cpp:149-172).
 * sgtd_save_table writes the table in insertion order (all descriptor fields, the frame
 * counter, the frame range); sgtd_load_table replaces the handle's table with a saved one —
 * the probe layout is re-derived by the next query (a sort of ~1 ms per 4 M entries), and
 * sgtd_add / sgtd_add_frames keep appending after it (new session on an old map).  The file
 * records std_side_resolution (sides are stored scaled): loading into a handle configured
 * differently is SGTD_ERR_INVALID.  I/O problems are SGTD_ERR_IO (sgtd_last_error names the file). */
int sgtd_save_table(sgtd_handle h, const char *path);
int sgtd_load_table(sgtd_handle h, const char *path);

/* ---- graph-JSON ingest (host code, no device needed) ----
 * readGraphFromFile / fromJSON (include/Semantic_Graph.hpp:122-184) + Graph2CloudL
 * (include/utility.hpp:646-659) for many files at once: {"nodes":[int], "centers":[[x,y,z]],
 * "poses":[12 floats], ...} (producer get_json.cpp:332-341; only these three keys are read;
 * numbers as nlohmann::json stores and casts them — integer tokens through strtoull / strtoll, the rest through
 * strtod, then get<float>() / get<int>() — pinned bit for bit against that library by
 * tests/cpp/test_ingest_nlohmann.cpp; a key that occurs twice keeps its LAST value like nlohmann::json 3.2 and later, its
 * first like 3.1.1 when SGTD_JSON_DUPLICATE_KEYS=first is set in the environment) parsed on
 * n_threads host threads into the arrays sgtd_add_frames / sgtd_query_frames take.  Frames
 * keep the order of `paths`.  On SGTD_ERR_IO *out still holds an object whose
 * sgtd_graphs_error() names the file ("Error opening file: ..." like Semantic_Graph.hpp:173);
 * free it with sgtd_graphs_free. */
typedef struct sgtd_graph_batch sgtd_graph_batch;
int sgtd_graphs_load(const char *const *paths, int n_files, int n_threads, sgtd_graph_batch **out);
/* binary cache of a parsed batch (skips JSON parsing at the next start) */
int sgtd_graphs_save_cache(const sgtd_graph_batch *b, const char *path);
int sgtd_graphs_load_cache(const char *path, sgtd_graph_batch **out);
/* borrowed pointers, valid until sgtd_graphs_free: xyz f32 [n_keypoints*3], label u32
 * [n_keypoints], kp_off i64 [n_frames+1], poses f32 [n_frames*12]; any pointer may be NULL */
int sgtd_graphs_view(const sgtd_graph_batch *b, int *n_frames, int64_t *n_keypoints, const float **xyz,
                     const uint32_t **label, const int64_t **kp_off, const float **poses);
const char *sgtd_graphs_error(const sgtd_graph_batch *b);
void sgtd_graphs_free(sgtd_graph_batch *b);

/* ---- labelled scans to keypoints (scan_kernels.hip.h) ----
 * What the reference's producer create_semantic_graph does on the CPU (src/sgtd/src/get_json.cpp:41-343: per semantic
 * class, DCVC clustering of the class's points, src/sgtd/include/cluster_manager.hpp:139-421, then one centroid and node
 * label per cluster) for a batch of scans on the device: points f32 (x y z, or x y z intensity: the .bin layout) and
 * labels u32 (sem | inst << 16: the .label layout) in, the xyz f32 + label u32 keypoints of sgtd_add_frames /
 * sgtd_query_frames / sgtd_loop_frames out.
 *
 * The reference's clustering cannot be reproduced bit for bit: DCVC() (:272-355) is one sequential sweep whose partition
 * depends on the order of the points and may split a connected group of voxels (:288, :332-334), labelAnalysis walks a
 * std::unordered_map (:408), points outside the range gate keep an unset polarCor entry and are clustered all the same
 * (:198,205), and the neighbour set is asymmetric at the azimuth seam (:377), at the top pitch layer (:213,235,370) and
 * at y > polarNum.  This call computes the fixed point the sweep approximates — the connected components of the
 * symmetrised curved-voxel graph — with every order fixed by point index.  Every sweep cluster lies inside one component.
 *
 * Arithmetic: f64, every operation rounded once (no contraction), f32 inputs widened exactly.
 * Per point: sem = label & 0xFFFF, inst = label >> 16, class s = sem.  Dropped: s >= 32, node_label[s] == 0, or a
 *   coordinate that is not finite.
 * Per (scan, class): mode 1 (instances) when any kept point of the class has inst != 0 (get_json.cpp:138), else mode 2.
 * Mode 1: one cluster per distinct inst (0 included), kept when its count > min_instance_points, in ascending inst order.
 * Mode 2: r = sqrt((x*x + y*y) + z*z); in range iff neither r >= max_range nor r <= min_range (:198; points out of
 *   range are dropped — a departure: the reference clusters garbage for them); pitch = (asin(z / r) * 180.0) / pi;
 *   a = atan2(y, x), azimuth = ((a > 0.0 ? a : a + 2.0 * pi) * 180.0) / pi (:178-196; the device math library's f64
 *   asin and atan2).  minPitch = maxPitch = 0.0 and minPolar = maxPolar = 5.0 to start with, then the min / max over the
 *   in-range points (:200-203,482-485).  width = (int)(round(360.0 / delta_a) + 1.0), height = (int)((maxPitch -
 *   minPitch) / delta_p); ring bounds (:214-220): range = minPolar, step = 1, while range <= maxPolar: range = range +
 *   (start_r - step * delta_r), append, step++; polarNum = their number.  polar = the first k with r < bound[k], else
 *   polarNum - 1 (:259-264); pit = (int)round((pitch - minPitch) / delta_p), azi = (int)round(azimuth / delta_a), C's
 *   round (:234-237).  N(v) = searchKNN's set (:365-385) with its hard-coded 300 read as width - 1 (its value at the
 *   shipped delta_a).  Two occupied voxels u, v are linked iff v is in N(u) or u is in N(v) (a departure: the reference
 *   follows N one way); the points of a voxel belong together; clusters = the connected components, kept when their
 *   count >= min_seg[s] (:409), ordered by their smallest point index (a departure: the reference's order is that of
 *   an unordered_map).
 * Keypoints of a scan: classes in ascending s, within a class the order above; label = node_label[s]; n_points = the
 *   cluster's count; each centre coordinate = (float)(SUM / (double)n_points), SUM in the fixed order: 256 accumulators
 *   from +0.0, the cluster's points in ascending point index, the point of rank k to accumulator k mod 256, then
 *   acc[l] += acc[l + w] for l < w, w = 128, ..., 1 (a departure by rounding only from the running f32 sum of
 *   get_json.cpp:266-274).  The edges and weights of gen_graphs (get_json.cpp:301-329) are not produced (nothing
 *   downstream reads them); no file is read in C.
 *
 * sgtd_scan_keypoints leaves the keypoints on the device; it is independent of the pending batch, the table and the
 * stored poses, uses buffers of its own, and its results last until the next scan call, the next
 * sgtd_local_map_keypoints (which clusters in the same work buffers: the scan getters return SGTD_ERR_STATE after it
 * until a scan call has run again) or sgtd_destroy.  points and
 * labels are host arrays, or device arrays with device_ptrs != 0; pt_off (n_scans + 1 offsets, in points) is a host
 * array.  sgtd_scan_device_view hands out borrowed device pointers (xyz f32 [n_keypoints * 3], label u32): with the
 * fetched kp_off they are what sgtd_add_frames / sgtd_query_frames / sgtd_loop_frames take with device_ptrs = 1.  A view
 * (sgtd_attach_table) runs the call whatever state its owner's table is in; a multi-device handle runs it on its first
 * device (its tables take host arrays: fetch the keypoints for them).  sgtd_result_scan_point_clusters: cluster[i] = the index within the scan of the keypoint point i went into,
 * or -1.  sgtd_result_scan_grids: grid rows per class = mode (0 none, 1 instance, 2 voxel), polarNum, width, height
 * (zeros unless mode 2); range rows = minPitch, maxPitch, minPolar, maxPolar (zeros unless mode 2).
 *
 * Errors, before the device is touched: h == NULL, a negative count, a NULL array with a positive count, stride_floats
 * neither 3 nor 4, offsets that decrease (or pt_off[0] != 0), a config value that is not finite and positive (delta_r may
 * be 0), min_range >= max_range, a node_label outside [0, 2^31), a negative min_seg or min_instance_points:
 * SGTD_ERR_INVALID.  More than SGTD_SCAN_MAX_SCANS scans or SGTD_SCAN_MAX_POINTS points in a batch, more than 1024
 * azimuth cells (width), pitch layers (180 / delta_p + 2) or rings: SGTD_ERR_UNSUPPORTED (sgtd_last_error says which).
 * The ring sequence qualifies when some n <= 1024 has every increment start_r - s * delta_r > 0 for s <= n and the
 * increments sum to at least max_range - min_range (the defaults need 466, and 470 to reach 120 m from 0).  The getters before a successful run:
 * SGTD_ERR_STATE; more than capacity: SGTD_ERR_CAPACITY (*n = the size needed, the first `capacity` entries written). */
#define SGTD_SCAN_MAX_CLASSES 32
#define SGTD_SCAN_MAX_SCANS 4096
#define SGTD_SCAN_MAX_POINTS (1 << 28)
#define SGTD_SCAN_MAX_CELLS 1024
typedef struct sgtd_scan_config {
  int32_t node_label[SGTD_SCAN_MAX_CLASSES]; /* semantic label s -> keypoint label; 0: class dropped */
  int32_t min_seg[SGTD_SCAN_MAX_CLASSES];    /* voxel mode: smallest cluster kept (minSeg)            */
  int32_t min_instance_points;               /* instance mode: kept when count > this (20)            */
  int32_t reserved;
  double start_r, delta_r, delta_p, delta_a; /* 0.35, 0.0004, 1.2, 1.2 (get_json.cpp:205-208)         */
  double min_range, max_range;               /* 0.5, 120.0 (cluster_manager.hpp:198)                  */
} sgtd_scan_config;
/* node_label[10..18] = 3..11, else 0 (the net effect of get_json.cpp:10-12,137,288); min_seg[15] = min_seg[17] =
 * min_seg[18] = 5, else 300 (get_json.cpp:164,178-181) */
void sgtd_default_scan_config(sgtd_scan_config *cfg);
/* the config part of sgtd_scan_keypoints' checks, without a handle (host code, no device needed): SGTD_OK,
 * SGTD_ERR_INVALID or SGTD_ERR_UNSUPPORTED; *why (may be NULL) names the reason, a static string */
int sgtd_scan_config_check(const sgtd_scan_config *cfg /* NULL = defaults */, const char **why);
int sgtd_scan_keypoints(sgtd_handle h, const sgtd_scan_config *cfg /* NULL = defaults */, const float *points,
                        int stride_floats /* 3, or 4 = x y z i */, const uint32_t *labels, const int64_t *pt_off /* host, n_scans + 1 */,
                        int n_scans, int device_ptrs);
/* kp_off [n_scans + 1]; xyz [capacity * 3], label, n_points [capacity]; any array may be NULL */
int sgtd_result_scan_keypoints(sgtd_handle h, int64_t *kp_off, float *xyz, uint32_t *label, int32_t *n_points, int64_t capacity,
                               int64_t *n_keypoints);
int sgtd_result_scan_point_clusters(sgtd_handle h, int scan, int32_t *cluster, int64_t capacity, int64_t *n);
int sgtd_result_scan_grids(sgtd_handle h, int scan, int32_t *grid /*[32*4]*/, double *range /*[32*4]*/);
int sgtd_scan_device_view(sgtd_handle h, const float **d_xyz, const uint32_t **d_label);
/* points per tile (workgroup) of the per-point passes: the tests place their edges there */
void sgtd_scan_tiles(int *point_tile);

/* ---- posed, labelled scans to the keypoints of local maps (local_map_kernels.hip.h) ----
 * What the reference's map-side producer local_map does (src/sgtd/src/local_map.cpp:213-482, gen_graphs :767-923, the
 * graph_DCVC_map files the localization node loads as its map): for every anchor scan j the scans whose pose lies within
 * `radius` of j's are moved into j's frame and appended behind j's own points, and the merged cloud is clustered like a
 * single scan.  A local map sees each object from several places: denser clusters, steadier keypoints, more of them.
 *
 * The rule.  All arithmetic is f64, every operation rounded once (no contraction); f32 inputs are widened exactly.  inv()
 * and mul() are those of sgtd_consistent_loops above, in their operation order.
 * Inputs: n_scans labelled scans as sgtd_scan_keypoints takes them; pose12 [n_scans * 12], a host array, f32, row-major
 *   3x4 [R | t]: the pose T_i of the frame scan i's points are given in (the sensor pose; the reference multiplies a fixed
 *   extrinsic in, BASE2OUSTER, :300 — here the caller composes it into the pose beforehand); anchors [n_anchors], a host
 *   array of scan indices (NULL: every scan, in order, n_anchors ignored); repeats are allowed, each entry is a local map
 *   of its own.
 * Members of anchor j: j itself, always, first.  Every other scan i iff d2 <= rr with dx = (double)t_i[0] - (double)t_j[0]
 *   (dy, dz alike), d2 = (dx*dx + dy*dy) + dz*dz, rr = radius * radius, listed in ascending i.  d2 == rr is in (the
 *   reference skips on > 15, :272).  A translation that is not finite makes d2 NaN or infinite: such a scan is a member of
 *   its own local map only.  With max_members = m > 0: the anchor and the m - 1 other members with the smallest (d2, i),
 *   ordered lexicographically (ties in d2 go to the smaller index), still listed in ascending i behind the anchor; m == 1
 *   keeps the anchor alone.
 * Merged cloud of anchor j: j's own points first, x y z as given (:260-264); then, for each other member i in list order,
 *   its points in their order, each p'[r] = (float)(((M[r][0]*x + M[r][1]*y) + M[r][2]*z) + M[r][3]), r = 0..2, with
 *   M = mul(inv(T_j), T_i) (:300-302,320-325).  Labels are carried along unchanged.  A coordinate that is NaN or infinite
 *   (a NaN in a rotation gives such points) is dropped by the scan rule as it is today.
 * Keypoints of anchor j: the rule of sgtd_scan_keypoints, unchanged, on the merged cloud as if it were one scan (classes,
 *   modes, range gate, the grid from the merged cloud's own min / max, components, size filter, order by smallest merged
 *   point index, the fixed-order 256-accumulator centres): xyz f32 in the anchor's frame, label u32, n_points.
 * Departures from the reference: local_map_creation re-opens the anchor's own files for every neighbour
 *   (current_scan_path, :281,305) and so merges copies of the anchor's cloud, not the neighbours' — this call merges the
 *   neighbours' clouds, plainly what was meant; the reference inverts T_j as a general 4x4 in f32 (:300), here it is the
 *   rigid inverse in f64; the distance test runs in f64 on the given (sensor) translations, not in f32 on base
 *   translations; the class rules of :372-442 (the lumped classes 9 / 10, the skipped classes, the per-class minima) are
 *   expressed through sgtd_scan_config's node_label / min_seg; "one cluster for the whole class" is not offered; densitys,
 *   edges and weights of the graph file are not produced (nothing downstream reads them).
 *
 * Passes: a local map of 30 members holds millions of points and the scan pipeline needs about 280 bytes of work space a
 * point, so consecutive anchors go into one pass while the sum of their merged sizes stays within max_pass_points (and
 * their number within SGTD_SCAN_MAX_SCANS); the keypoints of every pass are appended on the device.  No result depends on
 * where the pass boundaries fall.  An anchor whose merged cloud alone exceeds max_pass_points fails the call with
 * SGTD_ERR_UNSUPPORTED before any clustering runs (sgtd_last_error names the anchor and its size); no results are left
 * and the handle stays usable.
 *
 * The results stay on the device in buffers of their own until the next local-map call or sgtd_destroy;
 * sgtd_scan_keypoints does not disturb them.  The call clusters in the scan pipeline's work buffers and so invalidates the
 * results of an earlier sgtd_scan_keypoints (its getters: SGTD_ERR_STATE).  It is independent of the pending batch, the
 * table and the stored poses; a view (sgtd_attach_table) runs it whatever state its owner is in, a multi-device handle on
 * its first device.  sgtd_local_map_device_view: borrowed device pointers (xyz f32 [n_keypoints * 3], label u32), with the
 * fetched kp_off what sgtd_add_frames / sgtd_query_frames take with device_ptrs = 1.  sgtd_result_local_map_members:
 * mem_off [n_anchors + 1], member [capacity] (scan indices, the anchor first), merged_points [n_anchors], the number of
 * passes.  sgtd_local_map_stage_ms: milliseconds of the last call's member selection, gathers and scan passes between
 * events on its stream (zeros unless sgtd_set_timing is on).
 *
 * Errors, before the device is touched, SGTD_ERR_INVALID: everything sgtd_scan_keypoints rejects so; pose12 == NULL with
 * n_scans > 0; n_anchors < 0; an anchor outside [0, n_scans); radius NaN, negative or infinite; max_members < 0;
 * max_pass_points < 0 or above SGTD_SCAN_MAX_POINTS; reserved != 0.  The getters before a successful run: SGTD_ERR_STATE;
 * more than capacity: SGTD_ERR_CAPACITY (the size needed reported, the first `capacity` entries written). */
typedef struct sgtd_local_map_options {
  double  radius;           /* 15.0 (local_map.cpp:272); finite, >= 0 */
  int32_t max_members;      /* 0 = no cap; otherwise >= 1, the anchor included */
  int32_t reserved;         /* 0 */
  int64_t max_pass_points;  /* merged points clustered in one pass; 0 = default (1 << 26); <= SGTD_SCAN_MAX_POINTS */
} sgtd_local_map_options;
void sgtd_default_local_map_options(sgtd_local_map_options *opt);
int sgtd_local_map_keypoints(sgtd_handle h, const sgtd_scan_config *cfg, const sgtd_local_map_options *opt,
                             const float *points, int stride_floats, const uint32_t *labels, const int64_t *pt_off,
                             const float *pose12, int n_scans, const int32_t *anchors, int n_anchors, int device_ptrs);
int sgtd_result_local_map_keypoints(sgtd_handle h, int64_t *kp_off /* n_anchors + 1 */, float *xyz, uint32_t *label,
                                    int32_t *n_points, int64_t capacity, int64_t *n_keypoints);
int sgtd_result_local_map_members(sgtd_handle h, int64_t *mem_off /* n_anchors + 1 */, int32_t *member, int64_t capacity,
                                  int64_t *n_members, int64_t *merged_points /* n_anchors */, int32_t *n_passes);
int sgtd_local_map_device_view(sgtd_handle h, const float **d_xyz, const uint32_t **d_label);
int sgtd_local_map_stage_ms(sgtd_handle h, float *ms_members, float *ms_gather, float *ms_scan);

/* Dense registration of raw clouds on the device: plane-regularised GICP (the node's enable_gicp path,
 * semantic_graph_localization.cpp:651-723; fast_gicp::FastGICP, fast_gicp_impl.hpp / lsq_registration_impl.hpp), the one
 * stage behind sgtd_verify that sees the dense geometry.  n_clouds clouds lie back to back in `points` (stride_floats 3
 * or 4 floats a point, x y z first; cloud c = points pt_off[c] .. pt_off[c + 1]); pair k registers cloud src_cloud[k]
 * onto cloud tgt_cloud[k] from init_pose[k] (rel_pose layout: rot row-major (9), t (3); x = R p + t takes a source point
 * into the target's frame; NULL = the identity).  A cloud is given once and may be the source or the target of any number
 * of pairs; covariances are computed once per cloud that some pair names.
 * The rule.  All arithmetic is f64, every operation (+, -, *, /, sqrt) rounded once, no contraction, nothing else is used;
 * the f32 coordinates are widened exactly.  UNIT, ROT, "M v" and the 6x6 Cholesky with its two substitutions are those of
 * sgtd_relax_poses; mul3(a, b)[r][c] = (a[r][0]*b[0][c] + a[r][1]*b[1][c]) + a[r][2]*b[2][c]; svd3 is sgtd_verify's
 * one-sided Jacobi SVD (singular values descending), unpinned against Eigen's as there.
 *   d2(a, b) = (dx*dx + dy*dy) + dz*dz.  A search keeps the smallest (d2, index), lexicographically; a d2 that is NaN or
 *     +inf is never chosen (a point with a non-finite coordinate has no neighbour and is nobody's; the reference's
 *     kd-trees have no rule for it).
 *   SUM over the source points i of a pair: sgtd_refine_poses' ordered sum: SGTD_REG_SUM_W accumulators start at +0.0,
 *     point i is added to accumulator i mod W in ascending i, an unmatched point is skipped (not added as zero), then
 *     acc[l] = acc[l] + acc[l + s] for l < s, s = W/2, ..., 1.
 *   Covariance of point i of a cloud of n points (fast_gicp_impl.hpp:244-298, PLANE): k' = min(k_neighbors, n); the
 *     neighbours are the (at most) k' points of the cloud with the smallest (d2(p_i, p_j), j), i itself included; mu[a] =
 *     (from +0.0, + p_j[a] in that order) / (double)k'; c[a][b] = (from +0.0, + (p_j[a] - mu[a]) * (p_j[b] - mu[b]) in
 *     that order) / (double)k'; c = U S V^T by svd3; a column b of U with (U[0][b]*V[0][b] + U[1][b]*V[1][b]) +
 *     U[2][b]*V[2][b] < 0 is negated (svd3 completes the columns of U of zero singular values up to sign only: on an
 *     exactly flat neighbourhood C n = plane_eps n needs the normal's two copies to agree); C = mul3(mul3(U, D), V^T)
 *     with D = diag(1, 1, plane_eps), zeros written out.  Departures: ties by index where the reference has FLANN's
 *     order; k' in the divisor where the reference keeps k; svd3 in place of JacobiSVD.
 *   Correspondences at a pose (R, t) (:118-155): x_i = (R p_i) + t, x[r] = ((R[r][0]*p[0] + R[r][1]*p[1]) + R[r][2]*p[2])
 *     + t[r]; j(i) = the target index with the smallest (d2(x_i, w_j), j) and dd_i that d2 (+inf when no target has one);
 *     the match is kept iff dd_i < max_corr_dist * max_corr_dist, else j(i) = -1.  For a kept match S = C_B[j] + G with
 *     RC = mul3(R, C_A[i]), G[r][c] = (RC[r][0]*R[c][0] + RC[r][1]*R[c][1]) + RC[r][2]*R[c][2], and M_i = inverse of S:
 *       a00 = S11*S22 - S12*S21;  a01 = S02*S21 - S01*S22;  a02 = S01*S12 - S02*S11;
 *       a10 = S12*S20 - S10*S22;  a11 = S00*S22 - S02*S20;  a12 = S02*S10 - S00*S12;
 *       a20 = S10*S21 - S11*S20;  a21 = S01*S20 - S00*S21;  a22 = S00*S11 - S01*S10;
 *       det = (S00*a00 + S01*a10) + S02*a20;  M[r][c] = a[r][c] / det.
 *     Departures: the reference transforms and searches in f32, and inverts a 4x4 whose last row is padding.
 *   Linearisation (:158-214): e = w_j - x_i; y = M_i e; cost_i = (e[0]*y[0] + e[1]*y[1]) + e[2]*y[2]; J = [A | -I] with
 *     A = skew(x_i) = ((0, -x2, x1), (x2, 0, -x0), (-x1, x0, 0)), zeros written out; MA = mul3(M_i, A).  Only the lower
 *     triangle of H is formed: for a >= b in 0..2: H[a][b] = SUM of (A[0][a]*MA[0][b] + A[1][a]*MA[1][b]) + A[2][a]*MA[2][b];
 *     H[3+a][b] = SUM of -MA[a][b]; for a >= b: H[3+a][3+b] = SUM of M_i[a][b].  b[a] = SUM of (A[0][a]*y[0] + A[1][a]*y[1])
 *     + A[2][a]*y[2], b[3+a] = SUM of -y[a]; y0 = SUM of cost_i; n = the number of kept matches.  One iteration is counted.
 *     n == 0: the solve ends "no correspondence", the pose is kept.
 *   Step (lsq_registration_impl.hpp:123-168).  On the first linearisation of a pair lambda = lm_init_lambda_factor * m, m
 *     from 0.0 over a = 0..5: v = |H[a][a]|, m = v > m ? v : m.  nu = 2.0.  Up to lm_max_trials trials; when they run out
 *     the solve ends "LM failed", the pose is kept (:69-71).  A trial: (H + lambda I) d = -b by the Cholesky column by
 *     column (only the diagonal gets lambda: s starts from H[c][c] + lambda) and the two substitutions on r = -b.  A pivot
 *     that is not > 0: the trial is rejected with no more work: lambda = nu*lambda, nu = 2.0*nu.  Otherwise
 *     dR = ROT(UNIT((1.0, 0.5*d[0], 0.5*d[1], 0.5*d[2]))), dt = (d[3], d[4], d[5]) (departure: the first-order form of the
 *     reference's se3_exp, which takes sin and cos; the same fixed point); the trial pose R' = mul3(dR, R), t' = (dR t) +
 *     dt; yi = SUM of cost_i at the trial pose with the matches and M_i of the linearisation (:217-240); den = from t_0,
 *     + t_a ascending, t_a = d[a] * (lambda*d[a] - b[a]); rho = (y0 - yi) / den; mr = from 0.0 over dR's entries row-major:
 *     v = |dR[r][c] - I[r][c]|, m = v > m ? v : m; mt the same over |dt[a]|; u = mr / rotation_eps, v = mt / translation_eps;
 *     conv = (v > u ? v : u) < 1.0.  Not (rho >= 0) (a NaN rho too; departure: the reference accepts a NaN): with conv the
 *     iteration ends and the pose is kept; otherwise lambda = nu*lambda, nu = 2.0*nu and the next trial follows.
 *     Otherwise the trial becomes the pose, f = 2.0*rho - 1.0, g = 1.0 - (f*f)*f, lambda = lambda * (g > 1.0/3.0 ? g :
 *     1.0/3.0), and the iteration ends.  An iteration that ends with conv ends the solve "converged"; otherwise
 *     max_iterations counted iterations end it "iteration limit".
 *   Results per pair: the pose; cost = y0 of the first and of the last linearisation (NaN without one); the matches
 *     under the final pose from one more correspondence pass: tgt_index[i] = j(i) or -1 and d2[i] = dd_i; n_matched;
 *     fitness = SUM of dd_i over the kept matches / (double)n_matched, NaN without a match (with max_corr_dist = +inf
 *     pcl's getFitnessScore, in f64); iterations; status.  An empty source or target: "no points", pose = init_pose, no
 *     iteration.  No result of a pair depends on the other pairs of the call, or on how the work is tiled.
 * On the device: covariances a lane per point, the cloud streamed through LDS in tiles of SGTD_REG_TGT_TILE; the search
 * a workgroup per (tile of SGTD_REG_SRC_TILE source points, slice of the target), the slices' minima combined exactly;
 * every SUM one workgroup per pair; one lane per pair takes every decision, the host enqueues SGTD_REG_GROUP rounds
 * (search - match - linearise - trial; a pair in its trials skips the first three) and reads the number of unfinished
 * pairs once per group.  The search is brute force: n_source * n_target distances per pass, so thin raw scans first
 * (sgtd_thin_clouds below).
 * The call is a pure function of its arguments: independent of the pending batch, the table and the stored poses; it
 * uses buffers of its own on the handle's stream; a view runs it whatever state its owner is in; a multi-device handle
 * runs it on its first device.  The results last until the next sgtd_register_clouds call that passes its argument
 * checks, or sgtd_destroy.  device_ptrs != 0: `points` is a device array (everything else is the host's).
 * h == NULL, a negative count, with a positive count: pt_off, points, src_cloud or tgt_cloud NULL; a stride other than 3
 * or 4; pt_off[0] != 0 or decreasing offsets; a cloud index outside [0, n_clouds); a non-finite init_pose; k_neighbors
 * outside 3..32, max_iterations or lm_max_trials < 1, max_corr_dist NaN or <= 0 (+inf is allowed), another option not
 * finite and > 0, reserved != 0: SGTD_ERR_INVALID, before the device is touched and with the earlier results kept.  A
 * cloud of more than SGTD_REG_MAX_POINTS points, more than SGTD_REG_MAX_CLOUDS clouds, SGTD_REG_MAX_TOTAL_POINTS points in
 * all, SGTD_REG_MAX_PAIRS pairs or SGTD_REG_MAX_SOURCE_POINTS source points summed over the pairs: SGTD_ERR_UNSUPPORTED
 * (sgtd_last_error says which), the earlier results kept as well.
 * The getters before a successful run: SGTD_ERR_STATE; a cloud or pair outside the run: SGTD_ERR_INVALID; more than
 * capacity: SGTD_ERR_CAPACITY (*n = the size needed, the first `capacity` entries written).  Any array may be NULL.
 * sgtd_result_register_covariances: row-major 3x3 per point of the cloud; *n = 0 for a cloud no pair names.
 * sgtd_register_stage_ms: covariances, searches, everything else (matches, sums, control) and the whole call on the
 * device, from events on the stream (zeros unless sgtd_set_timing is on; the events serialise the call). */
#define SGTD_REG_SUM_W 256
#define SGTD_REG_SRC_TILE 128
#define SGTD_REG_TGT_TILE 512
#define SGTD_REG_SLICE_TILES 2
#define SGTD_REG_GROUP 4
#define SGTD_REG_MAX_K 32
#define SGTD_REG_MAX_POINTS (1 << 17)
#define SGTD_REG_MAX_CLOUDS (1 << 16)
#define SGTD_REG_MAX_TOTAL_POINTS (1 << 25)
#define SGTD_REG_MAX_PAIRS (1 << 16)
#define SGTD_REG_MAX_SOURCE_POINTS (1 << 24)
enum { SGTD_REG_CONVERGED = 0, SGTD_REG_ITERATION_LIMIT = 1, SGTD_REG_LM_FAILED = 2, SGTD_REG_NO_CORRESPONDENCE = 3, SGTD_REG_NO_POINTS = 4 };
typedef struct sgtd_register_options {
  int32_t k_neighbors;           /* 20 (SG_localization.yaml:24); 3..32 */
  int32_t max_iterations;        /* 64 (lsq_registration_impl.hpp:11; the node sets 10) */
  int32_t lm_max_trials;         /* 10 (:17) */
  int32_t reserved;              /* 0 */
  double max_corr_dist;          /* +inf (fast_gicp's default); > 0, +inf allowed */
  double lm_init_lambda_factor;  /* 1e-9 */
  double rotation_eps;           /* 2e-3 */
  double translation_eps;        /* 5e-4 */
  double plane_eps;              /* 1e-3: the PLANE regularisation's third value */
} sgtd_register_options;
void sgtd_default_register_options(sgtd_register_options *o);
int sgtd_register_clouds(sgtd_handle h, const sgtd_register_options *opt /* NULL = defaults */,
                         const float *points, int stride_floats /* 3 or 4 */, const int64_t *pt_off /* host, n_clouds + 1 */, int n_clouds,
                         const int32_t *src_cloud, const int32_t *tgt_cloud, const double *init_pose /* [n_pairs*12], NULL = identity */,
                         int n_pairs, int device_ptrs /* points only */);
int sgtd_result_registered(sgtd_handle h, double *pose /*[n*12]*/, double *fitness, double *cost /*[n*2] first, last*/,
                           int32_t *n_matched, int32_t *iterations, int32_t *status);
int sgtd_result_register_covariances(sgtd_handle h, int cloud, double *cov /*[cap*9]*/, int64_t capacity, int64_t *n);
int sgtd_result_register_matches(sgtd_handle h, int pair, int32_t *tgt_index, double *d2, int64_t capacity, int64_t *n);
int sgtd_register_stage_ms(sgtd_handle h, float *ms_cov, float *ms_search, float *ms_rest, float *ms_total);
/* the tile sizes above, and the slice length (targets) a call uses unless the SGTD_REG_SLICE_TILES environment hook,
 * read at every call, gives another number of tiles; a call whose slices' minima would pass 2^27 entries doubles the
 * length until they fit (no result depends on it) */
void sgtd_register_tiles(int *src_tile, int *tgt_tile, int *slice);

/* Dense clouds of map frames, keyed by global frame id, kept on the device with their covariances: frame frame_ids[i]
 * gets the points pt_off[i] .. pt_off[i+1] of `points` (stride_floats floats each, x y z first; a host array, or with
 * device_ptrs != 0 a device array; frame_ids and pt_off are the host's).  They are the targets of sgtd_register_stored
 * and sgtd_register_stored_loops.
 * The call behaves like sgtd_set_frame_keypoints: the clouds are copied at the call and are settings of the handle;
 * later calls overwrite; an id repeated within one call: the last one wins; points == NULL with n > 0 forgets the clouds of
 * those ids; frame_ids == NULL with n == 0 forgets all, frees the device memory and forgets k_neighbors and plane_eps;
 * ids may name frames not (yet) added; sgtd_add*, sgtd_remove_frames and sgtd_load_table leave them alone, the table file
 * does not hold them, a view (sgtd_attach_table) has a store of its own, and a multi-device handle keeps the store on its
 * first device, where sgtd_register_clouds runs.  A frame stored with zero points "has a cloud" (count 0).  Non-finite
 * coordinates are stored as given (the covariance rule says what they do).
 * Kept per frame: its points (x, y, z) and each point's covariance by sgtd_register_clouds' covariance rule with this
 * call's k_neighbors (3..32) and plane_eps, computed once, at the call.  The first call on an empty store fixes
 * k_neighbors and plane_eps; a later one with other values: SGTD_ERR_STATE (forget all first).
 * Memory: no host copy; 84 bytes a point on the device (12 of coordinates, 72 of covariance) in one arena, the stored
 * clouds at its front in arrival order; sgtd_register_stored packs its own clouds behind them for the length of the
 * call, so the arena also holds the room a call's clouds needed.  An overwritten or forgotten cloud stays as dead points
 * until they outnumber the live ones or the arena has to grow; then the live clouds are copied, in order, into new
 * arrays.  The arena always grows into new arrays that replace the old ones once they are complete, never by freeing
 * first: a device allocation that fails leaves the store exactly as it was before the call.
 * h == NULL, n < 0, frame_ids == NULL with n > 0, with points != NULL and n > 0: pt_off NULL, a stride other than 3 or 4,
 * pt_off[0] != 0 or decreasing offsets, k_neighbors outside 3..32, plane_eps not finite and > 0: SGTD_ERR_INVALID; an id
 * >= max_frame_n: SGTD_ERR_FRAME_LIMIT; a cloud of more than SGTD_REG_MAX_POINTS points, or more than
 * SGTD_CLOUD_STORE_MAX_POINTS live points in the store after the call: SGTD_ERR_UNSUPPORTED (sgtd_last_error says
 * which).  All before the device is touched and with the store unchanged.
 * sgtd_frame_clouds_info: frames that have a cloud, their points, the bytes of the arena's device arrays, the settings
 * (0 and 0.0 while there are none); any output may be NULL.
 * sgtd_result_frame_cloud: the stored points (3 floats each) and covariances (row-major 3x3) of one frame; *n = its
 * count, or -1 where the frame has no cloud (SGTD_OK); more than capacity: SGTD_ERR_CAPACITY (the first `capacity`
 * points written).  xyz or cov may be NULL. */
#define SGTD_CLOUD_STORE_MAX_POINTS (1 << 27)
int sgtd_set_frame_clouds(sgtd_handle h, const uint32_t *frame_ids, const int64_t *pt_off /* n + 1 */,
                          const float *points, int stride_floats /* 3 or 4 */, int64_t n,
                          int k_neighbors, double plane_eps, int device_ptrs /* points only */);
int sgtd_frame_clouds_info(sgtd_handle h, int64_t *n_frames, int64_t *n_points, int64_t *device_bytes,
                           int32_t *k_neighbors, double *plane_eps);
int sgtd_result_frame_cloud(sgtd_handle h, uint32_t frame, float *xyz /*[cap*3]*/, double *cov /*[cap*9]*/,
                            int64_t capacity, int64_t *n /* -1: the frame has no cloud */);

/* sgtd_register_clouds with the targets read from the cloud store: pair k registers the call's cloud src_cloud[k] onto
 * the stored cloud of frame tgt_frame[k].  The results are those of sgtd_register_clouds on the call's clouds followed
 * by the named frames' stored clouds, with the same options, bit for bit: pose, fitness, cost, n_matched, iterations,
 * status, every match and d2, and the source clouds' covariances (a cloud's covariances depend on that cloud alone, and
 * no result of a pair depends on the other pairs or on the tiling).  Covariances are computed only for the call's clouds
 * that some pair names; no target point crosses the link and no target covariance is computed again.
 * opt->k_neighbors or opt->plane_eps different from the store's: SGTD_ERR_STATE; a target frame without a stored cloud:
 * SGTD_ERR_INVALID (sgtd_last_error names the frame); everything sgtd_register_clouds rejects or caps is rejected or
 * capped the same way, its caps applied to the call's own clouds and pairs.  All before the device is touched and with
 * the earlier results kept.  The call has result buffers of its own: it never touches sgtd_register_clouds' or
 * sgtd_register_voxels' results, and they never touch its; its results last until the next sgtd_register_stored or
 * sgtd_register_stored_loops call that passes its argument checks, or sgtd_destroy (later sgtd_set_frame_clouds calls
 * do not change them).  A view uses its own store; a multi-device handle runs the call on its first device.
 * The getters follow the sgtd_result_register* family: sgtd_result_stored_matches' tgt_index counts within the frame's
 * cloud; sgtd_result_stored_covariances gives the call's clouds'.
 *
 * sgtd_register_stored_loops forms the pairs on the device from the pending batch's verification (after sgtd_verify,
 * sgtd_verify_masked, or sgtd_search_frame with flags 0); cloud q of the call is query q's raw cloud (pt_off: n_queries
 * + 1 offsets).  Per query: the candidates with a verification result (score >= 0) in descending score, ties in
 * ascending candidate index; the first max_per_query of them (clamped to candidate_num); of those, the ones whose frame
 * has no stored cloud are dropped, not replaced by the next candidate.  The rows are in (query, rank) order, init is the
 * relative pose of the stage `start` names (sgtd_result_verify's, sgtd_result_refined's, sgtd_result_aligned's), and the
 * getters above return the results per row; sgtd_result_stored_pairs returns the rows (*n = their count; more than
 * capacity: SGTD_ERR_CAPACITY; after sgtd_register_stored: SGTD_ERR_STATE).  The host reads the rows back once, to size
 * the tiles.  The call adds results and changes none of the batch's.
 * max_per_query < 0, an unknown start and what sgtd_register_stored rejects: SGTD_ERR_INVALID; no verification of the
 * pending batch, or the named stage has not run on it: SGTD_ERR_STATE; a multi-device handle: SGTD_ERR_UNSUPPORTED (its
 * batch results live on several engines: form the pairs and use sgtd_register_stored).  sgtd_register_clouds' caps on
 * the clouds are checked before the device is touched; its caps on the pairs can only be checked once the pairs are
 * formed, and a call that fails there leaves no results. */
int sgtd_register_stored(sgtd_handle h, const sgtd_register_options *opt /* NULL = defaults */,
                         const float *points, int stride_floats, const int64_t *pt_off /* host, n_clouds + 1 */, int n_clouds,
                         const int32_t *src_cloud, const uint32_t *tgt_frame, const double *init_pose /* [n_pairs*12], NULL = identity */,
                         int n_pairs, int device_ptrs /* points only */);
int sgtd_result_stored_registered(sgtd_handle h, double *pose /*[n*12]*/, double *fitness, double *cost /*[n*2] first, last*/,
                                  int32_t *n_matched, int32_t *iterations, int32_t *status);
int sgtd_result_stored_covariances(sgtd_handle h, int cloud, double *cov /*[cap*9]*/, int64_t capacity, int64_t *n);
int sgtd_result_stored_matches(sgtd_handle h, int pair, int32_t *tgt_index, double *d2, int64_t capacity, int64_t *n);
int sgtd_stored_register_stage_ms(sgtd_handle h, float *ms_cov, float *ms_search, float *ms_rest, float *ms_total);
enum { SGTD_START_VERIFY = 0, SGTD_START_REFINED = 1, SGTD_START_ALIGNED = 2 };
int sgtd_register_stored_loops(sgtd_handle h, const sgtd_register_options *opt /* NULL = defaults */,
                               const float *points, int stride_floats, const int64_t *pt_off /* n_queries + 1 */,
                               int max_per_query, int start, int device_ptrs /* points only */);
int sgtd_result_stored_pairs(sgtd_handle h, int32_t *query, int32_t *cand, int32_t *frame, double *init /*[n*12]*/,
                             int64_t capacity, int64_t *n);

/* Voxelised GICP of clouds against voxel maps on the device (fast_gicp::FastVGICP, fast_vgicp_impl.hpp /
 * fast_vgicp_voxel.hpp): the target of a pair is a map of Gaussian voxels accumulated from any number of posed clouds,
 * and a source point is matched by looking up the voxel it lands in (and its 6 or 26 neighbours), so an iteration's cost
 * does not depend on the target's size.  The clouds are given as for sgtd_register_clouds.  Map m has the members
 * map_off[m] .. map_off[m + 1] of map_cloud (cloud indices) and map_pose (12 doubles per member, rel_pose layout:
 * x = R p + t takes the member's points into the map's frame; NULL = the identity for every member, which goes through
 * the same arithmetic as one written out).  Pair k registers cloud src_cloud[k] onto map tgt_map[k] from init_pose[k]
 * (NULL = the identity).  A cloud may be a member of several maps, several times of one, and the source of pairs;
 * covariances are computed once per cloud that is a source or a member, by sgtd_register_clouds' covariance rule.
 * The rule builds on sgtd_register_clouds': all arithmetic is f64, every operation (+, -, *, /, sqrt) rounded once, no
 * contraction; floor is the one addition and is exact.  mul3, svd3, UNIT, ROT, the Cholesky, SUM (SGTD_REG_SUM_W
 * accumulators), d2 and the covariance rule are the ones stated there.
 *   A member point in its map: x = (R p) + t as x_i there; Cx[r][c] = (RC[r][0]*R[c][0] + RC[r][1]*R[c][1]) + RC[r][2]*R[c][2]
 *     with RC = mul3(R, C), C the point's covariance in its cloud; q[a] = floor(x[a] / voxel_resolution - 0.5)
 *     (fast_vgicp_voxel.hpp:159).  The point enters the map iff x[0], x[1], x[2] are finite and every q[a] lies in
 *     [-2^15, 2^15); otherwise it belongs to no voxel (departure: the reference casts to int unchecked).  Its voxel has the
 *     key map << 48 | (q0 + 2^15) << 32 | (q1 + 2^15) << 16 | (q2 + 2^15); the voxels of a map are numbered from 0 in
 *     ascending key.
 *   A voxel (ADDITIVE, :105-122) of n points: mean[a] = VSUM(x[a]) / (double)n, cov[r][c] = VSUM(Cx[r][c]) / (double)n, all
 *     nine entries.  VSUM: the voxel's points are ordered by member position within the map (map_off order), then by point
 *     index within the member; SGTD_VREG_SUM_W accumulators start at +0.0, the r-th point (r from 0) is added to accumulator
 *     r mod SGTD_VREG_SUM_W in ascending r, then acc[l] = acc[l] + acc[l + s] for l < s, s = SGTD_VREG_SUM_W / 2, ..., 1.
 *   Correspondences at a pose (R, t) (fast_vgicp_impl.hpp:73-116): x_i = (R p_i) + t and q from x_i as above; an x_i that
 *     is not finite or whose q is out of range has none.  For every offset o of neighbor_mode, in this order, the voxel
 *     with the coordinates q + o of the pair's map is a correspondence if it exists (a q + o outside [-2^15, 2^15) names no
 *     voxel).  Mode 1: (0,0,0).  Mode 7: (0,0,0), (1,0,0), (-1,0,0), (0,1,0), (0,-1,0), (0,0,1), (0,0,-1)
 *     (fast_vgicp_voxel.hpp:21-29).  Mode 27: (i-1, j-1, k-1) for i, j, k in 0..2, i outermost (:35-42).  For a
 *     correspondence with voxel v: S = cov_v + G_i, G_i as G in sgtd_register_clouds' rule from C_A[i] and R; M = the inverse
 *     of S by the cofactor form there; w = sqrt((double)n_v); Mw[r][c] = w * M[r][c].
 *   Linearisation: per correspondence e = mean_v - x_i and everything as in sgtd_register_clouds' rule with Mw in place
 *     of M_i: y = Mw e, cost = (e[0]*y[0] + e[1]*y[1]) + e[2]*y[2], MA = mul3(Mw, A), the 21 + 6 terms of H and b.  The term
 *     of a point is the sum of its correspondences' terms in offset order, starting from +0.0; SUM runs over the points,
 *     a point without a correspondence is skipped.  n = the number of correspondences; n == 0 ends the solve "no
 *     correspondence".  The trial cost yi is SUM over the points of (from +0.0, + cost of each correspondence in offset
 *     order) at the trial pose with the correspondences and Mw of the linearisation.  lambda, nu, the trials, rho, the
 *     convergence test, the iteration count and the statuses are sgtd_register_clouds'.  There is no max_corr_dist: the
 *     voxel neighbourhood is the gate.
 *   Results per pair: the pose; cost = y0 of the first and of the last linearisation (NaN without one); iterations;
 *     status; and from one more correspondence pass at the final pose: voxel[i * mode + o] = the index within the map of
 *     the voxel at q + o, or -1; n_corr = the number of correspondences; n_matched = the number of source points with at
 *     least one; fitness = SUM over those points of m_i / (double)n_matched, m_i = from +inf over the point's
 *     correspondences in offset order: dd = d2(x_i, mean_v), m = dd < m ? dd : m; NaN without a matched point.  A pair whose
 *     source is empty or whose map has no voxel: "no points", pose = init_pose, no iteration.  No result of a pair depends
 *     on the other pairs or maps of the call, or on how the work is tiled.
 * Departures from fast_gicp: those of sgtd_register_clouds (covariances, the first-order step, the rejected NaN rho, the
 * 3x3 inverse); the range check of q; f64 transforms of f32 points where the reference's voxel map is built from the f32
 * cloud; the fixed summation orders where the reference sums per OpenMP thread; one voxel numbering per map in key order
 * where the reference keeps a hash map; member poses and several members per map where the reference has one target
 * cloud; only the ADDITIVE mode (MULTIPLICATIVE and ADDITIVE_WEIGHTED are not offered); the fitness is taken against the
 * voxel means where the node's getFitnessScore searches the raw target cloud.
 * On the device: keys a lane per member point, the stable radix sort, voxel heads and per-map voxel ranges, a wave per
 * voxel for VSUM; per round a lane per source point looks its voxels up by binary search in the map's sorted keys and
 * writes the voxel ids and Mw to per-correspondence streams; the sums a workgroup per pair; one lane per pair decides, the
 * host enqueues SGTD_REG_GROUP rounds and reads the number of unfinished pairs once per group.
 * The call is a pure function of its arguments like sgtd_register_clouds: buffers of its own on the handle's stream,
 * usable on a view, on the first device of a multi-device handle; its results last until the next sgtd_register_voxels
 * call that passes its argument checks, or sgtd_destroy, and are independent of sgtd_register_clouds' (neither call
 * disturbs the other's results).  device_ptrs != 0: `points` is a device array (everything else is the host's).
 * SGTD_ERR_INVALID, before the device is touched and with the earlier results kept: everything sgtd_register_clouds
 * rejects of the clouds, pairs, init_pose and the shared options; n_maps < 0; with a positive count: map_off, map_cloud or
 * tgt_map NULL; map_off[0] != 0 or decreasing map_off; a member cloud outside [0, n_clouds); a pair's map outside
 * [0, n_maps); a non-finite map_pose; a voxel_resolution that is not finite and > 0; a neighbor_mode other than 1, 7, 27.
 * SGTD_ERR_UNSUPPORTED (sgtd_last_error says which), the earlier results kept as well: sgtd_register_clouds' caps on a
 * cloud, the clouds, all points and the pairs; more than SGTD_VREG_MAX_MAPS maps; more than SGTD_VREG_MAX_MEMBER_POINTS
 * member points summed over the maps; more than SGTD_VREG_MAX_CORR for the source points summed over the pairs times
 * neighbor_mode (the per-correspondence streams hold 76 bytes each).
 * The getters before a successful run: SGTD_ERR_STATE; a map or pair outside the run: SGTD_ERR_INVALID; more than
 * capacity: SGTD_ERR_CAPACITY (*n = the size needed, the first `capacity` entries written).  Any array may be NULL.
 * sgtd_result_voxel_map: the voxels of one map in their numbering: coord = q, n_points, mean, cov row-major.
 * sgtd_result_voxel_matches: voxel[i * mode + o] of one pair under its final pose.
 * sgtd_voxel_register_stage_ms: covariances, map build, correspondence passes, everything else and the whole call on
 * the device (zeros unless sgtd_set_timing is on; the events serialise the call). */
#define SGTD_VREG_SUM_W 64
#define SGTD_VREG_MAX_MAPS 65535
#define SGTD_VREG_MAX_MEMBER_POINTS (1 << 25)
#define SGTD_VREG_MAX_CORR (1 << 26)
typedef struct sgtd_voxel_register_options {
  double voxel_resolution;       /* 1.0 (fast_vgicp_impl.hpp:22); finite and > 0 */
  int32_t neighbor_mode;         /* 1 (DIRECT1, :23); 1, 7 or 27 */
  int32_t k_neighbors;           /* the rest: as in sgtd_register_options, the same defaults and ranges */
  int32_t max_iterations;
  int32_t lm_max_trials;
  double lm_init_lambda_factor;
  double rotation_eps;
  double translation_eps;
  double plane_eps;
  int64_t reserved;              /* 0 */
} sgtd_voxel_register_options;
void sgtd_default_voxel_register_options(sgtd_voxel_register_options *o);
int sgtd_register_voxels(sgtd_handle h, const sgtd_voxel_register_options *opt /* NULL = defaults */,
                         const float *points, int stride_floats /* 3 or 4 */, const int64_t *pt_off /* host, n_clouds + 1 */, int n_clouds,
                         const int32_t *map_off /* n_maps + 1 */, const int32_t *map_cloud, const double *map_pose /* [members*12], NULL = identity */,
                         int n_maps, const int32_t *src_cloud, const int32_t *tgt_map, const double *init_pose /* [n_pairs*12], NULL = identity */,
                         int n_pairs, int device_ptrs /* points only */);
int sgtd_result_voxel_registered(sgtd_handle h, double *pose /*[n*12]*/, double *fitness, double *cost /*[n*2] first, last*/,
                                 int32_t *n_matched, int32_t *n_corr, int32_t *iterations, int32_t *status);
int sgtd_result_voxel_map(sgtd_handle h, int map, int32_t *coord /*[cap*3]*/, int32_t *n_points, double *mean /*[cap*3]*/, double *cov /*[cap*9]*/,
                          int64_t capacity, int64_t *n);
int sgtd_result_voxel_matches(sgtd_handle h, int pair, int32_t *voxel /*[n_src*mode]*/, int64_t capacity, int64_t *n);
int sgtd_voxel_register_stage_ms(sgtd_handle h, float *ms_cov, float *ms_map, float *ms_corr, float *ms_rest, float *ms_total);

/* Voxelised GICP of the call's clouds against voxel maps whose members are stored clouds (sgtd_set_frame_clouds).
 * The call's clouds are the sources; map m has the members map_off[m] .. map_off[m + 1] of map_frame, global frame ids
 * that name stored clouds (a frame may be a member of several maps and several times of one); map_pose, src_cloud,
 * tgt_map, init_pose and the options are sgtd_register_voxels'.
 * The results are those of sgtd_register_voxels on [the call's clouds] followed by [the named frames' stored clouds]
 * (member j of map_frame being cloud n_clouds + j there), with the same options, bit for bit: every result row, every
 * voxel of every map, every match.  No member point crosses the link and no member covariance is computed again: the
 * call packs its clouds behind the arena's slots for its length, computes the covariances of its clouds that some pair
 * names, and runs sgtd_register_voxels' kernels over the arena, the members' points and covariances read in place.
 * Every call builds its maps anew.
 * Buffers and results of its own, as sgtd_register_stored has: it neither touches the results of sgtd_register_clouds,
 * sgtd_register_voxels and sgtd_register_stored nor is touched by them; its results last until the next
 * sgtd_register_stored_voxels call that passes its argument checks, or sgtd_destroy (later sgtd_set_frame_clouds calls
 * do not change them).  A view uses its own store; a multi-device handle runs the call on its first device.
 * Before the device is touched and with the earlier results kept: everything sgtd_register_voxels rejects or caps, its
 * caps applied to the call's clouds, the pairs, the maps and the member points (SGTD_ERR_INVALID, SGTD_ERR_UNSUPPORTED);
 * a member frame without a stored cloud: SGTD_ERR_INVALID (sgtd_last_error names the frame); opt's k_neighbors or
 * plane_eps other than the store's: SGTD_ERR_STATE.
 * The getters mirror sgtd_register_voxels', with the same SGTD_ERR_STATE, SGTD_ERR_INVALID and SGTD_ERR_CAPACITY
 * conditions; sgtd_stored_voxel_register_stage_ms' covariance time is that of the call's clouds alone. */
int sgtd_register_stored_voxels(sgtd_handle h, const sgtd_voxel_register_options *opt /* NULL = defaults */,
                                const float *points, int stride_floats /* 3 or 4 */, const int64_t *pt_off /* host, n_clouds + 1 */, int n_clouds,
                                const int32_t *map_off /* n_maps + 1 */, const uint32_t *map_frame, const double *map_pose /* [members*12], NULL = identity */,
                                int n_maps, const int32_t *src_cloud, const int32_t *tgt_map, const double *init_pose /* [n_pairs*12], NULL = identity */,
                                int n_pairs, int device_ptrs /* points only */);
int sgtd_result_stored_voxel_registered(sgtd_handle h, double *pose /*[n*12]*/, double *fitness, double *cost /*[n*2] first, last*/,
                                        int32_t *n_matched, int32_t *n_corr, int32_t *iterations, int32_t *status);
int sgtd_result_stored_voxel_map(sgtd_handle h, int map, int32_t *coord /*[cap*3]*/, int32_t *n_points, double *mean /*[cap*3]*/,
                                 double *cov /*[cap*9]*/, int64_t capacity, int64_t *n);
int sgtd_result_stored_voxel_matches(sgtd_handle h, int pair, int32_t *voxel /*[n_src*mode]*/, int64_t capacity, int64_t *n);
int sgtd_stored_voxel_register_stage_ms(sgtd_handle h, float *ms_cov, float *ms_map, float *ms_corr, float *ms_rest, float *ms_total);

/* sgtd_register_stored_local_loops: the pairs of the pending batch's verification, the local voxel maps around their
 * candidate frames and the members' relative poses, all formed on the device from the verification's results, the cloud
 * store and the poses of sgtd_set_frame_poses, then registered as sgtd_register_stored_voxels does.  Cloud q of the call
 * is query q's raw cloud (pt_off: n_queries + 1 offsets).  All arithmetic below is f64, every operation rounded once (no
 * contraction), on the stored f32 poses widened exactly; inv() and mul() are those of sgtd_consistent_loops above.
 * Eligible frame: it has a stored cloud (sgtd_set_frame_clouds; one of zero points counts) and a stored pose, and all 12
 *   floats of the pose are finite.
 * Rows: sgtd_register_stored_loops' rule.  Per query the candidates with a verification result (score >= 0) in descending
 *   score, ties in ascending candidate index; the first max_per_query of them (clamped to candidate_num); of those, the
 *   ones whose frame is not eligible are dropped, not replaced.  The rows are in (query, rank) order; init is the relative
 *   pose of the stage `start` names (SGTD_START_*).
 * Maps: one per distinct frame among the rows, numbered in ascending frame id and shared among the queries; a row's
 *   tgt_map names the map of its frame.
 * Members of the map of frame j: sgtd_local_map_keypoints' member rule over the eligible frames.  j itself, always,
 *   first.  Every other eligible frame i iff d2 <= rr with dx = (double)t_i[0] - (double)t_j[0] (dy, dz alike),
 *   d2 = (dx*dx + dy*dy) + dz*dz, rr = radius * radius, listed in ascending frame id; d2 == rr is in.  With
 *   max_members = m > 0: j and the m - 1 other members with the smallest (d2, id), ordered lexicographically (ties in d2
 *   go to the smaller id), still listed in ascending id behind j; m == 1 keeps j alone.  This is not
 *   STDescManager.voxel_map_members' cut, which keeps the first m in id order; with max_members = 0 the two agree on
 *   membership.
 * Member poses, in the rel_pose layout: the identity, written out (1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0), for j;
 *   mul(inv(T_j), T_i) for every other member i.
 * Results: those of sgtd_register_stored_voxels on these maps (map_frame = the members, map_pose = the member poses) and
 *   rows (src_cloud = query, tgt_map, init_pose = init), bit for bit, through sgtd_register_stored_voxels' getters;
 *   sgtd_result_stored_local_pairs returns the rows, sgtd_result_stored_local_maps the maps' frames, member offsets
 *   (n_maps + 1), member ids and member poses (*n = the counts; more than a capacity: SGTD_ERR_CAPACITY with the first
 *   entries written; after sgtd_register_stored_voxels: SGTD_ERR_STATE).
 * On the device: a lane per frame id for eligibility, a wave per query for the rows, flags over the frame ids and a scan
 *   for the maps, a workgroup per map that streams every id's translation (counts first, lists second; ascending id by
 *   prefix sums; the max_members cut by a radix select over (bits of d2, id)), a lane per member for the poses.  The pose
 *   store's device copy is the one sgtd_consistent_loops and sgtd_pose_consensus use.  The host reads back the rows, the
 *   maps' frames and the member counts and points once, to size the tiles and check the caps; the members, their poses
 *   and the start poses stay on the device.  The call adds results and changes none of the batch's.
 * max_per_query < 0, an unknown start, a radius that is NaN, negative or infinite, max_members < 0 and the options
 * sgtd_register_voxels rejects: SGTD_ERR_INVALID; k_neighbors or plane_eps other than the store's, no verification of the
 * pending batch, or the named stage has not run on it: SGTD_ERR_STATE; a multi-device handle: SGTD_ERR_UNSUPPORTED.
 * sgtd_register_clouds' caps on the clouds are checked before the device is touched; the caps on the pairs, the maps,
 * the member points (and as many members) and the correspondences can only be checked once rows and maps are formed: a
 * call that fails there returns SGTD_ERR_UNSUPPORTED and leaves no results. */
int sgtd_register_stored_local_loops(sgtd_handle h, const sgtd_voxel_register_options *opt /* NULL = defaults */,
                                     const float *points, int stride_floats, const int64_t *pt_off /* n_queries + 1 */,
                                     int max_per_query, int start, double radius, int max_members /* 0 = no cap */, int device_ptrs /* points only */);
int sgtd_result_stored_local_pairs(sgtd_handle h, int32_t *query, int32_t *cand, int32_t *frame, int32_t *tgt_map, double *init /*[n*12]*/,
                                   int64_t capacity, int64_t *n);
int sgtd_result_stored_local_maps(sgtd_handle h, uint32_t *map_frame, int64_t *mem_off /* n_maps + 1 */, uint32_t *member,
                                  double *member_pose /*[members*12]*/, int64_t cap_maps, int64_t cap_members, int64_t *n_maps, int64_t *n_members);

/* ---- voxel-grid thinning of raw clouds (thin_kernels.hip.h) ----
 * What the node does to a scan with pcl's ApproximateVoxelGrid before GICP (semantic_graph_localization.cpp:357-358, 660),
 * in the form of ingest.voxel_downsample, for a batch of clouds on the device.  The registration calls search by brute
 * force: thin raw scans with this call first.  sgtd_thin_clouds is a pure function of its arguments.
 *
 * Input: n_clouds clouds back to back in points, stride_floats (3 or 4) floats a point, x y z first; with 4 the fourth
 *   column is averaged like the others.  pt_off (n_clouds + 1 offsets, in points) is a host array; points is a host
 *   array, or a device array with device_ptrs != 0 (not the view of an earlier call on the same handle: the call writes
 *   there).  leaf: one per call, f64, finite and > 0.
 * Per point: dropped when x, y or z is not finite.  Else its cell is c[a] = floor((double)p[a] / leaf) per axis: one f64
 *   division, rounded once, then floor (-0.0 lies in cell 0).  A finite point with some c[a] outside
 *   [-SGTD_THIN_MAX_CELL, SGTD_THIN_MAX_CELL) is dropped too (a departure: ingest.voxel_downsample has no such bound;
 *   the two agree wherever no point is out of range).  Both kinds of drop are counted per cloud.
 * Per occupied cell of a cloud: one output point.  Column a = (float)(s_a / (double)count), where s_a starts at +0.0 and
 *   adds (double)p_i[a] over the cell's points in ascending point index: ONE sequential f64 sum, every addition rounded
 *   once — what np.bincount(weights=) does, and so ingest.voxel_downsample's bits — not the 256-accumulator SUM of the
 *   other stages.  A cell may hold a whole cloud: one lane walks it, which gives the same bits and is slow (the
 *   additions of one cell are never spread over lanes: that would be a tree).
 * Order: a cloud's cells in ascending order of their smallest point index; the clouds in order, cloud s at
 *   out_off[s] .. out_off[s + 1].  Cells of different clouds never merge, and no result of a cloud depends on the other
 *   clouds of the call or on how the work is tiled.
 * On the device: a key per point (cloud; cx, cy, cz offset to unsigned 21 bits each), two stable radix sorts (the 63
 *   cell bits, then the cloud; dropped points last), head flags and scans for the cells, a lane per cell for the sums.
 *   No floating-point atomic; the one integer atomic adds the drop counts.  The host reads the output size back once.
 *
 * The call uses buffers of its own on the handle's stream; a view (sgtd_attach_table) runs it whatever state its owner
 * is in; a multi-device handle runs it on its first device.  Results last until the next sgtd_thin_clouds call that
 * passes its checks, or sgtd_destroy.  n_clouds == 0 is a valid run with empty results.  sgtd_thinned_device_view hands
 * out the borrowed device pointer of the output (f32 [n_points * stride_floats]): with the host's out_off it is what
 * sgtd_set_frame_clouds, sgtd_register_clouds, sgtd_register_stored, sgtd_register_stored_loops, sgtd_register_voxels,
 * sgtd_register_stored_voxels and sgtd_register_stored_local_loops take with device_ptrs = 1, and it stays valid across
 * those calls: none of them touches the thin buffers.  A thinned cloud may hold more than SGTD_REG_MAX_POINTS points;
 * the registration call that receives it rejects it.  sgtd_thin_stage_ms: device milliseconds of the last call's two
 * sorts, of the rest, of the whole call (zeros unless sgtd_set_timing).
 *
 * Errors, before the device is touched and with the earlier results kept: h == NULL, a negative count, a NULL array with
 * a positive count, stride_floats neither 3 nor 4, pt_off[0] != 0 or offsets that decrease, leaf NaN, infinite or <= 0:
 * SGTD_ERR_INVALID.  More than SGTD_REG_MAX_CLOUDS clouds or SGTD_SCAN_MAX_POINTS points in all: SGTD_ERR_UNSUPPORTED.
 * The getters before a successful run: SGTD_ERR_STATE; more than capacity: SGTD_ERR_CAPACITY (*n = the size needed, the
 * first `capacity` points written).  Any output may be NULL. */
#define SGTD_THIN_MAX_CELL (1 << 20)   /* +-10 km at a 1 cm leaf */
int sgtd_thin_clouds(sgtd_handle h, const float *points, int stride_floats, const int64_t *pt_off, int n_clouds,
                     double leaf, int device_ptrs);
int sgtd_result_thinned(sgtd_handle h, int64_t *out_off /* n_clouds + 1 */, float *points /* [cap*stride] */,
                        int32_t *n_dropped /* [n_clouds*2]: non-finite, out of range */, int64_t capacity, int64_t *n);
int sgtd_thinned_device_view(sgtd_handle h, const float **d_points, int *stride_floats, int64_t *n_points);
int sgtd_thin_stage_ms(sgtd_handle h, float *ms_sort, float *ms_rest, float *ms_total);

/* Page-locked host memory for the destination buffers of the fetch calls (sgtd_fetch_entries,
 * sgtd_result_pairs, ...): a copy into it is one direct DMA transfer — pageable memory goes through the
 * runtime's staging at about a third of the rate.  Allocation is slow (milliseconds): keep the buffers
 * across calls, as adapter/STDesc_shim.hpp does.  bytes == 0 yields *out = NULL. */
int sgtd_host_alloc(size_t bytes, void **out);
int sgtd_host_free(void *p);

/* table entries by insertion index (to rebuild pair<STDesc,STDesc>) */
int sgtd_fetch_entries(sgtd_handle h, const int64_t *db_entry, int64_t n,
                       sgtd_desc_soa *out);

/* table layout for inspection: keys [U*4] = x,y,z,label code ascending by
 * (code,x,y,z); bucket_off [U+1]; entry ids [E] in bucket order */
int sgtd_table_dump(sgtd_handle h, int64_t *keys, int64_t *bucket_off,
                    int64_t *entry_ids, int64_t cap_buckets, int64_t cap_entries);

/* Largest number of query frames of n_keypoints keypoints each that one sgtd_query_frames call
 * should carry: the rough matches of a batch are indexed with 32 bits (more returns
 * SGTD_ERR_CAPACITY) and their records must fit the device memory that is free now.  Uses the
 * matches per query of the last batch when there is one, else an estimate from the table's
 * bucket statistics; conservative by a factor of about two. */
int sgtd_max_batch(sgtd_handle h, int n_keypoints, int64_t *max_queries);

/* waits for the stream, re-runs the last batch with larger work buffers if it
 * overflowed them, and fills the counters */
int sgtd_sync(sgtd_handle h);
int sgtd_get_stats(sgtd_handle h, sgtd_stats *out);

#ifdef __cplusplus
}
#endif
#endif
