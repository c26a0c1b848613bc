// sgtd_accel.hip — C ABI (include/sgtd_accel.h) over the gfx950 kernels.
// Host side: buffer ownership, launch order, result marshalling.  No CPU
// compute path exists here: every entry point needs the HIP device.
#include "../../include/sgtd_accel.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <unordered_set>
#include <vector>

#include "build_kernel.hip.h"
#include "common.hip.h"
#include "table_kernels.hip.h"
#include "probe_kernels.hip.h"
#include "order_kernels.hip.h"
#include "select_kernels.hip.h"
#include "verify_kernels.hip.h"
#include "verify_mfma.hip.h"
#include "exchange_kernels.hip.h"
#include "remove_kernels.hip.h"
#include "filter_kernels.hip.h"
#include "prior_kernels.hip.h"
#include "refine_kernels.hip.h"
#include "overlap_kernels.hip.h"
#include "align_kernels.hip.h"
#include "consistency_kernels.hip.h"
#include "relax_kernels.hip.h"
#include "register_kernels.hip.h"
#include "voxel_register_kernels.hip.h"
#include "cloud_store_kernels.hip.h"
#include "stored_local_kernels.hip.h"
#include "consensus_kernels.hip.h"
#include "scan_kernels.hip.h"
#include "local_map_kernels.hip.h"
#include "thin_kernels.hip.h"
#include "graph_ingest.hip.h"
#include "table_file.h"

namespace {

// A device array and its owner: freed with whatever holds it (the handle's device is current whenever one goes: sgtd_destroy
// selects it, every other place is inside a call that did).  Move-only; the moved-from buffer is empty.
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  bool borrowed = false;     // the memory belongs to another handle (sgtd_attach_table): never freed or regrown here
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes), borrowed(o.borrowed) { o.p = nullptr; o.bytes = 0; o.borrowed = false; }
  DevBuf &operator=(DevBuf &&o) noexcept {      // (this buffer's own memory goes; hipFree waits for the kernels that use it)
    if (this != &o) {
      if (p && !borrowed) (void)hipFree(p);
      p = o.p; bytes = o.bytes; borrowed = o.borrowed;
      o.p = nullptr; o.bytes = 0; o.borrowed = false;
    }
    return *this;
  }
  ~DevBuf() { if (p && !borrowed) (void)hipFree(p); }
  // the other handle's array in place of this buffer's own
  void borrow_from(const DevBuf &src) {
    *this = DevBuf();
    p = src.p; bytes = src.bytes; borrowed = true;
  }
  template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// A device array of T.  need() (below) is where one is sized: in elements, so the size and the pointer's type cannot disagree.
template <class T>
struct DevArr {
  DevBuf buf;
  T *p() const { return buf.as<T>(); }
};

struct DescStore {
  DevBuf side, angle, center, vertex, label, frame, node_id, qrec;
  size_t cap = 0;
  bool with_thr2 = false;   // query descriptors carry their squared match threshold
  DescArrays view() const {
    DescArrays a;
    a.side = side.as<double>(); a.angle = angle.as<double>(); a.center = center.as<double>();
    a.vertex = vertex.as<float>(); a.label = label.as<int>(); a.frame = frame.as<u32>();
    a.node_id = node_id.as<int>();
    a.qrec = with_thr2 ? qrec.as<QueryRec>() : nullptr;
    return a;
  }
};

// sgtd_set_frame_filter's rows as the caller gave them: bit f - lo of row r (word (f - lo) >> 6) set = frame f allowed
// to query r (every query when n_rows == 1); the bits beyond n of a row's last word are cleared
struct FrameFilter {
  u32 lo = 0, n = 0;
  int n_rows = 0;
  size_t words = 0;          // per row
  std::vector<u64> rows;
  u64 serial = 0;            // distinct for every filter a process makes
  const u64 *row(int r) const { return rows.data() + (size_t)(n_rows == 1 ? 0 : r) * words; }
};

// sgtd_set_position_prior's rows: (cx, cy, cz, r*r) per row in f64 (cz = 0 for dims 2); one for every query when
// n_rows == 1
struct PositionPrior {
  int n_rows = 0, dims = 2;
  std::vector<double4> prm;
  u64 serial = 0;            // distinct for every prior a process makes
};

// bits s .. s + 63 of a bit row of `words` 64-bit words (bit i: word i >> 6, bit i & 63); bits outside the row read 0
static u64 row_bits_at(const u64 *row, size_t words, long long s) {
  const long long w = s >= 0 ? s / 64 : -((-s + 63) / 64);
  const int sh = (int)(s - w * 64);
  auto word = [&](long long i) -> u64 { return i >= 0 && i < (long long)words ? row[i] : 0ull; };
  return sh == 0 ? word(w) : (word(w) >> sh) | (word(w + 1) << (64 - sh));
}

// A host array in page-locked memory (grow-only): the per-batch result tables land here by direct DMA — a copy into
// pageable memory goes through the runtime's staging at about a third of the rate (and ~150 us each on this runtime).
template <class T>
struct PinnedVec {
  T *p = nullptr;
  size_t n = 0, cap = 0;
  PinnedVec() = default;
  PinnedVec(const PinnedVec &) = delete;
  PinnedVec &operator=(const PinnedVec &) = delete;
  ~PinnedVec() { if (p) (void)hipHostFree(p); }
  bool resize(size_t want) {
    if (want > cap) {
      void *np = nullptr;
      const size_t c = std::max<size_t>(want + want / 4, 64);
      if (hipHostMalloc(&np, c * sizeof(T), hipHostMallocDefault) != hipSuccess) return false;
      if (p) (void)hipHostFree(p);      // (contents are not kept: every user refills after a resize)
      p = static_cast<T *>(np);
      cap = c;
    }
    n = want;
    return true;
  }
  T *data() { return p; }
  const T *data() const { return p; }
  T &operator[](size_t i) { return p[i]; }
  const T &operator[](size_t i) const { return p[i]; }
  size_t size() const { return n; }
};

constexpr size_t kCtrWords = CTR_XCD_HEADS + 8 * 1024;   // ProbeBuffers::ctr: counters + the sweep's ticket-queue heads
enum { EV_START = 0, EV_BUILD, EV_SORT, EV_PROBE, EV_VOTES, EV_TOPK, EV_COUNT_T, EV_SCAN, EV_WRITE, EV_COUNT };

// Every decision of a batch's query pipeline, made once when the batch is enqueued (plan_select) and kept in the handle:
// the stages of launch_select and whatever runs on the batch later (a re-run of the list pass, sgtd_finish_lists,
// sgtd_result_rough, sync_batch) read the same form and geometry.
struct SelectPlan {
  int nq = 0, cn = 0; long long n_slots = 0; u32 span = 1, frame_lo = 0, id_bits = 13;                  // batch shape
  // block geometry: descriptors per block of the block passes over the match records, blocks per query, groups of four blocks,
  // the block passes' grid (workgroup b serves query (b/8/groups)*8 + b%8)
  u32 chunk = SGTD_PROBE_CHUNK; int blocks = 0, groups = 0, agrid = 0;
  u32 tile_span = 1, n_tiles = 1; size_t hist_bytes = 0; bool lds_votes = false;                        // vote tiling
  bool votes_fit = false, table_fits = false, per_query = false, fused_pairs = false, fused_votes = false, votes_per_query = false;   // form of the record passes
  int cbits = 1, sub_bits = 0, key_bits = 0; bool small = false, pair = false; size_t max_pass_slots = 0;   // ordering
  bool order_fused = false; u32 order_tiles = 0, order_gtiles = 0;      // ... by order_kernels.hip.h's chain (32-bit keys, not `small`), its tiles
  int row_slots = 1; u32 ticket = 2; int sgrid = 0, pgrid = 0; bool narrow = false, frames = false;     // reservations and the sweep's shape
  bool narrow_pairs = false;      // list form: 4-byte words of the compact lists where an entry's rank among its frame's fits 19 bits, else 8
};

// What a stage measures of a call under sgtd_set_timing: milliseconds per kind of work, between events on the call's
// stream.  The events are made by the stage's first timed call and live as long as the handle.
struct LapClock {
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  LapClock() = default;
  LapClock(const LapClock &) = delete;
  LapClock &operator=(const LapClock &) = delete;
  ~LapClock() { destroy(); }
  int start(sgtd_engine *e, bool timed);                       // a call begins: no milliseconds yet, the events exist if it is timed
  int lap(sgtd_engine *e, int kind);                           // ms[kind] += the work since ev[0] (waited for); ev[0] is recorded anew
  int span(sgtd_engine *e, int a, int b, int kind, bool wait); // ms[kind] += the time from ev[a] to ev[b], recorded both (wait: ev[b] is waited for)
  void destroy();
};

}  // namespace

namespace multi { struct Group; }

struct sgtd_engine {
  multi::Group *grp = nullptr;   // set: this handle is a group of per-device engines (multi.hip.h)
  sgtd_config cfg;
  DevCfg dc;
  hipStream_t stream = nullptr;
  std::string err;
  int n_cus = 256;
  bool timing = false;
  hipEvent_t ev[EV_COUNT] = {};

  // ---- a handle may borrow the finalized table of another handle on the same device (sgtd_attach_table): its own
  // work buffers, results and stream, the owner's table — two batches in flight over one map
  sgtd_engine *attached_to = nullptr;
  unsigned long long table_version = 0;   // bumped by everything that changes the table or its probe layout
  unsigned long long attached_version = 0;
  int n_views = 0;                        // handles attached to this one's table
  // ---- table, insertion order (cold)
  u32 current_frame_id = 0;
  DescStore tab;
  int64_t n_entries = 0;
  int64_t n_add_calls = 0;
  bool have_frames = false;
  u32 frame_lo = 0, frame_hi = 0;
  bool finalized = false;  // the first query builds the (possibly empty) bucket directory

  // ---- table, probe layout (hot): a main segment and, after appends to a finalized table, a
  // tail segment — each a complete probe layout (HotEntry[n] 16 B, perm[n] for the table dump, bucket directory,
  // key hash) over a contiguous range of insertion indices.  Appending re-sorts only the tail;
  // the tail is merged into the main segment when it outgrows an eighth of it.
  struct Segment {
    DevBuf hot, perm, hash, bucket_start, bucket_key, dir;
    u32 hash_mask = 0;
    int64_t n_buckets = 0;
    int64_t g0 = 0, g1 = 0;              // insertion indices [g0, g1)
    double sum_len_sq = 0.0;             // sum over buckets of len^2 (sizes the first batch's work buffers)
    u32 frame_hi = 0;                    // largest frame id inside (at build time)
    bool built = false;
  };
  Segment seg[2];
  int n_seg = 1;
  u32 append_min_frame = 0xFFFFFFFFu;    // smallest frame id appended since the main segment was built
  int64_t tail_max = 0;                  // SGTD_TAIL_MAX: entries the tail may hold before a merge (0 = an eighth of the main segment)
  float ms_finalize = 0.f;               // wall time of the last probe-layout build
  u32 coarse_at = 62, whole_at = 62;     // SGTD_COARSE_AT, SGTD_WHOLE_AT: see TableView
  long long thr2_pending = 0;            // descriptors handed in by the caller whose QueryRec is still to be written (launch_select)
  u32 rec_rate_hook = 0;                 // SGTD_REC_RATE (test hook): ProbeBuffers::rec_rate, 1..256
  u32 rec_rate_cap = 256;                // upper bound on rec_rate for the pending batch: quartered by every re-run whose RESERVATIONS
                                         // (not its matches) outgrew the record buffer — long visit lists with few matches, skewed maps
  bool wide_pairs = false;               // SGTD_WIDE_PAIRS (test hook): 8-byte compact words whatever the ids' rank bits
  int tail_batches = 0;                  // query batches swept with the current tail (it is merged after a few: see settle_tail)
  DevBuf slice_of, sq_sum;
  // entry ids of the probe layout (common.hip.h IdMap), rebuilt over the whole table by every finalize
  DevBuf frame_first, by_frame, id_of_g, longest;
  u32 id_bits = 0;                       // bits of the in-frame rank the built segments' ids use (0: none built)
  bool id_by_frame = false;              // frames out of insertion order: by_frame / id_of_g are in use
  // sgtd_remove_frames: the removed set and the frames that have entries (bitmaps over the frame span), keep masks,
  // survivor counts per tile, and the out-of-place scratch of one field (freed when the call returns)
  DevBuf rm_bits, rm_present, rm_mask, rm_count, rm_scratch;
  // sgtd_set_frame_filter: the caller's rows (global frame ids; replaced as a whole, never changed), and the rows the
  // pending batch was enqueued with — a re-run filters with these whatever was set since.  filt_rows: the batch rows
  // re-based to the table's frame span on the device (filter_kernels.hip.h), made for (filt_rows_serial, _lo, _span)
  std::shared_ptr<const FrameFilter> filt, batch_filt;
  DevBuf filt_rows;
  std::vector<u64> filt_host;      // (the source of their upload)
  u64 filt_rows_serial = 0;
  u32 filt_rows_lo = 0, filt_rows_span = 0;
  // sgtd_set_frame_poses / sgtd_set_position_prior (prior_kernels.hip.h): the poses by global frame id (12 f32 each;
  // has_pose[id] != 0 where set; both grown to the largest id given), the prior, and the prior the pending batch was
  // enqueued with.  pos_dev: (t0, t1, t2, has pose) per local frame of the table's span, made for (pos_serial, _lo,
  // _span); prior_dev: the batch prior's rows; filt_base: the batch filter's rows re-based (when both are set), made
  // for (serial, lo, span) as filt_rows are.  The rows the kernel last wrote into filt_rows were made for prior_key.
  std::vector<float> poses;
  std::vector<unsigned char> has_pose;
  u64 poses_serial = 0;
  std::shared_ptr<const PositionPrior> prior, batch_prior;
  DevBuf pos_dev, prior_dev, filt_base;
  std::vector<float4> pos_host;      // (the source of pos_dev's upload)
  u64 pos_serial = 0;
  u32 pos_lo = 0, pos_span = 0;
  u64 filt_base_serial = 0;
  u32 filt_base_lo = 0, filt_base_span = 0;
  struct PriorKey {
    u64 prior = 0, poses = 0, filt = 0;
    u32 lo = 0, span = 0;
    int n_rows = 0;
    bool operator==(const PriorKey &o) const { return prior == o.prior && poses == o.poses && filt == o.filt && lo == o.lo && span == o.span && n_rows == o.n_rows; }
  } prior_key;
  bool prior_rows_valid = false;
  // sort scratch
  DevBuf keyA, keyB, valA, valB, hist, digit_tot, flags, bad_flag;
  DevBuf order_work;                   // order_kernels.hip.h: tickets, digit histograms and tile state words of a batch's ordering
  std::vector<DevBuf> scan_lvl;

  // ---- build scratch
  DevBuf kp_off_dev, xyz_dev, label_dev, ws_keys, ws_slots, cnt_scan;
  DevBuf b_kp_off_dev, b_xyz_dev, b_label_dev;   // sgtd_build's own staging (never the pending batch's inputs)
  DescStore tmp;        // strided build output for map construction
  DescStore fetch;      // sgtd_fetch_entries staging
  DevBuf fetch_idx;
  DevBuf tmp_count;

  // ---- query batch
  DescStore qd;         // strided query descriptors
  DevBuf q_count;
  long long q_stride = 0;
  int nq = 0;
  bool batch_valid = false, batch_synced = false;
  // inputs of the last batch (for a re-run after a work-buffer overflow)
  int last_kind = 0;    // 1 frames, 2 descs
  const float *last_xyz = nullptr;
  const u32 *last_label = nullptr;
  std::vector<long long> last_kp_off;
  int last_max_n = 0;
  u32 last_qframe = 0;  // current_frame_id_ when the batch was enqueued (a re-run stamps the same id)
  bool loop_batch = false;  // sgtd_loop_frames: query q is stamped last_qframe + q and sees the entries of frames
  int loop_skip = 0;        // below last_qframe + q - loop_skip only (the sweep's BOUND variant)
  DevBuf totals;        // 3 x u64, zeroed once: batch_totals_kernel's running counts
  DevBuf cursors, list, n_visit, votes, slot_of;   // cursors: the batch's counters, overflow flags and ticket heads (ProbeBuffers::ctr)
  DevBuf q_M, q_P, q_pairs, q_pair_base, blk_count, rec, rec_cell, rec_dis;
  DevBuf c_pair, c_blk;           // compact candidate-match lists between block_count and block_write
  DevBuf amb_queue;               // provisional records awaiting the exact test
  DevBuf n_cand, cand_frame, cand_votes, pair_off, pairs;
  DevBuf v_score, v_pose, v_inlier, v_best;   // sgtd_verify results of the batch
  DevBuf inl_pairs, inl_off;                  // sgtd_result_inlier_pairs staging
  bool verify_counted = false;                // the last verify_enqueue left the inlier counts in inl_counts
  DevBuf inl_counts;                          // sgtd_search_frame: inlier pairs per candidate
  DevBuf in_block;                            // copy_in: a frame's descriptors as they arrive, one block
  size_t frame_inl_cap = 0;                   // ... entries its gather has room for (grown when a frame has more inlier pairs)
  char *frame_host = nullptr;                 // ... page-locked host memory the call's last kernels write straight into: the packed small results,
  size_t frame_host_bytes = 0;                //     then the inlier pairs' entries field by field and their query indices (no copy, no second wait)
  DevBuf b_in, b_out;                         // sgtd_build's one-block staging on the device: inputs / all descriptor fields
  char *pin_build = nullptr;                  // ... and in page-locked host memory
  size_t pin_build_cap = 0;
  DevBuf v_hyp64, v_hyp32, v_bound;           // hypotheses between the two passes of sgtd_verify
  DevBuf v_hypB, v_tau, v_words;              // the matrix-core vote pass: hypothesis features, |t|^2, vote words
  DevBuf v_okey[2], v_oval[2];                // its dispatch order: (candidate frame, candidate index) sorted
  bool verified = false;
  // sgtd_refine_poses (refine_kernels.hip.h): the refit poses, residuals, pair counts and moments of the batch, and the
  // flags of the re-selected sets (two halves; sgtd_verify's v_inlier is only read)
  DevBuf r_pose, r_rmse, r_rmse_v, r_npairs, r_moments, r_flag;
  bool refined = false;
  // sgtd_set_frame_keypoints / sgtd_overlap (overlap_kernels.hip.h): the keypoints by global frame id (x, y, z bits and
  // the label, 16 B each; has_kps[id] != 0 where set, a frame of zero keypoints included).  kp_dev / kp_word: the device
  // copy (all stored keypoints back to back; per frame id first << 16 | count, or all ones), made for kp_dev_serial.
  // o_*: the overlap results of the batch and the caller's query keypoints when they were given to sgtd_overlap.
  std::vector<std::vector<uint4>> kps;
  std::vector<unsigned char> has_kps;
  u64 kps_serial = 0, kp_dev_serial = 0;
  DevBuf kp_dev, kp_word, o_cnt, o_val, o_qxyz, o_qlabel, o_qoff;
  std::vector<uint4> kp_host;        // (the sources of their upload)
  std::vector<u64> kp_word_host;
  int kp_dev_max = 0;                // keypoints of the longest frame of the device copy
  bool overlapped = false;
  // sgtd_align_keypoints (align_kernels.hip.h): the aligned results of the batch; a_assign holds candidate_num int32 per
  // query keypoint of the batch (a_qoff: the queries' keypoint offsets, from 0, as the call had them)
  DevBuf a_pose, a_fit, a_cnt, a_val, a_mom, a_assign;
  std::vector<long long> a_qoff;
  bool aligned = false;
  // sgtd_consistent_loops (consistency_kernels.hip.h): independent of the batch.  ck_store / ck_has: the pose store's
  // device copy, made for ck_store_serial; ck_in: the call's inputs; ck_soa / ck_valid: the prepared edges; ck_rows: the
  // bit matrix; ck_pmask, ck_out (in_set, degree, pick), ck_state: the greedy choice.  ck_n < 0: no results.
  DevBuf ck_store, ck_has, ck_in, ck_soa, ck_valid, ck_rows, ck_pmask, ck_out, ck_state;
  u64 ck_store_serial = ~0ull;
  int64_t ck_n = -1;
  double ck_thr[2] = {0.0, 0.0};
  hipEvent_t ck_ev[3] = {};
  // sgtd_pose_consensus (consensus_kernels.hip.h): cs_in: the rows form's inputs; cs_out: every output of the call
  // (ConsensusLayout); the pose store's device copy is ck_store / ck_has.  cs_n < 0: no results; cs_batch: they are the
  // batch form's, and go with the batch's verification (stale_stages).  A group's results live on its first device's
  // engine, which the group's batches and verifications pass through.
  DevBuf cs_in, cs_out;
  int64_t cs_n = -1;
  int cs_cn = 0;
  bool cs_batch = false;
  double cs_thr[2] = {0.0, 0.0};
  // sgtd_relax_poses (relax_kernels.hip.h): independent of the batch.  rx_in: the call's inputs and the node -> edge CSR;
  // rx_state: the two sets of node records; rx_edge: the per-edge streams and costs; rx_node: the node vectors, blocks
  // and factors; rx_ctl: RelaxState.  rx_n < 0: no results; rx_host_*: the sources of the uploads the host makes.
  DevBuf rx_in, rx_state, rx_edge, rx_node, rx_ctl;
  int64_t rx_n = -1, rx_m = 0;
  int rx_cur = 0;
  int rx_max_blocks = 0;      // SGTD_RELAX_MAX_BLOCKS (test hook, read at the handle's first run): the grid cap of its kernels
  std::vector<int> rx_host_csr;
  std::vector<double> rx_host_w;
  std::vector<unsigned char> rx_host_held;
  // A dense GICP run (register_kernels.hip.h): independent of the batch.  in: the call's index arrays, offsets and start
  // poses; pts: the points when the host gave them; cov: a covariance per point of the call's clouds; part: the slices'
  // minima; match: the last pass's matches and M_i; state: RegState per pair; out: the result rows; ctl: the count of
  // unfinished pairs (in, part, match, out: packed, several types each).  n < 0: no results; host_*: what the getters
  // need of the call; clock.ms: covariances, searches, the rest, the whole call (filled under sgtd_set_timing)
  struct DenseRun {
    DevBuf in;
    DevArr<float> pts;
    DevArr<double> cov;
    DevBuf part, match, state, out, ctl;
    int n = -1;
    std::vector<int64_t> host_off;
    std::vector<int> host_soff;         // src_off [n + 1]
    std::vector<unsigned char> host_named;
    std::vector<int> host_up;           // (the source of the index upload)
    LapClock clock;
  };
  DenseRun dense;      // sgtd_register_clouds: every cloud is the call's
  // sgtd_set_frame_clouds (cloud_store_kernels.hip.h): the cloud store, settings of the handle.  st: the arena (points,
  // covariances and the clouds' offsets on the device: the stored clouds are its first clouds, "slots", in arrival
  // order, a call's own clouds follow for the length of the call) and what the host knows of it.  A slot whose frame was
  // overwritten or forgotten is dead until the arena is rebuilt.  st_slot_of: frame id -> live slot or -1, on the host;
  // st_table: its device copy, made for st_table_serial (sgtd_register_stored_loops).  st_k == 0: no settings yet.
  struct CloudSlot { u32 frame; int64_t first, count; bool live; };
  struct CloudArena {
    DevBuf pts, cov, off;
    int64_t cap = 0, off_cap = 0;    // points and offset rows the buffers hold
    int64_t used = 0, live = 0;      // points of all slots, of the live ones
    std::vector<CloudSlot> slots;
  } st;
  std::vector<int> st_slot_of;
  int64_t st_frames = 0;             // frames that have a cloud
  int st_k = 0;
  double st_eps = 0.0;
  DevBuf st_stage, st_idx, st_table;
  u64 st_serial = 0, st_table_serial = ~0ull;
  // sgtd_register_stored / sgtd_register_stored_loops: the dense run over the cloud store's arena (RegSite), independent
  // of the other registration calls' buffers.  stored.cov: the covariances of the call's clouds, copied out of the arena.
  // sr_pairs: the loops form's counts, their scan, pair rows and start poses; sr_rows: the loops form's rows (query,
  // candidate, frame) on the host, sr_loops: the results are that form's.
  DenseRun stored;
  DevBuf sr_pairs;
  bool sr_loops = false;
  std::vector<int32_t> sr_rows;
  size_t sr_init_off = 0;            // the rows' start poses within sr_pairs
  // The runs of equal keys among sorted (key, value) pairs, as the stages that put points into voxels need them
  // (sorted_runs): the sort's pairs, the runs' head flags and their exclusive scan (excl[n]: the count of runs), the
  // counters of the head kernels, the runs' keys and first positions [runs + 1]
  struct RunScratch {
    DevArr<u64> key_a, key_b;
    DevArr<u32> val_a, val_b, flags, excl, counts;
    DevArr<u64> vkey;
    DevArr<u32> vstart;
  };
  // A voxelised GICP run (voxel_register_kernels.hip.h): independent of the batch.  n < 0: no results; mode: the call's
  // neighbor_mode; host_*: what the getters need of the call; clock.ms: covariances, map build, correspondence passes,
  // the rest, the whole call (filled under sgtd_set_timing)
  struct VoxelRun {
    DevArr<char> in;               // the call's index arrays, offsets and poses
    DevArr<float> pts;             // the points when the host gave them
    DevArr<double> cov;            // a covariance per point
    RunScratch runs;               // the members' points by voxel: the voxels' heads, keys and first points
    DevArr<u32> map_vox;           // the maps' ranges of voxels [n_maps + 1]
    DevArr<double> mean, vcov;     // the voxels' Gaussians
    DevArr<int> vid;               // the per-correspondence streams: the voxel,
    DevArr<double> mw;             // ... its weight matrix
    DevArr<RegState> state;        // as DenseRun's
    DevArr<char> out, ctl;
    int n = -1, mode = 1;
    std::vector<int> host_soff;         // src_off [n + 1]
    std::vector<int> host_up;           // (the source of the index upload)
    std::vector<u32> host_map_vox;      // [n_maps + 1]
    LapClock clock;
  };
  VoxelRun vox;        // sgtd_register_voxels: every cloud is the call's
  // sgtd_register_stored_voxels: the same run over the cloud store's arena (VregSite).  pts: the call's points when
  // the host gave them, before they are packed behind the slots; cov: unused, the covariances are the arena's
  VoxelRun svox;
  // sgtd_register_stored_local_loops (stored_local_kernels.hip.h): sv_form: the per-id streams, the rows and the per-map
  // records (StoredLocalParams); sv_members: the member lists, slots, sizes, point offsets and relative poses.  sv_local:
  // svox's results are that form's; sv_rows: its rows (query, candidate, frame, map), sv_map_frame, sv_mem_off: the maps'
  // frames and member offsets, on the host; sv_init_off / sv_member_off / sv_pose_off: where the start poses (in sv_form),
  // the member ids and their poses (in sv_members) lie
  DevBuf sv_form, sv_members;
  bool sv_local = false;
  std::vector<int32_t> sv_rows;
  std::vector<u32> sv_map_frame;
  std::vector<int64_t> sv_mem_off;
  size_t sv_init_off = 0, sv_member_off = 0, sv_pose_off = 0;
  // sgtd_scan_keypoints (scan_kernels.hip.h): independent of the batch, buffers of its own (scan_run, scan_device).
  // sk_n < 0: no results; sk_points / sk_kept: points and keypoints of the run; sk_off / sk_kp_off: the scans' offsets
  // on the host
  struct ScanBufs {
    DevArr<float> pts;                        // the host's points and labels (scan_run's staging),
    DevArr<u32> lab;
    DevArr<long long> off;                    // ... the scans' offsets [S + 1]
    DevArr<u32> sc;                           // per point: (scan, class), range, pitch, azimuth
    DevArr<double> r, pitch, azi;
    DevArr<u64> mm;                           // per (scan, class): the extrema, the votes, the grid's sizes, ranges and ring bounds
    DevArr<u32> vote;
    DevArr<int> grid;
    DevArr<double> range, bounds;
    RunScratch runs;                          // the points by voxel
    DevArr<u32> nbr, nbr_cnt, parent;         // per voxel: its links and its component's root
    DevArr<u32> changed;                      // per round of the components: did anything move
    DevArr<u32> ccount, cmin;                 // per component: its points, its smallest point
    DevArr<u64> ckey_a, ckey_b;               // the clusters' sort into keypoint order
    DevArr<u32> cval_a, cval_b;
    DevArr<long long> kp_off;                 // the scans' keypoint offsets [S + 1]
    DevArr<u32> cl_of_root, kcount, cstart;   // root -> keypoint; per keypoint: its points, their first place
    DevArr<u32> pkey_a, pkey_b, pval_a, pval_b;   // the points' sort by keypoint
    DevArr<int> cluster;                      // per point: its keypoint or -1
    DevArr<float> xyz;                        // the keypoints: centres, labels, point counts
    DevArr<u32> label;
    DevArr<int> npoints;
  } sk;
  int sk_n = -1;
  int64_t sk_points = 0, sk_kept = 0;
  std::vector<int64_t> sk_off, sk_kp_off;
  // sgtd_local_map_keypoints (local_map_kernels.hip.h); the clustering runs in the sk buffers above.  lm_n < 0: no
  // results; lm_kp_off / lm_mem_off / lm_merged: per anchor, on the host; lm_clock.ms: members, gather, scan passes of
  // the last call (filled under sgtd_set_timing)
  struct LocalMapBufs {
    DevArr<float> pose;                       // the scans' poses, offsets [S + 1], the anchors
    DevArr<long long> off;
    DevArr<int> anch, count;                  // per anchor: its members,
    DevArr<long long> merged, mem_off;        // ... its merged cloud's points, its members' offset [A + 1]
    DevArr<int> member;                       // the member lists
    DevArr<LmSeg> seg;                        // a pass's segments, their sizes and first places [n_seg + 1]
    DevArr<u32> cnt, start;
    DevArr<float> mpts;                       // ... and its merged cloud
    DevArr<u32> mlab;
    DevArr<float> xyz;                        // the appended keypoints of all passes
    DevArr<u32> label;
    DevArr<int> npoints;
  } lm;
  int lm_n = -1, lm_passes = 0;
  int64_t lm_kept = 0;
  std::vector<int64_t> lm_kp_off, lm_mem_off, lm_merged;
  LapClock lm_clock;
  // sgtd_thin_clouds (thin_kernels.hip.h): independent of everything else on the handle, buffers of its own (thin_run;
  // no other call touches them, so th.out, the device view, stays valid across the registration calls).
  // th_n < 0: no results; th_stride / th_kept: floats a point and points of th.out; th_out_off / th_dropped: per cloud,
  // on the host; th_clock.ms: the sorts, the whole call (filled under sgtd_set_timing)
  struct ThinBufs {
    DevArr<float> pts;                        // the host's points (staging), the clouds' offsets [S + 1]
    DevArr<long long> off;
    DevArr<u64> key_pt;                       // per point: its cell key, its cloud
    DevArr<u32> cl_pt;
    DevArr<u64> key_a, key_b;                 // the sort by cell, then (stable) by cloud: keys, cloud keys, the points' order
    DevArr<u32> ckey_a, ckey_b, val_a, val_b;
    DevArr<u32> flags, excl;                  // the cells' heads and their scan (excl[P]: the cells),
    DevArr<u32> first, first_excl;            // ... the cells by smallest point index and their scan
    DevArr<u32> counts, cstart;               // the head kernel's counters; the cells' first places [cells + 1]
    DevArr<int> dropped;                      // per cloud: its non-finite and its out-of-range points [S * 2]
    DevArr<long long> out_off;                // the thinned clouds' offsets [S + 1]
    DevArr<float> out;                        // the thinned points
  } th;
  int th_n = -1, th_stride = 3;
  int64_t th_kept = 0;
  std::vector<int64_t> th_out_off;
  std::vector<int32_t> th_dropped;
  LapClock th_clock;
  // ---- multi-GPU step (exchange_kernels.hip.h): the batch's local candidate tables are written, packed, into a caller
  // device buffer as soon as they are final (behind votes_topk_kernel / topk_kernel) and ev_cand is recorded; a side
  // stream waits for it (sgtd_export_wait), all-gathers and merges while the match lists are written, and records
  // ev_export_free (sgtd_export_release): the next batch's export waits for that before it overwrites the buffer
  int *export_packed = nullptr;
  size_t export_cap = 0;                      // ints the caller's buffer holds
  hipEvent_t ev_cand = nullptr, ev_export_free = nullptr;
  bool export_busy = false;
  u32 batch_serial = 0;
  bool defer_lists = false;                   // sgtd_set_deferred_lists: a batch stops behind the candidate tables, sgtd_finish_lists writes the lists
  bool lists_pending = false;                 // ... and has not been called for the batch yet
  bool lists_masked = false;                  // the batch's lists were written for a subset of its candidates (pair_off holds the masked offsets)
  const u64 *verify_keep = nullptr;           // sgtd_verify_masked: device mask of the candidates to verify (one launch)
  const u64 *list_keep = nullptr;             // the mask the batch's lists were last written with (a re-run of the list pass: the same)
  SelectPlan plan;                            // the pending batch's (plan_select): fused_pairs = its match lists come from pairs_query_kernel,
                                              // fused_votes = its candidate tables came from votes_topk_kernel (it also wrote the unmasked offsets)
  DevBuf rough_qi, rough_entry, rough_frame, rough_cell, rough_dis;
  size_t rec_cap = (size_t)1 << 25;    // match records (grown on overflow)
  bool rec_cap_fixed = false;          // SGTD_REC_CAP given: no pre-sizing from the table statistics
  size_t pair_cap = (size_t)1 << 24;   // candidate pairs (grown on overflow)
  DevBuf n_valid, cell_rows, gid, q_prefix, group_first, n_groups;
  DevBuf pos_of_slot, rec_off, pass_pool;   // pass slots and records (probe_kernels.hip.h)
  size_t pool_units = 0;                    // pass pool capacity in 16-B units (0: sized by the first batch; grown on overflow)
  size_t group_cap = 0;                     // GroupRows reserved (0: sized by the first batch; grown on overflow)
  size_t group_cap_hook = 0;                // SGTD_GROUP_CAP (test hook): the first reservation
  size_t amb_min = 65536;                   // SGTD_AMB_MIN (test hook): the undecided queue's floor in entries (above it: rec_cap / 64)
  int sorted_chunk = 0;                // > 0: fixed descriptors per ticket (SGTD_SORTED_CHUNK), else adaptive
  bool diag = false;                   // diagnostic probe build: cell index + distance per match
  int order_form = -1;                 // SGTD_ORDER_FORM (test hook): 0 the launch train, 1 order_kernels.hip.h's chain wherever it applies; unset: the
                                       // chain, except for a one-frame batch of at most SGTD_SMALL_SLOTS slots (plan_select)
  u32 order_polls = SGTD_ORDER_POLLS_DEFAULT;   // SGTD_ORDER_POLLS (test hook): state words a look-back may load before it gives up
  bool order_gave_up = false;          // the batch being synchronised gave up an ordering look-back: its re-runs take the launch train
  bool order_train = false;            // ... set around such a re-run
  int select_mode = 0;                 // SGTD_SELECT_MODE (test hook): 0 auto, 1 the five-kernel passes over the records, 2 the per-query
                                       // workgroups (select_kernels.hip.h) wherever they are supported, whatever the batch size
  // host copies after sync
  PinnedVec<u32> h_count, h_pair_base, h_q_M;
  PinnedVec<unsigned long long> h_q_P;
  PinnedVec<int> h_n_cand, h_cand_frame, h_cand_votes;
  PinnedVec<long long> h_pair_off;
  sgtd_stats stats{};
  // pinned host staging of the small transfers (see d2h / h2d below)
  char *pin = nullptr;
  size_t pin_cap = 0, pin_used = 0;
  struct PinCopy { void *dst; size_t off, bytes; };
  std::vector<PinCopy> pin_pending;
};

#include "multi.hip.h"

namespace {

#define HIPCHK(call)                                                          \
  do {                                                                        \
    hipError_t _s = (call);                                                   \
    if (_s != hipSuccess) {                                                   \
      e->err = std::string(#call) + ": " + hipGetErrorString(_s);             \
      return SGTD_ERR_HIP;                                                    \
    }                                                                         \
  } while (0)
#define CHK(call)                 \
  do {                            \
    int _r = (call);              \
    if (_r != SGTD_OK) return _r; \
  } while (0)

// what the stages on a verified batch left (sgtd_refine_poses, sgtd_overlap, sgtd_align_keypoints) belongs to the
// verification before this one
void stale_stages(sgtd_engine *e) {
  e->refined = false; e->overlapped = false; e->aligned = false;
  if (e->cs_batch) e->cs_n = -1;      // (sgtd_pose_consensus over this batch; the rows form's results stay)
}
// the batch's candidates or lists are new: so is, or will be, everything after them
void new_results(sgtd_engine *e, bool verified) { e->verified = verified; stale_stages(e); }

int ensure(sgtd_engine *e, DevBuf &b, size_t bytes, bool keep = false) {
  if (bytes <= b.bytes) return SGTD_OK;
  if (b.borrowed) { e->err = "a table attached from another handle cannot grow here"; return SGTD_ERR_STATE; }
  // (a buffer that grows again gets a quarter more than asked for: the one-frame-per-call pattern would
  // otherwise free and allocate a dozen work buffers on every frame that is a little larger than the last)
  size_t want = keep ? std::max(bytes, b.bytes + b.bytes / 2) : (b.p ? bytes + bytes / 4 : bytes);
  // nothing to keep: the old buffer goes first (a record buffer that grows from 30 to 45 GB must not need 75 for a moment)
  if (!keep && b.p) {
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipFree(b.p));
    b.p = nullptr; b.bytes = 0;
  }
  void *np = nullptr;
  {
    const hipError_t st_ = hipMalloc(&np, want);
    if (st_ != hipSuccess) {
      (void)hipGetLastError();      // (the runtime's "last error" is the caller's too — torch raises on it at its next call — this one is reported here)
      e->err = "hipMalloc of " + std::to_string(want) + " bytes: " + hipGetErrorString(st_);
      return SGTD_ERR_HIP;
    }
  }
  e->stats.device_allocs_total++;
  if (keep && b.p && b.bytes) {
    HIPCHK(hipMemcpyAsync(np, b.p, b.bytes, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  if (b.p) HIPCHK(hipFree(b.p));
  b.p = np;
  b.bytes = want;
  return SGTD_OK;
}

int ensure_store(sgtd_engine *e, DescStore &s, size_t cap, bool keep = false) {
  if (cap <= s.cap) return SGTD_OK;
  size_t want = keep ? std::max(cap, s.cap + s.cap / 2) : cap;
  CHK(ensure(e, s.side, want * 3 * sizeof(double), keep));
  CHK(ensure(e, s.angle, want * 3 * sizeof(double), keep));
  CHK(ensure(e, s.center, want * 3 * sizeof(double), keep));
  CHK(ensure(e, s.vertex, want * 9 * sizeof(float), keep));
  CHK(ensure(e, s.label, want * 3 * sizeof(int), keep));
  CHK(ensure(e, s.frame, want * sizeof(u32), keep));
  CHK(ensure(e, s.node_id, want * 3 * sizeof(int), keep));
  if (s.with_thr2) CHK(ensure(e, s.qrec, want * sizeof(QueryRec), keep));
  s.cap = want;
  return SGTD_OK;
}

// the one place a typed array is sized (16 bytes at the least: an empty call's kernels still get a pointer)
template <class T>
int need(sgtd_engine *e, DevArr<T> &a, size_t n_elems, bool keep = false) {
  return ensure(e, a.buf, std::max<size_t>(n_elems * sizeof(T), 16), keep);
}
// ... several arrays of n elements each, in the order given
template <class... A>
int need_each(sgtd_engine *e, size_t n, A &...a) {
  int r = SGTD_OK;
  (void)(((r = need(e, a, n)) == SGTD_OK) && ...);
  return r;
}

// a buffer released in the middle of a handle's life (whatever is left at the end goes with the handle)
void free_buf(DevBuf &b) { b = DevBuf(); }
using DenseRun = sgtd_engine::DenseRun;
using VoxelRun = sgtd_engine::VoxelRun;

// ---------------------------------------------------------------------------
// Small host <-> device transfers go through ONE pinned staging buffer per handle: a
// hipMemcpyAsync on pageable memory costs ~150 us each on this runtime (the reference's
// one-frame-per-call pattern issues ~60 of them per frame), on pinned memory a few.
// d2h: queue a copy device -> pinned and remember where the caller wants it; xfer_sync: wait for
// the stream, then move the queued results to the caller's (pageable) buffers.  h2d: copy the
// caller's data into pinned memory at once, queue pinned -> device; the pinned bytes are reused
// only after the next xfer_sync.  Transfers beyond kPinMax take the direct path (bandwidth-bound).
// ---------------------------------------------------------------------------
constexpr size_t kPinMax = (size_t)1 << 20, kPinCap = (size_t)16 << 20;   // (a frame's 7 200 descriptors: 172 KB of sides, 259 KB of vertices — one frame's fields all take
                                                                           // the staged path; beyond 1 MB a transfer is bandwidth-bound and the extra host copy costs more than it saves)

int xfer_sync(sgtd_engine *e) {
  HIPCHK(hipStreamSynchronize(e->stream));
  for (const auto &c : e->pin_pending) std::memcpy(c.dst, e->pin + c.off, c.bytes);
  e->pin_pending.clear();
  e->pin_used = 0;
  return SGTD_OK;
}

// d2h queues {destination, pinned offset}; only xfer_sync applies the queue.  A function that returns early (a failed
// HIP call between its d2h calls and its xfer_sync) must not leave entries behind whose destinations are its own
// locals: PinScope drops whatever is still queued when the function is left.
struct PinScope {
  sgtd_engine *e;
  explicit PinScope(sgtd_engine *e_) : e(e_) {}
  ~PinScope() {
    if (e && !e->pin_pending.empty()) {
      (void)hipStreamSynchronize(e->stream);      // (the copies into the pinned buffer may still be in flight)
      e->pin_pending.clear();
      e->pin_used = 0;
    }
  }
};

int pin_room(sgtd_engine *e, size_t bytes, size_t *off) {
  if (!e->pin) {
    void *p = nullptr;
    HIPCHK(hipHostMalloc(&p, kPinCap, hipHostMallocDefault));
    e->pin = static_cast<char *>(p);
    e->pin_cap = kPinCap;
  }
  const size_t need = (bytes + 255) & ~(size_t)255;
  if (e->pin_used + need > e->pin_cap) CHK(xfer_sync(e));   // full: finish what is queued, start over
  *off = e->pin_used;
  e->pin_used += need;
  return SGTD_OK;
}

int d2h(sgtd_engine *e, void *dst, const void *src_dev, size_t bytes) {
  if (bytes == 0) return SGTD_OK;
  if (bytes > kPinMax) {
    HIPCHK(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, e->stream));
    return SGTD_OK;
  }
  size_t off;
  CHK(pin_room(e, bytes, &off));
  HIPCHK(hipMemcpyAsync(e->pin + off, src_dev, bytes, hipMemcpyDeviceToHost, e->stream));
  e->pin_pending.push_back({dst, off, bytes});
  return SGTD_OK;
}

int h2d(sgtd_engine *e, void *dst_dev, const void *src, size_t bytes) {
  if (bytes == 0) return SGTD_OK;
  if (bytes > kPinMax) {
    HIPCHK(hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice, e->stream));
    return SGTD_OK;
  }
  size_t off;
  CHK(pin_room(e, bytes, &off));
  std::memcpy(e->pin + off, src, bytes);
  HIPCHK(hipMemcpyAsync(dst_dev, e->pin + off, bytes, hipMemcpyHostToDevice, e->stream));
  return SGTD_OK;
}

int grid_for(long long n, int threads) { return (int)((n + threads - 1) / threads); }
// what 32-bit indices can name: candidate pairs one by one, match records by granules of four (probe_kernels.hip.h)
constexpr size_t kIndexLimit = 0xFFFFFFF0ull;
constexpr size_t kRecLimit = kIndexLimit << SGTD_REC_SHIFT;
// dynamic LDS a kernel may ask for: gfx950 gives a workgroup 160 KB, the kernel's static __shared__ arrays included (the
// policy bound of 150 KB alone let a launch of a kernel with 12.6 KB of static LDS fail for spans that need 147.5 .. 150 KB)
template <class K>
size_t lds_room(K *kernel) {
  hipFuncAttributes a;
  const size_t fixed = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(kernel)) == hipSuccess ? a.sharedSizeBytes : 16384;
  return std::min<size_t>(150 * 1024, 160 * 1024 - std::min<size_t>(fixed, 160 * 1024));
}

// device-wide exclusive scan (u32), in place allowed
int device_scan(sgtd_engine *e, const u32 *in, u32 *out, long long n, size_t lvl = 0) {
  if (n <= 0) return SGTD_OK;
  const long long per = (long long)SGTD_SCAN_THREADS * SGTD_SCAN_ITEMS;
  const long long nb = (n + per - 1) / per;
  if (nb == 1) {
    scan_apply_kernel<<<1, SGTD_SCAN_THREADS, 0, e->stream>>>(in, out, nullptr, n);
    HIPCHK(hipGetLastError());
    return SGTD_OK;
  }
  if (e->scan_lvl.size() <= lvl) e->scan_lvl.resize(lvl + 1);
  CHK(ensure(e, e->scan_lvl[lvl], (size_t)nb * sizeof(u32)));
  u32 *sums = e->scan_lvl[lvl].as<u32>();
  scan_reduce_kernel<<<(int)nb, SGTD_SCAN_THREADS, 0, e->stream>>>(in, sums, n);
  HIPCHK(hipGetLastError());
  CHK(device_scan(e, sums, sums, nb, lvl + 1));
  sums = e->scan_lvl[lvl].as<u32>();
  scan_apply_kernel<<<(int)nb, SGTD_SCAN_THREADS, 0, e->stream>>>(in, out, sums, n);
  HIPCHK(hipGetLastError());
  return SGTD_OK;
}

// ---------------------------------------------------------------------------
// BuildSingleScanSTD launch for a batch of frames (inputs already on device)
// ---------------------------------------------------------------------------
// keypoints of one frame: the kernels keep a frame's keypoint indices and counts in 16 bits
constexpr int kMaxKeypoints = 65535;
bool keypoint_count_ok(long long n) { return n >= 0 && n <= kMaxKeypoints; }

int launch_build(sgtd_engine *e, const float *d_xyz, const u32 *d_label, const long long *d_kp_off,
                 int n_frames, int max_n, u32 frame_id0, int frame_step, DescArrays out,
                 long long out_stride, u32 *out_count) {
  if (n_frames <= 0) return SGTD_OK;
  if (max_n > kMaxKeypoints) return SGTD_ERR_UNSUPPORTED;
  const int K = e->dc.K, tpi = e->dc.tpi;
  long long max_t = (long long)std::max(max_n, 1) * tpi;
  int max_slots = 64;
  while (max_slots < max_t + 1) max_slots <<= 1;
  const size_t lds_limit = 160 * 1024;
  size_t lds_full = build_lds_bytes(std::max(max_n, 1), K, tpi, true, max_slots);
  size_t lds_base = build_lds_bytes(std::max(max_n, 1), K, tpi, false, max_slots);
  BuildParams P;
  P.xyz = d_xyz; P.label = d_label; P.kp_off = d_kp_off; P.n_frames = n_frames;
  P.frame_id0 = frame_id0; P.frame_id_step = frame_step; P.out_stride = out_stride;
  P.out_count = out_count; P.max_n = std::max(max_n, 1); P.max_slots = max_slots;
  P.ws_keys = nullptr; P.ws_slots = nullptr;
  if (lds_full <= lds_limit) {
    int per_cu = (int)std::max<size_t>(1, lds_limit / lds_full);
    int grid = std::min(n_frames, e->n_cus * std::min(per_cu, 4));
#define SGTD_LAUNCH_BUILD(DEDUP, KM_, LDS_)                                                                    \
  do {                                                                                                          \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&build_frames_kernel<DEDUP, KM_>),                \
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_)));                       \
    build_frames_kernel<DEDUP, KM_><<<grid, SGTD_BUILD_THREADS, (LDS_), e->stream>>>(P, e->dc, out);            \
  } while (0)
#define SGTD_LAUNCH_BUILD_K(DEDUP, LDS_)                                                                        \
  do {                                                                                                          \
    if (K <= 4) SGTD_LAUNCH_BUILD(DEDUP, 4, LDS_);                                                              \
    else if (K <= 8) SGTD_LAUNCH_BUILD(DEDUP, 8, LDS_);                                                         \
    else if (K <= 10) SGTD_LAUNCH_BUILD(DEDUP, 10, LDS_);                                                       \
    else if (K <= 12) SGTD_LAUNCH_BUILD(DEDUP, 12, LDS_);                                                       \
    else SGTD_LAUNCH_BUILD(DEDUP, 16, LDS_);                                                                    \
  } while (0)
    SGTD_LAUNCH_BUILD_K(true, lds_full);
  } else if (lds_base <= lds_limit) {
    int grid = std::min(n_frames, e->n_cus * 2);
    CHK(ensure(e, e->ws_keys, (size_t)grid * max_t * sizeof(u64)));
    CHK(ensure(e, e->ws_slots, (size_t)grid * max_slots * sizeof(u32)));
    P.ws_keys = e->ws_keys.as<u64>();
    P.ws_slots = e->ws_slots.as<u32>();
    SGTD_LAUNCH_BUILD_K(false, lds_base);
#undef SGTD_LAUNCH_BUILD_K
#undef SGTD_LAUNCH_BUILD
  } else {
    return SGTD_ERR_UNSUPPORTED;
  }
  HIPCHK(hipGetLastError());
  return SGTD_OK;
}

// uploads keypoints (or takes device pointers) and the offsets; returns views
// own_set: sgtd_build stages into buffers of its own — a synced query batch may still be re-run
// from the batch's staging buffers (sgtd_result_rough's diagnostic pass)
int stage_inputs(sgtd_engine *e, const float *xyz, const u32 *label, const int64_t *kp_off,
                 int n_frames, int device_ptrs, const float **d_xyz, const u32 **d_label,
                 int *max_n, bool own_set = false) {
  DevBuf &kp_buf = own_set ? e->b_kp_off_dev : e->kp_off_dev;
  DevBuf &xyz_buf = own_set ? e->b_xyz_dev : e->xyz_dev;
  DevBuf &label_buf = own_set ? e->b_label_dev : e->label_dev;
  std::vector<long long> off(n_frames + 1);
  int mx = 0;
  for (int f = 0; f <= n_frames; f++) off[f] = kp_off[f];
  for (int f = 0; f < n_frames; f++) {
    long long n = off[f + 1] - off[f];
    if (!keypoint_count_ok(n)) return SGTD_ERR_INVALID;
    mx = std::max(mx, (int)n);
  }
  *max_n = mx;
  CHK(ensure(e, kp_buf, (size_t)(n_frames + 1) * sizeof(long long)));
  // through the page-locked staging (the bytes leave `off` here): no wait for the stream — a caller that enqueues batch
  // after batch keeps the device fed, the next batch's kernels queue up behind the running one's
  if ((size_t)(n_frames + 1) * sizeof(long long) <= kPinMax) {
    CHK(h2d(e, kp_buf.p, off.data(), (size_t)(n_frames + 1) * sizeof(long long)));
  } else {
    HIPCHK(hipMemcpyAsync(kp_buf.p, off.data(), (size_t)(n_frames + 1) * sizeof(long long), hipMemcpyHostToDevice, e->stream));
    CHK(xfer_sync(e));      // (the staging vector dies at return)
  }
  const long long total = off[n_frames] - off[0];
  if (device_ptrs) {
    *d_xyz = xyz;
    *d_label = label;
  } else {
    CHK(ensure(e, xyz_buf, (size_t)std::max<long long>(total + off[0], 1) * 3 * sizeof(float)));
    CHK(ensure(e, label_buf, (size_t)std::max<long long>(total + off[0], 1) * sizeof(u32)));
    if (total > 0) {
      CHK(h2d(e, xyz_buf.as<float>() + off[0] * 3, xyz + off[0] * 3,
                            (size_t)total * 3 * sizeof(float)));
      CHK(h2d(e, label_buf.as<u32>() + off[0], label + off[0], (size_t)total * sizeof(u32)));
    }
    *d_xyz = xyz_buf.as<float>();
    *d_label = label_buf.as<u32>();
  }
  return SGTD_OK;
}

// device SoA range -> caller SoA (NULL members skipped)
int copy_out(sgtd_engine *e, const DescStore &s, size_t first, size_t n, sgtd_desc_soa *out, size_t dst0) {
  if (n == 0) return SGTD_OK;
#define CP(field, T, w)                                                                       \
  if (out->field)                                                                             \
    CHK(d2h(e, out->field + dst0 * (w), s.field.as<T>() + first * (w),             \
                          n * (w) * sizeof(T)));
  CP(side, double, 3) CP(angle, double, 3) CP(center, double, 3) CP(vertex, float, 9)
  CP(label, int, 3) CP(frame, u32, 1) CP(node_id, int, 3)
#undef CP
  CHK(xfer_sync(e));
  return SGTD_OK;
}

int copy_in(sgtd_engine *e, DescStore &s, size_t first, size_t n, const sgtd_desc_soa *in, bool wait = true) {
  if (n == 0) return SGTD_OK;
  // a frame's descriptors (up to a few MB): the seven fields side by side in the page-locked staging, ONE transfer into a block on
  // the device and a kernel that deals the words to the arrays — seven transfers of ~100 KB took ~0.2 ms before the first kernel
  // of a one-frame call could start, one takes 0.04
  const DescBlockOffsets bo = desc_block_offsets(n);
  static const bool block_on = [] { const char *o = getenv("SGTD_COPY_IN_BLOCK"); return !(o && !atoi(o)); }();
  if (block_on && bo.total <= (4u << 20)) {
    size_t off;
    CHK(pin_room(e, bo.total, &off));
    const void *src[7] = {in->side, in->angle, in->center, in->vertex, in->label, in->frame, in->node_id};
    void *dst[7] = {s.side.as<double>() + first * 3, s.angle.as<double>() + first * 3, s.center.as<double>() + first * 3, s.vertex.as<float>() + first * 9,
                    s.label.as<int>() + first * 3, s.frame.as<u32>() + first, s.node_id.as<int>() + first * 3};
    const size_t bytes[7] = {n * 24, n * 24, n * 24, n * 36, n * 12, n * 4, n * 12};
    u32 present = 0;
    for (int f = 0; f < 7; f++) {
      if (src[f]) { std::memcpy(e->pin + off + bo.off[f], src[f], bytes[f]); present |= 1u << f; }
      else HIPCHK(hipMemsetAsync(dst[f], 0, bytes[f], e->stream));
    }
    CHK(ensure(e, e->in_block, bo.total));
    HIPCHK(hipMemcpyAsync(e->in_block.p, e->pin + off, bo.total, hipMemcpyHostToDevice, e->stream));
    unpack_desc_block_kernel<<<(unsigned)std::min<long long>(grid_for((long long)n * 34, 256), 512), 256, 0, e->stream>>>(e->in_block.as<unsigned char>(), (u32)n, present, s.view(),
                                                                                                                       (long long)first);
    HIPCHK(hipGetLastError());
    if (wait) CHK(xfer_sync(e));
    return SGTD_OK;
  }
#define CP(field, T, w)                                                                        \
  if (in->field)                                                                               \
    CHK(h2d(e, s.field.as<T>() + first * (w), in->field, n * (w) * sizeof(T)));               \
  else                                                                                         \
    HIPCHK(hipMemsetAsync(s.field.as<T>() + first * (w), 0, n * (w) * sizeof(T), e->stream));
  CP(side, double, 3) CP(angle, double, 3) CP(center, double, 3) CP(vertex, float, 9)
  CP(label, int, 3) CP(frame, u32, 1) CP(node_id, int, 3)
#undef CP
  // (wait = false: every field went through the page-locked staging — at most 256 KB each — or is read from the caller's
  // memory until the caller's next wait on the stream: sgtd_search_frame, whose inputs stay valid for the call)
  if (wait) CHK(xfer_sync(e));
  return SGTD_OK;
}

void note_frames(sgtd_engine *e, u32 lo, u32 hi) {
  if (!e->have_frames) {
    e->frame_lo = lo; e->frame_hi = hi; e->have_frames = true;
  } else {
    e->frame_lo = std::min(e->frame_lo, lo);
    e->frame_hi = std::max(e->frame_hi, hi);
  }
}

// ---------------------------------------------------------------------------
// finalize: sort + CSR + hash
// ---------------------------------------------------------------------------
// stable LSD radix sort of (key, val) pairs by the low `bits` of the key, 8-bit digits; passes
// whose digit is the same for every key are skipped (skip_const: costs a host round trip per
// pass, only used by the once-per-map table build).  The result is in kin / vin.
template <class KeyT>
int radix_sort_pairs(sgtd_engine *e, KeyT *&kin, KeyT *&kout, u32 *&vin, u32 *&vout, long long n, int bits,
                     bool skip_const, const u32 *n_dev = nullptr) {
  const int nblocks = (int)((n + SGTD_RS_TILE - 1) / SGTD_RS_TILE);
  CHK(ensure(e, e->hist, (size_t)256 * nblocks * sizeof(u32)));
  CHK(ensure(e, e->digit_tot, 256 * sizeof(u32)));
  std::vector<u32> tot(256);
  for (int shift = 0; shift < bits; shift += 8) {
    u32 *hist = e->hist.as<u32>();
    radix_hist_kernel<KeyT><<<nblocks, SGTD_RS_THREADS, 0, e->stream>>>(kin, n, shift, hist, nblocks, n_dev);
    HIPCHK(hipGetLastError());
    if (skip_const) {
      radix_digit_totals_kernel<<<256, SGTD_SCAN_THREADS, 0, e->stream>>>(hist, nblocks, e->digit_tot.as<u32>());
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(tot.data(), e->digit_tot.p, 256 * sizeof(u32), hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      bool constant = false;
      for (int d = 0; d < 256; d++)
        if ((long long)tot[d] == n) constant = true;
      if (constant) continue;  // every key has the same digit here: the pass is the identity
    }
    CHK(device_scan(e, hist, hist, (long long)256 * nblocks));
    radix_scatter_kernel<KeyT><<<nblocks, SGTD_RS_THREADS, 0, e->stream>>>(kin, vin, kout, vout, n, shift,
                                                                       e->hist.as<u32>(), nblocks, n_dev);
    HIPCHK(hipGetLastError());
    std::swap(kin, kout);
    std::swap(vin, vout);
  }
  return SGTD_OK;
}

IdMap id_map(const sgtd_engine *e, u32 bits) {
  IdMap m;
  m.frame_first = e->frame_first.as<u32>();
  m.by_frame = e->id_by_frame ? e->by_frame.as<u32>() : nullptr;
  m.bits = bits;
  m.frame_lo = e->have_frames ? e->frame_lo : 0;
  return m;
}

// probe layout of the entries [g0, g1) into segment S: sort by key, slices, directory, hash
int build_segment(sgtd_engine *e, sgtd_engine::Segment &S, long long g0, long long g1) {
  const long long E = g1 - g0;
  S.g0 = g0; S.g1 = g1;
  S.n_buckets = 0;
  S.hash_mask = 1023;
  S.sum_len_sq = 0.0;
  S.frame_hi = e->have_frames ? e->frame_hi : 0;
  S.built = true;
  if (E == 0) {
    CHK(ensure(e, S.hash, (size_t)1024 * sizeof(HashSlot)));
    HIPCHK(hipMemsetAsync(S.hash.p, 0xFF, (size_t)1024 * sizeof(HashSlot), e->stream));
    return SGTD_OK;
  }
  // the arrays of this range, indexed by the entry's position inside it
  const double *side = e->tab.side.as<double>() + (size_t)g0 * 3;
  const int *label = e->tab.label.as<int>() + (size_t)g0 * 3;
  const u32 *frame = e->tab.frame.as<u32>() + (size_t)g0;
  CHK(ensure(e, e->keyA, (size_t)E * sizeof(u64)));
  CHK(ensure(e, e->keyB, (size_t)E * sizeof(u64)));
  CHK(ensure(e, e->valA, (size_t)E * sizeof(u32)));
  CHK(ensure(e, e->valB, (size_t)E * sizeof(u32)));
  CHK(ensure(e, e->bad_flag, 2 * sizeof(int)));
  HIPCHK(hipMemsetAsync(e->bad_flag.p, 0, 2 * sizeof(int), e->stream));
  make_keys_kernel<<<grid_for(E, 256), 256, 0, e->stream>>>(side, label, e->keyA.as<u64>(), e->valA.as<u32>(), E,
                                                             e->bad_flag.as<int>());
  HIPCHK(hipGetLastError());
  frame_monotone_kernel<<<grid_for(E, 256), 256, 0, e->stream>>>(frame, E, e->bad_flag.as<int>() + 1);
  HIPCHK(hipGetLastError());
  int bad[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(bad, e->bad_flag.p, sizeof(bad), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (bad[0]) { S.built = false; return SGTD_ERR_UNSUPPORTED; }  // a cell coordinate beyond 16 bits
  const bool monotone = bad[1] == 0;

  u64 *kin = e->keyA.as<u64>(), *kout = e->keyB.as<u64>();
  u32 *vin = e->valA.as<u32>(), *vout = e->valB.as<u32>();
  CHK(ensure(e, e->slice_of, (size_t)E));
  if (!monotone) {
    // frame ids out of insertion order (caller-stamped descriptors): the slice assignment needs
    // every bucket grouped by frame, so sort by (key, frame, g) for it, then start over
    frame_keys_kernel<<<grid_for(E, 256), 256, 0, e->stream>>>(frame, kin, vin, E);
    HIPCHK(hipGetLastError());
    CHK(radix_sort_pairs(e, kin, kout, vin, vout, E, 32, true));
    keys_of_order_kernel<<<grid_for(E, 256), 256, 0, e->stream>>>(side, label, vin, kin, E);
    HIPCHK(hipGetLastError());
    CHK(radix_sort_pairs(e, kin, kout, vin, vout, E, 60, true));
    slice_assign_kernel<<<grid_for(E, 256), 256, 0, e->stream>>>(kin, vin, side, frame, E, e->dc.rough, e->slice_of.as<unsigned char>());
    HIPCHK(hipGetLastError());
    kin = e->keyA.as<u64>(); kout = e->keyB.as<u64>(); vin = e->valA.as<u32>(); vout = e->valB.as<u32>();
    make_keys_kernel<<<grid_for(E, 256), 256, 0, e->stream>>>(side, label, kin, vin, E, e->bad_flag.as<int>());
    HIPCHK(hipGetLastError());
  }
  CHK(radix_sort_pairs(e, kin, kout, vin, vout, E, 60, true));   // (key, g): buckets in insertion order
  if (monotone) {
    slice_assign_kernel<<<grid_for(E, 256), 256, 0, e->stream>>>(kin, vin, side, frame, E, e->dc.rough, e->slice_of.as<unsigned char>());
    HIPCHK(hipGetLastError());
  }
  // buckets
  CHK(ensure(e, e->flags, (size_t)E * sizeof(u32)));
  head_flags_kernel<<<grid_for(E, 256), 256, 0, e->stream>>>(kin, e->flags.as<u32>(), E);
  HIPCHK(hipGetLastError());
  u32 last_flag = 0, last_excl = 0;
  HIPCHK(hipMemcpyAsync(&last_flag, e->flags.as<u32>() + (E - 1), sizeof(u32), hipMemcpyDeviceToHost, e->stream));
  CHK(device_scan(e, e->flags.as<u32>(), e->flags.as<u32>(), E));
  HIPCHK(hipMemcpyAsync(&last_excl, e->flags.as<u32>() + (E - 1), sizeof(u32), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  const u32 U = last_excl + last_flag;
  S.n_buckets = U;
  CHK(ensure(e, S.bucket_start, (size_t)(U + 1) * sizeof(u32)));
  CHK(ensure(e, S.bucket_key, (size_t)U * sizeof(u64)));
  bucket_starts_kernel<<<grid_for(E, 256), 256, 0, e->stream>>>(kin, e->flags.as<u32>(), S.bucket_start.as<u32>(),
                                                                 S.bucket_key.as<u64>(), E);
  HIPCHK(hipGetLastError());
  // probe order: every bucket partitioned by slice, insertion order inside a slice
  CHK(ensure(e, S.perm, (size_t)(E + SGTD_SENTINELS) * sizeof(u32)));
  CHK(ensure(e, S.dir, (size_t)U * sizeof(BucketDir)));
  slice_partition_kernel<<<e->n_cus * 8, 256, 0, e->stream>>>(S.bucket_start.as<u32>(), U, (u32)E, vin,
                                                               e->slice_of.as<unsigned char>(), S.perm.as<u32>(),
                                                               S.dir.as<BucketDir>());
  HIPCHK(hipGetLastError());
  // the probe layout of the tail segment lies BEHIND the main segment's (and its sentinels) in the main
  // segment's buffer: one base address for both, so that a pass's visit list can run through both segments
  HotEntry *hot = nullptr;
  if (&S == &e->seg[1]) {
    sgtd_engine::Segment &M = e->seg[0];
    const size_t m_ent = (size_t)(M.g1 - M.g0) + SGTD_SENTINELS;
    CHK(ensure(e, M.hot, (m_ent + (size_t)E + SGTD_SENTINELS) * sizeof(HotEntry), /*keep=*/true));
    hot = M.hot.as<HotEntry>() + m_ent;
  } else {
    // (with room for the largest tail do_finalize accepts, so that an append does not move the layout;
    // none under the SGTD_TAIL_MAX test hook: the tail's build then grows the buffer and moves it)
    const size_t tail_room = e->tail_max > 0 ? 0 : (size_t)std::max<long long>(262144, E / 8) + SGTD_SENTINELS;
    CHK(ensure(e, S.hot, ((size_t)(E + SGTD_SENTINELS) + tail_room) * sizeof(HotEntry)));
    hot = S.hot.as<HotEntry>();
  }
  gather_hot_kernel<<<grid_for(E + SGTD_SENTINELS, 256), 256, 0, e->stream>>>(
      S.perm.as<u32>(), side, frame, e->id_by_frame ? e->id_of_g.as<u32>() : nullptr, id_map(e, e->id_bits), hot, E, (u32)g0);
  HIPCHK(hipGetLastError());
  u32 cap = 1024;
  while (cap < 2ull * U) cap <<= 1;
  S.hash_mask = cap - 1;
  CHK(ensure(e, S.hash, (size_t)cap * sizeof(HashSlot)));
  HIPCHK(hipMemsetAsync(S.hash.p, 0xFF, (size_t)cap * sizeof(HashSlot), e->stream));
  hash_insert_kernel<<<grid_for(U, 256), 256, 0, e->stream>>>(S.bucket_key.as<u64>(), S.bucket_start.as<u32>(), U,
                                                               (u32)E, S.hash.as<HashSlot>(), S.hash_mask);
  HIPCHK(hipGetLastError());
  CHK(ensure(e, e->sq_sum, sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(e->sq_sum.p, 0, sizeof(unsigned long long), e->stream));
  bucket_sq_kernel<<<grid_for(U, 256), 256, 0, e->stream>>>(S.bucket_start.as<u32>(), U, (u32)E, e->sq_sum.as<unsigned long long>());
  HIPCHK(hipGetLastError());
  unsigned long long sq = 0;
  HIPCHK(hipMemcpyAsync(&sq, e->sq_sum.p, sizeof(sq), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  S.sum_len_sq = (double)sq;
  return SGTD_OK;
}

// The entry ids (IdMap) of the whole table: frame_first (+ by_frame, id_of_g when frame ids are out
// of insertion order) and the number of bits the in-frame rank needs.  `bits` is what the ids of
// the segments built from now on use; a change invalidates segments built with another value.
int build_idmap(sgtd_engine *e, u32 &bits) {
  const long long E = e->n_entries;
  bits = e->id_bits ? e->id_bits : 13;
  if (E == 0 || !e->have_frames) return SGTD_OK;
  const u32 lo = e->frame_lo, span = e->frame_hi - e->frame_lo + 1;
  const u32 *frame = e->tab.frame.as<u32>();
  CHK(ensure(e, e->frame_first, (size_t)span * sizeof(u32)));
  CHK(ensure(e, e->longest, 2 * sizeof(u32)));
  HIPCHK(hipMemsetAsync(e->longest.p, 0, 2 * sizeof(u32), e->stream));
  frame_monotone_kernel<<<grid_for(E, 256), 256, 0, e->stream>>>(frame, E, reinterpret_cast<int *>(e->longest.as<u32>() + 1));
  HIPCHK(hipGetLastError());
  u32 h[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(h, e->longest.p, sizeof(h), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->id_by_frame = h[1] != 0;
  const u32 *key = frame;
  if (e->id_by_frame) {
    CHK(ensure(e, e->keyA, (size_t)E * sizeof(u64)));
    CHK(ensure(e, e->keyB, (size_t)E * sizeof(u64)));
    CHK(ensure(e, e->valA, (size_t)E * sizeof(u32)));
    CHK(ensure(e, e->valB, (size_t)E * sizeof(u32)));
    u64 *kin = e->keyA.as<u64>(), *kout = e->keyB.as<u64>();
    u32 *vin = e->valA.as<u32>(), *vout = e->valB.as<u32>();
    frame_keys_kernel<<<grid_for(E, 256), 256, 0, e->stream>>>(frame, kin, vin, E);
    HIPCHK(hipGetLastError());
    CHK(radix_sort_pairs(e, kin, kout, vin, vout, E, 32, true));     // stable: insertion order inside a frame
    CHK(ensure(e, e->by_frame, (size_t)E * sizeof(u32)));
    CHK(ensure(e, e->id_of_g, (size_t)E * sizeof(u32)));
    HIPCHK(hipMemcpyAsync(e->by_frame.p, vin, (size_t)E * sizeof(u32), hipMemcpyDeviceToDevice, e->stream));
    // the sorted frame ids as 32-bit words in the sort's spare value buffer (the sort is over; the
    // kernels below run before build_segment reuses the scratch)
    low_words_kernel<<<grid_for(E, 256), 256, 0, e->stream>>>(kin, E, vout);
    HIPCHK(hipGetLastError());
    key = vout;
  }
  frame_first_kernel<<<grid_for(E, 256), 256, 0, e->stream>>>(key, E, lo, e->frame_first.as<u32>());
  HIPCHK(hipGetLastError());
  frame_longest_kernel<<<grid_for(E, 256), 256, 0, e->stream>>>(key, E, lo, e->frame_first.as<u32>(), e->longest.as<u32>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h, e->longest.p, sizeof(u32), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  u32 need = 1;
  while (need < 32 && (1ull << need) < (unsigned long long)h[0]) need++;
  // the local frame 2^(32 - bits) - 1 is the dead record's: span must stay below it
  auto fits = [&](u32 b) { return b < 32 && (unsigned long long)span < (1ull << (32 - b)) - 1ull; };
  if (bits < need || !fits(bits)) {
    bits = std::max<u32>(need, 13);
    if (!fits(bits)) bits = need;
    if (!fits(bits)) {
      e->err = "a 32-bit entry id cannot hold this table's frame span and its largest frame";
      return SGTD_ERR_UNSUPPORTED;
    }
  }
  if (e->id_by_frame) {
    id_of_sorted_kernel<<<grid_for(E, 256), 256, 0, e->stream>>>(key, e->by_frame.as<u32>(), E, lo, e->frame_first.as<u32>(), bits,
                                                                 e->id_of_g.as<u32>());
    HIPCHK(hipGetLastError());
  }
  return SGTD_OK;
}

// AddSTDescs only ever appends (STDesc.cpp:149-172).  After an append to a finalized table only
// the appended entries are sorted, into the tail segment (cost proportional to the tail); the
// query sweeps both segments — inside a bucket the reference's order is insertion order, i.e.
// main entries before tail entries, and a frame's entries all live in ONE segment (the tail only
// takes frames newer than every frame of the main segment), so the per-frame match order is
// unchanged.  The tail is merged (one full build) when it outgrows an eighth of the main
// segment; force_merge asks for the single-segment form (table dump).
int do_finalize(sgtd_engine *e, bool force_merge = false) {
  if (e->finalized && !(force_merge && e->n_seg > 1)) return SGTD_OK;
  if (e->attached_to) { e->err = "the table belongs to another handle (sgtd_attach_table): only its owner rebuilds it"; return SGTD_ERR_STATE; }
  e->table_version++;
  const long long E = e->n_entries;
  if (E >= (1ll << 32) - 2 - SGTD_SENTINELS) return SGTD_ERR_UNSUPPORTED;
  const auto t0 = std::chrono::steady_clock::now();
  sgtd_engine::Segment &M = e->seg[0], &T = e->seg[1];
  const long long tail_max = e->tail_max > 0 ? (long long)e->tail_max : std::max<long long>(262144, (M.g1 - M.g0) / 8);
  u32 bits = 0;
  CHK(build_idmap(e, bits));
  // (an appended frame older than the main segment's newest, a frame that outgrew the ids' rank
  // bits, or frame ids that just went out of insertion order: everything is rebuilt)
  const bool can_tail = !force_merge && M.built && M.g0 == 0 && M.g1 > 0 && M.g1 <= E && E - M.g1 <= tail_max &&
                        bits == e->id_bits && !e->id_by_frame && (E == M.g1 || e->append_min_frame > M.frame_hi);
  e->id_bits = bits;
  if (can_tail) {
    if (E > M.g1) { CHK(build_segment(e, T, M.g1, E)); e->n_seg = 2; }
    else { T.built = false; e->n_seg = 1; }
  } else {
    CHK(build_segment(e, M, 0, E));
    T.built = false; T.g0 = T.g1 = E;
    e->n_seg = 1;
    e->append_min_frame = 0xFFFFFFFFu;
  }
  e->ms_finalize = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  e->finalized = true;
  return SGTD_OK;
}

// ---------------------------------------------------------------------------
// the query pipeline on descriptors already in e->qd (strided)
// ---------------------------------------------------------------------------
int rec_alloc(sgtd_engine *e, bool compact_lists) {
  CHK(ensure(e, e->rec, (e->rec_cap + 16) * sizeof(u32)));     // + a few quads: the list passes read four records at the last list's tail
  // (the compact candidate lists between block_count and block_write: every block reserves room for all of its records —
  // twice the record buffer; the per-query list pass needs none)
  if (compact_lists) CHK(ensure(e, e->c_pair, std::min(e->rec_cap, kIndexLimit) * sizeof(u64)));
  if (e->diag) {
    CHK(ensure(e, e->rec_cell, e->rec_cap));
    CHK(ensure(e, e->rec_dis, e->rec_cap * sizeof(double)));
  }
  CHK(ensure(e, e->pairs, e->pair_cap * sizeof(u64)));
  CHK(ensure(e, e->amb_queue, std::max<size_t>(e->amb_min, e->rec_cap / 64) * sizeof(uint2)));
  return SGTD_OK;
}

// descriptors a pass of the sweep serves (pairs / quads of neighbours share a visit list, probe_kernels.hip.h)
constexpr double kDescsPerPass = SGTD_PAIR >= 4 ? 3.2 : (SGTD_PAIR >= 2 ? 1.9 : 1.0);
// candidate pairs the pair buffer holds, as a kernel is told (grown by sync_batch while a batch is pending: never stored)
u32 pair_room(const sgtd_engine *e) { return (u32)std::min<size_t>(e->pair_cap, 0xFFFFFFF0u); }

struct Views {
  TableView T;
  QueryView Q;
  ProbeBuffers B;
  u32 span;
};

// pass 2 of the match-list assembly, both word widths of the compact lists (ahead of plan_select: the code object keeps its kernels in the order this file first names them)
int launch_block_write(sgtd_engine *e, const SelectPlan &p, const Views &v, const CompactLists &CL) {
  auto write = [&](auto kernel) {
    kernel<<<p.agrid, 256, 0, e->stream>>>(v.Q, v.B, CL, p.blocks, e->blk_count.as<u32>(), p.cn, e->pair_off.as<long long>(), e->q_pair_base.as<u32>(),
                                           e->pairs.as<u64>(), v.T.map, e->n_cand.as<int>(), e->cand_frame.as<int>());
  };
  if (p.narrow_pairs) write(&block_write_kernel<true>); else write(&block_write_kernel<false>);
  HIPCHK(hipGetLastError());
  return SGTD_OK;
}

// The batch's plan from the handle's state at enqueue: launches nothing, allocates nothing, changes nothing.  The per-batch
// experiment knobs are read here, once each.
SelectPlan plan_select(const sgtd_engine *e) {
  SelectPlan p;
  const int nq = p.nq = e->nq, cn = p.cn = e->dc.cand_num;
  const long long n_slots = p.n_slots = (long long)nq * e->q_stride;
  const u32 span = p.span = e->have_frames ? (e->frame_hi - e->frame_lo + 1) : 1;
  p.frame_lo = e->have_frames ? e->frame_lo : 0;
  p.id_bits = e->id_bits ? e->id_bits : 13;
  // descriptors per block of the block passes over the match records (one wave per block): 128 — or 64 / 32 where the batch would
  // otherwise have fewer than a thousand blocks (a one-frame batch: 57 blocks = 57 waves on 1 024 SIMDs; SGTD_BLOCK_CHUNK overrides)
  while (p.chunk > SGTD_SUB_DESCS && (long long)nq * ((e->q_stride + p.chunk - 1) / p.chunk) < 1024) p.chunk >>= 1;
  if (const char *o = getenv("SGTD_BLOCK_CHUNK")) { const int c = atoi(o); if (c == 32 || c == 64 || c == 128) p.chunk = (u32)c; }
  p.blocks = (int)((e->q_stride + p.chunk - 1) / p.chunk);
  p.groups = (p.blocks + 3) / 4;
  p.agrid = ((nq + 7) / 8) * p.groups * 8;
  // one 16-wave workgroup per (query, frame tile) when that fills the chip: the tile's LDS histogram is final (no flush
  // atomics); spans beyond LDS take several tiles of 36 Ki frames
  p.tile_span = span <= 36 * 1024 ? span : 36 * 1024;
  p.n_tiles = (span + p.tile_span - 1) / p.tile_span;
  p.hist_bytes = (size_t)span * sizeof(u32);
  p.lds_votes = p.hist_bytes <= 150 * 1024;
  // Which passes over the match records (STDesc.cpp:404-453): one workgroup per query (select_kernels.hip.h) when the batch has a
  // query for every CU — votes + top-k in one launch while the query's vote histogram fits LDS, the match lists in one launch
  // while an entry's rank among its frame's fits the image word — else the five-kernel form with one wave per 128-descriptor block.
  // (automatic choice where a query's vote histogram fits LDS: with the candidates' hash instead of the frame -> slot byte table
  // the list pass is slower than the block passes — 100 000-frame map, 256 queries: 6.1 against 2.9 ms)
  static const size_t votes_room = lds_room(&votes_topk_kernel), list_room = lds_room(&pairs_query_kernel<true>);
  p.votes_fit = votes_topk_lds_bytes(span) <= votes_room;
  // ... or at least its frame -> slot byte table beside a tile's image (one workgroup per CU then; 100 000 frames, 256 queries:
  // votes by tiles + top-k + this list pass 15.1 ms per step against 16.1 with the block passes, gpurun_out/r05o_*)
  p.table_fits = (size_t)SGTD_PQ_TILE_RECS * sizeof(u32) + (((size_t)span + 15) & ~(size_t)15) + 16 <= list_room;
  p.per_query = e->select_mode == 2 || (e->select_mode == 0 && nq >= e->n_cus && (p.votes_fit || p.table_fits));
  // (an image word of the list pass is slot(6) | descriptor(9) | rank: with 64 candidates AND ranks of the full width the
  // word of slot 63, descriptor 511, rank 2^17 - 1 would be the pass's "no record" marker — that corner takes the block form)
  p.fused_pairs = p.per_query && !e->wide_pairs && p.id_bits <= SGTD_PQ_RANK_BITS && !(cn == SGTD_MAX_CAND && p.id_bits == SGTD_PQ_RANK_BITS);
  p.fused_votes = p.fused_pairs && p.votes_fit;     // (block_count_kernel wants topk_kernel's slot table)
  p.votes_per_query = p.n_tiles == 1 ? nq >= e->n_cus : ((long long)nq * p.n_tiles >= e->n_cus / 4 && p.n_tiles <= 8);
  p.narrow_pairs = p.id_bits <= SGTD_NARROW_RANK_BITS && !e->wide_pairs;
  // bits per cell coordinate of the sort key: the largest cell a built descriptor can have
  while ((1ll << p.cbits) < (long long)(e->dc.max_len * e->dc.scale) + 3 && p.cbits < 16) p.cbits++;
  // (+ the position inside the cell, home_keys_kernel: the bits that are free below the next multiple of a sort
  // digit, or four bits and one more pass)
  const int spare = (8 - (12 + 3 * p.cbits) % 8) % 8;
  p.sub_bits = spare >= 2 ? std::min(spare, 6) : 4;
  if (const char *o = getenv("SGTD_HOME_SUB_BITS")) p.sub_bits = std::min(6, std::max(0, atoi(o)));   // experiment knob
  p.key_bits = 12 + 3 * p.cbits + p.sub_bits;
  // one frame per call: the clearing of the batch's counters and tables and the whole ordering of its descriptors in ONE
  // launch (small_order_kernel; SGTD_SMALL_ORDER=0: the general form)
  const bool small_on = [] { const char *o = getenv("SGTD_SMALL_ORDER"); return !(o && !atoi(o)); }();
  p.small = small_on && nq == 1 && n_slots <= SGTD_SMALL_SLOTS && p.key_bits <= 32 && !p.fused_votes && span <= (1u << 20);
  // the general ordering: order_kernels.hip.h's chain for 32-bit keys, the launch train for wider ones, under SGTD_ORDER_FORM=0
  // and for the re-runs of a batch whose look-back gave up.  Without the hook, a one-frame batch that small_order_kernel would
  // have taken (it is here only under SGTD_SMALL_ORDER=0) keeps the launch train: the form that kernel is compared with
  const bool small_shape = nq == 1 && n_slots <= SGTD_SMALL_SLOTS;
  p.order_fused = !p.small && (e->order_form == 1 || (e->order_form < 0 && !small_shape)) && !e->order_train && p.key_bits <= 32 && n_slots > 0 &&
                  n_slots < SGTD_ORDER_MAX_KEYS;
  p.order_tiles = (u32)((n_slots + SGTD_OS_TILE - 1) / SGTD_OS_TILE);
  p.order_gtiles = (u32)((n_slots + SGTD_GI_TILE - 1) / SGTD_GI_TILE);
  // pass slots: at most one per group and one per two descriptors (probe_kernels.hip.h)
  p.pair = !e->diag && SGTD_PAIR >= 2;
  p.max_pass_slots = (size_t)pass_slot_count((u32)n_slots, (u32)n_slots, p.pair) + 64;
  p.row_slots = e->n_seg > 1 ? 2 : 1;       // with a tail segment: its 27 rows in the second KB of the slot
  // pass slots per wave ticket: about 1.5k entry visits (neighbouring home cells then go to different waves of one XCD at
  // about the same time and find each other's buckets in its L2: at six waves per SIMD tickets of 4 / 3 / 2 pass slots
  // fetch 8.0 / 6.0 / 4.2 GB per sweep of the default batch in the same 4.8-5.0 ms; 1: 3.1 GB in 6.0 ms), from the visits per descriptor the
  // previous batch measured (2 until there is one); SGTD_SORTED_CHUNK overrides
  if (e->stats.last_D > 0 && e->stats.last_P_swept > 0) {
    // last_P_swept counts a pass's shared list once: visits per pass ~ P_swept / (D / descriptors per pass)
    const double per_pass = (double)e->stats.last_P_swept / ((double)e->stats.last_D / (p.pair ? kDescsPerPass : 1.0));
    p.ticket = (u32)std::min(8.0, std::max(1.0, std::floor(1536.0 / per_pass + 0.5)));
  }
  if (e->sorted_chunk > 0) p.ticket = (u32)std::min(SGTD_TICKET_MAX, e->sorted_chunk);
  // the sweep's grid is sized by resident waves, not by work items: every wave pulls tickets
  p.sgrid = e->n_cus * 8;
  if (const char *o = getenv("SGTD_SWEEP_BLOCKS_PER_CU")) p.sgrid = e->n_cus * std::max(1, atoi(o));   // experiment knob
  // the planner: resident workgroups (five waves per SIMD: 100 vector registers, 7 KB of staged rows per wave) x 4 rounds,
  // grid-stride over the slots
  int plan_per_cu = 20;
  if (const char *o = getenv("SGTD_PLAN_BLOCKS_PER_CU")) plan_per_cu = std::max(1, atoi(o));   // experiment knob
  p.pgrid = (int)std::min<long long>(grid_for((long long)p.max_pass_slots, SGTD_PLAN_THREADS), (long long)e->n_cus * plan_per_cu);
  // 32-bit byte offsets into the probe layout while it stays below 4 GB (record addresses are a wave-uniform base + a 32-bit lane offset either way)
  const u32 n0 = (u32)(e->seg[0].g1 - e->seg[0].g0), n1 = (u32)(e->seg[1].g1 - e->seg[1].g0);
  p.narrow = ((unsigned long long)n0 + SGTD_SENTINELS + (e->n_seg > 1 ? n1 + SGTD_SENTINELS : 0u)) * sizeof(HotEntry) < (1ull << 32);
  // can a descriptor of the batch carry a frame id the table holds?  Frames built by sgtd_query_frames are stamped with the current
  // frame id (one beyond the newest map frame in the reference's use); descriptors handed in by the caller carry whatever they carry
  p.frames = e->last_kind != 1 || (e->have_frames && e->last_qframe >= e->frame_lo && e->last_qframe <= e->frame_hi);
  return p;
}

// the kernels' views of the table, the batch's descriptors and its work buffers as they stand now, in the batch's geometry
Views make_views(sgtd_engine *e) {
  const SelectPlan &p = e->plan;
  Views v;
  v.span = p.span;
  TableView &T = v.T;
  const sgtd_engine::Segment &S = e->seg[0], &S1 = e->seg[1];
  T.ent = S.hot.as<HotEntry>(); T.map = id_map(e, p.id_bits); T.cold_side = e->tab.side.as<double>();
  T.dir = S.dir.as<BucketDir>();
  T.hash = S.hash.as<HashSlot>(); T.hash_mask = S.hash_mask;
  T.coarse_at = e->coarse_at; T.whole_at = e->whole_at;
  T.n_entries = (u32)(S.g1 - S.g0); T.frame_lo = p.frame_lo; T.frame_span = v.span;
  // the tail segment (appends after the table was finalized): its own directory and hash, its probe
  // layout behind the main segment's in the same buffer
  T.tail_off = e->n_seg > 1 ? T.n_entries + SGTD_SENTINELS : 0u;
  T.dir1 = S1.dir.as<BucketDir>(); T.hash1 = S1.hash.as<HashSlot>(); T.hash_mask1 = S1.hash_mask;
  T.n_entries1 = e->n_seg > 1 ? (u32)(S1.g1 - S1.g0) : 0u;
  QueryView &Q = v.Q;
  Q.side = e->qd.side.as<double>(); Q.qrec = e->qd.qrec.as<QueryRec>();
  Q.label = e->qd.label.as<int>(); Q.frame = e->qd.frame.as<u32>();
  Q.count = e->q_count.as<u32>(); Q.stride = e->q_stride; Q.n_queries = e->nq; Q.chunk = p.chunk;
  ProbeBuffers &B = v.B;
  B.rec_cell = e->rec_cell.as<unsigned char>(); B.rec_dis = e->rec_dis.as<double>();
  B.rec_cap = (u32)std::min<size_t>(e->rec_cap >> SGTD_REC_SHIFT, kIndexLimit);      // granules
  B.rec = e->rec.as<u32>(); B.id_bits = p.id_bits;
  B.ctr = e->cursors.as<u32>();
  // the smallest slab: the streams of all resident waves hold one each (8192 waves x SGTD_PAIR streams) — together
  // at most a quarter of the record buffer (a 33 M-record buffer of a small batch: 512-record slabs).  (A slab is one
  // atomic add to the cursor, and ONE address takes 88 M of them per second, tools/atomic_rate.hip: the 1.8 G records
  // of the default batch in slabs of 8 K are 2.4 ms of the cursor's time inside a 5 ms sweep — but slabs of 32 K or
  // 128 K run no faster, SGTD_REC_SLAB: the waves do not wait for it.)
  {
    const size_t streams = (size_t)e->n_cus * 32 * SGTD_PAIR;
    u32 slab = SGTD_REC_SLAB;
    while (slab > 512u && (size_t)slab * streams * 4 > e->rec_cap) slab >>= 1;
    if (const char *o = getenv("SGTD_REC_SLAB")) slab = (u32)std::max(512, atoi(o));   // experiment knob
    B.rec_slab = slab >> SGTD_REC_SHIFT;      // granules
  }
  // room a list gets when its pass starts (ProbeBuffers::rec_rate): three times the matches per visited entry
  // and descriptor of the batch before; a quarter of the visit list for the first batch
  {
    const double per_pass = kDescsPerPass;
    B.rec_rate = 64;
    if (e->stats.last_P_swept > 0 && e->stats.last_M > 0) {
      // three times the batch before's matches per visited entry and descriptor — but not more than lets the
      // reservations of a batch like the one before (rate / 256 of every pass's visit list per descriptor, + 256
      // records each) fit three fifths of the record buffer (slabs strand an eighth, batches differ): on maps whose visit lists match little (skewed label
      // frequencies: a twelfth of the visits) three times the rate over-reserves the 32-bit record index by itself,
      // and every batch would pay a re-run.  Never below 1.2 times the measured rate (lists that outgrow their room move).
      const double meas = 256.0 * (double)e->stats.last_M / ((double)e->stats.last_P_swept * per_pass);
      const double scale = e->stats.last_queries > 0 ? (double)e->nq / (double)e->stats.last_queries : 1.0;
      const double fit = 256.0 * (0.6 * (double)e->rec_cap - 256.0 * (double)e->stats.last_D * scale) /
                         std::max(1.0, (double)e->stats.last_P_swept * scale * per_pass);
      const double want = std::max(std::min(3.0 * meas, fit), 1.2 * meas);
      B.rec_rate = (u32)std::min(256.0, std::max(want < 16.0 && fit < 16.0 ? 2.0 : 16.0, std::ceil(want)));
    }
    B.rec_rate = std::min(B.rec_rate, e->rec_rate_cap);
    if (e->diag) B.rec_rate = 256;
    if (e->rec_rate_hook) B.rec_rate = e->rec_rate_hook;
  }
  B.amb_queue = e->amb_queue.as<uint2>();
  B.amb_cap = (u32)std::min<size_t>(e->amb_queue.bytes / sizeof(uint2), 0xFFFFFFF0u);
  B.list = e->list.as<uint2>(); B.n_visit = e->n_visit.as<u32>();
  B.votes = e->votes.as<u32>();
  return v;
}

// the match lists of every query by a workgroup of its own (select_kernels.hip.h); the slot of a record's frame
// from a byte table in LDS while the frame span fits, else from the hash of the candidates
int launch_pairs_query(sgtd_engine *e, const Views &v, const u64 *keep = nullptr) {
  const int cn = e->dc.cand_num;
  const size_t img = (size_t)SGTD_PQ_TILE_RECS * sizeof(u32);
  const size_t tab = (((size_t)v.span + 15) & ~(size_t)15) + 16;     // (+ the bytes that answer for dead records)
  // (up to 100 KB two workgroups share a CU; a span whose byte table only fits alone — 100 000 frames: 132 KB with the
  // image — still beats the candidates' hash: one workgroup per CU)
  const bool table = e->plan.table_fits;
  if (table) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&pairs_query_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(img + tab)));
  auto lists = [&](auto kernel) {
    kernel<<<e->nq, SGTD_PQ_THREADS, table ? img + tab : img, e->stream>>>(v.Q, v.B, e->n_cand.as<int>(), e->cand_frame.as<int>(), cn, e->pair_off.as<long long>(),
                                                                           e->q_pair_base.as<u32>(), e->pairs.as<u64>(), v.T.map, v.span, v.T.frame_lo, keep);
  };
  if (table) lists(&pairs_query_kernel<true>); else lists(&pairs_query_kernel<false>);
  HIPCHK(hipGetLastError());
  return SGTD_OK;
}

// the batch's local candidate tables, packed, into the buffer a multi-GPU caller registered (exchange_kernels.hip.h);
// enqueued as soon as they are final, before the match lists are written
int export_candidates(sgtd_engine *e, const Views &v) {
  if (!e->export_packed) return SGTD_OK;
  const int nq = e->nq, cn = e->dc.cand_num;
  if (xchg_packed_ints(nq, cn) > e->export_cap) {
    e->err = "the registered candidate-export buffer is too small for this batch";
    return SGTD_ERR_CAPACITY;
  }
  if (e->export_busy) {     // a side stream may still be reading the table of the batch before
    HIPCHK(hipStreamWaitEvent(e->stream, e->ev_export_free, 0));
    e->export_busy = false;
  }
  export_candidates_kernel<<<std::min(grid_for((long long)nq * cn, 256), 512), 256, 0, e->stream>>>(
      e->cand_frame.as<int>(), e->cand_votes.as<int>(), v.B.overflow(), nq, cn, ++e->batch_serial, e->export_packed);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(e->ev_cand, e->stream));
  return SGTD_OK;
}

// The match lists of a batch whose candidate tables are final, by one workgroup per query (select_kernels.hip.h):
// offsets (the prefix sums of the candidates' votes — of the candidates in `keep` only, when a mask is given), the
// queries' bases, the lists.  Runs once per batch inside launch_select, or later and repeatedly through
// sgtd_finish_lists (the records stay intact: a list pass can be repeated with another mask).
int launch_lists(sgtd_engine *e, const Views &v, const u64 *keep, bool first) {
  const int nq = e->nq, cn = e->dc.cand_num;
  if (keep) {
    cand_prefix_masked_kernel<<<grid_for(nq, 256), 256, 0, e->stream>>>(e->n_cand.as<int>(), e->cand_votes.as<int>(), keep, cn, nq,
                                                                          e->pair_off.as<long long>(), e->q_pairs.as<u32>());
    HIPCHK(hipGetLastError());
  } else if (!e->plan.fused_votes || e->lists_masked) {
    // (votes_topk_kernel leaves the unmasked offsets itself)
    cand_prefix_kernel<<<grid_for(nq, 256), 256, 0, e->stream>>>(e->n_cand.as<int>(), e->cand_votes.as<int>(), cn, nq,
                                                                   e->pair_off.as<long long>(), e->q_pairs.as<u32>());
    HIPCHK(hipGetLastError());
  }
  e->lists_masked = keep != nullptr;
  e->list_keep = keep;
  if (e->timing && first) HIPCHK(hipEventRecord(e->ev[EV_COUNT_T], e->stream));
  if (!first) HIPCHK(hipMemsetAsync(v.B.overflow() + 1, 0, sizeof(int), e->stream));
  query_base_kernel<<<1, 256, 0, e->stream>>>(e->q_pairs.as<u32>(), e->q_pair_base.as<u32>(), nq, pair_room(e), v.B.overflow());
  HIPCHK(hipGetLastError());
  if (e->timing && first) HIPCHK(hipEventRecord(e->ev[EV_SCAN], e->stream));
  CHK(launch_pairs_query(e, v, keep));
  if (e->timing && first) HIPCHK(hipEventRecord(e->ev[EV_WRITE], e->stream));
  if (first) {
    batch_totals_kernel<<<1, 1, 0, e->stream>>>(v.B.ctr, e->totals.as<unsigned long long>());
    HIPCHK(hipGetLastError());
  }
  e->lists_pending = false;
  new_results(e, false);
  e->batch_synced = false;
  return SGTD_OK;
}

// The batch's filter rows re-based to the table's frame span: bit f of device row r = frame frame_lo + f allowed, into
// `dst` (n_rows rows of ceil(span / 64) words).
int rebase_filter(sgtd_engine *e, u32 frame_lo, u32 span, int n_rows, DevBuf &dst) {
  const FrameFilter &F = *e->batch_filt;
  const size_t words = ((size_t)span + 63) / 64;
  e->filt_host.assign((size_t)n_rows * words, 0ull);
  const long long shift = (long long)frame_lo - (long long)F.lo;
  const u64 last = span % 64 ? (1ull << (span % 64)) - 1ull : ~0ull;
  for (int r = 0; r < n_rows; r++) {
    u64 *dst = e->filt_host.data() + (size_t)r * words;
    for (size_t w = 0; w < words; w++) dst[w] = row_bits_at(F.row(r), F.words, shift + (long long)w * 64);
    dst[words - 1] &= last;
  }
  CHK(ensure(e, dst, e->filt_host.size() * sizeof(u64)));
  CHK(h2d(e, dst.p, e->filt_host.data(), e->filt_host.size() * sizeof(u64)));
  return SGTD_OK;
}

// Made again only when the rows or the span change (a batch of the same filter on the same table reuses them).
int prepare_filter(sgtd_engine *e, u32 frame_lo, u32 span) {
  const FrameFilter &F = *e->batch_filt;
  if (e->filt_rows.p && F.serial == e->filt_rows_serial && frame_lo == e->filt_rows_lo && span == e->filt_rows_span) return SGTD_OK;
  CHK(rebase_filter(e, frame_lo, span, F.n_rows == 1 ? 1 : e->nq, e->filt_rows));
  e->filt_rows_serial = F.serial; e->filt_rows_lo = frame_lo; e->filt_rows_span = span;
  e->prior_rows_valid = false;      // (filt_rows no longer hold a prior's rows)
  return SGTD_OK;
}

// rows of the batch's filter pass: one for every query when every row source (filter, prior) has one, else one per query
static int batch_row_count(const sgtd_engine *e) {
  const bool per_q = (e->batch_filt && e->batch_filt->n_rows > 1) || (e->batch_prior && e->batch_prior->n_rows > 1);
  return per_q ? e->nq : 1;
}

// The batch's rows from its position prior (prior_kernels.hip.h), ANDed with its filter's when one is set, written into
// filt_rows on the device.  The span's positions are uploaded again only when the poses or the span change; the rows
// are made again only when the prior, the poses, the filter, frame_lo or the span change.
int prepare_prior(sgtd_engine *e, u32 frame_lo, u32 span) {
  const PositionPrior &P = *e->batch_prior;
  const int n_rows = batch_row_count(e);
  const sgtd_engine::PriorKey key{P.serial, e->poses_serial, e->batch_filt ? e->batch_filt->serial : 0ull, frame_lo, span, n_rows};
  if (e->filt_rows.p && e->prior_rows_valid && key == e->prior_key) return SGTD_OK;
  if (!e->pos_dev.p || e->pos_serial != e->poses_serial || e->pos_lo != frame_lo || e->pos_span != span) {
    e->pos_host.assign(span, make_float4(0.f, 0.f, 0.f, 0.f));
    const size_t n_ids = e->has_pose.size();
    for (u32 f = 0; f < span; f++) {
      const size_t id = (size_t)frame_lo + f;
      if (id >= n_ids) break;
      if (e->has_pose[id]) {
        const float *m = e->poses.data() + id * 12;
        e->pos_host[f] = make_float4(m[3], m[7], m[11], 1.f);
      }
    }
    CHK(ensure(e, e->pos_dev, (size_t)span * sizeof(float4)));
    CHK(h2d(e, e->pos_dev.p, e->pos_host.data(), (size_t)span * sizeof(float4)));
    e->pos_serial = e->poses_serial; e->pos_lo = frame_lo; e->pos_span = span;
  }
  CHK(ensure(e, e->prior_dev, P.prm.size() * sizeof(double4)));
  CHK(h2d(e, e->prior_dev.p, P.prm.data(), P.prm.size() * sizeof(double4)));
  const u64 *base = nullptr;
  int base_rows = 1;
  if (e->batch_filt) {
    const FrameFilter &F = *e->batch_filt;
    base_rows = F.n_rows == 1 ? 1 : e->nq;
    if (!e->filt_base.p || F.serial != e->filt_base_serial || frame_lo != e->filt_base_lo || span != e->filt_base_span) {
      CHK(rebase_filter(e, frame_lo, span, base_rows, e->filt_base));
      e->filt_base_serial = F.serial; e->filt_base_lo = frame_lo; e->filt_base_span = span;
    }
    base = e->filt_base.as<u64>();
  }
  const u32 words = (span + 63) / 64;
  CHK(ensure(e, e->filt_rows, (size_t)n_rows * words * sizeof(u64)));
  const long long waves = (long long)n_rows * words;
  const int grid = (int)((waves + SGTD_PRIOR_THREADS / SGTD_WAVE - 1) / (SGTD_PRIOR_THREADS / SGTD_WAVE));
  prior_rows_kernel<<<grid, SGTD_PRIOR_THREADS, 0, e->stream>>>(e->pos_dev.as<float4>(), span, words, e->prior_dev.as<double4>(),
                                                               P.n_rows == 1 ? 1 : n_rows, P.dims, base, base_rows, n_rows, e->filt_rows.as<u64>());
  HIPCHK(hipGetLastError());
  e->prior_key = key; e->prior_rows_valid = true;
  e->filt_rows_serial = 0;          // (filt_rows no longer hold a filter's own rows)
  return SGTD_OK;
}

// filter_kernels.hip.h, right after the sweep's undecided records are resolved: the records of frames a query may not
// see die (the diagnostic build: leave their lists)
int launch_filter(sgtd_engine *e, const Views &v) {
  const int nq = e->nq, n_rows = batch_row_count(e);
  const u32 words = (v.span + 63) / 64;
  // workgroups per query: one once the batch fills the chip (8 per CU), more for small batches (one frame per call:
  // its ~4 500 lists over 18 workgroups), never more than its 64-list chunks need
  const long long chunks = (e->q_stride + SGTD_WAVE - 1) / SGTD_WAVE;
  const int want = (int)std::max<long long>(1, ((long long)e->n_cus * 8 + nq - 1) / nq);
  const int wg_per_q = (int)std::max<long long>(1, std::min<long long>(want, (chunks + SGTD_FILT_WAVES - 1) / SGTD_FILT_WAVES));
  const int grid = nq * wg_per_q;
  const size_t lds = (size_t)words * sizeof(u64);
  const u64 *rows = e->filt_rows.as<u64>();
  if (e->diag) {
    if (lds <= 65536) filter_compact_kernel<true><<<grid, SGTD_FILT_THREADS, lds, e->stream>>>(v.Q, v.B, rows, n_rows, words, v.span, wg_per_q);
    else filter_compact_kernel<false><<<grid, SGTD_FILT_THREADS, 0, e->stream>>>(v.Q, v.B, rows, n_rows, words, v.span, wg_per_q);
  } else {
    if (lds <= 65536)
      filter_records_kernel<true><<<grid, SGTD_FILT_THREADS, lds, e->stream>>>(v.Q, v.B, rows, n_rows, words, v.span, wg_per_q, e->q_M.as<u32>());
    else
      filter_records_kernel<false><<<grid, SGTD_FILT_THREADS, 0, e->stream>>>(v.Q, v.B, rows, n_rows, words, v.span, wg_per_q, e->q_M.as<u32>());
  }
  HIPCHK(hipGetLastError());
  return SGTD_OK;
}

// every work buffer of the batch, its filter's or prior's rows, and the reservations that grow from batch to batch
int reserve_select(sgtd_engine *e, const SelectPlan &p) {
  const int nq = p.nq, cn = p.cn;
  const size_t slots = (size_t)std::max<long long>(p.n_slots, 1), n_slots = (size_t)p.n_slots;
  CHK(ensure(e, e->cursors, kCtrWords * sizeof(u32)));
  if (!e->totals.p) {
    CHK(ensure(e, e->totals, 4 * sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(e->totals.p, 0, 4 * sizeof(unsigned long long), e->stream));
  }
  CHK(ensure(e, e->list, slots * sizeof(uint2)));
  CHK(ensure(e, e->n_visit, slots * sizeof(u32)));
  CHK(ensure(e, e->votes, (size_t)nq * p.span * sizeof(u32)));
  CHK(ensure(e, e->slot_of, (size_t)nq * p.span + 4));      // (+ a word: small_order_kernel clears it by words)
  for (DevBuf *b : {&e->q_M, &e->q_pairs, &e->q_prefix}) CHK(ensure(e, *b, (size_t)nq * sizeof(u32)));
  CHK(ensure(e, e->q_P, (size_t)nq * sizeof(unsigned long long)));
  CHK(ensure(e, e->q_pair_base, (size_t)(nq + 1) * sizeof(u32)));
  CHK(ensure(e, e->blk_count, (size_t)nq * p.blocks * 64 * sizeof(u32)));
  CHK(ensure(e, e->c_blk, (size_t)nq * p.blocks * 2 * sizeof(u32)));
  CHK(ensure(e, e->n_cand, (size_t)nq * sizeof(int)));
  for (DevBuf *b : {&e->cand_frame, &e->cand_votes}) CHK(ensure(e, *b, (size_t)nq * cn * sizeof(int)));
  CHK(ensure(e, e->pair_off, (size_t)nq * (cn + 1) * sizeof(long long)));
  if (e->batch_prior) CHK(prepare_prior(e, p.frame_lo, p.span));
  else if (e->batch_filt) CHK(prepare_filter(e, p.frame_lo, p.span));
  CHK(rec_alloc(e, !p.fused_pairs));
  // one GroupRow (1 KB) per distinct home cell of the batch: at most one per descriptor slot, in practice a twelfth of that (0.7 M
  // cells for 9.1 M descriptors at the default batch).  Reserved: every slot for small batches, an eighth of the slots for large
  // ones — a 15-GB reservation cost the first batch 0.4 s of hipMalloc — and what a batch really needed, plus a quarter, once one
  // has overflowed it (group_resolve_kernel raises the overflow flag, sync_batch re-runs).
  if (e->group_cap_hook) { if (e->group_cap == 0) e->group_cap = e->group_cap_hook; }
  else {
    // distinct home cells of a batch: every slot's for small batches (a single frame: ~40 % of its slots), about
    // 1.5 M at most on the shipped resolution (0.39 M for 256 frames, 0.7 M for 2048), never more than half the slots
    const long long want = p.n_slots <= 65536 ? p.n_slots : std::min<long long>(p.n_slots / 2, std::max<long long>(p.n_slots / 8, 1500000));
    e->group_cap = std::max<size_t>(e->group_cap, (size_t)want);
  }
  CHK(ensure(e, e->cell_rows, std::max<size_t>(e->group_cap, 1) * SGTD_GROUP_ROW_BYTES * p.row_slots));
  // the order of the batch's descriptors by home key: sort keys and values, group ids, pass slots
  for (DevBuf *b : {&e->keyA, &e->keyB}) CHK(ensure(e, *b, n_slots * sizeof(u64)));
  for (DevBuf *b : {&e->valA, &e->valB, &e->gid, &e->group_first}) CHK(ensure(e, *b, n_slots * sizeof(u32)));
  for (DevBuf *b : {&e->n_valid, &e->n_groups}) CHK(ensure(e, *b, sizeof(u32)));
  for (DevBuf *b : {&e->pos_of_slot, &e->rec_off}) CHK(ensure(e, *b, p.max_pass_slots * sizeof(u32)));
  if (p.order_fused) CHK(ensure(e, e->order_work, order_work_words((p.key_bits + 7) / 8, p.order_tiles, p.order_gtiles) * sizeof(u32)));
  // 160 B per descriptor slot (110 used at the 10 000-frame default), 256 B for tables beyond 1e8 entries (more of
  // the 27 cells of a home cell have a bucket: 190 B used at 100 000 frames); grown on overflow
  if (e->pool_units == 0) e->pool_units = std::max<size_t>(65536, n_slots * (e->n_entries > 100000000 ? 16 : 10));
  CHK(ensure(e, e->pass_pool, (e->pool_units + SGTD_PASS_SLACK_UNITS) * sizeof(uint4)));
  return SGTD_OK;
}

// the sweep records of descriptors the caller handed in, and the general form's clearing of the batch's counters and tables
// (a one-frame batch: inside small_order_kernel)
int clear_batch(sgtd_engine *e, const SelectPlan &p) {
  const int nq = p.nq, cn = p.cn;
  if (e->thr2_pending > 0) {      // (not inside small_order_kernel: the thresholds and gate masks of 7 000 descriptors are 50 us of ONE workgroup's time, 5 us of eighteen's)
    thr2_kernel<<<grid_for(e->thr2_pending, 256), 256, 0, e->stream>>>(e->qd.side.as<double>(), e->qd.frame.as<u32>(), e->qd.qrec.as<QueryRec>(), e->thr2_pending,
                                                                        e->dc.rough);
    HIPCHK(hipGetLastError());
  }
  if (p.small) return SGTD_OK;
  HIPCHK(hipMemsetAsync(e->cursors.p, 0, kCtrWords * sizeof(u32), e->stream));
  if (!p.fused_votes) {
    if (!p.votes_per_query) HIPCHK(hipMemsetAsync(e->votes.p, 0, (size_t)nq * p.span * sizeof(u32), e->stream));   // (global vote atomics)
    HIPCHK(hipMemsetAsync(e->slot_of.p, 0xFF, (size_t)nq * p.span, e->stream));
    HIPCHK(hipMemsetAsync(e->cand_frame.p, 0xFF, (size_t)nq * cn * sizeof(int), e->stream));
    HIPCHK(hipMemsetAsync(e->cand_votes.p, 0, (size_t)nq * cn * sizeof(int), e->stream));
  }
  if (p.order_fused) return SGTD_OK;      // (q_M and q_P: order_begin_kernel)
  HIPCHK(hipMemsetAsync(e->q_M.p, 0, (size_t)nq * sizeof(u32), e->stream));
  HIPCHK(hipMemsetAsync(e->q_P.p, 0, (size_t)nq * sizeof(unsigned long long), e->stream));
  return SGTD_OK;
}

// the general ordering of a batch with 32-bit home keys in nine launches, the counters' fill included (order_kernels.hip.h): what it leaves in order, gid,
// group_first, n_groups, pos_of_slot and n_valid is what order_descriptors' launch train below leaves there
int order_fused(sgtd_engine *e, const SelectPlan &p, const Views &v, u32 **order) {
  const long long n_slots = p.n_slots;
  const int passes = (p.key_bits + 7) / 8;
  u32 *kin = e->keyA.as<u32>(), *kout = e->keyB.as<u32>(), *vin = e->valA.as<u32>(), *vout = e->valB.as<u32>();
  u32 *nv = e->n_valid.as<u32>(), *work = e->order_work.as<u32>(), *giveup = e->cursors.as<u32>() + CTR_ORDER_GIVEUP;
  order_begin_kernel<<<1, 256, 0, e->stream>>>(e->q_count.as<u32>(), e->q_prefix.as<u32>(), p.nq, nv, e->q_M.as<u32>(),
                                               e->q_P.as<unsigned long long>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(work, 0, order_work_words(passes, p.order_tiles, p.order_gtiles) * sizeof(u32), e->stream));      // tickets, histograms, every pass's state words
  home_keys_hist_kernel<<<(unsigned)std::min<long long>(grid_for(n_slots, 256), (long long)e->n_cus * 8), 256, 0, e->stream>>>(v.Q, e->q_prefix.as<u32>(), kin, vin, n_slots,
                                                                                                                              p.cbits, p.sub_bits, work + OW_HIST, e->pos_of_slot.as<u32>(), p.max_pass_slots);
  HIPCHK(hipGetLastError());
  for (int pass = 0; pass < passes; pass++) {
    order_sort_pass_kernel<<<p.order_tiles, SGTD_OS_THREADS, 0, e->stream>>>(kin, vin, kout, vout, nv, n_slots, work, p.order_tiles, pass, e->order_polls, giveup);
    HIPCHK(hipGetLastError());
    std::swap(kin, kout);
    std::swap(vin, vout);
  }
  order_groups_kernel<<<p.order_gtiles, SGTD_GI_THREADS, 0, e->stream>>>(kin, nv, e->gid.as<u32>(), e->group_first.as<u32>(), e->n_groups.as<u32>(), e->pos_of_slot.as<u32>(),
                                                                        (u32)std::min<size_t>(p.max_pass_slots, 0xFFFFFFFFu), n_slots, work + OW_GROUP_TICKET,
                                                                        reinterpret_cast<u64 *>(work + order_group_state_at(passes, p.order_tiles)), p.order_gtiles, p.cbits,
                                                                        p.sub_bits, p.pair ? 1 : 0, e->order_polls, giveup, v.B.overflow());
  HIPCHK(hipGetLastError());
  e->thr2_pending = 0; *order = vin;
  return SGTD_OK;
}

// order of the batch's descriptors by home key (label code + truncated cell): stable 8-bit radix passes over
// 12 + 3*cbits + sub_bits key bits, group heads, their scan, the groups' firsts and the pass slots — or all of it in
// small_order_kernel's one launch.  *order: the descriptor slots in that order
int order_descriptors(sgtd_engine *e, const SelectPlan &p, const Views &v, u32 **order) {
  const long long n_slots = p.n_slots;
  u32 *vin = e->valA.as<u32>(), *vout = e->valB.as<u32>(), *gid = e->gid.as<u32>();
  const u32 *nv = e->n_valid.as<u32>();
  if (p.small) {
    SmallOrder SO;
    SO.ctr = e->cursors.as<u32>(); SO.ctr_words = (u32)kCtrWords;
    SO.q_M = e->q_M.as<u32>(); SO.q_P = e->q_P.as<unsigned long long>();
    SO.votes = p.votes_per_query ? nullptr : e->votes.as<u32>(); SO.slot_of_words = e->slot_of.as<u32>(); SO.span = p.span;
    SO.cand_frame = e->cand_frame.as<int>(); SO.cand_votes = e->cand_votes.as<int>(); SO.cand_num = p.cn;
    SO.q_prefix = e->q_prefix.as<u32>(); SO.n_valid = e->n_valid.as<u32>(); SO.order = vin; SO.gid = gid;
    SO.group_first = e->group_first.as<u32>(); SO.n_groups = e->n_groups.as<u32>(); SO.pos_of_slot = e->pos_of_slot.as<u32>();
    SO.n_slots = (u32)n_slots; SO.max_pass_slots = (u32)p.max_pass_slots; SO.cbits = p.cbits; SO.sub_bits = p.sub_bits; SO.pair = p.pair ? 1 : 0; SO.key_bits = p.key_bits;
    SO.qrec = nullptr; SO.n_qrec = 0; SO.rough = e->dc.rough;
    const size_t lds = (size_t)SGTD_SMALL_SLOTS * 16;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&small_order_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   // (per device: before every launch)
    small_order_kernel<<<1, SGTD_SMALL_THREADS, lds, e->stream>>>(v.Q, SO);
    HIPCHK(hipGetLastError());
    e->thr2_pending = 0; *order = vin;
    return SGTD_OK;
  }
  if (p.order_fused) return order_fused(e, p, v, order);
  query_prefix_kernel<<<1, 256, 0, e->stream>>>(e->q_count.as<u32>(), e->q_prefix.as<u32>(), p.nq, e->n_valid.as<u32>());
  HIPCHK(hipGetLastError());
  // keys, their sort (only the n_valid compact elements are live) and the heads of the groups, in the key's width
  auto sort_by_home = [&](auto *kin, auto *kout) -> int {
    using Key = typename std::remove_pointer<decltype(kin)>::type;
    home_keys_kernel<Key><<<grid_for(n_slots, 256), 256, 0, e->stream>>>(v.Q, e->q_prefix.as<u32>(), kin, vin, n_slots, p.cbits, p.sub_bits);
    HIPCHK(hipGetLastError());
    CHK(radix_sort_pairs(e, kin, kout, vin, vout, n_slots, p.key_bits, false, nv));
    group_heads_kernel<Key><<<grid_for(n_slots, 256), 256, 0, e->stream>>>(kin, nv, gid, n_slots, p.cbits, p.sub_bits);
    HIPCHK(hipGetLastError());
    return SGTD_OK;
  };
  if (p.key_bits <= 32) CHK(sort_by_home(e->keyA.as<u32>(), e->keyB.as<u32>()));      // 32-bit keys: a third less traffic in every sort pass
  else CHK(sort_by_home(e->keyA.as<u64>(), e->keyB.as<u64>()));
  CHK(device_scan(e, gid, gid, n_slots));
  group_first_kernel<<<grid_for(n_slots, 256), 256, 0, e->stream>>>(gid, nv, e->group_first.as<u32>(), e->n_groups.as<u32>(), n_slots);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(e->pos_of_slot.p, 0xFF, p.max_pass_slots * sizeof(u32), e->stream));
  pass_slots_kernel<<<grid_for(n_slots, 256), 256, 0, e->stream>>>(gid, e->group_first.as<u32>(), nv, e->pos_of_slot.as<u32>(), n_slots, p.pair ? 1 : 0);
  HIPCHK(hipGetLastError());
  e->thr2_pending = 0; *order = vin;      // (where the sort's last pass left it)
  return SGTD_OK;
}

// one GroupRow per home cell (both segments' directory rows), the passes' visit lists from it, then ONE sweep: a pass's
// list runs through the main segment's ranges and then the tail's, cell by cell; the sweep's undecided records; the filter
int plan_and_sweep(sgtd_engine *e, const SelectPlan &p, const Views &v, u32 *vin) {
  const u32 *nv = e->n_valid.as<u32>();
  const unsigned char *rows = e->cell_rows.as<unsigned char>();
  const u32 rows_cap = (u32)std::min<size_t>(e->group_cap, 0xFFFFFFFFu);
  PassPool PP;
  PP.pool = e->pass_pool.as<uint4>(); PP.rec_off = e->rec_off.as<u32>();
  PP.cursor = v.B.pool_cursor(); PP.cap = (u32)std::min<size_t>(e->pool_units, 0xFFFFFF00u);
  group_resolve_kernel<<<e->n_cus * 16, 256, 0, e->stream>>>(v.T, v.Q, vin, e->group_first.as<u32>(),
                                                              e->n_groups.as<u32>(), nv, e->cell_rows.as<unsigned char>(), rows_cap, v.B.overflow());
  HIPCHK(hipGetLastError());
#define SGTD_LAUNCH_PLAN(PR, TL)                                                                               \
  plan_passes_kernel<PR, TL><<<p.pgrid, SGTD_PLAN_THREADS, 0, e->stream>>>(v.T, v.Q, vin, e->gid.as<u32>(), e->pos_of_slot.as<u32>(), nv, \
                                                       e->n_groups.as<u32>(), rows, rows_cap, PP, v.B.n_visit, v.B.list,          \
                                                       v.B.overflow())
  if (v.T.tail_off) { if (p.pair) SGTD_LAUNCH_PLAN(true, true); else SGTD_LAUNCH_PLAN(false, true); }
  else { if (p.pair) SGTD_LAUNCH_PLAN(true, false); else SGTD_LAUNCH_PLAN(false, false); }
#undef SGTD_LAUNCH_PLAN
  HIPCHK(hipGetLastError());
  if (e->timing) HIPCHK(hipEventRecord(e->ev[EV_SORT], e->stream));   // ms_probe = the sweep from here
  // a loop batch (sgtd_loop_frames) takes the BOUND variants: an entry counts when its frame lies below the query's bound
#define SGTD_LAUNCH_SORTED(DG, WD, FR, BD)                                                                      \
  probe_sorted_kernel<DG, WD, FR, BD><<<p.sgrid, SGTD_PROBE_THREADS, 0, e->stream>>>(                           \
      v.T, v.B, v.Q, PP, e->dc.rough, e->n_valid.as<u32>(), e->n_groups.as<u32>(), p.ticket)
  if (e->diag) {
    if (e->loop_batch) SGTD_LAUNCH_SORTED(true, true, true, true);
    else SGTD_LAUNCH_SORTED(true, true, true, false);
  } else if (e->loop_batch) {
    if (p.narrow) SGTD_LAUNCH_SORTED(false, false, true, true);
    else SGTD_LAUNCH_SORTED(false, true, true, true);
  }
  else if (p.narrow && p.frames) SGTD_LAUNCH_SORTED(false, false, true, false);
  else if (p.narrow) SGTD_LAUNCH_SORTED(false, false, false, false);
  else if (p.frames) SGTD_LAUNCH_SORTED(false, true, true, false);
  else SGTD_LAUNCH_SORTED(false, true, false, false);
#undef SGTD_LAUNCH_SORTED
  HIPCHK(hipGetLastError());
  resolve_undecided_kernel<<<64, 256, 0, e->stream>>>(v.T, v.Q, v.B, e->q_M.as<u32>());
  HIPCHK(hipGetLastError());
  if (e->batch_filt || e->batch_prior) CHK(launch_filter(e, v));
#ifdef SGTD_EXP_PHASE
  {
    static int pcalls = 0;
    if (++pcalls == 6) {
      HIPCHK(hipStreamSynchronize(e->stream));
      unsigned long long ph[8];
      HIPCHK(hipMemcpyFromSymbol(ph, HIP_SYMBOL(g_phase), sizeof(ph)));
      const double tot = (double)ph[7];
      fprintf(stderr, "PHASE (fractions of wave life, %llu waves): prologue %.3f locate+issue %.3f wait-loads %.3f test %.3f epilogue %.3f between-passes %.3f rest %.3f\n",
              ph[6], ph[0] / tot, ph[1] / tot, ph[2] / tot, ph[3] / tot, ph[4] / tot, ph[5] / tot,
              (tot - ph[0] - ph[1] - ph[2] - ph[3] - ph[4] - ph[5]) / tot);
    }
  }
#endif
  if (e->timing) HIPCHK(hipEventRecord(e->ev[EV_PROBE], e->stream));
  return SGTD_OK;
}

// the votes of every query's records, in the plan's form: with top-k in one launch per query, per (query, frame tile),
// or by blocks into an LDS or a global histogram
int launch_votes(sgtd_engine *e, const SelectPlan &p, const Views &v) {
  u32 *q_M = e->q_M.as<u32>();
  unsigned long long *q_P = e->q_P.as<unsigned long long>();
  if (p.fused_votes) {
    const size_t lds = votes_topk_lds_bytes(p.span);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&votes_topk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    votes_topk_kernel<<<p.nq, SGTD_VT_THREADS, lds, e->stream>>>(v.Q, v.B, p.span, v.T.frame_lo, p.blocks, p.cn, q_M, q_P, e->n_cand.as<int>(),
                                                                  e->cand_frame.as<int>(), e->cand_votes.as<int>(), e->pair_off.as<long long>(),
                                                                  e->q_pairs.as<u32>());
  } else if (p.votes_per_query) {
    const size_t tile_bytes = (size_t)p.tile_span * sizeof(u32);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&votes_query_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_bytes));
    votes_query_kernel<<<p.nq * (int)p.n_tiles, SGTD_VOTES_Q_THREADS, tile_bytes, e->stream>>>(v.Q, v.B, p.span, v.T.frame_lo, p.tile_span, p.blocks, q_M, q_P);
  } else if (p.lds_votes) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&votes_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.hist_bytes));
    votes_kernel<true><<<p.agrid, 256, p.hist_bytes, e->stream>>>(v.Q, v.B, p.span, v.T.frame_lo, p.blocks, q_M, q_P);
  } else {
    votes_kernel<false><<<p.agrid, 256, 0, e->stream>>>(v.Q, v.B, p.span, v.T.frame_lo, p.blocks, q_M, q_P);
  }
  HIPCHK(hipGetLastError());
  if (e->timing) HIPCHK(hipEventRecord(e->ev[EV_VOTES], e->stream));
  return SGTD_OK;
}

int launch_topk(sgtd_engine *e, const SelectPlan &p, const Views &v) {
  if (!p.fused_votes) {
    topk_kernel<<<p.nq, SGTD_TOPK_THREADS, 0, e->stream>>>(e->votes.as<u32>(), p.span, v.T.frame_lo, p.cn, e->n_cand.as<int>(),
                                                            e->cand_frame.as<int>(), e->cand_votes.as<int>(), e->slot_of.as<unsigned char>());
    HIPCHK(hipGetLastError());
  }
  if (e->timing) HIPCHK(hipEventRecord(e->ev[EV_TOPK], e->stream));
  return SGTD_OK;
}

// the compact candidate lists between block_count_kernel and block_write_kernel, in the batch's geometry
CompactLists compact_lists(sgtd_engine *e, const SelectPlan &p, const Views &v) {
  CompactLists CL;
  CL.pair = e->c_pair.as<u64>();
  CL.blk_start = e->c_blk.as<u32>(); CL.blk_n = e->c_blk.as<u32>() + (size_t)p.nq * p.blocks;
  CL.cursor = v.B.compact_cursor(); CL.cap = (u32)std::min<size_t>(e->c_pair.bytes / sizeof(u64), 0xFFFFFFF0u);
  return CL;
}

// the match lists by the block passes: count (into the compact lists), scan, write
int launch_block_lists(sgtd_engine *e, const SelectPlan &p, const Views &v) {
  const int nq = p.nq;
  const CompactLists CL = compact_lists(e, p, v);
  // the frame -> slot byte table in LDS while the span fits
  const int sl_bytes = p.span <= 48 * 1024 ? (int)((p.span + 15) & ~15u) : 0;
  auto count = [&](auto kernel) -> int {
    if (sl_bytes) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, sl_bytes));
    kernel<<<p.agrid, 256, sl_bytes, e->stream>>>(v.Q, v.B, e->n_cand.as<int>(), e->cand_frame.as<int>(), p.cn, p.blocks, e->blk_count.as<u32>(), CL,
                                                  nullptr, nullptr, e->slot_of.as<unsigned char>(), p.span, v.T.frame_lo);
    HIPCHK(hipGetLastError());
    return SGTD_OK;
  };
  if (sl_bytes) CHK(p.narrow_pairs ? count(&block_count_kernel<true, true>) : count(&block_count_kernel<true, false>));
  else CHK(p.narrow_pairs ? count(&block_count_kernel<false, true>) : count(&block_count_kernel<false, false>));
  if (e->timing) HIPCHK(hipEventRecord(e->ev[EV_COUNT_T], e->stream));
  // (a one-query batch: the scan leaves the query's base and the batch's totals itself)
  block_scan_kernel<<<nq, 64, 0, e->stream>>>(e->blk_count.as<u32>(), p.blocks, p.cn, e->n_cand.as<int>(),
                                               e->pair_off.as<long long>(), e->q_pairs.as<u32>(),
                                               v.B.overflow(), nq == 1 ? e->q_pair_base.as<u32>() : nullptr, pair_room(e),
                                               nq == 1 ? e->totals.as<unsigned long long>() : nullptr);
  HIPCHK(hipGetLastError());
  if (nq != 1) {
    query_base_kernel<<<1, 256, 0, e->stream>>>(e->q_pairs.as<u32>(), e->q_pair_base.as<u32>(), nq, pair_room(e), v.B.overflow());
    HIPCHK(hipGetLastError());
  }
  if (e->timing) HIPCHK(hipEventRecord(e->ev[EV_SCAN], e->stream));
  CHK(launch_block_write(e, p, v, CL));
  if (e->timing) HIPCHK(hipEventRecord(e->ev[EV_WRITE], e->stream));
  if (nq != 1) {
    batch_totals_kernel<<<1, 1, 0, e->stream>>>(v.B.ctr, e->totals.as<unsigned long long>());
    HIPCHK(hipGetLastError());
  }
  e->batch_valid = true;
  new_results(e, false);
  e->batch_synced = false;
  return SGTD_OK;
}

// The engine's whole query pipeline behind descriptor construction, on the descriptors in e->qd: the batch's plan, then
// its stages in order.
int launch_select(sgtd_engine *e) {
  e->plan = plan_select(e);
  const SelectPlan &p = e->plan;
  CHK(reserve_select(e, p));
  CHK(clear_batch(e, p));
  const Views v = make_views(e);
  u32 *order = nullptr;
  CHK(order_descriptors(e, p, v, &order));
  CHK(plan_and_sweep(e, p, v, order));
  CHK(launch_votes(e, p, v));
  CHK(launch_topk(e, p, v));
  CHK(export_candidates(e, v));      // (multi-GPU step: the local tables start travelling before the lists are written)
  e->lists_pending = false;
  e->lists_masked = false;
  e->stats.select_form = p.fused_votes ? 2 : (p.fused_pairs ? 1 : 0);
  if (!p.fused_pairs) return launch_block_lists(e, p, v);
  // the lists' offsets are the prefix sums of the candidates' votes; the lists themselves by one workgroup per query
  e->batch_valid = true;
  if (!e->defer_lists) return launch_lists(e, v, nullptr, /*first=*/true);
  // the caller writes the lists itself once it knows which candidates survive the merge (sgtd_finish_lists)
  if (e->timing)
    for (int k : {EV_COUNT_T, EV_SCAN, EV_WRITE}) HIPCHK(hipEventRecord(e->ev[k], e->stream));
  batch_totals_kernel<<<1, 1, 0, e->stream>>>(v.B.ctr, e->totals.as<unsigned long long>());
  HIPCHK(hipGetLastError());
  e->lists_pending = true;
  new_results(e, false);
  e->batch_synced = false;
  return SGTD_OK;
}

int enqueue_frames(sgtd_engine *e) {
  // (re)runs the last frames batch: build on device, then select
  const int nq = e->nq;
  if (e->timing) HIPCHK(hipEventRecord(e->ev[EV_START], e->stream));
  CHK(launch_build(e, e->last_xyz, e->last_label, e->kp_off_dev.as<long long>(), nq, e->last_max_n,
                   e->last_qframe, e->loop_batch ? 1 : 0, e->qd.view(), e->q_stride, e->q_count.as<u32>()));
  if (e->loop_batch) {
    loop_bound_kernel<<<grid_for(e->q_stride * nq, 256), 256, 0, e->stream>>>(e->qd.qrec.as<QueryRec>(), e->q_stride, nq, e->last_qframe,
                                                                             e->loop_skip, e->have_frames ? e->frame_lo : 0);
    HIPCHK(hipGetLastError());
  }
  if (e->timing) HIPCHK(hipEventRecord(e->ev[EV_BUILD], e->stream));
  return launch_select(e);
}

int rerun(sgtd_engine *e) {
  e->order_train = e->order_gave_up;      // (read by plan_select)
  int st = SGTD_OK;
  if (e->last_kind == 1) st = enqueue_frames(e);
  else if (e->timing && hipEventRecord(e->ev[EV_START], e->stream) != hipSuccess) st = SGTD_ERR_HIP;
  else st = launch_select(e);
  e->order_train = false;
  return st;
}

// the candidate-pair buffer was too small: everything up to the per-block counts is intact,
// only the output offsets and the write pass run again
int rerun_write(sgtd_engine *e) {
  const SelectPlan &p = e->plan;
  CHK(ensure(e, e->pairs, e->pair_cap * sizeof(u64)));
  const Views v = make_views(e);
  HIPCHK(hipMemsetAsync(v.B.overflow() + 1, 0, sizeof(int), e->stream));
  if (p.fused_pairs) return launch_lists(e, v, e->lists_masked ? e->list_keep : nullptr, /*first=*/false);
  query_base_kernel<<<1, 256, 0, e->stream>>>(e->q_pairs.as<u32>(), e->q_pair_base.as<u32>(), p.nq, pair_room(e), v.B.overflow());
  HIPCHK(hipGetLastError());
  return launch_block_write(e, p, v, compact_lists(e, p, v));
}

// A handle attached to another one's table (sgtd_attach_table) holds that table's device pointers.  Whatever changes the
// owner's table — an add, a load, a finalize that rebuilds or merges a segment (its own fifth batch on a tail does) — may
// have freed them: every call of the view that would touch the table again (a batch's re-run, the verification, gathers of
// entries) asks here first.  (Work the view had already enqueued is safe: hipFree waits for the device.)
int view_current(sgtd_engine *e) {
  if (!e->attached_to) return SGTD_OK;
  if (e->attached_to->table_version != e->attached_version || !e->attached_to->finalized) {
    e->err = "the owner's table changed since sgtd_attach_table: attach again";
    e->batch_valid = false;
    return SGTD_ERR_STATE;
  }
  return SGTD_OK;
}

// the batch's stage times from its events (the batch has been waited for)
void stage_times(sgtd_engine *e) {
  if (!e->timing) return;
  sgtd_stats &s = e->stats;
  auto el = [&](int a, int b) { float ms = 0; (void)hipEventElapsedTime(&ms, e->ev[a], e->ev[b]); return ms; };
  if (e->last_kind == 1) { s.ms_build = el(EV_START, EV_BUILD); s.ms_sort = el(EV_BUILD, EV_SORT); }
  else { s.ms_build = 0; s.ms_sort = el(EV_START, EV_SORT); }
  s.ms_probe = el(EV_SORT, EV_PROBE); s.ms_votes = el(EV_PROBE, EV_VOTES);
  s.ms_topk = el(EV_VOTES, EV_TOPK); s.ms_count = el(EV_TOPK, EV_COUNT_T);
  s.ms_scan = el(EV_COUNT_T, EV_SCAN); s.ms_write = el(EV_SCAN, EV_WRITE);
  s.ms_total = el(EV_START, EV_WRITE);
}

int sync_batch(sgtd_engine *e) {
  PinScope pin_scope(e);
  if (!e->batch_valid) return SGTD_ERR_STATE;
  CHK(view_current(e));
  if (e->batch_synced) return SGTD_OK;
  e->stats.overflowed = 0;
  e->order_gave_up = false;
  unsigned long long swept = 0;
  for (int attempt = 0; attempt < 12; attempt++) {
    int ovf[2] = {0, 0};
    unsigned long long cursor = 0, need = 0;
    swept = 0;
    u32 total = 0, pool_used = 0;
    u32 ctr[CTR_COUNT];     // ProbeBuffers::ctr, one copy
    u32 n_groups = 0;
    unsigned long long tot[3] = {0, 0, 0};
    // (deferred lists that nobody finished, or a re-run that changed the candidates: the lists of all of them)
    if (e->lists_pending) CHK(launch_lists(e, make_views(e), nullptr, /*first=*/false));
    CHK(d2h(e, ctr, e->cursors.p, sizeof(ctr)));
    if (e->totals.p) CHK(d2h(e, tot, e->totals.p, sizeof(tot)));
    if (e->n_groups.p) CHK(d2h(e, &n_groups, e->n_groups.p, sizeof(u32)));
    CHK(d2h(e, &total, e->q_pair_base.as<u32>() + e->nq, sizeof(u32)));
    CHK(xfer_sync(e));
    std::memcpy(&cursor, ctr + CTR_REC_CURSOR, 8); std::memcpy(&need, ctr + CTR_REC_NEED, 8); std::memcpy(&swept, ctr + CTR_SWEPT, 8);
    cursor <<= SGTD_REC_SHIFT;          // (the device counts granules of four records)
    pool_used = ctr[CTR_POOL_CURSOR]; ovf[0] = (int)ctr[CTR_OVERFLOW]; ovf[1] = (int)ctr[CTR_OVERFLOW + 1];
    e->stats.last_list_moves = ctr[CTR_LIST_MOVES];
    e->stats.batches_total = (int64_t)tot[0]; e->stats.overflow_launches_total = (int64_t)tot[1]; e->stats.list_moves_total = (int64_t)tot[2];
    if (!ovf[0] && !ovf[1]) {
      // slab use varies a little from run to run (which wave sweeps what): when a batch comes within
      // a tenth of the capacity, make room for half as much again (reallocated at the next launch)
      const size_t lim0 = kRecLimit;
      if ((double)cursor * 1.1 > (double)e->rec_cap) e->rec_cap = std::min<size_t>(lim0, (size_t)((double)cursor * 1.5));
      break;
    }
    e->stats.overflowed = 1;
    if (ovf[0]) e->stats.reruns_total++; else e->stats.rewrites_total++;
    if (getenv("SGTD_DEBUG"))
      fprintf(stderr, "sgtd: batch re-run (attempt %d): flags %d %d, records %llu of %zu (+%llu wanted), pass pool %u of %zu units, home cells %u of %zu rows, pairs %u of %zu\n",
              attempt, ovf[0], ovf[1], cursor, e->rec_cap, need, pool_used, e->pool_units, n_groups, e->group_cap, total, e->pair_cap);
    if (attempt == 11) return SGTD_ERR_CAPACITY;
    if (ovf[0] && e->plan.order_fused) {
      // a look-back of the ordering gave up (order_kernels.hip.h): nothing was too small — the batch runs again with the launch train
      u32 gave_up = 0;
      CHK(d2h(e, &gave_up, e->cursors.as<u32>() + CTR_ORDER_GIVEUP, sizeof(u32)));
      CHK(xfer_sync(e));
      if (gave_up) {
        e->stats.order_giveups_total++;
        e->order_gave_up = true;
        CHK(rerun(e));
        continue;
      }
    }
    // grow towards the index limits; a batch that does not fit even there must be split
    const size_t lim = kRecLimit, pair_lim = kIndexLimit;
    if (ovf[0] && (size_t)n_groups > e->group_cap) {
      // more distinct home cells than GroupRows were reserved
      e->group_cap = (size_t)n_groups + (size_t)n_groups / 4 + 1024;
    } else if (ovf[0] && (size_t)pool_used > e->pool_units) {
      // the pass records did not fit (the cursor kept counting: pool_used is what the batch needs)
      if (e->pool_units >= 0xFFFFFF00ull) return SGTD_ERR_CAPACITY;
      e->pool_units = std::min<size_t>(0xFFFFFF00ull, (size_t)pool_used + (size_t)pool_used / 4 + 65536);
    } else if (ovf[0]) {
      // The cursor counts the room the lists RESERVED (rec_rate / 256 of every visit list), `need` the matches that
      // found none.  Reservations far beyond the buffer with few matches left over: the rate is too generous for
      // this table (a first batch on long buckets that match little: skewed label frequencies) — a list that
      // outgrows its room moves, so the rate can drop safely; only when it is at its floor is the batch too large.
      const bool reservations = (double)cursor > 1.5 * (double)e->rec_cap + 4.0 * (double)need;
      if (reservations && e->rec_rate_cap > 2) {
        e->rec_rate_cap = std::max<u32>(2, std::min<u32>(e->rec_rate_cap, 64) / 4);
      } else if (e->rec_cap >= lim) {
        return SGTD_ERR_CAPACITY;
      }
      // what was stored fits rec_cap, `need` matches did not; slabs leave about an eighth unused,
      // every wave strands part of its last slab
      const size_t want = (size_t)((double)(e->rec_cap + need) * 1.4) + (size_t)e->n_cus * 32 * SGTD_PAIR * 512;
      e->rec_cap = std::min<size_t>(lim, std::max<size_t>(reservations ? e->rec_cap : e->rec_cap * 2, want));
    } else if (ovf[1]) {
      if (e->pair_cap >= pair_lim) return SGTD_ERR_CAPACITY;
      e->pair_cap = std::min<size_t>(pair_lim, std::max<size_t>(e->pair_cap * 2, (size_t)total + (total >> 3) + 65536));
      CHK(rerun_write(e));
      continue;
    }
    CHK(rerun(e));
  }
  const int nq = e->nq, cn = e->dc.cand_num;
  if (!(e->h_count.resize(nq) && e->h_pair_base.resize(nq + 1) && e->h_q_M.resize(nq) && e->h_q_P.resize(nq) &&
        e->h_n_cand.resize(nq) && e->h_cand_frame.resize((size_t)nq * cn) && e->h_cand_votes.resize((size_t)nq * cn) &&
        e->h_pair_off.resize((size_t)nq * (cn + 1)))) {
    e->err = "hipHostMalloc of the result tables failed";
    return SGTD_ERR_HIP;
  }
  // the batch's result tables: eight direct DMA transfers into page-locked arrays the handle keeps
  auto pull = [&](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream) : hipSuccess; };
  HIPCHK(pull(e->h_count.data(), e->q_count.p, nq * sizeof(u32)));
  HIPCHK(pull(e->h_pair_base.data(), e->q_pair_base.p, (nq + 1) * sizeof(u32)));
  HIPCHK(pull(e->h_q_M.data(), e->q_M.p, nq * sizeof(u32)));
  HIPCHK(pull(e->h_q_P.data(), e->q_P.p, nq * sizeof(unsigned long long)));
  HIPCHK(pull(e->h_n_cand.data(), e->n_cand.p, nq * sizeof(int)));
  HIPCHK(pull(e->h_cand_frame.data(), e->cand_frame.p, (size_t)nq * cn * sizeof(int)));
  HIPCHK(pull(e->h_cand_votes.data(), e->cand_votes.p, (size_t)nq * cn * sizeof(int)));
  HIPCHK(pull(e->h_pair_off.data(), e->pair_off.p, (size_t)nq * (cn + 1) * sizeof(long long)));
  CHK(xfer_sync(e));
  sgtd_stats &s = e->stats;
  s.last_queries = nq;
  s.last_D = 0; s.last_P = 0; s.last_M = 0; s.last_cand_pairs = 0;
  s.last_P_swept = (int64_t)swept;
  for (int q = 0; q < nq; q++) {
    s.last_D += e->h_count[q];
    s.last_P += (int64_t)e->h_q_P[q];
    s.last_M += e->h_q_M[q];
    s.last_cand_pairs += e->h_pair_off[(size_t)q * (cn + 1) + cn];
  }
  stage_times(e);
  e->batch_synced = true;
  return SGTD_OK;
}

// A pending query batch keeps its inputs in the handle's staging buffers for a re-run after a
// work-buffer overflow: anything that is about to reuse them settles the batch first.
// Expected rough matches of one query frame of n_keypoints keypoints, before any batch has been
// measured.  A query descriptor distributed like the table's entries meets buckets of
// L = sum(len^2) / E entries on average; its matches are the entries inside its threshold ball:
// about 0.55 L for the shipped rough_dis_threshold 0.03 (ball of ~0.5 m in cells of 1 m^3; the
// ball's volume grows with the cube of the threshold) plus the re-observations of the same
// place, ~65 per descriptor on the synthetic maps (measured 73 / 166 matches per descriptor at
// 1 k / 10 k frames: the estimate gives 77 / 185).  About 62 % of the 36 n_keypoints triplets
// survive the length filter and the dedup.
double est_matches_per_query(const sgtd_engine *e, int n_keypoints) {
  if (e->stats.last_queries > 0 && e->stats.last_D > 0 && e->nq > 0 && e->q_stride > 0) {
    // measured: matches per descriptor slot of the last batch, scaled to this frame size
    const double per_slot = (double)e->stats.last_M / ((double)e->stats.last_queries * (double)e->q_stride);
    return per_slot * (double)n_keypoints * e->dc.tpi;
  }
  if (e->n_entries <= 0) return 0.0;
  const double L = (e->seg[0].sum_len_sq + (e->n_seg > 1 ? e->seg[1].sum_len_sq : 0.0)) / (double)e->n_entries;
  const double r = e->dc.rough / 0.03;
  const double per_desc = 0.55 * L * std::min(27.0, r * r * r) + 65.0;
  return 0.62 * (double)n_keypoints * e->dc.tpi * per_desc;
}

int settle_pending(sgtd_engine *e) {
  if (e->batch_valid && !e->batch_synced) return sync_batch(e);
  return SGTD_OK;
}

// A tail segment makes every visit list run through two sets of buckets (+11 % step time).  While appends
// keep arriving that is the cheap side of the trade (each append sorts only the tail); once
// SGTD_TAIL_BATCHES batches in a row have used the same tail the next one merges it into the main segment
// (one full build, ~0.25 ms per million entries).
#define SGTD_TAIL_BATCHES 4
int settle_tail(sgtd_engine *e) {
  if (e->attached_to) return view_current(e);
  if (e->finalized && e->n_seg == 2) {
    if (e->tail_batches >= SGTD_TAIL_BATCHES) { e->tail_batches = 0; return do_finalize(e, /*force_merge=*/true); }
    e->tail_batches++;
  } else {
    e->tail_batches = 1;    // no tail, or an append since the last batch (do_finalize rebuilds the tail): its first batch
  }
  return do_finalize(e);
}

// sgtd_remove_frames on one device: the entries whose frame has its bit set in `bits` (bit f - frame_lo over the table's
// frame span) leave the cold store and the survivors keep their order (remove_kernels.hip.h).  No second copy of the
// store: each field is compacted into a scratch buffer of the survivors' size, which then replaces the field's buffer,
// and the old buffer is freed before the next field — the extra memory peaks at 36 B per surviving entry (the vertex
// field, done first while the freed memory can only grow), and the table ends in buffers sized to the survivors.
// (Handing each freed buffer on as the next, narrower field's scratch saves the allocations — 4.4 against 6.5 ms on
// a 44 M-entry table — but keeps each field in a buffer sized for a wider one: 28 B more per entry for good.)  The probe
// layout is not touched here: the next finalize builds it over the whole table, as for a table just loaded.
// *n_removed: the entries removed (0: nothing changed).
int remove_entries(sgtd_engine *e, const std::vector<u32> &bits, u32 span, int64_t *n_removed) {
  *n_removed = 0;
  const long long E = e->n_entries;
  const u32 lo = e->frame_lo, words = (u32)(((u64)span + 31) / 32);
  const long long n_tiles = (E + SGTD_RM_TILE - 1) / SGTD_RM_TILE;
  CHK(ensure(e, e->rm_bits, (size_t)words * sizeof(u32)));
  CHK(ensure(e, e->rm_present, (size_t)words * sizeof(u32)));
  CHK(ensure(e, e->rm_mask, (size_t)n_tiles * SGTD_RM_MASKS * sizeof(u64)));
  CHK(ensure(e, e->rm_count, (size_t)n_tiles * sizeof(u32)));
  HIPCHK(hipMemcpyAsync(e->rm_bits.p, bits.data(), (size_t)words * sizeof(u32), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemsetAsync(e->rm_present.p, 0, (size_t)words * sizeof(u32), e->stream));
  // pass 1: the keep masks and survivors per tile; each workgroup copies the removed set into its LDS once and walks
  // tiles grid-stride (a set beyond 64 KB, 2^19 frames, is read from memory instead)
  const int grid = (int)std::min<long long>(n_tiles, (long long)e->n_cus * 4);
  const size_t lds = (size_t)words * sizeof(u32);
  if (lds <= 65536) {
    remove_flag_kernel<true><<<grid, SGTD_RM_THREADS, lds, e->stream>>>(e->tab.frame.as<u32>(), E, e->rm_bits.as<u32>(), lo, span,
                                                                      e->rm_mask.as<u64>(), e->rm_count.as<u32>(), e->rm_present.as<u32>());
  } else {
    remove_flag_kernel<false><<<grid, SGTD_RM_THREADS, 0, e->stream>>>(e->tab.frame.as<u32>(), E, e->rm_bits.as<u32>(), lo, span,
                                                                     e->rm_mask.as<u64>(), e->rm_count.as<u32>(), e->rm_present.as<u32>());
  }
  HIPCHK(hipGetLastError());
  u32 last_cnt = 0, last_off = 0;
  std::vector<u32> present(words);
  HIPCHK(hipMemcpyAsync(&last_cnt, e->rm_count.as<u32>() + (n_tiles - 1), sizeof(u32), hipMemcpyDeviceToHost, e->stream));
  CHK(device_scan(e, e->rm_count.as<u32>(), e->rm_count.as<u32>(), n_tiles));     // the tiles' output offsets
  HIPCHK(hipMemcpyAsync(&last_off, e->rm_count.as<u32>() + (n_tiles - 1), sizeof(u32), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(present.data(), e->rm_present.p, (size_t)words * sizeof(u32), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  const long long kept = (long long)last_off + last_cnt;
  if (kept == E) {      // the named frames have no entries
    free_buf(e->rm_mask);
    free_buf(e->rm_count);
    return SGTD_OK;
  }
  // pass 2, field by field (W: 32-bit words per entry)
  if (kept > 0) {
    struct Field { DevBuf *buf; int w; };
    const Field fields[7] = {{&e->tab.vertex, 9}, {&e->tab.side, 6}, {&e->tab.angle, 6}, {&e->tab.center, 6},
                             {&e->tab.label, 3}, {&e->tab.node_id, 3}, {&e->tab.frame, 1}};
    for (const Field &f : fields) {
      CHK(ensure(e, e->rm_scratch, (size_t)kept * f.w * sizeof(u32)));
      const u32 *src = f.buf->as<u32>();
      u32 *dst = e->rm_scratch.as<u32>();
      const u64 *mask = e->rm_mask.as<u64>();
      const u32 *off = e->rm_count.as<u32>();
      const int tiles = (int)n_tiles;
      switch (f.w) {
        case 9: remove_compact_kernel<9><<<tiles, SGTD_RM_THREADS, 0, e->stream>>>(src, dst, E, mask, off); break;
        case 6: remove_compact_kernel<6><<<tiles, SGTD_RM_THREADS, 0, e->stream>>>(src, dst, E, mask, off); break;
        case 3: remove_compact_kernel<3><<<tiles, SGTD_RM_THREADS, 0, e->stream>>>(src, dst, E, mask, off); break;
        default: remove_compact_kernel<1><<<tiles, SGTD_RM_THREADS, 0, e->stream>>>(src, dst, E, mask, off); break;
      }
      HIPCHK(hipGetLastError());
      std::swap(*f.buf, e->rm_scratch);
      free_buf(e->rm_scratch);      // the field's old buffer (hipFree waits for the kernel)
    }
    size_t cap = SIZE_MAX;
    for (const Field &f : fields) cap = std::min(cap, f.buf->bytes / ((size_t)f.w * sizeof(u32)));
    e->tab.cap = cap;
  }
  // the survivors' frame range, and one AddSTDescs call fewer for every removed frame that had entries
  long long gone_frames = 0;
  long long first = -1, last = -1;
  for (u32 w = 0; w < words; w++) {
    gone_frames += __builtin_popcount(present[w] & bits[w]);
    const u32 stay = present[w] & ~bits[w];
    if (stay) {
      if (first < 0) first = (long long)w * 32 + __builtin_ctz(stay);
      last = (long long)w * 32 + 31 - __builtin_clz(stay);
    }
  }
  free_buf(e->rm_mask);      // (an eighth of a byte per entry: not kept for a call that is rare)
  free_buf(e->rm_count);
  *n_removed = E - kept;
  e->n_entries = kept;
  e->n_add_calls = std::max<int64_t>(0, e->n_add_calls - gone_frames);
  e->have_frames = kept > 0;
  e->frame_lo = kept > 0 ? lo + (u32)first : 0;
  e->frame_hi = kept > 0 ? lo + (u32)last : 0;
  // the probe layout of the old table is gone: the next finalize builds one segment and the entry ids afresh
  for (sgtd_engine::Segment &S : e->seg) { S.built = false; S.n_buckets = 0; S.sum_len_sq = 0.0; S.g0 = S.g1 = 0; }
  e->n_seg = 1;
  e->append_min_frame = 0xFFFFFFFFu;
  e->id_bits = 0;
  e->tail_batches = 0;
  e->finalized = false;
  e->batch_valid = false;
  e->table_version++;
  return SGTD_OK;
}

int check_cfg(const sgtd_config *c) {
  if (c->descriptor_near_num < 3 || c->descriptor_near_num > SGTD_MAX_K) return SGTD_ERR_UNSUPPORTED;
  if (c->candidate_num < 1 || c->candidate_num > SGTD_MAX_CAND) return SGTD_ERR_UNSUPPORTED;
  if (c->max_frame_n < 1) return SGTD_ERR_INVALID;
  if (!(c->std_side_resolution > 0) || !(c->descriptor_max_len > 0)) return SGTD_ERR_INVALID;
  if (!(c->descriptor_max_len * 1000.0 < 2097151.0)) return SGTD_ERR_UNSUPPORTED;
  if (!(c->descriptor_max_len / c->std_side_resolution + 2.0 < 65535.0)) return SGTD_ERR_UNSUPPORTED;
  return SGTD_OK;
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
namespace {
// one SoA field <-> file, staged through a bounded host buffer
template <class T>
int stream_field(sgtd_engine *e, FILE *f, T *dev, size_t n_items, bool to_file, std::vector<char> &stage) {
  const size_t chunk = stage.size() / sizeof(T);
  for (size_t o = 0; o < n_items; o += chunk) {
    const size_t m = std::min(chunk, n_items - o);
    if (to_file) {
      HIPCHK(hipMemcpyAsync(stage.data(), dev + o, m * sizeof(T), hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      if (fwrite(stage.data(), sizeof(T), m, f) != m) return SGTD_ERR_IO;
    } else {
      if (fread(stage.data(), sizeof(T), m, f) != m) return SGTD_ERR_IO;
      HIPCHK(hipMemcpyAsync(dev + o, stage.data(), m * sizeof(T), hipMemcpyHostToDevice, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
    }
  }
  return SGTD_OK;
}
int stream_table(sgtd_engine *e, FILE *f, size_t n, bool to_file) {
  std::vector<char> stage((size_t)64 << 20);
  CHK(stream_field(e, f, e->tab.side.as<double>(), n * 3, to_file, stage));
  CHK(stream_field(e, f, e->tab.angle.as<double>(), n * 3, to_file, stage));
  CHK(stream_field(e, f, e->tab.center.as<double>(), n * 3, to_file, stage));
  CHK(stream_field(e, f, e->tab.vertex.as<float>(), n * 9, to_file, stage));
  CHK(stream_field(e, f, e->tab.label.as<int>(), n * 3, to_file, stage));
  CHK(stream_field(e, f, e->tab.frame.as<u32>(), n, to_file, stage));
  CHK(stream_field(e, f, e->tab.node_id.as<int>(), n * 3, to_file, stage));
  return SGTD_OK;
}
}  // namespace

extern "C" {

void sgtd_order_tiles(int *sort_tile, int *group_tile) {
  if (sort_tile) *sort_tile = SGTD_OS_TILE;
  if (group_tile) *group_tile = SGTD_GI_TILE;
}

void sgtd_default_config(sgtd_config *cfg) {
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->descriptor_near_num = 10;
  cfg->candidate_num = 50;
  cfg->max_frame_n = 20000;
  cfg->device_id = 0;
  cfg->descriptor_min_len = 0.5;
  cfg->descriptor_max_len = 50.0;
  cfg->std_side_resolution = 1.0;
  cfg->rough_dis_threshold = 0.03;
  cfg->first_frame_id = 0;
}

const char *sgtd_strerror(int status) {
  switch (status) {
    case SGTD_OK: return "ok";
    case SGTD_ERR_INVALID: return "invalid argument";
    case SGTD_ERR_NO_DEVICE: return "no usable gfx950 HIP device";
    case SGTD_ERR_HIP: return "HIP runtime error";
    case SGTD_ERR_CAPACITY: return "buffer capacity exceeded";
    case SGTD_ERR_FRAME_LIMIT: return "frame id beyond max_frame_n";
    case SGTD_ERR_UNSUPPORTED: return "configuration outside the kernels' envelope";
    case SGTD_ERR_STATE: return "call order";
    case SGTD_ERR_IO: return "graph file could not be opened or parsed";
    default: return "unknown status";
  }
}

const char *sgtd_last_error(sgtd_handle h) { return h ? h->err.c_str() : ""; }

uint32_t sgtd_label_code(int a, int b, int c) { return label_code(a, b, c); }
uint64_t sgtd_table_key(uint32_t code, uint32_t x, uint32_t y, uint32_t z) { return pack_key(code, x, y, z); }
uint64_t sgtd_dedup_key(uint64_t mx, uint64_t my, uint64_t mz) { return pack_milli_key(mx, my, mz); }

int sgtd_create(const sgtd_config *cfg, sgtd_handle *out) {
  if (!cfg || !out) return SGTD_ERR_INVALID;
  *out = nullptr;
  int r = check_cfg(cfg);
  if (r != SGTD_OK) return r;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SGTD_ERR_NO_DEVICE;
  if (cfg->device_id < 0 || cfg->device_id >= ndev) return SGTD_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device_id) != hipSuccess) return SGTD_ERR_NO_DEVICE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SGTD_ERR_NO_DEVICE;
  if (hipSetDevice(cfg->device_id) != hipSuccess) return SGTD_ERR_NO_DEVICE;
  sgtd_engine *e = new sgtd_engine();
  e->cfg = *cfg;
  e->dc.K = cfg->descriptor_near_num;
  e->dc.tpi = (cfg->descriptor_near_num - 1) * (cfg->descriptor_near_num - 2) / 2;
  e->dc.cand_num = cfg->candidate_num;
  e->dc.min_len = cfg->descriptor_min_len;
  e->dc.max_len = cfg->descriptor_max_len;
  e->dc.scale = 1.0 / cfg->std_side_resolution;  // STDesc.cpp:178
  e->dc.rough = cfg->rough_dis_threshold;
  e->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  e->current_frame_id = cfg->first_frame_id;
  e->qd.with_thr2 = true;
  if (const char *o = getenv("SGTD_SORTED_CHUNK")) e->sorted_chunk = atoi(o);
  if (const char *o = getenv("SGTD_TAIL_MAX")) e->tail_max = atoll(o);
  if (const char *o = getenv("SGTD_COARSE_AT")) e->coarse_at = (u32)std::min(62ll, std::max(0ll, atoll(o)));
  if (const char *o = getenv("SGTD_REC_RATE")) e->rec_rate_hook = (u32)std::min(256, std::max(1, atoi(o)));
  if (const char *o = getenv("SGTD_WIDE_PAIRS")) e->wide_pairs = atoi(o) != 0;
  if (const char *o = getenv("SGTD_ORDER_FORM")) e->order_form = atoi(o) != 0 ? 1 : 0;
  if (const char *o = getenv("SGTD_ORDER_POLLS")) e->order_polls = (u32)std::min(1ll << 30, std::max(0ll, atoll(o)));
  if (const char *o = getenv("SGTD_SELECT_MODE")) e->select_mode = std::min(2, std::max(0, atoi(o)));
  if (const char *o = getenv("SGTD_WHOLE_AT")) e->whole_at = (u32)std::min(62ll, std::max(0ll, atoll(o)));
  // test hook: start with a small match-record buffer so that the overflow / re-run path runs
  if (const char *o = getenv("SGTD_REC_CAP")) { e->rec_cap = (size_t)std::max(1024ll, atoll(o)); e->rec_cap_fixed = true; }
  // test hooks: start with a tiny pass pool / GroupRow reservation so that their overflow / re-run paths run
  if (const char *o = getenv("SGTD_POOL_UNITS")) e->pool_units = (size_t)std::max(64ll, atoll(o));
  if (const char *o = getenv("SGTD_GROUP_CAP")) e->group_cap_hook = (size_t)std::max(1ll, atoll(o));
  if (const char *o = getenv("SGTD_PAIR_CAP")) { e->pair_cap = (size_t)std::max(64ll, atoll(o)); e->rec_cap_fixed = true; }
  // test hook: the undecided queue's floor, so that a small record buffer gives a queue of rec_cap / 64 entries that overflows
  if (const char *o = getenv("SGTD_AMB_MIN")) e->amb_min = (size_t)std::max(1ll, atoll(o));
  for (int i = 0; i < EV_COUNT; i++)
    if (hipEventCreate(&e->ev[i]) != hipSuccess) { sgtd_destroy(e); return SGTD_ERR_HIP; }      // (the events made so far go too)
  if (hipEventCreateWithFlags(&e->ev_cand, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&e->ev_export_free, hipEventDisableTiming) != hipSuccess) { sgtd_destroy(e); return SGTD_ERR_HIP; }
  *out = e;
  return SGTD_OK;
}

int sgtd_create_multi(const sgtd_config *cfg, const int *device_ids, int n_dev, sgtd_handle *out) {
  if (n_dev == 1 && cfg && device_ids && out) {   // one device: the ordinary handle
    sgtd_config c = *cfg;
    c.device_id = device_ids[0];
    return sgtd_create(&c, out);
  }
  return multi::create(cfg, device_ids, n_dev, out);
}

int sgtd_device_count(sgtd_handle e) { return !e ? 0 : (e->grp ? multi::device_count(e) : 1); }

sgtd_handle sgtd_device_handle(sgtd_handle e, int k) {
  if (!e) return nullptr;
  if (!e->grp) return k == 0 ? e : nullptr;
  return multi::device_handle(e, k);
}

int sgtd_destroy(sgtd_handle e) {
  if (e && e->grp) return multi::destroy(e);
  if (!e) return SGTD_OK;
  if (e->n_views > 0) { e->err = "other handles are attached to this handle's table (sgtd_attach_table): destroy them first"; return SGTD_ERR_STATE; }
  (void)hipSetDevice(e->cfg.device_id);
  (void)hipStreamSynchronize(e->stream);
  if (e->attached_to) { e->attached_to->n_views--; e->attached_to = nullptr; }
  for (hipEvent_t ev : e->ck_ev)
    if (ev) (void)hipEventDestroy(ev);
  if (e->pin) (void)hipHostFree(e->pin);
  if (e->frame_host) (void)hipHostFree(e->frame_host);
  if (e->pin_build) (void)hipHostFree(e->pin_build);
  for (int i = 0; i < EV_COUNT; i++)
    if (e->ev[i]) (void)hipEventDestroy(e->ev[i]);
  if (e->ev_cand) (void)hipEventDestroy(e->ev_cand);
  if (e->ev_export_free) (void)hipEventDestroy(e->ev_export_free);
  delete e;      // (every device buffer and the stages' clocks go here, with the device selected above)
  return SGTD_OK;
}

int sgtd_set_stream(sgtd_handle e, void *hip_stream) {
  if (e && e->grp) { e->err = "not available on a multi-device handle (use the per-device form, sgtd_amd/dist.py)"; return SGTD_ERR_UNSUPPORTED; }
  if (!e) return SGTD_ERR_INVALID;
  // what is queued on the old stream (copies out of the pinned staging buffer included) finishes there first: the
  // staging bytes are reused as soon as the new stream has been waited for
  CHK(xfer_sync(e));
  e->stream = reinterpret_cast<hipStream_t>(hip_stream);
  return SGTD_OK;
}

int sgtd_set_timing(sgtd_handle e, int enabled) {
  if (e && e->grp) { for (int k = 0; k < sgtd_device_count(e); k++) sgtd_set_timing(sgtd_device_handle(e, k), enabled); return SGTD_OK; }
  if (!e) return SGTD_ERR_INVALID;
  e->timing = enabled != 0;
  return SGTD_OK;
}

int sgtd_current_frame_id(sgtd_handle e, uint32_t *out) {
  if (e && e->grp && out) { *out = multi::current_frame_id(e); return SGTD_OK; }
  if (!e || !out) return SGTD_ERR_INVALID;
  *out = e->current_frame_id;
  return SGTD_OK;
}

int64_t sgtd_max_descs(sgtd_handle e, int n_keypoints) {
  if (e && e->grp) return (int64_t)n_keypoints * ((e->cfg.descriptor_near_num - 1) * (e->cfg.descriptor_near_num - 2) / 2);
  if (!e || n_keypoints < 0) return 0;
  return (int64_t)n_keypoints * e->dc.tpi;
}

int sgtd_build(sgtd_handle e, const float *xyz, const uint32_t *label, int n, sgtd_desc_soa *out,
               int64_t capacity, int64_t *n_out) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (e && e->grp) return multi::build(e, xyz, label, n, out, capacity, n_out);
  if (!e || !out || !n_out || n < 0 || (n > 0 && (!xyz || !label))) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  *n_out = 0;
  if (n == 0) return SGTD_OK;
  CHK(settle_pending(e));
  {
    // One frame, the reference's call pattern: ONE transfer in (offsets, keypoints, labels in one page-locked block), the
    // build, which writes the count and every descriptor field straight into page-locked host memory (the kernel only ever
    // stores to its output: 0.6 MB over the link inside the kernel instead of a 1.2 MB copy behind it), and one wait — the
    // general path below issues a dozen small copies and three waits.  Frames whose descriptors exceed 4 MB take it.
    const long long cap = (long long)n * e->dc.tpi;
    const size_t in_bytes = 16 + (size_t)n * 16, out_bytes = 16 + (size_t)cap * 136;
    if (out_bytes <= ((size_t)4 << 20) && n >= e->dc.K) {
#ifdef SGTD_EXP_FRAME_LAPS      // host time of the call by part, to stderr (an experiment build)
      struct BLaps {
        std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), t = t0;
        std::string s;
        void lap(const char *what) { const auto n = std::chrono::steady_clock::now(); char b[64]; snprintf(b, sizeof b, " %s %.0f", what, std::chrono::duration<double, std::micro>(n - t).count()); s += b; t = n; }
        ~BLaps() { fprintf(stderr, "[build laps us]%s | all %.0f\n", s.c_str(), std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count()); }
      } blaps;
#define BLAP(x) blaps.lap(x)
#else
#define BLAP(x) do { } while (0)
#endif
      CHK(ensure(e, e->b_in, in_bytes));
      const size_t in_room = (in_bytes + 255) & ~(size_t)255;
      if (e->pin_build_cap < in_room + out_bytes) {
        if (e->pin_build) (void)hipHostFree(e->pin_build);
        e->pin_build = nullptr; e->pin_build_cap = 0;
        void *pp = nullptr;
        HIPCHK(hipHostMalloc(&pp, (in_room + out_bytes) * 2, hipHostMallocDefault));
        e->pin_build = static_cast<char *>(pp);
        e->pin_build_cap = (in_room + out_bytes) * 2;
      }
      char *hin = e->pin_build, *hout = e->pin_build + in_room;
      const long long off2[2] = {0, n};
      std::memcpy(hin, off2, 16);
      std::memcpy(hin + 16, xyz, (size_t)n * 12);
      std::memcpy(hin + 16 + (size_t)n * 12, label, (size_t)n * 4);
      HIPCHK(hipMemcpyAsync(e->b_in.p, hin, in_bytes, hipMemcpyHostToDevice, e->stream));
      BLAP("in");
      char *din = e->b_in.as<char>(), *dout = hout;      // (page-locked memory is device-visible at its own address)
      DescArrays o;
      o.side = reinterpret_cast<double *>(dout + 16); o.angle = o.side + cap * 3; o.center = o.angle + cap * 3;
      o.vertex = reinterpret_cast<float *>(o.center + cap * 3); o.label = reinterpret_cast<int *>(o.vertex + cap * 9);
      o.frame = reinterpret_cast<u32 *>(o.label + cap * 3); o.node_id = reinterpret_cast<int *>(o.frame + cap);
      o.qrec = nullptr;
      CHK(launch_build(e, reinterpret_cast<const float *>(din + 16), reinterpret_cast<const u32 *>(din + 16 + (size_t)n * 12),
                       reinterpret_cast<const long long *>(din), 1, n, e->current_frame_id, 0, o, cap, reinterpret_cast<u32 *>(dout)));
      BLAP("launch");
      HIPCHK(hipStreamSynchronize(e->stream));
      BLAP("out_and_wait");
      const u32 cnt = *reinterpret_cast<const u32 *>(hout);
      *n_out = cnt;
      if ((int64_t)cnt > capacity) return SGTD_ERR_CAPACITY;
      const char *hp = hout + 16;
      auto take = [&](void *dst, size_t width, size_t elem) {       // field of `width` elements per descriptor
        if (dst) std::memcpy(dst, hp, (size_t)cnt * width * elem);
        hp += (size_t)cap * width * elem;
      };
      take(out->side, 3, 8); take(out->angle, 3, 8); take(out->center, 3, 8); take(out->vertex, 9, 4); take(out->label, 3, 4);
      take(out->frame, 1, 4); take(out->node_id, 3, 4);
      BLAP("fields");
#undef BLAP
      return SGTD_OK;
    }
  }
  int64_t off[2] = {0, n};
  const float *dx; const u32 *dl; int max_n;
  CHK(stage_inputs(e, xyz, label, off, 1, 0, &dx, &dl, &max_n, /*own_set=*/true));
  const long long stride = (long long)n * e->dc.tpi;
  CHK(ensure_store(e, e->tmp, (size_t)std::max<long long>(stride, 1)));
  CHK(ensure(e, e->tmp_count, sizeof(u32)));
  CHK(launch_build(e, dx, dl, e->b_kp_off_dev.as<long long>(), 1, max_n, e->current_frame_id, 0,
                   e->tmp.view(), stride, e->tmp_count.as<u32>()));
  u32 cnt = 0;
  CHK(d2h(e, &cnt, e->tmp_count.p, sizeof(u32)));
  CHK(xfer_sync(e));
  *n_out = cnt;
  if ((int64_t)cnt > capacity) return SGTD_ERR_CAPACITY;
  return copy_out(e, e->tmp, 0, cnt, out, 0);
}

int sgtd_add(sgtd_handle e, const sgtd_desc_soa *d, int64_t n) {
  if (e && e->grp) return multi::add(e, d, n);
  if (!e || n < 0 || (n > 0 && (!d || !d->side || !d->label || !d->frame))) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  u32 lo = 0xFFFFFFFFu, hi = 0;
  for (int64_t i = 0; i < n; i++) {
    lo = std::min(lo, d->frame[i]);
    hi = std::max(hi, d->frame[i]);
  }
  if (n > 0 && hi >= (u32)e->cfg.max_frame_n) return SGTD_ERR_FRAME_LIMIT;
  if (e->attached_to) { e->err = "the table belongs to another handle (sgtd_attach_table): add to its owner"; return SGTD_ERR_STATE; }
  CHK(settle_pending(e));
  e->table_version++;
  e->current_frame_id++;  // STDesc.cpp:151, before anything is inserted
  e->n_add_calls++;
  if (n == 0) return SGTD_OK;
  CHK(ensure_store(e, e->tab, (size_t)(e->n_entries + n), true));
  CHK(copy_in(e, e->tab, (size_t)e->n_entries, (size_t)n, d));
  e->n_entries += n;
  note_frames(e, lo, hi);
  e->append_min_frame = std::min(e->append_min_frame, lo);
  e->finalized = false;
  e->batch_valid = false;
  return SGTD_OK;
}

int sgtd_add_frames(sgtd_handle e, const float *xyz, const uint32_t *label, const int64_t *kp_off,
                    int n_frames, int device_ptrs) {
  if (e && e->grp) return multi::add_frames(e, xyz, label, kp_off, n_frames, device_ptrs);
  if (!e || n_frames < 0 || !kp_off) return SGTD_ERR_INVALID;
  if (n_frames == 0) return SGTD_OK;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  if (e->attached_to) { e->err = "the table belongs to another handle (sgtd_attach_table): add to its owner"; return SGTD_ERR_STATE; }
  if ((uint64_t)e->current_frame_id + (uint64_t)n_frames > (uint64_t)e->cfg.max_frame_n)
    return SGTD_ERR_FRAME_LIMIT;
  CHK(settle_pending(e));
  e->table_version++;
  const int chunk = 512;
  for (int f0 = 0; f0 < n_frames; f0 += chunk) {
    const int nf = std::min(chunk, n_frames - f0);
    const float *dx; const u32 *dl; int max_n;
    CHK(stage_inputs(e, xyz, label, kp_off + f0, nf, device_ptrs, &dx, &dl, &max_n));
    const long long stride = (long long)std::max(max_n, 1) * e->dc.tpi;
    CHK(ensure_store(e, e->tmp, (size_t)stride * nf));
    CHK(ensure(e, e->tmp_count, (size_t)nf * sizeof(u32)));
    CHK(ensure(e, e->cnt_scan, (size_t)nf * sizeof(u32)));
    CHK(launch_build(e, dx, dl, e->kp_off_dev.as<long long>(), nf, max_n, e->current_frame_id, 1,
                     e->tmp.view(), stride, e->tmp_count.as<u32>()));
    std::vector<u32> cnt(nf);
    HIPCHK(hipMemcpyAsync(cnt.data(), e->tmp_count.p, (size_t)nf * sizeof(u32), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    std::vector<u32> goff(nf);
    long long total = 0;
    for (int f = 0; f < nf; f++) { goff[f] = (u32)total; total += cnt[f]; }
    if (e->n_entries + total >= (1ll << 32) - 2) return SGTD_ERR_UNSUPPORTED;
    CHK(ensure_store(e, e->tab, (size_t)(e->n_entries + total), true));
    HIPCHK(hipMemcpyAsync(e->cnt_scan.p, goff.data(), (size_t)nf * sizeof(u32), hipMemcpyHostToDevice, e->stream));
    AppendParams A;
    A.in_stride = stride; A.count = e->tmp_count.as<u32>(); A.goff = e->cnt_scan.as<u32>(); A.g0 = e->n_entries;
    append_descs_kernel<<<nf, 256, 0, e->stream>>>(A, e->tmp.view(), e->tab.view());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));  // goff staging vector dies here
    e->n_entries += total;
    note_frames(e, e->current_frame_id, e->current_frame_id + (u32)nf - 1);
    e->append_min_frame = std::min(e->append_min_frame, e->current_frame_id);
    e->current_frame_id += (u32)nf;   // one AddSTDescs (:151) per frame
    e->n_add_calls += nf;
  }
  e->finalized = false;
  e->batch_valid = false;
  return SGTD_OK;
}

int sgtd_attach_table(sgtd_handle v, sgtd_handle o) {
  if (!v || !o || v == o) return SGTD_ERR_INVALID;
  if (v->grp || o->grp) { v->err = "not available on a multi-device handle"; return SGTD_ERR_UNSUPPORTED; }
  sgtd_engine *e = v;
  if (o->attached_to) { e->err = "attach to the handle that owns the table"; return SGTD_ERR_INVALID; }
  if (v->cfg.device_id != o->cfg.device_id || v->cfg.descriptor_near_num != o->cfg.descriptor_near_num ||
      v->cfg.descriptor_min_len != o->cfg.descriptor_min_len || v->cfg.descriptor_max_len != o->cfg.descriptor_max_len ||
      v->cfg.std_side_resolution != o->cfg.std_side_resolution || v->cfg.rough_dis_threshold != o->cfg.rough_dis_threshold ||
      v->cfg.max_frame_n != o->cfg.max_frame_n) {
    e->err = "sgtd_attach_table: the two handles are configured differently";
    return SGTD_ERR_INVALID;
  }
  if (!v->attached_to && (v->n_entries != 0 || v->n_views != 0)) { e->err = "sgtd_attach_table: this handle holds a table of its own"; return SGTD_ERR_STATE; }
  HIPCHK(hipSetDevice(v->cfg.device_id));
  CHK(settle_pending(v));
  HIPCHK(hipStreamSynchronize(v->stream));
  {
    const int st = do_finalize(o);      // the probe layout the view borrows
    if (st != SGTD_OK) { e->err = "sgtd_attach_table: the owner's table could not be finalized"; return st; }
    if (hipStreamSynchronize(o->stream) != hipSuccess) return SGTD_ERR_HIP;
  }
  v->tab.side.borrow_from(o->tab.side); v->tab.angle.borrow_from(o->tab.angle); v->tab.center.borrow_from(o->tab.center);
  v->tab.vertex.borrow_from(o->tab.vertex); v->tab.label.borrow_from(o->tab.label); v->tab.frame.borrow_from(o->tab.frame);
  v->tab.node_id.borrow_from(o->tab.node_id);
  v->tab.cap = o->tab.cap;
  for (int k = 0; k < 2; k++) {
    sgtd_engine::Segment &d = v->seg[k];
    const sgtd_engine::Segment &s = o->seg[k];
    d.hot.borrow_from(s.hot); d.perm.borrow_from(s.perm); d.hash.borrow_from(s.hash); d.bucket_start.borrow_from(s.bucket_start);
    d.bucket_key.borrow_from(s.bucket_key); d.dir.borrow_from(s.dir);
    d.hash_mask = s.hash_mask; d.n_buckets = s.n_buckets; d.g0 = s.g0; d.g1 = s.g1; d.sum_len_sq = s.sum_len_sq;
    d.frame_hi = s.frame_hi; d.built = s.built;
  }
  v->frame_first.borrow_from(o->frame_first); v->by_frame.borrow_from(o->by_frame); v->id_of_g.borrow_from(o->id_of_g);
  v->n_seg = o->n_seg; v->id_bits = o->id_bits; v->id_by_frame = o->id_by_frame;
  v->n_entries = o->n_entries; v->n_add_calls = o->n_add_calls; v->have_frames = o->have_frames;
  v->frame_lo = o->frame_lo; v->frame_hi = o->frame_hi; v->current_frame_id = o->current_frame_id;
  v->ms_finalize = o->ms_finalize;
  v->finalized = true;
  v->batch_valid = false;
  if (v->attached_to != o) {
    if (v->attached_to) v->attached_to->n_views--;
    o->n_views++;
  }
  v->attached_to = o;
  v->attached_version = o->table_version;
  return SGTD_OK;
}

int sgtd_finalize(sgtd_handle e) {
  if (e && e->grp) return multi::finalize(e);
  if (!e) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  return do_finalize(e);
}

// a batch of query frames built on the device: query q is stamped qframe (loop: qframe + q and the sweep's bound)
// a batch of n_queries against the filter's rows: one row for all, or one per query
static int filter_fits(sgtd_engine *e, int n_queries) {
  if (e->filt && e->filt->n_rows > 1 && e->filt->n_rows != n_queries) {
    e->err = "the frame filter has " + std::to_string(e->filt->n_rows) + " rows for a batch of " + std::to_string(n_queries) + " queries";
    return SGTD_ERR_INVALID;
  }
  return SGTD_OK;
}

// a batch of n_queries against the position prior's rows: one row for all, or one per query
static int prior_fits(sgtd_engine *e, int n_queries) {
  if (e->prior && e->prior->n_rows > 1 && e->prior->n_rows != n_queries) {
    e->err = "the position prior has " + std::to_string(e->prior->n_rows) + " rows for a batch of " + std::to_string(n_queries) + " queries";
    return SGTD_ERR_INVALID;
  }
  return SGTD_OK;
}

// What every batch starts with: its shape and kind, the filter and the prior it runs under (a loop batch: none), the
// product form of the sweep, the reservation rate's recovery, room for its descriptors and their counts.
static int begin_batch(sgtd_engine *e, int nq, long long q_stride, int kind, bool loop = false, int32_t skip_near = 0) {
  e->nq = nq;
  e->q_stride = q_stride;
  e->last_kind = kind;
  e->loop_batch = loop; e->loop_skip = loop ? skip_near : 0;
  e->batch_filt = loop ? nullptr : e->filt;
  e->batch_prior = loop ? nullptr : e->prior;
  e->diag = false;   // a new batch runs the product sweep; sgtd_result_rough re-runs it in the diagnostic form
  e->rec_rate_cap = e->stats.overflowed ? e->rec_rate_cap : std::min<u32>(256, e->rec_rate_cap * 2);   // (a cap a re-run needed recovers slowly)
  CHK(ensure_store(e, e->qd, (size_t)q_stride * nq));
  CHK(ensure(e, e->q_count, (size_t)nq * sizeof(u32)));
  return SGTD_OK;
}

static int query_frames_batch(sgtd_handle e, const float *xyz, const uint32_t *label, const int64_t *kp_off,
                              int n_queries, int device_ptrs, u32 qframe, bool loop, int32_t skip_near) {
  CHK(settle_tail(e));
  const float *dx; const u32 *dl; int max_n;
  CHK(stage_inputs(e, xyz, label, kp_off, n_queries, device_ptrs, &dx, &dl, &max_n));
  e->last_xyz = dx; e->last_label = dl; e->last_max_n = max_n;
  e->last_qframe = qframe;
  CHK(begin_batch(e, n_queries, (long long)std::max(max_n, 1) * e->dc.tpi, /*kind=*/1, loop, skip_near));
  if (!e->rec_cap_fixed && e->stats.last_queries == 0) {
    // first batch of this handle: size the match-record buffer from the table statistics instead
    // of growing it through overflow re-runs (each costs a whole sweep)
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    // ... plus what the slabs of all resident streams leave unused: each holds about half a slab of eight expected lists
    const double per_query = est_matches_per_query(e, max_n);
    const double per_desc = per_query / std::max(1.0, 0.62 * (double)max_n * e->dc.tpi);
    const double slab_slack = (double)e->n_cus * 32.0 * SGTD_PAIR * 0.5 * 8.0 * (3.0 * per_desc + 256.0);
    const double margin = e->n_entries > 100000000 ? 1.75 : 1.3;    // (long buckets: the estimate runs low at 100 000 frames)
    const double want = margin * per_query * (double)n_queries + std::min(slab_slack, margin * per_query * (double)n_queries);
    const double cap_mem = (double)free_b / 4.0 / 16.0;    // records + compact list + pairs, a quarter of what is free
    const size_t cap = (size_t)std::min(std::min(want, cap_mem), (double)kRecLimit);
    if (cap > e->rec_cap) e->rec_cap = cap;
    if (std::min(cap / 2, kIndexLimit) > e->pair_cap) e->pair_cap = std::min(cap / 2, kIndexLimit);   // candidate pairs: 0.2 .. 0.5 of the matches
  }
  return enqueue_frames(e);
}

int sgtd_query_frames(sgtd_handle e, const float *xyz, const uint32_t *label, const int64_t *kp_off,
                      int n_queries, int device_ptrs) {
  if (e && e->grp) return multi::query_frames(e, xyz, label, kp_off, n_queries, device_ptrs);
  if (!e || n_queries <= 0 || !kp_off || !xyz || !label) return SGTD_ERR_INVALID;
  CHK(filter_fits(e, n_queries));
  CHK(prior_fits(e, n_queries));
  HIPCHK(hipSetDevice(e->cfg.device_id));
  return query_frames_batch(e, xyz, label, kp_off, n_queries, device_ptrs, e->current_frame_id, false, 0);
}

int sgtd_loop_frames(sgtd_handle e, const float *xyz, const uint32_t *label, const int64_t *kp_off,
                     int n_frames, int32_t skip_near, int device_ptrs) {
  if (e && e->grp) {
    // (its round-robin frame blocks make the local frame index non-monotonic in the frame id: a bound on it would be wrong)
    e->err = "not available on a multi-device handle";
    return SGTD_ERR_UNSUPPORTED;
  }
  if (!e || n_frames <= 0 || !kp_off || !xyz || !label || skip_near < 0) return SGTD_ERR_INVALID;
  if (e->filt) { e->err = "a frame filter is set (sgtd_set_frame_filter): clear it before sgtd_loop_frames"; return SGTD_ERR_STATE; }
  if (e->prior) { e->err = "a position prior is set (sgtd_set_position_prior): clear it before sgtd_loop_frames"; return SGTD_ERR_STATE; }
  HIPCHK(hipSetDevice(e->cfg.device_id));
  if (e->attached_to) { e->err = "the table belongs to another handle (sgtd_attach_table): a view cannot add frames"; return SGTD_ERR_STATE; }
  const u32 c = e->current_frame_id;
  // the frames join the table first (sgtd_add_frames' build stamps c + k), then every frame is a query that sees
  // only what was added before it: the bound c + k - skip_near
  CHK(sgtd_add_frames(e, xyz, label, kp_off, n_frames, device_ptrs));
  return query_frames_batch(e, xyz, label, kp_off, n_frames, device_ptrs, c, true, skip_near);
}

int sgtd_query_descs(sgtd_handle e, const sgtd_desc_soa *q, int64_t nq) {
  if (e && e->grp) return multi::query_descs(e, q, nq);
  if (!e || nq < 0 || (nq > 0 && (!q || !q->side || !q->label || !q->frame))) return SGTD_ERR_INVALID;
  CHK(filter_fits(e, 1));
  CHK(prior_fits(e, 1));
  HIPCHK(hipSetDevice(e->cfg.device_id));
  CHK(settle_tail(e));
  CHK(begin_batch(e, 1, std::max<long long>(nq, 1), /*kind=*/2));
  CHK(copy_in(e, e->qd, 0, (size_t)nq, q));
  e->thr2_pending = nq;      // the descriptors' sweep records (thresholds, gate masks): launch_select writes them — one frame per call in its one launch
  u32 cnt = (u32)nq;
  CHK(h2d(e, e->q_count.p, &cnt, sizeof(u32)));
  CHK(xfer_sync(e));
  if (e->timing) HIPCHK(hipEventRecord(e->ev[EV_START], e->stream));
  return launch_select(e);
}

int sgtd_max_batch(sgtd_handle e, int n_keypoints, int64_t *max_queries) {
  if (e && e->grp) return multi::max_batch(e, n_keypoints, max_queries);
  if (!e || !max_queries || n_keypoints < 0) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  CHK(settle_tail(e));
  const double per_query = std::max(1.0, est_matches_per_query(e, n_keypoints)) * 2.0;   // margin: slab slack, variation
  size_t free_b = 0, total_b = 0;
  (void)hipMemGetInfo(&free_b, &total_b);
  // records are named by granules (6.9e10 of them), a batch's candidate pairs one by one: 0.2 .. 0.5 of the matches on the
  // uniform maps (four tenths before anything was measured; per_query carries a factor of two already)
  double pair_share = 0.4;
  if (e->stats.last_M > 0 && e->stats.last_cand_pairs > 0)      // measured on the batch before, half as much again
    pair_share = std::min(1.0, std::max(0.05, 1.5 * (double)e->stats.last_cand_pairs / (double)e->stats.last_M));
  // memory: 4 B per record and 8 B per candidate pair on top of what the buffers already hold (a batch this large takes the
  // per-query passes: no compact lists between the block passes, which would be 8 B per record more)
  const double mem_records = ((double)free_b * 0.8 + (double)e->rec.bytes + (double)e->c_pair.bytes + (double)e->pairs.bytes) / (4.0 + 8.0 * pair_share);
  const double lim = std::min(std::min((double)kRecLimit, mem_records), (double)kIndexLimit / pair_share * 2.0);
  *max_queries = (int64_t)std::max(1.0, std::floor(lim / per_query));
  return SGTD_OK;
}

int sgtd_sync(sgtd_handle e) {
  if (e && e->grp) return multi::sync(e);
  if (!e) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  if (!e->batch_valid) {
    HIPCHK(hipStreamSynchronize(e->stream));
    return SGTD_OK;
  }
  return sync_batch(e);
}

int sgtd_result_candidates(sgtd_handle e, int32_t *n_cand, int32_t *cand_frame, int32_t *cand_votes,
                           int64_t *pair_off) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (e && e->grp) return multi::result_candidates(e, n_cand, cand_frame, cand_votes, pair_off);
  if (!e) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  CHK(sync_batch(e));
  const int nq = e->nq, cn = e->dc.cand_num;
  if (n_cand) std::memcpy(n_cand, e->h_n_cand.data(), nq * sizeof(int));
  if (cand_frame) std::memcpy(cand_frame, e->h_cand_frame.data(), (size_t)nq * cn * sizeof(int));
  if (cand_votes) std::memcpy(cand_votes, e->h_cand_votes.data(), (size_t)nq * cn * sizeof(int));
  if (pair_off)
    for (size_t i = 0; i < (size_t)nq * (cn + 1); i++) pair_off[i] = e->h_pair_off[i];
  return SGTD_OK;
}

int sgtd_export_candidates_dev(sgtd_handle e, int32_t *d_cand_frame, int32_t *d_cand_votes) {
  if (e && e->grp) { e->err = "not available on a multi-device handle (use the per-device form, sgtd_amd/dist.py)"; return SGTD_ERR_UNSUPPORTED; }
  if (!e || !d_cand_frame || !d_cand_votes) return SGTD_ERR_INVALID;
  if (!e->batch_valid) return SGTD_ERR_STATE;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  // a batch that outgrew a work buffer has empty candidate tables until it is re-run:
  // resolve that first (one stream wait per batch; the tables of an intact batch are final)
  CHK(sync_batch(e));
  const size_t bytes = (size_t)e->nq * e->dc.cand_num * sizeof(int);
  HIPCHK(hipMemcpyAsync(d_cand_frame, e->cand_frame.p, bytes, hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(d_cand_votes, e->cand_votes.p, bytes, hipMemcpyDeviceToDevice, e->stream));
  return SGTD_OK;
}

int64_t sgtd_candidate_export_ints(int n_queries, int cand_num) {
  if (n_queries < 0 || cand_num < 0) return 0;
  return (int64_t)xchg_packed_ints(n_queries, cand_num);
}

#define SGTD_NO_GROUP(e)                                                                                                   \
  if ((e) && (e)->grp) { (e)->err = "not available on a multi-device handle (use the per-device form, sgtd_amd/dist.py)"; return SGTD_ERR_UNSUPPORTED; }

int sgtd_set_candidate_export(sgtd_handle e, int32_t *d_packed, int64_t capacity_ints) {
  SGTD_NO_GROUP(e);
  if (!e || capacity_ints < 0 || (d_packed && capacity_ints < SGTD_XCHG_FLAG_WORDS)) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  // (what is enqueued may still write the buffer registered before)
  HIPCHK(hipStreamSynchronize(e->stream));
  e->export_packed = d_packed;
  e->export_cap = d_packed ? (size_t)capacity_ints : 0;
  e->export_busy = false;
  return SGTD_OK;
}

int sgtd_export_wait(sgtd_handle e, void *side_stream) {
  SGTD_NO_GROUP(e);
  if (!e) return SGTD_ERR_INVALID;
  if (!e->export_packed || !e->batch_valid) return SGTD_ERR_STATE;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  HIPCHK(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(side_stream), e->ev_cand, 0));
  return SGTD_OK;
}

int sgtd_export_release(sgtd_handle e, void *side_stream) {
  SGTD_NO_GROUP(e);
  if (!e) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  HIPCHK(hipEventRecord(e->ev_export_free, reinterpret_cast<hipStream_t>(side_stream)));
  e->export_busy = true;
  return SGTD_OK;
}

int sgtd_merge_candidates_dev(sgtd_handle e, void *stream, const int32_t *d_gathered, int n_tables, int my_table, int n_queries,
                              int32_t *d_frame, int32_t *d_votes, int32_t *d_n_cand, int32_t *d_src, uint64_t *d_keep, int32_t *d_flags) {
  SGTD_NO_GROUP(e);
  if (!e || !d_gathered || !d_frame || !d_votes || !d_n_cand || !d_src || !d_keep || !d_flags || n_tables < 1 || n_queries < 0 ||
      my_table < -1 || my_table >= n_tables)
    return SGTD_ERR_INVALID;
  const int cn = e->dc.cand_num;
  if ((long long)n_tables * cn > (long long)SGTD_MERGE_PER_LANE * SGTD_WAVE || n_tables > 0x7FFFFF) return SGTD_ERR_UNSUPPORTED;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  // (min_votes 5: max_vote >= 5, STDesc.cpp:433)
  const int n_keys = n_tables * cn;
#define SGTD_MERGE(PER) merge_candidates_kernel<PER><<<std::max(1, grid_for(n_queries, 4)), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>( \
      d_gathered, (long long)xchg_packed_ints(n_queries, cn), n_tables, my_table, n_queries, cn, 5, d_frame, d_votes, d_n_cand, d_src,             \
      reinterpret_cast<u64 *>(d_keep), d_flags)
  if (n_keys <= SGTD_WAVE) SGTD_MERGE(1);
  else if (n_keys <= 4 * SGTD_WAVE) SGTD_MERGE(4);
  else if (n_keys <= 8 * SGTD_WAVE) SGTD_MERGE(8);
  else SGTD_MERGE(SGTD_MERGE_PER_LANE);
#undef SGTD_MERGE
  HIPCHK(hipGetLastError());
  return SGTD_OK;
}

int sgtd_gather_verified_dev(sgtd_handle e, void *stream, const double *d_gathered, int n_tables, const int32_t *d_src, int n_queries,
                             double *d_score, double *d_pose) {
  SGTD_NO_GROUP(e);
  if (!e || !d_gathered || !d_src || !d_score || !d_pose || n_tables < 1 || n_queries < 0) return SGTD_ERR_INVALID;
  const int cn = e->dc.cand_num;
  if (n_queries == 0) return SGTD_OK;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  gather_verified_kernel<<<grid_for((long long)n_queries * cn, 256), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
      d_gathered, (long long)n_queries * cn * 13, d_src, n_queries, cn, d_score, d_pose);
  HIPCHK(hipGetLastError());
  return SGTD_OK;
}

int sgtd_set_deferred_lists(sgtd_handle e, int on) {
  SGTD_NO_GROUP(e);
  if (!e) return SGTD_ERR_INVALID;
  e->defer_lists = on != 0;
  return SGTD_OK;
}

int sgtd_finish_lists(sgtd_handle e, const uint64_t *d_keep) {
  SGTD_NO_GROUP(e);
  if (!e) return SGTD_ERR_INVALID;
  if (!e->batch_valid) return SGTD_ERR_STATE;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  if (!e->plan.fused_pairs) {
    // the lists of this batch came from the passes of one wave per 128-descriptor block (small batches, frame spans
    // beyond LDS): they hold every local candidate already; a mask only matters to sgtd_verify_masked
    return SGTD_OK;
  }
  return launch_lists(e, make_views(e), reinterpret_cast<const u64 *>(d_keep), /*first=*/false);
}
#undef SGTD_NO_GROUP

int sgtd_result_query_desc_count(sgtd_handle e, int q, int64_t *n) {
  if (e && e->grp) return multi::result_query_desc_count(e, q, n);
  if (!e || !n) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  CHK(sync_batch(e));
  if (q < 0 || q >= e->nq) return SGTD_ERR_INVALID;
  *n = e->h_count[q];
  return SGTD_OK;
}

int sgtd_result_pairs(sgtd_handle e, int q, int32_t *q_idx, int64_t *db_entry, int64_t capacity,
                      int64_t *n_pairs) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (e && e->grp) return multi::result_pairs(e, q, q_idx, db_entry, capacity, n_pairs);
  if (!e || !n_pairs) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  CHK(sync_batch(e));
  if (q < 0 || q >= e->nq) return SGTD_ERR_INVALID;
  const int cn = e->dc.cand_num;
  const int64_t n = e->h_pair_off[(size_t)q * (cn + 1) + cn];
  *n_pairs = n;
  if (n > capacity) return SGTD_ERR_CAPACITY;
  if (n == 0) return SGTD_OK;
  std::vector<u64> pr(n);
  CHK(d2h(e, pr.data(), e->pairs.as<u64>() + e->h_pair_base[q], n * sizeof(u64)));
  CHK(xfer_sync(e));
  for (int64_t i = 0; i < n; i++) {
    if (q_idx) q_idx[i] = (int32_t)(pr[i] >> 32);
    if (db_entry) db_entry[i] = (int64_t)(pr[i] & 0xFFFFFFFFull);
  }
  return SGTD_OK;
}

int sgtd_result_query_descs(sgtd_handle e, int q, sgtd_desc_soa *out, int64_t capacity, int64_t *n_out) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (e && e->grp) return multi::result_query_descs(e, q, out, capacity, n_out);
  if (!e || !out || !n_out) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  CHK(sync_batch(e));
  if (q < 0 || q >= e->nq) return SGTD_ERR_INVALID;
  *n_out = e->h_count[q];
  if (*n_out > capacity) return SGTD_ERR_CAPACITY;
  return copy_out(e, e->qd, (size_t)q * e->q_stride, e->h_count[q], out, 0);
}

int sgtd_result_votes(sgtd_handle e, int q, uint32_t *votes, int64_t capacity, uint32_t *frame_lo, int64_t *n) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (e && e->grp) return multi::result_votes(e, q, votes, capacity, frame_lo, n);
  if (!e || !n) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  CHK(sync_batch(e));
  if (q < 0 || q >= e->nq) return SGTD_ERR_INVALID;
  const u32 span = e->have_frames ? (e->frame_hi - e->frame_lo + 1) : 1;
  *n = span;
  if (frame_lo) *frame_lo = e->have_frames ? e->frame_lo : 0;
  if (!votes) return SGTD_OK;
  if ((int64_t)span > capacity) return SGTD_ERR_CAPACITY;
  HIPCHK(hipMemcpyAsync(votes, e->votes.as<u32>() + (size_t)q * span, (size_t)span * sizeof(u32), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return SGTD_OK;
}

int sgtd_result_rough(sgtd_handle e, int q, int32_t *q_idx, int32_t *cell, int64_t *db_entry, uint32_t *frame,
                      double *dis, int64_t capacity, int64_t *n_rough) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (e && e->grp) { e->err = "not available on a multi-device handle (use the per-device form, sgtd_amd/dist.py)"; return SGTD_ERR_UNSUPPORTED; }
  if (!e || !n_rough) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  if (!e->batch_valid) return SGTD_ERR_STATE;
  if (!e->diag) {
    // the ordered rough list (cell index, distance, reference order inside a cell) comes from the
    // diagnostic probe build: switch it on and re-run the batch
    e->diag = true;
    CHK(rec_alloc(e, false));     // (the diagnostic arrays; the re-run below sizes the rest)
    CHK(rerun(e));
  }
  CHK(sync_batch(e));
  if (q < 0 || q >= e->nq) return SGTD_ERR_INVALID;
  const int64_t n = e->h_q_M[q];
  *n_rough = n;
  if (n > capacity) return SGTD_ERR_CAPACITY;
  if (n == 0) return SGTD_OK;
  CHK(ensure(e, e->rough_qi, n * sizeof(u32)));
  CHK(ensure(e, e->rough_entry, n * sizeof(u32)));
  CHK(ensure(e, e->rough_frame, n * sizeof(u32)));
  if (e->diag) {
    CHK(ensure(e, e->rough_cell, n));
    CHK(ensure(e, e->rough_dis, n * sizeof(double)));
  }
  Views v = make_views(e);
  rough_gather_kernel<<<1, 256, 0, e->stream>>>(v.Q, v.B, v.T.map, q, e->rough_qi.as<u32>(), e->rough_entry.as<u32>(),
                                                 e->rough_frame.as<u32>(),
                                                 e->diag ? e->rough_cell.as<unsigned char>() : nullptr,
                                                 e->diag ? e->rough_dis.as<double>() : nullptr);
  HIPCHK(hipGetLastError());
  std::vector<u32> a(n), g(n);
  std::vector<unsigned char> c(n);
  HIPCHK(hipMemcpyAsync(a.data(), e->rough_qi.p, n * sizeof(u32), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(g.data(), e->rough_entry.p, n * sizeof(u32), hipMemcpyDeviceToHost, e->stream));
  if (cell) HIPCHK(hipMemcpyAsync(c.data(), e->rough_cell.p, n, hipMemcpyDeviceToHost, e->stream));
  if (frame) HIPCHK(hipMemcpyAsync(frame, e->rough_frame.p, n * sizeof(u32), hipMemcpyDeviceToHost, e->stream));
  if (dis) HIPCHK(hipMemcpyAsync(dis, e->rough_dis.p, n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (int64_t i = 0; i < n; i++) {
    if (q_idx) q_idx[i] = (int32_t)a[i];
    if (db_entry) db_entry[i] = (int64_t)g[i];
    if (cell) cell[i] = c[i];
  }
  return SGTD_OK;
}

int sgtd_verify_masked(sgtd_handle e, const uint64_t *d_keep) {
  if (e && e->grp) { e->err = "not available on a multi-device handle (use the per-device form, sgtd_amd/dist.py)"; return SGTD_ERR_UNSUPPORTED; }
  if (!e) return SGTD_ERR_INVALID;
  e->verify_keep = reinterpret_cast<const u64 *>(d_keep);
  const int st = sgtd_verify(e);
  e->verify_keep = nullptr;
  return st;
}

}  // extern "C"

namespace {
// The batch's nb (query, candidate) slots in the order of the candidates' frames (empty slots last), for the kernels that
// take one block per slot: the table gathers and the keypoints of one frame stay close.  *order: the slots in dispatch
// order, in the handle's v_oval
int frame_order(sgtd_engine *e, size_t nb, const u32 **order) {
  for (int k = 0; k < 2; k++) { CHK(ensure(e, e->v_okey[k], nb * sizeof(u32))); CHK(ensure(e, e->v_oval[k], nb * sizeof(u32))); }
  u32 *kin = e->v_okey[0].as<u32>(), *kout = e->v_okey[1].as<u32>(), *vin = e->v_oval[0].as<u32>(), *vout = e->v_oval[1].as<u32>();
  const u32 last = e->frame_hi + 1u;          // key of a candidate slot that is empty
  verify_order_keys_kernel<<<grid_for((long long)nb, 256), 256, 0, e->stream>>>(e->cand_frame.as<int>(), e->n_cand.as<int>(), e->dc.cand_num, (u32)nb, last, kin, vin);
  HIPCHK(hipGetLastError());
  int bits = 1;
  while (bits < 32 && (last >> bits)) bits++;
  CHK(radix_sort_pairs<u32>(e, kin, kout, vin, vout, (long long)nb, bits, false));
  *order = vin;
  return SGTD_OK;
}

// candidate_verify + triangle_solver (STDesc.cpp:462-571) of every (query, candidate) of the batch, enqueued behind it;
// total = an upper bound on the pairs of all lists (sizes the per-pair scratch); guard: the kernels look at the batch's
// overflow flags first (the batch has not been waited for)
int verify_enqueue(sgtd_engine *e, int64_t total, bool guard) {
  const int cn = e->dc.cand_num, nq = e->nq;
  CHK(ensure(e, e->v_score, (size_t)nq * cn * sizeof(double)));
  CHK(ensure(e, e->v_pose, (size_t)nq * cn * 12 * sizeof(double)));
  CHK(ensure(e, e->v_inlier, (size_t)std::max<int64_t>(total, 1)));
  VerifyParams P;
  P.pairs = e->pairs.as<u64>(); P.pair_off = e->pair_off.as<long long>(); P.q_pair_base = e->q_pair_base.as<u32>();
  P.n_cand = e->n_cand.as<int>(); P.cand_num = cn; P.q_stride = e->q_stride;
  P.q_vertex = e->qd.vertex.as<float>(); P.q_center = e->qd.center.as<double>();
  P.t_vertex = e->tab.vertex.as<float>(); P.t_center = e->tab.center.as<double>();
  P.score = e->v_score.as<double>(); P.pose = e->v_pose.as<double>(); P.inlier = e->v_inlier.as<unsigned char>();
  P.thr2 = 9.0;   // sqrt_rn(y) < 3.0 <=> y < 9.0 (sqrt(9) = 3, sqrt(pred(9)) rounds to pred(3)); dis_threshold :469
  { const char *o = getenv("SGTD_VERIFY_EXACT"); P.exact_only = (o && atoi(o)) ? 1 : 0; }
  // the vote pass: on the matrix cores (verify_mfma.hip.h) unless SGTD_VERIFY_FORM=valu asks for the packed-f32 form
  bool mfma = true;
  { const char *o = getenv("SGTD_VERIFY_FORM"); if (o && !strcmp(o, "valu")) mfma = false; }
  CHK(ensure(e, e->v_hyp64, (size_t)nq * cn * SGTD_VERIFY_MAX_HYP * SGTD_HYP_F64 * sizeof(double)));
  CHK(ensure(e, e->v_bound, (size_t)nq * cn * 2 * sizeof(u32)));
  P.hyp64 = e->v_hyp64.as<double>(); P.bound = e->v_bound.as<u32>();
  P.passed = nullptr; P.hyp32 = nullptr; P.words = nullptr; P.hypB = nullptr; P.tau = nullptr;
  if (mfma) {
    // a row of 64 vote words per 32 pairs; candidate k of the batch starts at row (first pair / 32 + k)
    CHK(ensure(e, e->v_words, ((size_t)std::max<int64_t>(total, 1) / 32 + (size_t)nq * cn + 2) * 64 * sizeof(u32)));
    CHK(ensure(e, e->v_hypB, (size_t)nq * cn * 6 * 64 * sizeof(uint4)));
    CHK(ensure(e, e->v_tau, (size_t)nq * cn * 2 * SGTD_VERIFY_MAX_HYP * sizeof(float)));
    P.words = e->v_words.as<u32>(); P.hypB = e->v_hypB.as<uint4>(); P.tau = e->v_tau.as<float>();
  } else {
    // per-pair vote masks between the kernel's two passes (a buffer of their own: the compact candidate lists in c_pair may
    // still be needed by a re-run of the batch's list pass when this is enqueued behind an unfinished batch)
    CHK(ensure(e, e->v_words, (size_t)std::max<int64_t>(total, 1) * sizeof(u64)));
    CHK(ensure(e, e->v_hyp32, (size_t)nq * cn * SGTD_VERIFY_MAX_HYP * SGTD_HYP_F32 * sizeof(float)));
    P.passed = e->v_words.as<u64>(); P.hyp32 = e->v_hyp32.as<float>();
    HIPCHK(hipMemsetAsync(e->v_pose.p, 0, (size_t)nq * cn * 12 * sizeof(double), e->stream));     // (the matrix-core kernel writes every pose itself)
  }
  P.keep = e->verify_keep;
  P.inl_count = nullptr;
  if (guard && mfma) {        // (sgtd_search_frame: the kernel leaves the candidates' inlier counts behind)
    CHK(ensure(e, e->inl_counts, (size_t)std::max(nq * cn, SGTD_MAX_CAND) * sizeof(u32)));
    P.inl_count = e->inl_counts.as<u32>();
  }
  e->verify_counted = P.inl_count != nullptr;
  P.overflow = guard ? reinterpret_cast<const int *>(e->cursors.as<u32>() + CTR_OVERFLOW) : nullptr;
  P.order = nullptr; P.n_blocks = (u32)(nq * cn);
  int grid = nq * cn;
  // a batch of many candidates is dispatched in the order of the candidates' frames (SGTD_VERIFY_ORDER=0: as they stand)
  static const bool order_on = [] { const char *o = getenv("SGTD_VERIFY_ORDER"); return !(o && !atoi(o)); }();
  if (mfma && order_on && !guard && nq * cn >= 4096 && e->have_frames) {
    CHK(frame_order(e, (size_t)(nq * cn), &P.order));
    grid = 8 * ((nq * cn + 7) / 8);
  }
  verify_solve_kernel<<<nq * cn, SGTD_WAVE, 0, e->stream>>>(P);
  HIPCHK(hipGetLastError());
  if (mfma && nq * cn >= 1024) verify_mfma_kernel<4><<<grid, 4 * SGTD_WAVE, 0, e->stream>>>(P);
  else if (mfma) verify_mfma_kernel<8><<<grid, 8 * SGTD_WAVE, 0, e->stream>>>(P);
  else verify_kernel<<<nq * cn, SGTD_VERIFY_THREADS, 0, e->stream>>>(P);
  HIPCHK(hipGetLastError());
#ifdef SGTD_EXP_VSTAT
  {
    unsigned long long st[8];
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpyFromSymbol(st, HIP_SYMBOL(g_vstat), sizeof(st)));
    fprintf(stderr, "[vstat] steps %llu  steps with a pair left by vertex A %llu  with eight or more %llu | (pair, hypothesis) tests %llu  left by A %llu  of them in steps "
            "with eight or more %llu  not far on all three %llu  certain votes %llu\n", st[0], st[1], st[3], st[7], st[2], st[5], st[6], st[4]);
    unsigned long long z[8] = {0};
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_vstat), z, sizeof(z)));
    HIPCHK(hipMemcpyFromSymbol(st, HIP_SYMBOL(g_vmstat), sizeof(st)));
    fprintf(stderr, "[vmstat] (32 pairs x 32 hypotheses) steps %llu  with something left open %llu | combinations queued for the exact test %llu  of them votes %llu  "
            "queue drains %llu  certain votes %llu\n", st[0], st[1], st[2], st[3], st[4], st[5]);
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_vmstat), z, sizeof(z)));
  }
#endif
  return SGTD_OK;
}
}  // namespace

extern "C" {

int sgtd_verify(sgtd_handle e) {
  if (e && e->grp) return multi::verify(e);
  if (!e) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  CHK(sync_batch(e));
  if (!e->batch_valid) return SGTD_ERR_INVALID;
  const int cn = e->dc.cand_num, nq = e->nq;
  stale_stages(e);
  if (nq == 0) { e->verified = true; return SGTD_OK; }
  int64_t total = 0;
  for (int q = 0; q < nq; q++) total = std::max<int64_t>(total, (int64_t)e->h_pair_base[q] + e->h_pair_off[(size_t)q * (cn + 1) + cn]);
  CHK(verify_enqueue(e, total, /*guard=*/false));
  e->verified = true;
  return SGTD_OK;
}

int sgtd_result_verify(sgtd_handle e, int q, double *score, double *pose) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (e && e->grp) return multi::result_verify(e, q, score, pose);
  if (!e) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  if (!e->verified || !e->batch_valid || q < 0 || q >= e->nq) return SGTD_ERR_INVALID;
  const int cn = e->dc.cand_num;
  if (score) CHK(d2h(e, score, e->v_score.as<double>() + (size_t)q * cn, cn * sizeof(double)));
  if (pose) CHK(d2h(e, pose, e->v_pose.as<double>() + (size_t)q * cn * 12, (size_t)cn * 12 * sizeof(double)));
  CHK(xfer_sync(e));
  return SGTD_OK;
}

int sgtd_export_verify_dev(sgtd_handle e, double *d_score, double *d_pose) {
  if (e && e->grp) { e->err = "not available on a multi-device handle (use the per-device form, sgtd_amd/dist.py)"; return SGTD_ERR_UNSUPPORTED; }
  if (!e) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  if (!e->verified || !e->batch_valid) return SGTD_ERR_STATE;
  const size_t n = (size_t)e->nq * e->dc.cand_num;
  if (n == 0) return SGTD_OK;
  if (d_score) HIPCHK(hipMemcpyAsync(d_score, e->v_score.p, n * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  if (d_pose) HIPCHK(hipMemcpyAsync(d_pose, e->v_pose.p, n * 12 * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  return SGTD_OK;
}

int sgtd_result_inliers(sgtd_handle e, int q, int cand, int32_t *idx, int64_t capacity, int64_t *n) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (e && e->grp) return multi::result_inliers(e, q, cand, idx, capacity, n);
  if (!e || !n) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  if (!e->verified || !e->batch_valid || q < 0 || q >= e->nq) return SGTD_ERR_INVALID;
  const int cn = e->dc.cand_num;
  if (cand < 0 || cand >= e->h_n_cand[q]) return SGTD_ERR_INVALID;
  const int64_t lo = e->h_pair_off[(size_t)q * (cn + 1) + cand], hi = e->h_pair_off[(size_t)q * (cn + 1) + cand + 1];
  std::vector<unsigned char> fl((size_t)(hi - lo));
  if (hi > lo) {
    CHK(d2h(e, fl.data(), e->v_inlier.as<unsigned char>() + e->h_pair_base[q] + lo, (size_t)(hi - lo)));
    CHK(xfer_sync(e));
  }
  int64_t cnt = 0;
  for (int64_t j = 0; j < hi - lo; j++)
    if (fl[(size_t)j]) {
      if (idx && cnt < capacity) idx[cnt] = (int32_t)j;
      cnt++;
    }
  *n = cnt;
  return (idx && cnt > capacity) ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int sgtd_result_inlier_pairs(sgtd_handle e, int q, int64_t *cand_off, int32_t *q_idx, int64_t *db_entry, int64_t capacity,
                             int64_t *n_pairs) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (e && e->grp) return multi::result_inlier_pairs(e, q, cand_off, q_idx, db_entry, capacity, n_pairs);
  if (!e || !n_pairs || !cand_off) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  if (!e->verified || !e->batch_valid || q < 0 || q >= e->nq) return SGTD_ERR_INVALID;
  const int cn = e->dc.cand_num;
  const int64_t total = e->h_pair_off[(size_t)q * (cn + 1) + cn];
  CHK(ensure(e, e->inl_pairs, (size_t)std::max<int64_t>(total, 1) * sizeof(u64)));
  CHK(ensure(e, e->inl_off, (size_t)(cn + 1) * sizeof(long long)));
  inlier_pairs_kernel<<<1, SGTD_INLIER_THREADS, 0, e->stream>>>(e->pairs.as<u64>() + e->h_pair_base[q], e->v_inlier.as<unsigned char>() + e->h_pair_base[q],
                                                                e->pair_off.as<long long>() + (size_t)q * (cn + 1), cn, e->inl_pairs.as<u64>(),
                                                                e->inl_off.as<long long>());
  HIPCHK(hipGetLastError());
  std::vector<long long> off((size_t)cn + 1);
  CHK(d2h(e, off.data(), e->inl_off.p, off.size() * sizeof(long long)));
  CHK(xfer_sync(e));
  for (int k = 0; k <= cn; k++) cand_off[k] = off[(size_t)k];
  const int64_t n = off[(size_t)cn];
  *n_pairs = n;
  if (n > capacity) return SGTD_ERR_CAPACITY;
  if (n == 0) return SGTD_OK;
  std::vector<u64> pr((size_t)n);
  CHK(d2h(e, pr.data(), e->inl_pairs.p, (size_t)n * sizeof(u64)));
  CHK(xfer_sync(e));
  for (int64_t i = 0; i < n; i++) {
    if (q_idx) q_idx[i] = (int32_t)(pr[(size_t)i] >> 32);
    if (db_entry) db_entry[i] = (int64_t)(pr[(size_t)i] & 0xFFFFFFFFull);
  }
  return SGTD_OK;
}

int sgtd_result_inlier_entries(sgtd_handle e, int q, int64_t *cand_off, int32_t *q_idx, sgtd_desc_soa *entries, int64_t capacity,
                               int64_t *n_pairs) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (!e || !n_pairs || !cand_off) return SGTD_ERR_INVALID;
  if (e->grp) {
    // several devices: the pairs from the devices that own the candidates, then their entries (db_entry ids name the owner)
    std::vector<int64_t> ent((size_t)std::max<int64_t>(capacity, 0));
    const int st = sgtd_result_inlier_pairs(e, q, cand_off, q_idx, ent.data(), capacity, n_pairs);
    if (st != SGTD_OK) return st;
    return entries ? sgtd_fetch_entries(e, ent.data(), *n_pairs, entries) : SGTD_OK;
  }
  HIPCHK(hipSetDevice(e->cfg.device_id));
  CHK(view_current(e));
  if (!e->verified || !e->batch_valid || q < 0 || q >= e->nq) return SGTD_ERR_INVALID;
  const int cn = e->dc.cand_num;
  const int64_t total = e->h_pair_off[(size_t)q * (cn + 1) + cn];
  CHK(ensure(e, e->inl_pairs, (size_t)std::max<int64_t>(total, 1) * sizeof(u64)));
  CHK(ensure(e, e->inl_off, (size_t)(cn + 1) * sizeof(long long)));
  // index list, q_idx list and the gathered entries for the most there can be, so that everything is enqueued
  // before the one wait for the offsets
  CHK(ensure(e, e->fetch_idx, (size_t)std::max<int64_t>(total, 1) * (sizeof(long long) + sizeof(int))));
  CHK(ensure_store(e, e->fetch, (size_t)std::max<int64_t>(total, 1)));
  long long *d_idx = e->fetch_idx.as<long long>();
  int *d_qi = reinterpret_cast<int *>(d_idx + std::max<int64_t>(total, 1));
  inlier_pairs_kernel<<<1, SGTD_INLIER_THREADS, 0, e->stream>>>(e->pairs.as<u64>() + e->h_pair_base[q], e->v_inlier.as<unsigned char>() + e->h_pair_base[q],
                                                                e->pair_off.as<long long>() + (size_t)q * (cn + 1), cn, e->inl_pairs.as<u64>(),
                                                                e->inl_off.as<long long>());
  HIPCHK(hipGetLastError());
  if (total > 0) {
    split_pairs_kernel<<<grid_for(total, 256), 256, 0, e->stream>>>(e->inl_pairs.as<u64>(), e->inl_off.as<long long>() + cn, (long long)total, d_idx, d_qi);
    HIPCHK(hipGetLastError());
    gather_entries_counted_kernel<<<grid_for(total, 256), 256, 0, e->stream>>>(d_idx, e->inl_off.as<long long>() + cn, (long long)total, e->tab.view(), e->fetch.view());
    HIPCHK(hipGetLastError());
  }
  std::vector<long long> off((size_t)cn + 1);
  CHK(d2h(e, off.data(), e->inl_off.p, off.size() * sizeof(long long)));
  CHK(xfer_sync(e));
  for (int k = 0; k <= cn; k++) cand_off[k] = off[(size_t)k];
  const int64_t n = off[(size_t)cn];
  *n_pairs = n;
  if (n > capacity) return SGTD_ERR_CAPACITY;
  if (n == 0) return SGTD_OK;
  if (q_idx) CHK(d2h(e, q_idx, d_qi, (size_t)n * sizeof(int)));
  if (entries) return copy_out(e, e->fetch, 0, (size_t)n, entries, 0);
  return xfer_sync(e);
}

int sgtd_search_loop(sgtd_handle e, double icp_threshold, int32_t *best_cand, int32_t *best_frame, double *best_score) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (e && e->grp) return multi::search_loop(e, icp_threshold, best_cand, best_frame, best_score);
  if (!e) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  if (!e->verified || !e->batch_valid) return SGTD_ERR_INVALID;
  const int cn = e->dc.cand_num, nq = e->nq;
  if (nq == 0) return SGTD_OK;
  CHK(ensure(e, e->v_best, (size_t)nq * (2 * sizeof(int) + sizeof(double))));
  double *d_score = e->v_best.as<double>();
  int *d_cand = reinterpret_cast<int *>(d_score + nq), *d_frame = d_cand + nq;
  search_loop_kernel<<<grid_for(nq, 256), 256, 0, e->stream>>>(e->v_score.as<double>(), e->cand_frame.as<int>(), e->n_cand.as<int>(), cn, nq,
                                                               icp_threshold, d_cand, d_frame, d_score);
  HIPCHK(hipGetLastError());
  if (best_cand) CHK(d2h(e, best_cand, d_cand, nq * sizeof(int)));
  if (best_frame) CHK(d2h(e, best_frame, d_frame, nq * sizeof(int)));
  if (best_score) CHK(d2h(e, best_score, d_score, nq * sizeof(double)));
  CHK(xfer_sync(e));
  return SGTD_OK;
}

// [p, p + bytes) is page-locked host memory a kernel can write through the same address (hipHostMalloc / sgtd_host_alloc)
static bool device_can_write(const void *p, size_t bytes) {
  if (!p) return true;        // (a member the caller does not want)
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (a.type != hipMemoryTypeHost || a.devicePointer != p) return false;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) != hipSuccess) { (void)hipGetLastError(); return false; }
  return static_cast<const char *>(p) + bytes <= static_cast<const char *>(base) + size;
}

// One query frame through candidate_selector, candidate_verify and the inlier pairs with their table entries in ONE call
// and (normally) two waits: the reference's per-frame call pattern (semantic_graph_localization.cpp:590-603 ->
// STDesc.cpp:84-147) as sgtd_query_descs + sgtd_verify + sgtd_result_candidates + sgtd_result_verify +
// sgtd_result_inlier_entries issue it costs eight waits and some sixty small copies.  Everything is enqueued behind the
// batch without looking at it — the kernels behind the lists check the batch's overflow flags themselves — the small
// results come back as one packed block (FramePack), then the inlier pairs' entries.  The call by parts, in their order:
#ifdef SGTD_EXP_FRAME_LAPS      // host time of the call by part, to stderr (an experiment build)
struct FrameLaps {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), t = t0;
  std::string s;
  void lap(const char *what) { const auto n = std::chrono::steady_clock::now(); char b[64]; snprintf(b, sizeof b, " %s %.0f", what, std::chrono::duration<double, std::micro>(n - t).count()); s += b; t = n; }
  ~FrameLaps() { fprintf(stderr, "[frame laps us]%s | all %.0f\n", s.c_str(), std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count()); }
};
#define LAP(x) c.laps.lap(x)
#else
#define LAP(x) do { } while (0)
#endif
// what the parts of one call share
struct FrameCall {
  sgtd_frame_search *io = nullptr;
  int cn = 0;
  bool lists_only = false;     // candidate_selector alone: no verification, every pair of every list
  bool direct = false;         // the entries go straight into the caller's (page-locked) arrays
  size_t pack_bytes = 0;       // the packed block's share of the handle's host block; the staged entries lie behind it
  const int *ovf = nullptr;    // the batch's overflow flags on the device
  // the pairs whose entries go to the caller, and their offsets per candidate: the inlier pairs (compacted by frame_verify), or — lists only —
  // the match lists as they stand (a one-query batch's pairs start at 0 of the pair buffer; pair_off[cn] = their number)
  const u64 *out_pairs = nullptr;
  const long long *out_off = nullptr;
  DescArrays host_out{};       // staged form: this frame's entries and query indices in the host block
  int *host_qi = nullptr;
#ifdef SGTD_EXP_FRAME_LAPS
  FrameLaps laps;
#endif
};

// 1. the checks, then sgtd_query_descs without its waits
static int frame_batch(sgtd_engine *e, const sgtd_desc_soa *q, int64_t nq, sgtd_frame_search *io, FrameCall &c) {
  if (e && e->grp) { e->err = "not available on a multi-device handle"; return SGTD_ERR_UNSUPPORTED; }
  if (!e || !io || nq < 0 || (nq > 0 && (!q || !q->side || !q->label || !q->frame)) || io->capacity < 0) return SGTD_ERR_INVALID;
  CHK(filter_fits(e, 1));
  CHK(prior_fits(e, 1));
  HIPCHK(hipSetDevice(e->cfg.device_id));
  c.io = io;
  c.cn = e->dc.cand_num;
  c.lists_only = (io->flags & SGTD_FRAME_LISTS_ONLY) != 0;
  io->n_cand = 0; io->n_inliers = 0;
  CHK(settle_tail(e));
  CHK(begin_batch(e, 1, std::max<long long>(nq, 1), /*kind=*/2));
  CHK(copy_in(e, e->qd, 0, (size_t)nq, q, /*wait=*/false));
  LAP("descriptors_in");
  e->thr2_pending = nq;      // the descriptors' sweep records (thresholds, gate masks): launch_select writes them — one frame per call in its one launch
  const u32 cnt = (u32)nq;
  CHK(h2d(e, e->q_count.p, &cnt, sizeof(u32)));      // (staged: the bytes are copied out of `cnt` here)
  if (e->timing) HIPCHK(hipEventRecord(e->ev[EV_START], e->stream));
  const bool deferred = e->defer_lists;
  e->defer_lists = false;
  const int ls = launch_select(e);
  e->defer_lists = deferred;
  CHK(ls);
  LAP("select_launches");
  c.ovf = reinterpret_cast<const int *>(e->cursors.as<u32>() + CTR_OVERFLOW);
  c.out_pairs = e->pairs.as<u64>();
  c.out_off = e->pair_off.as<long long>();
  return SGTD_OK;
}

// 2. candidate_verify behind it, sized by what the pair buffer holds, and the inlier pairs of every candidate, compacted by one
// workgroup per candidate
static int frame_verify(sgtd_engine *e, FrameCall &c) {
  const int cn = c.cn;
  CHK(verify_enqueue(e, (int64_t)pair_room(e), /*guard=*/true));
  CHK(ensure(e, e->inl_counts, (size_t)SGTD_MAX_CAND * sizeof(u32)));
  CHK(ensure(e, e->inl_off, (size_t)(cn + 1) * sizeof(long long)));
  CHK(ensure(e, e->inl_pairs, (size_t)pair_room(e) * sizeof(u64)));
  if (!e->verify_counted) {     // (the packed-f32 form of the vote pass does not count)
    inlier_count_kernel<<<cn, SGTD_INLIER_CAND_THREADS, 0, e->stream>>>(e->v_inlier.as<unsigned char>(), e->pair_off.as<long long>(), e->n_cand.as<int>(), c.ovf,
                                                                         e->inl_counts.as<u32>());
    HIPCHK(hipGetLastError());
  }
  inlier_compact_kernel<<<cn, SGTD_INLIER_CAND_THREADS, 0, e->stream>>>(e->pairs.as<u64>(), e->v_inlier.as<unsigned char>(), e->pair_off.as<long long>(),
                                                                         e->n_cand.as<int>(), c.ovf, e->inl_counts.as<u32>(), cn, e->inl_pairs.as<u64>(),
                                                                         e->inl_off.as<long long>());
  HIPCHK(hipGetLastError());
  c.out_pairs = e->inl_pairs.as<u64>();
  c.out_off = e->inl_off.as<long long>();
  return SGTD_OK;
}

// 3. the entries of the first `room` pairs (their count is on the device) enqueued: into the caller's arrays, or into the handle's
// host block behind the pack, which grows to hold them
static int frame_gather(sgtd_engine *e, FrameCall &c, size_t room) {
  const size_t need = c.pack_bytes + (c.direct ? 0 : room * 144);
  if (need > e->frame_host_bytes) {
    HIPCHK(hipStreamSynchronize(e->stream));          // (nothing may still be writing the block that is given back)
    if (e->frame_host) (void)hipHostFree(e->frame_host);
    e->frame_host = nullptr; e->frame_host_bytes = 0;
    void *hp = nullptr;
    if (hipHostMalloc(&hp, need, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); e->err = "hipHostMalloc of the frame results failed"; return SGTD_ERR_HIP; }
    e->frame_host = static_cast<char *>(hp); e->frame_host_bytes = need;
  }
  if (c.direct) {
    const sgtd_desc_soa &o = c.io->entries;
    DescArrays user{};
    user.side = o.side; user.angle = o.angle; user.center = o.center; user.vertex = o.vertex; user.label = o.label; user.frame = o.frame; user.node_id = o.node_id;
    gather_pair_entries_kernel<<<1024, 256, 0, e->stream>>>(c.out_pairs, c.out_off + c.cn, (long long)c.io->capacity, c.io->inlier_q_idx, e->tab.view(), user, c.ovf);
    HIPCHK(hipGetLastError());
    return SGTD_OK;
  }
  DescArrays &h = c.host_out;
  char *at = e->frame_host + c.pack_bytes;               // (doubles first: every array stays aligned to its element)
  h.side = reinterpret_cast<double *>(at); at += room * 24;
  h.angle = reinterpret_cast<double *>(at); at += room * 24;
  h.center = reinterpret_cast<double *>(at); at += room * 24;
  h.vertex = reinterpret_cast<float *>(at); at += room * 36;
  h.label = reinterpret_cast<int *>(at); at += room * 12;
  h.node_id = reinterpret_cast<int *>(at); at += room * 12;
  h.frame = reinterpret_cast<u32 *>(at); at += room * 4;
  c.host_qi = reinterpret_cast<int *>(at);
  h.qrec = nullptr;
  gather_pair_entries_kernel<<<(unsigned)std::min<long long>(grid_for((long long)room * 8, 256), 1024), 256, 0, e->stream>>>(
      c.out_pairs, c.out_off + c.cn, (long long)room, c.host_qi, e->tab.view(), h, c.ovf);
  HIPCHK(hipGetLastError());
  return SGTD_OK;
}

// The results go where the host reads them: page-locked memory the kernels write over the link — the packed block first (the
// handle's), then the inlier pairs' entries and query indices: straight into the CALLER's arrays when those are page-locked
// (sgtd_host_alloc: the 23 MB of a frame's 160 000 pairs on a 10 000-frame map cross the link once, at its rate, and the call
// has ONE wait), else into the handle's own block, room for `room` pairs, and from there with memcpy.  (Copies device ->
// host cost 0.15 ms each on this runtime and ran at 16 GB/s: eight of them for the entries were 1.4 ms of the call.)
static int frame_results(sgtd_engine *e, FrameCall &c) {
  const int cn = c.cn;
  c.pack_bytes = (FramePack(nullptr, cn).bytes() + 255) & ~(size_t)255;
  const size_t ucap = (size_t)c.io->capacity;
  const sgtd_desc_soa &o = c.io->entries;
  static const bool direct_on = [] { const char *v = getenv("SGTD_FRAME_DIRECT"); return !(v && !atoi(v)); }();
  c.direct = direct_on && ucap > 0 && device_can_write(c.io->inlier_q_idx, ucap * 4) && device_can_write(o.side, ucap * 24) && device_can_write(o.angle, ucap * 24) &&
             device_can_write(o.center, ucap * 24) && device_can_write(o.vertex, ucap * 36) && device_can_write(o.label, ucap * 12) &&
             device_can_write(o.node_id, ucap * 12) && device_can_write(o.frame, ucap * 4);
  if (e->frame_inl_cap == 0) e->frame_inl_cap = 16384;
  CHK(frame_gather(e, c, c.direct ? ucap : e->frame_inl_cap));
  pack_frame_kernel<<<1, 256, 0, e->stream>>>(e->cursors.as<u32>(), e->n_cand.as<int>(), e->q_M.as<u32>(), e->q_pair_base.as<u32>(), e->q_count.as<u32>(),
                                              e->q_P.as<unsigned long long>(), e->cand_frame.as<int>(), e->cand_votes.as<int>(),
                                              e->pair_off.as<long long>(), c.lists_only ? nullptr : e->v_score.as<double>(), c.lists_only ? nullptr : e->v_pose.as<double>(), c.out_off,
                                              cn, reinterpret_cast<unsigned char *>(e->frame_host), e->totals.as<unsigned long long>());
  HIPCHK(hipGetLastError());
  LAP("verify_and_result_launches");
  return SGTD_OK;
}

// 4. the batch outgrew a work buffer (a first frame, a frame unlike the ones before): sgtd_sync re-runs it, then the calls this
// one stands for, one after the other
static int frame_fallback(sgtd_engine *e, FrameCall &c) {
  sgtd_frame_search *io = c.io;
  CHK(sync_batch(e));
  if (c.lists_only) {
    std::vector<int64_t> off((size_t)c.cn + 1, 0);
    CHK(sgtd_result_candidates(e, &io->n_cand, io->cand_frame, io->cand_votes, off.data()));
    if (io->pair_off) std::memcpy(io->pair_off, off.data(), off.size() * sizeof(int64_t));
    if (io->inlier_off) std::memcpy(io->inlier_off, off.data(), off.size() * sizeof(int64_t));
    const int64_t total = off[(size_t)io->n_cand];
    io->n_inliers = total;
    if (total > io->capacity) return SGTD_ERR_CAPACITY;
    if (total == 0) return SGTD_OK;
    std::vector<int64_t> ids((size_t)total);
    std::vector<int32_t> qi;
    int64_t got = 0;
    if (!io->inlier_q_idx) qi.resize((size_t)total);
    CHK(sgtd_result_pairs(e, 0, io->inlier_q_idx ? io->inlier_q_idx : qi.data(), ids.data(), total, &got));
    return sgtd_fetch_entries(e, ids.data(), total, &io->entries);
  }
  CHK(sgtd_verify(e));
  CHK(sgtd_result_candidates(e, &io->n_cand, io->cand_frame, io->cand_votes, io->pair_off));
  CHK(sgtd_result_verify(e, 0, io->score, io->pose));
  std::vector<int64_t> off((size_t)c.cn + 1);
  const int st = sgtd_result_inlier_entries(e, 0, off.data(), io->inlier_q_idx, &io->entries, io->capacity, &io->n_inliers);
  if (io->inlier_off) std::memcpy(io->inlier_off, off.data(), off.size() * sizeof(int64_t));
  return st;
}

// 5. the host-side state every sgtd_result_* call reads, as sync_batch leaves it, from the pack
static int frame_host_tables(sgtd_engine *e, const FrameCall &c, const FramePack &pack) {
  const size_t cn = (size_t)c.cn;
  if (!(e->h_count.resize(1) && e->h_pair_base.resize(2) && e->h_q_M.resize(1) && e->h_q_P.resize(1) && e->h_n_cand.resize(1) &&
        e->h_cand_frame.resize(cn) && e->h_cand_votes.resize(cn) && e->h_pair_off.resize(cn + 1))) {
    e->err = "hipHostMalloc of the result tables failed";
    return SGTD_ERR_HIP;
  }
  e->h_count[0] = *pack.q_count(); e->h_pair_base[0] = 0; e->h_pair_base[1] = *pack.pairs_total(); e->h_q_M[0] = *pack.q_M();
  std::memcpy(&e->h_q_P[0], pack.q_P(), 8);
  e->h_n_cand[0] = *pack.n_cand();
  std::memcpy(e->h_cand_frame.data(), pack.cand_frame(), cn * 4); std::memcpy(e->h_cand_votes.data(), pack.cand_votes(), cn * 4);
  std::memcpy(e->h_pair_off.data(), pack.pair_off(), (cn + 1) * 8);
  sgtd_stats &st = e->stats;
  const u32 *ctr = pack.ctr();
  unsigned long long swept = 0;
  std::memcpy(&swept, ctr + CTR_SWEPT, 8);
  st.overflowed = 0; st.last_list_moves = ctr[CTR_LIST_MOVES];
  st.last_queries = 1; st.last_D = *pack.q_count(); st.last_P = (int64_t)e->h_q_P[0]; st.last_M = *pack.q_M(); st.last_P_swept = (int64_t)swept;
  st.last_cand_pairs = pack.pair_off()[cn];
  if (e->totals.p) {      // the handle's running totals, as sync_batch reads them
    const unsigned long long *tot = pack.totals();
    st.batches_total = (int64_t)tot[0]; st.overflow_launches_total = (int64_t)tot[1]; st.list_moves_total = (int64_t)tot[2];
  }
  stage_times(e);
  e->batch_synced = true;
  new_results(e, !c.lists_only);
  return SGTD_OK;
}

// 6. the caller's io from the pack, then — staged form — the entries from the host block: gathered once more, with a wait, when the
// frame has more pairs than the block had room for
static int frame_copy_out(sgtd_engine *e, FrameCall &c, const FramePack &pack) {
  sgtd_frame_search *io = c.io;
  const size_t cn = (size_t)c.cn;
  io->n_cand = (int32_t)*pack.n_cand();
  if (io->cand_frame) std::memcpy(io->cand_frame, pack.cand_frame(), cn * 4);
  if (io->cand_votes) std::memcpy(io->cand_votes, pack.cand_votes(), cn * 4);
  if (io->pair_off) std::memcpy(io->pair_off, pack.pair_off(), (cn + 1) * 8);
  if (io->score && !c.lists_only) std::memcpy(io->score, pack.score(), cn * 8);
  if (io->pose && !c.lists_only) std::memcpy(io->pose, pack.pose(), cn * 96);
  if (io->inlier_off) std::memcpy(io->inlier_off, pack.inl_off(), (cn + 1) * 8);
  const int64_t n_inl = pack.inl_off()[cn];
  io->n_inliers = n_inl;
  if (n_inl > io->capacity) return SGTD_ERR_CAPACITY;       // (everything else is valid; sgtd_result_inlier_entries with more room gives the pairs)
  if (n_inl == 0) return SGTD_OK;
  if (c.direct) { LAP("entries_in_place"); return SGTD_OK; }  // (the kernel wrote the caller's arrays)
  if ((size_t)n_inl > e->frame_inl_cap) {                   // more inlier pairs than the gather had room for: once more, with room
    e->frame_inl_cap = (size_t)n_inl + (size_t)n_inl / 2;   // (everything of the pack was copied out above: the block may move)
    CHK(frame_gather(e, c, e->frame_inl_cap));
    HIPCHK(hipStreamSynchronize(e->stream));
  } else if ((size_t)n_inl * 2 > e->frame_inl_cap) {
    e->frame_inl_cap = (size_t)n_inl * 2;                   // (room for the next frame; host_out still names this frame's arrays)
  }
  LAP("host_tables");
  const size_t n = (size_t)n_inl;
  const sgtd_desc_soa &o = io->entries;
  const DescArrays &h = c.host_out;
  if (io->inlier_q_idx) std::memcpy(io->inlier_q_idx, c.host_qi, n * sizeof(int));
  if (o.side) std::memcpy(o.side, h.side, n * 24);
  if (o.angle) std::memcpy(o.angle, h.angle, n * 24);
  if (o.center) std::memcpy(o.center, h.center, n * 24);
  if (o.vertex) std::memcpy(o.vertex, h.vertex, n * 36);
  if (o.label) std::memcpy(o.label, h.label, n * 12);
  if (o.node_id) std::memcpy(o.node_id, h.node_id, n * 12);
  if (o.frame) std::memcpy(o.frame, h.frame, n * 4);
  LAP("entries_out");
  return SGTD_OK;
}

int sgtd_search_frame(sgtd_handle e, const sgtd_desc_soa *q, int64_t nq, sgtd_frame_search *io) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  FrameCall c;
  CHK(frame_batch(e, q, nq, io, c));
  if (!c.lists_only) CHK(frame_verify(e, c));
  CHK(frame_results(e, c));
  CHK(xfer_sync(e));                                        // ---- the call's one wait (nothing is queued for it: it also gives the staging back)
  const FramePack pack(e->frame_host, c.cn);
  LAP("wait_1");
  if (pack.overflowed()) return frame_fallback(e, c);
  CHK(frame_host_tables(e, c, pack));
  return frame_copy_out(e, c, pack);
}
#undef LAP

int sgtd_save_table(sgtd_handle e, const char *path) {
  if (e && e->grp) { e->err = "not available on a multi-device handle (use the per-device form, sgtd_amd/dist.py)"; return SGTD_ERR_UNSUPPORTED; }
  if (!e || !path) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  FILE *f = fopen(path, "wb");
  if (!f) { e->err = std::string("cannot open for writing: ") + path; return SGTD_ERR_IO; }
  TableHeader h{};
  h.side_resolution = e->cfg.std_side_resolution; h.min_len = e->cfg.descriptor_min_len; h.max_len = e->cfg.descriptor_max_len;
  h.near_num = e->cfg.descriptor_near_num; h.have_frames = e->have_frames ? 1 : 0;
  h.current_frame_id = e->current_frame_id; h.frame_lo = e->frame_lo; h.frame_hi = e->frame_hi;
  h.n_entries = e->n_entries; h.n_add_calls = e->n_add_calls;
  int st = (fwrite(kTableMagic, 1, 8, f) == 8 && fwrite(&h, sizeof(h), 1, f) == 1) ? SGTD_OK : SGTD_ERR_IO;
  if (st == SGTD_OK) st = stream_table(e, f, (size_t)e->n_entries, true);
  if (fclose(f) != 0 && st == SGTD_OK) st = SGTD_ERR_IO;
  if (st == SGTD_ERR_IO) e->err = std::string("write failed: ") + path;
  return st;
}

int sgtd_load_table(sgtd_handle e, const char *path) {
  if (e && e->grp) { e->err = "not available on a multi-device handle (use the per-device form, sgtd_amd/dist.py)"; return SGTD_ERR_UNSUPPORTED; }
  if (!e || !path) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  if (e->attached_to) { e->err = "the table belongs to another handle (sgtd_attach_table): load into its owner"; return SGTD_ERR_STATE; }
  CHK(settle_pending(e));
  e->table_version++;
  FILE *f = fopen(path, "rb");
  if (!f) { e->err = std::string("Error opening file: ") + path; return SGTD_ERR_IO; }
  TableHeader h{};
  {
    const int hs = read_table_header(f, path, e->cfg, h, e->err);
    if (hs != SGTD_OK) { fclose(f); return hs; }
  }
  int st = ensure_store(e, e->tab, (size_t)std::max<int64_t>(h.n_entries, 1), false);
  if (st == SGTD_OK) st = stream_table(e, f, (size_t)h.n_entries, false);
  fclose(f);
  if (st == SGTD_OK && h.n_entries > 0) {
    // the votes are indexed by frame - frame_lo: every stored frame id must lie in the header's range
    int bad = 0;
    st = ensure(e, e->bad_flag, sizeof(int));
    if (st == SGTD_OK) {
      HIPCHK(hipMemsetAsync(e->bad_flag.p, 0, sizeof(int), e->stream));
      frame_range_check_kernel<<<grid_for(h.n_entries, 256), 256, 0, e->stream>>>(e->tab.frame.as<u32>(), h.n_entries, h.frame_lo, h.frame_hi,
                                                                                   e->bad_flag.as<int>());
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(&bad, e->bad_flag.p, sizeof(int), hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      if (bad) st = SGTD_ERR_IO;
    }
  }
  if (st != SGTD_OK) {
    if (st == SGTD_ERR_IO) e->err = std::string(path) + ": truncated or damaged table file";
    e->n_entries = 0; e->have_frames = false; e->finalized = false; e->batch_valid = false;
    e->seg[0].built = false; e->seg[1].built = false;
    return st;
  }
  e->n_entries = h.n_entries; e->n_add_calls = h.n_add_calls; e->current_frame_id = h.current_frame_id;
  e->have_frames = h.have_frames != 0; e->frame_lo = h.frame_lo; e->frame_hi = h.frame_hi;
  e->seg[0].built = false; e->seg[1].built = false;
  e->finalized = false;
  e->batch_valid = false;
  return SGTD_OK;
}

int sgtd_remove_frames(sgtd_handle e, const uint32_t *frame_ids, int64_t n, int64_t *n_removed) {
  if (n_removed) *n_removed = 0;
  if (e && e->grp) return multi::remove_frames(e, frame_ids, n, n_removed);
  if (!e || n < 0 || (n > 0 && !frame_ids)) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  if (e->attached_to) { e->err = "the table belongs to another handle (sgtd_attach_table): remove frames through its owner"; return SGTD_ERR_STATE; }
  if (n == 0 || !e->have_frames || e->n_entries == 0) return SGTD_OK;
  // the removed set over the table's frame span; ids outside it have no entries
  const u32 lo = e->frame_lo;
  const u64 span = (u64)e->frame_hi - lo + 1;
  if (span > 0x80000000ull) { e->err = "the table's frame span is too wide for sgtd_remove_frames"; return SGTD_ERR_UNSUPPORTED; }
  std::vector<u32> bits((size_t)((span + 31) / 32), 0u);
  bool any = false;
  for (int64_t i = 0; i < n; i++) {
    const u64 d = (u64)(frame_ids[i] - lo);
    if (frame_ids[i] >= lo && d < span) { bits[(size_t)(d >> 5)] |= 1u << (d & 31); any = true; }
  }
  if (!any) return SGTD_OK;
  CHK(settle_pending(e));     // (a pending batch may still re-run over the table)
  int64_t r = 0;
  CHK(remove_entries(e, bits, (u32)span, &r));
  if (n_removed) *n_removed = r;
  return SGTD_OK;
}

int sgtd_set_frame_filter(sgtd_handle e, uint32_t frame_lo, uint32_t n_frames, const uint64_t *rows, int n_rows) {
  if (!e || n_rows < 0 || (n_rows > 0 && (!rows || n_frames == 0))) return SGTD_ERR_INVALID;
  if (e->grp) return multi::set_frame_filter(e, frame_lo, n_frames, rows, n_rows);
  if (n_rows == 0) { e->filt.reset(); return SGTD_OK; }
  static std::atomic<u64> serial{0};
  auto F = std::make_shared<FrameFilter>();
  F->lo = frame_lo; F->n = n_frames; F->n_rows = n_rows;
  F->words = ((size_t)n_frames + 63) / 64;
  F->rows.assign(rows, rows + (size_t)n_rows * F->words);
  if (n_frames % 64)
    for (int r = 0; r < n_rows; r++) F->rows[(size_t)r * F->words + F->words - 1] &= (1ull << (n_frames % 64)) - 1ull;
  F->serial = ++serial;
  e->filt = std::move(F);
  return SGTD_OK;
}

// the poses of `n` frames kept on a handle (global ids: sgtd_set_frame_poses has checked them); pose12 == nullptr forgets
static void store_poses(sgtd_engine *e, const uint32_t *frame_ids, const float *pose12, int64_t n) {
  for (int64_t i = 0; i < n; i++) {
    const size_t id = frame_ids[i];
    if (id >= e->has_pose.size()) {
      if (!pose12) continue;
      e->has_pose.resize(id + 1, 0);
      e->poses.resize((id + 1) * 12, 0.f);
    }
    e->has_pose[id] = pose12 ? 1 : 0;
    if (pose12) std::memcpy(e->poses.data() + id * 12, pose12 + (size_t)i * 12, 12 * sizeof(float));
  }
}

static u64 next_pose_serial() {
  static std::atomic<u64> serial{0};
  return ++serial;
}

int sgtd_set_frame_poses(sgtd_handle e, const uint32_t *frame_ids, const float *pose12, int64_t n) {
  if (!e || n < 0 || (n > 0 && !frame_ids)) return SGTD_ERR_INVALID;
  for (int64_t i = 0; i < n; i++)
    if (frame_ids[i] >= (uint32_t)e->cfg.max_frame_n) return SGTD_ERR_FRAME_LIMIT;
  if (e->grp) CHK(multi::set_frame_poses(e, frame_ids, pose12, n));
  if (n == 0) {
    if (frame_ids) return SGTD_OK;
    e->poses.clear(); e->has_pose.clear();
  } else {
    store_poses(e, frame_ids, pose12, n);
  }
  e->poses_serial = next_pose_serial();
  return SGTD_OK;
}

int sgtd_set_position_prior(sgtd_handle e, const double *center, const double *radius, int n_rows, int dims) {
  if (!e || n_rows < 0) return SGTD_ERR_INVALID;
  if (n_rows > 0) {
    if (!center || !radius || (dims != 2 && dims != 3)) return SGTD_ERR_INVALID;
    for (int r = 0; r < n_rows; r++) {
      for (int i = 0; i < dims; i++)
        if (!std::isfinite(center[(size_t)r * dims + i])) return SGTD_ERR_INVALID;
      if (std::isnan(radius[r]) || radius[r] < 0.0) return SGTD_ERR_INVALID;
    }
  }
  if (e->grp) CHK(multi::set_position_prior(e, center, radius, n_rows, dims));
  if (n_rows == 0) { e->prior.reset(); return SGTD_OK; }
  static std::atomic<u64> serial{0};
  auto P = std::make_shared<PositionPrior>();
  P->n_rows = n_rows; P->dims = dims;
  P->prm.resize((size_t)n_rows);
  for (int r = 0; r < n_rows; r++) {
    const double *c = center + (size_t)r * dims;
    P->prm[(size_t)r] = make_double4(c[0], c[1], dims == 3 ? c[2] : 0.0, radius[r] * radius[r]);
  }
  P->serial = ++serial;
  e->prior = std::move(P);
  return SGTD_OK;
}

}  // extern "C"

// ---- what the stages on a verified batch share (sgtd_refine_poses, sgtd_overlap, sgtd_align_keypoints) and what reads
// their results ----
namespace {
// "<who> needs <what> on the pending batch"
int needs(sgtd_engine *e, const char *who, const char *what) {
  e->err = std::string(who) + " needs " + what + " on the pending batch";
  return SGTD_ERR_STATE;
}

// what a stage's getter says where the stage has not run on the pending batch
const char kNoRefined[] = "no refined poses: sgtd_refine_poses comes after sgtd_verify on the pending batch";
const char kNoOverlap[] = "no overlap results: sgtd_overlap comes after sgtd_verify on the pending batch";
const char kNoAligned[] = "no aligned results: sgtd_align_keypoints comes after sgtd_verify on the pending batch";

// a stage's getter of query q on a single-device handle: the stage has run on the pending batch (`missing` says what
// has not), q is one of its queries, the table is still the one the batch ran on
int result_ready(sgtd_engine *e, int q, bool done, const char *missing) {
  if (!e->batch_valid || !e->verified || !done) { e->err = missing; return SGTD_ERR_STATE; }
  if (q < 0 || q >= e->nq) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  return view_current(e);
}

// what a keypoint pass's kernel takes from the batch, the keypoint store's device copy (prepare_keypoints) and the call:
// the members OverlapParams and AlignParams have in common, but the query keypoints (stage_query_keypoints)
template <class Params>
void keypoint_params(sgtd_engine *e, bool refined, double radius, size_t nb, Params *P) {
  P->n_cand = e->n_cand.as<int>(); P->cand_frame = e->cand_frame.as<int>(); P->cand_num = e->dc.cand_num;
  P->score = e->v_score.as<double>();
  P->pose = refined ? e->r_pose.as<double>() : e->v_pose.as<double>();
  P->kp = e->kp_dev.as<uint4>(); P->f_word = e->kp_word.as<u64>(); P->n_ids = (u32)e->has_kps.size();
  P->rr = radius * radius;
  P->order = nullptr; P->n_blocks = (u32)nb;
}

// ---- what the cloud and graph stages share (sgtd_consistent_loops, sgtd_relax_poses, sgtd_pose_consensus,
// sgtd_scan_keypoints, sgtd_local_map_keypoints, sgtd_register_clouds, sgtd_register_voxels): their results do not belong
// to a batch and live on one engine ----
// the engine a handle's batch-independent results live on: the handle itself, a group's first device
sgtd_engine *home_engine(sgtd_engine *e) { return e->grp ? multi::device_handle(e, 0) : e; }

// a stage's count of results, by the engine's member that stands for the stage: the count itself, or the registration
// run that holds it
template <class N> N &stage_count(N &n) { return n; }
int &stage_count(DenseRun &r) { return r.n; }
int &stage_count(VoxelRun &r) { return r.n; }

// a getter's state check: *c is e's home engine, whose count of results (stage_count of `stage`) is negative while the
// stage has not run (`missing` says so on the caller's handle)
template <class S>
int stage_ready(sgtd_engine *e, S sgtd_engine::*stage, const char *missing, sgtd_engine **c) {
  *c = home_engine(e);
  if (stage_count((*c)->*stage) < 0) { e->err = missing; return SGTD_ERR_STATE; }
  return SGTD_OK;
}

// A getter's copies from the home engine c to the caller's arrays: the device is selected, a copy is skipped where
// the caller passed no array, has nothing to get or an earlier step failed, finish() waits for them all and hands a
// group handle the failure's text.  (Leaving the scope drops what a failed getter left queued: PinScope.)
struct CopyOut {
  sgtd_engine *e, *c;
  PinScope pin;
  int st;
  CopyOut(sgtd_engine *e_, sgtd_engine *c_) : e(e_), c(c_), pin(c_), st(hipSetDevice(c->cfg.device_id) == hipSuccess ? SGTD_OK : SGTD_ERR_HIP) {}
  void get(void *dst, const void *dev_src, size_t bytes) {
    if (st == SGTD_OK && dst && bytes) st = d2h(c, dst, dev_src, bytes);
  }
  int finish() {
    if (st == SGTD_OK) st = xfer_sync(c);
    if (st != SGTD_OK && c != e) e->err = c->err;
    return st;
  }
};

// An entry point's run on the home engine c: from here on the stage has no results (its count, *n, is negative; no
// device is touched yet), on_device() selects c's device and runs the stage's work at once (nothing may switch the
// device in between: a group's getters do), and end() marks the results present unless that work failed, whose text
// it hands a group handle.  A call with nothing to run ends without on_device().
template <class N>
struct StageRun {
  sgtd_engine *e, *c;
  N *n;
  PinScope pin;
  int st = SGTD_OK;
  template <class S>
  StageRun(sgtd_engine *e_, S sgtd_engine::*stage) : e(e_), c(home_engine(e_)), n(&stage_count(c->*stage)), pin(c) { *n = -1; }
  int select() {
    sgtd_engine *e = c;      // (HIPCHK reports on the engine that runs the stage)
    HIPCHK(hipSetDevice(c->cfg.device_id));
    return SGTD_OK;
  }
  template <class Work>
  void on_device(Work &&work) {
    st = select();
    if (st == SGTD_OK) st = work(c);
  }
  int end(N have) {
    if (st != SGTD_OK) {
      if (c != e) e->err = c->err;
      return st;
    }
    *n = have;
    return SGTD_OK;
  }
};

// the call's points on the device: the caller's array as it is, or (points from the host) a copy in buf
int points_on_device(sgtd_engine *c, DevBuf &buf, const float *points, size_t floats, int device_ptrs, const float **d_pts) {
  *d_pts = points;
  if (device_ptrs || floats == 0) return SGTD_OK;
  CHK(ensure(c, buf, floats * sizeof(float)));
  CHK(h2d(c, buf.p, points, floats * sizeof(float)));
  *d_pts = buf.as<float>();
  return SGTD_OK;
}

// a call's clouds (scans), back to back: the offsets start at 0 and do not fall, a point has 3 or 4 floats, and where
// there is a point there are the arrays (labels only where the call takes them: need_labels)
bool cloud_set_ok(const int64_t *pt_off, int n_clouds, int stride_floats, const float *points, bool need_labels, const uint32_t *labels) {
  if (n_clouds < 0 || !pt_off || (stride_floats != 3 && stride_floats != 4) || pt_off[0] != 0) return false;
  for (int cl = 0; cl < n_clouds; cl++)
    if (pt_off[cl + 1] < pt_off[cl]) return false;
  return pt_off[n_clouds] == 0 || (points && (labels || !need_labels));
}

int key_bits(u64 v) { int b = 0; while (v) { b++; v >>= 1; } return std::max(b, 1); }

// The runs of equal keys in n sorted keys (keys from `drop` on belong to no run): head flags, their exclusive scan
// (excl[n]: the count of runs), the runs' keys and first positions.  counts: zeroed on the stream by the caller.
int voxel_runs(sgtd_engine *e, const u64 *keys, long long n, u64 drop, u32 *flags, u32 *excl, u32 *counts, u64 *vkey, u32 *vstart) {
  scan_heads_kernel<<<grid_for(n + 1, 256), 256, 0, e->stream>>>(keys, n, drop, flags, counts);
  HIPCHK(hipGetLastError());
  CHK(device_scan(e, flags, excl, n + 1));
  scan_voxels_kernel<<<grid_for(n, 256), 256, 0, e->stream>>>(keys, flags, excl, n, counts, vkey, vstart);
  return SGTD_OK;      // (the caller asks for the launches' error, behind what it launches next)
}

using RunScratch = sgtd_engine::RunScratch;
// room for the runs among n pairs
int need_runs(sgtd_engine *e, RunScratch &R, size_t n) {
  CHK(need_each(e, n, R.key_a, R.key_b, R.val_a, R.val_b));
  CHK(need_each(e, n + 1, R.flags, R.excl));
  CHK(need(e, R.counts, 4));
  CHK(need(e, R.vkey, n));
  return need(e, R.vstart, n + 1);
}
// The n pairs a kernel left in key_a / val_a, sorted by the low `bits` of the key (stable), and their runs (voxel_runs;
// keys from `drop` on belong to none).  *keys / *vals: where the sort left the pairs.
int sorted_runs(sgtd_engine *e, RunScratch &R, long long n, int bits, bool skip_const, u64 drop, u64 **keys, u32 **vals) {
  u64 *kin = R.key_a.p(), *kout = R.key_b.p();
  u32 *vin = R.val_a.p(), *vout = R.val_b.p();
  CHK(radix_sort_pairs<u64>(e, kin, kout, vin, vout, n, bits, skip_const));
  HIPCHK(hipMemsetAsync(R.counts.p(), 0, 4 * sizeof(u32), e->stream));
  CHK(voxel_runs(e, kin, n, drop, R.flags.p(), R.excl.p(), R.counts.p(), R.vkey.p(), R.vstart.p()));
  *keys = kin; *vals = vin;
  return SGTD_OK;
}

int LapClock::start(sgtd_engine *e, bool timed) {
  for (float &v : ms) v = 0.f;
  if (timed)
    for (hipEvent_t &v : ev)
      if (!v) HIPCHK(hipEventCreate(&v));
  return SGTD_OK;
}
int LapClock::lap(sgtd_engine *e, int kind) {
  HIPCHK(hipEventRecord(ev[1], e->stream));
  CHK(span(e, 0, 1, kind, true));
  HIPCHK(hipEventRecord(ev[0], e->stream));
  return SGTD_OK;
}
int LapClock::span(sgtd_engine *e, int a, int b, int kind, bool wait) {
  if (wait) HIPCHK(hipEventSynchronize(ev[b]));
  float t = 0.f;
  HIPCHK(hipEventElapsedTime(&t, ev[a], ev[b]));
  ms[kind] += t;
  return SGTD_OK;
}
void LapClock::destroy() {
  for (hipEvent_t &v : ev) {
    if (v) (void)hipEventDestroy(v);
    v = nullptr;
  }
}

// query q's candidate count and frames, of a single-device handle or of a group
int batch_candidates(sgtd_engine *e, int q, int *n_cand, int *cand_frame) {
  if (e->grp) return multi::candidates_of(e, q, n_cand, cand_frame);
  CHK(sync_batch(e));
  const int cn = e->cfg.candidate_num;
  *n_cand = e->h_n_cand[(size_t)q];
  std::memcpy(cand_frame, e->h_cand_frame.data() + (size_t)q * cn, (size_t)cn * sizeof(int));
  return SGTD_OK;
}

// world[k * 12 ..] = the stored pose M of the frame of query q's candidate k composed with its relative pose (R, t cast
// to f32), each operation an f32 rounding in the order include/sgtd_accel.h states; NaNs past the query's candidates, for
// candidates without a result (has(k) says which have one) and for frames without a pose.  pose: what a stage's getter
// gave for q (which has checked q)
template <class Has>
int world_poses_of(sgtd_engine *e, int q, const double *pose, Has has, float *world) {
  const int cn = e->cfg.candidate_num;
  std::vector<int> cand_frame((size_t)cn);
  int n_cand = 0;
  CHK(batch_candidates(e, q, &n_cand, cand_frame.data()));
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (int k = 0; k < cn; k++) {
    float *w = world + (size_t)k * 12;
    std::fill(w, w + 12, nan);
    if (k >= n_cand || !has(k)) continue;
    const size_t id = (size_t)(u32)cand_frame[(size_t)k];
    if (id >= e->has_pose.size() || !e->has_pose[id]) continue;
    const float *M = e->poses.data() + id * 12;
    const double *rel = pose + (size_t)k * 12;
    float R[9], t[3];
    for (int i = 0; i < 9; i++) R[i] = (float)rel[i];
    for (int i = 0; i < 3; i++) t[i] = (float)rel[9 + i];
    for (int i = 0; i < 3; i++) {
      const float *m = M + i * 4;
      for (int j = 0; j < 3; j++) w[i * 4 + j] = (m[0] * R[j] + m[1] * R[3 + j]) + m[2] * R[6 + j];
      w[i * 4 + 3] = ((m[0] * t[0] + m[1] * t[1]) + m[2] * t[2]) + m[3];
    }
  }
  return SGTD_OK;
}
}  // namespace

extern "C" {

int sgtd_result_world_poses(sgtd_handle e, int q, float *world) {
  if (!e || !world) return SGTD_ERR_INVALID;
  const size_t cn = (size_t)e->cfg.candidate_num;
  std::vector<double> score(cn), pose(cn * 12);
  CHK(sgtd_result_verify(e, q, score.data(), pose.data()));
  return world_poses_of(e, q, pose.data(), [&](int k) { return score[(size_t)k] >= 0.0; }, world);
}

// ---- sgtd_refine_poses: the least-squares refit over every candidate's inlier pairs (refine_kernels.hip.h) ----
int sgtd_refine_poses(sgtd_handle e, int iterations) {
  if (!e || iterations < 1) return SGTD_ERR_INVALID;
  if (e->grp) return multi::refine_poses(e, iterations);
  if (!e->batch_valid || !e->verified) return needs(e, "sgtd_refine_poses", "sgtd_verify");
  HIPCHK(hipSetDevice(e->cfg.device_id));
  CHK(sync_batch(e));
  e->refined = false;
  const int cn = e->dc.cand_num, nq = e->nq;
  if (nq == 0) { e->refined = true; return SGTD_OK; }
  int64_t total = 0;
  for (int q = 0; q < nq; q++) total = std::max<int64_t>(total, (int64_t)e->h_pair_base[q] + e->h_pair_off[(size_t)q * (cn + 1) + cn]);
  const size_t nb = (size_t)nq * cn, half = (size_t)std::max<int64_t>(total, 1);
  CHK(ensure(e, e->r_pose, nb * 12 * sizeof(double)));
  CHK(ensure(e, e->r_rmse, nb * sizeof(double)));
  CHK(ensure(e, e->r_rmse_v, nb * sizeof(double)));
  CHK(ensure(e, e->r_npairs, nb * sizeof(int)));
  CHK(ensure(e, e->r_moments, nb * 15 * sizeof(double)));
  if (iterations > 1) CHK(ensure(e, e->r_flag, 2 * half));
  RefineParams P;
  P.pairs = e->pairs.as<u64>(); P.pair_off = e->pair_off.as<long long>(); P.q_pair_base = e->q_pair_base.as<u32>();
  P.n_cand = e->n_cand.as<int>(); P.cand_num = cn; P.q_stride = e->q_stride;
  P.q_vertex = e->qd.vertex.as<float>(); P.t_vertex = e->tab.vertex.as<float>();
  P.score = e->v_score.as<double>(); P.v_pose = e->v_pose.as<double>(); P.v_inlier = e->v_inlier.as<unsigned char>();
  P.flag = e->r_flag.as<unsigned char>(); P.flag_half = half;
  P.thr2 = 9.0;                 // (verify_enqueue's: sqrt_rn(y) < 3.0 <=> y < 9.0)
  P.iterations = iterations;
  P.order = nullptr; P.n_blocks = (u32)nb;
  P.pose = e->r_pose.as<double>(); P.rmse = e->r_rmse.as<double>(); P.rmse_verify = e->r_rmse_v.as<double>();
  P.n_pairs = e->r_npairs.as<int>(); P.moments = e->r_moments.as<double>();
  if (nb >= 4096 && e->have_frames) CHK(frame_order(e, nb, &P.order));      // (as its verification was dispatched)
  const size_t lds = refine_lds_bytes();
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&refine_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   // (per device)
  refine_kernel<<<(int)nb, SGTD_REFINE_THREADS, lds, e->stream>>>(P);
  HIPCHK(hipGetLastError());
  e->refined = true;
  return SGTD_OK;
}

int sgtd_result_refined(sgtd_handle e, int q, double *pose, double *rmse, double *rmse_verify, int32_t *n_pairs, double *moments) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (!e) return SGTD_ERR_INVALID;
  if (e->grp) return multi::result_refined(e, q, pose, rmse, rmse_verify, n_pairs, moments);
  CHK(result_ready(e, q, e->refined, kNoRefined));
  const size_t cn = (size_t)e->dc.cand_num, o = (size_t)q * cn;
  if (pose) CHK(d2h(e, pose, e->r_pose.as<double>() + o * 12, cn * 12 * sizeof(double)));
  if (rmse) CHK(d2h(e, rmse, e->r_rmse.as<double>() + o, cn * sizeof(double)));
  if (rmse_verify) CHK(d2h(e, rmse_verify, e->r_rmse_v.as<double>() + o, cn * sizeof(double)));
  if (n_pairs) CHK(d2h(e, n_pairs, e->r_npairs.as<int>() + o, cn * sizeof(int)));
  if (moments) CHK(d2h(e, moments, e->r_moments.as<double>() + o * 15, cn * 15 * sizeof(double)));
  CHK(xfer_sync(e));
  return SGTD_OK;
}

int sgtd_result_refined_world_poses(sgtd_handle e, int q, float *world) {
  if (!e || !world) return SGTD_ERR_INVALID;
  const size_t cn = (size_t)e->cfg.candidate_num;
  std::vector<double> pose(cn * 12);
  std::vector<int32_t> np(cn);
  CHK(sgtd_result_refined(e, q, pose.data(), nullptr, nullptr, np.data(), nullptr));
  return world_poses_of(e, q, pose.data(), [&](int k) { return np[(size_t)k] > 0; }, world);     // (a candidate without a result has no pairs)
}

// ---- sgtd_set_frame_keypoints / sgtd_overlap: the keypoint overlap of the verified candidates (overlap_kernels.hip.h) ----
int sgtd_set_frame_keypoints(sgtd_handle e, const uint32_t *frame_ids, const int64_t *kp_off, const float *xyz, const uint32_t *label, int64_t n) {
  if (!e || n < 0 || (n > 0 && !frame_ids)) return SGTD_ERR_INVALID;
  if (n > 0 && xyz && (!kp_off || !label)) return SGTD_ERR_INVALID;
  if (n > 0 && xyz)
    for (int64_t i = 0; i < n; i++)
      if (!keypoint_count_ok(kp_off[i + 1] - kp_off[i])) return SGTD_ERR_INVALID;
  for (int64_t i = 0; i < n; i++)
    if (frame_ids[i] >= (uint32_t)e->cfg.max_frame_n) return SGTD_ERR_FRAME_LIMIT;
  if (e->grp) CHK(multi::set_frame_keypoints(e, frame_ids, kp_off, xyz, label, n));
  if (n == 0) {
    if (frame_ids) return SGTD_OK;
    e->kps.clear(); e->has_kps.clear();
  } else {
    for (int64_t i = 0; i < n; i++) {
      const size_t id = frame_ids[i];
      if (id >= e->has_kps.size()) {
        if (!xyz) continue;
        e->has_kps.resize(id + 1, 0);
        e->kps.resize(id + 1);
      }
      e->has_kps[id] = xyz ? 1 : 0;
      std::vector<uint4> &v = e->kps[id];
      v.clear();
      if (!xyz) { v.shrink_to_fit(); continue; }
      v.resize((size_t)(kp_off[i + 1] - kp_off[i]));
      for (size_t j = 0; j < v.size(); j++) {
        const size_t k = (size_t)kp_off[i] + j;
        u32 b[3];
        std::memcpy(b, xyz + k * 3, sizeof(b));
        v[j] = make_uint4(b[0], b[1], b[2], label[k]);
      }
    }
  }
  static std::atomic<u64> serial{0};
  e->kps_serial = ++serial;
  return SGTD_OK;
}

// the keypoint store's device copy, made again only when the store changed
static int prepare_keypoints(sgtd_engine *e) {
  if (e->kp_word.p && e->kp_dev_serial == e->kps_serial) return SGTD_OK;
  const size_t n_ids = e->has_kps.size();
  e->kp_word_host.assign(std::max<size_t>(n_ids, 1), SGTD_OVERLAP_NONE);
  e->kp_host.clear();
  int mx = 0;
  for (size_t id = 0; id < n_ids; id++) {
    if (!e->has_kps[id]) continue;
    const std::vector<uint4> &v = e->kps[id];
    e->kp_word_host[id] = ((u64)e->kp_host.size() << 16) | (u64)v.size();
    e->kp_host.insert(e->kp_host.end(), v.begin(), v.end());
    mx = std::max(mx, (int)v.size());
  }
  CHK(ensure(e, e->kp_word, e->kp_word_host.size() * sizeof(u64)));
  CHK(ensure(e, e->kp_dev, std::max<size_t>(e->kp_host.size(), 1) * sizeof(uint4)));
  CHK(h2d(e, e->kp_word.p, e->kp_word_host.data(), e->kp_word_host.size() * sizeof(u64)));
  CHK(h2d(e, e->kp_dev.p, e->kp_host.data(), e->kp_host.size() * sizeof(uint4)));
  e->kp_dev_max = mx;
  e->kp_dev_serial = e->kps_serial;
  return SGTD_OK;
}

// the query keypoints of an overlap or alignment pass: the caller's host arrays (copied to the handle's o_q* buffers,
// free at return) or the batch's own.  host_off (or NULL): the nq + 1 offsets, from 0, on the host
static int stage_query_keypoints(sgtd_engine *e, int nq, const float *q_xyz, const uint32_t *q_label, const int64_t *q_kp_off,
                                 const float **d_xyz, const u32 **d_label, const long long **d_off, std::vector<long long> *host_off) {
  if (q_xyz) {
    std::vector<long long> off((size_t)nq + 1);
    for (int q = 0; q <= nq; q++) off[(size_t)q] = q_kp_off[q] - q_kp_off[0];
    const size_t total = (size_t)off[(size_t)nq];
    CHK(ensure(e, e->o_qoff, off.size() * sizeof(long long)));
    CHK(ensure(e, e->o_qxyz, std::max<size_t>(total, 1) * 3 * sizeof(float)));
    CHK(ensure(e, e->o_qlabel, std::max<size_t>(total, 1) * sizeof(u32)));
    CHK(h2d(e, e->o_qoff.p, off.data(), off.size() * sizeof(long long)));
    CHK(h2d(e, e->o_qxyz.p, q_xyz + (size_t)q_kp_off[0] * 3, total * 3 * sizeof(float)));
    CHK(h2d(e, e->o_qlabel.p, q_label + (size_t)q_kp_off[0], total * sizeof(u32)));
    CHK(xfer_sync(e));          // (the offsets' staging vector and the caller's arrays are free at return)
    *d_xyz = e->o_qxyz.as<float>(); *d_label = e->o_qlabel.as<u32>(); *d_off = e->o_qoff.as<long long>();
    if (host_off) host_off->swap(off);
  } else {
    *d_xyz = e->last_xyz; *d_label = e->last_label; *d_off = e->kp_off_dev.as<long long>();
    if (host_off) {
      host_off->resize((size_t)nq + 1);
      CHK(d2h(e, host_off->data(), e->kp_off_dev.p, host_off->size() * sizeof(long long)));
      CHK(xfer_sync(e));
      const long long o0 = (*host_off)[0];
      for (long long &o : *host_off) o -= o0;
    }
  }
  return SGTD_OK;
}

// The head of a keypoint pass (`pass`: its entry point's name) in two parts, the hand-over to a group between them.
// First what holds for both kinds of handle: the arguments, a verified batch (*nq: its queries), the caller's keypoint counts
static int keypoint_pass_args(sgtd_engine *e, const char *pass, double radius, const float *q_xyz, const uint32_t *q_label,
                              const int64_t *q_kp_off, int *nq) {
  if (!(radius >= 0.0) || std::isinf(radius)) return SGTD_ERR_INVALID;
  if (q_xyz && (!q_label || !q_kp_off)) return SGTD_ERR_INVALID;
  if (e->grp) {
    if (multi::nq_of(e, nq) != SGTD_OK) return needs(e, pass, "sgtd_verify");
  } else {
    if (!e->batch_valid || !e->verified) return needs(e, pass, "sgtd_verify");
    *nq = e->nq;
  }
  if (q_xyz)
    for (int q = 0; q < *nq; q++)
      if (!keypoint_count_ok(q_kp_off[q + 1] - q_kp_off[q])) return SGTD_ERR_INVALID;
  return SGTD_OK;
}

// ... then, on a single device: the refit if its poses are asked for (refined_flag: the flag's name, or NULL), keypoints
// to run on, the batch settled; the pass's results (*done) are gone from here on
static int keypoint_pass_begin(sgtd_engine *e, const char *pass, const char *refined_flag, bool own_keypoints, bool *done) {
  if (refined_flag && !e->refined) return needs(e, refined_flag, "sgtd_refine_poses");
  if (own_keypoints && e->last_kind != 1) {
    e->err = std::string("the batch has no keypoints of its own (sgtd_query_descs, sgtd_search_frame): pass them to ") + pass;
    return SGTD_ERR_STATE;
  }
  HIPCHK(hipSetDevice(e->cfg.device_id));
  CHK(sync_batch(e));
  *done = false;
  return SGTD_OK;
}

int sgtd_overlap(sgtd_handle e, double radius, int flags, const float *q_xyz, const uint32_t *q_label, const int64_t *q_kp_off) {
  if (!e || (flags & ~SGTD_OVERLAP_REFINED)) return SGTD_ERR_INVALID;
  int nq = 0;
  CHK(keypoint_pass_args(e, "sgtd_overlap", radius, q_xyz, q_label, q_kp_off, &nq));
  if (e->grp) return multi::overlap(e, radius, flags, q_xyz, q_label, q_kp_off);
  const bool refined = (flags & SGTD_OVERLAP_REFINED) != 0;
  CHK(keypoint_pass_begin(e, "sgtd_overlap", refined ? "SGTD_OVERLAP_REFINED" : nullptr, !q_xyz, &e->overlapped));
  if (nq == 0) { e->overlapped = true; return SGTD_OK; }
  CHK(prepare_keypoints(e));
  const size_t nb = (size_t)nq * e->dc.cand_num;
  CHK(ensure(e, e->o_cnt, nb * sizeof(int4)));
  CHK(ensure(e, e->o_val, nb * sizeof(double2)));
  OverlapParams P;
  keypoint_params(e, refined, radius, nb, &P);
  CHK(stage_query_keypoints(e, nq, q_xyz, q_label, q_kp_off, &P.q_xyz, &P.q_label, &P.q_off, nullptr));
  P.hit_off = (u32)overlap_hit_off(e->kp_dev_max);
  P.cnt = e->o_cnt.as<int4>(); P.val = e->o_val.as<double2>();
  if (nb >= 4096 && e->have_frames) CHK(frame_order(e, nb, &P.order));      // (as its verification was dispatched)
  const size_t lds = overlap_lds_bytes(e->kp_dev_max);
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&overlap_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   // (per device)
  overlap_kernel<<<(int)nb, SGTD_OVERLAP_THREADS, lds, e->stream>>>(P);
  HIPCHK(hipGetLastError());
  e->overlapped = true;
  return SGTD_OK;
}

int sgtd_result_overlap(sgtd_handle e, int q, int32_t *n_query_kp, int32_t *n_frame_kp, int32_t *n_hit_query, int32_t *n_hit_frame,
                        double *overlap, double *rms) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (!e) return SGTD_ERR_INVALID;
  if (e->grp) return multi::result_overlap(e, q, n_query_kp, n_frame_kp, n_hit_query, n_hit_frame, overlap, rms);
  CHK(result_ready(e, q, e->overlapped, kNoOverlap));
  const size_t cn = (size_t)e->dc.cand_num, o = (size_t)q * cn;
  std::vector<int4> cnt(cn);
  std::vector<double2> val(cn);
  CHK(d2h(e, cnt.data(), e->o_cnt.as<int4>() + o, cn * sizeof(int4)));
  CHK(d2h(e, val.data(), e->o_val.as<double2>() + o, cn * sizeof(double2)));
  CHK(xfer_sync(e));
  for (size_t k = 0; k < cn; k++) {
    if (n_query_kp) n_query_kp[k] = cnt[k].x;
    if (n_frame_kp) n_frame_kp[k] = cnt[k].y;
    if (n_hit_query) n_hit_query[k] = cnt[k].z;
    if (n_hit_frame) n_hit_frame[k] = cnt[k].w;
    if (overlap) overlap[k] = val[k].x;
    if (rms) rms[k] = val[k].y;
  }
  return SGTD_OK;
}

// sgtd_search_loop's rule over the candidates whose overlap reaches min_overlap, in host code (one rule for single and
// multi-device handles)
int sgtd_search_loop_overlap(sgtd_handle e, double icp_threshold, double min_overlap, int32_t *best_cand, int32_t *best_frame,
                             double *best_score, double *best_overlap) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (!e) return SGTD_ERR_INVALID;
  const bool gate = min_overlap > 0.0;
  const bool have = e->grp ? multi::has_overlap(e) != 0 : (e->batch_valid && e->verified && e->overlapped);
  if (gate && !have) return needs(e, "sgtd_search_loop_overlap with min_overlap > 0", "sgtd_overlap");
  const int cn = e->cfg.candidate_num;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  int nq = 0;
  std::vector<double> score, ov;
  std::vector<int> n_cand, frames;
  if (e->grp) {
    if (multi::nq_of(e, &nq) != SGTD_OK) return SGTD_ERR_INVALID;
    score.resize((size_t)nq * cn); ov.assign((size_t)nq * cn, nan); n_cand.resize((size_t)nq); frames.resize((size_t)nq * cn);
    for (int q = 0; q < nq; q++) {
      CHK(multi::result_verify(e, q, score.data() + (size_t)q * cn, nullptr));
      CHK(batch_candidates(e, q, &n_cand[(size_t)q], frames.data() + (size_t)q * cn));
      if (have) CHK(multi::result_overlap(e, q, nullptr, nullptr, nullptr, nullptr, ov.data() + (size_t)q * cn, nullptr));
    }
  } else {
    HIPCHK(hipSetDevice(e->cfg.device_id));
    if (!e->verified || !e->batch_valid) return SGTD_ERR_INVALID;
    CHK(sync_batch(e));
    nq = e->nq;
    if (nq == 0) return SGTD_OK;
    const size_t nb = (size_t)nq * cn;
    score.resize(nb); ov.assign(nb, nan);
    std::vector<double2> val(have ? nb : 0);
    CHK(d2h(e, score.data(), e->v_score.p, nb * sizeof(double)));
    if (have) CHK(d2h(e, val.data(), e->o_val.p, nb * sizeof(double2)));
    CHK(xfer_sync(e));
    for (size_t i = 0; i < val.size(); i++) ov[i] = val[i].x;
    n_cand.assign(e->h_n_cand.data(), e->h_n_cand.data() + nq);
    frames.assign(e->h_cand_frame.data(), e->h_cand_frame.data() + nb);
  }
  for (int q = 0; q < nq; q++) {
    double bs = 0;
    int bc = -1;
    for (int c = 0; c < n_cand[(size_t)q]; c++) {
      const size_t i = (size_t)q * cn + c;
      if (gate && !(ov[i] >= min_overlap)) continue;        // (NaN: left out)
      if (score[i] > bs) { bs = score[i]; bc = c; }
    }
    const bool ok = bc >= 0 && bs > icp_threshold;
    if (best_cand) best_cand[q] = ok ? bc : -1;
    if (best_frame) best_frame[q] = ok ? frames[(size_t)q * cn + bc] : -1;
    if (best_score) best_score[q] = ok ? bs : 0.0;
    if (best_overlap) best_overlap[q] = ok ? ov[(size_t)q * cn + bc] : nan;
  }
  return SGTD_OK;
}

// ---- sgtd_align_keypoints: closest-keypoint alignment of the verified candidates (align_kernels.hip.h) ----
int sgtd_align_keypoints(sgtd_handle e, double radius, int iterations, int flags, const float *q_xyz, const uint32_t *q_label,
                         const int64_t *q_kp_off) {
  if (!e || iterations < 1 || (flags & ~SGTD_ALIGN_REFINED)) return SGTD_ERR_INVALID;
  int nq = 0;
  CHK(keypoint_pass_args(e, "sgtd_align_keypoints", radius, q_xyz, q_label, q_kp_off, &nq));
  if (e->grp) return multi::align_keypoints(e, radius, iterations, flags, q_xyz, q_label, q_kp_off);
  const bool refined = (flags & SGTD_ALIGN_REFINED) != 0;
  CHK(keypoint_pass_begin(e, "sgtd_align_keypoints", refined ? "SGTD_ALIGN_REFINED" : nullptr, !q_xyz, &e->aligned));
  const int cn = e->dc.cand_num;
  if (nq == 0) { e->a_qoff.assign(1, 0); e->aligned = true; return SGTD_OK; }
  CHK(prepare_keypoints(e));
  const size_t nb = (size_t)nq * cn;
  AlignParams P;
  CHK(stage_query_keypoints(e, nq, q_xyz, q_label, q_kp_off, &P.q_xyz, &P.q_label, &P.q_off, &e->a_qoff));
  const size_t total = (size_t)e->a_qoff[(size_t)nq];
  CHK(ensure(e, e->a_pose, nb * 12 * sizeof(double)));
  CHK(ensure(e, e->a_fit, nb * sizeof(int4)));
  CHK(ensure(e, e->a_cnt, nb * 2 * sizeof(int4)));
  CHK(ensure(e, e->a_val, nb * 4 * sizeof(double)));
  CHK(ensure(e, e->a_mom, nb * 15 * sizeof(double)));
  CHK(ensure(e, e->a_assign, std::max<size_t>(total * (size_t)cn, 1) * sizeof(int)));
  keypoint_params(e, refined, radius, nb, &P);
  P.hit_off = (u32)align_hit_off(e->kp_dev_max); P.asg_off = (u32)align_asg_off(e->kp_dev_max);
  P.iterations = iterations;
  P.o_pose = e->a_pose.as<double>(); P.fit = e->a_fit.as<int4>(); P.cnt = e->a_cnt.as<int4>(); P.val = e->a_val.as<double>();
  P.moments = e->a_mom.as<double>(); P.assign = e->a_assign.as<int>();
  if (nb >= 4096 && e->have_frames) CHK(frame_order(e, nb, &P.order));      // (as its verification was dispatched)
  const size_t lds = align_lds_bytes(e->kp_dev_max);
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&align_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   // (per device)
  align_kernel<<<(int)nb, SGTD_ALIGN_THREADS, lds, e->stream>>>(P);
  HIPCHK(hipGetLastError());
  e->aligned = true;
  return SGTD_OK;
}

int sgtd_result_aligned(sgtd_handle e, int q, double *pose, int32_t *n_fits, int32_t *n_corr, int32_t *stop, int32_t *counts_before,
                        int32_t *counts_after, double *overlap_before, double *rms_before, double *overlap_after, double *rms_after,
                        double *moments) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (!e) return SGTD_ERR_INVALID;
  if (e->grp) return multi::result_aligned(e, q, pose, n_fits, n_corr, stop, counts_before, counts_after, overlap_before, rms_before, overlap_after, rms_after, moments);
  CHK(result_ready(e, q, e->aligned, kNoAligned));
  const size_t cn = (size_t)e->dc.cand_num, o = (size_t)q * cn;
  std::vector<int4> fit(cn), cnt(cn * 2);
  std::vector<double> val(cn * 4);
  if (pose) CHK(d2h(e, pose, e->a_pose.as<double>() + o * 12, cn * 12 * sizeof(double)));
  if (moments) CHK(d2h(e, moments, e->a_mom.as<double>() + o * 15, cn * 15 * sizeof(double)));
  CHK(d2h(e, fit.data(), e->a_fit.as<int4>() + o, cn * sizeof(int4)));
  CHK(d2h(e, cnt.data(), e->a_cnt.as<int4>() + o * 2, cn * 2 * sizeof(int4)));
  CHK(d2h(e, val.data(), e->a_val.as<double>() + o * 4, cn * 4 * sizeof(double)));
  CHK(xfer_sync(e));
  for (size_t k = 0; k < cn; k++) {
    if (n_fits) n_fits[k] = fit[k].x;
    if (n_corr) n_corr[k] = fit[k].y;
    if (stop) stop[k] = fit[k].z;
    if (counts_before) std::memcpy(counts_before + k * 4, &cnt[k * 2], sizeof(int4));
    if (counts_after) std::memcpy(counts_after + k * 4, &cnt[k * 2 + 1], sizeof(int4));
    if (overlap_before) overlap_before[k] = val[k * 4];
    if (rms_before) rms_before[k] = val[k * 4 + 1];
    if (overlap_after) overlap_after[k] = val[k * 4 + 2];
    if (rms_after) rms_after[k] = val[k * 4 + 3];
  }
  return SGTD_OK;
}

int sgtd_result_aligned_pairs(sgtd_handle e, int q, int cand, int32_t *frame_kp, int64_t capacity, int64_t *n) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (!e || !n) return SGTD_ERR_INVALID;
  if (e->grp) return multi::result_aligned_pairs(e, q, cand, frame_kp, capacity, n);
  CHK(result_ready(e, q, e->aligned, kNoAligned));
  CHK(sync_batch(e));
  if (cand < 0 || cand >= e->h_n_cand[(size_t)q]) return SGTD_ERR_INVALID;
  const int64_t nqk = e->a_qoff[(size_t)q + 1] - e->a_qoff[(size_t)q];
  *n = nqk;
  const int64_t take = frame_kp ? std::min<int64_t>(nqk, std::max<int64_t>(capacity, 0)) : 0;
  if (take > 0) {
    const size_t at = (size_t)e->a_qoff[(size_t)q] * (size_t)e->dc.cand_num + (size_t)cand * (size_t)nqk;
    CHK(d2h(e, frame_kp, e->a_assign.as<int>() + at, (size_t)take * sizeof(int)));
    CHK(xfer_sync(e));
  }
  return (frame_kp && nqk > capacity) ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int sgtd_result_aligned_world_poses(sgtd_handle e, int q, float *world) {
  if (!e || !world) return SGTD_ERR_INVALID;
  const size_t cn = (size_t)e->cfg.candidate_num;
  std::vector<double> pose(cn * 12);
  std::vector<int32_t> stop(cn);
  CHK(sgtd_result_aligned(e, q, pose.data(), nullptr, nullptr, stop.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  return world_poses_of(e, q, pose.data(), [&](int k) { return stop[(size_t)k] >= 0; }, world);     // (stop -1: a candidate without a result)
}

// the lowest registration fitness among the candidates that pass the bounds, in host code over the public results (one
// rule for single and multi-device handles)
int sgtd_search_loop_aligned(sgtd_handle e, double min_overlap, double max_rms, int32_t *best_cand, int32_t *best_frame,
                             double *best_rms, double *best_overlap) {
  if (!e || std::isnan(min_overlap) || std::isnan(max_rms)) return SGTD_ERR_INVALID;
  const bool have = e->grp ? multi::has_aligned(e) != 0 : (e->batch_valid && e->verified && e->aligned);
  if (!have) return needs(e, "sgtd_search_loop_aligned", "sgtd_align_keypoints");
  const int cn = e->cfg.candidate_num;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const bool gate_ov = min_overlap > 0.0, gate_rms = max_rms > 0.0 && !std::isinf(max_rms);
  int nq = 0;
  if (e->grp) CHK(multi::nq_of(e, &nq)); else nq = e->nq;
  std::vector<double> score((size_t)cn), ov((size_t)cn), rms((size_t)cn);
  std::vector<int32_t> stop((size_t)cn);
  std::vector<int> frames((size_t)cn);
  for (int q = 0; q < nq; q++) {
    int n_cand = 0;
    CHK(sgtd_result_verify(e, q, score.data(), nullptr));
    CHK(sgtd_result_aligned(e, q, nullptr, nullptr, nullptr, stop.data(), nullptr, nullptr, nullptr, nullptr, ov.data(), rms.data(), nullptr));
    CHK(batch_candidates(e, q, &n_cand, frames.data()));       // (settled and current: the two getters above looked)
    int bc = -1;
    for (int c = 0; c < n_cand; c++) {
      if (stop[(size_t)c] < 0 || std::isnan(rms[(size_t)c])) continue;
      if (gate_ov && !(ov[(size_t)c] >= min_overlap)) continue;         // (NaN: left out)
      if (gate_rms && !(rms[(size_t)c] <= max_rms)) continue;
      if (bc < 0 || rms[(size_t)c] < rms[(size_t)bc] || (rms[(size_t)c] == rms[(size_t)bc] && score[(size_t)c] > score[(size_t)bc])) bc = c;
    }
    if (best_cand) best_cand[q] = bc;
    if (best_frame) best_frame[q] = bc >= 0 ? frames[(size_t)bc] : -1;
    if (best_rms) best_rms[q] = bc >= 0 ? rms[(size_t)bc] : nan;
    if (best_overlap) best_overlap[q] = bc >= 0 ? ov[(size_t)bc] : nan;
  }
  return SGTD_OK;
}

int sgtd_host_alloc(size_t bytes, void **out) {
  if (!out) return SGTD_ERR_INVALID;
  *out = nullptr;
  if (bytes == 0) return SGTD_OK;
  return hipHostMalloc(out, bytes, hipHostMallocPortable) == hipSuccess ? SGTD_OK : SGTD_ERR_HIP;
}

int sgtd_host_free(void *p) {
  if (!p) return SGTD_OK;
  return hipHostFree(p) == hipSuccess ? SGTD_OK : SGTD_ERR_INVALID;
}

int sgtd_fetch_entries(sgtd_handle e, const int64_t *db_entry, int64_t n, sgtd_desc_soa *out) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (e && e->grp) return multi::fetch_entries(e, db_entry, n, out);
  if (!e || n < 0 || (n > 0 && (!db_entry || !out))) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  CHK(view_current(e));
  if (n == 0) return SGTD_OK;
  bool contiguous = true;
  for (int64_t i = 0; i < n; i++) {
    if (db_entry[i] < 0 || db_entry[i] >= e->n_entries) return SGTD_ERR_INVALID;
    if (i && db_entry[i] != db_entry[i - 1] + 1) contiguous = false;
  }
  if (contiguous) return copy_out(e, e->tab, (size_t)db_entry[0], (size_t)n, out, 0);
  // scattered ids (a match list): gathered on the device, then one copy per field
  CHK(ensure(e, e->fetch_idx, (size_t)n * sizeof(long long)));
  CHK(ensure_store(e, e->fetch, (size_t)n));
  CHK(h2d(e, e->fetch_idx.p, db_entry, (size_t)n * sizeof(long long)));
  gather_entries_kernel<<<grid_for(n, 256), 256, 0, e->stream>>>(e->fetch_idx.as<long long>(), n, e->tab.view(), e->fetch.view());
  HIPCHK(hipGetLastError());
  return copy_out(e, e->fetch, 0, (size_t)n, out, 0);
}

int sgtd_table_dump(sgtd_handle e, int64_t *keys, int64_t *bucket_off, int64_t *entry_ids,
                    int64_t cap_buckets, int64_t cap_entries) {
  PinScope pin_scope(e && !e->grp ? e : nullptr);
  if (e && e->grp) { e->err = "not available on a multi-device handle (use the per-device form, sgtd_amd/dist.py)"; return SGTD_ERR_UNSUPPORTED; }
  if (!e) return SGTD_ERR_INVALID;
  HIPCHK(hipSetDevice(e->cfg.device_id));
  if (e->attached_to && e->n_seg > 1) { e->err = "dump the table through its owner"; return SGTD_ERR_STATE; }
  CHK(do_finalize(e, /*force_merge=*/true));   // one segment: the dump shows whole buckets
  const sgtd_engine::Segment &S = e->seg[0];
  const int64_t U = S.n_buckets, E = e->n_entries;
  if (U > cap_buckets || E > cap_entries) return SGTD_ERR_CAPACITY;
  if (E == 0) { if (bucket_off) bucket_off[0] = 0; return SGTD_OK; }
  std::vector<u64> k(U);
  std::vector<u32> st(U), pm(E);
  HIPCHK(hipMemcpy(k.data(), S.bucket_key.p, U * sizeof(u64), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(st.data(), S.bucket_start.p, U * sizeof(u32), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(pm.data(), S.perm.p, E * sizeof(u32), hipMemcpyDeviceToHost));
  for (int64_t u = 0; u < U; u++) {
    if (keys) {
      keys[u * 4 + 0] = (int64_t)((k[u] >> 32) & 0xFFFF);
      keys[u * 4 + 1] = (int64_t)((k[u] >> 16) & 0xFFFF);
      keys[u * 4 + 2] = (int64_t)(k[u] & 0xFFFF);
      keys[u * 4 + 3] = (int64_t)(k[u] >> 48);
    }
    if (bucket_off) bucket_off[u] = st[u];
  }
  if (bucket_off) bucket_off[U] = E;
  if (entry_ids) {
    // the probe layout keeps every bucket partitioned by slice; the dump shows each bucket in
    // insertion order (ascending entry id), the order of the reference's bucket vector
    for (int64_t u = 0; u < U; u++) {
      const int64_t lo = st[u], hi = (u + 1 < U) ? (int64_t)st[u + 1] : E;
      std::sort(pm.begin() + lo, pm.begin() + hi);
    }
    for (int64_t p = 0; p < E; p++) entry_ids[p] = pm[p];
  }
  return SGTD_OK;
}

}  // extern "C"

// ---- sgtd_consistent_loops: pairwise consistency over a list of loop closures and the greedy clique
// (consistency_kernels.hip.h) ----
namespace {
const char kNoConsistency[] = "no consistency results: sgtd_consistent_loops has not run";

// the pose store `owner` holds (its own handle's, or the group's), copied to c's device when it changed
int cons_upload_store(sgtd_engine *c, const sgtd_engine *owner) {
  if (c->ck_store.p && c->ck_store_serial == owner->poses_serial) return SGTD_OK;
  const size_t n_ids = owner->has_pose.size();
  CHK(ensure(c, c->ck_store, std::max<size_t>(n_ids, 1) * 12 * sizeof(float)));
  CHK(ensure(c, c->ck_has, std::max<size_t>(n_ids, 1)));
  CHK(h2d(c, c->ck_store.p, owner->poses.data(), n_ids * 12 * sizeof(float)));
  CHK(h2d(c, c->ck_has.p, owner->has_pose.data(), n_ids));
  CHK(xfer_sync(c));
  c->ck_store_serial = owner->poses_serial;
  return SGTD_OK;
}

int cons_run(sgtd_engine *c, const sgtd_engine *owner, int n, const uint32_t *frame_a, const uint32_t *frame_b, const double *rel_pose,
             const float *pose_a, double tt, double min_trace, int32_t *n_set) {
  sgtd_engine *e = c;      // (HIPCHK reports on the engine that runs the pass)
  CHK(cons_upload_store(c, owner));
  const u32 words = (u32)((n + 63) / 64);
  const size_t ns = (size_t)words * 64;
  // the call's inputs, back to back: rel_pose, pose_a, frame_b, frame_a
  const size_t o_rel = 0, o_pa = o_rel + (size_t)n * 12 * sizeof(double), o_fb = o_pa + (pose_a ? (size_t)n * 12 * sizeof(float) : 0),
               o_fa = o_fb + (size_t)n * sizeof(u32), in_bytes = o_fa + (frame_a ? (size_t)n * sizeof(u32) : 0);
  CHK(ensure(c, c->ck_in, in_bytes));
  CHK(ensure(c, c->ck_soa, (size_t)SGTD_CONS_STREAMS * ns * sizeof(double)));
  CHK(ensure(c, c->ck_valid, ns));
  CHK(ensure(c, c->ck_rows, (size_t)n * words * sizeof(u64)));
  CHK(ensure(c, c->ck_pmask, (size_t)words * sizeof(u64)));
  CHK(ensure(c, c->ck_out, (size_t)n * 3 * sizeof(int)));
  CHK(ensure(c, c->ck_state, sizeof(ConsState)));
  if (c->timing)
    for (hipEvent_t &ev : c->ck_ev)
      if (!ev) HIPCHK(hipEventCreate(&ev));
  char *in = c->ck_in.as<char>();
  CHK(h2d(c, in + o_rel, rel_pose, (size_t)n * 12 * sizeof(double)));
  if (pose_a) CHK(h2d(c, in + o_pa, pose_a, (size_t)n * 12 * sizeof(float)));
  CHK(h2d(c, in + o_fb, frame_b, (size_t)n * sizeof(u32)));
  if (frame_a) CHK(h2d(c, in + o_fa, frame_a, (size_t)n * sizeof(u32)));

  ConsPrepareParams pp;
  pp.store = c->ck_store.as<float>(); pp.has = c->ck_has.as<unsigned char>(); pp.n_ids = (u32)owner->has_pose.size();
  pp.frame_a = frame_a ? reinterpret_cast<const u32 *>(in + o_fa) : nullptr;
  pp.frame_b = reinterpret_cast<const u32 *>(in + o_fb);
  pp.rel = reinterpret_cast<const double *>(in + o_rel);
  pp.pose_a = pose_a ? reinterpret_cast<const float *>(in + o_pa) : nullptr;
  pp.n = n; pp.ns = ns; pp.soa = c->ck_soa.as<double>(); pp.valid = c->ck_valid.as<unsigned char>();
  cons_prepare_kernel<<<grid_for(n, SGTD_CONS_THREADS), SGTD_CONS_THREADS, 0, c->stream>>>(pp);
  HIPCHK(hipGetLastError());

  if (c->timing) HIPCHK(hipEventRecord(c->ck_ev[0], c->stream));
  ConsPairParams pr;
  pr.soa = pp.soa; pr.ns = ns; pr.valid = pp.valid; pr.n = n; pr.words = words; pr.tt = tt; pr.min_trace = min_trace;
  pr.rows = c->ck_rows.as<u64>();
  const dim3 pgrid((words + SGTD_CONS_TILE / SGTD_WAVE - 1) / (SGTD_CONS_TILE / SGTD_WAVE), (u32)grid_for(n, SGTD_CONS_ROWS));
  cons_pair_kernel<<<pgrid, SGTD_CONS_THREADS, 0, c->stream>>>(pr);
  HIPCHK(hipGetLastError());
  if (c->timing) HIPCHK(hipEventRecord(c->ck_ev[1], c->stream));

  int *in_set = c->ck_out.as<int>(), *degree = in_set + n, *pick = degree + n;
  ConsState *st = c->ck_state.as<ConsState>();
  HIPCHK(hipMemsetAsync(st, 0, sizeof(ConsState), c->stream));
  cons_init_kernel<<<grid_for((long long)words * SGTD_WAVE, SGTD_CONS_THREADS), SGTD_CONS_THREADS, 0, c->stream>>>(
      pp.valid, n, words, c->ck_pmask.as<u64>(), in_set, degree, pick, st);
  HIPCHK(hipGetLastError());
  // rounds in groups that fall through once the choice is complete; the state is read once per group
  const int cgrid = std::min(grid_for(n, SGTD_CONS_THREADS / SGTD_WAVE), 4 * c->n_cus);
  ConsState host{};
  int group = 16, rounds_sent = 0;
  for (;;) {
    for (int r = 0; r < group; r++) {
      cons_count_kernel<<<cgrid, SGTD_CONS_THREADS, 0, c->stream>>>(pr.rows, c->ck_pmask.as<u64>(), n, words, degree, st);
      cons_select_kernel<<<1, SGTD_CONS_SELECT_THREADS, 0, c->stream>>>(pr.rows, c->ck_pmask.as<u64>(), words, in_set, pick, st);
    }
    HIPCHK(hipGetLastError());
    rounds_sent += group;
    CHK(d2h(c, &host, st, sizeof(ConsState)));
    if (c->timing) HIPCHK(hipEventRecord(c->ck_ev[2], c->stream));
    CHK(xfer_sync(c));
    if (host.done) break;
    if (rounds_sent > n + 16) { c->err = "sgtd_consistent_loops: the greedy choice did not end"; return SGTD_ERR_HIP; }   // (a round removes its pick from P)
    group = std::min(group * 2, 256);
  }
  c->stats.consistency_rounds = host.round;
  c->stats.ms_consistency_pairs = c->stats.ms_consistency_greedy = 0.f;
  if (c->timing) {
    HIPCHK(hipEventElapsedTime(&c->stats.ms_consistency_pairs, c->ck_ev[0], c->ck_ev[1]));
    HIPCHK(hipEventElapsedTime(&c->stats.ms_consistency_greedy, c->ck_ev[1], c->ck_ev[2]));
  }
  *n_set = host.n_set;
  return SGTD_OK;
}
}  // namespace

extern "C" {

int sgtd_consistent_loops(sgtd_handle e, int64_t n, const uint32_t *frame_a, const uint32_t *frame_b, const double *rel_pose,
                          const float *pose_a, double max_trans, double max_rot, int32_t *n_set) {
  if (!e || n < 0 || !n_set) return SGTD_ERR_INVALID;
  if (n > 0 && (!frame_b || !rel_pose || (!frame_a && !pose_a))) return SGTD_ERR_INVALID;
  if (!(max_trans >= 0.0) || std::isinf(max_trans)) return SGTD_ERR_INVALID;
  if (!(max_rot >= 0.0 && max_rot <= 3.14159265358979323846)) return SGTD_ERR_INVALID;
  StageRun<int64_t> run(e, &sgtd_engine::ck_n);
  if (n > SGTD_MAX_LOOP_EDGES) {
    e->err = "sgtd_consistent_loops takes at most " + std::to_string(SGTD_MAX_LOOP_EDGES) + " edges in one call (" + std::to_string(n) + " given)";
    return SGTD_ERR_UNSUPPORTED;
  }
  const double tt = max_trans * max_trans, min_trace = 1.0 + 2.0 * std::cos(max_rot);
  *n_set = 0;
  if (n > 0) run.on_device([&](sgtd_engine *c) { return cons_run(c, e, (int)n, frame_a, frame_b, rel_pose, pose_a, tt, min_trace, n_set); });
  if (run.st == SGTD_OK) { run.c->ck_thr[0] = tt; run.c->ck_thr[1] = min_trace; }
  return run.end(n);
}

int sgtd_result_consistent(sgtd_handle e, int32_t *in_set, int32_t *degree, int32_t *pick, double *thresholds) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::ck_n, kNoConsistency, &c));
  if (thresholds) { thresholds[0] = c->ck_thr[0]; thresholds[1] = c->ck_thr[1]; }
  const size_t n = (size_t)c->ck_n;
  if (n == 0) return SGTD_OK;
  CopyOut out(e, c);
  const int *d = c->ck_out.as<int>();
  out.get(in_set, d, n * sizeof(int));
  out.get(degree, d + n, n * sizeof(int));
  out.get(pick, d + 2 * n, n * sizeof(int));
  return out.finish();
}

int sgtd_result_consistency_rows(sgtd_handle e, int64_t first, int64_t n_rows, uint64_t *rows) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::ck_n, kNoConsistency, &c));
  if (first < 0 || n_rows < 0 || first > c->ck_n || n_rows > c->ck_n - first || (n_rows > 0 && !rows)) return SGTD_ERR_INVALID;
  if (n_rows == 0) return SGTD_OK;
  const size_t words = (size_t)((c->ck_n + 63) / 64);
  CopyOut out(e, c);      // (rows of more than kPinMax bytes take d2h's direct copy: the staging bounds nothing)
  out.get(rows, c->ck_rows.as<u64>() + (size_t)first * words, (size_t)n_rows * words * sizeof(u64));
  return out.finish();
}

int sgtd_result_loop_edges(sgtd_handle e, double icp_threshold, int flags, int32_t *query, uint32_t *frame_a, uint32_t *frame_b,
                           double *rel_pose, double *score, int64_t capacity, int64_t *n_edges) {
  if (!e || !n_edges || capacity < 0 || (flags & ~SGTD_LOOP_EDGES_REFINED)) return SGTD_ERR_INVALID;
  const bool refined = (flags & SGTD_LOOP_EDGES_REFINED) != 0;
  const bool have_v = e->grp ? (e->grp->batch_valid && e->grp->verified) : (e->batch_valid && e->verified);
  if (!have_v) return needs(e, "sgtd_result_loop_edges", "sgtd_verify");
  if (refined && !(e->grp ? e->grp->refined : e->refined)) return needs(e, "SGTD_LOOP_EDGES_REFINED", "sgtd_refine_poses");
  const int nq = e->grp ? e->grp->nq : e->nq;
  const size_t cn = (size_t)e->cfg.candidate_num;
  std::vector<int32_t> cand((size_t)std::max(nq, 1)), frame((size_t)std::max(nq, 1));
  std::vector<double> best((size_t)std::max(nq, 1)), pose(cn * 12);
  CHK(sgtd_search_loop(e, icp_threshold, cand.data(), frame.data(), best.data()));
  int64_t m = 0;
  for (int q = 0; q < nq; q++) {
    if (cand[(size_t)q] < 0) continue;
    if (m < capacity) {
      if (rel_pose) {
        if (refined) CHK(sgtd_result_refined(e, q, pose.data(), nullptr, nullptr, nullptr, nullptr));
        else CHK(sgtd_result_verify(e, q, nullptr, pose.data()));
        std::memcpy(rel_pose + (size_t)m * 12, pose.data() + (size_t)cand[(size_t)q] * 12, 12 * sizeof(double));
      }
      if (query) query[m] = q;
      // the frame id the query's descriptors carry: c + q for a sgtd_loop_frames batch, current_frame_id_ otherwise
      if (frame_a) frame_a[m] = e->grp ? e->grp->current_frame_id : (e->last_kind == 1 ? e->last_qframe + (e->loop_batch ? (u32)q : 0u) : e->current_frame_id);
      if (frame_b) frame_b[m] = (uint32_t)frame[(size_t)q];
      if (score) score[m] = best[(size_t)q];
    }
    m++;
  }
  *n_edges = m;
  return m > capacity ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int sgtd_get_stats(sgtd_handle e, sgtd_stats *out) {
  if (e && e->grp) return multi::get_stats(e, out);
  if (!e || !out) return SGTD_ERR_INVALID;
  e->stats.n_entries = e->n_entries;
  e->stats.n_buckets = e->seg[0].n_buckets + (e->n_seg > 1 ? e->seg[1].n_buckets : 0);
  e->stats.n_frames = e->n_add_calls;
  e->stats.hbm_bytes_table = e->n_entries * (int64_t)SGTD_HOT_BYTES;
  e->stats.bucket_len_sq_over_E = e->n_entries > 0 ? (e->seg[0].sum_len_sq + (e->n_seg > 1 ? e->seg[1].sum_len_sq : 0.0)) / (double)e->n_entries : 0.0;
  e->stats.ms_finalize = e->ms_finalize;
  e->stats.tail_entries = e->n_seg > 1 ? e->seg[1].g1 - e->seg[1].g0 : 0;
  *out = e->stats;
  return SGTD_OK;
}

}  // extern "C"

// ---- sgtd_pose_consensus: per query, the consistent set of its verified candidates and their fused pose
// (consensus_kernels.hip.h) ----
namespace {
// cs_out: the 8-byte outputs first
struct ConsensusLayout {
  size_t pose, figs, mask, rows, counts, degree, pick, total;
  ConsensusLayout(size_t nq, size_t cn) {
    pose = 0; figs = pose + nq * 12 * sizeof(double); mask = figs + nq * 3 * sizeof(double); rows = mask + nq * sizeof(u64);
    counts = rows + nq * cn * sizeof(u64); degree = counts + nq * 3 * sizeof(int); pick = degree + nq * cn * sizeof(int);
    total = pick + nq * cn * sizeof(int);
  }
};

bool consensus_bounds_ok(double max_trans, double max_rot) {
  return max_trans >= 0.0 && !std::isinf(max_trans) && max_rot >= 0.0 && max_rot <= 3.14159265358979323846;
}

bool have_verified(const sgtd_engine *e) { return e->grp ? (e->grp->batch_valid && e->grp->verified) : (e->batch_valid && e->verified); }

// one launch over nq queries whose candidates, scores and poses are on c's device; owner: whose pose store is used
int consensus_launch(sgtd_engine *c, const sgtd_engine *owner, int nq, int cn, const int *d_n_cand, const int *d_cand_frame,
                     const double *d_score, const double *d_rel, double tt, double min_trace) {
  sgtd_engine *e = c;
  CHK(cons_upload_store(c, owner));
  const ConsensusLayout L((size_t)nq, (size_t)cn);
  CHK(ensure(c, c->cs_out, L.total));
  char *out = c->cs_out.as<char>();
  ConsensusParams P;
  P.store = c->ck_store.as<float>(); P.has = c->ck_has.as<unsigned char>(); P.n_ids = (u32)owner->has_pose.size();
  P.n_cand = d_n_cand; P.cand_frame = d_cand_frame; P.score = d_score; P.rel = d_rel; P.cn = cn; P.tt = tt; P.min_trace = min_trace;
  P.pose = reinterpret_cast<double *>(out + L.pose); P.figs = reinterpret_cast<double *>(out + L.figs);
  P.mask = reinterpret_cast<u64 *>(out + L.mask); P.rows = reinterpret_cast<u64 *>(out + L.rows);
  P.counts = reinterpret_cast<int *>(out + L.counts); P.degree = reinterpret_cast<int *>(out + L.degree);
  P.pick = reinterpret_cast<int *>(out + L.pick);
  consensus_kernel<<<nq, SGTD_WAVE, 0, c->stream>>>(P);
  HIPCHK(hipGetLastError());
  return SGTD_OK;
}

// the rows form: the caller's host arrays go to c's device first; the host waits for the pass
int consensus_rows_run(sgtd_engine *c, const sgtd_engine *owner, int nq, int cn, const int32_t *n_cand, const int32_t *cand_frame,
                       const double *score, const double *rel_pose, double tt, double min_trace) {
  const size_t nb = (size_t)nq * cn;
  const size_t o_rel = 0, o_score = o_rel + nb * 12 * sizeof(double), o_frame = o_score + nb * sizeof(double),
               o_n = o_frame + nb * sizeof(int), in_bytes = o_n + (size_t)nq * sizeof(int);
  CHK(ensure(c, c->cs_in, in_bytes));
  char *in = c->cs_in.as<char>();
  CHK(h2d(c, in + o_rel, rel_pose, nb * 12 * sizeof(double)));
  CHK(h2d(c, in + o_score, score, nb * sizeof(double)));
  CHK(h2d(c, in + o_frame, cand_frame, nb * sizeof(int)));
  CHK(h2d(c, in + o_n, n_cand, (size_t)nq * sizeof(int)));
  CHK(consensus_launch(c, owner, nq, cn, reinterpret_cast<const int *>(in + o_n), reinterpret_cast<const int *>(in + o_frame),
                       reinterpret_cast<const double *>(in + o_score), reinterpret_cast<const double *>(in + o_rel), tt, min_trace));
  return xfer_sync(c);
}

// the relative poses of query q's candidates the flag names (the stage has run: the caller has checked)
int consensus_batch_pose(sgtd_engine *e, int q, int flags, double *pose) {
  if (flags & SGTD_CONSENSUS_REFINED) return sgtd_result_refined(e, q, pose, nullptr, nullptr, nullptr, nullptr);
  if (flags & SGTD_CONSENSUS_ALIGNED)
    return sgtd_result_aligned(e, q, pose, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  return sgtd_result_verify(e, q, nullptr, pose);
}

// the pending batch's candidate frames and verify scores on the host, [nq * cn] each
int consensus_batch_scores(sgtd_engine *e, int nq, std::vector<int> *frame, std::vector<double> *score) {
  const size_t cn = (size_t)e->cfg.candidate_num;
  frame->assign((size_t)nq * cn, -1);
  score->assign((size_t)nq * cn, -1.0);
  if (nq == 0) return SGTD_OK;
  if (!e->grp) {
    HIPCHK(hipSetDevice(e->cfg.device_id));
    CHK(sync_batch(e));
    std::memcpy(frame->data(), e->h_cand_frame.data(), (size_t)nq * cn * sizeof(int));
    CHK(d2h(e, score->data(), e->v_score.as<double>(), (size_t)nq * cn * sizeof(double)));
    return xfer_sync(e);
  }
  int n_cand = 0;
  for (int q = 0; q < nq; q++) {
    CHK(batch_candidates(e, q, &n_cand, frame->data() + (size_t)q * cn));
    CHK(sgtd_result_verify(e, q, score->data() + (size_t)q * cn, nullptr));
  }
  return SGTD_OK;
}

// the getters' state checks; *out: the engine that holds the results
int consensus_ready(sgtd_engine *e, sgtd_engine **out) {
  sgtd_engine *c = home_engine(e);
  if (c->cs_n >= 0 && c->cs_batch && !have_verified(e)) c->cs_n = -1;      // (the batch went without a new one)
  return stage_ready(e, &sgtd_engine::cs_n, "no consensus results: sgtd_pose_consensus has not run (or its batch has gone)", out);
}

// sgtd_search_loop_consensus' choice for every query of the batch form's results: cand, frame, score [nq] (-1, -1, 0
// where the set is smaller than min_support) and n_set
int consensus_choice(sgtd_engine *e, int min_support, std::vector<int32_t> *cand, std::vector<int32_t> *frame, std::vector<double> *best,
                     std::vector<int32_t> *n_set) {
  sgtd_engine *c = nullptr;
  CHK(consensus_ready(e, &c));
  if (!c->cs_batch) { e->err = "the consensus results are those of sgtd_pose_consensus_rows: the choice needs the batch form"; return SGTD_ERR_STATE; }
  const int nq = (int)c->cs_n;
  const size_t cn = (size_t)c->cs_cn;
  cand->assign((size_t)nq, -1); frame->assign((size_t)nq, -1); best->assign((size_t)nq, 0.0); n_set->assign((size_t)nq, 0);
  if (nq == 0) return SGTD_OK;
  std::vector<uint64_t> mask((size_t)nq);
  CHK(sgtd_result_consensus(e, 0, nq, nullptr, nullptr, n_set->data(), nullptr, mask.data(), nullptr, nullptr, nullptr, nullptr));
  std::vector<int> frames;
  std::vector<double> scores;
  CHK(consensus_batch_scores(e, nq, &frames, &scores));
  for (int q = 0; q < nq; q++) {
    if ((*n_set)[(size_t)q] < min_support) continue;
    int bk = -1;
    double bs = 0.0;
    for (u64 b = mask[(size_t)q]; b; b &= b - 1) {
      const int k = __builtin_ctzll(b);
      const double s = scores[(size_t)q * cn + k];
      if (bk < 0 || s > bs) { bk = k; bs = s; }
    }
    if (bk < 0) continue;
    (*cand)[(size_t)q] = bk; (*frame)[(size_t)q] = frames[(size_t)q * cn + bk]; (*best)[(size_t)q] = bs;
  }
  return SGTD_OK;
}
}  // namespace

extern "C" {

int sgtd_pose_consensus_rows(sgtd_handle e, int64_t n_queries, int cand_num, const int32_t *n_cand, const int32_t *cand_frame,
                             const double *score, const double *rel_pose, double max_trans, double max_rot) {
  if (!e) return SGTD_ERR_INVALID;
  StageRun<int64_t> run(e, &sgtd_engine::cs_n);
  if (n_queries < 0 || cand_num < 1 || cand_num > SGTD_MAX_CAND || !consensus_bounds_ok(max_trans, max_rot)) return SGTD_ERR_INVALID;
  if (n_queries > 0 && (!n_cand || !cand_frame || !score || !rel_pose)) return SGTD_ERR_INVALID;
  if (n_queries > 0x7FFFFFFF / SGTD_MAX_CAND) {
    e->err = "sgtd_pose_consensus_rows takes at most " + std::to_string(0x7FFFFFFF / SGTD_MAX_CAND) + " queries in one call";
    return SGTD_ERR_UNSUPPORTED;
  }
  const double tt = max_trans * max_trans, min_trace = 1.0 + 2.0 * std::cos(max_rot);
  if (n_queries > 0)
    run.on_device([&](sgtd_engine *c) { return consensus_rows_run(c, e, (int)n_queries, cand_num, n_cand, cand_frame, score, rel_pose, tt, min_trace); });
  if (run.st == SGTD_OK) { run.c->cs_thr[0] = tt; run.c->cs_thr[1] = min_trace; run.c->cs_cn = cand_num; run.c->cs_batch = false; }
  return run.end(n_queries);
}

int sgtd_pose_consensus(sgtd_handle e, double max_trans, double max_rot, int flags) {
  if (!e) return SGTD_ERR_INVALID;
  StageRun<int64_t> run(e, &sgtd_engine::cs_n);
  if ((flags & ~(SGTD_CONSENSUS_REFINED | SGTD_CONSENSUS_ALIGNED)) || flags == (SGTD_CONSENSUS_REFINED | SGTD_CONSENSUS_ALIGNED)) return SGTD_ERR_INVALID;
  if (!consensus_bounds_ok(max_trans, max_rot)) return SGTD_ERR_INVALID;
  if (!have_verified(e)) return needs(e, "sgtd_pose_consensus", "sgtd_verify");
  if ((flags & SGTD_CONSENSUS_REFINED) && !(e->grp ? e->grp->refined : e->refined)) return needs(e, "SGTD_CONSENSUS_REFINED", "sgtd_refine_poses");
  if ((flags & SGTD_CONSENSUS_ALIGNED) && !(e->grp ? e->grp->aligned : e->aligned)) return needs(e, "SGTD_CONSENSUS_ALIGNED", "sgtd_align_keypoints");
  const double tt = max_trans * max_trans, min_trace = 1.0 + 2.0 * std::cos(max_rot);
  const int cn = e->cfg.candidate_num, nq = e->grp ? e->grp->nq : e->nq;
  if (e->grp) {
    // every candidate's result from its owner, then the rows form on the first device with the group's poses
    const size_t nb = (size_t)std::max(nq, 1) * cn;
    std::vector<int32_t> n_cand((size_t)std::max(nq, 1)), frame(nb);
    std::vector<double> score(nb), pose(nb * 12);
    for (int q = 0; q < nq; q++) {
      CHK(batch_candidates(e, q, &n_cand[(size_t)q], frame.data() + (size_t)q * cn));
      CHK(sgtd_result_verify(e, q, score.data() + (size_t)q * cn, nullptr));
      CHK(consensus_batch_pose(e, q, flags, pose.data() + (size_t)q * cn * 12));
    }
    // (the gather above left the device of a candidate's owner selected: on_device selects the first again)
    if (nq > 0)
      run.on_device([&](sgtd_engine *c) { return consensus_rows_run(c, e, nq, cn, n_cand.data(), frame.data(), score.data(), pose.data(), tt, min_trace); });
  } else {
    run.on_device([&](sgtd_engine *) -> int {
      CHK(view_current(e));
      const double *rel = (flags & SGTD_CONSENSUS_REFINED) ? e->r_pose.as<double>() : (flags & SGTD_CONSENSUS_ALIGNED) ? e->a_pose.as<double>() : e->v_pose.as<double>();
      // the batch's candidates, scores and poses are read where the earlier stages left them: nothing travels
      if (nq > 0) CHK(consensus_launch(e, e, nq, cn, e->n_cand.as<int>(), e->cand_frame.as<int>(), e->v_score.as<double>(), rel, tt, min_trace));
      return SGTD_OK;
    });
  }
  if (run.st == SGTD_OK) { run.c->cs_thr[0] = tt; run.c->cs_thr[1] = min_trace; run.c->cs_cn = cn; run.c->cs_batch = true; }
  return run.end(nq);
}

int sgtd_result_consensus(sgtd_handle e, int64_t first, int64_t n, double *pose, int32_t *n_valid, int32_t *n_set, int32_t *seed,
                          uint64_t *mask, double *support_score, double *spread_t2, double *spread_trace, double *thresholds) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(consensus_ready(e, &c));
  if (first < 0 || n < 0 || first > c->cs_n || n > c->cs_n - first) return SGTD_ERR_INVALID;
  if (thresholds) { thresholds[0] = c->cs_thr[0]; thresholds[1] = c->cs_thr[1]; }
  if (n == 0) return SGTD_OK;
  const ConsensusLayout L((size_t)c->cs_n, (size_t)c->cs_cn);
  const char *dev = c->cs_out.as<char>();
  const size_t f = (size_t)first, m = (size_t)n;
  // (the figures and the counts come interleaved: through a host copy, where the caller asks for any of them)
  std::vector<double> figs(support_score || spread_t2 || spread_trace ? m * 3 : 0);
  std::vector<int> counts(n_valid || n_set || seed ? m * 3 : 0);
  CopyOut out(e, c);
  out.get(pose, dev + L.pose + f * 12 * sizeof(double), m * 12 * sizeof(double));
  out.get(mask, dev + L.mask + f * sizeof(u64), m * sizeof(u64));
  out.get(figs.data(), dev + L.figs + f * 3 * sizeof(double), figs.size() * sizeof(double));
  out.get(counts.data(), dev + L.counts + f * 3 * sizeof(int), counts.size() * sizeof(int));
  CHK(out.finish());
  for (size_t i = 0; i < m; i++) {
    if (support_score) support_score[i] = figs[i * 3 + 0];
    if (spread_t2) spread_t2[i] = figs[i * 3 + 1];
    if (spread_trace) spread_trace[i] = figs[i * 3 + 2];
    if (n_valid) n_valid[i] = counts[i * 3 + 0];
    if (n_set) n_set[i] = counts[i * 3 + 1];
    if (seed) seed[i] = counts[i * 3 + 2];
  }
  return SGTD_OK;
}

int sgtd_result_consensus_rows(sgtd_handle e, int q, uint64_t *rows, int32_t *degree, int32_t *pick) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(consensus_ready(e, &c));
  if (q < 0 || q >= c->cs_n) return SGTD_ERR_INVALID;
  const size_t cn = (size_t)c->cs_cn, o = (size_t)q * cn;
  const ConsensusLayout L((size_t)c->cs_n, cn);
  const char *dev = c->cs_out.as<char>();
  CopyOut out(e, c);
  out.get(rows, dev + L.rows + o * sizeof(u64), cn * sizeof(u64));
  out.get(degree, dev + L.degree + o * sizeof(int), cn * sizeof(int));
  out.get(pick, dev + L.pick + o * sizeof(int), cn * sizeof(int));
  return out.finish();
}

int sgtd_search_loop_consensus(sgtd_handle e, int min_support, int32_t *best_cand, int32_t *best_frame, double *best_score, int32_t *support) {
  if (!e || min_support < 1) return SGTD_ERR_INVALID;
  std::vector<int32_t> cand, frame, n_set;
  std::vector<double> best;
  CHK(consensus_choice(e, min_support, &cand, &frame, &best, &n_set));
  const size_t nq = cand.size();
  if (best_cand) std::copy(cand.begin(), cand.end(), best_cand);
  if (best_frame) std::copy(frame.begin(), frame.end(), best_frame);
  if (best_score) std::copy(best.begin(), best.end(), best_score);
  if (support) std::copy(n_set.begin(), n_set.begin() + (std::ptrdiff_t)nq, support);
  return SGTD_OK;
}

int sgtd_result_consensus_edges(sgtd_handle e, int min_support, int32_t *query, uint32_t *frame_a, uint32_t *frame_b, double *rel_pose,
                                double *score, int64_t capacity, int64_t *n_edges) {
  if (!e || !n_edges || capacity < 0 || min_support < 1) return SGTD_ERR_INVALID;
  std::vector<int32_t> cand, frame, n_set;
  std::vector<double> best;
  CHK(consensus_choice(e, min_support, &cand, &frame, &best, &n_set));
  const int nq = (int)cand.size();
  std::vector<double> fused((size_t)std::max(nq, 1) * 12), support((size_t)std::max(nq, 1));
  if (nq > 0) CHK(sgtd_result_consensus(e, 0, nq, fused.data(), nullptr, nullptr, nullptr, nullptr, support.data(), nullptr, nullptr, nullptr));
  int64_t m = 0;
  for (int q = 0; q < nq; q++) {
    if (cand[(size_t)q] < 0) continue;
    if (m < capacity) {
      if (rel_pose) {
        // rel_pose = mul(inv(B), fused), B the stored pose of the chosen member's frame (a member's frame has one)
        const size_t id = (size_t)(u32)frame[(size_t)q];
        if (id >= e->has_pose.size() || !e->has_pose[id]) { e->err = "sgtd_result_consensus_edges: the stored poses changed since sgtd_pose_consensus"; return SGTD_ERR_STATE; }
        const float *M = e->poses.data() + id * 12;
        const double *F = fused.data() + (size_t)q * 12;
        double Br[9], Bt[3], Fr[9], Ft[3], Ir[9], It[3];
        for (int r = 0; r < 3; r++) {
          for (int cc = 0; cc < 3; cc++) { Br[r * 3 + cc] = (double)M[r * 4 + cc]; Fr[r * 3 + cc] = F[r * 4 + cc]; }
          Bt[r] = (double)M[r * 4 + 3]; Ft[r] = F[r * 4 + 3];
        }
        for (int r = 0; r < 3; r++)
          for (int cc = 0; cc < 3; cc++) Ir[r * 3 + cc] = Br[cc * 3 + r];
        for (int r = 0; r < 3; r++) It[r] = -((Ir[r * 3 + 0] * Bt[0] + Ir[r * 3 + 1] * Bt[1]) + Ir[r * 3 + 2] * Bt[2]);
        double *out = rel_pose + (size_t)m * 12;
        for (int r = 0; r < 3; r++) {
          for (int cc = 0; cc < 3; cc++) out[r * 3 + cc] = (Ir[r * 3 + 0] * Fr[cc] + Ir[r * 3 + 1] * Fr[3 + cc]) + Ir[r * 3 + 2] * Fr[6 + cc];
          out[9 + r] = ((Ir[r * 3 + 0] * Ft[0] + Ir[r * 3 + 1] * Ft[1]) + Ir[r * 3 + 2] * Ft[2]) + It[r];
        }
      }
      if (query) query[m] = q;
      if (frame_a) frame_a[m] = e->grp ? e->grp->current_frame_id : (e->last_kind == 1 ? e->last_qframe + (e->loop_batch ? (u32)q : 0u) : e->current_frame_id);
      if (frame_b) frame_b[m] = (uint32_t)frame[(size_t)q];
      if (score) score[m] = support[(size_t)q];
    }
    m++;
  }
  *n_edges = m;
  return m > capacity ? SGTD_ERR_CAPACITY : SGTD_OK;
}

}  // extern "C"

// ---- sgtd_relax_poses: pose-graph relaxation (relax_kernels.hip.h) ----
namespace {
static_assert(SGTD_RELAX_W == SGTD_RELAX_SUM_W, "relax_ctl_kernel's accumulators are the header's");
size_t relax_up(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// rx_edge, in f64: iz 12, jac 27, y 6 streams of ms = m rounded up to 64, then csum [m], then ec [2][m][2]
struct RelaxEdgeLayout {
  size_t ms, iz, jac, y, csum, ec, total;
  explicit RelaxEdgeLayout(size_t m) : ms((m + 63) & ~(size_t)63), iz(0), jac(12 * ms), y(39 * ms), csum(45 * ms), ec(45 * ms + m), total(45 * ms + 5 * m) {}
  size_t ec_of(int set, size_t m) const { return ec + (size_t)set * m * 2; }
};

int relax_run(sgtd_engine *c, int n, const double *pose0, const uint8_t *fixed, int m, const int32_t *node_i, const int32_t *node_j,
              const double *meas, const double *w_trans, const double *w_rot, const sgtd_relax_options &o, bool all_held, RelaxState *out) {
  sgtd_engine *e = c;      // (HIPCHK reports on the engine that runs the pass)
  const RelaxEdgeLayout lay((size_t)m);
  const size_t ms = lay.ms;
  // the node -> edge CSR, the entries of a node in ascending edge index: off [n + 1], then ent [2 m]
  std::vector<int> &csr = c->rx_host_csr;
  csr.assign((size_t)n + 1 + 2 * (size_t)m, 0);
  int *off = csr.data(), *ent = off + n + 1;
  for (int k = 0; k < m; k++) { off[node_i[k] + 1]++; off[node_j[k] + 1]++; }
  for (int v = 0; v < n; v++) off[v + 1] += off[v];
  {
    std::vector<int> at(off, off + n);
    for (int k = 0; k < m; k++) { ent[at[(size_t)node_i[k]]++] = k << 1; ent[at[(size_t)node_j[k]]++] = (k << 1) | 1; }
  }
  std::vector<double> &w = c->rx_host_w;
  w.resize(2 * (size_t)m);
  for (int k = 0; k < m; k++) { w[(size_t)k] = w_trans ? w_trans[k] : 1.0; w[(size_t)m + k] = w_rot ? w_rot[k] : 1.0; }
  std::vector<unsigned char> &held = c->rx_host_held;
  held.resize((size_t)n);
  for (int v = 0; v < n; v++) held[(size_t)v] = fixed ? (fixed[v] != 0) : (v == 0);

  // inputs, back to back (each at a 256-byte boundary): pose0, meas, weights, node_i, node_j, csr, held
  const size_t o_pose = 0, o_meas = o_pose + relax_up((size_t)n * 12 * sizeof(double)), o_w = o_meas + relax_up((size_t)m * 12 * sizeof(double)),
               o_i = o_w + relax_up(2 * (size_t)m * sizeof(double)), o_j = o_i + relax_up((size_t)m * sizeof(int)),
               o_csr = o_j + relax_up((size_t)m * sizeof(int)), o_held = o_csr + relax_up(csr.size() * sizeof(int)),
               in_bytes = o_held + relax_up((size_t)n);
  // per-node: r x p z ap [n][6], H L [n][36], ok [n]
  const size_t edge_bytes = lay.total * sizeof(double);
  const size_t node_bytes = (size_t)n * (30 + 72) * sizeof(double) + (size_t)n;
  CHK(ensure(c, c->rx_in, in_bytes));
  CHK(ensure(c, c->rx_state, 2 * (size_t)n * SGTD_RELAX_REC * sizeof(double)));
  CHK(ensure(c, c->rx_edge, edge_bytes));
  CHK(ensure(c, c->rx_node, node_bytes));
  CHK(ensure(c, c->rx_ctl, sizeof(RelaxState)));
  char *in = c->rx_in.as<char>();
  CHK(h2d(c, in + o_pose, pose0, (size_t)n * 12 * sizeof(double)));
  CHK(h2d(c, in + o_meas, meas, (size_t)m * 12 * sizeof(double)));
  CHK(h2d(c, in + o_w, w.data(), w.size() * sizeof(double)));
  CHK(h2d(c, in + o_i, node_i, (size_t)m * sizeof(int)));
  CHK(h2d(c, in + o_j, node_j, (size_t)m * sizeof(int)));
  CHK(h2d(c, in + o_csr, csr.data(), csr.size() * sizeof(int)));
  CHK(h2d(c, in + o_held, held.data(), (size_t)n));

  RelaxParams P;
  P.n = n; P.m = m; P.ms = ms;
  P.state = c->rx_state.as<double>();
  P.held = reinterpret_cast<const unsigned char *>(in + o_held);
  P.ei = reinterpret_cast<const int *>(in + o_i); P.ej = reinterpret_cast<const int *>(in + o_j);
  P.wt = reinterpret_cast<const double *>(in + o_w); P.wr = P.wt + m;
  double *eb = c->rx_edge.as<double>();
  P.iz = eb + lay.iz; P.jac = eb + lay.jac; P.y = eb + lay.y; P.csum = eb + lay.csum; P.ec = eb + lay.ec;
  P.off = reinterpret_cast<const int *>(in + o_csr); P.ent = P.off + n + 1;
  P.r = c->rx_node.as<double>(); P.x = P.r + (size_t)n * 6; P.p = P.x + (size_t)n * 6; P.z = P.p + (size_t)n * 6; P.ap = P.z + (size_t)n * 6;
  P.H = P.ap + (size_t)n * 6; P.L = P.H + (size_t)n * 36;
  P.ok = reinterpret_cast<unsigned char *>(P.L + (size_t)n * 36);
  P.st = c->rx_ctl.as<RelaxState>();
  P.lmin = o.lambda_min; P.lmax = o.lambda_max; P.tol2 = o.cg_tol * o.cg_tol; P.step_tol = o.step_tol;
  P.max_outer = o.max_outer; P.all_held = all_held ? 1 : 0;

  RelaxState host{};
  host.lambda = o.lambda_init;
  CHK(h2d(c, P.st, &host, sizeof(RelaxState)));
  if (c->rx_max_blocks == 0) {
    const char *hook = getenv("SGTD_RELAX_MAX_BLOCKS");
    c->rx_max_blocks = hook && atoi(hook) > 0 ? atoi(hook) : 4 * c->n_cus;
  }
  const int ngrid = std::min(grid_for(n, SGTD_RELAX_THREADS), c->rx_max_blocks), egrid = std::min(grid_for(m, SGTD_RELAX_THREADS), c->rx_max_blocks);
  hipStream_t s = c->stream;
  relax_init_kernel<<<std::max(ngrid, egrid), SGTD_RELAX_THREADS, 0, s>>>(P, reinterpret_cast<const double *>(in + o_pose), reinterpret_cast<const double *>(in + o_meas));
  relax_edge_kernel<<<egrid, SGTD_RELAX_THREADS, 0, s>>>(P, 0);
  relax_ctl_kernel<<<1, SGTD_RELAX_W, 0, s>>>(P, RELAX_CTL_COST0);
  HIPCHK(hipGetLastError());
  // outer iterations in groups that fall through once the solve has ended; the state is read once per group.  Every
  // iteration sent either counts as one or finds the solve ended, so max_outer of them are the hard bound
  int sent = 0;
  for (;;) {
    const int group = std::min<int>(SGTD_RELAX_GROUP, o.max_outer - sent);
    for (int g = 0; g < group; g++) {
      relax_setup_kernel<<<ngrid, SGTD_RELAX_THREADS, 0, s>>>(P);
      relax_ctl_kernel<<<1, SGTD_RELAX_W, 0, s>>>(P, RELAX_CTL_RZ0);
      for (int it = 0; it < o.max_inner; it++) {
        relax_cg_edge_kernel<<<egrid, SGTD_RELAX_THREADS, 0, s>>>(P);
        relax_cg_node_kernel<<<ngrid, SGTD_RELAX_THREADS, 0, s>>>(P);
        relax_ctl_kernel<<<1, SGTD_RELAX_W, 0, s>>>(P, RELAX_CTL_PQ);
        relax_cg_update_kernel<<<ngrid, SGTD_RELAX_THREADS, 0, s>>>(P);
        relax_ctl_kernel<<<1, SGTD_RELAX_W, 0, s>>>(P, RELAX_CTL_RZ);
      }
      relax_retract_kernel<<<ngrid, SGTD_RELAX_THREADS, 0, s>>>(P);
      relax_edge_kernel<<<egrid, SGTD_RELAX_THREADS, 0, s>>>(P, 1);
      relax_ctl_kernel<<<1, SGTD_RELAX_W, 0, s>>>(P, RELAX_CTL_ACCEPT);
      relax_edge_kernel<<<egrid, SGTD_RELAX_THREADS, 0, s>>>(P, 0);
      HIPCHK(hipGetLastError());
    }
    sent += group;
    CHK(d2h(c, &host, P.st, sizeof(RelaxState)));
    CHK(xfer_sync(c));
    if (host.done) break;
    if (sent >= o.max_outer) { c->err = "sgtd_relax_poses: the solve did not end within its outer limit"; return SGTD_ERR_HIP; }
  }
  *out = host;
  return SGTD_OK;
}

bool relax_finite(const double *v, size_t n) {
  for (size_t k = 0; k < n; k++)
    if (!std::isfinite(v[k])) return false;
  return true;
}
}  // namespace

extern "C" {

void sgtd_default_relax_options(sgtd_relax_options *o) {
  if (!o) return;
  o->max_outer = 50; o->max_inner = 64;
  o->lambda_init = 1e-4; o->lambda_min = 1e-9; o->lambda_max = 1e9;
  o->cg_tol = 1e-4; o->step_tol = 1e-6;
}

int sgtd_relax_poses(sgtd_handle e, int64_t n_nodes, const double *pose0, const uint8_t *fixed, int64_t n_edges, const int32_t *node_i,
                     const int32_t *node_j, const double *meas, const double *w_trans, const double *w_rot, const sgtd_relax_options *opt,
                     sgtd_relax_report *report) {
  if (!e || n_nodes < 0 || n_edges < 0) return SGTD_ERR_INVALID;
  if (n_nodes > 0 && !pose0) return SGTD_ERR_INVALID;
  if (n_edges > 0 && (!node_i || !node_j || !meas)) return SGTD_ERR_INVALID;
  sgtd_relax_options o;
  sgtd_default_relax_options(&o);
  if (opt) o = *opt;
  auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
  if (o.max_outer <= 0 || o.max_inner <= 0 || !pos(o.lambda_init) || !pos(o.lambda_min) || !pos(o.lambda_max) || !pos(o.cg_tol) || !pos(o.step_tol))
    return SGTD_ERR_INVALID;
  if (n_nodes > SGTD_RELAX_MAX_NODES || n_edges > SGTD_RELAX_MAX_EDGES) {
    e->err = "sgtd_relax_poses takes at most " + std::to_string(SGTD_RELAX_MAX_NODES) + " nodes and " + std::to_string(SGTD_RELAX_MAX_EDGES) + " edges";
    return SGTD_ERR_UNSUPPORTED;
  }
  for (int64_t k = 0; k < n_edges; k++) {
    if (node_i[k] < 0 || node_i[k] >= n_nodes || node_j[k] < 0 || node_j[k] >= n_nodes || node_i[k] == node_j[k]) return SGTD_ERR_INVALID;
    if ((w_trans && !(std::isfinite(w_trans[k]) && w_trans[k] >= 0.0)) || (w_rot && !(std::isfinite(w_rot[k]) && w_rot[k] >= 0.0))) return SGTD_ERR_INVALID;
  }
  if (!relax_finite(pose0, (size_t)n_nodes * 12) || !relax_finite(meas, (size_t)n_edges * 12)) return SGTD_ERR_INVALID;
  sgtd_relax_report rep{};
  rep.lambda = o.lambda_init;
  rep.status = SGTD_RELAX_NOTHING_FREE;
  if (n_nodes == 0 || n_edges == 0) {      // (nothing runs and no device is touched: the empty result)
    sgtd_engine *c = home_engine(e);
    c->rx_n = 0; c->rx_m = 0;
    if (report) *report = rep;
    return SGTD_OK;
  }
  bool all_held = fixed != nullptr;
  for (int64_t v = 0; all_held && v < n_nodes; v++) all_held = fixed[v] != 0;
  if (!fixed && n_nodes == 1) all_held = true;
  StageRun<int64_t> run(e, &sgtd_engine::rx_n);
  RelaxState st{};
  run.on_device([&](sgtd_engine *c) { return relax_run(c, (int)n_nodes, pose0, fixed, (int)n_edges, node_i, node_j, meas, w_trans, w_rot, o, all_held, &st); });
  CHK(run.end(n_nodes));
  run.c->rx_m = n_edges; run.c->rx_cur = st.cur;
  rep.cost_before = st.cost_before; rep.cost_after = st.cost; rep.lambda = st.lambda;
  rep.outer_iterations = st.outer; rep.steps_accepted = st.accepted; rep.cg_iterations = st.cg_total; rep.status = st.status;
  if (report) *report = rep;
  return SGTD_OK;
}

int sgtd_result_relaxed(sgtd_handle e, double *pose, double *edge_cost) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::rx_n, "no relaxed poses: sgtd_relax_poses has not run", &c));
  const size_t n = (size_t)c->rx_n, m = (size_t)c->rx_m;
  if (n == 0) return SGTD_OK;
  std::vector<double> rec(pose ? n * SGTD_RELAX_REC : 0);      // (the node records: the pose is part of one)
  CopyOut out(e, c);
  out.get(rec.data(), c->rx_state.as<double>() + (size_t)c->rx_cur * n * SGTD_RELAX_REC, rec.size() * sizeof(double));
  out.get(edge_cost, c->rx_edge.as<double>() + RelaxEdgeLayout(m).ec_of(c->rx_cur, m), m * 2 * sizeof(double));
  CHK(out.finish());
  if (pose)
    for (size_t v = 0; v < n; v++)
      for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) pose[v * 12 + r * 4 + k] = rec[v * SGTD_RELAX_REC + 7 + r * 3 + k];
        pose[v * 12 + r * 4 + 3] = rec[v * SGTD_RELAX_REC + 4 + r];
      }
  return SGTD_OK;
}

}  // extern "C"

// ---- sgtd_register_clouds: dense GICP registration (register_kernels.hip.h) ----
namespace {
static_assert(SGTD_REG_W == SGTD_REG_SUM_W && SGTD_REG_THREADS == SGTD_REG_SRC_TILE && SGTD_REG_TILE == SGTD_REG_TGT_TILE && SGTD_REG_K == SGTD_REG_MAX_K,
              "the register kernels' sizes are the header's");
constexpr size_t kRegPartMax = (size_t)1 << 27;      // entries of the slices' minima (12 B each) a call may hold: longer slices beyond

// tiles of a slice: the header's, or the SGTD_REG_SLICE_TILES environment hook's
int reg_slice_tiles() {
  const char *hook = getenv("SGTD_REG_SLICE_TILES");
  return hook && atoi(hook) > 0 ? std::min(atoi(hook), 1 << 10) : SGTD_REG_SLICE_TILES;
}

// ---- what sgtd_register_clouds and sgtd_register_voxels share on the host: one GICP call skeleton
// the result rows, in one buffer: pose [n][12], fitness [n], cost [n][2] in f64, then matched, iterations, status [n] in
// i32 and, where the call counts correspondences (sgtd_register_voxels), n_corr [n]
struct RegOut {
  size_t n;
  bool with_corr;
  RegOut(size_t n_, bool with_corr_) : n(n_), with_corr(with_corr_) {}
  size_t bytes() const { return n * (15 * sizeof(double) + (with_corr ? 4 : 3) * sizeof(int)); }
  double *pose(void *p) const { return static_cast<double *>(p); }
  double *fitness(void *p) const { return pose(p) + n * 12; }
  double *cost(void *p) const { return fitness(p) + n; }
  int *matched(void *p) const { return reinterpret_cast<int *>(cost(p) + n * 2); }
  int *iters(void *p) const { return matched(p) + n; }
  int *status(void *p) const { return iters(p) + n; }
  int *corr(void *p) const { return status(p) + n; }
};

// the rows a getter asks for, from the home engine c's buffer ob (n_corr: NULL where the call has none)
int reg_rows_out(sgtd_engine *e, sgtd_engine *c, const RegOut &out, void *ob, double *pose, double *fitness, double *cost, int32_t *n_matched,
                 int32_t *n_corr, int32_t *iterations, int32_t *status) {
  const size_t n = out.n;
  CopyOut copy(e, c);
  copy.get(pose, out.pose(ob), n * 12 * sizeof(double));
  copy.get(fitness, out.fitness(ob), n * sizeof(double));
  copy.get(cost, out.cost(ob), n * 2 * sizeof(double));
  copy.get(n_matched, out.matched(ob), n * sizeof(int));
  if (out.with_corr) copy.get(n_corr, out.corr(ob), n * sizeof(int));
  copy.get(iterations, out.iters(ob), n * sizeof(int));
  copy.get(status, out.status(ob), n * sizeof(int));
  return copy.finish();
}

// the options the two calls' structs share: their check, and what the kernels take of them
bool gicp_options_ok(int k, int max_iterations, int lm_max_trials, int reserved, double lambda_factor, double rotation_eps, double translation_eps,
                     double plane_eps) {
  auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
  return k >= 3 && k <= SGTD_REG_MAX_K && max_iterations >= 1 && lm_max_trials >= 1 && reserved == 0 && pos(lambda_factor) && pos(rotation_eps) &&
         pos(translation_eps) && pos(plane_eps);
}
RegOptionsDev gicp_options(int k, int max_iterations, int lm_max_trials, double max_corr_dist, double lambda_factor, double rotation_eps,
                           double translation_eps, double plane_eps) {
  RegOptionsDev o;
  o.k = k; o.max_iterations = max_iterations; o.lm_max_trials = lm_max_trials;
  o.max2 = max_corr_dist * max_corr_dist; o.lambda_factor = lambda_factor;
  o.rotation_eps = rotation_eps; o.translation_eps = translation_eps; o.plane_eps = plane_eps;
  return o;
}

// the caps both calls put on the clouds and the pairs, and the part of the message that names them
bool gicp_caps_ok(const int64_t *pt_off, int n_clouds, int n_pairs) {
  int64_t max_cloud = 0;
  for (int cl = 0; cl < n_clouds; cl++) max_cloud = std::max(max_cloud, pt_off[cl + 1] - pt_off[cl]);
  return max_cloud <= SGTD_REG_MAX_POINTS && n_clouds <= SGTD_REG_MAX_CLOUDS && pt_off[n_clouds] <= SGTD_REG_MAX_TOTAL_POINTS && n_pairs <= SGTD_REG_MAX_PAIRS;
}
std::string gicp_caps_text(const char *call) {
  return std::string(call) + " takes at most " + std::to_string(SGTD_REG_MAX_POINTS) + " points a cloud, " + std::to_string(SGTD_REG_MAX_CLOUDS) +
         " clouds, " + std::to_string(SGTD_REG_MAX_TOTAL_POINTS) + " points in all";
}

// The index arrays of a call, packed into one upload.  The two calls have in common: src [n], src_off [n + 1] (the
// pairs' source points back to back), the tiles of SGTD_REG_THREADS points of the pairs' sources (the pair, the first
// point within its source) and of the clouds that are named (the cloud, the first point).
struct GicpIndex {
  std::vector<int> &up;
  std::vector<int> tile_pair, tile_first, ctile_cloud, ctile_first;
  size_t u_src = 0, u_soff = 0, u_tiles = 0;
  explicit GicpIndex(std::vector<int> &up_) : up(up_) { up.clear(); }
  size_t put(const int *p, size_t cnt) { const size_t at = up.size(); up.insert(up.end(), p, p + cnt); return at; }
  void tiles(const int64_t *pt_off, int n_clouds, const int32_t *src, int n, const unsigned char *named, std::vector<int> *soff) {
    soff->assign((size_t)n + 1, 0);
    for (int k = 0; k < n; k++) {
      const int ns = (int)(pt_off[src[k] + 1] - pt_off[src[k]]);
      (*soff)[(size_t)k + 1] = (*soff)[(size_t)k] + ns;
      for (int f = 0; f < ns; f += SGTD_REG_THREADS) { tile_pair.push_back(k); tile_first.push_back(f); }
    }
    for (int cl = 0; cl < n_clouds; cl++) {
      if (!named[cl]) continue;
      const int np = (int)(pt_off[cl + 1] - pt_off[cl]);
      for (int f = 0; f < np; f += SGTD_REG_THREADS) { ctile_cloud.push_back(cl); ctile_first.push_back(f); }
    }
  }
  void put_tiles() {
    u_tiles = put(tile_pair.data(), tile_pair.size());
    put(tile_first.data(), tile_first.size());
    put(ctile_cloud.data(), ctile_cloud.size());
    put(ctile_first.data(), ctile_first.size());
  }
};

// what RegParams holds for both calls: the points, the uploaded offsets (d_pt_off) and index arrays (di), the per-point
// covariances, the solves' state and counter, the result rows, the options; the rest is zero
void gicp_params(RegParams &P, const GicpIndex &G, const float *points, int stride, const void *d_pt_off, const int *di, int n, size_t total_src,
                 double *cov, void *state, void *ctl, const RegOut &out, void *ob, const RegOptionsDev &o) {
  std::memset(&P, 0, sizeof(P));
  P.pts = points; P.stride = stride;
  P.pt_off = static_cast<const long long *>(d_pt_off);
  P.src = di + G.u_src; P.src_off = di + G.u_soff;
  P.tile_pair = di + G.u_tiles; P.tile_first = P.tile_pair + G.tile_pair.size();
  P.ctile_cloud = P.tile_first + G.tile_first.size(); P.ctile_first = P.ctile_cloud + G.ctile_cloud.size();
  P.n_pairs = n; P.n_tiles = (int)G.tile_pair.size(); P.n_ctiles = (int)G.ctile_cloud.size(); P.total_src = (int)total_src;
  P.cov = cov;
  P.st = static_cast<RegState *>(state);
  P.unfinished = static_cast<int *>(ctl);
  P.out_pose = out.pose(ob); P.out_fitness = out.fitness(ob); P.out_cost = out.cost(ob);
  P.out_matched = out.matched(ob); P.out_iters = out.iters(ob); P.out_status = out.status(ob);
  P.o = o;
}

// The solves' rounds, in groups that fall through for the pairs that have ended; the count of unfinished pairs is read
// once per group.  Every round (one call of `round`: its launches) is one trial of every unfinished pair, so
// max_iterations * lm_max_trials rounds are the hard bound.
template <class Round>
int gicp_rounds(sgtd_engine *c, const char *call, const RegParams &P, int unfinished, Round &&round) {
  const long long bound = (long long)P.o.max_iterations * P.o.lm_max_trials;
  long long sent = 0;
  while (unfinished > 0) {
    if (sent >= bound) { c->err = std::string(call) + ": the solves did not end within their limits"; return SGTD_ERR_HIP; }
    const int group = (int)std::min<long long>(SGTD_REG_GROUP, bound - sent);
    for (int g = 0; g < group; g++) CHK(round());
    sent += group;
    CHK(d2h(c, &unfinished, P.unfinished, sizeof(int)));
    CHK(xfer_sync(c));
  }
  return SGTD_OK;
}

// Where a dense run keeps its buffers and finds its clouds: sgtd_register_clouds' own arrays, or sgtd_register_stored's
// over the cloud store's arena, whose stored clouds come before the call's.
struct RegSite {
  const char *call;
  DenseRun &R;         // the run's buffers, host arrays and clock
  const float *pts;                 // the points of every cloud the kernels may name, on the device
  int stride;
  double *cov;                      // where the covariances of those clouds go; NULL: R.cov, grown to the call's points
  const long long *d_off;           // the clouds' offsets where they are on the device already; NULL: pt_off is uploaded
  int first;                        // the index the kernels know the call's cloud 0 by
  const double *d_init;             // the start poses where they are on the device already (init is NULL then)
};

// One dense GICP run.  pt_off, n_clouds, named, src: the call's clouds, which of them need covariances, the pairs'
// sources; tgt, tgt_n: the targets as the kernels know them, and their sizes
int reg_run(sgtd_engine *c, const RegSite &S, const sgtd_register_options &o, const int64_t *pt_off, int n_clouds, const unsigned char *named,
            const int32_t *src, const int32_t *tgt, const int64_t *tgt_n, const double *init, int n) {
  sgtd_engine *e = c;      // (HIPCHK reports on the engine that runs the pass)
  const bool timed = c->timing;
  DenseRun &R = S.R;
  LapClock &clock = R.clock;
  CHK(clock.start(c, timed));
  const size_t total = (size_t)pt_off[n_clouds];
  // the tiles: of the pairs' sources, of the clouds that need covariances
  int64_t max_tgt = 0;
  for (int k = 0; k < n; k++) max_tgt = std::max<int64_t>(max_tgt, tgt_n[k]);
  GicpIndex G(R.host_up);
  G.tiles(pt_off, n_clouds, src, n, named, &R.host_soff);
  if (n == 0) return SGTD_OK;      // (a run without a pair: no cloud is named, nothing comes back)
  const int total_src = R.host_soff[(size_t)n], n_tiles = (int)G.tile_pair.size();
  long long slice = (long long)reg_slice_tiles() * SGTD_REG_TILE;
  auto slices_of = [&](long long len) { return (size_t)std::max<long long>((max_tgt + len - 1) / len, 1); };
  while ((size_t)total_src * slices_of(slice) > kRegPartMax) slice *= 2;
  const size_t n_slices = slices_of(slice);

  // the index upload: src, tgt, src_off, the tiles (clouds by the index the kernels know them by)
  G.u_src = G.put(src, (size_t)n);
  const size_t u_tgt = G.put(tgt, (size_t)n);
  G.u_soff = G.put(R.host_soff.data(), (size_t)n + 1);
  if (S.first) {
    for (int k = 0; k < n; k++) R.host_up[G.u_src + (size_t)k] += S.first;
    for (int &cl : G.ctile_cloud) cl += S.first;
  }
  G.put_tiles();
  const size_t o_off = 0, o_init = o_off + relax_up((size_t)(n_clouds + 1) * sizeof(int64_t)), o_idx = o_init + relax_up((size_t)n * 12 * sizeof(double)),
               in_bytes = o_idx + relax_up(G.up.size() * sizeof(int));
  const size_t ts = (size_t)std::max(total_src, 1);
  const RegOut out((size_t)n, false);
  CHK(ensure(c, R.in, in_bytes));
  if (!S.cov) CHK(need(c, R.cov, std::max<size_t>(total, 1) * 9));
  CHK(ensure(c, R.part, ts * n_slices * (sizeof(double) + sizeof(int))));
  CHK(ensure(c, R.match, ts * (10 * sizeof(double) + sizeof(int))));
  CHK(ensure(c, R.state, (size_t)n * sizeof(RegState)));
  CHK(ensure(c, R.out, out.bytes()));
  CHK(ensure(c, R.ctl, 64));
  char *in = R.in.as<char>();
  if (!S.d_off) CHK(h2d(c, in + o_off, pt_off, (size_t)(n_clouds + 1) * sizeof(int64_t)));
  if (init) CHK(h2d(c, in + o_init, init, (size_t)n * 12 * sizeof(double)));
  CHK(h2d(c, in + o_idx, G.up.data(), G.up.size() * sizeof(int)));
  const double *d_init = init ? reinterpret_cast<const double *>(in + o_init) : S.d_init;

  RegParams P;
  const int *di = reinterpret_cast<const int *>(in + o_idx);
  gicp_params(P, G, S.pts, S.stride, S.d_off ? static_cast<const void *>(S.d_off) : in + o_off, di, n, ts, S.cov ? S.cov : R.cov.p(),
              R.state.p, R.ctl.p, out, R.out.p,
              gicp_options(o.k_neighbors, o.max_iterations, o.lm_max_trials, o.max_corr_dist, o.lm_init_lambda_factor, o.rotation_eps, o.translation_eps,
                           o.plane_eps));
  P.tgt = di + u_tgt; P.slice = (int)slice;
  P.part_d2 = R.part.as<double>(); P.part_j = reinterpret_cast<int *>(P.part_d2 + ts * n_slices);
  P.md2 = R.match.as<double>(); P.M = P.md2 + ts; P.mj = reinterpret_cast<int *>(P.M + 9 * ts);

  int unfinished = 0;
  for (int k = 0; k < n; k++)
    if (pt_off[src[k] + 1] > pt_off[src[k]] && tgt_n[k] > 0) unfinished++;
  CHK(h2d(c, P.unfinished, &unfinished, sizeof(int)));
  hipStream_t s = c->stream;
  const dim3 sgrid((unsigned)n_tiles, (unsigned)n_slices);
  if (timed) { HIPCHK(hipEventRecord(clock.ev[2], s)); HIPCHK(hipEventRecord(clock.ev[0], s)); }
  if (P.n_ctiles) reg_cov_kernel<<<P.n_ctiles, SGTD_REG_THREADS, 0, s>>>(P);
  if (timed) CHK(clock.lap(c, 0));
  reg_init_kernel<<<grid_for(n, SGTD_REG_W), SGTD_REG_W, 0, s>>>(P, d_init);
  HIPCHK(hipGetLastError());
  CHK(gicp_rounds(c, S.call, P, unfinished, [&]() -> int {
    reg_search_kernel<<<sgrid, SGTD_REG_THREADS, 0, s>>>(P, 0);
    if (timed) CHK(clock.lap(c, 1));
    reg_match_kernel<<<n_tiles, SGTD_REG_THREADS, 0, s>>>(P, 0);
    reg_lin_kernel<<<n, SGTD_REG_W, 0, s>>>(P);
    reg_trial_kernel<<<n, SGTD_REG_W, 0, s>>>(P);
    if (timed) CHK(clock.lap(c, 2));
    HIPCHK(hipGetLastError());
    return SGTD_OK;
  }));
  if (n_tiles) {
    reg_search_kernel<<<sgrid, SGTD_REG_THREADS, 0, s>>>(P, 1);
    if (timed) CHK(clock.lap(c, 1));
    reg_match_kernel<<<n_tiles, SGTD_REG_THREADS, 0, s>>>(P, 1);
  }
  reg_final_kernel<<<n, SGTD_REG_W, 0, s>>>(P);
  HIPCHK(hipGetLastError());
  if (timed) {
    CHK(clock.lap(c, 2));
    CHK(clock.span(c, 2, 1, 3, false));
  }
  CHK(xfer_sync(c));
  return SGTD_OK;
}

// sgtd_register_clouds' run: every cloud is the call's, and a cloud some pair names needs covariances
int reg_clouds_run(sgtd_engine *c, const sgtd_register_options &o, const float *points, int stride, const int64_t *pt_off, int n_clouds,
                   const int32_t *src, const int32_t *tgt, const double *init, int n) {
  DenseRun &R = c->dense;
  // what the getters need
  R.host_off.assign(pt_off, pt_off + n_clouds + 1);
  R.host_named.assign((size_t)n_clouds, 0);
  std::vector<int64_t> tgt_n((size_t)n);
  for (int k = 0; k < n; k++) {
    R.host_named[(size_t)src[k]] = 1; R.host_named[(size_t)tgt[k]] = 1;
    tgt_n[(size_t)k] = pt_off[tgt[k] + 1] - pt_off[tgt[k]];
  }
  const RegSite S{"sgtd_register_clouds", R, points, stride, nullptr, nullptr, 0, nullptr};
  return reg_run(c, S, o, pt_off, n_clouds, R.host_named.data(), src, tgt, tgt_n.data(), init, n);
}

// the options of a dense call: the defaults or the caller's, checked
int dense_options(const sgtd_register_options *opt, sgtd_register_options *o) {
  sgtd_default_register_options(o);
  if (opt) *o = *opt;
  if (!gicp_options_ok(o->k_neighbors, o->max_iterations, o->lm_max_trials, o->reserved, o->lm_init_lambda_factor, o->rotation_eps, o->translation_eps,
                       o->plane_eps) ||
      !(o->max_corr_dist > 0.0))
    return SGTD_ERR_INVALID;
  return SGTD_OK;
}

// What both dense calls check of their arguments before the device is touched, in sgtd_register_clouds' order.
// target_ok(k): whether pair k's target is one of the call's (sgtd_register_clouds: a cloud's index).  The frames of
// sgtd_register_stored are looked up behind the caps and the store's settings, which come after this: that call checks
// them itself.
template <class TargetOk>
int dense_check(sgtd_engine *e, const char *call, const sgtd_register_options *opt, sgtd_register_options *o, const float *points, int stride_floats,
                const int64_t *pt_off, int n_clouds, const int32_t *src_cloud, const void *targets, const double *init_pose, int n_pairs,
                TargetOk &&target_ok) {
  if (!e || n_pairs < 0) return SGTD_ERR_INVALID;
  if (n_pairs > 0 && (!src_cloud || !targets)) return SGTD_ERR_INVALID;
  CHK(dense_options(opt, o));
  if (!cloud_set_ok(pt_off, n_clouds, stride_floats, points, false, nullptr)) return SGTD_ERR_INVALID;
  int64_t total_src = 0;
  for (int k = 0; k < n_pairs; k++) {
    if (src_cloud[k] < 0 || src_cloud[k] >= n_clouds || !target_ok(k)) return SGTD_ERR_INVALID;
    total_src += pt_off[src_cloud[k] + 1] - pt_off[src_cloud[k]];
  }
  if (init_pose && !relax_finite(init_pose, (size_t)n_pairs * 12)) return SGTD_ERR_INVALID;
  if (!gicp_caps_ok(pt_off, n_clouds, n_pairs) || total_src > SGTD_REG_MAX_SOURCE_POINTS) {
    e->err = gicp_caps_text(call) + ", " + std::to_string(SGTD_REG_MAX_PAIRS) + " pairs and " + std::to_string(SGTD_REG_MAX_SOURCE_POINTS) +
             " source points over the pairs";
    return SGTD_ERR_UNSUPPORTED;
  }
  return SGTD_OK;
}

// The getters of a dense run, over the buffers and host arrays of the call that made it: `run` on e's home engine
// (`missing`: what the handle is told where that call has not run)
int dense_rows_out(sgtd_engine *e, DenseRun sgtd_engine::*run, const char *missing, double *pose, double *fitness, double *cost, int32_t *n_matched,
                   int32_t *iterations, int32_t *status) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, run, missing, &c));
  const DenseRun &R = c->*run;
  if (R.n == 0) return SGTD_OK;
  return reg_rows_out(e, c, RegOut((size_t)R.n, false), R.out.p, pose, fitness, cost, n_matched, nullptr, iterations, status);
}

int dense_cov_out(sgtd_engine *e, DenseRun sgtd_engine::*run, const char *missing, int cloud, double *cov, int64_t capacity, int64_t *n) {
  if (!e || capacity < 0) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, run, missing, &c));
  const DenseRun &R = c->*run;
  if (cloud < 0 || (size_t)cloud >= R.host_named.size()) return SGTD_ERR_INVALID;
  const int64_t first = R.host_off[(size_t)cloud];
  const int64_t need = R.host_named[(size_t)cloud] ? R.host_off[(size_t)cloud + 1] - first : 0;
  if (n) *n = need;
  const size_t m = (size_t)std::min(need, capacity);
  CopyOut out(e, c);
  out.get(cov, R.cov.p() + (size_t)first * 9, m * 9 * sizeof(double));
  CHK(out.finish());
  return need > capacity && cov ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int dense_matches_out(sgtd_engine *e, DenseRun sgtd_engine::*run, const char *missing, int pair, int32_t *tgt_index, double *d2, int64_t capacity,
                      int64_t *n) {
  if (!e || capacity < 0) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, run, missing, &c));
  const DenseRun &R = c->*run;
  if (pair < 0 || pair >= R.n) return SGTD_ERR_INVALID;
  const int *soff = R.host_soff.data();
  const int64_t first = soff[pair], need = soff[pair + 1] - first;
  const size_t ts = (size_t)std::max(soff[R.n], 1);
  if (n) *n = need;
  const size_t m = (size_t)std::min(need, capacity);
  const double *md2 = R.match.as<double>();
  const int *mj = reinterpret_cast<const int *>(md2 + 10 * ts);
  CopyOut out(e, c);
  out.get(tgt_index, mj + first, m * sizeof(int));
  out.get(d2, md2 + first, m * sizeof(double));
  CHK(out.finish());
  return need > capacity && (tgt_index || d2) ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int dense_ms_out(sgtd_engine *e, DenseRun sgtd_engine::*run, const char *missing, float *ms_cov, float *ms_search, float *ms_rest, float *ms_total) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, run, missing, &c));
  const float *ms = (c->*run).clock.ms;
  if (ms_cov) *ms_cov = ms[0];
  if (ms_search) *ms_search = ms[1];
  if (ms_rest) *ms_rest = ms[2];
  if (ms_total) *ms_total = ms[3];
  return SGTD_OK;
}

const char kNoRegistered[] = "no registered clouds: sgtd_register_clouds has not run";
}  // namespace

extern "C" {

void sgtd_default_register_options(sgtd_register_options *o) {
  if (!o) return;
  o->k_neighbors = 20; o->max_iterations = 64; o->lm_max_trials = 10; o->reserved = 0;
  o->max_corr_dist = std::numeric_limits<double>::infinity();
  o->lm_init_lambda_factor = 1e-9; o->rotation_eps = 2e-3; o->translation_eps = 5e-4; o->plane_eps = 1e-3;
}

void sgtd_register_tiles(int *src_tile, int *tgt_tile, int *slice) {
  if (src_tile) *src_tile = SGTD_REG_SRC_TILE;
  if (tgt_tile) *tgt_tile = SGTD_REG_TGT_TILE;
  if (slice) *slice = reg_slice_tiles() * SGTD_REG_TGT_TILE;
}

int sgtd_register_clouds(sgtd_handle e, const sgtd_register_options *opt, const float *points, int stride_floats, const int64_t *pt_off, int n_clouds,
                         const int32_t *src_cloud, const int32_t *tgt_cloud, const double *init_pose, int n_pairs, int device_ptrs) {
  sgtd_register_options o;
  CHK(dense_check(e, "sgtd_register_clouds", opt, &o, points, stride_floats, pt_off, n_clouds, src_cloud, tgt_cloud, init_pose, n_pairs,
                  [&](int k) { return tgt_cloud[k] >= 0 && tgt_cloud[k] < n_clouds; }));
  const int64_t total = pt_off[n_clouds];
  StageRun<int> run(e, &sgtd_engine::dense);
  run.on_device([&](sgtd_engine *c) -> int {
    const float *d_pts = nullptr;
    CHK(points_on_device(c, c->dense.pts.buf, points, (size_t)total * stride_floats, device_ptrs, &d_pts));
    return reg_clouds_run(c, o, d_pts, stride_floats, pt_off, n_clouds, src_cloud, tgt_cloud, init_pose, n_pairs);
  });
  return run.end(n_pairs);
}

int sgtd_result_registered(sgtd_handle e, double *pose, double *fitness, double *cost, int32_t *n_matched, int32_t *iterations, int32_t *status) {
  return dense_rows_out(e, &sgtd_engine::dense, kNoRegistered, pose, fitness, cost, n_matched, iterations, status);
}

int sgtd_result_register_covariances(sgtd_handle e, int cloud, double *cov, int64_t capacity, int64_t *n) {
  return dense_cov_out(e, &sgtd_engine::dense, kNoRegistered, cloud, cov, capacity, n);
}

int sgtd_result_register_matches(sgtd_handle e, int pair, int32_t *tgt_index, double *d2, int64_t capacity, int64_t *n) {
  return dense_matches_out(e, &sgtd_engine::dense, kNoRegistered, pair, tgt_index, d2, capacity, n);
}

int sgtd_register_stage_ms(sgtd_handle e, float *ms_cov, float *ms_search, float *ms_rest, float *ms_total) {
  return dense_ms_out(e, &sgtd_engine::dense, kNoRegistered, ms_cov, ms_search, ms_rest, ms_total);
}

}  // extern "C"

// ---- sgtd_set_frame_clouds / sgtd_register_stored / sgtd_register_stored_loops (cloud_store_kernels.hip.h) ----
namespace {
using CloudSlot = sgtd_engine::CloudSlot;
using CloudArena = sgtd_engine::CloudArena;
constexpr int64_t kStoreInitPoints = 1 << 16;      // the arena's first capacity, unless the SGTD_CLOUD_STORE_INIT_POINTS hook (tests) gives another

int64_t store_init_points() {
  const char *hook = getenv("SGTD_CLOUD_STORE_INIT_POINTS");
  return hook && atoll(hook) > 0 ? std::min<int64_t>(atoll(hook), SGTD_CLOUD_STORE_MAX_POINTS) : kStoreInitPoints;
}

// a new device array for the arena: the old one is neither freed nor touched, so a failure leaves the store as it was
int store_alloc(sgtd_engine *e, DevBuf &b, size_t bytes) {
  void *p = nullptr;
  const hipError_t st_ = hipMalloc(&p, std::max<size_t>(bytes, 1));
  if (st_ != hipSuccess) {
    (void)hipGetLastError();
    e->err = "hipMalloc of " + std::to_string(bytes) + " bytes for the cloud store: " + hipGetErrorString(st_);
    return SGTD_ERR_HIP;
  }
  e->stats.device_allocs_total++;
  b.p = p; b.bytes = bytes;
  return SGTD_OK;
}

// A change of the arena that is not the store's until store_commit: the slots that die (`dies`, indices into the
// current arena), and `next` where the change needs new arrays (the live slots, in order, copied into them).  Leaving
// the scope frees whichever arrays are not the store's: next's after a failure, the old ones after a commit.
struct StoreChange {
  std::vector<int> dies;
  CloudArena next;
  bool rebuilt = false;
};

// Room behind the slots for `pts` points and `clouds` clouds.  *A = the arena to write to: the store's own where they
// fit and the dead points (the dying slots included) do not outnumber the live ones plus `incoming`; otherwise W.next,
// NEW arrays into which the live slots are compacted and renumbered.  The store itself is unchanged either way.
int store_prepare(sgtd_engine *e, StoreChange &W, int64_t pts, int64_t clouds, int64_t incoming, CloudArena **A) {
  CloudArena &cur = e->st;
  std::vector<unsigned char> dying(cur.slots.size(), 0);
  int64_t live = cur.live;
  for (int s : W.dies) { dying[(size_t)s] = 1; live -= cur.slots[(size_t)s].count; }
  const int64_t dead = cur.used - live;
  const bool fits = cur.pts.p && cur.cap >= cur.used + pts && cur.off_cap >= (int64_t)cur.slots.size() + clouds + 1;
  *A = &cur;
  if (fits && dead <= live + incoming) return SGTD_OK;
  CloudArena &N = W.next;
  std::vector<long long> move;      // from [n_live + 1], to [n_live + 1]
  for (size_t s = 0; s < cur.slots.size(); s++)
    if (cur.slots[s].live && !dying[s]) N.slots.push_back(cur.slots[s]);
  const size_t nl = N.slots.size();
  move.assign(2 * (nl + 1), 0);
  int64_t at = 0;
  for (size_t s = 0; s < nl; s++) {
    move[s] = N.slots[s].first; move[nl + 1 + s] = at;
    N.slots[s].first = at;
    at += N.slots[s].count;
  }
  move[nl] = 0; move[2 * nl + 1] = at;
  N.used = N.live = at;
  const int64_t need = at + pts, rows = (int64_t)nl + clouds + 1;
  N.cap = std::max<int64_t>(need + need / 2, cur.cap ? 1 : store_init_points());      // (the hook: a store's first capacity)
  N.off_cap = std::max<int64_t>(2 * rows, 64);
  CHK(store_alloc(e, N.pts, (size_t)N.cap * 3 * sizeof(float)));
  CHK(store_alloc(e, N.cov, (size_t)N.cap * 9 * sizeof(double)));
  CHK(store_alloc(e, N.off, (size_t)N.off_cap * sizeof(long long)));
  CHK(ensure(e, e->st_idx, move.size() * sizeof(long long)));
  CHK(h2d(e, e->st_idx.p, move.data(), move.size() * sizeof(long long)));
  if (at > 0) {
    StoreMoveParams P;
    P.pts_in = cur.pts.as<float>(); P.cov_in = cur.cov.as<double>(); P.pts_out = N.pts.as<float>(); P.cov_out = N.cov.as<double>();
    P.from = e->st_idx.as<long long>(); P.to = P.from + nl + 1; P.n_live = (int)nl; P.total = at;
    const int grid = (int)std::min<long long>(grid_for(at * 12, SGTD_STORE_THREADS), (long long)e->n_cus * 16);
    store_compact_kernel<<<grid, SGTD_STORE_THREADS, 0, e->stream>>>(P);
    HIPCHK(hipGetLastError());
  }
  // the slots' offsets: row s = the first point of slot s, row n_live = the points in use
  CHK(h2d(e, N.off.p, move.data() + nl + 1, (nl + 1) * sizeof(long long)));
  CHK(xfer_sync(e));      // (move is this function's)
  W.rebuilt = true;
  *A = &W.next;
  return SGTD_OK;
}

// the change becomes the store's: the work enqueued on the new arrays has been waited for
void store_commit(sgtd_engine *e, StoreChange &W) {
  CloudArena &cur = e->st;
  if (W.rebuilt) {
    std::swap(cur, W.next);      // (the old arrays are W's now, and go with it)
    std::fill(e->st_slot_of.begin(), e->st_slot_of.end(), SGTD_STORE_NONE);
    for (size_t s = 0; s < cur.slots.size(); s++) e->st_slot_of[cur.slots[s].frame] = (int)s;
    e->st_frames = (int64_t)cur.slots.size();
  } else {
    for (int s : W.dies) {
      CloudSlot &sl = cur.slots[(size_t)s];
      sl.live = false;
      cur.live -= sl.count;
      e->st_slot_of[sl.frame] = SGTD_STORE_NONE;
      e->st_frames--;
    }
  }
  static std::atomic<u64> serial{0};
  e->st_serial = ++serial;
}

// room for a call's own clouds behind the slots (a rebuild renumbers the slots: frames are looked up after this)
int store_room(sgtd_engine *e, int64_t pts, int64_t clouds) {
  StoreChange W;
  CloudArena *A = nullptr;
  CHK(store_prepare(e, W, pts, clouds, 0, &A));
  if (W.rebuilt) store_commit(e, W);
  return SGTD_OK;
}

// the frame -> slot table on the device, made again when the store has changed (the loops forms read it)
int store_table(sgtd_engine *e) {
  if (e->st_table_serial == e->st_serial && e->st_table.p) return SGTD_OK;
  CHK(ensure(e, e->st_table, std::max<size_t>(e->st_slot_of.size(), 1) * sizeof(int)));
  CHK(h2d(e, e->st_table.p, e->st_slot_of.data(), e->st_slot_of.size() * sizeof(int)));
  e->st_table_serial = e->st_serial;
  return SGTD_OK;
}

// `total` points of the given stride, on the device, into the arena from point `first` on
int store_pack(sgtd_engine *e, CloudArena &A, const float *d_src, int stride, int64_t total, int64_t first) {
  if (total == 0) return SGTD_OK;
  const int grid = (int)std::min<long long>(grid_for(total * 3, SGTD_STORE_THREADS), (long long)e->n_cus * 16);
  store_pack_kernel<<<grid, SGTD_STORE_THREADS, 0, e->stream>>>(d_src, stride, total, A.pts.as<float>() + (size_t)first * 3);
  HIPCHK(hipGetLastError());
  return SGTD_OK;
}

// the offsets of `n` clouds that follow the arena's slots: rows [slots .. slots + n] of its offsets
int store_tail_rows(sgtd_engine *e, CloudArena &A, const int64_t *pt_off, int64_t n, std::vector<long long> &rows) {
  rows.resize((size_t)n + 1);
  for (int64_t i = 0; i <= n; i++) rows[(size_t)i] = A.used + pt_off[i];
  return h2d(e, A.off.as<long long>() + A.slots.size(), rows.data(), rows.size() * sizeof(long long));
}

// the set call on the home engine: the arguments are checked, `win[i]` says that cloud i is the last of its id
int store_set(sgtd_engine *e, const uint32_t *frame_ids, const int64_t *pt_off, const float *points, int stride, int64_t n, const std::vector<unsigned char> &win,
              int k, double eps, int device_ptrs) {
  PinScope pin(e);
  HIPCHK(hipSetDevice(e->cfg.device_id));
  StoreChange W;
  int64_t incoming = 0;
  for (int64_t i = 0; i < n; i++) {
    if (!win[(size_t)i]) continue;
    const size_t id = frame_ids[i];
    if (id < e->st_slot_of.size() && e->st_slot_of[id] != SGTD_STORE_NONE) W.dies.push_back(e->st_slot_of[id]);
    if (points) incoming += pt_off[i + 1] - pt_off[i];
  }
  if (!points && W.dies.empty()) return SGTD_OK;
  const int64_t total = points ? pt_off[n] : 0;
  CloudArena *A = nullptr;
  CHK(store_prepare(e, W, total, points ? n : 0, incoming, &A));
  if (!points) { store_commit(e, W); return SGTD_OK; }
  // the call's clouds become the slots behind the last one: packed, their offsets, the covariances of the ones that stay
  const float *d_src = nullptr;
  CHK(points_on_device(e, e->st_stage, points, (size_t)total * stride, device_ptrs, &d_src));
  CHK(store_pack(e, *A, d_src, stride, total, A->used));
  std::vector<long long> rows;
  CHK(store_tail_rows(e, *A, pt_off, n, rows));
  const int first = (int)A->slots.size();
  std::vector<int> tiles[2];
  for (int64_t i = 0; i < n; i++) {
    if (!win[(size_t)i]) continue;
    for (int64_t f = 0; f < pt_off[i + 1] - pt_off[i]; f += SGTD_REG_THREADS) { tiles[0].push_back(first + (int)i); tiles[1].push_back((int)f); }
  }
  const size_t nt = tiles[0].size();
  if (nt) {
    tiles[0].insert(tiles[0].end(), tiles[1].begin(), tiles[1].end());
    CHK(ensure(e, e->st_idx, 2 * nt * sizeof(int)));
    CHK(h2d(e, e->st_idx.p, tiles[0].data(), 2 * nt * sizeof(int)));
    RegParams P;
    std::memset(&P, 0, sizeof(P));
    P.pts = A->pts.as<float>(); P.stride = 3; P.pt_off = A->off.as<long long>(); P.cov = A->cov.as<double>();
    P.ctile_cloud = e->st_idx.as<int>(); P.ctile_first = P.ctile_cloud + nt; P.n_ctiles = (int)nt;
    P.o.k = k; P.o.plane_eps = eps;
    reg_cov_kernel<<<P.n_ctiles, SGTD_REG_THREADS, 0, e->stream>>>(P);
    HIPCHK(hipGetLastError());
  }
  CHK(xfer_sync(e));      // (rows, tiles and the caller's points are read until here)
  store_commit(e, W);
  CloudArena &cur = e->st;
  for (int64_t i = 0; i < n; i++) {
    const size_t id = frame_ids[i];
    const bool live = win[(size_t)i] != 0;
    cur.slots.push_back(CloudSlot{frame_ids[i], cur.used + pt_off[i], pt_off[i + 1] - pt_off[i], live});
    if (!live) continue;
    if (id >= e->st_slot_of.size()) e->st_slot_of.resize(id + 1, SGTD_STORE_NONE);
    e->st_slot_of[id] = (int)cur.slots.size() - 1;
    cur.live += pt_off[i + 1] - pt_off[i];
    e->st_frames++;
  }
  cur.used += total;
  e->st_k = k; e->st_eps = eps;
  if (!device_ptrs) free_buf(e->st_stage);      // (once a map: not worth keeping)
  return SGTD_OK;
}

const char kNoStored[] = "no stored registration: sgtd_register_stored has not run";

// The stored call's run on the home engine, behind store_room: the call's clouds packed behind the slots, their
// offsets, the dense run over the arena (targets = slots), the call's covariances copied out of the arena
int stored_run(sgtd_engine *c, const sgtd_register_options &o, const float *points, int stride, const int64_t *pt_off, int n_clouds, int device_ptrs,
               const int32_t *src, const int32_t *slot, const double *init, const double *d_init, int n) {
  sgtd_engine *e = c;
  CloudArena &A = c->st;
  DenseRun &R = c->stored;
  R.host_off.assign(pt_off, pt_off + n_clouds + 1);
  R.host_named.assign((size_t)n_clouds, 0);
  std::vector<int64_t> tgt_n((size_t)n);
  for (int k = 0; k < n; k++) {
    R.host_named[(size_t)src[k]] = 1;
    tgt_n[(size_t)k] = A.slots[(size_t)slot[k]].count;
  }
  if (n == 0) { R.host_soff.assign(1, 0); return SGTD_OK; }
  const int64_t total = pt_off[n_clouds];
  const float *d_src = nullptr;
  CHK(points_on_device(c, R.pts.buf, points, (size_t)total * stride, device_ptrs, &d_src));
  CHK(store_pack(c, A, d_src, stride, total, A.used));
  std::vector<long long> rows;
  CHK(store_tail_rows(c, A, pt_off, n_clouds, rows));
  const RegSite S{"sgtd_register_stored", R, A.pts.as<float>(), 3, A.cov.as<double>(), A.off.as<long long>(), (int)A.slots.size(), d_init};
  CHK(reg_run(c, S, o, pt_off, n_clouds, R.host_named.data(), src, slot, tgt_n.data(), init, n));
  CHK(need(c, R.cov, std::max<size_t>((size_t)total, 1) * 9));
  if (total) HIPCHK(hipMemcpyAsync(R.cov.p(), A.cov.as<double>() + (size_t)A.used * 9, (size_t)total * 9 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  CHK(xfer_sync(c));
  return SGTD_OK;
}

// what the stored calls check of the store's settings
int stored_settings(sgtd_engine *e, const char *call, int k_neighbors, double plane_eps) {
  const sgtd_engine *c = home_engine(e);
  if (c->st_k == 0 || (k_neighbors == c->st_k && plane_eps == c->st_eps)) return SGTD_OK;
  e->err = std::string(call) + ": k_neighbors and plane_eps must be the cloud store's (" + std::to_string(c->st_k) + ", " + std::to_string(c->st_eps) + ")";
  return SGTD_ERR_STATE;
}

// What both loops calls (sgtd_register_stored_loops, sgtd_register_stored_local_loops) check of the batch and of the
// queries' clouds, behind their options (k_neighbors, plane_eps: the checked options'), and the batch waited for.
// instead: what the refusal of a multi-device handle advises.
int loops_begin(sgtd_engine *e, const char *call, const char *instead, const float *points, int stride_floats, const int64_t *pt_off, int max_per_query,
                int start, int k_neighbors, double plane_eps) {
  if (max_per_query < 0 || start < SGTD_START_VERIFY || start > SGTD_START_ALIGNED) return SGTD_ERR_INVALID;
  if (!pt_off || (stride_floats != 3 && stride_floats != 4)) return SGTD_ERR_INVALID;
  if (e->grp) {
    e->err = std::string(call) + ": a multi-device handle's batch results live on several engines: " + instead;
    return SGTD_ERR_UNSUPPORTED;
  }
  if (!e->batch_valid || !e->verified) return needs(e, call, "sgtd_verify");
  if (start == SGTD_START_REFINED && !e->refined) return needs(e, call, "sgtd_refine_poses");
  if (start == SGTD_START_ALIGNED && !e->aligned) return needs(e, call, "sgtd_align_keypoints");
  if (!cloud_set_ok(pt_off, e->nq, stride_floats, points, false, nullptr)) return SGTD_ERR_INVALID;
  if (!gicp_caps_ok(pt_off, e->nq, 0)) { e->err = gicp_caps_text(call); return SGTD_ERR_UNSUPPORTED; }
  CHK(stored_settings(e, call, k_neighbors, plane_eps));
  HIPCHK(hipSetDevice(e->cfg.device_id));
  return sync_batch(e);
}

// the batch's poses a loops call starts from
const double *start_pose(sgtd_engine *c, int start) {
  return start == SGTD_START_REFINED ? c->r_pose.as<double>() : start == SGTD_START_ALIGNED ? c->a_pose.as<double>() : c->v_pose.as<double>();
}
}  // namespace

extern "C" {

int sgtd_set_frame_clouds(sgtd_handle e, const uint32_t *frame_ids, const int64_t *pt_off, const float *points, int stride_floats, int64_t n,
                          int k_neighbors, double plane_eps, int device_ptrs) {
  if (!e || n < 0 || n > std::numeric_limits<int>::max() - 1 || (n > 0 && !frame_ids)) return SGTD_ERR_INVALID;
  const bool put = n > 0 && points;
  if (put) {
    if (!cloud_set_ok(pt_off, (int)n, stride_floats, points, false, nullptr)) return SGTD_ERR_INVALID;
    if (k_neighbors < 3 || k_neighbors > SGTD_REG_MAX_K || !(std::isfinite(plane_eps) && plane_eps > 0.0)) return SGTD_ERR_INVALID;
  }
  for (int64_t i = 0; i < n; i++)
    if (frame_ids[i] >= (uint32_t)e->cfg.max_frame_n) return SGTD_ERR_FRAME_LIMIT;
  sgtd_engine *c = home_engine(e);
  if (n == 0) {
    if (frame_ids) return SGTD_OK;
    (void)hipSetDevice(c->cfg.device_id);
    (void)hipStreamSynchronize(c->stream);
    c->st = CloudArena();
    for (DevBuf *b : {&c->st_stage, &c->st_idx, &c->st_table}) free_buf(*b);
    c->st_slot_of.clear(); c->st_frames = 0; c->st_k = 0; c->st_eps = 0.0;
    c->st_serial = 0; c->st_table_serial = ~0ull;
    return SGTD_OK;
  }
  // the last cloud of an id wins; the store's live points behind the call
  std::vector<unsigned char> win((size_t)n, 0);
  std::unordered_set<uint32_t> seen;
  int64_t live = c->st.live;
  for (int64_t i = n - 1; i >= 0; i--) {
    if (!seen.insert(frame_ids[i]).second) continue;
    win[(size_t)i] = 1;
    const size_t id = frame_ids[i];
    if (id < c->st_slot_of.size() && c->st_slot_of[id] != SGTD_STORE_NONE) live -= c->st.slots[(size_t)c->st_slot_of[id]].count;
    if (put) live += pt_off[i + 1] - pt_off[i];
  }
  if (put) {
    for (int64_t i = 0; i < n; i++)
      if (pt_off[i + 1] - pt_off[i] > SGTD_REG_MAX_POINTS) {
        e->err = "sgtd_set_frame_clouds takes at most " + std::to_string(SGTD_REG_MAX_POINTS) + " points a cloud";
        return SGTD_ERR_UNSUPPORTED;
      }
    if (live > SGTD_CLOUD_STORE_MAX_POINTS) {
      e->err = "sgtd_set_frame_clouds: the cloud store holds at most " + std::to_string(SGTD_CLOUD_STORE_MAX_POINTS) + " live points";
      return SGTD_ERR_UNSUPPORTED;
    }
    if (c->st_k != 0 && (k_neighbors != c->st_k || plane_eps != c->st_eps)) {
      e->err = "sgtd_set_frame_clouds: the cloud store was made with k_neighbors " + std::to_string(c->st_k) + " and plane_eps " + std::to_string(c->st_eps) +
               ": forget all clouds first";
      return SGTD_ERR_STATE;
    }
  }
  const int st = store_set(c, frame_ids, pt_off, put ? points : nullptr, stride_floats, n, win, k_neighbors, plane_eps, device_ptrs);
  if (st != SGTD_OK && c != e) e->err = c->err;
  return st;
}

int sgtd_frame_clouds_info(sgtd_handle e, int64_t *n_frames, int64_t *n_points, int64_t *device_bytes, int32_t *k_neighbors, double *plane_eps) {
  if (!e) return SGTD_ERR_INVALID;
  const sgtd_engine *c = home_engine(e);
  if (n_frames) *n_frames = c->st_frames;
  if (n_points) *n_points = c->st.live;
  if (device_bytes) *device_bytes = (int64_t)(c->st.pts.bytes + c->st.cov.bytes + c->st.off.bytes);
  if (k_neighbors) *k_neighbors = c->st_k;
  if (plane_eps) *plane_eps = c->st_eps;
  return SGTD_OK;
}

int sgtd_result_frame_cloud(sgtd_handle e, uint32_t frame, float *xyz, double *cov, int64_t capacity, int64_t *n) {
  if (!e || capacity < 0) return SGTD_ERR_INVALID;
  sgtd_engine *c = home_engine(e);
  const int slot = frame < c->st_slot_of.size() ? c->st_slot_of[frame] : SGTD_STORE_NONE;
  if (slot == SGTD_STORE_NONE) { if (n) *n = -1; return SGTD_OK; }
  const CloudSlot &sl = c->st.slots[(size_t)slot];
  if (n) *n = sl.count;
  const size_t m = (size_t)std::min(sl.count, capacity);
  CopyOut out(e, c);
  out.get(xyz, c->st.pts.as<float>() + (size_t)sl.first * 3, m * 3 * sizeof(float));
  out.get(cov, c->st.cov.as<double>() + (size_t)sl.first * 9, m * 9 * sizeof(double));
  CHK(out.finish());
  return sl.count > capacity && (xyz || cov) ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int sgtd_register_stored(sgtd_handle e, const sgtd_register_options *opt, const float *points, int stride_floats, const int64_t *pt_off, int n_clouds,
                         const int32_t *src_cloud, const uint32_t *tgt_frame, const double *init_pose, int n_pairs, int device_ptrs) {
  sgtd_register_options o;
  CHK(dense_check(e, "sgtd_register_stored", opt, &o, points, stride_floats, pt_off, n_clouds, src_cloud, tgt_frame, init_pose, n_pairs,
                  [](int) { return true; }));
  const int64_t total = pt_off[n_clouds];
  CHK(stored_settings(e, "sgtd_register_stored", o.k_neighbors, o.plane_eps));
  {
    const sgtd_engine *c = home_engine(e);
    for (int k = 0; k < n_pairs; k++)
      if (tgt_frame[k] >= c->st_slot_of.size() || c->st_slot_of[tgt_frame[k]] == SGTD_STORE_NONE) {
        e->err = "sgtd_register_stored: frame " + std::to_string(tgt_frame[k]) + " has no stored cloud (sgtd_set_frame_clouds)";
        return SGTD_ERR_INVALID;
      }
  }
  StageRun<int> run(e, &sgtd_engine::stored);
  run.c->sr_loops = false;
  run.on_device([&](sgtd_engine *c) -> int {
    if (n_pairs > 0) CHK(store_room(c, total, n_clouds));
    std::vector<int32_t> slot((size_t)n_pairs);
    for (int k = 0; k < n_pairs; k++) slot[(size_t)k] = c->st_slot_of[tgt_frame[k]];
    return stored_run(c, o, points, stride_floats, pt_off, n_clouds, device_ptrs, src_cloud, slot.data(), init_pose, nullptr, n_pairs);
  });
  return run.end(n_pairs);
}

int sgtd_register_stored_loops(sgtd_handle e, const sgtd_register_options *opt, const float *points, int stride_floats, const int64_t *pt_off,
                               int max_per_query, int start, int device_ptrs) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_register_options o;
  CHK(dense_options(opt, &o));
  CHK(loops_begin(e, "sgtd_register_stored_loops", "form the pairs and use sgtd_register_stored", points, stride_floats, pt_off, max_per_query, start,
                  o.k_neighbors, o.plane_eps));
  const int nq = e->nq, cn = e->dc.cand_num, mpq = std::min(max_per_query, cn);
  const int64_t total = pt_off[nq];
  const size_t upper = (size_t)nq * mpq;
  int n = 0;
  StageRun<int> run(e, &sgtd_engine::stored);
  e->sr_loops = true;
  e->sr_rows.clear();
  run.on_device([&](sgtd_engine *c) -> int {
    std::vector<int32_t> src, slot;
    if (upper > 0 && c->st_frames > 0) {
      CHK(store_room(c, total, nq));
      CHK(store_table(c));
      // the pairs: counts per query, their scan, the rows; the host reads the total and the rows back once
      const size_t o_count = 0, o_first = o_count + relax_up(((size_t)nq + 1) * sizeof(u32)), o_rows = o_first + relax_up(((size_t)nq + 1) * sizeof(u32)),
                   o_init = o_rows + relax_up(upper * sizeof(int4));
      CHK(ensure(c, c->sr_pairs, o_init + upper * 12 * sizeof(double)));
      char *pb = c->sr_pairs.as<char>();
      c->sr_init_off = o_init;
      StorePairParams P;
      P.score = c->v_score.as<double>(); P.n_cand = c->n_cand.as<int>(); P.cand_frame = c->cand_frame.as<int>();
      P.pose = start_pose(c, start);
      P.slot_of = c->st_table.as<int>(); P.n_ids = (u32)c->st_slot_of.size();
      P.cand_num = cn; P.nq = nq; P.max_per_query = mpq;
      P.count = reinterpret_cast<u32 *>(pb + o_count); P.first = reinterpret_cast<const u32 *>(pb + o_first);
      P.rows = reinterpret_cast<int4 *>(pb + o_rows); P.init = reinterpret_cast<double *>(pb + o_init);
      HIPCHK(hipMemsetAsync(P.count, 0, ((size_t)nq + 1) * sizeof(u32), c->stream));
      const int grid = grid_for(nq, SGTD_STORE_THREADS / 64);
      store_pairs_kernel<<<grid, SGTD_STORE_THREADS, 0, c->stream>>>(P, 0);
      HIPCHK(hipGetLastError());
      CHK(device_scan(c, P.count, reinterpret_cast<u32 *>(pb + o_first), (long long)nq + 1));
      store_pairs_kernel<<<grid, SGTD_STORE_THREADS, 0, c->stream>>>(P, 1);
      HIPCHK(hipGetLastError());
      u32 found = 0;
      std::vector<int32_t> rows(upper * 4);
      CHK(d2h(c, &found, P.first + nq, sizeof(u32)));
      CHK(d2h(c, rows.data(), P.rows, upper * sizeof(int4)));
      CHK(xfer_sync(c));
      int64_t total_src = 0;
      for (u32 k = 0; k < found; k++) total_src += pt_off[rows[(size_t)k * 4] + 1] - pt_off[rows[(size_t)k * 4]];
      if (found > SGTD_REG_MAX_PAIRS || total_src > SGTD_REG_MAX_SOURCE_POINTS) {
        c->err = "sgtd_register_stored_loops: the pairs formed pass " + std::to_string(SGTD_REG_MAX_PAIRS) + " pairs or " +
                 std::to_string(SGTD_REG_MAX_SOURCE_POINTS) + " source points over the pairs";
        return SGTD_ERR_UNSUPPORTED;
      }
      n = (int)found;
      for (int k = 0; k < n; k++) {
        const int32_t *r = rows.data() + (size_t)k * 4;
        src.push_back(r[0]); slot.push_back(r[3]);
        c->sr_rows.insert(c->sr_rows.end(), r, r + 3);
      }
    }
    return stored_run(c, o, points, stride_floats, pt_off, nq, device_ptrs, src.data(), slot.data(), nullptr,
                      n ? reinterpret_cast<const double *>(c->sr_pairs.as<char>() + c->sr_init_off) : nullptr, n);
  });
  return run.end(n);
}

int sgtd_result_stored_pairs(sgtd_handle e, int32_t *query, int32_t *cand, int32_t *frame, double *init, int64_t capacity, int64_t *n) {
  if (!e || capacity < 0) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::stored, kNoStored, &c));
  if (!c->sr_loops) { e->err = "no pair rows: sgtd_register_stored_loops has not run"; return SGTD_ERR_STATE; }
  const int64_t need = c->stored.n;
  if (n) *n = need;
  const size_t m = (size_t)std::min(need, capacity);
  for (size_t k = 0; k < m; k++) {
    if (query) query[k] = c->sr_rows[k * 3];
    if (cand) cand[k] = c->sr_rows[k * 3 + 1];
    if (frame) frame[k] = c->sr_rows[k * 3 + 2];
  }
  if (m) {
    CopyOut out(e, c);
    out.get(init, c->sr_pairs.as<char>() + c->sr_init_off, m * 12 * sizeof(double));
    CHK(out.finish());
  }
  return need > capacity && (query || cand || frame || init) ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int sgtd_result_stored_registered(sgtd_handle e, double *pose, double *fitness, double *cost, int32_t *n_matched, int32_t *iterations, int32_t *status) {
  return dense_rows_out(e, &sgtd_engine::stored, kNoStored, pose, fitness, cost, n_matched, iterations, status);
}

int sgtd_result_stored_covariances(sgtd_handle e, int cloud, double *cov, int64_t capacity, int64_t *n) {
  return dense_cov_out(e, &sgtd_engine::stored, kNoStored, cloud, cov, capacity, n);
}

int sgtd_result_stored_matches(sgtd_handle e, int pair, int32_t *tgt_index, double *d2, int64_t capacity, int64_t *n) {
  return dense_matches_out(e, &sgtd_engine::stored, kNoStored, pair, tgt_index, d2, capacity, n);
}

int sgtd_stored_register_stage_ms(sgtd_handle e, float *ms_cov, float *ms_search, float *ms_rest, float *ms_total) {
  return dense_ms_out(e, &sgtd_engine::stored, kNoStored, ms_cov, ms_search, ms_rest, ms_total);
}

}  // extern "C"

// ---- sgtd_register_voxels: voxelised GICP against voxel maps (voxel_register_kernels.hip.h) ----
namespace {
static_assert(SGTD_VREG_W == SGTD_VREG_SUM_W, "the voxel kernels' sizes are the header's");

// Where a voxel run keeps its buffers and finds its clouds: sgtd_register_voxels' own arrays, or
// sgtd_register_stored_voxels' over the cloud store's arena, whose stored clouds come before the call's.
struct VregSite {
  const char *call;
  VoxelRun &R;         // the run's buffers, mode, host arrays and clock
  const float *pts;                 // the points of every cloud the kernels may name, on the device
  int stride;
  double *cov;                      // the covariances of those clouds; NULL: the run's cov, grown to the call's points
  const long long *d_off;           // the clouds' offsets where they are on the device already; NULL: pt_off is uploaded
  int first;                        // the index the kernels know the call's cloud 0 by
  // the members where they were formed on the device (sgtd_register_stored_local_loops): their clouds, maps, first points
  // [members + 1] and poses, the members' points in all, and the pairs' start poses; mem_cloud, mem_n, map_pose and init
  // are NULL then
  const int *d_mem_cloud = nullptr, *d_mem_map = nullptr, *d_mem_pt_off = nullptr;
  const double *d_map_pose = nullptr;
  long long d_member_pts = 0;
  const double *d_init = nullptr;
};

// One voxelised run.  pt_off, n_clouds, named, src: the call's clouds, which of them need covariances, the pairs'
// sources; mem_cloud, mem_n: the maps' members as the kernels know them, and their sizes
int vreg_run(sgtd_engine *c, const VregSite &S, const sgtd_voxel_register_options &o, const int64_t *pt_off, int n_clouds, const unsigned char *named,
             const int32_t *map_off, const int32_t *mem_cloud, const int64_t *mem_n, const double *map_pose, int n_maps, const int32_t *src,
             const int32_t *tgt, const double *init, int n) {
  sgtd_engine *e = c;      // (HIPCHK reports on the engine that runs the pass)
  const bool timed = c->timing;
  VoxelRun &R = S.R;
  LapClock &clock = R.clock;
  CHK(clock.start(c, timed));
  const size_t total = (size_t)pt_off[n_clouds];
  const int mode = o.neighbor_mode, n_members = n_maps ? map_off[n_maps] : 0;
  R.mode = mode;
  // the members' points back to back, the tiles: of the pairs' sources, of the clouds that need covariances
  const bool on_device = S.d_mem_cloud != nullptr;
  std::vector<int> mem_map, mem_pt_off;
  if (!on_device) {
    mem_map.resize((size_t)n_members);
    mem_pt_off.assign((size_t)n_members + 1, 0);
    for (int m = 0; m < n_maps; m++)
      for (int j = map_off[m]; j < map_off[m + 1]; j++) {
        mem_map[(size_t)j] = m;
        mem_pt_off[(size_t)j + 1] = mem_pt_off[(size_t)j] + (int)mem_n[j];
      }
  }
  const long long MP = on_device ? S.d_member_pts : mem_pt_off[(size_t)n_members];
  std::vector<int> &soff = R.host_soff;
  GicpIndex G(R.host_up);
  G.tiles(pt_off, n_clouds, src, n, named, &soff);
  const int total_src = soff[(size_t)n], n_tiles = (int)G.tile_pair.size();

  // the index upload: src, tgt_map, src_off, map_off, map_cloud, mem_map, mem_pt_off, the tiles (clouds by the index the
  // kernels know them by)
  G.u_src = G.put(src, (size_t)n);
  const size_t u_tgt = G.put(tgt, (size_t)n);
  G.u_soff = G.put(soff.data(), soff.size());
  const size_t u_moff = n_maps ? G.put(map_off, (size_t)n_maps + 1) : G.up.size(), u_mcl = G.put(mem_cloud, on_device ? 0 : (size_t)n_members);
  const size_t u_mmap = G.put(mem_map.data(), mem_map.size()), u_mpo = G.put(mem_pt_off.data(), mem_pt_off.size());
  if (S.first) {
    for (int k = 0; k < n; k++) R.host_up[G.u_src + (size_t)k] += S.first;
    for (int &cl : G.ctile_cloud) cl += S.first;
  }
  G.put_tiles();
  const size_t o_off = 0, o_init = o_off + relax_up((size_t)(n_clouds + 1) * sizeof(int64_t)), o_pose = o_init + relax_up((size_t)n * 12 * sizeof(double)),
               o_idx = o_pose + relax_up((size_t)n_members * 12 * sizeof(double)), in_bytes = o_idx + relax_up(G.up.size() * sizeof(int));
  const size_t ts = (size_t)std::max(total_src, 1), mp = (size_t)std::max<long long>(MP, 1), nn = (size_t)std::max(n, 1);
  const RegOut out((size_t)n, true);
  CHK(need(c, R.in, in_bytes));
  if (!S.cov) CHK(need(c, R.cov, std::max<size_t>(total, 1) * 9));
  CHK(need_runs(c, R.runs, mp));
  CHK(need(c, R.map_vox, (size_t)n_maps + 1));
  CHK(need(c, R.vid, ts * mode));
  CHK(need(c, R.mw, ts * mode * 9));
  CHK(need(c, R.state, nn));
  CHK(need(c, R.out, out.bytes()));
  CHK(need(c, R.ctl, 64));
  char *in = R.in.p();
  if (!S.d_off) CHK(h2d(c, in + o_off, pt_off, (size_t)(n_clouds + 1) * sizeof(int64_t)));
  if (init) CHK(h2d(c, in + o_init, init, (size_t)n * 12 * sizeof(double)));
  if (map_pose) CHK(h2d(c, in + o_pose, map_pose, (size_t)n_members * 12 * sizeof(double)));
  CHK(h2d(c, in + o_idx, G.up.data(), G.up.size() * sizeof(int)));

  RegParams P;
  const int *di = reinterpret_cast<const int *>(in + o_idx);
  void *ob = R.out.p();
  gicp_params(P, G, S.pts, S.stride, S.d_off ? static_cast<const void *>(S.d_off) : in + o_off, di, n, ts, S.cov ? S.cov : R.cov.p(), R.state.p(),
              R.ctl.p(), out, ob,
              gicp_options(o.k_neighbors, o.max_iterations, o.lm_max_trials, std::numeric_limits<double>::infinity(), o.lm_init_lambda_factor, o.rotation_eps,
                           o.translation_eps, o.plane_eps));
  VregParams V;
  std::memset(&V, 0, sizeof(V));
  V.map_off = di + u_moff; V.map_cloud = di + u_mcl; V.mem_map = di + u_mmap; V.mem_pt_off = di + u_mpo;
  V.map_pose = map_pose ? reinterpret_cast<const double *>(in + o_pose) : nullptr;
  if (on_device) { V.map_cloud = S.d_mem_cloud; V.mem_map = S.d_mem_map; V.mem_pt_off = S.d_mem_pt_off; V.map_pose = S.d_map_pose; }
  V.tgt_map = di + u_tgt;
  V.n_maps = n_maps; V.n_members = n_members; V.n_member_pts = (int)MP; V.mode = mode; V.res = o.voxel_resolution;
  V.map_vox = R.map_vox.p();
  V.vid = R.vid.p(); V.Mw = R.mw.p();
  V.out_corr = out.corr(ob);

  hipStream_t s = c->stream;
  if (timed) { HIPCHK(hipEventRecord(clock.ev[2], s)); HIPCHK(hipEventRecord(clock.ev[0], s)); }
  if (P.n_ctiles) reg_cov_kernel<<<P.n_ctiles, SGTD_REG_THREADS, 0, s>>>(P);
  HIPCHK(hipGetLastError());
  if (timed) CHK(clock.lap(c, 0));

  // the maps: keys, the stable sort, the voxels' heads, the Gaussians, the maps' ranges
  u32 n_vox = 0;
  if (MP > 0) {
    u64 *keys = nullptr;
    u32 *order = nullptr;
    vreg_keys_kernel<<<grid_for(MP, 256), 256, 0, s>>>(P, V, R.runs.key_a.p(), R.runs.val_a.p());
    HIPCHK(hipGetLastError());
    CHK(sorted_runs(c, R.runs, MP, 48 + key_bits((u64)n_maps), true, (u64)n_maps << 48, &keys, &order));
    HIPCHK(hipGetLastError());
    CHK(d2h(c, &n_vox, R.runs.excl.p() + MP, sizeof(u32)));
    CHK(xfer_sync(c));
    V.vkey = R.runs.vkey.p(); V.vstart = R.runs.vstart.p(); V.order = order; V.n_vox = n_vox;
    const size_t nv = std::max<size_t>(n_vox, 1);
    CHK(need(c, R.mean, nv * 3));
    CHK(need(c, R.vcov, nv * 9));
    V.vmean = R.mean.p(); V.vcov = R.vcov.p();
    if (n_vox) vreg_voxel_kernel<<<grid_for(n_vox, 4), 256, 0, s>>>(P, V);
  }
  vreg_ranges_kernel<<<grid_for(n_maps + 1, 256), 256, 0, s>>>(V);
  HIPCHK(hipGetLastError());
  R.host_map_vox.assign((size_t)n_maps + 1, 0);
  CHK(d2h(c, R.host_map_vox.data(), V.map_vox, ((size_t)n_maps + 1) * sizeof(u32)));
  CHK(xfer_sync(c));
  if (timed) CHK(clock.lap(c, 1));
  if (n == 0) {
    if (timed) CHK(clock.span(c, 2, 1, 4, false));
    return SGTD_OK;
  }

  const std::vector<u32> &mv = R.host_map_vox;
  int unfinished = 0;
  for (int k = 0; k < n; k++)
    if (soff[(size_t)k + 1] > soff[(size_t)k] && mv[(size_t)tgt[k] + 1] > mv[(size_t)tgt[k]]) unfinished++;
  CHK(h2d(c, P.unfinished, &unfinished, sizeof(int)));
  vreg_init_kernel<<<grid_for(n, SGTD_REG_W), SGTD_REG_W, 0, s>>>(P, V, init ? reinterpret_cast<const double *>(in + o_init) : S.d_init);
  HIPCHK(hipGetLastError());
  CHK(gicp_rounds(c, S.call, P, unfinished, [&]() -> int {
    if (timed) CHK(clock.lap(c, 3));
    vreg_corr_kernel<<<n_tiles, SGTD_REG_THREADS, 0, s>>>(P, V, 0);
    if (timed) CHK(clock.lap(c, 2));
    vreg_lin_kernel<<<n, SGTD_REG_W, 0, s>>>(P, V);
    vreg_trial_kernel<<<n, SGTD_REG_W, 0, s>>>(P, V);
    HIPCHK(hipGetLastError());
    return SGTD_OK;
  }));
  if (timed) CHK(clock.lap(c, 3));
  if (n_tiles) {
    vreg_corr_kernel<<<n_tiles, SGTD_REG_THREADS, 0, s>>>(P, V, 1);
    if (timed) CHK(clock.lap(c, 2));
  }
  vreg_final_kernel<<<n, SGTD_REG_W, 0, s>>>(P, V);
  HIPCHK(hipGetLastError());
  if (timed) {
    CHK(clock.lap(c, 3));
    CHK(clock.span(c, 2, 1, 4, false));
  }
  CHK(xfer_sync(c));
  return SGTD_OK;
}

// sgtd_register_voxels' run: every cloud is the call's, and a cloud that is a source or a member needs covariances
int vreg_clouds_run(sgtd_engine *c, const sgtd_voxel_register_options &o, const float *points, int stride, const int64_t *pt_off, int n_clouds,
                    const int32_t *map_off, const int32_t *map_cloud, const double *map_pose, int n_maps, const int32_t *src, const int32_t *tgt,
                    const double *init, int n) {
  const int n_members = n_maps ? map_off[n_maps] : 0;
  std::vector<unsigned char> named((size_t)n_clouds, 0);
  std::vector<int64_t> mem_n((size_t)n_members);
  for (int j = 0; j < n_members; j++) {
    named[(size_t)map_cloud[j]] = 1;
    mem_n[(size_t)j] = pt_off[map_cloud[j] + 1] - pt_off[map_cloud[j]];
  }
  for (int k = 0; k < n; k++) named[(size_t)src[k]] = 1;
  const VregSite S{"sgtd_register_voxels", c->vox, points, stride, nullptr, nullptr, 0};
  return vreg_run(c, S, o, pt_off, n_clouds, named.data(), map_off, map_cloud, mem_n.data(), map_pose, n_maps, src, tgt, init, n);
}

// the options of a voxel call: the defaults or the caller's, checked
int vreg_options(const sgtd_voxel_register_options *opt, sgtd_voxel_register_options *o) {
  sgtd_default_voxel_register_options(o);
  if (opt) *o = *opt;
  if (!gicp_options_ok(o->k_neighbors, o->max_iterations, o->lm_max_trials, o->reserved, o->lm_init_lambda_factor, o->rotation_eps, o->translation_eps,
                       o->plane_eps) ||
      !(std::isfinite(o->voxel_resolution) && o->voxel_resolution > 0.0) || (o->neighbor_mode != 1 && o->neighbor_mode != 7 && o->neighbor_mode != 27))
    return SGTD_ERR_INVALID;
  return SGTD_OK;
}

// What both voxel calls check of their arguments before the device is touched, in sgtd_register_voxels' order.
// member_points(j, &np): the points of member j, or the code that rejects it (its text is the callback's).
template <class MemberPoints>
int vreg_check(sgtd_engine *e, const char *call, const sgtd_voxel_register_options *opt, sgtd_voxel_register_options *o, const float *points,
               int stride_floats, const int64_t *pt_off, int n_clouds, const int32_t *map_off, const void *members, const double *map_pose, int n_maps,
               const int32_t *src_cloud, const int32_t *tgt_map, const double *init_pose, int n_pairs, MemberPoints &&member_points) {
  if (!e || n_pairs < 0 || n_maps < 0) return SGTD_ERR_INVALID;
  if (n_pairs > 0 && (!src_cloud || !tgt_map)) return SGTD_ERR_INVALID;
  if (n_maps > 0 && !map_off) return SGTD_ERR_INVALID;
  CHK(vreg_options(opt, o));
  if (!cloud_set_ok(pt_off, n_clouds, stride_floats, points, false, nullptr)) return SGTD_ERR_INVALID;
  if (n_maps > 0 && map_off[0] != 0) return SGTD_ERR_INVALID;
  for (int m = 0; m < n_maps; m++)
    if (map_off[m + 1] < map_off[m]) return SGTD_ERR_INVALID;
  const int n_members = n_maps ? map_off[n_maps] : 0;
  if (n_members > 0 && !members) return SGTD_ERR_INVALID;
  int64_t total_src = 0, member_pts = 0;
  for (int j = 0; j < n_members; j++) {
    int64_t np = 0;
    CHK(member_points(j, &np));
    member_pts += np;
  }
  for (int k = 0; k < n_pairs; k++) {
    if (src_cloud[k] < 0 || src_cloud[k] >= n_clouds || tgt_map[k] < 0 || tgt_map[k] >= n_maps) return SGTD_ERR_INVALID;
    total_src += pt_off[src_cloud[k] + 1] - pt_off[src_cloud[k]];
  }
  if (init_pose && !relax_finite(init_pose, (size_t)n_pairs * 12)) return SGTD_ERR_INVALID;
  if (map_pose && !relax_finite(map_pose, (size_t)n_members * 12)) return SGTD_ERR_INVALID;
  if (!gicp_caps_ok(pt_off, n_clouds, n_pairs)) {
    e->err = gicp_caps_text(call) + " and " + std::to_string(SGTD_REG_MAX_PAIRS) + " pairs";
    return SGTD_ERR_UNSUPPORTED;
  }
  if (n_maps > SGTD_VREG_MAX_MAPS) {
    e->err = std::string(call) + " takes at most " + std::to_string(SGTD_VREG_MAX_MAPS) + " maps (SGTD_VREG_MAX_MAPS)";
    return SGTD_ERR_UNSUPPORTED;
  }
  if (member_pts > SGTD_VREG_MAX_MEMBER_POINTS) {
    e->err = std::string(call) + " takes at most " + std::to_string(SGTD_VREG_MAX_MEMBER_POINTS) + " member points over the maps (SGTD_VREG_MAX_MEMBER_POINTS)";
    return SGTD_ERR_UNSUPPORTED;
  }
  if (total_src * o->neighbor_mode > SGTD_VREG_MAX_CORR) {
    e->err = std::string(call) + " takes at most " + std::to_string(SGTD_VREG_MAX_CORR) +
             " for the source points over the pairs times neighbor_mode (SGTD_VREG_MAX_CORR)";
    return SGTD_ERR_UNSUPPORTED;
  }
  return SGTD_OK;
}

// The getters of a voxel run, over the buffers and host arrays of the call that made it: `run` on e's home engine
// (`missing`: what the handle is told where that call has not run)
int vreg_rows_out(sgtd_engine *e, VoxelRun sgtd_engine::*run, const char *missing, double *pose, double *fitness, double *cost, int32_t *n_matched,
                  int32_t *n_corr, int32_t *iterations, int32_t *status) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, run, missing, &c));
  VoxelRun &R = c->*run;
  if (R.n == 0) return SGTD_OK;
  return reg_rows_out(e, c, RegOut((size_t)R.n, true), R.out.p(), pose, fitness, cost, n_matched, n_corr, iterations, status);
}

int vreg_map_out(sgtd_engine *e, VoxelRun sgtd_engine::*run, const char *missing, int map, int32_t *coord, int32_t *n_points, double *mean, double *cov,
                 int64_t capacity, int64_t *n) {
  if (!e || capacity < 0) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, run, missing, &c));
  const VoxelRun &R = c->*run;
  const std::vector<u32> &map_vox = R.host_map_vox;
  if (map < 0 || (size_t)map + 1 >= map_vox.size()) return SGTD_ERR_INVALID;
  const int64_t first = map_vox[(size_t)map], need = (int64_t)map_vox[(size_t)map + 1] - first;
  if (n) *n = need;
  const bool any = coord || n_points || mean || cov;
  const size_t m = any ? (size_t)std::min(need, capacity) : 0;
  std::vector<u64> keys(coord ? m : 0);
  std::vector<u32> starts(n_points && m ? m + 1 : 0);
  CopyOut out(e, c);
  out.get(keys.data(), R.runs.vkey.p() + first, keys.size() * sizeof(u64));
  out.get(starts.data(), R.runs.vstart.p() + first, starts.size() * sizeof(u32));
  out.get(mean, R.mean.p() + (size_t)first * 3, m * 3 * sizeof(double));
  out.get(cov, R.vcov.p() + (size_t)first * 9, m * 9 * sizeof(double));
  CHK(out.finish());
  for (size_t v = 0; v < keys.size(); v++)
    for (int a = 0; a < 3; a++) coord[v * 3 + a] = (int32_t)((keys[v] >> (32 - 16 * a)) & 0xFFFFu) - 32768;
  for (size_t v = 0; v + 1 < starts.size(); v++) n_points[v] = (int32_t)(starts[v + 1] - starts[v]);
  return need > capacity && any ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int vreg_matches_out(sgtd_engine *e, VoxelRun sgtd_engine::*run, const char *missing, int pair, int32_t *voxel, int64_t capacity, int64_t *n) {
  if (!e || capacity < 0) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, run, missing, &c));
  VoxelRun &R = c->*run;
  if (pair < 0 || pair >= R.n) return SGTD_ERR_INVALID;
  const int64_t first = (int64_t)R.host_soff[(size_t)pair] * R.mode;
  const int64_t need = (int64_t)R.host_soff[(size_t)pair + 1] * R.mode - first;
  if (n) *n = need;
  CopyOut out(e, c);
  out.get(voxel, R.vid.p() + first, (size_t)std::min(need, capacity) * sizeof(int));
  CHK(out.finish());
  return need > capacity && voxel ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int vreg_ms_out(sgtd_engine *e, VoxelRun sgtd_engine::*run, const char *missing, float *ms_cov, float *ms_map, float *ms_corr, float *ms_rest,
                float *ms_total) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, run, missing, &c));
  const float *ms = (c->*run).clock.ms;
  if (ms_cov) *ms_cov = ms[0];
  if (ms_map) *ms_map = ms[1];
  if (ms_corr) *ms_corr = ms[2];
  if (ms_rest) *ms_rest = ms[3];
  if (ms_total) *ms_total = ms[4];
  return SGTD_OK;
}

const char kNoVoxelRegistered[] = "no voxel registration: sgtd_register_voxels has not run";
}  // namespace

extern "C" {

void sgtd_default_voxel_register_options(sgtd_voxel_register_options *o) {
  if (!o) return;
  o->voxel_resolution = 1.0; o->neighbor_mode = 1;
  o->k_neighbors = 20; o->max_iterations = 64; o->lm_max_trials = 10;
  o->lm_init_lambda_factor = 1e-9; o->rotation_eps = 2e-3; o->translation_eps = 5e-4; o->plane_eps = 1e-3;
  o->reserved = 0;
}

int sgtd_register_voxels(sgtd_handle e, const sgtd_voxel_register_options *opt, const float *points, int stride_floats, const int64_t *pt_off, int n_clouds,
                         const int32_t *map_off, const int32_t *map_cloud, const double *map_pose, int n_maps, const int32_t *src_cloud,
                         const int32_t *tgt_map, const double *init_pose, int n_pairs, int device_ptrs) {
  sgtd_voxel_register_options o;
  CHK(vreg_check(e, "sgtd_register_voxels", opt, &o, points, stride_floats, pt_off, n_clouds, map_off, map_cloud, map_pose, n_maps, src_cloud, tgt_map,
                 init_pose, n_pairs, [&](int j, int64_t *np) -> int {
                   if (map_cloud[j] < 0 || map_cloud[j] >= n_clouds) return SGTD_ERR_INVALID;
                   *np = pt_off[map_cloud[j] + 1] - pt_off[map_cloud[j]];
                   return SGTD_OK;
                 }));
  const int64_t total = pt_off[n_clouds];
  StageRun<int> run(e, &sgtd_engine::vox);
  run.on_device([&](sgtd_engine *c) -> int {
    const float *d_pts = nullptr;
    CHK(points_on_device(c, c->vox.pts.buf, points, (size_t)total * stride_floats, device_ptrs, &d_pts));
    return vreg_clouds_run(c, o, d_pts, stride_floats, pt_off, n_clouds, map_off, map_cloud, map_pose, n_maps, src_cloud, tgt_map, init_pose, n_pairs);
  });
  return run.end(n_pairs);
}

int sgtd_result_voxel_registered(sgtd_handle e, double *pose, double *fitness, double *cost, int32_t *n_matched, int32_t *n_corr, int32_t *iterations,
                                 int32_t *status) {
  return vreg_rows_out(e, &sgtd_engine::vox, kNoVoxelRegistered, pose, fitness, cost, n_matched, n_corr, iterations, status);
}

int sgtd_result_voxel_map(sgtd_handle e, int map, int32_t *coord, int32_t *n_points, double *mean, double *cov, int64_t capacity, int64_t *n) {
  return vreg_map_out(e, &sgtd_engine::vox, kNoVoxelRegistered, map, coord, n_points, mean, cov, capacity, n);
}

int sgtd_result_voxel_matches(sgtd_handle e, int pair, int32_t *voxel, int64_t capacity, int64_t *n) {
  return vreg_matches_out(e, &sgtd_engine::vox, kNoVoxelRegistered, pair, voxel, capacity, n);
}

int sgtd_voxel_register_stage_ms(sgtd_handle e, float *ms_cov, float *ms_map, float *ms_corr, float *ms_rest, float *ms_total) {
  return vreg_ms_out(e, &sgtd_engine::vox, kNoVoxelRegistered, ms_cov, ms_map, ms_corr, ms_rest, ms_total);
}

}  // extern "C"

// ---- sgtd_register_stored_voxels: the voxel run over the cloud store's arena ----
namespace {
const char kNoStoredVoxel[] = "no stored voxel registration: sgtd_register_stored_voxels has not run";

// the members of a run where sgtd_register_stored_local_loops formed them on the device (VregSite's d_* members)
struct StoredMembers {
  const int *slot, *map, *pt_off;
  const double *pose;
  long long pts;
  const double *init;
};

// The stored voxel calls' run on the home engine, behind store_room: the call's clouds packed behind the slots, their
// offsets, the voxel run over the arena (members = slots, given by the host or formed on the device).  Nothing reads the
// call's covariances afterwards (the call has no covariance getter), so they stay where the run left them in the arena.
int stored_voxels_run(sgtd_engine *c, const sgtd_voxel_register_options &o, const float *points, int stride, const int64_t *pt_off, int n_clouds,
                      int device_ptrs, const int32_t *map_off, const int32_t *slot, const double *map_pose, int n_maps, const int32_t *src,
                      const int32_t *tgt, const double *init, int n, const StoredMembers *formed = nullptr) {
  CloudArena &A = c->st;
  const int n_members = n_maps ? map_off[n_maps] : 0;
  std::vector<unsigned char> named((size_t)n_clouds, 0);
  std::vector<int64_t> mem_n(formed ? 0 : (size_t)n_members);
  for (size_t j = 0; j < mem_n.size(); j++) mem_n[j] = A.slots[(size_t)slot[j]].count;
  for (int k = 0; k < n; k++) named[(size_t)src[k]] = 1;
  const int64_t total = pt_off[n_clouds];
  const float *d_src = nullptr;
  CHK(points_on_device(c, c->svox.pts.buf, points, (size_t)total * stride, device_ptrs, &d_src));
  CHK(store_pack(c, A, d_src, stride, total, A.used));
  std::vector<long long> rows;
  CHK(store_tail_rows(c, A, pt_off, n_clouds, rows));
  VregSite S{formed ? "sgtd_register_stored_local_loops" : "sgtd_register_stored_voxels", c->svox, A.pts.as<float>(), 3, A.cov.as<double>(),
             A.off.as<long long>(), (int)A.slots.size()};
  if (formed) {
    S.d_mem_cloud = formed->slot; S.d_mem_map = formed->map; S.d_mem_pt_off = formed->pt_off; S.d_map_pose = formed->pose;
    S.d_member_pts = formed->pts; S.d_init = formed->init;
  }
  return vreg_run(c, S, o, pt_off, n_clouds, named.data(), map_off, slot, mem_n.data(), map_pose, n_maps, src, tgt, init, n);      // (it ends waited for)
}
}  // namespace

extern "C" {

int sgtd_register_stored_voxels(sgtd_handle e, const sgtd_voxel_register_options *opt, const float *points, int stride_floats, const int64_t *pt_off,
                                int n_clouds, const int32_t *map_off, const uint32_t *map_frame, const double *map_pose, int n_maps,
                                const int32_t *src_cloud, const int32_t *tgt_map, const double *init_pose, int n_pairs, int device_ptrs) {
  sgtd_voxel_register_options o;
  CHK(vreg_check(e, "sgtd_register_stored_voxels", opt, &o, points, stride_floats, pt_off, n_clouds, map_off, map_frame, map_pose, n_maps, src_cloud, tgt_map,
                 init_pose, n_pairs, [&](int j, int64_t *np) -> int {
                   const sgtd_engine *c = home_engine(e);
                   if (map_frame[j] >= c->st_slot_of.size() || c->st_slot_of[map_frame[j]] == SGTD_STORE_NONE) {
                     e->err = "sgtd_register_stored_voxels: frame " + std::to_string(map_frame[j]) + " has no stored cloud (sgtd_set_frame_clouds)";
                     return SGTD_ERR_INVALID;
                   }
                   *np = c->st.slots[(size_t)c->st_slot_of[map_frame[j]]].count;
                   return SGTD_OK;
                 }));
  CHK(stored_settings(e, "sgtd_register_stored_voxels", o.k_neighbors, o.plane_eps));
  const int64_t total = pt_off[n_clouds];
  const int n_members = n_maps ? map_off[n_maps] : 0;
  StageRun<int> run(e, &sgtd_engine::svox);
  run.c->sv_local = false;
  run.on_device([&](sgtd_engine *c) -> int {
    CHK(store_room(c, total, n_clouds));      // (a rebuild renumbers the slots: the members are looked up behind it)
    std::vector<int32_t> slot((size_t)n_members);
    for (int j = 0; j < n_members; j++) slot[(size_t)j] = c->st_slot_of[map_frame[j]];
    return stored_voxels_run(c, o, points, stride_floats, pt_off, n_clouds, device_ptrs, map_off, slot.data(), map_pose, n_maps, src_cloud, tgt_map,
                             init_pose, n_pairs);
  });
  return run.end(n_pairs);
}

int sgtd_register_stored_local_loops(sgtd_handle e, const sgtd_voxel_register_options *opt, const float *points, int stride_floats, const int64_t *pt_off,
                                     int max_per_query, int start, double radius, int max_members, int device_ptrs) {
  if (!e || !(std::isfinite(radius) && radius >= 0.0) || max_members < 0) return SGTD_ERR_INVALID;
  sgtd_voxel_register_options o;
  CHK(vreg_options(opt, &o));
  const char *call = "sgtd_register_stored_local_loops";
  CHK(loops_begin(e, call, "form the maps and use sgtd_register_stored_voxels", points, stride_floats, pt_off, max_per_query, start, o.k_neighbors,
                  o.plane_eps));
  const int nq = e->nq, cn = e->dc.cand_num, mpq = std::min(max_per_query, cn);
  const int64_t total = pt_off[nq];
  const size_t upper = (size_t)nq * mpq;
  int n = 0;
  StageRun<int> run(e, &sgtd_engine::svox);
  e->sv_local = true;
  e->sv_rows.clear(); e->sv_map_frame.clear(); e->sv_mem_off.assign(1, 0);
  run.on_device([&](sgtd_engine *c) -> int {
    const size_t n_ids = std::min(c->st_slot_of.size(), c->has_pose.size());
    CHK(store_room(c, total, nq));      // (a rebuild renumbers the slots: the table is made behind it)
    if (upper == 0 || c->st_frames == 0 || n_ids == 0)      // (no row can form: a run without a pair and without a map)
      return stored_voxels_run(c, o, points, stride_floats, pt_off, nq, device_ptrs, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0);
    CHK(store_table(c));
    CHK(cons_upload_store(c, c));       // (the pose store's device copy is the consistency and consensus stages')
    // one buffer: the per-id streams, the rows, the per-map records (a map per row at the most, and per id)
    const size_t max_maps = std::min(upper, n_ids);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t was = at; at += relax_up(bytes); return was; };
    const size_t o_elig = take(n_ids), o_trans = take(3 * n_ids * sizeof(double)), o_flag = take((n_ids + 1) * sizeof(u32)),
                 o_mapof = take((n_ids + 1) * sizeof(u32)), o_count = take(((size_t)nq + 1) * sizeof(u32)), o_first = take(((size_t)nq + 1) * sizeof(u32)),
                 o_rows = take(upper * sizeof(int4)), o_init = take(upper * 12 * sizeof(double)), o_mframe = take(max_maps * sizeof(u32)),
                 o_mcount = take(max_maps * sizeof(int)), o_mpts = take(max_maps * sizeof(long long)), o_mcut = take(max_maps * sizeof(int)),
                 o_thr = take(max_maps * sizeof(u64)), o_thrid = take(max_maps * sizeof(u32)), o_moff = take((max_maps + 1) * sizeof(int));
    CHK(ensure(c, c->sv_form, at));
    char *fb = c->sv_form.as<char>();
    c->sv_init_off = o_init;
    StoredLocalParams P;
    std::memset(&P, 0, sizeof(P));
    P.score = c->v_score.as<double>(); P.n_cand = c->n_cand.as<int>(); P.cand_frame = c->cand_frame.as<int>();
    P.pose = start_pose(c, start);
    P.cand_num = cn; P.nq = nq; P.max_per_query = mpq;
    P.slot_of = c->st_table.as<int>(); P.pose_store = c->ck_store.as<float>(); P.has_pose = c->ck_has.as<unsigned char>();
    P.arena_off = c->st.off.as<long long>(); P.n_ids = (u32)n_ids;
    P.elig = reinterpret_cast<unsigned char *>(fb + o_elig); P.trans = reinterpret_cast<double *>(fb + o_trans);
    P.count = reinterpret_cast<u32 *>(fb + o_count); P.first = reinterpret_cast<const u32 *>(fb + o_first);
    P.rows = reinterpret_cast<int4 *>(fb + o_rows); P.init = reinterpret_cast<double *>(fb + o_init);
    P.flag = reinterpret_cast<u32 *>(fb + o_flag); P.map_of = reinterpret_cast<const u32 *>(fb + o_mapof);
    P.map_frame = reinterpret_cast<u32 *>(fb + o_mframe);
    P.rr = radius * radius; P.max_members = max_members;
    P.mem_count = reinterpret_cast<int *>(fb + o_mcount); P.mem_pts = reinterpret_cast<long long *>(fb + o_mpts);
    P.mem_cut = reinterpret_cast<int *>(fb + o_mcut); P.thr_d2 = reinterpret_cast<u64 *>(fb + o_thr); P.thr_id = reinterpret_cast<u32 *>(fb + o_thrid);
    P.mem_off = reinterpret_cast<const int *>(fb + o_moff);
    hipStream_t s = c->stream;
    const int id_grid = grid_for((long long)n_ids + 1, SGTD_SL_THREADS), q_grid = grid_for(nq, SGTD_SL_THREADS / 64);
    sl_eligible_kernel<<<id_grid, SGTD_SL_THREADS, 0, s>>>(P);
    HIPCHK(hipMemsetAsync(P.count, 0, ((size_t)nq + 1) * sizeof(u32), s));
    sl_rows_kernel<<<q_grid, SGTD_SL_THREADS, 0, s>>>(P, 0);
    HIPCHK(hipGetLastError());
    CHK(device_scan(c, P.count, reinterpret_cast<u32 *>(fb + o_first), (long long)nq + 1));
    CHK(device_scan(c, P.flag, reinterpret_cast<u32 *>(fb + o_mapof), (long long)n_ids + 1));
    sl_rows_kernel<<<q_grid, SGTD_SL_THREADS, 0, s>>>(P, 1);
    sl_map_frames_kernel<<<id_grid, SGTD_SL_THREADS, 0, s>>>(P);
    sl_members_kernel<<<(unsigned)max_maps, SGTD_SL_THREADS, 0, s>>>(P, 0);
    HIPCHK(hipGetLastError());
    // the one read-back: the rows, the maps' frames, the member counts and points
    u32 found = 0, n_maps = 0;
    std::vector<int32_t> rows(upper * 4);
    std::vector<u32> map_frame(max_maps);
    std::vector<int> mem_count(max_maps);
    std::vector<long long> mem_pts(max_maps);
    CHK(d2h(c, &found, P.first + nq, sizeof(u32)));
    CHK(d2h(c, &n_maps, P.map_of + n_ids, sizeof(u32)));
    CHK(d2h(c, rows.data(), P.rows, upper * sizeof(int4)));
    CHK(d2h(c, map_frame.data(), P.map_frame, max_maps * sizeof(u32)));
    CHK(d2h(c, mem_count.data(), P.mem_count, max_maps * sizeof(int)));
    CHK(d2h(c, mem_pts.data(), P.mem_pts, max_maps * sizeof(long long)));
    CHK(xfer_sync(c));
    if (found == 0)
      return stored_voxels_run(c, o, points, stride_floats, pt_off, nq, device_ptrs, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0);
    int64_t total_src = 0, member_pts = 0, members = 0;
    for (u32 k = 0; k < found; k++) total_src += pt_off[rows[(size_t)k * 4] + 1] - pt_off[rows[(size_t)k * 4]];
    for (u32 m = 0; m < n_maps; m++) { member_pts += mem_pts[m]; members += mem_count[m]; }
    if (found > SGTD_REG_MAX_PAIRS || n_maps > SGTD_VREG_MAX_MAPS || member_pts > SGTD_VREG_MAX_MEMBER_POINTS || members > SGTD_VREG_MAX_MEMBER_POINTS ||
        total_src * o.neighbor_mode > SGTD_VREG_MAX_CORR) {
      c->err = std::string(call) + ": the rows and maps formed pass " + std::to_string(SGTD_REG_MAX_PAIRS) + " pairs, " + std::to_string(SGTD_VREG_MAX_MAPS) +
               " maps, " + std::to_string(SGTD_VREG_MAX_MEMBER_POINTS) + " members or member points, or " + std::to_string(SGTD_VREG_MAX_CORR) +
               " source points over the pairs times neighbor_mode";
      return SGTD_ERR_UNSUPPORTED;
    }
    n = (int)found;
    std::vector<int32_t> src, tgt, map_off((size_t)n_maps + 1, 0);
    for (int k = 0; k < n; k++) {
      const int32_t *r = rows.data() + (size_t)k * 4;
      src.push_back(r[0]); tgt.push_back(r[3]);
      c->sv_rows.insert(c->sv_rows.end(), r, r + 4);
    }
    for (u32 m = 0; m < n_maps; m++) map_off[(size_t)m + 1] = map_off[m] + mem_count[m];
    c->sv_map_frame.assign(map_frame.begin(), map_frame.begin() + n_maps);
    c->sv_mem_off.assign(map_off.begin(), map_off.end());
    // the members: ids, slots, maps, sizes and their scan, poses
    const size_t nm = (size_t)members;
    at = 0;
    const size_t o_member = take(nm * sizeof(int)), o_slot = take(nm * sizeof(int)), o_map = take(nm * sizeof(int)), o_size = take((nm + 1) * sizeof(u32)),
                 o_ptoff = take((nm + 1) * sizeof(u32)), o_pose = take(nm * 12 * sizeof(double));
    CHK(ensure(c, c->sv_members, at));
    char *mb = c->sv_members.as<char>();
    c->sv_member_off = o_member; c->sv_pose_off = o_pose;
    P.member = reinterpret_cast<int *>(mb + o_member); P.mem_slot = reinterpret_cast<int *>(mb + o_slot); P.mem_map = reinterpret_cast<int *>(mb + o_map);
    P.mem_size = reinterpret_cast<u32 *>(mb + o_size); P.mem_pose = reinterpret_cast<double *>(mb + o_pose);
    CHK(h2d(c, fb + o_moff, map_off.data(), map_off.size() * sizeof(int)));
    HIPCHK(hipMemsetAsync(P.mem_size + nm, 0, sizeof(u32), s));
    sl_members_kernel<<<n_maps, SGTD_SL_THREADS, 0, s>>>(P, 1);
    HIPCHK(hipGetLastError());
    CHK(device_scan(c, P.mem_size, reinterpret_cast<u32 *>(mb + o_ptoff), (long long)nm + 1));
    sl_poses_kernel<<<grid_for((long long)nm, SGTD_SL_THREADS), SGTD_SL_THREADS, 0, s>>>(P, (int)nm);
    HIPCHK(hipGetLastError());
    const StoredMembers formed{P.mem_slot, P.mem_map, reinterpret_cast<const int *>(mb + o_ptoff), P.mem_pose, member_pts, P.init};
    return stored_voxels_run(c, o, points, stride_floats, pt_off, nq, device_ptrs, map_off.data(), nullptr, nullptr, (int)n_maps, src.data(), tgt.data(),
                             nullptr, n, &formed);
  });
  return run.end(n);
}

int sgtd_result_stored_local_pairs(sgtd_handle e, int32_t *query, int32_t *cand, int32_t *frame, int32_t *tgt_map, double *init, int64_t capacity,
                                   int64_t *n) {
  if (!e || capacity < 0) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::svox, kNoStoredVoxel, &c));
  if (!c->sv_local) { e->err = "no rows: sgtd_register_stored_local_loops has not run"; return SGTD_ERR_STATE; }
  const int64_t need = c->svox.n;
  if (n) *n = need;
  const size_t m = (size_t)std::min(need, capacity);
  for (size_t k = 0; k < m; k++) {
    if (query) query[k] = c->sv_rows[k * 4];
    if (cand) cand[k] = c->sv_rows[k * 4 + 1];
    if (frame) frame[k] = c->sv_rows[k * 4 + 2];
    if (tgt_map) tgt_map[k] = c->sv_rows[k * 4 + 3];
  }
  if (m) {
    CopyOut out(e, c);
    out.get(init, c->sv_form.as<char>() + c->sv_init_off, m * 12 * sizeof(double));
    CHK(out.finish());
  }
  return need > capacity && (query || cand || frame || tgt_map || init) ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int sgtd_result_stored_local_maps(sgtd_handle e, uint32_t *map_frame, int64_t *mem_off, uint32_t *member, double *member_pose, int64_t cap_maps,
                                  int64_t cap_members, int64_t *n_maps, int64_t *n_members) {
  if (!e || cap_maps < 0 || cap_members < 0) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::svox, kNoStoredVoxel, &c));
  if (!c->sv_local) { e->err = "no maps: sgtd_register_stored_local_loops has not run"; return SGTD_ERR_STATE; }
  const int64_t maps = (int64_t)c->sv_map_frame.size(), members = c->sv_mem_off.back();
  if (n_maps) *n_maps = maps;
  if (n_members) *n_members = members;
  const size_t m = (size_t)std::min(maps, cap_maps), k = (size_t)std::min(members, cap_members);
  if (map_frame) std::copy(c->sv_map_frame.begin(), c->sv_map_frame.begin() + m, map_frame);
  if (mem_off && (maps <= cap_maps)) std::copy(c->sv_mem_off.begin(), c->sv_mem_off.end(), mem_off);
  else if (mem_off) std::copy(c->sv_mem_off.begin(), c->sv_mem_off.begin() + m, mem_off);
  if (k) {
    CopyOut out(e, c);
    out.get(member, c->sv_members.as<char>() + c->sv_member_off, k * sizeof(int));
    out.get(member_pose, c->sv_members.as<char>() + c->sv_pose_off, k * 12 * sizeof(double));
    CHK(out.finish());
  }
  const bool short_maps = maps > cap_maps && (map_frame || mem_off), short_members = members > cap_members && (member || member_pose);
  return short_maps || short_members ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int sgtd_result_stored_voxel_registered(sgtd_handle e, double *pose, double *fitness, double *cost, int32_t *n_matched, int32_t *n_corr, int32_t *iterations,
                                        int32_t *status) {
  return vreg_rows_out(e, &sgtd_engine::svox, kNoStoredVoxel, pose, fitness, cost, n_matched, n_corr, iterations, status);
}

int sgtd_result_stored_voxel_map(sgtd_handle e, int map, int32_t *coord, int32_t *n_points, double *mean, double *cov, int64_t capacity, int64_t *n) {
  return vreg_map_out(e, &sgtd_engine::svox, kNoStoredVoxel, map, coord, n_points, mean, cov, capacity, n);
}

int sgtd_result_stored_voxel_matches(sgtd_handle e, int pair, int32_t *voxel, int64_t capacity, int64_t *n) {
  return vreg_matches_out(e, &sgtd_engine::svox, kNoStoredVoxel, pair, voxel, capacity, n);
}

int sgtd_stored_voxel_register_stage_ms(sgtd_handle e, float *ms_cov, float *ms_map, float *ms_corr, float *ms_rest, float *ms_total) {
  return vreg_ms_out(e, &sgtd_engine::svox, kNoStoredVoxel, ms_cov, ms_map, ms_corr, ms_rest, ms_total);
}

}  // extern "C"

// ---- sgtd_scan_keypoints: labelled scans to keypoints on the device (scan_kernels.hip.h) ----
namespace {
// the ring envelope: some n <= SGTD_SCAN_MAX_CELLS has every increment start_r - s * delta_r > 0 for s <= n and the
// increments sum to at least max_range - min_range
bool scan_rings_fit(const sgtd_scan_config &c) {
  double sum = 0.0;
  for (int s = 1; s <= SGTD_SCAN_MAX_CELLS; s++) {
    const double inc = c.start_r - (double)s * c.delta_r;
    if (!(inc > 0.0)) return false;
    sum += inc;
    if (sum >= c.max_range - c.min_range) return true;
  }
  return false;
}

// the pipeline from "points on the device" onward: d_pts / d_lab are device arrays (nullptr: scan_run's own staging
// buffers sk.pts / sk.lab, which it has filled), pt_off is the host's.  sgtd_local_map_keypoints calls it once per pass.
int scan_device(sgtd_engine *e, const ScanCfgDev &C, const float *d_pts, int stride, const u32 *d_lab, const int64_t *pt_off, int S);

int scan_run(sgtd_engine *e, const ScanCfgDev &C, const float *points, int stride, const uint32_t *labels, const int64_t *pt_off, int S,
             int device_ptrs) {
  const long long P = pt_off[S];
  if (device_ptrs || S == 0 || P == 0) return scan_device(e, C, points, stride, labels, pt_off, S);
  const size_t np = (size_t)P;
  CHK(need(e, e->sk.pts, np * stride));
  CHK(need(e, e->sk.lab, np));
  CHK(h2d(e, e->sk.pts.p(), points, np * stride * sizeof(float)));
  CHK(h2d(e, e->sk.lab.p(), labels, np * sizeof(u32)));
  return scan_device(e, C, nullptr, stride, nullptr, pt_off, S);
}

int scan_device(sgtd_engine *e, const ScanCfgDev &C, const float *d_pts, int stride, const u32 *d_lab, const int64_t *pt_off, int S) {
  const long long P = pt_off[S];
  const int n_sc = S * 32;
  sgtd_engine::ScanBufs &B = e->sk;
  const size_t np = (size_t)P;
  e->sk_off.assign(pt_off, pt_off + S + 1);
  e->sk_kp_off.assign((size_t)S + 1, 0);
  e->sk_points = P; e->sk_kept = 0;
  CHK(need(e, B.grid, (size_t)std::max(n_sc, 1) * 4));
  CHK(need(e, B.range, (size_t)std::max(n_sc, 1) * 4));
  CHK(need_each(e, 0, B.xyz, B.label));      // (a run without keypoints still has results to point to)
  if (S == 0 || P == 0) {
    if (n_sc > 0) {
      HIPCHK(hipMemsetAsync(B.grid.p(), 0, (size_t)n_sc * 4 * sizeof(int), e->stream));
      HIPCHK(hipMemsetAsync(B.range.p(), 0, (size_t)n_sc * 4 * sizeof(double), e->stream));
    }
    return xfer_sync(e);
  }
  if (!d_pts) d_pts = B.pts.p();
  if (!d_lab) d_lab = B.lab.p();
  CHK(need(e, B.off, (size_t)S + 1));
  CHK(h2d(e, B.off.p(), pt_off, ((size_t)S + 1) * sizeof(long long)));
  CHK(need_each(e, np, B.sc, B.r, B.pitch, B.azi));
  CHK(need(e, B.mm, (size_t)n_sc * 4));
  CHK(need(e, B.vote, (size_t)n_sc));
  CHK(need(e, B.bounds, (size_t)n_sc * SGTD_SCAN_CELLS));
  CHK(need_runs(e, B.runs, np));
  CHK(need(e, B.nbr, np * SGTD_SCAN_NBR));
  CHK(need_each(e, np, B.nbr_cnt, B.parent));
  constexpr int kMaxRounds = 4096, kGroup = 8;
  CHK(need(e, B.changed, kMaxRounds));
  CHK(need_each(e, np, B.ccount, B.cmin, B.ckey_a, B.ckey_b, B.cval_a, B.cval_b));
  CHK(need(e, B.kp_off, (size_t)S + 1));
  CHK(need_each(e, np, B.cl_of_root, B.pkey_a, B.pkey_b, B.pval_a, B.pval_b, B.cluster));
  const hipStream_t st = e->stream;
  const int gp = grid_for(P, 256);
  const long long *d_off = B.off.p();
  int *grid = B.grid.p();
  double *range = B.range.p(), *bounds = B.bounds.p();

  // per point, per (scan, class), keys
  scan_init_kernel<<<grid_for(n_sc, 256), 256, 0, st>>>(B.mm.p(), B.vote.p(), n_sc);
  ScanPointParams PP;
  PP.pts = d_pts; PP.stride = stride; PP.labels = d_lab; PP.pt_off = d_off; PP.n = P;
  PP.sc_of = B.sc.p(); PP.r = B.r.p(); PP.pitch = B.pitch.p();
  PP.azimuth = B.azi.p(); PP.mm = B.mm.p(); PP.vote = B.vote.p();
  scan_point_kernel<<<grid_for(P, SGTD_SCAN_TILE), 256, 0, st>>>(PP, C);
  scan_rings_kernel<<<grid_for(n_sc, 64), 64, 0, st>>>(PP.mm, PP.vote, n_sc, C, grid, range, bounds);
  scan_keys_kernel<<<gp, 256, 0, st>>>(PP.sc_of, d_lab, PP.r, PP.pitch, PP.azimuth, grid, range, bounds, C, P, B.runs.key_a.p(), B.runs.val_a.p());
  HIPCHK(hipGetLastError());

  // voxels, links, components
  u64 *kin = nullptr;
  u32 *vin = nullptr;
  CHK(sorted_runs(e, B.runs, P, 38 + key_bits((u64)S), false, (u64)S << 38, &kin, &vin));
  u32 *flags = B.runs.flags.p(), *excl = B.runs.excl.p(), *counts = B.runs.counts.p();
  const u32 *n_vox_p = excl + P;
  u64 *vkey = B.runs.vkey.p();
  u32 *vstart = B.runs.vstart.p(), *nbr = B.nbr.p(), *nbr_cnt = B.nbr_cnt.p();
  u32 *parent = B.parent.p(), *changed = B.changed.p();
  u32 *ccount = B.ccount.p(), *cmin = B.cmin.p();
  HIPCHK(hipMemsetAsync(changed, 0, kMaxRounds * sizeof(u32), st));
  HIPCHK(hipMemsetAsync(ccount, 0, np * sizeof(u32), st));
  HIPCHK(hipMemsetAsync(cmin, 0xFF, np * sizeof(u32), st));
  HIPCHK(hipMemsetAsync(B.cl_of_root.p(), 0xFF, np * sizeof(u32), st));
  scan_links_kernel<<<gp, 256, 0, st>>>(vkey, n_vox_p, grid, nbr, nbr_cnt, parent);
  HIPCHK(hipGetLastError());
  bool settled = false;
  std::vector<u32> ch(kGroup);
  for (int r0 = 0; r0 < kMaxRounds && !settled; r0 += kGroup) {
    for (int r = r0; r < r0 + kGroup; r++) {
      scan_hook_kernel<<<gp, 256, 0, st>>>(n_vox_p, nbr, nbr_cnt, parent, changed, r);
      scan_jump_kernel<<<gp, 256, 0, st>>>(n_vox_p, parent, changed, r);
    }
    HIPCHK(hipGetLastError());
    CHK(d2h(e, ch.data(), changed + r0, kGroup * sizeof(u32)));
    CHK(xfer_sync(e));
    for (int r = 0; r < kGroup; r++) settled = settled || ch[r] == 0;
  }
  if (!settled) { e->err = "sgtd_scan_keypoints: the components did not settle in " + std::to_string(kMaxRounds) + " rounds"; return SGTD_ERR_UNSUPPORTED; }
  scan_component_kernel<<<gp, 256, 0, st>>>(n_vox_p, parent, vstart, vin, ccount, cmin);

  // kept clusters in keypoint order, the offsets
  u64 *ckin = B.ckey_a.p(), *ckout = B.ckey_b.p();
  u32 *cvin = B.cval_a.p(), *cvout = B.cval_b.p();
  scan_cluster_keys_kernel<<<gp, 256, 0, st>>>(n_vox_p, vkey, parent, ccount, cmin, grid, C, ckin, cvin);
  HIPCHK(hipGetLastError());
  CHK(radix_sort_pairs<u64>(e, ckin, ckout, cvin, cvout, P, 37 + key_bits((u64)S), false, n_vox_p));
  long long *d_kp_off = B.kp_off.p();
  scan_offsets_kernel<<<grid_for(S + 1, 256), 256, 0, st>>>(ckin, n_vox_p, S, d_kp_off);
  HIPCHK(hipGetLastError());
  CHK(d2h(e, e->sk_kp_off.data(), d_kp_off, ((size_t)S + 1) * sizeof(long long)));
  CHK(xfer_sync(e));
  const long long K = e->sk_kp_off[(size_t)S];
  e->sk_kept = K;

  // the points by keypoint, the centres
  const size_t nk = (size_t)std::max<long long>(K, 1);
  CHK(need_each(e, nk, B.kcount, B.cstart));
  CHK(need(e, B.xyz, nk * 3));
  CHK(need_each(e, nk, B.label, B.npoints));
  u32 *kcount = B.kcount.p(), *cstart = B.cstart.p();
  u32 *cl_of_root = B.cl_of_root.p();
  if (K > 0) scan_cluster_ids_kernel<<<grid_for(K, 256), 256, 0, st>>>(ckin, cvin, (u32)K, ccount, C, cl_of_root, kcount, B.npoints.p(), B.label.p());
  u32 *pkin = B.pkey_a.p(), *pkout = B.pkey_b.p();
  u32 *pvin = B.pval_a.p(), *pvout = B.pval_b.p();
  scan_point_clusters_kernel<<<gp, 256, 0, st>>>(kin, vin, flags, excl, counts, parent, cl_of_root, d_kp_off, P, (u32)K, pkin, pvin, B.cluster.p());
  HIPCHK(hipGetLastError());
  if (K > 0) {
    CHK(radix_sort_pairs<u32>(e, pkin, pkout, pvin, pvout, P, key_bits((u64)K), false));
    CHK(device_scan(e, kcount, cstart, K));
    float *xyz = B.xyz.p();
    scan_sum_wave_kernel<<<grid_for(K, 4), 256, 0, st>>>(d_pts, stride, pvin, cstart, kcount, (u32)K, xyz);
    scan_sum_block_kernel<<<(unsigned)K, 256, 0, st>>>(d_pts, stride, pvin, cstart, kcount, xyz);
    HIPCHK(hipGetLastError());
  }
  // (the caller's arrays are read for the last time by the sums: the call returns when they are done)
  return xfer_sync(e);
}

// the first m keypoints a stage left on its home engine c, to those of the caller's arrays that are given
int keypoints_out(sgtd_engine *e, sgtd_engine *c, const DevArr<float> &xyz_dev, const DevArr<u32> &label_dev, const DevArr<int> &n_points_dev, size_t m,
                  float *xyz, uint32_t *label, int32_t *n_points) {
  CopyOut out(e, c);
  out.get(xyz, xyz_dev.p(), m * 3 * sizeof(float));
  out.get(label, label_dev.p(), m * sizeof(u32));
  out.get(n_points, n_points_dev.p(), m * sizeof(int));
  return out.finish();
}

const char kNoScan[] = "no scan keypoints: sgtd_scan_keypoints has not run";
const char kNoLocalMap[] = "no local-map keypoints: sgtd_local_map_keypoints has not run";

ScanCfgDev scan_cfg_dev(const sgtd_scan_config &c, int n_scans) {
  ScanCfgDev C;
  for (int s = 0; s < 32; s++) { C.node_label[s] = c.node_label[s]; C.min_seg[s] = c.min_seg[s]; }
  C.min_inst = c.min_instance_points; C.n_scans = n_scans;
  C.start_r = c.start_r; C.delta_r = c.delta_r; C.delta_p = c.delta_p; C.delta_a = c.delta_a; C.min_range = c.min_range; C.max_range = c.max_range;
  return C;
}

// ---- sgtd_local_map_keypoints (local_map_kernels.hip.h) ----

int local_map_run(sgtd_engine *e, const sgtd_scan_config &cfg, const sgtd_local_map_options &opt, const float *points, int stride,
                  const uint32_t *labels, const int64_t *pt_off, const float *pose12, int S, const int32_t *anchors, int A, int device_ptrs) {
  sgtd_engine::LocalMapBufs &B = e->lm;
  const hipStream_t st = e->stream;
  const bool timed = e->timing;
  LapClock &clock = e->lm_clock;      // (ms: members, gather, scan passes; the events bracket the work they measure)
  CHK(clock.start(e, timed));
  e->lm_kp_off.assign((size_t)A + 1, 0);
  e->lm_mem_off.assign((size_t)A + 1, 0);
  e->lm_merged.assign((size_t)A, 0);
  e->lm_kept = 0; e->lm_passes = 0;
  CHK(need_each(e, 0, B.xyz, B.label, B.npoints, B.member));      // (a call without anchors or keypoints still has results to point to)
  if (A == 0) return SGTD_OK;

  // members: counts and merged sizes, the host's plan, then the lists
  std::vector<int32_t> anch((size_t)A);
  for (int a = 0; a < A; a++) anch[(size_t)a] = anchors ? anchors[a] : a;
  CHK(need(e, B.pose, (size_t)S * 12));
  CHK(need(e, B.off, (size_t)S + 1));
  CHK(need_each(e, (size_t)A, B.anch, B.count, B.merged));
  CHK(need(e, B.mem_off, (size_t)A + 1));
  CHK(h2d(e, B.pose.p(), pose12, (size_t)S * 12 * sizeof(float)));
  CHK(h2d(e, B.off.p(), pt_off, ((size_t)S + 1) * sizeof(long long)));
  CHK(h2d(e, B.anch.p(), anch.data(), (size_t)A * sizeof(int)));
  const float *d_pose = B.pose.p();
  const long long *d_off = B.off.p();
  const int *d_anch = B.anch.p();
  const double rr = opt.radius * opt.radius;
  if (timed) HIPCHK(hipEventRecord(clock.ev[0], st));
  lm_members_kernel<<<A, SGTD_LM_THREADS, 0, st>>>(d_pose, d_off, S, d_anch, rr, opt.max_members, nullptr, nullptr, B.count.p(), B.merged.p());
  HIPCHK(hipGetLastError());
  if (timed) HIPCHK(hipEventRecord(clock.ev[1], st));
  std::vector<int32_t> count((size_t)A);
  CHK(d2h(e, count.data(), B.count.p(), (size_t)A * sizeof(int)));
  CHK(d2h(e, e->lm_merged.data(), B.merged.p(), (size_t)A * sizeof(long long)));
  CHK(xfer_sync(e));
  if (timed) CHK(clock.span(e, 0, 1, 0, true));
  const int64_t cap = opt.max_pass_points > 0 ? opt.max_pass_points : (int64_t)1 << 26;
  for (int a = 0; a < A; a++) {
    e->lm_mem_off[(size_t)a + 1] = e->lm_mem_off[(size_t)a] + count[(size_t)a];
    if (e->lm_merged[(size_t)a] > cap) {
      e->err = "sgtd_local_map_keypoints: the merged cloud of anchor " + std::to_string(a) + " (scan " + std::to_string(anch[(size_t)a]) + ") holds " +
               std::to_string(e->lm_merged[(size_t)a]) + " points, more than max_pass_points = " + std::to_string(cap) +
               " (lower radius or max_members, or raise max_pass_points)";
      return SGTD_ERR_UNSUPPORTED;
    }
  }
  const int64_t M = e->lm_mem_off[(size_t)A];
  CHK(need(e, B.member, (size_t)M));
  CHK(h2d(e, B.mem_off.p(), e->lm_mem_off.data(), ((size_t)A + 1) * sizeof(long long)));
  const long long *d_mem_off = B.mem_off.p();
  int *d_member = B.member.p();
  if (timed) HIPCHK(hipEventRecord(clock.ev[0], st));
  lm_members_kernel<<<A, SGTD_LM_THREADS, 0, st>>>(d_pose, d_off, S, d_anch, rr, opt.max_members, d_mem_off, d_member, B.count.p(), B.merged.p());
  HIPCHK(hipGetLastError());
  if (timed) {
    HIPCHK(hipEventRecord(clock.ev[1], st));
    CHK(clock.span(e, 0, 1, 0, true));
  }

  // the scans on the device (the scan pipeline's staging buffers: it reads the merged cloud, not these)
  const float *d_pts = points;
  const u32 *d_lab = labels;
  const size_t np = (size_t)pt_off[S];
  e->sk_n = -1;
  if (!device_ptrs && np) {
    CHK(ensure(e, e->sk.pts.buf, np * stride * sizeof(float)));      // (as they always were here: to the byte, no floor of 16)
    CHK(ensure(e, e->sk.lab.buf, np * sizeof(u32)));
    CHK(h2d(e, e->sk.pts.p(), points, np * stride * sizeof(float)));
    CHK(h2d(e, e->sk.lab.p(), labels, np * sizeof(u32)));
    d_pts = e->sk.pts.p();
    d_lab = e->sk.lab.p();
  }
  const bool vec = stride == 4 && ((uintptr_t)d_pts & 15) == 0;

  // passes of consecutive anchors
  std::vector<int64_t> pass_off;
  for (int a0 = 0; a0 < A;) {
    int a1 = a0;
    int64_t Pp = 0;
    while (a1 < A && a1 - a0 < SGTD_SCAN_MAX_SCANS && Pp + e->lm_merged[(size_t)a1] <= cap) Pp += e->lm_merged[(size_t)a1++];
    const int na = a1 - a0;
    const int64_t n_seg64 = e->lm_mem_off[(size_t)a1] - e->lm_mem_off[(size_t)a0];
    if (n_seg64 > (int64_t)1 << 30) { e->err = "sgtd_local_map_keypoints: more than 2^30 members in one pass"; return SGTD_ERR_UNSUPPORTED; }
    const int n_seg = (int)n_seg64;
    pass_off.assign((size_t)na + 1, 0);
    for (int a = 0; a < na; a++) pass_off[(size_t)a + 1] = pass_off[(size_t)a] + e->lm_merged[(size_t)(a0 + a)];
    CHK(need(e, B.seg, (size_t)n_seg));
    CHK(need_each(e, (size_t)n_seg + 1, B.cnt, B.start));
    CHK(need(e, B.mpts, (size_t)Pp * 3));
    CHK(need(e, B.mlab, (size_t)Pp));
    LmSeg *seg = B.seg.p();
    u32 *cnt = B.cnt.p(), *start = B.start.p();
    float *m_pts = B.mpts.p();
    u32 *m_lab = B.mlab.p();
    if (timed) HIPCHK(hipEventRecord(clock.ev[0], st));
    if (Pp > 0) {
      lm_segments_kernel<<<grid_for((long long)n_seg + 1, 256), 256, 0, st>>>(d_pose, d_off, d_anch, d_mem_off, d_member, a0, na, n_seg, seg, cnt);
      HIPCHK(hipGetLastError());
      CHK(device_scan(e, cnt, start, (long long)n_seg + 1));
      const int tiles = grid_for(Pp, SGTD_SCAN_TILE);
      if (vec) lm_gather_kernel<4, true><<<tiles, SGTD_LM_THREADS, 0, st>>>(d_pts, d_lab, seg, start, n_seg, (u32)Pp, m_pts, m_lab);
      else if (stride == 4) lm_gather_kernel<4, false><<<tiles, SGTD_LM_THREADS, 0, st>>>(d_pts, d_lab, seg, start, n_seg, (u32)Pp, m_pts, m_lab);
      else lm_gather_kernel<3, false><<<tiles, SGTD_LM_THREADS, 0, st>>>(d_pts, d_lab, seg, start, n_seg, (u32)Pp, m_pts, m_lab);
      HIPCHK(hipGetLastError());
    }
    if (timed) HIPCHK(hipEventRecord(clock.ev[1], st));
    const ScanCfgDev C = scan_cfg_dev(cfg, na);
    CHK(scan_device(e, C, m_pts, 3, m_lab, pass_off.data(), na));
    if (timed) {
      HIPCHK(hipEventRecord(clock.ev[2], st));
      CHK(clock.span(e, 0, 1, 1, true));
      CHK(clock.span(e, 1, 2, 2, true));
    }
    // the pass's keypoints behind those of the passes before it
    const int64_t K = e->sk_kept, K0 = e->lm_kept;
    for (int a = 0; a <= na; a++) e->lm_kp_off[(size_t)(a0 + a)] = K0 + e->sk_kp_off[(size_t)a];
    if (K > 0) {
      CHK(need(e, B.xyz, (size_t)(K0 + K) * 3, true));
      CHK(need(e, B.label, (size_t)(K0 + K), true));
      CHK(need(e, B.npoints, (size_t)(K0 + K), true));
      HIPCHK(hipMemcpyAsync(B.xyz.p() + (size_t)K0 * 3, e->sk.xyz.p(), (size_t)K * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpyAsync(B.label.p() + (size_t)K0, e->sk.label.p(), (size_t)K * sizeof(u32), hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpyAsync(B.npoints.p() + (size_t)K0, e->sk.npoints.p(), (size_t)K * sizeof(int), hipMemcpyDeviceToDevice, st));
    }
    e->lm_kept = K0 + K;
    e->lm_passes++;
    a0 = a1;
  }
  // (the caller's arrays and the scan buffers are read for the last time by the copies: the call returns when they are done)
  return xfer_sync(e);
}

}  // namespace

extern "C" {

void sgtd_scan_tiles(int *point_tile) {
  if (point_tile) *point_tile = SGTD_SCAN_TILE;
}

void sgtd_default_scan_config(sgtd_scan_config *cfg) {
  if (!cfg) return;
  std::memset(cfg, 0, sizeof(*cfg));
  for (int s = 0; s < SGTD_SCAN_MAX_CLASSES; s++) cfg->min_seg[s] = 300;
  for (int s = 10; s <= 18; s++) cfg->node_label[s] = s - 7;
  cfg->min_seg[15] = cfg->min_seg[17] = cfg->min_seg[18] = 5;
  cfg->min_instance_points = 20;
  cfg->start_r = 0.35; cfg->delta_r = 0.0004; cfg->delta_p = 1.2; cfg->delta_a = 1.2;
  cfg->min_range = 0.5; cfg->max_range = 120.0;
}

int sgtd_scan_config_check(const sgtd_scan_config *cfg, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  sgtd_scan_config c;
  sgtd_default_scan_config(&c);
  if (cfg) c = *cfg;
  auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
  *why = "a config value is not finite and positive, min_range >= max_range, or a label or count is negative";
  if (!pos(c.start_r) || !(std::isfinite(c.delta_r) && c.delta_r >= 0.0) || !pos(c.delta_p) || !pos(c.delta_a) || !pos(c.min_range) ||
      !pos(c.max_range) || c.min_range >= c.max_range || c.min_instance_points < 0)
    return SGTD_ERR_INVALID;
  for (int s = 0; s < SGTD_SCAN_MAX_CLASSES; s++)
    if (c.node_label[s] < 0 || c.min_seg[s] < 0) return SGTD_ERR_INVALID;
  *why = "delta_a gives more than 1024 azimuth cells";
  if (!(std::round(360.0 / c.delta_a) + 1.0 <= (double)SGTD_SCAN_MAX_CELLS)) return SGTD_ERR_UNSUPPORTED;
  *why = "delta_p gives more than 1024 pitch layers";
  if (!(180.0 / c.delta_p + 2.0 <= (double)SGTD_SCAN_MAX_CELLS)) return SGTD_ERR_UNSUPPORTED;
  *why = "start_r and delta_r do not cover the range gate with at most 1024 rings of positive width";
  if (!scan_rings_fit(c)) return SGTD_ERR_UNSUPPORTED;
  *why = "";
  return SGTD_OK;
}

int sgtd_scan_keypoints(sgtd_handle e, const sgtd_scan_config *cfg, const float *points, int stride_floats, const uint32_t *labels,
                        const int64_t *pt_off, int n_scans, int device_ptrs) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_scan_config c;
  sgtd_default_scan_config(&c);
  if (cfg) c = *cfg;
  const char *why = nullptr;
  const int cs = sgtd_scan_config_check(&c, &why);
  if (cs == SGTD_ERR_INVALID) return cs;
  if (!cloud_set_ok(pt_off, n_scans, stride_floats, points, true, labels)) return SGTD_ERR_INVALID;
  const int64_t P = pt_off[n_scans];
  if (n_scans > SGTD_SCAN_MAX_SCANS || P > SGTD_SCAN_MAX_POINTS) {
    e->err = "sgtd_scan_keypoints takes at most " + std::to_string(SGTD_SCAN_MAX_SCANS) + " scans and " + std::to_string(SGTD_SCAN_MAX_POINTS) +
             " points in one call";
    return SGTD_ERR_UNSUPPORTED;
  }
  if (cs != SGTD_OK) {
    e->err = std::string("sgtd_scan_keypoints: ") + why;
    return cs;
  }
  StageRun<int> run(e, &sgtd_engine::sk_n);
  run.on_device([&](sgtd_engine *k) { return scan_run(k, scan_cfg_dev(c, n_scans), points, stride_floats, labels, pt_off, n_scans, device_ptrs); });
  return run.end(n_scans);
}

int sgtd_result_scan_keypoints(sgtd_handle e, int64_t *kp_off, float *xyz, uint32_t *label, int32_t *n_points, int64_t capacity, int64_t *n_keypoints) {
  if (!e || capacity < 0) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::sk_n, kNoScan, &c));
  const int64_t K = c->sk_kept;
  if (n_keypoints) *n_keypoints = K;
  if (kp_off) std::memcpy(kp_off, c->sk_kp_off.data(), c->sk_kp_off.size() * sizeof(int64_t));
  CHK(keypoints_out(e, c, c->sk.xyz, c->sk.label, c->sk.npoints, (size_t)std::min(K, capacity), xyz, label, n_points));
  return K > capacity && (xyz || label || n_points) ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int sgtd_result_scan_point_clusters(sgtd_handle e, int scan, int32_t *cluster, int64_t capacity, int64_t *n) {
  if (!e || capacity < 0) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::sk_n, kNoScan, &c));
  if (scan < 0 || scan >= c->sk_n) return SGTD_ERR_INVALID;
  const int64_t first = c->sk_off[(size_t)scan], need = c->sk_off[(size_t)scan + 1] - first;
  if (n) *n = need;
  CopyOut out(e, c);
  out.get(cluster, c->sk.cluster.p() + first, (size_t)std::min(need, capacity) * sizeof(int));
  CHK(out.finish());
  return need > capacity && cluster ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int sgtd_result_scan_grids(sgtd_handle e, int scan, int32_t *grid, double *range) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::sk_n, kNoScan, &c));
  if (scan < 0 || scan >= c->sk_n) return SGTD_ERR_INVALID;
  CopyOut out(e, c);
  out.get(grid, c->sk.grid.p() + (size_t)scan * 128, 128 * sizeof(int));
  out.get(range, c->sk.range.p() + (size_t)scan * 128, 128 * sizeof(double));
  return out.finish();
}

int sgtd_scan_device_view(sgtd_handle e, const float **d_xyz, const uint32_t **d_label) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::sk_n, kNoScan, &c));
  if (d_xyz) *d_xyz = c->sk.xyz.p();
  if (d_label) *d_label = c->sk.label.p();
  return SGTD_OK;
}

void sgtd_default_local_map_options(sgtd_local_map_options *opt) {
  if (!opt) return;
  std::memset(opt, 0, sizeof(*opt));
  opt->radius = 15.0;
}

int sgtd_local_map_keypoints(sgtd_handle e, const sgtd_scan_config *cfg, const sgtd_local_map_options *opt, const float *points, int stride_floats,
                             const uint32_t *labels, const int64_t *pt_off, const float *pose12, int n_scans, const int32_t *anchors, int n_anchors,
                             int device_ptrs) {
  if (!e || n_anchors < 0) return SGTD_ERR_INVALID;
  sgtd_scan_config c;
  sgtd_default_scan_config(&c);
  if (cfg) c = *cfg;
  sgtd_local_map_options o;
  sgtd_default_local_map_options(&o);
  if (opt) o = *opt;
  const char *why = nullptr;
  const int cs = sgtd_scan_config_check(&c, &why);
  if (cs == SGTD_ERR_INVALID) return cs;
  if (!(std::isfinite(o.radius) && o.radius >= 0.0) || o.max_members < 0 || o.reserved != 0 || o.max_pass_points < 0 ||
      o.max_pass_points > SGTD_SCAN_MAX_POINTS)
    return SGTD_ERR_INVALID;
  if (!cloud_set_ok(pt_off, n_scans, stride_floats, points, true, labels)) return SGTD_ERR_INVALID;
  const int64_t P = pt_off[n_scans];
  if (n_scans > 0 && !pose12) return SGTD_ERR_INVALID;
  const int A = anchors ? n_anchors : n_scans;      // NULL: every scan, in order
  if (anchors)
    for (int a = 0; a < n_anchors; a++)
      if (anchors[a] < 0 || anchors[a] >= n_scans) return SGTD_ERR_INVALID;
  if (n_scans > SGTD_SCAN_MAX_SCANS || P > SGTD_SCAN_MAX_POINTS) {
    e->err = "sgtd_local_map_keypoints takes at most " + std::to_string(SGTD_SCAN_MAX_SCANS) + " scans and " + std::to_string(SGTD_SCAN_MAX_POINTS) +
             " points in one call";
    return SGTD_ERR_UNSUPPORTED;
  }
  if (cs != SGTD_OK) {
    e->err = std::string("sgtd_local_map_keypoints: ") + why;
    return cs;
  }
  StageRun<int> run(e, &sgtd_engine::lm_n);
  run.on_device([&](sgtd_engine *k) { return local_map_run(k, c, o, points, stride_floats, labels, pt_off, pose12, n_scans, anchors, A, device_ptrs); });
  return run.end(A);
}

int sgtd_result_local_map_keypoints(sgtd_handle e, int64_t *kp_off, float *xyz, uint32_t *label, int32_t *n_points, int64_t capacity,
                                    int64_t *n_keypoints) {
  if (!e || capacity < 0) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::lm_n, kNoLocalMap, &c));
  const int64_t K = c->lm_kept;
  if (n_keypoints) *n_keypoints = K;
  if (kp_off) std::memcpy(kp_off, c->lm_kp_off.data(), c->lm_kp_off.size() * sizeof(int64_t));
  CHK(keypoints_out(e, c, c->lm.xyz, c->lm.label, c->lm.npoints, (size_t)std::min(K, capacity), xyz, label, n_points));
  return K > capacity && (xyz || label || n_points) ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int sgtd_result_local_map_members(sgtd_handle e, int64_t *mem_off, int32_t *member, int64_t capacity, int64_t *n_members, int64_t *merged_points,
                                  int32_t *n_passes) {
  if (!e || capacity < 0) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::lm_n, kNoLocalMap, &c));
  const int64_t M = c->lm_mem_off.back();
  if (n_members) *n_members = M;
  if (n_passes) *n_passes = c->lm_passes;
  if (mem_off) std::memcpy(mem_off, c->lm_mem_off.data(), c->lm_mem_off.size() * sizeof(int64_t));
  if (merged_points && !c->lm_merged.empty()) std::memcpy(merged_points, c->lm_merged.data(), c->lm_merged.size() * sizeof(int64_t));
  CopyOut out(e, c);
  out.get(member, c->lm.member.p(), (size_t)std::min(M, capacity) * sizeof(int));
  CHK(out.finish());
  return M > capacity && member ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int sgtd_local_map_device_view(sgtd_handle e, const float **d_xyz, const uint32_t **d_label) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::lm_n, kNoLocalMap, &c));
  if (d_xyz) *d_xyz = c->lm.xyz.p();
  if (d_label) *d_label = c->lm.label.p();
  return SGTD_OK;
}

int sgtd_local_map_stage_ms(sgtd_handle e, float *ms_members, float *ms_gather, float *ms_scan) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::lm_n, kNoLocalMap, &c));
  if (ms_members) *ms_members = c->lm_clock.ms[0];
  if (ms_gather) *ms_gather = c->lm_clock.ms[1];
  if (ms_scan) *ms_scan = c->lm_clock.ms[2];
  return SGTD_OK;
}

}  // extern "C"

// ---- sgtd_thin_clouds: voxel-grid thinning of raw clouds on the device (thin_kernels.hip.h) ----
namespace {

int thin_run(sgtd_engine *e, const float *points, int stride, const int64_t *pt_off, int S, double leaf, int device_ptrs) {
  const long long P = pt_off[S];
  const size_t np = (size_t)P;
  sgtd_engine::ThinBufs &B = e->th;
  const hipStream_t st = e->stream;
  const bool timed = e->timing;
  LapClock &clock = e->th_clock;      // (ms: the two sorts, the whole call)
  CHK(clock.start(e, timed));
  e->th_out_off.assign((size_t)S + 1, 0);
  e->th_dropped.assign((size_t)S * 2, 0);
  e->th_stride = stride; e->th_kept = 0;
  CHK(need(e, B.out, 0));      // (a call that keeps nothing still has results to point to)
  if (S == 0 || P == 0) return xfer_sync(e);

  const float *d_pts = nullptr;
  CHK(points_on_device(e, B.pts.buf, points, np * stride, device_ptrs, &d_pts));
  CHK(need(e, B.off, (size_t)S + 1));
  CHK(h2d(e, B.off.p(), pt_off, ((size_t)S + 1) * sizeof(long long)));
  CHK(need_each(e, np, B.key_pt, B.cl_pt, B.key_a, B.key_b, B.ckey_a, B.ckey_b, B.val_a, B.val_b));
  CHK(need_each(e, np + 1, B.flags, B.excl, B.first, B.first_excl));
  CHK(need(e, B.counts, 4));
  CHK(need(e, B.cstart, np + 1));
  CHK(need(e, B.dropped, (size_t)S * 2));
  CHK(need(e, B.out_off, (size_t)S + 1));
  const int gp = grid_for(P, 256);
  const long long *d_off = B.off.p();
  u64 *key_pt = B.key_pt.p();
  u32 *cl_pt = B.cl_pt.p();
  u64 *kin = B.key_a.p(), *kout = B.key_b.p();
  u32 *ckin = B.ckey_a.p(), *ckout = B.ckey_b.p();
  u32 *vin = B.val_a.p(), *vout = B.val_b.p();
  u32 *flags = B.flags.p(), *excl = B.excl.p();
  u32 *first = B.first.p(), *first_excl = B.first_excl.p();
  u32 *counts = B.counts.p(), *cstart = B.cstart.p();
  int *dropped = B.dropped.p();
  long long *d_out_off = B.out_off.p();

  // keys, the two sorts
  if (timed) HIPCHK(hipEventRecord(clock.ev[0], st));
  HIPCHK(hipMemsetAsync(dropped, 0, (size_t)S * 2 * sizeof(int), st));
  HIPCHK(hipMemsetAsync(counts, 0, 4 * sizeof(u32), st));
  HIPCHK(hipMemsetAsync(first, 0, (np + 1) * sizeof(u32), st));
  thin_keys_kernel<<<gp, 256, 0, st>>>(d_pts, stride, d_off, S, P, leaf, key_pt, cl_pt, kin, vin, dropped);
  HIPCHK(hipGetLastError());
  if (timed) HIPCHK(hipEventRecord(clock.ev[1], st));
  CHK(radix_sort_pairs<u64>(e, kin, kout, vin, vout, P, 3 * SGTD_THIN_CELL_BITS, false));
  thin_cloud_keys_kernel<<<gp, 256, 0, st>>>(vin, cl_pt, P, ckin);
  HIPCHK(hipGetLastError());
  CHK(radix_sort_pairs<u32>(e, ckin, ckout, vin, vout, P, key_bits((u64)S), false));
  if (timed) HIPCHK(hipEventRecord(clock.ev[2], st));

  // cells in key order, their places by smallest point index, the clouds' offsets
  thin_heads_kernel<<<grid_for(P + 1, 256), 256, 0, st>>>(vin, key_pt, cl_pt, P, (u32)S, flags, first, counts);
  HIPCHK(hipGetLastError());
  CHK(device_scan(e, flags, excl, P + 1));
  CHK(device_scan(e, first, first_excl, P + 1));
  thin_cells_kernel<<<gp, 256, 0, st>>>(flags, excl, P, counts, cstart);
  thin_offsets_kernel<<<grid_for(S + 1, 256), 256, 0, st>>>(first_excl, d_off, S, d_out_off);
  HIPCHK(hipGetLastError());
  CHK(d2h(e, e->th_out_off.data(), d_out_off, ((size_t)S + 1) * sizeof(long long)));
  CHK(d2h(e, e->th_dropped.data(), dropped, (size_t)S * 2 * sizeof(int)));
  CHK(xfer_sync(e));
  if (timed) CHK(clock.span(e, 1, 2, 0, true));
  const long long K = e->th_out_off[(size_t)S];
  e->th_kept = K;

  // the sums
  CHK(need(e, B.out, (size_t)std::max<long long>(K, 1) * stride));
  if (K > 0) {
    float *out = B.out.p();
    if (stride == 3) thin_sum_kernel<3><<<grid_for(K, 256), 256, 0, st>>>(d_pts, vin, cstart, first_excl, excl + P, out);
    else thin_sum_kernel<4><<<grid_for(K, 256), 256, 0, st>>>(d_pts, vin, cstart, first_excl, excl + P, out);
    HIPCHK(hipGetLastError());
  }
  if (timed) {
    HIPCHK(hipEventRecord(clock.ev[1], st));
    CHK(clock.span(e, 0, 1, 1, true));
  }
  // (the caller's array is read for the last time by the sums: the call returns when they are done)
  return xfer_sync(e);
}

const char kNoThin[] = "no thinned clouds: sgtd_thin_clouds has not run";

}  // namespace

extern "C" {

int sgtd_thin_clouds(sgtd_handle e, const float *points, int stride_floats, const int64_t *pt_off, int n_clouds, double leaf, int device_ptrs) {
  if (!e) return SGTD_ERR_INVALID;
  if (!cloud_set_ok(pt_off, n_clouds, stride_floats, points, false, nullptr)) return SGTD_ERR_INVALID;
  if (!(std::isfinite(leaf) && leaf > 0.0)) return SGTD_ERR_INVALID;
  if (n_clouds > SGTD_REG_MAX_CLOUDS || pt_off[n_clouds] > SGTD_SCAN_MAX_POINTS) {
    e->err = "sgtd_thin_clouds takes at most " + std::to_string(SGTD_REG_MAX_CLOUDS) + " clouds and " + std::to_string(SGTD_SCAN_MAX_POINTS) +
             " points in one call";
    return SGTD_ERR_UNSUPPORTED;
  }
  StageRun<int> run(e, &sgtd_engine::th_n);
  run.on_device([&](sgtd_engine *k) { return thin_run(k, points, stride_floats, pt_off, n_clouds, leaf, device_ptrs); });
  return run.end(n_clouds);
}

int sgtd_result_thinned(sgtd_handle e, int64_t *out_off, float *points, int32_t *n_dropped, int64_t capacity, int64_t *n) {
  if (!e || capacity < 0) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::th_n, kNoThin, &c));
  const int64_t K = c->th_kept;
  if (n) *n = K;
  if (out_off) std::memcpy(out_off, c->th_out_off.data(), c->th_out_off.size() * sizeof(int64_t));
  if (n_dropped && !c->th_dropped.empty()) std::memcpy(n_dropped, c->th_dropped.data(), c->th_dropped.size() * sizeof(int32_t));
  CopyOut out(e, c);
  out.get(points, c->th.out.p(), (size_t)std::min(K, capacity) * c->th_stride * sizeof(float));
  CHK(out.finish());
  return K > capacity && points ? SGTD_ERR_CAPACITY : SGTD_OK;
}

int sgtd_thinned_device_view(sgtd_handle e, const float **d_points, int *stride_floats, int64_t *n_points) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::th_n, kNoThin, &c));
  if (d_points) *d_points = c->th.out.p();
  if (stride_floats) *stride_floats = c->th_stride;
  if (n_points) *n_points = c->th_kept;
  return SGTD_OK;
}

int sgtd_thin_stage_ms(sgtd_handle e, float *ms_sort, float *ms_rest, float *ms_total) {
  if (!e) return SGTD_ERR_INVALID;
  sgtd_engine *c = nullptr;
  CHK(stage_ready(e, &sgtd_engine::th_n, kNoThin, &c));
  if (ms_sort) *ms_sort = c->th_clock.ms[0];
  if (ms_rest) *ms_rest = c->th_clock.ms[1] - c->th_clock.ms[0];
  if (ms_total) *ms_total = c->th_clock.ms[1];
  return SGTD_OK;
}

}  // extern "C"

#include "graph_ingest_abi.h"
#include "multi_impl.hip.h"
