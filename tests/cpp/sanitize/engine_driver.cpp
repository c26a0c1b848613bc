// engine_driver.cpp — the engine's host code (sgtd_accel.hip, multi_impl.hip.h) under ASan + UBSan, against hip_stub.cpp.
// No kernel runs: "device" buffers are zeroed host memory and the launch hook below leaves behind what selected kernels
// would have — overflow flags, record needs, pair totals, a frame's packed results — so that the host walks its growth,
// re-run, stale-view, capacity and table-file paths with every copy checked by the sanitizer.  The stages on a verified batch
// (sgtd_refine_poses, sgtd_overlap, sgtd_align_keypoints) run in a scenario of their own below, whose stand-in results name the
// (query, candidate) slot they belong to.  The forms of the query pipeline (launch_select's plan and stages, the list pass run
// again, deferred lists, the diagnostic re-run) run in a third scenario with the stand-in's trace on: every launch, memset,
// attribute and event record is a line of the transcript.  Compiled for the host only
// (hipcc --cuda-host-only: the kernel headers are needed for the argument structs); tests/test_sanitizers.py builds and runs it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include <stdint.h>

#include "../../../include/sgtd_accel.h"
// the kernels' argument structs (ProbeBuffers, the frame pack's layout) come with the kernels themselves: in a namespace of
// their own here, so that this file's copies of the host-side launch stubs do not collide with the engine's
namespace kernels_of_the_engine {
#include "../../../sgtd_amd/csrc/build_kernel.hip.h"       // (the engine's own include order: the headers lean on each other)
#include "../../../sgtd_amd/csrc/common.hip.h"
#include "../../../sgtd_amd/csrc/table_kernels.hip.h"
#include "../../../sgtd_amd/csrc/probe_kernels.hip.h"
#include "../../../sgtd_amd/csrc/select_kernels.hip.h"
#include "../../../sgtd_amd/csrc/verify_kernels.hip.h"
#include "../../../sgtd_amd/csrc/refine_kernels.hip.h"
#include "../../../sgtd_amd/csrc/overlap_kernels.hip.h"
#include "../../../sgtd_amd/csrc/align_kernels.hip.h"
}  // namespace kernels_of_the_engine
using kernels_of_the_engine::ProbeBuffers;
using kernels_of_the_engine::frame_pack_bytes;
using kernels_of_the_engine::FramePack;
using kernels_of_the_engine::u32;
using kernels_of_the_engine::u64;

extern "C" {
typedef void (*launch_hook_t)(const char *name, void **args, void *user);
void sgtd_stub_set_launch_hook(launch_hook_t h, void *user);
unsigned long long sgtd_stub_launches();
unsigned long long sgtd_stub_copies();
unsigned long long sgtd_stub_waits();
unsigned sgtd_stub_grid_x();
size_t sgtd_stub_device_bytes();
size_t sgtd_stub_device_peak();
size_t sgtd_stub_device_peak_restart();
size_t sgtd_stub_device_blocks();
size_t sgtd_stub_block_size(const void *p);
void sgtd_stub_set_trace(FILE *f);
}

#define REQUIRE(x) do { if (!(x)) { fprintf(stderr, "engine_driver: %s failed at line %d\n", #x, __LINE__); exit(1); } } while (0)
static sgtd_handle g_last = nullptr;     // (whose error text a failed call reports)
#define OK(call) do { const int st_ = (call); if (st_ != SGTD_OK) { fprintf(stderr, "engine_driver: %s = %d at line %d (%s)\n", #call, st_, __LINE__, g_last ? sgtd_last_error(g_last) : ""); exit(1); } } while (0)

namespace {
struct Scenario {
  int sweep_overflows = 0;          // the next launches of the sweep report that the record buffer was too small ...
  unsigned long long need = 0;      // ... by this many records,
  bool reservations = false;        // ... or that the RESERVATIONS outran it (the host then drops the reservation rate)
  int pair_overflows = 0;           // the next launches of query_base_kernel report that the pair buffer was too small
  unsigned pairs_total = 0;         // candidate pairs of the batch (q_pair_base[nq])
  int cand_num = 50;
  long long frame_inliers = -1;     // pack_frame_kernel: inlier pairs the frame's verification "found" (-1: leave zeros)
  int frame_overflow = 0;           // pack_frame_kernel: the next packs carry a set overflow flag (sgtd_search_frame falls back)
  unsigned long long sweeps = 0, packs = 0;
  // the stages' scenario: the candidate tables and the results of the verification and of the three stages are filled in
  bool stages = false;
  int expect_order = -1;            // the frame-ordered dispatch of the four kernels that take one: 1 it must be there, 0 it must not, -1 either
  unsigned long long stage_launches[4] = {0, 0, 0, 0};      // verify, refine, overlap, align
  // the select-forms scenario
  unsigned longest = 0;             // frame_longest_kernel: entries of the table's largest frame (0: leave the zero), sizes the entry ids' rank
  unsigned rough_matches = 0;       // resolve_undecided_kernel: rough matches of query 0 (sgtd_result_rough has something to gather)
};
bool g_tracing = false;             // the select-forms scenario: every launch adds its scalars to the transcript (trace_args)
void trace_args(const char *name, void **args);

// bytes from p to the end of the block it lies in
size_t room_of(const void *p) {
  hipDeviceptr_t base; size_t size;
  REQUIRE(hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) == hipSuccess);
  return size - (size_t)(static_cast<const char *>(p) - static_cast<const char *>(base));
}

// FramePack puts every field where the arithmetic it replaced put it (the offsets written out once more, as numbers), and
// every 8-byte field on an 8-byte boundary
bool frame_pack_layout_holds(int cn) {
  namespace K = kernels_of_the_engine;
  alignas(8) static unsigned char block[112 + 128 * 64];
  const FramePack F(block, cn);
  const size_t n = (size_t)cn;
  auto at = [&](const void *p) { return (size_t)(static_cast<const unsigned char *>(p) - block); };
  const size_t eight[] = {at(F.q_P()), at(F.pair_off()), at(F.score()), at(F.pose()), at(F.inl_off()), at(F.totals())};
  for (size_t o : eight)
    if (o % 8) return false;
  return at(F.ctr()) == 0 && at(F.ctr() + K::CTR_SWEPT) == 24 && at(F.ctr() + K::CTR_LIST_MOVES) == 36 &&
         at(F.ctr() + K::CTR_OVERFLOW) == 40 && K::CTR_COUNT == 12 &&
         at(F.n_cand()) == 48 && at(F.q_M()) == 52 && at(F.pairs_total()) == 56 && at(F.q_count()) == 60 && at(F.q_P()) == 64 &&
         at(F.cand_frame()) == 72 && at(F.cand_votes()) == 72 + n * 4 && at(F.pair_off()) == 72 + n * 8 &&
         at(F.score()) == 72 + n * 8 + (n + 1) * 8 && at(F.pose()) == 72 + n * 8 + (n + 1) * 8 + n * 8 &&
         at(F.inl_off()) == 72 + n * 8 + (n + 1) * 8 + n * 8 + n * 96 && at(F.totals()) == 72 + n * 8 + (n + 1) * 8 + n * 8 + n * 96 + (n + 1) * 8 &&
         at(F.totals()) == frame_pack_bytes(cn) && F.bytes() == frame_pack_bytes(cn) + 24 && F.bytes() == 112 + 128 * n;
}

// ---- what the stages' scenario leaves in the candidate tables: functions of (query, slot) alone, the same on every "device"
int cand_count_of(int q, int cn) { return q % 7 == 3 ? 0 : std::min(cn, 18 + (q * 11) % 40); }
int cand_frame_of(int q, int k) { return (q + k) % 64; }           // (a device's local id: distinct within a query)
int cand_votes_of(int q, int k) { return (cand_frame_of(q, k) * 13 + q * 5) % 41; }      // (some below the merge's five)
const double kNaN = std::numeric_limits<double>::quiet_NaN();

void fill_candidates(int nq, int cn, int *n_cand, int *frame, int *votes) {
  REQUIRE(room_of(n_cand) >= (size_t)nq * 4 && room_of(frame) >= (size_t)nq * cn * 4 && room_of(votes) >= (size_t)nq * cn * 4);
  for (int q = 0; q < nq; q++) {
    n_cand[q] = cand_count_of(q, cn);
    for (int k = 0; k < cn; k++) {
      const bool live = k < n_cand[q];
      frame[(size_t)q * cn + k] = live ? cand_frame_of(q, k) : -1;
      votes[(size_t)q * cn + k] = live ? cand_votes_of(q, k) : 0;
    }
  }
}
void fill_offsets(int nq, int cn, const int *n_cand, const int *votes, long long *pair_off, u32 *q_pairs) {
  REQUIRE(room_of(pair_off) >= (size_t)nq * (cn + 1) * 8 && room_of(q_pairs) >= (size_t)nq * 4);
  for (int q = 0; q < nq; q++) {
    long long acc = 0;
    for (int k = 0; k <= cn; k++) {
      pair_off[(size_t)q * (cn + 1) + k] = acc;
      if (k < n_cand[q]) acc += votes[(size_t)q * cn + k];
    }
    q_pairs[q] = (u32)acc;
  }
}

// what every kernel of a stage is handed in common: the frame-ordered dispatch as the scenario expects it, the batch's tables
template <class P> int stage_head(Scenario &S, const P &p, int stage) {
  S.stage_launches[stage]++;
  const u32 nb = p.n_blocks;
  REQUIRE(p.cand_num > 0 && nb % (u32)p.cand_num == 0 && sgtd_stub_grid_x() >= nb);
  if (S.expect_order >= 0) REQUIRE((p.order != nullptr) == (S.expect_order == 1));
  if (p.order) REQUIRE(room_of(p.order) >= (size_t)nb * 4);
  const int nq = (int)(nb / (u32)p.cand_num);
  REQUIRE(room_of(p.n_cand) >= (size_t)nq * 4 && room_of(p.score) >= (size_t)nb * 8);
  return nq;
}
template <class P> bool slot_live(const P &p, u32 blk) {
  return (int)(blk % (u32)p.cand_num) < p.n_cand[blk / (u32)p.cand_num] && p.score[blk] >= 0.0;
}
// the keypoint passes' inputs: the query keypoints with their offsets, the store's device copy
template <class P> void keypoint_room(const P &p, int nq) {
  REQUIRE(room_of(p.cand_frame) >= (size_t)p.n_blocks * 4 && room_of(p.pose) >= (size_t)p.n_blocks * 12 * 8);
  REQUIRE(room_of(p.q_off) >= (size_t)(nq + 1) * 8);
  const size_t last = (size_t)p.q_off[nq];
  if (last) REQUIRE(room_of(p.q_xyz) >= last * 12 && room_of(p.q_label) >= last * 4);
  REQUIRE(room_of(p.f_word) >= (size_t)std::max<u32>(p.n_ids, 1) * 8);
  size_t kp_end = 0;
  for (u32 id = 0; id < p.n_ids; id++)
    if (p.f_word[id] != SGTD_OVERLAP_NONE) kp_end = std::max(kp_end, (size_t)(p.f_word[id] >> 16) + (size_t)(p.f_word[id] & 0xFFFFull));
  REQUIRE(room_of(p.kp) >= std::max<size_t>(kp_end, 1) * 16);
}

std::vector<const void *> g_gathers_into;      // gather_pair_entries_kernel launches: the `side` array each was handed

void hook(const char *name, void **args, void *user) {
  Scenario &S = *static_cast<Scenario *>(user);
  if (g_tracing) trace_args(name, args);
  if (strstr(name, "frame_longest_kernel")) {
    if (S.longest) (*static_cast<u32 **>(args[4]))[0] = S.longest;
  } else if (strstr(name, "resolve_undecided_kernel")) {
    if (S.rough_matches) (*static_cast<u32 **>(args[3]))[0] = S.rough_matches;
  } else if (strstr(name, "probe_sorted_kernel")) {
    S.sweeps++;
    const ProbeBuffers &B = *static_cast<const ProbeBuffers *>(args[1]);
    REQUIRE(sgtd_stub_block_size(B.ctr) >= 12 * sizeof(u32));
    // the record buffer the kernel was handed really has the granules it was told (+ the quads read past the last list)
    REQUIRE(sgtd_stub_block_size(B.rec) >= ((size_t)B.rec_cap << SGTD_REC_SHIFT) * sizeof(u32));
    REQUIRE(B.rec_slab >= 1 && B.rec_rate >= 1 && B.rec_rate <= 256);
    if (S.sweep_overflows > 0) {
      S.sweep_overflows--;
      B.overflow()[0] = 1;
      *B.rec_need() = S.need;
      *B.rec_cursor() = S.reservations ? (unsigned long long)B.rec_cap * 4ull : (unsigned long long)B.rec_cap;
    } else {
      *B.rec_cursor() = B.rec_cap / 2;
    }
  } else if (strstr(name, "small_order_kernel")) {
    // a one-frame batch clears its counters inside this kernel (the general form: a memset, which the stand-in performs)
    const kernels_of_the_engine::SmallOrder &O = *static_cast<const kernels_of_the_engine::SmallOrder *>(args[1]);
    REQUIRE(sgtd_stub_block_size(O.ctr) >= (size_t)O.ctr_words * sizeof(u32) && sgtd_stub_block_size(O.pos_of_slot) >= (size_t)O.max_pass_slots * sizeof(u32));
    REQUIRE(!O.votes || sgtd_stub_block_size(O.votes) >= (size_t)O.span * sizeof(u32));
    REQUIRE(sgtd_stub_block_size(O.slot_of_words) >= (size_t)((O.span + 3u) / 4u) * sizeof(u32));
    REQUIRE(sgtd_stub_block_size(O.gid) >= (size_t)O.n_slots * sizeof(u32) && sgtd_stub_block_size(O.order) >= (size_t)O.n_slots * sizeof(u32));
    memset(O.ctr, 0, (size_t)O.ctr_words * sizeof(u32));
  } else if (strstr(name, "head_flags_kernel")) {
    // the bucket count of a segment = (head flag of the last entry) + (exclusive scan at the last entry): with no scan running both
    // reads see this word — half the buckets the table is to "have"
    u32 *flags = *static_cast<u32 **>(args[1]);
    const long long E = *static_cast<long long *>(args[2]);
    REQUIRE(E > 0 && sgtd_stub_block_size(flags) >= (size_t)E * sizeof(u32));
    flags[E - 1] = (u32)(E / 32 + 1);
  } else if (strstr(name, "query_base_kernel")) {
    u32 *q_pair_base = *static_cast<u32 **>(args[1]);
    const int nq = *static_cast<int *>(args[2]);
    int *overflow = *static_cast<int **>(args[4]);
    REQUIRE(sgtd_stub_block_size(q_pair_base) >= (size_t)(nq + 1) * sizeof(u32));
    if (S.stages) {
      const u32 *q_pairs = *static_cast<u32 **>(args[0]);
      q_pair_base[0] = 0;
      for (int q = 0; q < nq; q++) q_pair_base[q + 1] = q_pair_base[q] + q_pairs[q];
    } else {
      for (int q = 0; q <= nq; q++) q_pair_base[q] = (u32)((unsigned long long)S.pairs_total * q / nq);
    }
    if (S.pair_overflows > 0) { S.pair_overflows--; overflow[1] = 1; }
  } else if (strstr(name, "block_scan_kernel")) {
    // a one-query batch: the scan leaves the query's base and total itself (no query_base_kernel launch)
    u32 *base_of_one = *static_cast<u32 **>(args[7]);
    int *overflow = *static_cast<int **>(args[6]);
    if (base_of_one) {
      REQUIRE(sgtd_stub_block_size(base_of_one) >= 2 * sizeof(u32));
      base_of_one[0] = 0; base_of_one[1] = S.pairs_total;
      if (S.pair_overflows > 0) { S.pair_overflows--; overflow[1] = 1; }
    }
  } else if (strstr(name, "gather_pair_entries_kernel")) {
    // where the entries go, and that every array the kernel is handed has the room it is told
    const long long cap = *static_cast<long long *>(args[2]);
    int *qi = *static_cast<int **>(args[3]);
    const kernels_of_the_engine::DescArrays &out = *static_cast<const kernels_of_the_engine::DescArrays *>(args[5]);
    REQUIRE(room_of(out.side) >= (size_t)cap * 24 && room_of(out.angle) >= (size_t)cap * 24 && room_of(out.center) >= (size_t)cap * 24);
    REQUIRE(room_of(out.vertex) >= (size_t)cap * 36 && room_of(out.label) >= (size_t)cap * 12 && room_of(out.node_id) >= (size_t)cap * 12);
    REQUIRE(room_of(out.frame) >= (size_t)cap * 4 && room_of(qi) >= (size_t)cap * 4);
    g_gathers_into.push_back(out.side);
  } else if (S.stages && strstr(name, "topk_kernel")) {
    // the candidate tables (votes_topk_kernel leaves the lists' offsets too); one block per query
    const bool fused = strstr(name, "votes_topk_kernel") != nullptr;
    const int cn = *static_cast<int *>(args[fused ? 5 : 3]), nq = (int)sgtd_stub_grid_x();
    int *n_cand = *static_cast<int **>(args[fused ? 8 : 4]), *frame = *static_cast<int **>(args[fused ? 9 : 5]), *votes = *static_cast<int **>(args[fused ? 10 : 6]);
    fill_candidates(nq, cn, n_cand, frame, votes);
    if (fused) fill_offsets(nq, cn, n_cand, votes, *static_cast<long long **>(args[11]), *static_cast<u32 **>(args[12]));
  } else if (S.stages && strstr(name, "cand_prefix_kernel")) {
    fill_offsets(*static_cast<int *>(args[3]), *static_cast<int *>(args[2]), *static_cast<int **>(args[0]), *static_cast<int **>(args[1]),
                 *static_cast<long long **>(args[4]), *static_cast<u32 **>(args[5]));
  } else if (S.stages && strstr(name, "verify_solve_kernel")) {
    const kernels_of_the_engine::VerifyParams &P = *static_cast<const kernels_of_the_engine::VerifyParams *>(args[0]);
    const int nq = stage_head(S, P, 0);
    REQUIRE(room_of(P.pose) >= (size_t)P.n_blocks * 12 * 8 && room_of(P.pair_off) >= (size_t)nq * (P.cand_num + 1) * 8);
    for (u32 b = 0; b < P.n_blocks; b++) {
      const bool live = (int)(b % (u32)P.cand_num) < P.n_cand[b / (u32)P.cand_num];
      P.score[b] = (live && b % 11 != 5) ? 0.05 + 0.001 * (double)((b * 37u) % 800u) : -1.0;
      for (int i = 0; i < 12; i++) P.pose[(size_t)b * 12 + i] = P.score[b] >= 0.0 ? (i % 4 == 0 && i < 9 ? 1.0 : 0.0) + 0.001 * (double)((b + i) % 17u) + (i >= 9 ? (double)(b % 13u) : 0.0) : 0.0;
    }
  } else if (S.stages && strstr(name, "refine_kernel")) {
    const kernels_of_the_engine::RefineParams &P = *static_cast<const kernels_of_the_engine::RefineParams *>(args[0]);
    const int nq = stage_head(S, P, 1);
    const size_t nb = P.n_blocks;
    REQUIRE(room_of(P.v_pose) >= nb * 12 * 8 && room_of(P.pair_off) >= (size_t)nq * (P.cand_num + 1) * 8 && room_of(P.q_pair_base) >= (size_t)(nq + 1) * 4);
    REQUIRE(room_of(P.pose) >= nb * 12 * 8 && room_of(P.rmse) >= nb * 8 && room_of(P.rmse_verify) >= nb * 8 && room_of(P.n_pairs) >= nb * 4 && room_of(P.moments) >= nb * 15 * 8);
    // every list lies inside the flags of the verification and, from the second iteration on, inside each half of the stage's own
    for (int q = 0; q < nq; q++) {
      const size_t end = (size_t)P.q_pair_base[q] + (size_t)P.pair_off[(size_t)q * (P.cand_num + 1) + P.cand_num];
      REQUIRE(end <= P.flag_half);
      if (end) REQUIRE(room_of(P.v_inlier) >= end);
    }
    if (P.iterations > 1) REQUIRE(room_of(P.flag) >= 2 * P.flag_half);
    for (u32 b = 0; b < P.n_blocks; b++) {
      const bool live = slot_live(P, b) && b % 13 != 4;       // (a candidate without a result has no pairs)
      for (int i = 0; i < 12; i++) P.pose[(size_t)b * 12 + i] = live ? P.v_pose[(size_t)b * 12 + i] + 0.25 : 0.0;
      P.rmse[b] = live ? 0.125 * (double)(b % 9u) : kNaN;
      P.rmse_verify[b] = live ? 0.5 + 0.125 * (double)(b % 7u) : kNaN;
      P.n_pairs[b] = live ? 3 + (int)(b % 5u) : 0;
      for (int i = 0; i < 15; i++) P.moments[(size_t)b * 15 + i] = live ? (double)b + (double)i / 16.0 : kNaN;
    }
  } else if (S.stages && strstr(name, "overlap_kernel")) {
    const kernels_of_the_engine::OverlapParams &P = *static_cast<const kernels_of_the_engine::OverlapParams *>(args[0]);
    const int nq = stage_head(S, P, 2);
    keypoint_room(P, nq);
    REQUIRE(room_of(P.cnt) >= (size_t)P.n_blocks * 16 && room_of(P.val) >= (size_t)P.n_blocks * 16);
    for (u32 b = 0; b < P.n_blocks; b++) {
      const bool live = slot_live(P, b);
      const int q = (int)(b / (u32)P.cand_num), nqk = (int)(P.q_off[q + 1] - P.q_off[q]);
      // (the second value is the pose the pass was handed: sgtd_verify's or sgtd_refine_poses')
      P.cnt[b] = live ? make_int4(nqk, 10 + (int)(b % 20u), (int)(b % 7u), (int)(b % 5u)) : make_int4(-1, -1, -1, -1);
      P.val[b] = live ? make_double2((double)(b % 10u) / 10.0, P.pose[(size_t)b * 12]) : make_double2(kNaN, kNaN);
    }
  } else if (S.stages && strstr(name, "align_kernel")) {
    const kernels_of_the_engine::AlignParams &P = *static_cast<const kernels_of_the_engine::AlignParams *>(args[0]);
    const int nq = stage_head(S, P, 3);
    keypoint_room(P, nq);
    const size_t nb = P.n_blocks, total = (size_t)(P.q_off[nq] - P.q_off[0]);
    REQUIRE(room_of(P.o_pose) >= nb * 12 * 8 && room_of(P.fit) >= nb * 16 && room_of(P.cnt) >= nb * 32 && room_of(P.val) >= nb * 32 && room_of(P.moments) >= nb * 15 * 8);
    REQUIRE(room_of(P.assign) >= std::max<size_t>(total * (size_t)P.cand_num, 1) * 4);
    for (u32 b = 0; b < P.n_blocks; b++) {
      const bool live = slot_live(P, b) && b % 17 != 2;        // (stop -1: a candidate without a result)
      const int q = (int)(b / (u32)P.cand_num), c = (int)(b % (u32)P.cand_num), nqk = (int)(P.q_off[q + 1] - P.q_off[q]);
      for (int i = 0; i < 12; i++) P.o_pose[(size_t)b * 12 + i] = live ? P.pose[(size_t)b * 12 + i] + 0.5 : 0.0;
      for (int i = 0; i < 15; i++) P.moments[(size_t)b * 15 + i] = live ? 0.5 * (double)b + (double)i / 16.0 : kNaN;
      P.fit[b] = live ? make_int4(1 + (int)(b % 3u), (int)(b % 9u), (int)(b % 3u), 0) : make_int4(0, 0, -1, 0);
      P.cnt[(size_t)b * 2] = live ? make_int4(nqk, 10 + (int)(b % 20u), (int)(b % 7u), (int)(b % 5u)) : make_int4(-1, -1, -1, -1);
      P.cnt[(size_t)b * 2 + 1] = live ? make_int4(nqk, 10 + (int)(b % 20u), (int)(b % 8u), (int)(b % 6u)) : make_int4(-1, -1, -1, -1);
      const double rms_after = b % 6 == 1 ? kNaN : 0.25 + 0.03125 * (double)(b % 23u);
      const double v[4] = {(double)(b % 7u) / 8.0, P.pose[(size_t)b * 12], (double)(b % 10u) / 10.0, rms_after};
      for (int i = 0; i < 4; i++) P.val[(size_t)b * 4 + i] = live ? v[i] : kNaN;
      int *asg = P.assign + (size_t)(P.q_off[q] - P.q_off[0]) * (size_t)P.cand_num + (size_t)c * (size_t)nqk;
      for (int j = 0; j < nqk; j++) asg[j] = live ? (j * 7 + c + q) % 19 - 1 : -1;
    }
  } else if (strstr(name, "pack_frame_kernel")) {
    S.packs++;
    const int cn = *static_cast<int *>(args[12]);
    unsigned char *out = *static_cast<unsigned char **>(args[13]);
    REQUIRE(sgtd_stub_block_size(out) >= frame_pack_bytes(cn));
    REQUIRE(frame_pack_layout_holds(1) && frame_pack_layout_holds(50) && frame_pack_layout_holds(64));
    namespace K = kernels_of_the_engine;
    const FramePack F(out, cn);
    memcpy(F.ctr(), *static_cast<const u32 **>(args[0]), K::CTR_COUNT * sizeof(u32));      // (the batch's counters and flags, as the kernel copies them)
    if (S.frame_overflow > 0) { S.frame_overflow--; F.ctr()[K::CTR_OVERFLOW] = 1; return; }
    if (S.frame_inliers >= 0) {
      *F.n_cand() = 1; *F.q_M() = 100; *F.pairs_total() = (u32)S.frame_inliers; *F.q_count() = 64;
      for (int k = 1; k <= cn; k++) { F.pair_off()[k] = S.frame_inliers; F.inl_off()[k] = S.frame_inliers; }
      F.score()[0] = (double)S.frame_inliers;
    }
  }
}

struct Descs {
  std::vector<double> side, angle, center;
  std::vector<float> vertex;
  std::vector<int32_t> label, node;
  std::vector<uint32_t> frame;
  sgtd_desc_soa soa() { return sgtd_desc_soa{side.data(), angle.data(), center.data(), vertex.data(), label.data(), frame.data(), node.data()}; }
  void resize(size_t n) { side.resize(n * 3); angle.resize(n * 3); center.resize(n * 3); vertex.resize(n * 9); label.resize(n * 3); node.resize(n * 3); frame.resize(n); }
};
Descs random_descs(std::mt19937 &rng, size_t n, uint32_t frame) {
  Descs d;
  d.resize(n);
  std::uniform_real_distribution<double> u(2.0, 28.0);
  for (size_t i = 0; i < n; i++) {
    double s[3] = {u(rng), u(rng), u(rng)};
    if (s[0] > s[1]) std::swap(s[0], s[1]);
    if (s[1] > s[2]) std::swap(s[1], s[2]);
    if (s[0] > s[1]) std::swap(s[0], s[1]);
    for (int k = 0; k < 3; k++) { d.side[i * 3 + k] = s[k]; d.label[i * 3 + k] = 3 + (int)(rng() % 9); d.node[i * 3 + k] = (int)(rng() % 200); d.center[i * 3 + k] = u(rng); }
    for (int k = 0; k < 9; k++) d.vertex[i * 9 + k] = (float)u(rng);
    d.frame[i] = frame;
  }
  return d;
}

// ---- the stages on a verified batch: sgtd_refine_poses, sgtd_overlap, sgtd_align_keypoints and what reads their results ----
// One line per call goes to the transcript (if one is asked for): the call, its status, the handle's error text, the stand-in's
// launch, copy and wait counts, a hash of every output array.  Two builds of the engine behave alike if their transcripts are equal.
FILE *g_transcript = nullptr;
void hash_bytes(u64 &h, const void *p, size_t n) {
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
}
template <class... V> void logged(int line, int expect, const char *call, sgtd_handle h, int st, const V &...outs) {
  u64 hash = 1469598103934665603ull;
  (void)std::initializer_list<int>{(hash_bytes(hash, outs.data(), outs.size() * sizeof(outs[0])), 0)...};
  if (g_transcript)
    fprintf(g_transcript, "%s = %d \"%s\" launches %llu copies %llu waits %llu out %016llx\n", call, st, sgtd_last_error(h), sgtd_stub_launches(),
            sgtd_stub_copies(), sgtd_stub_waits(), (unsigned long long)hash);
  if (st != expect) { fprintf(stderr, "engine_driver: %s = %d, not %d, at line %d (%s)\n", call, st, expect, line, sgtd_last_error(h)); exit(1); }
}
#define CALL(expect, h, call, ...) logged(__LINE__, expect, #call, h, (call), ##__VA_ARGS__)

bool same(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0 || (std::isnan(a) && std::isnan(b)); }
bool same(const double *a, const double *b, size_t n) { for (size_t i = 0; i < n; i++) if (!same(a[i], b[i])) return false; return true; }

struct Keypoints {        // of some frames or queries: offsets, positions, labels
  std::vector<int64_t> off{0};
  std::vector<float> xyz;
  std::vector<uint32_t> label;
  void add(std::mt19937 &rng, int n) {
    std::uniform_real_distribution<float> u(-20.f, 20.f);
    for (int i = 0; i < n; i++) { for (int k = 0; k < 3; k++) xyz.push_back(u(rng)); label.push_back(3 + rng() % 9); }
    if (xyz.empty()) xyz.reserve(3);
    if (label.empty()) label.reserve(1);
    off.push_back((int64_t)label.size());
  }
};

// one query's results as the public getters give them
struct Results {
  int cn;
  std::vector<int32_t> n_cand, frame;       // of the whole batch
  std::vector<int64_t> pair_off;            // of the whole batch: [nq][cn + 1]
  std::vector<int32_t> p_q; std::vector<int64_t> p_entry, i_off, i_entry; std::vector<int32_t> i_q;      // match lists and inlier pairs
  std::vector<double> score, pose;
  std::vector<double> r_pose, rmse, rmse_v, r_mom; std::vector<int32_t> np;
  std::vector<int32_t> o_cnt[4]; std::vector<double> o_ov, o_rms;
  std::vector<double> a_pose, a_mom, a_val[4]; std::vector<int32_t> a_fit[3], a_cnt[2];
  explicit Results(int cn_, int nq) : cn(cn_), n_cand((size_t)nq), frame((size_t)nq * cn_), pair_off((size_t)nq * (cn_ + 1)), i_off((size_t)cn_ + 1), score(cn_), pose((size_t)cn_ * 12), r_pose((size_t)cn_ * 12), rmse(cn_), rmse_v(cn_),
      r_mom((size_t)cn_ * 15), np(cn_), o_ov(cn_), o_rms(cn_), a_pose((size_t)cn_ * 12), a_mom((size_t)cn_ * 15) {
    for (auto &v : o_cnt) v.resize(cn_);
    for (auto &v : a_val) v.resize(cn_);
    for (auto &v : a_fit) v.resize(cn_);
    for (auto &v : a_cnt) v.resize((size_t)cn_ * 4);
  }
  void candidates(sgtd_handle h) { CALL(SGTD_OK, h, sgtd_result_candidates(h, n_cand.data(), frame.data(), nullptr, pair_off.data()), n_cand, frame, pair_off); }
  // query q's match lists (all of them: their total is the last offset) and inlier pairs (how many first, then the pairs)
  void lists(sgtd_handle h, int q) {
    std::vector<int64_t> n(1, -1);
    const size_t total = (size_t)pair_off[(size_t)q * (cn + 1) + cn];
    p_q.assign(total + 1, -7); p_entry.assign(total + 1, -7);
    if (total > 0) CALL(SGTD_ERR_CAPACITY, h, sgtd_result_pairs(h, q, p_q.data(), p_entry.data(), (int64_t)total - 1, n.data()), n);
    CALL(SGTD_OK, h, sgtd_result_pairs(h, q, p_q.data(), p_entry.data(), (int64_t)total, n.data()), p_q, p_entry, n);
    REQUIRE(n[0] == (int64_t)total && p_q[total] == -7 && p_entry[total] == -7);
    const int st = sgtd_result_inlier_pairs(h, q, i_off.data(), nullptr, nullptr, 0, n.data());
    REQUIRE(st == SGTD_OK || st == SGTD_ERR_CAPACITY);
    i_q.assign((size_t)n[0] + 1, -7); i_entry.assign((size_t)n[0] + 1, -7);
    CALL(SGTD_OK, h, sgtd_result_inlier_pairs(h, q, i_off.data(), i_q.data(), i_entry.data(), n[0], n.data()), i_off, i_q, i_entry, n);
    REQUIRE(i_off[(size_t)cn] == n[0] && i_q[(size_t)n[0]] == -7);
  }
  void verify(sgtd_handle h, int q) { CALL(SGTD_OK, h, sgtd_result_verify(h, q, score.data(), pose.data()), score, pose); }
  void refined(sgtd_handle h, int q) { CALL(SGTD_OK, h, sgtd_result_refined(h, q, r_pose.data(), rmse.data(), rmse_v.data(), np.data(), r_mom.data()), r_pose, rmse, rmse_v, np, r_mom); }
  void overlap(sgtd_handle h, int q) {
    CALL(SGTD_OK, h, sgtd_result_overlap(h, q, o_cnt[0].data(), o_cnt[1].data(), o_cnt[2].data(), o_cnt[3].data(), o_ov.data(), o_rms.data()), o_cnt[0], o_cnt[1], o_cnt[2], o_cnt[3], o_ov, o_rms);
  }
  void aligned(sgtd_handle h, int q) {
    CALL(SGTD_OK, h, sgtd_result_aligned(h, q, a_pose.data(), a_fit[0].data(), a_fit[1].data(), a_fit[2].data(), a_cnt[0].data(), a_cnt[1].data(), a_val[0].data(), a_val[1].data(),
                                         a_val[2].data(), a_val[3].data(), a_mom.data()), a_pose, a_fit[0], a_fit[1], a_fit[2], a_cnt[0], a_cnt[1], a_val[0], a_val[1], a_val[2], a_val[3], a_mom);
  }
};

struct Stages {
  sgtd_handle h = nullptr;
  int n_dev = 1, cn = 0, n_frames = 130;
  std::vector<float> map_pose;            // [n_frames][12]; frame 5 has none
  std::vector<char> has_pose;
  Keypoints own, theirs;                  // the batch's keypoints, and others the caller passes to a keypoint pass
  std::vector<int> kp_count;              // of the batch's queries: whose keypoints a pass ran on (own or theirs)
  bool refined = false, overlapped = false, aligned = false;

  // the world pose of candidate k as include/sgtd_accel.h states it: every operation an f32 rounding, NaN where there is none
  void check_world(const std::vector<float> &world, int n_cand, const int32_t *frame, const double *pose, const std::vector<char> &has) const {
    for (int k = 0; k < cn; k++) {
      float w[12];
      for (float &x : w) x = std::numeric_limits<float>::quiet_NaN();
      const bool live = k < n_cand && has[(size_t)k] && frame[k] >= 0 && frame[k] < n_frames && has_pose[(size_t)frame[k]];
      if (live) {
        const float *M = map_pose.data() + (size_t)frame[k] * 12;
        float R[9], t[3];
        for (int i = 0; i < 9; i++) R[i] = (float)pose[(size_t)k * 12 + i];
        for (int i = 0; i < 3; i++) t[i] = (float)pose[(size_t)k * 12 + 9 + i];
        for (int i = 0; i < 3; i++) {
          const float *m = M + i * 4;
          for (int j = 0; j < 3; j++) w[i * 4 + j] = (m[0] * R[j] + m[1] * R[3 + j]) + m[2] * R[6 + j];
          w[i * 4 + 3] = ((m[0] * t[0] + m[1] * t[1]) + m[2] * t[2]) + m[3];
        }
      }
      for (int i = 0; i < 12; i++) REQUIRE(live ? std::memcmp(&w[i], &world[(size_t)k * 12 + i], 4) == 0 : std::isnan(world[(size_t)k * 12 + i]));
    }
  }

  // every getter of every query of a verified batch, with what can be derived from them asserted; on a handle of several
  // "devices" each merged candidate's results against its owner's own getters
  void read_all(int nq) {
    Results r(cn, nq);
    r.candidates(h);
    std::vector<Results> dev;
    for (int s = 0; s < n_dev && n_dev > 1; s++) { dev.emplace_back(cn, nq); dev.back().candidates(sgtd_device_handle(h, s)); }
    std::vector<float> world((size_t)cn * 12);
    std::vector<char> has((size_t)cn);
    std::vector<std::vector<double>> all_score, all_ov, all_a_ov, all_a_rms; std::vector<std::vector<int32_t>> all_stop;
    for (int q = 0; q < nq; q++) {
      const int nc = r.n_cand[(size_t)q];
      const int32_t *frame = r.frame.data() + (size_t)q * cn;
      r.verify(h, q);
      r.lists(h, q);
      all_score.push_back(r.score);
      CALL(SGTD_OK, h, sgtd_result_world_poses(h, q, world.data()), world);
      for (int k = 0; k < cn; k++) has[(size_t)k] = r.score[(size_t)k] >= 0.0;
      check_world(world, nc, frame, r.pose.data(), has);
      if (refined) {
        r.refined(h, q);
        CALL(SGTD_OK, h, sgtd_result_refined_world_poses(h, q, world.data()), world);
        for (int k = 0; k < cn; k++) has[(size_t)k] = r.np[(size_t)k] > 0;
        check_world(world, nc, frame, r.r_pose.data(), has);
      }
      if (overlapped) {
        r.overlap(h, q);
        all_ov.push_back(r.o_ov);
        for (int k = 0; k < nc; k++) REQUIRE(r.o_cnt[0][(size_t)k] == -1 || r.o_cnt[0][(size_t)k] == kp_count[(size_t)q]);
      }
      std::vector<std::vector<int32_t>> asg((size_t)cn);
      if (aligned) {
        r.aligned(h, q);
        all_stop.push_back(r.a_fit[2]); all_a_ov.push_back(r.a_val[2]); all_a_rms.push_back(r.a_val[3]);
        CALL(SGTD_OK, h, sgtd_result_aligned_world_poses(h, q, world.data()), world);
        for (int k = 0; k < cn; k++) has[(size_t)k] = r.a_fit[2][(size_t)k] >= 0;
        check_world(world, nc, frame, r.a_pose.data(), has);
        // every candidate's assignment: its length with no array, a capacity one short, all of it
        for (int k = 0; k < nc; k++) {
          std::vector<int64_t> n(1, -1);
          CALL(SGTD_OK, h, sgtd_result_aligned_pairs(h, q, k, nullptr, 0, n.data()), n);
          REQUIRE(n[0] == kp_count[(size_t)q]);
          asg[(size_t)k].assign((size_t)n[0] + 1, -7);
          if (n[0] > 0) CALL(SGTD_ERR_CAPACITY, h, sgtd_result_aligned_pairs(h, q, k, asg[(size_t)k].data(), n[0] - 1, n.data()), n);
          CALL(SGTD_OK, h, sgtd_result_aligned_pairs(h, q, k, asg[(size_t)k].data(), n[0], n.data()), asg[(size_t)k], n);
          REQUIRE(asg[(size_t)k][(size_t)n[0]] == -7);
        }
        std::vector<int64_t> n(1, -1);
        CALL(SGTD_ERR_INVALID, h, sgtd_result_aligned_pairs(h, q, nc, nullptr, 0, n.data()));
        CALL(SGTD_ERR_INVALID, h, sgtd_result_aligned_pairs(h, q, 0, nullptr, 0, nullptr));
      }
      if (n_dev == 1) continue;
      // ---- the gather from the owners
      std::vector<Results> &d = dev;
      for (int s = 0; s < n_dev; s++) {
        sgtd_handle c = sgtd_device_handle(h, s);
        d[(size_t)s].verify(c, q);
        d[(size_t)s].lists(c, q);
        if (refined) d[(size_t)s].refined(c, q);
        if (overlapped) d[(size_t)s].overlap(c, q);
        if (aligned) d[(size_t)s].aligned(c, q);
      }
      int from[2] = {0, 0};
      for (int k = 0; k < cn; k++) {
        if (k >= nc) {        // no candidate: what the handle states for an empty slot
          REQUIRE(r.score[(size_t)k] == -1.0);
          for (int i = 0; i < 12; i++) REQUIRE(r.pose[(size_t)k * 12 + i] == 0.0);
          if (refined) REQUIRE(r.np[(size_t)k] == 0 && std::isnan(r.rmse[(size_t)k]) && std::isnan(r.rmse_v[(size_t)k]) && std::isnan(r.r_mom[(size_t)k * 15]) && r.r_pose[(size_t)k * 12] == 0.0);
          if (overlapped) REQUIRE(r.o_cnt[0][(size_t)k] == -1 && r.o_cnt[3][(size_t)k] == -1 && std::isnan(r.o_ov[(size_t)k]) && std::isnan(r.o_rms[(size_t)k]));
          if (aligned) REQUIRE(r.a_fit[0][(size_t)k] == 0 && r.a_fit[1][(size_t)k] == 0 && r.a_fit[2][(size_t)k] == -1 && r.a_cnt[0][(size_t)k * 4] == -1 && r.a_cnt[1][(size_t)k * 4 + 3] == -1 &&
                               std::isnan(r.a_val[0][(size_t)k]) && std::isnan(r.a_val[3][(size_t)k]) && std::isnan(r.a_mom[(size_t)k * 15]) && r.a_pose[(size_t)k * 12] == 0.0);
          continue;
        }
        // the owner: the shard of the merged (global) frame id; the slot: where the owner's own table has the frame's local id
        const uint32_t g = (uint32_t)frame[k];
        const int s = (int)((g / 64u) % (uint32_t)n_dev);
        const int32_t local = (int32_t)((g / (64u * (uint32_t)n_dev)) * 64u + g % 64u);
        const Results &o = d[(size_t)s];
        int ks = -1;
        for (int j = 0; j < o.n_cand[(size_t)q]; j++) if (o.frame[(size_t)q * cn + j] == local) ks = j;
        REQUIRE(ks >= 0);
        from[s]++;
        REQUIRE(same(r.score[(size_t)k], o.score[(size_t)ks]) && same(&r.pose[(size_t)k * 12], &o.pose[(size_t)ks * 12], 12));
        {     // its match list and inlier pairs: the owner's, the owner in the entry ids' upper bits
          const int64_t *mo = &r.pair_off[(size_t)q * (cn + 1) + k], *oo = &o.pair_off[(size_t)q * (cn + 1) + ks];
          REQUIRE(mo[1] - mo[0] == oo[1] - oo[0] && r.i_off[(size_t)k + 1] - r.i_off[(size_t)k] == o.i_off[(size_t)ks + 1] - o.i_off[(size_t)ks]);
          for (int64_t j = 0; j < mo[1] - mo[0]; j++)
            REQUIRE(r.p_q[(size_t)(mo[0] + j)] == o.p_q[(size_t)(oo[0] + j)] && r.p_entry[(size_t)(mo[0] + j)] == (((int64_t)s << 40) | o.p_entry[(size_t)(oo[0] + j)]));
          for (int64_t j = 0; j < r.i_off[(size_t)k + 1] - r.i_off[(size_t)k]; j++)
            REQUIRE(r.i_q[(size_t)(r.i_off[(size_t)k] + j)] == o.i_q[(size_t)(o.i_off[(size_t)ks] + j)] &&
                    r.i_entry[(size_t)(r.i_off[(size_t)k] + j)] == (((int64_t)s << 40) | o.i_entry[(size_t)(o.i_off[(size_t)ks] + j)]));
        }
        if (refined) REQUIRE(same(&r.r_pose[(size_t)k * 12], &o.r_pose[(size_t)ks * 12], 12) && same(r.rmse[(size_t)k], o.rmse[(size_t)ks]) && same(r.rmse_v[(size_t)k], o.rmse_v[(size_t)ks]) &&
                             r.np[(size_t)k] == o.np[(size_t)ks] && same(&r.r_mom[(size_t)k * 15], &o.r_mom[(size_t)ks * 15], 15));
        if (overlapped) {
          for (int a = 0; a < 4; a++) REQUIRE(r.o_cnt[a][(size_t)k] == o.o_cnt[a][(size_t)ks]);
          REQUIRE(same(r.o_ov[(size_t)k], o.o_ov[(size_t)ks]) && same(r.o_rms[(size_t)k], o.o_rms[(size_t)ks]));
        }
        if (aligned) {
          REQUIRE(same(&r.a_pose[(size_t)k * 12], &o.a_pose[(size_t)ks * 12], 12) && same(&r.a_mom[(size_t)k * 15], &o.a_mom[(size_t)ks * 15], 15));
          for (int a = 0; a < 3; a++) REQUIRE(r.a_fit[a][(size_t)k] == o.a_fit[a][(size_t)ks]);
          for (int a = 0; a < 2; a++) REQUIRE(std::memcmp(&r.a_cnt[a][(size_t)k * 4], &o.a_cnt[a][(size_t)ks * 4], 16) == 0);
          for (int a = 0; a < 4; a++) REQUIRE(same(r.a_val[a][(size_t)k], o.a_val[a][(size_t)ks]));
          std::vector<int32_t> mine((size_t)kp_count[(size_t)q] + 1, -7);
          std::vector<int64_t> n(1, -1);
          sgtd_handle c = sgtd_device_handle(h, s);
          CALL(SGTD_OK, c, sgtd_result_aligned_pairs(c, q, ks, mine.data(), kp_count[(size_t)q], n.data()), mine, n);
          REQUIRE(mine == asg[(size_t)k]);
        }
      }
      if (nc == cn) REQUIRE(from[0] > 0 && from[1] > 0);       // (a full merged list draws on both owners)
    }
    // ---- the three search loops, against their rules over the public results
    std::vector<int32_t> bc((size_t)nq), bf((size_t)nq);
    std::vector<double> bs((size_t)nq), bo((size_t)nq);
    CALL(SGTD_OK, h, sgtd_search_loop(h, 0.4, bc.data(), bf.data(), bs.data()), bc, bf, bs);
    auto pick_score = [&](int q, double thr, double min_ov, int *cand, double *score) {     // the highest score above thr (the first of equals)
      *cand = -1; *score = 0.0;
      for (int c = 0; c < r.n_cand[(size_t)q]; c++) {
        if (min_ov > 0.0 && !(all_ov[(size_t)q][(size_t)c] >= min_ov)) continue;
        if (all_score[(size_t)q][(size_t)c] > *score) { *score = all_score[(size_t)q][(size_t)c]; *cand = c; }
      }
      if (!(*cand >= 0 && *score > thr)) { *cand = -1; *score = 0.0; }
    };
    for (int q = 0; q < nq && n_dev > 1; q++) {     // (on one device the rule runs in a kernel: nothing to compare with here)
      int c; double sc;
      pick_score(q, 0.4, 0.0, &c, &sc);
      REQUIRE(bc[(size_t)q] == c && same(bs[(size_t)q], sc) && bf[(size_t)q] == (c >= 0 ? r.frame[(size_t)q * cn + c] : -1));
    }
    for (double min_ov : {0.0, 0.5}) {
      if (min_ov > 0.0 && !overlapped) {
        CALL(SGTD_ERR_STATE, h, sgtd_search_loop_overlap(h, 0.4, min_ov, bc.data(), bf.data(), bs.data(), bo.data()));
        continue;
      }
      CALL(SGTD_OK, h, sgtd_search_loop_overlap(h, 0.4, min_ov, bc.data(), bf.data(), bs.data(), bo.data()), bc, bf, bs, bo);
      for (int q = 0; q < nq; q++) {
        int c; double sc;
        pick_score(q, 0.4, min_ov, &c, &sc);
        REQUIRE(bc[(size_t)q] == c && same(bs[(size_t)q], sc) && bf[(size_t)q] == (c >= 0 ? r.frame[(size_t)q * cn + c] : -1));
        REQUIRE(same(bo[(size_t)q], c >= 0 && overlapped ? all_ov[(size_t)q][(size_t)c] : kNaN));
      }
    }
    if (!aligned) {
      CALL(SGTD_ERR_STATE, h, sgtd_search_loop_aligned(h, 0.0, 0.0, bc.data(), bf.data(), bs.data(), bo.data()));
      return;
    }
    const double bounds[3][2] = {{0.0, 0.0}, {0.5, 0.0}, {0.3, 0.6}};
    for (const double *b : bounds) {
      CALL(SGTD_OK, h, sgtd_search_loop_aligned(h, b[0], b[1], bc.data(), bf.data(), bs.data(), bo.data()), bc, bf, bs, bo);
      for (int q = 0; q < nq; q++) {       // the lowest rms after alignment inside the bounds; of equals the higher score, then the first
        int best = -1;
        const std::vector<double> &rms = all_a_rms[(size_t)q], &ov = all_a_ov[(size_t)q], &sc = all_score[(size_t)q];
        for (int c = 0; c < r.n_cand[(size_t)q]; c++) {
          if (all_stop[(size_t)q][(size_t)c] < 0 || std::isnan(rms[(size_t)c])) continue;
          if (b[0] > 0.0 && !(ov[(size_t)c] >= b[0])) continue;
          if (b[1] > 0.0 && !(rms[(size_t)c] <= b[1])) continue;
          if (best < 0 || rms[(size_t)c] < rms[(size_t)best] || (rms[(size_t)c] == rms[(size_t)best] && sc[(size_t)c] > sc[(size_t)best])) best = c;
        }
        REQUIRE(bc[(size_t)q] == best && bf[(size_t)q] == (best >= 0 ? r.frame[(size_t)q * cn + best] : -1));
        REQUIRE(same(bs[(size_t)q], best >= 0 ? rms[(size_t)best] : kNaN) && same(bo[(size_t)q], best >= 0 ? ov[(size_t)best] : kNaN));
      }
    }
  }

  // the state errors of a batch none of whose stage results exist (any more)
  void nothing_to_read() {
    std::vector<double> d((size_t)cn * 15);
    std::vector<int32_t> i((size_t)cn * 4);
    std::vector<float> w((size_t)cn * 12);
    std::vector<int64_t> n(1);
    CALL(SGTD_ERR_STATE, h, sgtd_result_refined(h, 0, d.data(), nullptr, nullptr, nullptr, nullptr));
    CALL(SGTD_ERR_STATE, h, sgtd_result_refined_world_poses(h, 0, w.data()));
    CALL(SGTD_ERR_STATE, h, sgtd_result_overlap(h, 0, i.data(), nullptr, nullptr, nullptr, d.data(), nullptr));
    CALL(SGTD_ERR_STATE, h, sgtd_search_loop_overlap(h, 0.4, 0.5, i.data(), nullptr, nullptr, nullptr));
    CALL(SGTD_ERR_STATE, h, sgtd_result_aligned(h, 0, d.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    CALL(SGTD_ERR_STATE, h, sgtd_result_aligned_pairs(h, 0, 0, nullptr, 0, n.data()));
    CALL(SGTD_ERR_STATE, h, sgtd_result_aligned_world_poses(h, 0, w.data()));
    CALL(SGTD_ERR_STATE, h, sgtd_search_loop_aligned(h, 0.0, 0.0, i.data(), nullptr, nullptr, nullptr));
    refined = overlapped = aligned = false;
  }
  void stages_refuse(int expect) {       // the three stages where the batch is not verified
    CALL(expect, h, sgtd_refine_poses(h, 1));
    CALL(expect, h, sgtd_overlap(h, 0.5, 0, nullptr, nullptr, nullptr));
    CALL(expect, h, sgtd_overlap(h, 0.5, 0, theirs.xyz.data(), theirs.label.data(), theirs.off.data()));
    CALL(expect, h, sgtd_align_keypoints(h, 0.5, 3, 0, nullptr, nullptr, nullptr));
    CALL(expect, h, sgtd_align_keypoints(h, 0.5, 3, 0, theirs.xyz.data(), theirs.label.data(), theirs.off.data()));
  }
  void counts_of(const Keypoints &k, int nq) { kp_count.resize((size_t)nq); for (int q = 0; q < nq; q++) kp_count[(size_t)q] = (int)(k.off[(size_t)q + 1] - k.off[(size_t)q]); }
  void frames_batch(std::mt19937 &rng, int nq) {
    own = Keypoints(); theirs = Keypoints();
    for (int q = 0; q < nq; q++) { own.add(rng, q == 2 ? 0 : 12 + q % 5); theirs.add(rng, 7 + q % 3); }
    CALL(SGTD_OK, h, sgtd_query_frames(h, own.xyz.data(), own.label.data(), own.off.data(), nq, 0));
    refined = overlapped = aligned = false;
  }

  void run(Scenario &S, const sgtd_config &cfg, std::mt19937 &rng, int n_dev_) {
    n_dev = n_dev_; cn = cfg.candidate_num;
    S.stages = true; S.expect_order = -1;
    if (n_dev == 1) OK(sgtd_create(&cfg, &h));
    else { const int ids[2] = {0, 0}; OK(sgtd_create_multi(&cfg, ids, 2, &h)); }
    g_last = h;
    for (int f = 0; f < n_frames; f++) { Descs d = random_descs(rng, 60, (uint32_t)f); sgtd_desc_soa s = d.soa(); OK(sgtd_add(h, &s, 60)); }
    OK(sgtd_finalize(h));
    // ---- the map's poses (all frames but 5) and keypoints (all but 9; frame 11 has an empty set); a set of 65536 is refused
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::vector<uint32_t> ids;
    Keypoints map_kp;
    map_pose.assign((size_t)n_frames * 12, 0.f); has_pose.assign((size_t)n_frames, 0);
    std::vector<float> rows;
    for (int f = 0; f < n_frames; f++) {
      if (f == 5) continue;
      ids.push_back((uint32_t)f); has_pose[(size_t)f] = 1;
      for (int i = 0; i < 12; i++) { map_pose[(size_t)f * 12 + i] = u(rng) * (i % 4 == 3 ? 50.f : 1.f); rows.push_back(map_pose[(size_t)f * 12 + i]); }
    }
    CALL(SGTD_OK, h, sgtd_set_frame_poses(h, ids.data(), rows.data(), (int64_t)ids.size()));
    ids.clear();
    for (int f = 0; f < n_frames; f++) {
      if (f == 9) continue;
      ids.push_back((uint32_t)f);
      map_kp.add(rng, f == 11 ? 0 : 20 + f % 7);
    }
    CALL(SGTD_OK, h, sgtd_set_frame_keypoints(h, ids.data(), map_kp.off.data(), map_kp.xyz.data(), map_kp.label.data(), (int64_t)ids.size()));
    {
      const uint32_t one[1] = {3};
      const int64_t big[2] = {0, 65536}, most[2] = {0, 65535};
      std::vector<float> xyz((size_t)65536 * 3, 1.f);
      std::vector<uint32_t> lab(65536, 4u);
      CALL(SGTD_ERR_INVALID, h, sgtd_set_frame_keypoints(h, one, big, xyz.data(), lab.data(), 1));
      CALL(SGTD_OK, h, sgtd_set_frame_keypoints(h, one, most, xyz.data(), lab.data(), 1));
      CALL(SGTD_OK, h, sgtd_set_frame_keypoints(h, one, map_kp.off.data() + 3, map_kp.xyz.data(), map_kp.label.data(), 1));
    }
    // ---- no batch yet: every stage and every getter refuses
    theirs.add(rng, 5);
    stages_refuse(SGTD_ERR_STATE);
    nothing_to_read();

    // ---- a batch of nine query frames: the stages before sgtd_verify; each getter before its stage; *_REFINED before
    // sgtd_refine_poses; each stage with the batch's own keypoints and with the caller's, from sgtd_verify's poses and
    // from the refined ones; every getter after every step
    const int nq = 9;
    frames_batch(rng, nq);
    stages_refuse(SGTD_ERR_STATE);
    CALL(SGTD_OK, h, sgtd_verify(h));
    nothing_to_read();
    read_all(nq);
    CALL(SGTD_ERR_STATE, h, sgtd_overlap(h, 0.5, SGTD_OVERLAP_REFINED, nullptr, nullptr, nullptr));
    CALL(SGTD_ERR_STATE, h, sgtd_align_keypoints(h, 0.5, 3, SGTD_ALIGN_REFINED, nullptr, nullptr, nullptr));
    CALL(SGTD_ERR_INVALID, h, sgtd_overlap(h, -1.0, 0, nullptr, nullptr, nullptr));
    CALL(SGTD_ERR_INVALID, h, sgtd_overlap(h, 0.5, 2, nullptr, nullptr, nullptr));
    CALL(SGTD_ERR_INVALID, h, sgtd_overlap(h, 0.5, 0, theirs.xyz.data(), nullptr, theirs.off.data()));
    CALL(SGTD_ERR_INVALID, h, sgtd_align_keypoints(h, 0.5, 0, 0, nullptr, nullptr, nullptr));
    CALL(SGTD_ERR_INVALID, h, sgtd_align_keypoints(h, 0.5, 3, 2, nullptr, nullptr, nullptr));
    CALL(SGTD_ERR_INVALID, h, sgtd_refine_poses(h, 0));
    {     // a query with 65536 keypoints (the count is refused before anything is read); and that mistake together with a missing refit
      std::vector<int64_t> off(theirs.off);
      for (int q = 4; q <= nq; q++) off[(size_t)q] += 65536 - (theirs.off[4] - theirs.off[3]);
      CALL(SGTD_ERR_INVALID, h, sgtd_overlap(h, 0.5, 0, theirs.xyz.data(), theirs.label.data(), off.data()));
      CALL(SGTD_ERR_INVALID, h, sgtd_align_keypoints(h, 0.5, 3, 0, theirs.xyz.data(), theirs.label.data(), off.data()));
      CALL(SGTD_ERR_INVALID, h, sgtd_overlap(h, 0.5, SGTD_OVERLAP_REFINED, theirs.xyz.data(), theirs.label.data(), off.data()));
      CALL(SGTD_ERR_INVALID, h, sgtd_align_keypoints(h, 0.5, 3, SGTD_ALIGN_REFINED, theirs.xyz.data(), theirs.label.data(), off.data()));
    }
    counts_of(theirs, nq);
    CALL(SGTD_OK, h, sgtd_overlap(h, 0.5, 0, theirs.xyz.data(), theirs.label.data(), theirs.off.data()));
    overlapped = true;
    read_all(nq);
    counts_of(own, nq);
    CALL(SGTD_OK, h, sgtd_overlap(h, 0.5, 0, nullptr, nullptr, nullptr));
    read_all(nq);
    CALL(SGTD_OK, h, sgtd_align_keypoints(h, 0.5, 3, 0, nullptr, nullptr, nullptr));
    aligned = true;
    read_all(nq);
    CALL(SGTD_OK, h, sgtd_refine_poses(h, 1));
    refined = true;
    read_all(nq);
    CALL(SGTD_OK, h, sgtd_refine_poses(h, 3));
    counts_of(theirs, nq);
    CALL(SGTD_OK, h, sgtd_overlap(h, 0.5, SGTD_OVERLAP_REFINED, theirs.xyz.data(), theirs.label.data(), theirs.off.data()));
    CALL(SGTD_OK, h, sgtd_align_keypoints(h, 0.5, 2, SGTD_ALIGN_REFINED, theirs.xyz.data(), theirs.label.data(), theirs.off.data()));
    read_all(nq);
    counts_of(own, nq);
    CALL(SGTD_OK, h, sgtd_overlap(h, 0.5, SGTD_OVERLAP_REFINED, nullptr, nullptr, nullptr));
    CALL(SGTD_OK, h, sgtd_align_keypoints(h, 0.5, 1, SGTD_ALIGN_REFINED, nullptr, nullptr, nullptr));
    read_all(nq);
    {     // a query out of range
      std::vector<double> d((size_t)cn * 15);
      std::vector<float> w((size_t)cn * 12);
      std::vector<int64_t> n(1);
      for (int q : {-1, nq}) {
        CALL(SGTD_ERR_INVALID, h, sgtd_result_refined(h, q, d.data(), nullptr, nullptr, nullptr, nullptr));
        CALL(SGTD_ERR_INVALID, h, sgtd_result_overlap(h, q, nullptr, nullptr, nullptr, nullptr, d.data(), nullptr));
        CALL(SGTD_ERR_INVALID, h, sgtd_result_aligned(h, q, d.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        CALL(SGTD_ERR_INVALID, h, sgtd_result_aligned_pairs(h, q, 0, nullptr, 0, n.data()));
        CALL(SGTD_ERR_INVALID, h, sgtd_result_world_poses(h, q, w.data()));
        CALL(SGTD_ERR_INVALID, h, sgtd_result_refined_world_poses(h, q, w.data()));
        CALL(SGTD_ERR_INVALID, h, sgtd_result_aligned_world_poses(h, q, w.data()));
      }
    }
    // a new sgtd_verify makes the three results stale; so does a new batch
    CALL(SGTD_OK, h, sgtd_verify(h));
    nothing_to_read();
    CALL(SGTD_OK, h, sgtd_refine_poses(h, 2)); CALL(SGTD_OK, h, sgtd_overlap(h, 0.25, 0, nullptr, nullptr, nullptr)); CALL(SGTD_OK, h, sgtd_align_keypoints(h, 0.25, 2, 0, nullptr, nullptr, nullptr));
    refined = overlapped = aligned = true;
    read_all(nq);
    frames_batch(rng, nq);
    nothing_to_read();
    stages_refuse(SGTD_ERR_STATE);

    // ---- a batch of descriptors has no keypoints of its own: a keypoint pass takes the caller's; so does a batch of no
    // descriptors.  (A batch of no QUERIES, nq == 0, cannot be made through the public calls: sgtd_query_frames refuses
    // n_queries <= 0, a descriptor batch and sgtd_search_frame are one query.  The stages' `nq == 0` exits are therefore
    // not reached here or anywhere; the nearest cases run instead: this batch of one query without descriptors, and
    // query 2 of every frame batch, which has no keypoints.)
    for (int64_t n_descs : {(int64_t)400, (int64_t)0}) {
      Descs q = random_descs(rng, 400, (uint32_t)n_frames);
      sgtd_desc_soa qs = q.soa();
      CALL(SGTD_OK, h, sgtd_query_descs(h, &qs, n_descs));
      CALL(SGTD_OK, h, sgtd_verify(h));
      CALL(SGTD_ERR_STATE, h, sgtd_overlap(h, 0.5, 0, nullptr, nullptr, nullptr));
      CALL(SGTD_ERR_STATE, h, sgtd_align_keypoints(h, 0.5, 3, 0, nullptr, nullptr, nullptr));
      CALL(SGTD_ERR_STATE, h, sgtd_overlap(h, 0.5, SGTD_OVERLAP_REFINED, nullptr, nullptr, nullptr));      // (two mistakes: the missing refit is named)
      nothing_to_read();
      counts_of(theirs, 1);
      CALL(SGTD_OK, h, sgtd_refine_poses(h, 2));
      CALL(SGTD_OK, h, sgtd_overlap(h, 0.5, SGTD_OVERLAP_REFINED, theirs.xyz.data(), theirs.label.data(), theirs.off.data()));
      CALL(SGTD_OK, h, sgtd_align_keypoints(h, 0.5, 3, 0, theirs.xyz.data(), theirs.label.data(), theirs.off.data()));
      refined = overlapped = aligned = true;
      read_all(1);
    }

    // ---- the frame-ordered dispatch: from 4096 (query, candidate) slots on, on a table that has frames, all four kernels
    // that take an order get one (82 queries of 50 candidates: 4100); one query fewer (4050) and none does
    for (int big : {82, 81}) {
      REQUIRE(cn == 50);
      S.expect_order = big == 82 ? 1 : 0;
      for (unsigned long long &n : S.stage_launches) n = 0;
      frames_batch(rng, big);
      CALL(SGTD_OK, h, sgtd_verify(h));
      CALL(SGTD_OK, h, sgtd_refine_poses(h, 2));
      CALL(SGTD_OK, h, sgtd_overlap(h, 0.5, 0, nullptr, nullptr, nullptr));
      CALL(SGTD_OK, h, sgtd_align_keypoints(h, 0.5, 2, SGTD_ALIGN_REFINED, nullptr, nullptr, nullptr));
      for (unsigned long long n : S.stage_launches) REQUIRE(n == (unsigned long long)n_dev);
      S.expect_order = -1;
      refined = overlapped = aligned = true;
      counts_of(own, big);
      if (big == 81) read_all(big);
    }
    OK(sgtd_destroy(h));
    S.stages = false;
  }
};
// ---- the forms of the query pipeline (launch_select and what runs on its batch later), launch by launch ----
// While the stand-in's trace is on, every launch, memset, attribute and event record of the engine is a line of the transcript,
// and the hook adds the scalars of the launch it can type.  Two builds of the engine whose transcripts are equal enqueue the
// same work with the same geometry.
std::vector<std::string> g_launched;      // kernel names (as registered) launched while the trace was on, each once
template <class T> const T &arg(void **a, int k) { return *static_cast<const T *>(a[k]); }

void trace_args(const char *name, void **a) {
  namespace K = kernels_of_the_engine;
  FILE *f = g_transcript;
  if (std::find(g_launched.begin(), g_launched.end(), name) == g_launched.end()) g_launched.push_back(name);
  if (!f) return;
  auto has = [&](const char *s) { return strstr(name, s) != nullptr; };
  auto i = [&](const char *n, int k) { fprintf(f, " %s %d", n, arg<int>(a, k)); };
  auto u = [&](const char *n, int k) { fprintf(f, " %s %u", n, arg<u32>(a, k)); };
  auto l = [&](const char *n, int k) { fprintf(f, " %s %lld", n, arg<long long>(a, k)); };
  auto p = [&](const char *n, int k) { fprintf(f, " %s %d", n, arg<const void *>(a, k) != nullptr); };
  auto Q = [&](int k) { const K::QueryView &q = arg<K::QueryView>(a, k); fprintf(f, " Q{stride %lld n_queries %d chunk %u}", q.stride, q.n_queries, q.chunk); };
  auto B = [&](int k) {
    const ProbeBuffers &b = arg<ProbeBuffers>(a, k);
    fprintf(f, " B{rec_cap %u rec_slab %u rec_rate %u id_bits %u amb_cap %u rec room %zu}", b.rec_cap, b.rec_slab, b.rec_rate, b.id_bits, b.amb_cap, sgtd_stub_block_size(b.rec));
  };
  auto T = [&](int k) {
    const K::TableView &t = arg<K::TableView>(a, k);
    fprintf(f, " T{n_entries %u frame_lo %u frame_span %u tail_off %u n_entries1 %u map.bits %u map.frame_lo %u by_frame %d coarse_at %u whole_at %u}", t.n_entries, t.frame_lo, t.frame_span,
            t.tail_off, t.n_entries1, t.map.bits, t.map.frame_lo, t.map.by_frame != nullptr, t.coarse_at, t.whole_at);
  };
  auto M = [&](int k) { const K::IdMap &m = arg<K::IdMap>(a, k); fprintf(f, " map{bits %u frame_lo %u}", m.bits, m.frame_lo); };
  auto PP = [&](int k) { fprintf(f, " pool.cap %u", arg<K::PassPool>(a, k).cap); };
  auto CL = [&](int k) { const K::CompactLists &c = arg<K::CompactLists>(a, k); fprintf(f, " CL{cap %u blocks %lld}", c.cap, (long long)(c.blk_n - c.blk_start)); };
  fprintf(f, "  args");
  if (has("small_order_kernel")) {
    const K::SmallOrder &o = arg<K::SmallOrder>(a, 1);
    Q(0);
    fprintf(f, " SO{ctr_words %u votes %d span %u cand_num %d n_slots %u max_pass_slots %u cbits %d sub_bits %d pair %d key_bits %d n_qrec %u rough %.17g}", o.ctr_words, o.votes != nullptr,
            o.span, o.cand_num, o.n_slots, o.max_pass_slots, o.cbits, o.sub_bits, o.pair, o.key_bits, o.n_qrec, o.rough);
  } else if (has("thr2_kernel")) { l("n", 3); fprintf(f, " rough %.17g", arg<double>(a, 4)); }
  else if (has("loop_bound_kernel")) { l("stride", 1); i("nq", 2); u("frame0", 3); i("skip_near", 4); u("frame_lo", 5); }
  else if (has("query_prefix_kernel")) i("nq", 2);
  else if (has("home_keys_kernel")) { Q(0); l("n_slots", 4); i("cbits", 5); i("sub_bits", 6); }
  else if (has("radix_hist_kernel")) { l("n", 1); i("shift", 2); i("nblocks", 4); p("n_dev", 5); }
  else if (has("group_heads_kernel")) { l("n", 3); i("cbits", 4); i("sub_bits", 5); }
  else if (has("group_first_kernel")) l("n", 4);
  else if (has("pass_slots_kernel")) { l("n", 4); i("pair", 5); }
  else if (has("group_resolve_kernel")) { T(0); Q(1); u("rows_cap", 7); fprintf(f, " rows room %zu", sgtd_stub_block_size(arg<const void *>(a, 6))); }
  else if (has("plan_passes_kernel")) { T(0); Q(1); u("rows_cap", 8); PP(9); }
  else if (has("probe_sorted_kernel")) { T(0); B(1); Q(2); PP(3); fprintf(f, " rough %.17g", arg<double>(a, 4)); u("ticket", 7); }
  else if (has("resolve_undecided_kernel")) { T(0); Q(1); B(2); }
  else if (has("filter_records_kernel") || has("filter_compact_kernel")) { Q(0); B(1); i("n_rows", 3); u("n_words", 4); u("span", 5); i("wg_per_q", 6); }
  else if (has("prior_rows_kernel")) { u("span", 1); u("words", 2); i("prm_rows", 4); i("dims", 5); p("base", 6); i("base_rows", 7); i("n_rows", 8); }
  else if (has("votes_topk_kernel")) { Q(0); B(1); u("span", 2); u("frame_lo", 3); i("blocks", 4); i("cn", 5); }
  else if (has("votes_query_kernel")) { Q(0); B(1); u("span", 2); u("frame_lo", 3); u("tile_span", 4); i("blocks", 5); }
  else if (has("votes_kernel")) { Q(0); B(1); u("span", 2); u("frame_lo", 3); i("blocks", 4); }
  else if (has("topk_kernel")) { u("span", 1); u("frame_lo", 2); i("cn", 3); }
  else if (has("export_candidates_kernel")) { i("nq", 3); i("cn", 4); u("serial", 5); }
  else if (has("cand_prefix_masked_kernel")) { i("cn", 3); i("nq", 4); }
  else if (has("cand_prefix_kernel")) { i("cn", 2); i("nq", 3); }
  else if (has("query_base_kernel")) { i("nq", 2); u("pair_cap", 3); }
  else if (has("pairs_query_kernel")) { Q(0); B(1); i("cn", 4); M(8); u("span", 9); u("frame_lo", 10); p("keep", 11); }
  else if (has("block_count_kernel")) { Q(0); B(1); i("cn", 4); i("blocks", 5); CL(7); u("span", 11); u("frame_lo", 12); }
  else if (has("block_scan_kernel")) { i("blocks", 1); i("cn", 2); p("base_of_one", 7); u("pair_cap", 8); p("totals_of_one", 9); }
  else if (has("block_write_kernel")) { Q(0); B(1); CL(2); i("blocks", 3); i("cn", 5); M(9); }
  else if (has("rough_gather_kernel")) { Q(0); B(1); M(2); i("q", 3); p("cell", 7); p("dis", 8); }
  fprintf(f, "\n");
}

struct Env {      // an environment knob for the length of a scope
  const char *key;
  Env(const char *k, const char *v) : key(k) { setenv(k, v, 1); }
  ~Env() { unsetenv(key); }
};

struct SelectForms {
  Scenario &S;
  std::mt19937 &rng;
  sgtd_config base;
  sgtd_handle h = nullptr;
  void note(const char *fmt, long long a = 0, long long b = 0, long long c = 0) { if (g_transcript) { fprintf(g_transcript, "# "); fprintf(g_transcript, fmt, a, b, c); fprintf(g_transcript, "\n"); } }

  // a finalized table of two frames, ids 0 and span - 1 (the span costs nothing but the per-frame arrays); `stamp`: the id
  // the next query frame is stamped with, less two; tail: a third frame appended behind the finalized table
  void table(const sgtd_config &cfg_, uint32_t span, uint32_t stamp = 0, bool tail = false) {
    sgtd_config cfg = cfg_;
    cfg.max_frame_n = 700000; cfg.first_frame_id = stamp;
    note("table: span %lld, stamp %lld, tail %lld", span, stamp, tail);
    OK(sgtd_create(&cfg, &h));
    g_last = h;
    for (uint32_t id : {0u, span - 1}) {
      if (id == 0 && span == 1) continue;
      Descs d = random_descs(rng, 60, id);
      sgtd_desc_soa s = d.soa();
      CALL(SGTD_OK, h, sgtd_add(h, &s, 60));
    }
    CALL(SGTD_OK, h, sgtd_finalize(h));
    if (tail) {
      Descs d = random_descs(rng, 40, span);      // (newer than the main segment's newest frame: the span grows by one)
      sgtd_desc_soa s = d.soa();
      CALL(SGTD_OK, h, sgtd_add(h, &s, 40));
      CALL(SGTD_OK, h, sgtd_finalize(h));
      sgtd_stats st;
      OK(sgtd_get_stats(h, &st));
      REQUIRE(st.tail_entries > 0);
    }
  }
  void done() { OK(sgtd_destroy(h)); h = nullptr; g_last = nullptr; }

  void frames(int nq, int kp = 14, bool sync = true) {
    Keypoints k;
    for (int q = 0; q < nq; q++) k.add(rng, kp - q % 3);
    note("frames batch: %lld queries of up to %lld keypoints", nq, kp);
    CALL(SGTD_OK, h, sgtd_query_frames(h, k.xyz.data(), k.label.data(), k.off.data(), nq, 0));
    if (sync) CALL(SGTD_OK, h, sgtd_sync(h));
  }
  void descs(int n, bool sync = true) {
    Descs q = random_descs(rng, (size_t)n, 3);
    sgtd_desc_soa qs = q.soa();
    note("one-query batch: %lld descriptors", n);
    CALL(SGTD_OK, h, sgtd_query_descs(h, &qs, n));
    if (sync) CALL(SGTD_OK, h, sgtd_sync(h));
  }
  void rough(int q) {       // the diagnostic re-run and its gather
    std::vector<int32_t> qi(64), cell(64); std::vector<int64_t> en(64), n(1); std::vector<uint32_t> fr(64); std::vector<double> dis(64);
    S.rough_matches = 5;
    CALL(SGTD_OK, h, sgtd_result_rough(h, q, qi.data(), cell.data(), en.data(), fr.data(), dis.data(), 64, n.data()), n);
    CALL(SGTD_OK, h, sgtd_result_rough(h, q, qi.data(), cell.data(), en.data(), fr.data(), dis.data(), 64, n.data()), n);      // (diagnostic already: no re-run)
    S.rough_matches = 0;
  }
  // both overflows of a batch in the form the handle gives `nq` queries: a sweep that outgrows the records (a whole re-run), candidate
  // pairs that outgrow their buffer (the list pass alone)
  void overflows(int nq) {
    sgtd_stats st;
    S.sweep_overflows = 1; S.need = 200000;
    frames(nq);
    OK(sgtd_get_stats(h, &st));
    REQUIRE(st.overflowed == 1 && S.sweep_overflows == 0);
    S.pair_overflows = 1; S.pairs_total = 2000000;
    frames(nq);
    OK(sgtd_get_stats(h, &st));
    REQUIRE(st.rewrites_total >= 1 && S.pair_overflows == 0);
    S.pairs_total = 100;
  }

  void run() {
    S.pairs_total = 100;
    const size_t peak_before = sgtd_stub_device_peak_restart();
    g_tracing = true;
    sgtd_stub_set_trace(g_transcript);
    // ---- spans on both sides of every threshold the choice of forms compares against, in the three select modes; the stand-in
    // leaves a kernel 150 KB of dynamic LDS
    const size_t room = 150 * 1024;
    uint32_t fit_votes = 1, fit_table = 1;
    while (kernels_of_the_engine::votes_topk_lds_bytes(fit_votes + 1) <= room) fit_votes++;
    while ((size_t)SGTD_PQ_TILE_RECS * sizeof(u32) + (((size_t)fit_table + 1 + 15) & ~(size_t)15) + 16 <= room) fit_table++;
    note("largest span whose vote histogram fits votes_topk_kernel: %lld; whose byte table fits pairs_query_kernel: %lld", fit_votes, fit_table);
    std::vector<uint32_t> spans = {1, 100, fit_votes, fit_votes + 1, 36 * 1024, 36 * 1024 + 1, 150 * 1024 / 4, 150 * 1024 / 4 + 1, 48 * 1024, 48 * 1024 + 1,
                                   fit_table, fit_table + 1, 8 * 36 * 1024, 8 * 36 * 1024 + 1};
    for (uint32_t span : spans)
      for (const char *mode : {"0", "1", "2"}) {
        note("---- span %lld, SGTD_SELECT_MODE %lld", span, atoi(mode));
        { Env m("SGTD_SELECT_MODE", mode); table(base, span); }
        frames(8);
        frames(span > 200000 ? 2 : 256);        // (few queries for the widest spans)
        if (span <= 100) { frames(255); frames(256, 15); }     // (256 queries of 540 slots: 1280 blocks of 128, the chunk does not halve)
        descs(700);
        done();
      }
    // ---- the compact lists' 8-byte words (SGTD_WIDE_PAIRS=1), with the slot table in LDS and with the candidates' hash
    for (uint32_t span : {48u * 1024, 48u * 1024 + 1}) {
      { Env w("SGTD_WIDE_PAIRS", "1"); table(base, span); }
      frames(8); frames(256); descs(700);
      done();
    }
    // ---- one-query batches: at most 8 192 slots and more, the general ordering chain by SGTD_SMALL_ORDER=0; the block chunk by
    // SGTD_BLOCK_CHUNK; the other per-batch knobs; sgtd_search_frame; timing on
    table(base, 100);
    descs(8192); descs(8193);
    { Env o("SGTD_SMALL_ORDER", "0"); descs(700); }
    { Env c("SGTD_BLOCK_CHUNK", "32"); frames(256, 15); descs(700); }
    { Env c("SGTD_BLOCK_CHUNK", "64"); frames(8); }
    { Env a("SGTD_HOME_SUB_BITS", "3"); Env b("SGTD_SWEEP_BLOCKS_PER_CU", "3"); Env c("SGTD_PLAN_BLOCKS_PER_CU", "2"); Env d("SGTD_REC_SLAB", "2048"); frames(8); descs(700); }
    CALL(SGTD_OK, h, sgtd_set_timing(h, 1));
    frames(8); frames(256); descs(700);
    {
      const int cn = base.candidate_num;
      std::vector<int32_t> fcf((size_t)cn), fcv((size_t)cn), fqi(4000);
      std::vector<int64_t> fpo((size_t)cn + 1), fio((size_t)cn + 1);
      std::vector<double> fsc((size_t)cn), fps((size_t)cn * 12);
      Descs ent; ent.resize(4000);
      Descs q = random_descs(rng, 700, 3);
      sgtd_desc_soa qs = q.soa();
      sgtd_frame_search io{};
      io.cand_frame = fcf.data(); io.cand_votes = fcv.data(); io.pair_off = fpo.data(); io.score = fsc.data(); io.pose = fps.data();
      io.inlier_off = fio.data(); io.inlier_q_idx = fqi.data(); io.entries = ent.soa(); io.capacity = 4000;
      S.frame_inliers = 10;
      CALL(SGTD_OK, h, sgtd_set_deferred_lists(h, 1));          // (suspended inside the call)
      CALL(SGTD_OK, h, sgtd_search_frame(h, &qs, 700, &io));
      io.flags = SGTD_FRAME_LISTS_ONLY;
      CALL(SGTD_OK, h, sgtd_search_frame(h, &qs, 700, &io));
      CALL(SGTD_OK, h, sgtd_set_deferred_lists(h, 0));
      S.frame_inliers = -1;
    }
    rough(0);
    done();
    // ---- the overflows, once in each list form and in a one-query batch (small work buffers: SGTD_REC_CAP, SGTD_PAIR_CAP)
    { Env r("SGTD_REC_CAP", "1048576"); Env c("SGTD_PAIR_CAP", "65536"); table(base, 100); }
    overflows(8); overflows(256);
    { S.sweep_overflows = 1; S.need = 10; S.reservations = true; descs(700); S.reservations = false; S.pair_overflows = 1; S.pairs_total = 2000000; descs(700); S.pairs_total = 100; }
    done();
    // ---- a key of more than 32 bits (cells of a quarter of the default: 8 bits a coordinate)
    { sgtd_config c = base; c.std_side_resolution = 0.25; table(c, 100); }
    frames(8); descs(700);
    done();
    // ---- 64 candidates; ranks of 17 bits with them (the corner that takes the block form), of 18 and of 20 bits (8-byte compact words)
    for (unsigned longest : {0u, 1u << 17, (1u << 17) + 1, (1u << 19) + 1}) {
      sgtd_config c = base; c.candidate_num = 64;
      S.longest = longest;
      { Env m("SGTD_SELECT_MODE", "2"); table(c, 100); }
      S.longest = 0;
      frames(8); descs(700);
      done();
    }
    // ---- a tail segment; a frames batch stamped outside the table's frame range; the diagnostic re-run of each
    table(base, 100, 0, /*tail=*/true);
    frames(8); rough(0); frames(256); descs(700); rough(0);
    done();
    table(base, 100, /*stamp=*/500);
    frames(8); rough(0); frames(256);
    done();
    // ---- sgtd_loop_frames: the frames join the table, each is a query bounded by its own id; its diagnostic re-run
    table(base, 100, /*stamp=*/100);
    {
      Keypoints k;
      for (int q = 0; q < 6; q++) k.add(rng, 14);
      CALL(SGTD_OK, h, sgtd_loop_frames(h, k.xyz.data(), k.label.data(), k.off.data(), 6, 2, 0));
      CALL(SGTD_OK, h, sgtd_sync(h));
      rough(0);
    }
    done();
    // ---- deferred lists (one workgroup per query): finished with a mask, with none, by a plain sgtd_sync; with timing; on a batch
    // in the block form (nothing to finish); a registered candidate-export buffer beside them
    {
      { Env m("SGTD_SELECT_MODE", "0"); table(base, 100); }
      void *keep = nullptr, *packed = nullptr;
      REQUIRE(hipMalloc(&keep, 256 * sizeof(u64)) == hipSuccess && hipMalloc(&packed, (size_t)(1 << 16) * sizeof(int)) == hipSuccess);
      memset(keep, 0x55, 256 * sizeof(u64));
      CALL(SGTD_OK, h, sgtd_set_candidate_export(h, static_cast<int32_t *>(packed), 1 << 16));
      CALL(SGTD_OK, h, sgtd_set_deferred_lists(h, 1));
      for (int timing : {0, 1}) {
        CALL(SGTD_OK, h, sgtd_set_timing(h, timing));
        frames(256, 14, false);
        CALL(SGTD_OK, h, sgtd_finish_lists(h, static_cast<const uint64_t *>(keep)));
        CALL(SGTD_OK, h, sgtd_sync(h));
        if (!timing) {      // (the re-run of a masked list pass: the same mask)
          S.pair_overflows = 1; S.pairs_total = 2000000;
          CALL(SGTD_OK, h, sgtd_finish_lists(h, static_cast<const uint64_t *>(keep)));
          CALL(SGTD_OK, h, sgtd_sync(h));
          S.pairs_total = 100;
        }
        frames(256, 14, false);
        CALL(SGTD_OK, h, sgtd_finish_lists(h, nullptr));
        CALL(SGTD_OK, h, sgtd_sync(h));
        frames(256, 14, false);
        CALL(SGTD_OK, h, sgtd_sync(h));       // (finds the lists pending)
        frames(8, 14, false);
        CALL(SGTD_OK, h, sgtd_finish_lists(h, static_cast<const uint64_t *>(keep)));
        CALL(SGTD_OK, h, sgtd_sync(h));
      }
      {     // a registered buffer too small for the batch's tables
        CALL(SGTD_OK, h, sgtd_set_candidate_export(h, static_cast<int32_t *>(packed), 1024));
        Keypoints k;
        for (int q = 0; q < 256; q++) k.add(rng, 14);
        CALL(SGTD_ERR_CAPACITY, h, sgtd_query_frames(h, k.xyz.data(), k.label.data(), k.off.data(), 256, 0));
      }
      done();
      REQUIRE(hipFree(keep) == hipSuccess && hipFree(packed) == hipSuccess);
    }
    // ---- a frame filter (one row, a row per query) and a position prior over stored poses (alone, and with the filter), in both
    // list forms and in the diagnostic re-run; then a span whose filter rows do not fit the filter kernels' LDS
    for (uint32_t span : {100u, 600000u}) {
      table(base, span);
      const uint32_t words = (span + 63) / 64;
      const int many = span == 100 ? 256 : 2;
      std::vector<uint64_t> rows((size_t)words * many, 0x0F0F0F0F0F0F0F0Full);
      std::vector<uint32_t> ids = {0, span - 1};
      std::vector<float> poses(24, 0.f);
      poses[0] = poses[5] = poses[10] = poses[12] = poses[17] = poses[22] = 1.f; poses[3] = 4.f; poses[15] = 90.f;
      const double center[3] = {0.0, 0.0, 0.0}, radius[1] = {10.0};
      std::vector<double> centers((size_t)many * 3, 1.0), radii((size_t)many, 20.0);
      CALL(SGTD_OK, h, sgtd_set_frame_filter(h, 0, span, rows.data(), 1));
      frames(8); frames(many); frames(many);      // (the second batch of the same filter reuses its rows)
      descs(700); rough(0);
      CALL(SGTD_OK, h, sgtd_set_frame_filter(h, 0, span, rows.data(), many));
      frames(many);
      CALL(SGTD_OK, h, sgtd_set_frame_poses(h, ids.data(), poses.data(), 2));
      CALL(SGTD_OK, h, sgtd_set_position_prior(h, centers.data(), radii.data(), many, 3));
      frames(many);
      CALL(SGTD_OK, h, sgtd_set_frame_filter(h, 0, 0, nullptr, 0));
      CALL(SGTD_OK, h, sgtd_set_position_prior(h, center, radius, 1, 2));
      frames(8); frames(many); descs(700); rough(0);
      done();
    }
    sgtd_stub_set_trace(nullptr);
    g_tracing = false;
    const size_t peak = sgtd_stub_device_peak_restart();
    printf("select forms: %zu kernel forms launched, device peak %.1f MB (before: %.1f MB)\n", g_launched.size(), peak / 1048576.0, peak_before / 1048576.0);
    REQUIRE(peak < ((size_t)2 << 30));
    // ---- coverage, from the trace itself: every kernel instantiation these functions can launch was launched.  Not reached: the three
    // probe_sorted_kernel forms with 64-bit probe offsets outside the diagnostic build — they need a probe layout of 4 GB, 268 M entries.
    auto forms = [&](const char *kernel) { int n = 0; for (const std::string &k : g_launched) n += strstr(k.c_str(), kernel) != nullptr; return n; };
    const struct { const char *kernel; int forms; } want[] = {
        {"thr2_kernel", 1}, {"small_order_kernel", 1}, {"query_prefix_kernel", 1}, {"home_keys_kernel", 2}, {"group_heads_kernel", 2}, {"group_first_kernel", 1},
        {"pass_slots_kernel", 1}, {"group_resolve_kernel", 1}, {"plan_passes_kernel", 4}, {"probe_sorted_kernel", 5}, {"resolve_undecided_kernel", 1},
        {"filter_records_kernel", 2}, {"filter_compact_kernel", 2}, {"prior_rows_kernel", 1}, {"votes_topk_kernel", 1}, {"votes_query_kernel", 1}, {"votes_kernel", 2},
        {"topk_kernel", 2 /* votes_topk_kernel too */}, {"export_candidates_kernel", 1}, {"cand_prefix_kernel", 1}, {"cand_prefix_masked_kernel", 1}, {"query_base_kernel", 1},
        {"pairs_query_kernel", 2}, {"block_count_kernel", 4}, {"block_scan_kernel", 1}, {"block_write_kernel", 2}, {"batch_totals_kernel", 1}, {"loop_bound_kernel", 1},
        {"rough_gather_kernel", 1}};
    for (const auto &w : want)
      if (forms(w.kernel) != w.forms) { fprintf(stderr, "engine_driver: %d forms of %s launched, not %d\n", forms(w.kernel), w.kernel, w.forms); exit(1); }
  }
};
}  // namespace

int main(int argc, char **argv) {
  const int frames = argc > 1 ? atoi(argv[1]) : 40;
  const std::string dir = argc > 2 ? argv[2] : "/tmp";
  if (argc > 3) { g_transcript = fopen(argv[3], "w"); REQUIRE(g_transcript); }     // (one line per call of the stages' scenario)
  std::mt19937 rng(20261003);
  Scenario S;
  sgtd_stub_set_launch_hook(hook, &S);
  sgtd_config cfg;
  sgtd_default_config(&cfg);
  S.cand_num = cfg.candidate_num;
  const int cn = cfg.candidate_num;

  // ---- a table from host descriptors, frame by frame; finalize; appends into a tail; more appends until the tail is merged
  sgtd_handle h = nullptr;
  OK(sgtd_create(&cfg, &h));
  g_last = h;
  for (int f = 0; f < frames; f++) {
    Descs d = random_descs(rng, 300 + rng() % 500, (uint32_t)f);
    sgtd_desc_soa s = d.soa();
    OK(sgtd_add(h, &s, (int64_t)d.frame.size()));
  }
  OK(sgtd_finalize(h));
  OK(sgtd_finalize(h));       // idempotent
  sgtd_stats st;
  OK(sgtd_get_stats(h, &st));
  REQUIRE(st.n_frames == frames && st.n_entries > 0);
  for (int f = frames; f < frames + 3; f++) {
    Descs d = random_descs(rng, 200, (uint32_t)f);
    sgtd_desc_soa s = d.soa();
    OK(sgtd_add(h, &s, 200));
    OK(sgtd_finalize(h));
  }
  OK(sgtd_get_stats(h, &st));
  REQUIRE(st.tail_entries > 0);

  // ---- batches of host descriptors: a clean one; one whose sweep outgrows the record buffer twice (re-runs, growth); one whose
  // reservations outran the buffer (the rate drops); one whose candidate pairs outgrow theirs (the list pass alone is re-run)
  Descs q = random_descs(rng, 700, (uint32_t)(frames + 3));
  sgtd_desc_soa qs = q.soa();
  std::vector<int32_t> n_cand(1), cf((size_t)cn), cv((size_t)cn);
  std::vector<int64_t> po((size_t)cn + 1);
  S.pairs_total = 5000;
  OK(sgtd_query_descs(h, &qs, 700));
  OK(sgtd_result_candidates(h, n_cand.data(), cf.data(), cv.data(), po.data()));
  S.sweep_overflows = 2; S.need = 3000000;
  OK(sgtd_query_descs(h, &qs, 700));
  OK(sgtd_sync(h));
  OK(sgtd_get_stats(h, &st));
  REQUIRE(st.overflowed == 1 && st.reruns_total >= 2 && S.sweep_overflows == 0);
  S.sweep_overflows = 1; S.need = 10; S.reservations = true;
  OK(sgtd_query_descs(h, &qs, 700));
  OK(sgtd_sync(h));
  S.reservations = false;
  S.pair_overflows = 1; S.pairs_total = 40000000;
  OK(sgtd_query_descs(h, &qs, 700));
  OK(sgtd_sync(h));
  OK(sgtd_get_stats(h, &st));
  REQUIRE(st.rewrites_total >= 1);
  // the verification and what follows it, on the batch's (stand-in) 4e7 pairs
  OK(sgtd_verify(h));
  std::vector<double> score((size_t)cn), pose((size_t)cn * 12);
  OK(sgtd_result_verify(h, 0, score.data(), pose.data()));
  int32_t bc = 0, bf = 0;
  double bs = 0;
  OK(sgtd_search_loop(h, 0.4, &bc, &bf, &bs));
  {
    std::vector<int64_t> off((size_t)cn + 1);
    std::vector<int32_t> qi(64);
    Descs ent; ent.resize(64);
    sgtd_desc_soa es = ent.soa();
    int64_t n_pairs = -1;
    OK(sgtd_result_inlier_entries(h, 0, off.data(), qi.data(), &es, 64, &n_pairs));
    REQUIRE(n_pairs == 0);
    std::vector<int32_t> pq(16); std::vector<int64_t> pe(16);
    int64_t np = 0;
    const int stp = sgtd_result_pairs(h, 0, pq.data(), pe.data(), 16, &np);
    REQUIRE(stp == SGTD_OK || stp == SGTD_ERR_CAPACITY);
  }
  // the hooks that shrink the work buffers (first batches overflow for real in the tests): honoured by a fresh handle
  S.pairs_total = 100;

  // ---- sgtd_search_frame: the one-wait path, too little room for the inlier pairs, more inlier pairs than the gather's first room
  // (the gather is enqueued again with room), a frame whose batch outgrew a work buffer (falls back to the separate calls)
  {
    std::vector<int32_t> fcf((size_t)cn), fcv((size_t)cn), fqi(40000);
    std::vector<int64_t> fpo((size_t)cn + 1), fio((size_t)cn + 1);
    std::vector<double> fsc((size_t)cn), fps((size_t)cn * 12);
    Descs ent; ent.resize(40000);
    sgtd_frame_search io{};
    io.cand_frame = fcf.data(); io.cand_votes = fcv.data(); io.pair_off = fpo.data(); io.score = fsc.data(); io.pose = fps.data();
    io.inlier_off = fio.data(); io.inlier_q_idx = fqi.data(); io.entries = ent.soa();
    S.frame_inliers = 0; io.capacity = 40000;
    OK(sgtd_search_frame(h, &qs, 700, &io));
    REQUIRE(io.n_inliers == 0 && io.n_cand == 1);
    S.frame_inliers = 100; io.capacity = 10;
    REQUIRE(sgtd_search_frame(h, &qs, 700, &io) == SGTD_ERR_CAPACITY && io.n_inliers == 100);
    io.capacity = 40000;
    OK(sgtd_search_frame(h, &qs, 700, &io));
    REQUIRE(io.n_inliers == 100);
    S.frame_inliers = 30000;                     // beyond the gather's first room of 16 384
    OK(sgtd_search_frame(h, &qs, 700, &io));
    REQUIRE(io.n_inliers == 30000);
    S.frame_inliers = 5; S.frame_overflow = 1;
    OK(sgtd_search_frame(h, &qs, 700, &io));
    S.frame_inliers = -1;
    OK(sgtd_get_stats(h, &st));
    REQUIRE(st.batches_total >= 0);
    // the caller's arrays page-locked (sgtd_host_alloc): the gather is handed them as they are — each must hold `capacity` entries.
    // One array shorter than that (the caller's mistake would be a kernel writing past it): the engine must see it and take its own block
    g_gathers_into.clear();
    void *pl[8];
    const size_t room = 2000, widths[8] = {24, 24, 24, 36, 12, 4, 12, 4};
    for (int k = 0; k < 8; k++) OK(sgtd_host_alloc(room * widths[k], &pl[k]));
    sgtd_frame_search d = io;
    d.entries = sgtd_desc_soa{(double *)pl[0], (double *)pl[1], (double *)pl[2], (float *)pl[3], (int32_t *)pl[4], (uint32_t *)pl[5], (int32_t *)pl[6]};
    d.inlier_q_idx = (int32_t *)pl[7];
    d.capacity = (int64_t)room; S.frame_inliers = 100;
    OK(sgtd_search_frame(h, &qs, 700, &d));
    REQUIRE(d.n_inliers == 100 && !g_gathers_into.empty() && g_gathers_into.back() == pl[0]);
    d.capacity = (int64_t)room + 1;             // one more than the arrays hold
    OK(sgtd_search_frame(h, &qs, 700, &d));
    REQUIRE(g_gathers_into.back() != pl[0]);
    d.capacity = (int64_t)room; d.entries.vertex = ent.vertex.data();       // one ordinary array among them
    OK(sgtd_search_frame(h, &qs, 700, &d));
    REQUIRE(g_gathers_into.back() != pl[0]);
    // candidate_selector alone in the one call (SGTD_FRAME_LISTS_ONLY): no verification is enqueued, the pairs are the lists' own; its
    // three ways out (one wait, too little room, the fall-back after an overflow) with page-locked and with ordinary arrays
    d.entries.vertex = (float *)pl[3];
    d.flags = SGTD_FRAME_LISTS_ONLY; d.capacity = (int64_t)room; S.frame_inliers = 100;
    OK(sgtd_search_frame(h, &qs, 700, &d));
    REQUIRE(d.n_inliers == 100 && g_gathers_into.back() == pl[0]);
    d.capacity = 10;
    REQUIRE(sgtd_search_frame(h, &qs, 700, &d) == SGTD_ERR_CAPACITY && d.n_inliers == 100);
    d.capacity = (int64_t)room; S.frame_overflow = 1;
    OK(sgtd_search_frame(h, &qs, 700, &d));
    io.flags = SGTD_FRAME_LISTS_ONLY; io.capacity = 40000; S.frame_inliers = 30000;
    OK(sgtd_search_frame(h, &qs, 700, &io));
    REQUIRE(io.n_inliers == 30000);
    io.flags = 0;
    S.frame_inliers = -1;
    for (int k = 0; k < 8; k++) OK(sgtd_host_free(pl[k]));
  }

  // ---- views: a second handle on the same table; its pending batch after the owner's table changed; destroy order
  sgtd_handle v = nullptr;
  OK(sgtd_create(&cfg, &v));
  OK(sgtd_attach_table(v, h));
  OK(sgtd_query_descs(v, &qs, 700));
  OK(sgtd_sync(v));
  OK(sgtd_query_descs(v, &qs, 700));          // pending ...
  {
    Descs d = random_descs(rng, 150, (uint32_t)(frames + 4));
    sgtd_desc_soa s = d.soa();
    OK(sgtd_add(h, &s, 150));                 // ... while the owner's table changes (its buffers are reallocated)
    OK(sgtd_finalize(h));
  }
  REQUIRE(sgtd_verify(v) == SGTD_ERR_STATE);
  REQUIRE(sgtd_query_descs(v, &qs, 700) == SGTD_ERR_STATE);
  { int64_t e0[4] = {0, 1, 2, 3}; Descs o4; o4.resize(4); sgtd_desc_soa os = o4.soa(); REQUIRE(sgtd_fetch_entries(v, e0, 4, &os) == SGTD_ERR_STATE); }
  REQUIRE(sgtd_destroy(h) == SGTD_ERR_STATE);  // a view is still attached
  OK(sgtd_attach_table(v, h));
  OK(sgtd_query_descs(v, &qs, 700));
  OK(sgtd_verify(v));
  { Descs d = random_descs(rng, 10, 0); sgtd_desc_soa s = d.soa(); REQUIRE(sgtd_add(v, &s, 10) == SGTD_ERR_STATE); }
  // the owner's own batches on a tail: the fifth merges the tail (a rebuild) — the view must notice
  for (int b = 0; b < 6; b++) { OK(sgtd_query_descs(h, &qs, 700)); OK(sgtd_sync(h)); }
  OK(sgtd_get_stats(h, &st));
  REQUIRE(st.tail_entries == 0);
  REQUIRE(sgtd_query_descs(v, &qs, 700) == SGTD_ERR_STATE);
  OK(sgtd_destroy(v));

  // ---- the table file: save, load into a fresh handle (header checks, sizes), append, query; damaged files refuse
  const std::string path = dir + "/engine_driver_table.bin";
  OK(sgtd_save_table(h, path.c_str()));
  sgtd_handle l = nullptr;
  OK(sgtd_create(&cfg, &l));
  OK(sgtd_load_table(l, path.c_str()));
  sgtd_stats sl;
  OK(sgtd_get_stats(l, &sl));
  OK(sgtd_get_stats(h, &st));
  REQUIRE(sl.n_entries == st.n_entries && sl.n_frames == st.n_frames);
  { Descs d = random_descs(rng, 120, (uint32_t)(frames + 5)); sgtd_desc_soa s = d.soa(); OK(sgtd_add(l, &s, 120)); }
  OK(sgtd_query_descs(l, &qs, 700));
  OK(sgtd_sync(l));
  {
    FILE *f = fopen(path.c_str(), "rb");
    REQUIRE(f);
    std::vector<unsigned char> bytes;
    unsigned char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + got);
    fclose(f);
    const std::string cut = dir + "/engine_driver_table_cut.bin";
    for (size_t keep : {(size_t)0, (size_t)7, (size_t)60, bytes.size() / 2, bytes.size() - 1}) {
      f = fopen(cut.c_str(), "wb"); REQUIRE(f);
      fwrite(bytes.data(), 1, keep, f); fclose(f);
      sgtd_handle t = nullptr;
      OK(sgtd_create(&cfg, &t));
      REQUIRE(sgtd_load_table(t, cut.c_str()) != SGTD_OK);
      OK(sgtd_destroy(t));
    }
    remove(cut.c_str());
  }
  OK(sgtd_destroy(l));
  remove(path.c_str());

  // ---- two "devices" behind one handle (both shards on the stand-in's device 0): add, finalize, a batch, the verification
  {
    const int ids[2] = {0, 0};
    sgtd_handle m = nullptr;
    OK(sgtd_create_multi(&cfg, ids, 2, &m));
    REQUIRE(sgtd_device_count(m) == 2);
    for (int f = 0; f < 12; f++) { Descs d = random_descs(rng, 250, (uint32_t)f); sgtd_desc_soa s = d.soa(); OK(sgtd_add(m, &s, 250)); }
    OK(sgtd_finalize(m));
    OK(sgtd_query_descs(m, &qs, 700));
    OK(sgtd_result_candidates(m, n_cand.data(), cf.data(), cv.data(), po.data()));
    OK(sgtd_verify(m));
    OK(sgtd_result_verify(m, 0, score.data(), pose.data()));
    OK(sgtd_destroy(m));
  }

  OK(sgtd_destroy(h));

  // ---- the stages on a verified batch, on one device and on two "devices" behind one handle
  for (int n_dev : {1, 2}) { Stages st; st.run(S, cfg, rng, n_dev); }

  // ---- the forms of the query pipeline, launch by launch
  { SelectForms sf{S, rng, cfg}; sf.run(); }
  g_last = nullptr;
  if (g_transcript) fclose(g_transcript);
  REQUIRE(sgtd_stub_device_blocks() == 0 && sgtd_stub_device_bytes() == 0);       // every device buffer was freed
  printf("engine host code under the sanitizers: ok (%llu launches, %llu sweeps, %llu frame packs, device peak %.1f MB)\n",
         sgtd_stub_launches(), S.sweeps, S.packs, sgtd_stub_device_peak() / 1048576.0);
  return 0;
}
