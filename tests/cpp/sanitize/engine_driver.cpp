// engine_driver.cpp — the engine's host code (sgtd_accel.hip, multi_impl.hip.h) under ASan + UBSan, against hip_stub.cpp.
// No kernel runs: "device" buffers are zeroed host memory and the launch hook below leaves behind what selected kernels
// would have — overflow flags, record needs, pair totals, a frame's packed results — so that the host walks its growth,
// re-run, stale-view, capacity and table-file paths with every copy checked by the sanitizer.  The stages on a verified batch
// (sgtd_refine_poses, sgtd_overlap, sgtd_align_keypoints) run in a scenario of their own below, whose stand-in results name the
// (query, candidate) slot they belong to.  The forms of the query pipeline (launch_select's plan and stages, the list pass run
// again, deferred lists, the diagnostic re-run) run in a third scenario with the stand-in's trace on: every launch, memset,
// attribute and event record is a line of the transcript.  The stages that belong to no batch (sgtd_register_clouds,
// sgtd_register_voxels, sgtd_scan_keypoints, sgtd_local_map_keypoints, sgtd_consistent_loops, sgtd_relax_poses, sgtd_pose_consensus)
// and every getter of theirs run in a fourth, traced like the third, on one device and on two.  Compiled for the host only
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
#include "../../../sgtd_amd/csrc/consistency_kernels.hip.h"
#include "../../../sgtd_amd/csrc/relax_kernels.hip.h"
#include "../../../sgtd_amd/csrc/register_kernels.hip.h"
#include "../../../sgtd_amd/csrc/voxel_register_kernels.hip.h"
#include "../../../sgtd_amd/csrc/consensus_kernels.hip.h"
#include "../../../sgtd_amd/csrc/scan_kernels.hip.h"
#include "../../../sgtd_amd/csrc/local_map_kernels.hip.h"
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
  // the cloud and graph stages' scenario
  long long solve_rounds = 0;       // reg_trial_kernel / vreg_trial_kernel: the launch of a call that leaves no pair unfinished (0: none does)
  long long trials = 0;             // ... launches since the call's reg_init_kernel / vreg_init_kernel
  size_t cloud_floats = 0;          // floats of the call's points (reg_cov_kernel checks the array it is handed)
  std::vector<u32> map_voxels;      // vreg_ranges_kernel: voxels of each map (their sum: what scan_voxels_kernel leaves as the run's count)
  unsigned voxels = 0;              // scan_voxels_kernel: the voxels of a scan pipeline's run
  long long kept = 0;               // scan_offsets_kernel: keypoints the run keeps, spread over its scans
  bool relax_ends = true;           // relax_ctl_kernel: an accepted step ends the solve
};
bool g_tracing = false;             // the select-forms scenario: every launch adds its scalars to the transcript (trace_args)
void trace_args(const char *name, void **args);

// bytes from p to the end of the block it lies in; none where p is the end of a block (an empty array may start there).  Any other
// pointer is a stray one
size_t room_of(const void *p) {
  hipDeviceptr_t base; size_t size;
  if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) != hipSuccess) {
    const char *before = static_cast<const char *>(p) - 1;
    REQUIRE(p && hipMemGetAddressRange(&base, &size, const_cast<char *>(before)) == hipSuccess && static_cast<const char *>(base) + size == p);
    return 0;
  }
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

// `kernel` is the function the (mangled) name names: reg_init_kernel is not vreg_init_kernel
bool names(const char *name, const char *kernel) {
  const char *at = strstr(name, kernel);
  return at && at > name && at[-1] >= '0' && at[-1] <= '9';
}

// ---- the cloud and graph stages (sgtd_register_clouds, sgtd_register_voxels, sgtd_scan_keypoints, sgtd_local_map_keypoints,
// sgtd_consistent_loops, sgtd_relax_poses, sgtd_pose_consensus): the few words the host reads back, the room of what a launch is handed
void reg_room(const kernels_of_the_engine::RegParams &P, bool dense) {
  const size_t n = (size_t)P.n_pairs, ts = (size_t)P.total_src;
  REQUIRE(room_of(P.src) >= n * 4 && room_of(P.src_off) >= (n + 1) * 4 && room_of(P.unfinished) >= 4);
  REQUIRE(room_of(P.tile_pair) >= (size_t)P.n_tiles * 4 && room_of(P.tile_first) >= (size_t)P.n_tiles * 4);
  REQUIRE(room_of(P.ctile_cloud) >= (size_t)P.n_ctiles * 4 && room_of(P.ctile_first) >= (size_t)P.n_ctiles * 4);
  REQUIRE(room_of(P.st) >= std::max<size_t>(n, 1) * sizeof(kernels_of_the_engine::RegState));
  REQUIRE(room_of(P.out_pose) >= n * 12 * 8 && room_of(P.out_fitness) >= n * 8 && room_of(P.out_cost) >= n * 16);
  REQUIRE(room_of(P.out_matched) >= n * 4 && room_of(P.out_iters) >= n * 4 && room_of(P.out_status) >= n * 4);
  if (dense) REQUIRE(room_of(P.tgt) >= n * 4 && room_of(P.md2) >= ts * 8 && room_of(P.M) >= ts * 72 && room_of(P.mj) >= ts * 4 && room_of(P.part_d2) >= ts * 8 && room_of(P.part_j) >= ts * 4);
}
void vreg_room(const kernels_of_the_engine::RegParams &P, const kernels_of_the_engine::VregParams &V) {
  const size_t n = (size_t)P.n_pairs, ts = (size_t)P.total_src, nm = (size_t)V.n_members;
  REQUIRE(room_of(V.tgt_map) >= n * 4 && room_of(V.map_off) >= (V.n_maps ? (size_t)V.n_maps + 1 : 0) * 4 && room_of(V.map_cloud) >= nm * 4);
  REQUIRE(room_of(V.mem_map) >= nm * 4 && room_of(V.mem_pt_off) >= (nm + 1) * 4 && room_of(V.map_vox) >= ((size_t)V.n_maps + 1) * 4);
  REQUIRE(room_of(V.vid) >= ts * (size_t)V.mode * 4 && room_of(V.Mw) >= ts * (size_t)V.mode * 72 && room_of(V.out_corr) >= n * 4);
  if (V.map_pose) REQUIRE(room_of(V.map_pose) >= nm * 96);
  if (V.n_vox) REQUIRE(room_of(V.vkey) >= (size_t)V.n_vox * 8 && room_of(V.vstart) >= ((size_t)V.n_vox + 1) * 4 && room_of(V.vmean) >= (size_t)V.n_vox * 24 && room_of(V.vcov) >= (size_t)V.n_vox * 72);
}
bool cloud_hook(Scenario &S, const char *name, void **args) {
  namespace K = kernels_of_the_engine;
  if (names(name, "reg_cov_kernel")) {
    const K::RegParams &P = *static_cast<const K::RegParams *>(args[0]);
    REQUIRE(P.n_ctiles > 0 && sgtd_stub_grid_x() == (unsigned)P.n_ctiles && room_of(P.pts) >= S.cloud_floats * 4 && room_of(P.cov) >= S.cloud_floats / (size_t)P.stride * 72);
  } else if (names(name, "reg_init_kernel") || names(name, "vreg_init_kernel")) {
    const K::RegParams &P = *static_cast<const K::RegParams *>(args[0]);
    const bool dense = names(name, "reg_init_kernel");
    reg_room(P, dense);
    if (!dense) vreg_room(P, *static_cast<const K::VregParams *>(args[1]));
    const double *init = *static_cast<const double **>(args[dense ? 1 : 2]);
    if (init) REQUIRE(room_of(init) >= (size_t)P.n_pairs * 96);
    S.trials = 0;
  } else if (names(name, "reg_trial_kernel") || names(name, "vreg_trial_kernel")) {
    const K::RegParams &P = *static_cast<const K::RegParams *>(args[0]);
    REQUIRE(sgtd_stub_grid_x() == (unsigned)P.n_pairs);
    if (++S.trials == S.solve_rounds) *P.unfinished = 0;
  } else if (names(name, "reg_final_kernel") || names(name, "vreg_final_kernel")) {
    // the result rows name their pair
    const K::RegParams &P = *static_cast<const K::RegParams *>(args[0]);
    for (int k = 0; k < P.n_pairs; k++) {
      for (int i = 0; i < 12; i++) P.out_pose[(size_t)k * 12 + i] = (double)k + (double)i / 16.0;
      P.out_fitness[k] = 0.5 * k; P.out_cost[2 * k] = 2.0 * k; P.out_cost[2 * k + 1] = 1.0 * k;
      P.out_matched[k] = 3 * k; P.out_iters[k] = (int)S.trials; P.out_status[k] = k % 5;
      if (names(name, "vreg_final_kernel")) static_cast<const K::VregParams *>(args[1])->out_corr[k] = 7 * k;
    }
  } else if (names(name, "vreg_ranges_kernel")) {
    const K::VregParams &V = *static_cast<const K::VregParams *>(args[0]);
    REQUIRE(room_of(V.map_vox) >= ((size_t)V.n_maps + 1) * 4);
    V.map_vox[0] = 0;
    for (int m = 0; m < V.n_maps; m++) V.map_vox[m + 1] = V.map_vox[m] + (V.n_vox ? S.map_voxels[(size_t)m] : 0u);
    REQUIRE(V.map_vox[V.n_maps] == V.n_vox);
  } else if (names(name, "scan_heads_kernel")) {
    const long long n = *static_cast<long long *>(args[1]);
    REQUIRE(room_of(*static_cast<void **>(args[0])) >= (size_t)n * 8 && room_of(*static_cast<void **>(args[3])) >= ((size_t)n + 1) * 4 && room_of(*static_cast<void **>(args[4])) >= 16);
  } else if (names(name, "scan_voxels_kernel")) {
    // the count of runs is the scan's last word
    u32 *excl = *static_cast<u32 **>(args[2]);
    const long long n = *static_cast<long long *>(args[3]);
    REQUIRE(room_of(excl) >= ((size_t)n + 1) * 4 && room_of(*static_cast<void **>(args[5])) >= (size_t)n * 8 && room_of(*static_cast<void **>(args[6])) >= ((size_t)n + 1) * 4);
    excl[n] = (u32)std::min<long long>(S.voxels, n);
  } else if (names(name, "scan_point_kernel")) {
    const K::ScanPointParams &P = *static_cast<const K::ScanPointParams *>(args[0]);
    const size_t n = (size_t)P.n;
    REQUIRE(room_of(P.pts) >= n * (size_t)P.stride * 4 && room_of(P.labels) >= n * 4 && room_of(P.sc_of) >= n * 4 && room_of(P.r) >= n * 8 && room_of(P.pitch) >= n * 8 && room_of(P.azimuth) >= n * 8);
  } else if (names(name, "scan_jump_kernel")) {
    REQUIRE(room_of(*static_cast<u32 **>(args[2])) >= ((size_t)*static_cast<int *>(args[3]) + 1) * 4);      // (changed[round] stays zero: settled)
  } else if (names(name, "scan_offsets_kernel")) {
    const int n_scans = *static_cast<int *>(args[2]);
    long long *kp_off = *static_cast<long long **>(args[3]);
    REQUIRE(room_of(kp_off) >= ((size_t)n_scans + 1) * 8);
    for (int s = 0; s <= n_scans; s++) kp_off[s] = S.kept * s / n_scans;
  } else if (names(name, "scan_sum_wave_kernel")) {
    const u32 n_kept = *static_cast<u32 *>(args[5]);
    float *xyz = *static_cast<float **>(args[6]);
    REQUIRE(room_of(xyz) >= (size_t)n_kept * 12);
    for (u32 i = 0; i < n_kept * 3; i++) xyz[i] = (float)i / 4.f;
  } else if (names(name, "lm_members_kernel")) {
    // an anchor's members: its scan and, for every other anchor, the next one
    const long long *pt_off = *static_cast<const long long **>(args[1]), *mem_off = *static_cast<const long long **>(args[6]);
    const int n_scans = *static_cast<int *>(args[2]), A = (int)sgtd_stub_grid_x();
    const int *anchors = *static_cast<const int **>(args[3]);
    int *member = *static_cast<int **>(args[7]), *count = *static_cast<int **>(args[8]);
    long long *merged = *static_cast<long long **>(args[9]);
    REQUIRE(room_of(pt_off) >= ((size_t)n_scans + 1) * 8 && room_of(anchors) >= (size_t)A * 4 && room_of(count) >= (size_t)A * 4 && room_of(merged) >= (size_t)A * 8);
    REQUIRE(room_of(*static_cast<void **>(args[0])) >= (size_t)n_scans * 48);
    if (mem_off) REQUIRE(room_of(mem_off) >= ((size_t)A + 1) * 8 && room_of(member) >= (size_t)mem_off[A] * 4);
    for (int a = 0; a < A; a++) {
      const int s = anchors[a], t = (s + 1) % n_scans, c = a % 2 == 1 && t != s ? 2 : 1;
      count[a] = c;
      merged[a] = (pt_off[s + 1] - pt_off[s]) + (c == 2 ? pt_off[t + 1] - pt_off[t] : 0);
      if (mem_off) { member[mem_off[a]] = s; if (c == 2) member[mem_off[a] + 1] = t; }
    }
  } else if (names(name, "lm_gather_kernel")) {
    const int n_seg = *static_cast<int *>(args[4]);
    const u32 Pp = *static_cast<u32 *>(args[5]);
    REQUIRE(room_of(*static_cast<void **>(args[2])) >= (size_t)n_seg * sizeof(K::LmSeg) && room_of(*static_cast<void **>(args[3])) >= ((size_t)n_seg + 1) * 4);
    REQUIRE(room_of(*static_cast<void **>(args[6])) >= (size_t)Pp * 12 && room_of(*static_cast<void **>(args[7])) >= (size_t)Pp * 4);
  } else if (names(name, "cons_pair_kernel")) {
    const K::ConsPairParams &P = *static_cast<const K::ConsPairParams *>(args[0]);
    REQUIRE(room_of(P.soa) >= (size_t)SGTD_CONS_STREAMS * P.ns * 8 && room_of(P.valid) >= P.ns && room_of(P.rows) >= (size_t)P.n * P.words * 8);
    for (size_t i = 0; i < (size_t)P.n * P.words; i++) P.rows[i] = 0x0101010101010101ull * (i % 251);
  } else if (names(name, "cons_select_kernel")) {
    // the first round completes the choice
    int *in_set = *static_cast<int **>(args[3]);
    K::ConsState *st = *static_cast<K::ConsState **>(args[5]);
    REQUIRE(room_of(st) >= sizeof(K::ConsState) && room_of(in_set) >= 12);
    st->done = 1; st->n_set = 1; st->round = 1;
    in_set[0] = 1;
  } else if (names(name, "consensus_kernel")) {
    const K::ConsensusParams &P = *static_cast<const K::ConsensusParams *>(args[0]);
    const size_t nq = sgtd_stub_grid_x(), cn = (size_t)P.cn;
    REQUIRE(room_of(P.n_cand) >= nq * 4 && room_of(P.cand_frame) >= nq * cn * 4 && room_of(P.score) >= nq * cn * 8 && room_of(P.rel) >= nq * cn * 96);
    REQUIRE(room_of(P.pose) >= nq * 96 && room_of(P.figs) >= nq * 24 && room_of(P.mask) >= nq * 8 && room_of(P.counts) >= nq * 12);
    REQUIRE(room_of(P.rows) >= nq * cn * 8 && room_of(P.degree) >= nq * cn * 4 && room_of(P.pick) >= nq * cn * 4);
    REQUIRE(room_of(P.store) >= std::max<size_t>(P.n_ids, 1) * 48 && room_of(P.has) >= std::max<size_t>(P.n_ids, 1));
    // every query's set: its first two candidates (its first, of one)
    for (size_t q = 0; q < nq; q++) {
      const int set = std::min(P.n_cand[q], 2);
      P.mask[q] = set == 2 ? 3u : (u64)set;
      P.counts[q * 3] = P.n_cand[q]; P.counts[q * 3 + 1] = set; P.counts[q * 3 + 2] = set ? 0 : -1;
      for (int i = 0; i < 3; i++) P.figs[q * 3 + i] = (double)q + 0.25 * i;
      for (int i = 0; i < 12; i++) P.pose[q * 12 + i] = set ? P.rel[q * cn * 12 + i] : kNaN;
      for (size_t k = 0; k < cn; k++) { P.rows[q * cn + k] = P.mask[q]; P.degree[q * cn + k] = (int)k; P.pick[q * cn + k] = k < (size_t)set ? (int)k : -1; }
    }
  } else if (names(name, "relax_init_kernel")) {
    const K::RelaxParams &P = *static_cast<const K::RelaxParams *>(args[0]);
    const size_t n = (size_t)P.n, m = (size_t)P.m;
    REQUIRE(room_of(P.state) >= 2 * n * SGTD_RELAX_REC * 8 && room_of(P.held) >= n && room_of(P.ok) >= n && room_of(P.ei) >= m * 4 && room_of(P.ej) >= m * 4);
    REQUIRE(room_of(P.wt) >= 2 * m * 8 && room_of(P.iz) >= 45 * P.ms * 8 + 5 * m * 8 && room_of(P.ec) >= 4 * m * 8 && room_of(P.off) >= (n + 1 + 2 * m) * 4);
    REQUIRE(room_of(P.r) >= n * 102 * 8 + n && room_of(P.st) >= sizeof(K::RelaxState));
    REQUIRE(room_of(*static_cast<void **>(args[1])) >= n * 96 && room_of(*static_cast<void **>(args[2])) >= m * 96);
    for (size_t i = 0; i < 2 * n * SGTD_RELAX_REC; i++) P.state[i] = (double)i / 8.0;
  } else if (names(name, "relax_ctl_kernel")) {
    const K::RelaxParams &P = *static_cast<const K::RelaxParams *>(args[0]);
    if (*static_cast<int *>(args[1]) == K::RELAX_CTL_ACCEPT) {
      P.st->outer++; P.st->accepted++; P.st->cg_total += 3; P.st->cost = 0.5; P.st->cost_before = 2.0; P.st->cur = 1;
      if (S.relax_ends) { P.st->done = 1; P.st->status = 0; }
    }
  } else {
    return false;
  }
  return true;
}

void hook(const char *name, void **args, void *user) {
  Scenario &S = *static_cast<Scenario *>(user);
  if (g_tracing) trace_args(name, args);
  if (cloud_hook(S, name, args)) return;
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
  } else if (strstr(name, "remove_flag_kernel")) {
    // the survivors = (count of the last tile) + (exclusive scan at the last tile): with no scan running both reads see this word —
    // a quarter of the entries, so half of them "survive"; every frame of the span has entries
    const long long E = *static_cast<long long *>(args[1]);
    const u32 span = *static_cast<u32 *>(args[4]);
    u32 *count = *static_cast<u32 **>(args[6]), *present = *static_cast<u32 **>(args[7]);
    const size_t tiles = ((size_t)E + 1023) / 1024, words = ((size_t)span + 31) / 32;
    REQUIRE(sgtd_stub_block_size(count) >= tiles * sizeof(u32) && sgtd_stub_block_size(present) >= words * sizeof(u32));
    count[tiles - 1] = (u32)(E / 4);
    memset(present, 0xFF, words * sizeof(u32));
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
  // ---- the cloud and graph stages
  auto d = [&](const char *n, int k) { fprintf(f, " %s %.17g", n, arg<double>(a, k)); };
  auto R = [&](int k) {
    const K::RegParams &r = arg<K::RegParams>(a, k);
    fprintf(f, " R{stride %d n_pairs %d n_tiles %d n_ctiles %d total_src %d slice %d k %d max_iterations %d lm_max_trials %d max2 %.17g lambda_factor %.17g eps %.17g %.17g %.17g}", r.stride, r.n_pairs,
            r.n_tiles, r.n_ctiles, r.total_src, r.slice, r.o.k, r.o.max_iterations, r.o.lm_max_trials, r.o.max2, r.o.lambda_factor, r.o.rotation_eps, r.o.translation_eps, r.o.plane_eps);
  };
  auto V = [&](int k) {
    const K::VregParams &v = arg<K::VregParams>(a, k);
    fprintf(f, " V{n_maps %d n_members %d n_member_pts %d mode %d res %.17g n_vox %u map_pose %d}", v.n_maps, v.n_members, v.n_member_pts, v.mode, v.res, v.n_vox, v.map_pose != nullptr);
  };
  auto X = [&](int k) { const K::RelaxParams &r = arg<K::RelaxParams>(a, k); fprintf(f, " X{n %d m %d ms %zu max_outer %d all_held %d lmin %.17g lmax %.17g tol2 %.17g step_tol %.17g}", r.n, r.m, r.ms, r.max_outer, r.all_held, r.lmin, r.lmax, r.tol2, r.step_tol); };
  if (names(name, "reg_cov_kernel") || names(name, "reg_lin_kernel") || names(name, "reg_trial_kernel") || names(name, "reg_final_kernel")) R(0);
  else if (names(name, "reg_init_kernel")) { R(0); p("init", 1); }
  else if (names(name, "reg_search_kernel") || names(name, "reg_match_kernel")) { R(0); i("final", 1); }
  else if (names(name, "vreg_ranges_kernel")) V(0);
  else if (names(name, "vreg_init_kernel")) { R(0); V(1); p("init", 2); }
  else if (names(name, "vreg_corr_kernel")) { R(0); V(1); i("final", 2); }
  else if (has("vreg_")) { R(0); V(1); }
  else if (names(name, "scan_init_kernel")) i("n_sc", 2);
  else if (names(name, "scan_point_kernel")) { const K::ScanPointParams &s = arg<K::ScanPointParams>(a, 0); fprintf(f, " stride %d n %lld n_scans %d", s.stride, s.n, arg<K::ScanCfgDev>(a, 1).n_scans); }
  else if (names(name, "scan_rings_kernel")) i("n_sc", 2);
  else if (names(name, "scan_keys_kernel")) l("n", 9);
  else if (names(name, "scan_heads_kernel")) { l("n", 1); fprintf(f, " drop %llx", (unsigned long long)arg<u64>(a, 2)); }
  else if (names(name, "scan_voxels_kernel")) l("n", 3);
  else if (names(name, "scan_hook_kernel")) i("round", 5);
  else if (names(name, "scan_jump_kernel")) i("round", 3);
  else if (names(name, "scan_offsets_kernel")) i("n_scans", 2);
  else if (names(name, "scan_cluster_ids_kernel")) u("n_kept", 2);
  else if (names(name, "scan_point_clusters_kernel")) { l("n", 8); u("n_kept", 9); }
  else if (names(name, "scan_sum_wave_kernel")) { i("stride", 1); u("n_kept", 5); }
  else if (names(name, "scan_sum_block_kernel")) i("stride", 1);
  else if (names(name, "lm_members_kernel")) { i("n_scans", 2); d("rr", 4); i("max_members", 5); p("mem_off", 6); }
  else if (names(name, "lm_segments_kernel")) { i("a0", 5); i("n_pass", 6); i("n_seg", 7); }
  else if (names(name, "lm_gather_kernel")) { i("n_seg", 4); u("n_points", 5); }
  else if (names(name, "cons_prepare_kernel")) { const K::ConsPrepareParams &c = arg<K::ConsPrepareParams>(a, 0); fprintf(f, " n %d ns %zu n_ids %u frame_a %d pose_a %d", c.n, c.ns, c.n_ids, c.frame_a != nullptr, c.pose_a != nullptr); }
  else if (names(name, "cons_pair_kernel")) { const K::ConsPairParams &c = arg<K::ConsPairParams>(a, 0); fprintf(f, " n %d ns %zu words %u tt %.17g min_trace %.17g", c.n, c.ns, c.words, c.tt, c.min_trace); }
  else if (names(name, "cons_init_kernel")) { i("n", 1); u("words", 2); }
  else if (names(name, "cons_count_kernel")) { i("n", 2); u("words", 3); }
  else if (names(name, "cons_select_kernel")) u("words", 2);
  else if (names(name, "consensus_kernel")) { const K::ConsensusParams &c = arg<K::ConsensusParams>(a, 0); fprintf(f, " n_ids %u cn %d tt %.17g min_trace %.17g", c.n_ids, c.cn, c.tt, c.min_trace); }
  else if (names(name, "relax_init_kernel") || names(name, "relax_setup_kernel") || names(name, "relax_cg_edge_kernel") || names(name, "relax_cg_node_kernel") || names(name, "relax_cg_update_kernel") ||
           names(name, "relax_retract_kernel")) X(0);
  else if (names(name, "relax_edge_kernel")) { X(0); i("trial", 1); }
  else if (names(name, "relax_ctl_kernel")) { X(0); i("mode", 1); }
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

// ---- the cloud and graph stages, launch by launch: sgtd_register_clouds, sgtd_register_voxels, sgtd_scan_keypoints,
// sgtd_local_map_keypoints, sgtd_consistent_loops, sgtd_relax_poses, sgtd_pose_consensus (both forms) and every getter of theirs,
// on one device and on two "devices" behind one handle (their results live on the first device's engine) ----
struct Clouds {       // labelled clouds back to back
  int stride;
  std::vector<int64_t> off{0};
  std::vector<float> pts;
  std::vector<uint32_t> lab;
  Clouds(std::mt19937 &rng, int stride_, std::initializer_list<int> sizes) : stride(stride_) {
    std::uniform_real_distribution<float> u(-30.f, 30.f);
    for (int n : sizes) {
      for (int i = 0; i < n * stride; i++) pts.push_back(u(rng));
      for (int i = 0; i < n; i++) lab.push_back(10 + rng() % 9);
      off.push_back((int64_t)lab.size());
    }
    pts.reserve(4); lab.reserve(1);
  }
  int n() const { return (int)off.size() - 1; }
};
struct OnDevice {     // a copy in "device" memory, `skew` bytes into its block
  void *block = nullptr;
  char *p = nullptr;
  OnDevice(const void *src, size_t bytes, size_t skew = 0) {
    REQUIRE(hipMalloc(&block, bytes + skew + 16) == hipSuccess);
    p = static_cast<char *>(block) + skew;
    memcpy(p, src, bytes);
  }
  ~OnDevice() { REQUIRE(hipFree(block) == hipSuccess); }
  template <class T> const T *as() const { return reinterpret_cast<const T *>(p); }
};

struct CloudStages {
  Scenario &S;
  std::mt19937 &rng;
  sgtd_config cfg;
  sgtd_handle h = nullptr;
  int n_dev = 1;
  void note(const char *text) { if (g_transcript) fprintf(g_transcript, "# %s\n", text); }
  void timing(int on) { CALL(SGTD_OK, h, sgtd_set_timing(h, on)); }

  // ---- sgtd_register_clouds
  void registered(int expect, int n_pairs, int n_clouds) {
    const size_t n = (size_t)std::max(n_pairs, 1);
    std::vector<double> pose(n * 12, -7.0), fit(n, -7.0), cost(n * 2, -7.0), cov(700 * 9, -7.0), d2(700, -7.0);
    std::vector<int32_t> matched(n, -7), iters(n, -7), status(n, -7), tgt(700, -7);
    std::vector<int64_t> cnt(1, -7);
    std::vector<float> ms(4, -7.f);
    CALL(expect, h, sgtd_result_registered(h, pose.data(), fit.data(), cost.data(), matched.data(), iters.data(), status.data()), pose, fit, cost, matched, iters, status);
    CALL(expect, h, sgtd_result_registered(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    CALL(expect, h, sgtd_register_stage_ms(h, &ms[0], &ms[1], &ms[2], &ms[3]));
    CALL(expect, h, sgtd_register_stage_ms(h, nullptr, nullptr, nullptr, nullptr));
    if (expect != SGTD_OK) {
      CALL(expect, h, sgtd_result_register_covariances(h, 0, cov.data(), 700, cnt.data()), cnt);
      CALL(expect, h, sgtd_result_register_matches(h, 0, tgt.data(), d2.data(), 700, cnt.data()), cnt);
      return;
    }
    for (int cl = 0; cl < n_clouds; cl++) {
      CALL(SGTD_OK, h, sgtd_result_register_covariances(h, cl, nullptr, 0, cnt.data()), cnt);
      const int64_t need = cnt[0];
      if (need > 0) CALL(SGTD_ERR_CAPACITY, h, sgtd_result_register_covariances(h, cl, cov.data(), need - 1, cnt.data()), cov, cnt);
      cov.assign(700 * 9, -7.0);
      CALL(SGTD_OK, h, sgtd_result_register_covariances(h, cl, cov.data(), need, cnt.data()), cov, cnt);
      REQUIRE(cnt[0] == need && cov[(size_t)need * 9] == -7.0);
    }
    CALL(SGTD_ERR_INVALID, h, sgtd_result_register_covariances(h, n_clouds, cov.data(), 700, cnt.data()));
    CALL(SGTD_ERR_INVALID, h, sgtd_result_register_covariances(h, 0, cov.data(), -1, cnt.data()));
    for (int k = 0; k < n_pairs; k++) {
      CALL(SGTD_OK, h, sgtd_result_register_matches(h, k, nullptr, nullptr, 0, cnt.data()), cnt);
      const int64_t need = cnt[0];
      if (need > 0) CALL(SGTD_ERR_CAPACITY, h, sgtd_result_register_matches(h, k, tgt.data(), nullptr, need - 1, cnt.data()), tgt, cnt);
      tgt.assign(700, -7);
      CALL(SGTD_OK, h, sgtd_result_register_matches(h, k, tgt.data(), d2.data(), need, nullptr), tgt, d2);
      REQUIRE(cnt[0] == need && tgt[(size_t)need] == -7);
    }
    CALL(SGTD_ERR_INVALID, h, sgtd_result_register_matches(h, n_pairs, tgt.data(), d2.data(), 700, cnt.data()));
  }
  void register_clouds() {
    note("sgtd_register_clouds");
    Env slice("SGTD_REG_SLICE_TILES", "1");       // (a slice of one tile of 512 targets: the cloud of 600 has two)
    const Clouds c(rng, 3, {0, 5, 130, 600}), c4(rng, 4, {0, 5, 130, 600});
    // an empty source; one tile; two source tiles against two target slices; the reverse; an empty target
    const int32_t src[5] = {0, 1, 2, 3, 2}, tgt[5] = {3, 3, 3, 2, 0};
    std::vector<double> init(5 * 12, 0.0);
    for (int k = 0; k < 5; k++) init[(size_t)k * 12] = init[(size_t)k * 12 + 5] = init[(size_t)k * 12 + 10] = 1.0;
    sgtd_register_options o;
    sgtd_default_register_options(&o);
    registered(SGTD_ERR_STATE, 5, 4);
    S.cloud_floats = c.pts.size();
    for (int on : {0, 1}) {
      timing(on);
      S.solve_rounds = 2;                         // (within the first group of SGTD_REG_GROUP rounds)
      CALL(SGTD_OK, h, sgtd_register_clouds(h, nullptr, c.pts.data(), 3, c.off.data(), 4, src, tgt, nullptr, 5, 0));
      registered(SGTD_OK, 5, 4);
      S.solve_rounds = SGTD_REG_GROUP + 2;        // (in the second)
      const OnDevice d(c.pts.data(), c.pts.size() * 4);
      CALL(SGTD_OK, h, sgtd_register_clouds(h, &o, d.as<float>(), 3, c.off.data(), 4, src, tgt, init.data(), 5, 1));
      registered(SGTD_OK, 5, 4);
    }
    S.cloud_floats = c4.pts.size();
    S.solve_rounds = 1;
    CALL(SGTD_OK, h, sgtd_register_clouds(h, &o, c4.pts.data(), 4, c4.off.data(), 4, src + 1, tgt + 1, init.data(), 2, 0));
    registered(SGTD_OK, 2, 4);
    // solves that never end: the rounds' bound and its error (on a group: raised on the first device's engine)
    o.max_iterations = 1; o.lm_max_trials = 2;
    S.solve_rounds = 0;
    CALL(SGTD_ERR_HIP, h, sgtd_register_clouds(h, &o, c4.pts.data(), 4, c4.off.data(), 4, src, tgt, nullptr, 5, 0));
    registered(SGTD_ERR_STATE, 5, 4);
    sgtd_default_register_options(&o);
    // only pairs none of whose solves starts; no pair; no cloud
    CALL(SGTD_OK, h, sgtd_register_clouds(h, nullptr, c4.pts.data(), 4, c4.off.data(), 4, src, tgt, nullptr, 1, 0));
    registered(SGTD_OK, 1, 4);
    CALL(SGTD_OK, h, sgtd_register_clouds(h, nullptr, c4.pts.data(), 4, c4.off.data(), 4, nullptr, nullptr, nullptr, 0, 0));
    registered(SGTD_OK, 0, 4);
    const int64_t none[1] = {0};
    CALL(SGTD_OK, h, sgtd_register_clouds(h, nullptr, nullptr, 3, none, 0, nullptr, nullptr, nullptr, 0, 0));
    registered(SGTD_OK, 0, 0);
    timing(0);
    // every exit of the validation, in its order; the results of the last call stay
    const float *p = c.pts.data();
    const int64_t *off = c.off.data();
    CALL(SGTD_ERR_INVALID, h, sgtd_register_clouds(h, nullptr, p, 3, off, -1, src, tgt, nullptr, 5, 0));
    CALL(SGTD_ERR_INVALID, h, sgtd_register_clouds(h, nullptr, p, 3, off, 4, src, tgt, nullptr, -1, 0));
    CALL(SGTD_ERR_INVALID, h, sgtd_register_clouds(h, nullptr, p, 3, nullptr, 4, src, tgt, nullptr, 5, 0));
    CALL(SGTD_ERR_INVALID, h, sgtd_register_clouds(h, nullptr, p, 5, off, 4, src, tgt, nullptr, 5, 0));
    CALL(SGTD_ERR_INVALID, h, sgtd_register_clouds(h, nullptr, p, 3, off, 4, nullptr, tgt, nullptr, 5, 0));
    for (int bad = 0; bad < 9; bad++) {
      sgtd_register_options b;
      sgtd_default_register_options(&b);
      if (bad == 0) b.k_neighbors = 2; else if (bad == 1) b.k_neighbors = SGTD_REG_MAX_K + 1; else if (bad == 2) b.max_iterations = 0; else if (bad == 3) b.lm_max_trials = 0;
      else if (bad == 4) b.reserved = 1; else if (bad == 5) b.max_corr_dist = 0.0; else if (bad == 6) b.lm_init_lambda_factor = kNaN; else if (bad == 7) b.rotation_eps = 0.0;
      else b.plane_eps = -1.0;
      CALL(SGTD_ERR_INVALID, h, sgtd_register_clouds(h, &b, p, 3, off, 4, src, tgt, nullptr, 5, 0));
    }
    const int64_t from_one[5] = {1, 1, 6, 136, 736}, back[5] = {0, 0, 5, 4, 604};
    CALL(SGTD_ERR_INVALID, h, sgtd_register_clouds(h, nullptr, p, 3, from_one, 4, src, tgt, nullptr, 5, 0));
    CALL(SGTD_ERR_INVALID, h, sgtd_register_clouds(h, nullptr, p, 3, back, 4, src, tgt, nullptr, 5, 0));
    CALL(SGTD_ERR_INVALID, h, sgtd_register_clouds(h, nullptr, nullptr, 3, off, 4, src, tgt, nullptr, 5, 0));
    const int32_t past[5] = {0, 1, 2, 4, 2}, below[5] = {3, -1, 3, 2, 0};
    CALL(SGTD_ERR_INVALID, h, sgtd_register_clouds(h, nullptr, p, 3, off, 4, past, tgt, nullptr, 5, 0));
    CALL(SGTD_ERR_INVALID, h, sgtd_register_clouds(h, nullptr, p, 3, off, 4, src, below, nullptr, 5, 0));
    init[17] = std::numeric_limits<double>::infinity();
    CALL(SGTD_ERR_INVALID, h, sgtd_register_clouds(h, nullptr, p, 3, off, 4, src, tgt, init.data(), 5, 0));
    const int64_t large[2] = {0, (int64_t)SGTD_REG_MAX_POINTS + 1};
    const int32_t zero[1] = {0};
    CALL(SGTD_ERR_UNSUPPORTED, h, sgtd_register_clouds(h, nullptr, p, 3, large, 1, zero, zero, nullptr, 1, 0));
    // (an invalid option together with a cloud too large: INVALID comes first)
    { sgtd_register_options b; sgtd_default_register_options(&b); b.k_neighbors = 2; CALL(SGTD_ERR_INVALID, h, sgtd_register_clouds(h, &b, p, 3, large, 1, zero, zero, nullptr, 1, 0)); }
    registered(SGTD_OK, 0, 0);
  }

  // ---- sgtd_register_voxels
  void voxel_registered(int expect, int n_pairs, int n_maps) {
    const size_t n = (size_t)std::max(n_pairs, 1);
    std::vector<double> pose(n * 12, -7.0), fit(n, -7.0), cost(n * 2, -7.0), mean(8 * 3, -7.0), cov(8 * 9, -7.0);
    std::vector<int32_t> matched(n, -7), corr(n, -7), iters(n, -7), status(n, -7), coord(8 * 3, -7), np(8, -7), vox(700 * 27, -7);
    std::vector<int64_t> cnt(1, -7);
    std::vector<float> ms(5, -7.f);
    CALL(expect, h, sgtd_result_voxel_registered(h, pose.data(), fit.data(), cost.data(), matched.data(), corr.data(), iters.data(), status.data()), pose, fit, cost, matched, corr, iters, status);
    CALL(expect, h, sgtd_result_voxel_registered(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    CALL(expect, h, sgtd_voxel_register_stage_ms(h, &ms[0], &ms[1], &ms[2], &ms[3], &ms[4]));
    if (expect != SGTD_OK) {
      CALL(expect, h, sgtd_result_voxel_map(h, 0, coord.data(), np.data(), mean.data(), cov.data(), 8, cnt.data()), cnt);
      CALL(expect, h, sgtd_result_voxel_matches(h, 0, vox.data(), 700, cnt.data()), cnt);
      return;
    }
    for (int m = 0; m < n_maps; m++) {
      CALL(SGTD_OK, h, sgtd_result_voxel_map(h, m, nullptr, nullptr, nullptr, nullptr, 0, cnt.data()), cnt);
      const int64_t need = cnt[0];
      REQUIRE(need <= 8);
      if (need > 0) CALL(SGTD_ERR_CAPACITY, h, sgtd_result_voxel_map(h, m, coord.data(), np.data(), nullptr, cov.data(), need - 1, cnt.data()), coord, np, cov, cnt);
      CALL(SGTD_OK, h, sgtd_result_voxel_map(h, m, coord.data(), np.data(), mean.data(), cov.data(), need, cnt.data()), coord, np, mean, cov, cnt);
      CALL(SGTD_OK, h, sgtd_result_voxel_map(h, m, nullptr, np.data(), nullptr, nullptr, need, nullptr), np);
    }
    CALL(SGTD_ERR_INVALID, h, sgtd_result_voxel_map(h, n_maps, coord.data(), np.data(), mean.data(), cov.data(), 8, cnt.data()));
    for (int k = 0; k < n_pairs; k++) {
      CALL(SGTD_OK, h, sgtd_result_voxel_matches(h, k, nullptr, 0, cnt.data()), cnt);
      const int64_t need = cnt[0];
      if (need > 0) CALL(SGTD_ERR_CAPACITY, h, sgtd_result_voxel_matches(h, k, vox.data(), need - 1, cnt.data()), vox, cnt);
      CALL(SGTD_OK, h, sgtd_result_voxel_matches(h, k, vox.data(), need, cnt.data()), vox, cnt);
    }
    CALL(SGTD_ERR_INVALID, h, sgtd_result_voxel_matches(h, n_pairs, vox.data(), 700, cnt.data()));
  }
  void register_voxels() {
    note("sgtd_register_voxels");
    const Clouds c(rng, 3, {0, 5, 130, 600});
    // maps: the cloud of 600; no member; the clouds of 130 and 5.  Pairs: against a map with voxels (one and two source tiles),
    // an empty source, a map whose range stays empty
    const int32_t map_off[4] = {0, 1, 1, 3}, map_cloud[3] = {3, 2, 1}, src[4] = {1, 2, 0, 1}, tgt[4] = {0, 2, 0, 1};
    std::vector<double> init(4 * 12, 0.0), map_pose(3 * 12, 0.0);
    for (int k = 0; k < 4; k++) init[(size_t)k * 12] = init[(size_t)k * 12 + 5] = init[(size_t)k * 12 + 10] = 1.0;
    for (int k = 0; k < 3; k++) { map_pose[(size_t)k * 12] = map_pose[(size_t)k * 12 + 5] = map_pose[(size_t)k * 12 + 10] = 1.0; map_pose[(size_t)k * 12 + 3] = 0.5 * k; }
    sgtd_voxel_register_options o;
    sgtd_default_voxel_register_options(&o);
    voxel_registered(SGTD_ERR_STATE, 4, 3);
    S.cloud_floats = c.pts.size();
    S.map_voxels = {5, 0, 3}; S.voxels = 8;
    const int modes[3] = {1, 7, 27};
    for (int on : {0, 1}) {
      timing(on);
      S.solve_rounds = 2;
      o.neighbor_mode = modes[on];
      CALL(SGTD_OK, h, sgtd_register_voxels(h, &o, c.pts.data(), 3, c.off.data(), 4, map_off, map_cloud, nullptr, 3, src, tgt, nullptr, 4, 0));
      voxel_registered(SGTD_OK, 4, 3);
      S.solve_rounds = SGTD_REG_GROUP + 2;
      o.neighbor_mode = modes[on + 1];
      const OnDevice d(c.pts.data(), c.pts.size() * 4);
      CALL(SGTD_OK, h, sgtd_register_voxels(h, &o, d.as<float>(), 3, c.off.data(), 4, map_off, map_cloud, map_pose.data(), 3, src, tgt, init.data(), 4, 1));
      voxel_registered(SGTD_OK, 4, 3);
      // maps and no pair
      CALL(SGTD_OK, h, sgtd_register_voxels(h, nullptr, c.pts.data(), 3, c.off.data(), 4, map_off, map_cloud, nullptr, 3, nullptr, nullptr, nullptr, 0, 0));
      voxel_registered(SGTD_OK, 0, 3);
    }
    o.max_iterations = 1; o.lm_max_trials = 2;
    S.solve_rounds = 0;
    CALL(SGTD_ERR_HIP, h, sgtd_register_voxels(h, &o, c.pts.data(), 3, c.off.data(), 4, map_off, map_cloud, nullptr, 3, src, tgt, nullptr, 4, 0));
    voxel_registered(SGTD_ERR_STATE, 4, 3);
    // the hook leaves every range empty: no solve starts.  Maps whose members have no points.  No map
    S.map_voxels = {0, 0, 0}; S.voxels = 0;
    CALL(SGTD_OK, h, sgtd_register_voxels(h, nullptr, c.pts.data(), 3, c.off.data(), 4, map_off, map_cloud, nullptr, 3, src, tgt, nullptr, 4, 0));
    voxel_registered(SGTD_OK, 4, 3);
    const int32_t hollow_off[3] = {0, 1, 2}, hollow_cloud[2] = {0, 0}, hollow_tgt[2] = {1, 0};
    CALL(SGTD_OK, h, sgtd_register_voxels(h, nullptr, c.pts.data(), 3, c.off.data(), 4, hollow_off, hollow_cloud, map_pose.data(), 2, src, hollow_tgt, nullptr, 2, 0));
    voxel_registered(SGTD_OK, 2, 2);
    CALL(SGTD_OK, h, sgtd_register_voxels(h, nullptr, c.pts.data(), 3, c.off.data(), 4, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 0));
    voxel_registered(SGTD_OK, 0, 0);
    timing(0);
    // every exit of the validation, in its order
    const float *p = c.pts.data();
    const int64_t *off = c.off.data();
    sgtd_default_voxel_register_options(&o);
#define VOX(status, opt, pts, stride, off_, nc, mo, mc, mp, nm, s, t, in, np) CALL(status, h, sgtd_register_voxels(h, opt, pts, stride, off_, nc, mo, mc, mp, nm, s, t, in, np, 0))
    VOX(SGTD_ERR_INVALID, nullptr, p, 3, off, -1, map_off, map_cloud, nullptr, 3, src, tgt, nullptr, 4);
    VOX(SGTD_ERR_INVALID, nullptr, p, 3, off, 4, map_off, map_cloud, nullptr, -1, src, tgt, nullptr, 4);
    VOX(SGTD_ERR_INVALID, nullptr, p, 2, off, 4, map_off, map_cloud, nullptr, 3, src, tgt, nullptr, 4);
    VOX(SGTD_ERR_INVALID, nullptr, p, 3, off, 4, map_off, map_cloud, nullptr, 3, src, nullptr, nullptr, 4);
    VOX(SGTD_ERR_INVALID, nullptr, p, 3, off, 4, nullptr, map_cloud, nullptr, 3, src, tgt, nullptr, 4);
    for (int bad = 0; bad < 6; bad++) {
      sgtd_voxel_register_options b;
      sgtd_default_voxel_register_options(&b);
      if (bad == 0) b.k_neighbors = 2; else if (bad == 1) b.max_iterations = 0; else if (bad == 2) b.reserved = 1; else if (bad == 3) b.voxel_resolution = 0.0; else if (bad == 4) b.neighbor_mode = 6;
      else b.translation_eps = kNaN;
      VOX(SGTD_ERR_INVALID, &b, p, 3, off, 4, map_off, map_cloud, nullptr, 3, src, tgt, nullptr, 4);
    }
    const int64_t from_one[5] = {1, 1, 6, 136, 736}, back[5] = {0, 0, 5, 4, 604};
    VOX(SGTD_ERR_INVALID, nullptr, p, 3, from_one, 4, map_off, map_cloud, nullptr, 3, src, tgt, nullptr, 4);
    VOX(SGTD_ERR_INVALID, nullptr, p, 3, back, 4, map_off, map_cloud, nullptr, 3, src, tgt, nullptr, 4);
    VOX(SGTD_ERR_INVALID, nullptr, nullptr, 3, off, 4, map_off, map_cloud, nullptr, 3, src, tgt, nullptr, 4);
    const int32_t moff_one[4] = {1, 1, 1, 3}, moff_back[4] = {0, 2, 1, 3}, mcl_past[3] = {3, 4, 1}, tgt_past[4] = {0, 3, 0, 1}, src_below[4] = {1, -1, 0, 1};
    VOX(SGTD_ERR_INVALID, nullptr, p, 3, off, 4, moff_one, map_cloud, nullptr, 3, src, tgt, nullptr, 4);
    VOX(SGTD_ERR_INVALID, nullptr, p, 3, off, 4, moff_back, map_cloud, nullptr, 3, src, tgt, nullptr, 4);
    VOX(SGTD_ERR_INVALID, nullptr, p, 3, off, 4, map_off, nullptr, nullptr, 3, src, tgt, nullptr, 4);
    VOX(SGTD_ERR_INVALID, nullptr, p, 3, off, 4, map_off, mcl_past, nullptr, 3, src, tgt, nullptr, 4);
    VOX(SGTD_ERR_INVALID, nullptr, p, 3, off, 4, map_off, map_cloud, nullptr, 3, src, tgt_past, nullptr, 4);
    VOX(SGTD_ERR_INVALID, nullptr, p, 3, off, 4, map_off, map_cloud, nullptr, 3, src_below, tgt, nullptr, 4);
    init[40] = kNaN;
    VOX(SGTD_ERR_INVALID, nullptr, p, 3, off, 4, map_off, map_cloud, nullptr, 3, src, tgt, init.data(), 4);
    map_pose[30] = kNaN;
    VOX(SGTD_ERR_INVALID, nullptr, p, 3, off, 4, map_off, map_cloud, map_pose.data(), 3, src, tgt, nullptr, 4);
    // the caps: a cloud too large; too many maps; too many member points; too many correspondences
    const int64_t large[2] = {0, (int64_t)SGTD_REG_MAX_POINTS + 1};
    const int32_t zero[2] = {0, 0};
    VOX(SGTD_ERR_UNSUPPORTED, nullptr, p, 3, large, 1, zero, zero, nullptr, 1, zero, zero, nullptr, 1);
    {
      std::vector<int32_t> many((size_t)SGTD_VREG_MAX_MAPS + 2, 0);
      VOX(SGTD_ERR_UNSUPPORTED, nullptr, p, 3, off, 4, many.data(), map_cloud, nullptr, SGTD_VREG_MAX_MAPS + 1, src, zero, nullptr, 1);
      const int64_t full[2] = {0, (int64_t)SGTD_REG_MAX_POINTS};
      const int members = SGTD_VREG_MAX_MEMBER_POINTS / SGTD_REG_MAX_POINTS + 1;
      const int32_t one_map[2] = {0, members};
      std::vector<int32_t> same((size_t)members, 0);
      VOX(SGTD_ERR_UNSUPPORTED, nullptr, p, 3, full, 1, one_map, same.data(), nullptr, 1, zero, zero, nullptr, 1);
      const int pairs = SGTD_VREG_MAX_CORR / 27 / SGTD_REG_MAX_POINTS + 1;
      std::vector<int32_t> zeros((size_t)pairs, 0);
      sgtd_voxel_register_options b;
      sgtd_default_voxel_register_options(&b);
      b.neighbor_mode = 27;
      VOX(SGTD_ERR_UNSUPPORTED, &b, p, 3, full, 1, zero, zero, nullptr, 1, zeros.data(), zeros.data(), nullptr, pairs);
    }
#undef VOX
    voxel_registered(SGTD_OK, 0, 0);
  }

  // ---- sgtd_scan_keypoints and sgtd_local_map_keypoints
  void scan_read(int expect, int n_scans, int64_t kept) {
    const size_t k1 = (size_t)kept + 1;
    std::vector<int64_t> kp_off((size_t)std::max(n_scans, 0) + 1, -7), cnt(1, -7);
    std::vector<float> xyz(k1 * 3, -7.f);
    std::vector<uint32_t> label(k1, 7u);
    std::vector<int32_t> np(k1, -7), cluster(1100, -7), grid(128, -7);
    std::vector<double> range(128, -7.0);
    const float *dx = nullptr; const uint32_t *dl = nullptr;
    CALL(expect, h, sgtd_result_scan_keypoints(h, kp_off.data(), xyz.data(), label.data(), np.data(), kept, cnt.data()), kp_off, xyz, label, np, cnt);
    CALL(expect, h, sgtd_result_scan_keypoints(h, nullptr, nullptr, nullptr, nullptr, 0, nullptr));
    CALL(expect, h, sgtd_scan_device_view(h, &dx, &dl));
    if (expect != SGTD_OK) {
      CALL(expect, h, sgtd_result_scan_point_clusters(h, 0, cluster.data(), 1100, cnt.data()));
      CALL(expect, h, sgtd_result_scan_grids(h, 0, grid.data(), range.data()));
      return;
    }
    REQUIRE(cnt[0] == kept && kp_off.back() == kept && xyz[(size_t)kept * 3] == -7.f);
    if (kept > 0) {
      CALL(SGTD_ERR_CAPACITY, h, sgtd_result_scan_keypoints(h, nullptr, xyz.data(), nullptr, np.data(), kept - 1, cnt.data()), xyz, np, cnt);
      CALL(SGTD_OK, h, sgtd_result_scan_keypoints(h, nullptr, nullptr, nullptr, nullptr, kept - 1, cnt.data()), cnt);
      REQUIRE(sgtd_stub_block_size(dx) >= (size_t)kept * 12 && sgtd_stub_block_size(dl) >= (size_t)kept * 4);
    }
    CALL(SGTD_ERR_INVALID, h, sgtd_result_scan_keypoints(h, nullptr, nullptr, nullptr, nullptr, -1, cnt.data()));
    for (int s = 0; s < n_scans; s++) {
      CALL(SGTD_OK, h, sgtd_result_scan_point_clusters(h, s, nullptr, 0, cnt.data()), cnt);
      const int64_t need = cnt[0];
      if (need > 0) CALL(SGTD_ERR_CAPACITY, h, sgtd_result_scan_point_clusters(h, s, cluster.data(), need - 1, cnt.data()), cluster, cnt);
      CALL(SGTD_OK, h, sgtd_result_scan_point_clusters(h, s, cluster.data(), need, cnt.data()), cluster, cnt);
      CALL(SGTD_OK, h, sgtd_result_scan_grids(h, s, grid.data(), range.data()), grid, range);
      CALL(SGTD_OK, h, sgtd_result_scan_grids(h, s, nullptr, nullptr));
    }
    CALL(SGTD_ERR_INVALID, h, sgtd_result_scan_point_clusters(h, n_scans, cluster.data(), 1100, cnt.data()));
    CALL(SGTD_ERR_INVALID, h, sgtd_result_scan_grids(h, n_scans, grid.data(), range.data()));
  }
  void scan_keypoints() {
    note("sgtd_scan_keypoints");
    const Clouds one(rng, 3, {1025}), two(rng, 4, {1025, 7}), hollow(rng, 3, {0, 0});      // (1025: two tiles of SGTD_SCAN_TILE)
    const int64_t none[1] = {0};
    scan_read(SGTD_ERR_STATE, 1, 0);
    CALL(SGTD_OK, h, sgtd_scan_keypoints(h, nullptr, nullptr, 3, nullptr, none, 0, 0));
    scan_read(SGTD_OK, 0, 0);
    CALL(SGTD_OK, h, sgtd_scan_keypoints(h, nullptr, nullptr, 3, nullptr, hollow.off.data(), 2, 0));
    scan_read(SGTD_OK, 2, 0);
    sgtd_scan_config sc;
    sgtd_default_scan_config(&sc);
    for (int on : {0, 1}) {
      timing(on);
      S.voxels = 40; S.kept = on ? 3 : 0;
      CALL(SGTD_OK, h, sgtd_scan_keypoints(h, on ? &sc : nullptr, one.pts.data(), 3, one.lab.data(), one.off.data(), 1, 0));
      scan_read(SGTD_OK, 1, S.kept);
      S.kept = on ? 0 : 5;
      const OnDevice dp(two.pts.data(), two.pts.size() * 4), dl(two.lab.data(), two.lab.size() * 4);
      CALL(SGTD_OK, h, sgtd_scan_keypoints(h, &sc, dp.as<float>(), 4, dl.as<uint32_t>(), two.off.data(), 2, 1));
      scan_read(SGTD_OK, 2, S.kept);
    }
    timing(0);
    // every exit of the validation, in its order: the config's INVALID before the caps, its UNSUPPORTED after them
    const float *p = one.pts.data();
    const uint32_t *l = one.lab.data();
    CALL(SGTD_ERR_INVALID, h, sgtd_scan_keypoints(h, nullptr, p, 3, l, one.off.data(), -1, 0));
    CALL(SGTD_ERR_INVALID, h, sgtd_scan_keypoints(h, nullptr, p, 3, l, nullptr, 1, 0));
    CALL(SGTD_ERR_INVALID, h, sgtd_scan_keypoints(h, nullptr, p, 5, l, one.off.data(), 1, 0));
    sgtd_scan_config bad = sc, wide = sc;
    bad.start_r = -1.0; wide.delta_a = 0.1;
    std::vector<int64_t> many((size_t)SGTD_SCAN_MAX_SCANS + 2, 0);
    const int64_t from_one[2] = {1, 1026}, back[3] = {0, 5, 4};
    CALL(SGTD_ERR_INVALID, h, sgtd_scan_keypoints(h, &bad, p, 3, l, many.data(), SGTD_SCAN_MAX_SCANS + 1, 0));
    CALL(SGTD_ERR_INVALID, h, sgtd_scan_keypoints(h, nullptr, p, 3, l, from_one, 1, 0));
    CALL(SGTD_ERR_INVALID, h, sgtd_scan_keypoints(h, nullptr, p, 3, l, back, 2, 0));
    CALL(SGTD_ERR_INVALID, h, sgtd_scan_keypoints(h, nullptr, p, 3, nullptr, one.off.data(), 1, 0));
    CALL(SGTD_ERR_UNSUPPORTED, h, sgtd_scan_keypoints(h, &wide, p, 3, l, many.data(), SGTD_SCAN_MAX_SCANS + 1, 0));      // (the caps' text)
    CALL(SGTD_ERR_UNSUPPORTED, h, sgtd_scan_keypoints(h, &wide, p, 3, l, one.off.data(), 1, 0));                       // (the config's)
    scan_read(SGTD_OK, 2, 0);
  }
  // passes: those the call made, each of which keeps S.kept keypoints (where it has any point)
  void local_map_read(int expect, int n_anchors, int n_passes) {
    std::vector<int64_t> kp_off((size_t)n_anchors + 1, -7), mem_off((size_t)n_anchors + 1, -7), merged((size_t)n_anchors + 1, -7), cnt(1, 0);
    if (expect == SGTD_OK) CALL(SGTD_OK, h, sgtd_result_local_map_keypoints(h, nullptr, nullptr, nullptr, nullptr, 0, cnt.data()), cnt);
    const int64_t kept = cnt[0];
    REQUIRE(kept <= S.kept * n_passes);
    const size_t k1 = (size_t)kept + 1;
    std::vector<float> xyz(k1 * 3, -7.f), ms(3, -7.f);
    std::vector<uint32_t> label(k1, 7u);
    std::vector<int32_t> np(k1, -7), member(64, -7), passes(1, -7);
    const float *dx = nullptr; const uint32_t *dl = nullptr;
    CALL(expect, h, sgtd_result_local_map_keypoints(h, kp_off.data(), xyz.data(), label.data(), np.data(), kept, cnt.data()), kp_off, xyz, label, np, cnt);
    CALL(expect, h, sgtd_result_local_map_keypoints(h, nullptr, nullptr, nullptr, nullptr, 0, nullptr));
    CALL(expect, h, sgtd_result_local_map_members(h, mem_off.data(), nullptr, 0, cnt.data(), merged.data(), passes.data()), mem_off, cnt, merged, passes);
    CALL(expect, h, sgtd_local_map_device_view(h, &dx, &dl));
    CALL(expect, h, sgtd_local_map_stage_ms(h, &ms[0], &ms[1], &ms[2]));
    if (expect != SGTD_OK) return;
    REQUIRE(kp_off.back() == kept && xyz[(size_t)kept * 3] == -7.f && (passes[0] == n_passes || kept == 0));
    const int64_t need = cnt[0];
    if (kept > 0) CALL(SGTD_ERR_CAPACITY, h, sgtd_result_local_map_keypoints(h, nullptr, nullptr, label.data(), nullptr, kept - 1, cnt.data()), label, cnt);
    REQUIRE(need <= 63);
    if (need > 0) CALL(SGTD_ERR_CAPACITY, h, sgtd_result_local_map_members(h, nullptr, member.data(), need - 1, cnt.data(), nullptr, nullptr), member, cnt);
    CALL(SGTD_OK, h, sgtd_result_local_map_members(h, nullptr, member.data(), need, nullptr, nullptr, nullptr), member);
    REQUIRE(member[(size_t)need] == -7);
    CALL(SGTD_ERR_INVALID, h, sgtd_result_local_map_members(h, nullptr, member.data(), -1, cnt.data(), nullptr, nullptr));
  }
  void local_map_keypoints() {
    note("sgtd_local_map_keypoints");
    const Clouds c3(rng, 3, {1025, 7, 0}), c4(rng, 4, {1025, 7, 0});
    std::vector<float> pose(3 * 12, 0.f);
    for (int s = 0; s < 3; s++) { pose[(size_t)s * 12] = pose[(size_t)s * 12 + 5] = pose[(size_t)s * 12 + 10] = 1.f; pose[(size_t)s * 12 + 3] = 2.f * s; }
    const int64_t none[1] = {0};
    const int32_t anchors[4] = {1, 0, 2, 0};
    sgtd_local_map_options o;
    sgtd_default_local_map_options(&o);
    local_map_read(SGTD_ERR_STATE, 1, 0);
    CALL(SGTD_OK, h, sgtd_local_map_keypoints(h, nullptr, nullptr, nullptr, 3, nullptr, none, nullptr, 0, nullptr, 0, 0));
    local_map_read(SGTD_OK, 0, 0);
    CALL(SGTD_OK, h, sgtd_local_map_keypoints(h, nullptr, nullptr, c3.pts.data(), 3, c3.lab.data(), c3.off.data(), pose.data(), 3, anchors, 0, 0));
    local_map_read(SGTD_OK, 0, 0);
    for (int on : {0, 1}) {
      timing(on);
      // every scan an anchor, one pass; the points with three floats each
      S.voxels = 40; S.kept = on ? 0 : 4;
      CALL(SGTD_OK, h, sgtd_local_map_keypoints(h, nullptr, nullptr, c3.pts.data(), 3, c3.lab.data(), c3.off.data(), pose.data(), 3, nullptr, 3, 0));
      local_map_read(SGTD_OK, 3, 1);
      scan_read(SGTD_ERR_STATE, 1, 0);       // (the clustering ran in the scan stage's buffers)
      // anchors given, three passes (max_pass_points holds one merged cloud of two scans); four floats a point, from the host (16-byte rows) ...
      o.max_pass_points = 1035; o.max_members = 2;
      S.kept = 2;
      CALL(SGTD_OK, h, sgtd_local_map_keypoints(h, nullptr, &o, c4.pts.data(), 4, c4.lab.data(), c4.off.data(), pose.data(), 3, anchors, 4, 0));
      local_map_read(SGTD_OK, 4, 3);
      // ... and on the device four bytes off a 16-byte boundary
      const OnDevice dp(c4.pts.data(), c4.pts.size() * 4, 4), dl(c4.lab.data(), c4.lab.size() * 4);
      CALL(SGTD_OK, h, sgtd_local_map_keypoints(h, nullptr, &o, dp.as<float>(), 4, dl.as<uint32_t>(), c4.off.data(), pose.data(), 3, anchors, 2, 1));
      local_map_read(SGTD_OK, 2, 2);
    }
    timing(0);
    // a merged cloud larger than a pass may be (on a group: raised on the first device's engine)
    o.max_pass_points = 100;
    CALL(SGTD_ERR_UNSUPPORTED, h, sgtd_local_map_keypoints(h, nullptr, &o, c3.pts.data(), 3, c3.lab.data(), c3.off.data(), pose.data(), 3, nullptr, 3, 0));
    local_map_read(SGTD_ERR_STATE, 3, 0);
    S.kept = 1;
    CALL(SGTD_OK, h, sgtd_local_map_keypoints(h, nullptr, nullptr, c3.pts.data(), 3, c3.lab.data(), c3.off.data(), pose.data(), 3, anchors + 2, 1, 0));      // (a pass without a point)
    local_map_read(SGTD_OK, 1, 0);
    CALL(SGTD_OK, h, sgtd_local_map_keypoints(h, nullptr, nullptr, c3.pts.data(), 3, c3.lab.data(), c3.off.data(), pose.data(), 3, anchors, 1, 0));
    // every exit of the validation, in its order
    const float *p = c3.pts.data();
    const uint32_t *l = c3.lab.data();
    const int64_t *off = c3.off.data();
    sgtd_scan_config sc, bad, wide;
    sgtd_default_scan_config(&sc);
    bad = wide = sc;
    bad.min_range = 200.0; wide.delta_p = 0.1;
    std::vector<int64_t> many((size_t)SGTD_SCAN_MAX_SCANS + 2, 0);
    std::vector<float> many_poses(((size_t)SGTD_SCAN_MAX_SCANS + 1) * 12, 0.f);
    const int64_t from_one[4] = {1, 1026, 1033, 1033}, back[4] = {0, 1025, 1024, 1032};
    const int32_t past[2] = {0, 3};
#define LM(status, cfg_, opt, pts, stride, lab, off_, pose_, ns, anch, na) CALL(status, h, sgtd_local_map_keypoints(h, cfg_, opt, pts, stride, lab, off_, pose_, ns, anch, na, 0))
    LM(SGTD_ERR_INVALID, nullptr, nullptr, p, 3, l, off, pose.data(), -1, nullptr, 0);
    LM(SGTD_ERR_INVALID, nullptr, nullptr, p, 3, l, off, pose.data(), 3, anchors, -1);
    LM(SGTD_ERR_INVALID, nullptr, nullptr, p, 3, l, nullptr, pose.data(), 3, nullptr, 0);
    LM(SGTD_ERR_INVALID, nullptr, nullptr, p, 2, l, off, pose.data(), 3, nullptr, 0);
    LM(SGTD_ERR_INVALID, &bad, nullptr, p, 3, l, many.data(), many_poses.data(), SGTD_SCAN_MAX_SCANS + 1, nullptr, 0);
    for (int k = 0; k < 5; k++) {
      sgtd_local_map_options b;
      sgtd_default_local_map_options(&b);
      if (k == 0) b.radius = -1.0; else if (k == 1) b.max_members = -1; else if (k == 2) b.reserved = 1; else if (k == 3) b.max_pass_points = -1; else b.max_pass_points = (int64_t)SGTD_SCAN_MAX_POINTS + 1;
      LM(SGTD_ERR_INVALID, nullptr, &b, p, 3, l, off, pose.data(), 3, nullptr, 0);
    }
    LM(SGTD_ERR_INVALID, nullptr, nullptr, p, 3, l, from_one, pose.data(), 3, nullptr, 0);
    LM(SGTD_ERR_INVALID, nullptr, nullptr, p, 3, l, back, pose.data(), 3, nullptr, 0);
    LM(SGTD_ERR_INVALID, nullptr, nullptr, nullptr, 3, l, off, pose.data(), 3, nullptr, 0);
    LM(SGTD_ERR_INVALID, nullptr, nullptr, p, 3, l, off, nullptr, 3, nullptr, 0);
    LM(SGTD_ERR_INVALID, nullptr, nullptr, p, 3, l, off, pose.data(), 3, past, 2);
    LM(SGTD_ERR_UNSUPPORTED, &wide, nullptr, p, 3, l, many.data(), many_poses.data(), SGTD_SCAN_MAX_SCANS + 1, nullptr, 0);
    LM(SGTD_ERR_UNSUPPORTED, &wide, nullptr, p, 3, l, off, pose.data(), 3, nullptr, 0);
#undef LM
    local_map_read(SGTD_OK, 1, 1);
  }

  // ---- sgtd_consistent_loops, sgtd_relax_poses
  void consistent_read(int expect, int64_t n) {
    const size_t m = (size_t)std::max<int64_t>(n, 1), words = (m + 63) / 64;
    std::vector<int32_t> in_set(m, -7), degree(m, -7), pick(m, -7);
    std::vector<double> thr(2, -7.0);
    std::vector<uint64_t> rows(m * words, 7u);
    CALL(expect, h, sgtd_result_consistent(h, in_set.data(), degree.data(), pick.data(), thr.data()), in_set, degree, pick, thr);
    CALL(expect, h, sgtd_result_consistent(h, nullptr, nullptr, nullptr, nullptr));
    CALL(expect, h, sgtd_result_consistency_rows(h, 0, n, rows.data()), rows);
    if (expect != SGTD_OK) return;
    if (n > 1) CALL(SGTD_OK, h, sgtd_result_consistency_rows(h, 1, n - 1, rows.data()), rows);
    CALL(SGTD_OK, h, sgtd_result_consistency_rows(h, n, 0, nullptr));
    CALL(SGTD_ERR_INVALID, h, sgtd_result_consistency_rows(h, 0, n + 1, rows.data()));
    CALL(SGTD_ERR_INVALID, h, sgtd_result_consistency_rows(h, -1, 0, rows.data()));
    if (n > 0) CALL(SGTD_ERR_INVALID, h, sgtd_result_consistency_rows(h, 0, n, nullptr));
  }
  void consistent_loops() {
    note("sgtd_consistent_loops");
    const int n = 70;       // (two words a row)
    std::vector<uint32_t> fa((size_t)n), fb((size_t)n);
    std::vector<double> rel((size_t)n * 12, 0.0);
    std::vector<float> pa((size_t)n * 12, 0.f);
    for (int k = 0; k < n; k++) {
      fa[(size_t)k] = (uint32_t)(k % 5); fb[(size_t)k] = (uint32_t)(k % 7 + 5);
      rel[(size_t)k * 12] = rel[(size_t)k * 12 + 4] = rel[(size_t)k * 12 + 8] = 1.0; rel[(size_t)k * 12 + 9] = 0.25 * k;
      pa[(size_t)k * 12] = pa[(size_t)k * 12 + 5] = pa[(size_t)k * 12 + 10] = 1.f;
    }
    std::vector<int32_t> n_set(1, -7);
    consistent_read(SGTD_ERR_STATE, 5);
    CALL(SGTD_OK, h, sgtd_consistent_loops(h, 0, nullptr, nullptr, nullptr, nullptr, 0.5, 0.1, n_set.data()), n_set);
    consistent_read(SGTD_OK, 0);
    for (int on : {0, 1}) {
      timing(on);
      CALL(SGTD_OK, h, sgtd_consistent_loops(h, 5, fa.data(), fb.data(), rel.data(), nullptr, 0.5, 0.1, n_set.data()), n_set);
      consistent_read(SGTD_OK, 5);
      CALL(SGTD_OK, h, sgtd_consistent_loops(h, n, on ? fa.data() : nullptr, fb.data(), rel.data(), pa.data(), 1.5, 0.2, n_set.data()), n_set);
      consistent_read(SGTD_OK, n);
    }
    timing(0);
    CALL(SGTD_ERR_INVALID, h, sgtd_consistent_loops(h, -1, fa.data(), fb.data(), rel.data(), nullptr, 0.5, 0.1, n_set.data()));
    CALL(SGTD_ERR_INVALID, h, sgtd_consistent_loops(h, 5, nullptr, fb.data(), rel.data(), nullptr, 0.5, 0.1, n_set.data()));
    CALL(SGTD_ERR_INVALID, h, sgtd_consistent_loops(h, 5, fa.data(), fb.data(), rel.data(), nullptr, -1.0, 0.1, n_set.data()));
    CALL(SGTD_ERR_INVALID, h, sgtd_consistent_loops(h, 5, fa.data(), fb.data(), rel.data(), nullptr, 0.5, 4.0, n_set.data()));
    consistent_read(SGTD_OK, n);       // (the results stay)
    CALL(SGTD_ERR_UNSUPPORTED, h, sgtd_consistent_loops(h, (int64_t)SGTD_MAX_LOOP_EDGES + 1, fa.data(), fb.data(), rel.data(), nullptr, 0.5, 0.1, n_set.data()));
    consistent_read(SGTD_ERR_STATE, 5);       // (they are gone)
  }
  void relaxed_read(int expect, int n, int m) {
    std::vector<double> pose((size_t)std::max(n, 1) * 12, -7.0), cost((size_t)std::max(m, 1) * 2, -7.0);
    CALL(expect, h, sgtd_result_relaxed(h, pose.data(), cost.data()), pose, cost);
    CALL(expect, h, sgtd_result_relaxed(h, nullptr, cost.data()), cost);
    CALL(expect, h, sgtd_result_relaxed(h, nullptr, nullptr));
  }
  void relax_poses() {
    note("sgtd_relax_poses");
    const int n = 4, m = 4;
    std::vector<double> pose0((size_t)n * 12, 0.0), meas((size_t)m * 12, 0.0), wt((size_t)m, 2.0), wr((size_t)m, 0.5);
    for (int v = 0; v < n; v++) { pose0[(size_t)v * 12] = pose0[(size_t)v * 12 + 5] = pose0[(size_t)v * 12 + 10] = 1.0; pose0[(size_t)v * 12 + 3] = 1.0 * v; }
    for (int k = 0; k < m; k++) { meas[(size_t)k * 12] = meas[(size_t)k * 12 + 5] = meas[(size_t)k * 12 + 10] = 1.0; meas[(size_t)k * 12 + 3] = 1.0; }
    const int32_t ni[4] = {0, 1, 2, 3}, nj[4] = {1, 2, 3, 0};
    const uint8_t fixed[4] = {1, 0, 0, 1}, all[4] = {1, 1, 1, 1};
    std::vector<sgtd_relax_report> rep(1);
    sgtd_relax_options o;
    sgtd_default_relax_options(&o);
    Env blocks("SGTD_RELAX_MAX_BLOCKS", "2");
    relaxed_read(SGTD_ERR_STATE, n, m);
    CALL(SGTD_OK, h, sgtd_relax_poses(h, n, pose0.data(), nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rep.data()), rep);
    relaxed_read(SGTD_OK, 0, 0);
    CALL(SGTD_OK, h, sgtd_relax_poses(h, n, pose0.data(), nullptr, m, ni, nj, meas.data(), nullptr, nullptr, nullptr, rep.data()), rep);
    relaxed_read(SGTD_OK, n, m);
    o.max_inner = 2;
    CALL(SGTD_OK, h, sgtd_relax_poses(h, n, pose0.data(), fixed, m, ni, nj, meas.data(), wt.data(), wr.data(), &o, nullptr));
    relaxed_read(SGTD_OK, n, m);
    CALL(SGTD_OK, h, sgtd_relax_poses(h, n, pose0.data(), all, m, ni, nj, meas.data(), wt.data(), nullptr, &o, rep.data()), rep);
    // a solve that never ends, in the second group of SGTD_RELAX_GROUP iterations
    S.relax_ends = false;
    o.max_outer = SGTD_RELAX_GROUP + 1;
    CALL(SGTD_ERR_HIP, h, sgtd_relax_poses(h, n, pose0.data(), fixed, m, ni, nj, meas.data(), wt.data(), wr.data(), &o, rep.data()));
    S.relax_ends = true;
    relaxed_read(SGTD_ERR_STATE, n, m);
    CALL(SGTD_OK, h, sgtd_relax_poses(h, n, pose0.data(), fixed, m, ni, nj, meas.data(), wt.data(), wr.data(), &o, rep.data()), rep);
    CALL(SGTD_ERR_INVALID, h, sgtd_relax_poses(h, n, nullptr, fixed, m, ni, nj, meas.data(), nullptr, nullptr, nullptr, nullptr));
    o.cg_tol = 0.0;
    CALL(SGTD_ERR_INVALID, h, sgtd_relax_poses(h, n, pose0.data(), fixed, m, ni, nj, meas.data(), nullptr, nullptr, &o, nullptr));
    CALL(SGTD_ERR_INVALID, h, sgtd_relax_poses(h, n, pose0.data(), fixed, m, ni, ni, meas.data(), nullptr, nullptr, nullptr, nullptr));
    CALL(SGTD_ERR_UNSUPPORTED, h, sgtd_relax_poses(h, (int64_t)SGTD_RELAX_MAX_NODES + 1, pose0.data(), nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    relaxed_read(SGTD_OK, n, m);       // (the results stay)
  }

  // ---- sgtd_pose_consensus_rows, sgtd_pose_consensus
  void consensus_read(int expect, int nq, int cn, bool batch) {
    const size_t m = (size_t)std::max(nq, 1);
    std::vector<double> pose(m * 12, -7.0), support(m, -7.0), t2(m, -7.0), trace(m, -7.0), thr(2, -7.0), best(m, -7.0), rel(m * 12, -7.0);
    std::vector<int32_t> n_valid(m, -7), n_set(m, -7), seed(m, -7), degree((size_t)cn, -7), pick((size_t)cn, -7), cand(m, -7), frame(m, -7), query(m, -7);
    std::vector<uint64_t> mask(m, 7u), rows((size_t)cn, 7u);
    std::vector<uint32_t> fa(m, 7u), fb(m, 7u);
    std::vector<int64_t> cnt(1, -7);
    CALL(expect, h, sgtd_result_consensus(h, 0, nq, pose.data(), n_valid.data(), n_set.data(), seed.data(), mask.data(), support.data(), t2.data(), trace.data(), thr.data()), pose, n_valid, n_set, seed,
         mask, support, t2, trace, thr);
    CALL(expect, h, sgtd_result_consensus(h, 0, nq, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    CALL(nq > 0 ? expect : (expect == SGTD_OK ? SGTD_ERR_INVALID : expect), h, sgtd_result_consensus_rows(h, 0, rows.data(), degree.data(), pick.data()), rows, degree, pick);
    const int choice = expect != SGTD_OK || batch ? expect : SGTD_ERR_STATE;       // (the choice needs the batch form)
    CALL(choice, h, sgtd_search_loop_consensus(h, 1, cand.data(), frame.data(), best.data(), n_set.data()), cand, frame, best, n_set);
    CALL(choice, h, sgtd_result_consensus_edges(h, 2, query.data(), fa.data(), fb.data(), nullptr, best.data(), nq, cnt.data()), query, fa, fb, best, cnt);
    if (expect != SGTD_OK) return;
    if (nq > 1) {
      CALL(SGTD_OK, h, sgtd_result_consensus(h, 1, nq - 1, pose.data(), nullptr, n_set.data(), nullptr, nullptr, nullptr, t2.data(), nullptr, nullptr), pose, n_set, t2);
      CALL(SGTD_OK, h, sgtd_result_consensus_rows(h, nq - 1, nullptr, nullptr, nullptr));
    }
    CALL(SGTD_OK, h, sgtd_result_consensus(h, nq, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, thr.data()), thr);
    CALL(SGTD_ERR_INVALID, h, sgtd_result_consensus(h, 0, nq + 1, pose.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    CALL(SGTD_ERR_INVALID, h, sgtd_result_consensus_rows(h, nq, rows.data(), nullptr, nullptr));
    if (batch && cnt[0] > 0) CALL(SGTD_ERR_CAPACITY, h, sgtd_result_consensus_edges(h, 2, query.data(), nullptr, fb.data(), nullptr, nullptr, cnt[0] - 1, cnt.data()), query, fb, cnt);
  }
  void pose_consensus() {
    note("sgtd_pose_consensus_rows");
    const int nq = 3, cn = 4;
    std::vector<int32_t> n_cand = {4, 0, 1}, frame((size_t)nq * cn);
    std::vector<double> score((size_t)nq * cn), rel((size_t)nq * cn * 12, 0.0);
    for (int i = 0; i < nq * cn; i++) { frame[(size_t)i] = i % 6; score[(size_t)i] = 0.5 + 0.01 * i; rel[(size_t)i * 12] = rel[(size_t)i * 12 + 5] = rel[(size_t)i * 12 + 10] = 1.0; rel[(size_t)i * 12 + 3] = 0.1 * i; }
    consensus_read(SGTD_ERR_STATE, nq, cn, false);
    CALL(SGTD_OK, h, sgtd_pose_consensus_rows(h, 0, cn, nullptr, nullptr, nullptr, nullptr, 0.5, 0.1));
    consensus_read(SGTD_OK, 0, cn, false);
    CALL(SGTD_OK, h, sgtd_pose_consensus_rows(h, nq, cn, n_cand.data(), frame.data(), score.data(), rel.data(), 0.5, 0.1));
    consensus_read(SGTD_OK, nq, cn, false);
    CALL(SGTD_ERR_UNSUPPORTED, h, sgtd_pose_consensus_rows(h, (int64_t)0x7FFFFFFF / SGTD_MAX_CAND + 1, cn, n_cand.data(), frame.data(), score.data(), rel.data(), 0.5, 0.1));
    consensus_read(SGTD_ERR_STATE, nq, cn, false);
    CALL(SGTD_OK, h, sgtd_pose_consensus_rows(h, nq, cn, n_cand.data(), frame.data(), score.data(), rel.data(), 0.5, 0.1));
    CALL(SGTD_ERR_INVALID, h, sgtd_pose_consensus_rows(h, nq, SGTD_MAX_CAND + 1, n_cand.data(), frame.data(), score.data(), rel.data(), 0.5, 0.1));
    CALL(SGTD_ERR_INVALID, h, sgtd_pose_consensus_rows(h, nq, cn, n_cand.data(), nullptr, score.data(), rel.data(), 0.5, 0.1));
    consensus_read(SGTD_ERR_STATE, nq, cn, false);      // (an invalid call takes the results with it)

    // the batch form: a table, a batch of frames, its verification (the candidate tables and scores of the stages' scenario)
    note("sgtd_pose_consensus");
    S.stages = true; S.expect_order = -1;
    const int n_frames = 130, bq = 5, bcn = cfg.candidate_num;
    for (int f = 0; f < n_frames; f++) { Descs d = random_descs(rng, 60, (uint32_t)f); sgtd_desc_soa s = d.soa(); OK(sgtd_add(h, &s, 60)); }
    OK(sgtd_finalize(h));
    std::vector<uint32_t> ids;
    std::vector<float> poses;
    for (int f = 0; f < n_frames; f++) { ids.push_back((uint32_t)f); for (int i = 0; i < 12; i++) poses.push_back(i % 5 == 0 ? 1.f : (i % 4 == 3 ? 0.5f * f : 0.f)); }
    CALL(SGTD_OK, h, sgtd_set_frame_poses(h, ids.data(), poses.data(), (int64_t)ids.size()));
    Keypoints kp;
    for (int q = 0; q < bq; q++) kp.add(rng, 12 + q);
    CALL(SGTD_OK, h, sgtd_query_frames(h, kp.xyz.data(), kp.label.data(), kp.off.data(), bq, 0));
    CALL(SGTD_ERR_STATE, h, sgtd_pose_consensus(h, 0.5, 0.1, 0));
    CALL(SGTD_OK, h, sgtd_verify(h));
    CALL(SGTD_ERR_STATE, h, sgtd_pose_consensus(h, 0.5, 0.1, SGTD_CONSENSUS_REFINED));
    CALL(SGTD_ERR_STATE, h, sgtd_pose_consensus(h, 0.5, 0.1, SGTD_CONSENSUS_ALIGNED));
    CALL(SGTD_ERR_INVALID, h, sgtd_pose_consensus(h, 0.5, 0.1, SGTD_CONSENSUS_REFINED | SGTD_CONSENSUS_ALIGNED));
    CALL(SGTD_ERR_INVALID, h, sgtd_pose_consensus(h, 0.5, -0.1, 0));
    consensus_read(SGTD_ERR_STATE, bq, bcn, true);
    CALL(SGTD_OK, h, sgtd_pose_consensus(h, 0.5, 0.1, 0));
    consensus_read(SGTD_OK, bq, bcn, true);
    CALL(SGTD_OK, h, sgtd_refine_poses(h, 1));
    CALL(SGTD_OK, h, sgtd_pose_consensus(h, 0.75, 0.2, SGTD_CONSENSUS_REFINED));
    consensus_read(SGTD_OK, bq, bcn, true);
    CALL(SGTD_OK, h, sgtd_align_keypoints(h, 0.5, 2, 0, nullptr, nullptr, nullptr));
    CALL(SGTD_OK, h, sgtd_pose_consensus(h, 0.75, 0.2, SGTD_CONSENSUS_ALIGNED));
    consensus_read(SGTD_OK, bq, bcn, true);
    // the consistency pass over the store's poses, ids outside it among the edges
    {
      const uint32_t fa[4] = {0, 3, 129, 500}, fb[4] = {7, 9, 2, 1};
      std::vector<double> r4(4 * 12, 0.0);
      for (int k = 0; k < 4; k++) r4[(size_t)k * 12] = r4[(size_t)k * 12 + 4] = r4[(size_t)k * 12 + 8] = 1.0;
      std::vector<int32_t> n_set(1, -7);
      CALL(SGTD_OK, h, sgtd_consistent_loops(h, 4, fa, fb, r4.data(), nullptr, 0.5, 0.1, n_set.data()), n_set);
      consistent_read(SGTD_OK, 4);
    }
    // a new batch takes the batch form's results with it
    CALL(SGTD_OK, h, sgtd_query_frames(h, kp.xyz.data(), kp.label.data(), kp.off.data(), bq, 0));
    consensus_read(SGTD_ERR_STATE, bq, bcn, true);
    S.stages = false;
  }

  void run(int n_dev_) {
    n_dev = n_dev_;
    if (g_transcript) fprintf(g_transcript, "# ---- the cloud and graph stages on %d device(s)\n", n_dev);
    if (n_dev == 1) OK(sgtd_create(&cfg, &h));
    else { const int ids[2] = {0, 0}; OK(sgtd_create_multi(&cfg, ids, 2, &h)); }
    g_last = h;
    register_clouds();
    register_voxels();
    scan_keypoints();
    local_map_keypoints();
    consistent_loops();
    relax_poses();
    pose_consensus();
    OK(sgtd_destroy(h));
    h = nullptr; g_last = nullptr;
  }

  // every kernel these stages can launch was launched (lm_gather_kernel in its three forms)
  static void check_coverage() {
    const struct { const char *kernel; int forms; } want[] = {
        {"reg_cov_kernel", 1}, {"reg_init_kernel", 1}, {"reg_search_kernel", 1}, {"reg_match_kernel", 1}, {"reg_lin_kernel", 1}, {"reg_trial_kernel", 1}, {"reg_final_kernel", 1},
        {"vreg_keys_kernel", 1}, {"vreg_ranges_kernel", 1}, {"vreg_voxel_kernel", 1}, {"vreg_init_kernel", 1}, {"vreg_corr_kernel", 1}, {"vreg_lin_kernel", 1}, {"vreg_trial_kernel", 1},
        {"vreg_final_kernel", 1}, {"scan_init_kernel", 1}, {"scan_point_kernel", 1}, {"scan_rings_kernel", 1}, {"scan_keys_kernel", 1}, {"scan_heads_kernel", 1}, {"scan_voxels_kernel", 1},
        {"scan_links_kernel", 1}, {"scan_hook_kernel", 1}, {"scan_jump_kernel", 1}, {"scan_component_kernel", 1}, {"scan_cluster_keys_kernel", 1}, {"scan_offsets_kernel", 1},
        {"scan_cluster_ids_kernel", 1}, {"scan_point_clusters_kernel", 1}, {"scan_sum_wave_kernel", 1}, {"scan_sum_block_kernel", 1}, {"lm_members_kernel", 1}, {"lm_segments_kernel", 1},
        {"lm_gather_kernel", 3}, {"cons_prepare_kernel", 1}, {"cons_pair_kernel", 1}, {"cons_init_kernel", 1}, {"cons_count_kernel", 1}, {"cons_select_kernel", 1}, {"consensus_kernel", 1},
        {"relax_init_kernel", 1}, {"relax_edge_kernel", 1}, {"relax_ctl_kernel", 1}, {"relax_setup_kernel", 1}, {"relax_cg_edge_kernel", 1}, {"relax_cg_node_kernel", 1},
        {"relax_cg_update_kernel", 1}, {"relax_retract_kernel", 1}};
    for (const auto &w : want) {
      int n = 0;
      for (const std::string &k : g_launched) n += names(k.c_str(), w.kernel);
      if (n != w.forms) { fprintf(stderr, "engine_driver: %d forms of %s launched, not %d\n", n, w.kernel, w.forms); exit(1); }
    }
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

  // ---- sgtd_remove_frames: every field compacted into a scratch buffer that takes the field's place; the old buffers, the keep
  // masks and the tile counts are freed by the call, the two bitmaps stay with the handle
  {
    sgtd_handle t = nullptr;
    OK(sgtd_create(&cfg, &t));
    for (int f = 0; f < 4; f++) { Descs d = random_descs(rng, 300, (uint32_t)f); sgtd_desc_soa s = d.soa(); OK(sgtd_add(t, &s, 300)); }
    const size_t blocks = sgtd_stub_device_blocks();
    const uint32_t gone[2] = {1, 900};          // (900: outside the table's frames)
    int64_t removed = -1;
    OK(sgtd_remove_frames(t, gone, 2, &removed));
    REQUIRE(removed == 1200 - 2 * (1200 / 4) && sgtd_stub_device_blocks() == blocks + 2);
    OK(sgtd_get_stats(t, &st));
    REQUIRE(st.n_entries == 1200 - removed);
    OK(sgtd_destroy(t));
  }

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

  // ---- the cloud and graph stages, launch by launch, on one device and on two "devices" behind one handle
  {
    g_launched.clear();
    g_tracing = true;
    sgtd_stub_set_trace(g_transcript);
    for (int n_dev : {1, 2}) { CloudStages cs{S, rng, cfg}; cs.run(n_dev); }
    sgtd_stub_set_trace(nullptr);
    g_tracing = false;
    CloudStages::check_coverage();
    printf("cloud and graph stages: %zu kernel forms launched\n", g_launched.size());
  }
  g_last = nullptr;
  if (g_transcript) fclose(g_transcript);
  REQUIRE(sgtd_stub_device_blocks() == 0 && sgtd_stub_device_bytes() == 0);       // every device buffer was freed
  printf("engine host code under the sanitizers: ok (%llu launches, %llu sweeps, %llu frame packs, device peak %.1f MB)\n",
         sgtd_stub_launches(), S.sweeps, S.packs, sgtd_stub_device_peak() / 1048576.0);
  return 0;
}
