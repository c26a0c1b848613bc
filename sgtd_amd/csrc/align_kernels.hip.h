// align_kernels.hip.h — label-aware closest-keypoint alignment of every verified candidate (sgtd_align_keypoints; the
// rule is stated in include/sgtd_accel.h, DESIGN.md has the LDS budget).
//
// sgtd_overlap measures how well a candidate's pose puts the query's keypoints onto the keypoints of the candidate's
// frame; this pass reduces that distance: assign every query keypoint to the nearest frame keypoint of its label within
// `radius`, refit the pose over the assigned pairs, and again until the assignment stops changing.  One 256-thread
// workgroup per (query, candidate), in candidate-frame order:
//   walk        overlap_kernel's walk (overlap_walk, the frame's keypoints in LDS tiles, broadcast reads) with the index
//               of the minimum kept beside it.  Thread l owns the query keypoints i = l, l + 256, ...; their assignment
//               lives in LDS (SGTD_ALIGN_CAP keypoints) or, for a longer query, in the workgroup's slice of the handle's
//               assignment buffer — the slice the result is handed out from, so nothing is copied at the end.  Only
//               the owner touches an entry.  Every walk is a whole evaluation of sgtd_overlap's rule (the hit bytes, the
//               counts, the ordered sum): the first is the "before" result, the last the "after" result.
//   fit         centroid sums, then the covariance about the centroids, each as 256 per-thread accumulators combined by
//               refine_tree; thread 0 solves the 3x3 problem (refine_solve: svd3_dev, V U^T, the K correction).  The
//               positions come from memory again in each pass (28 B a pair, from cache).
//   stop        fewer than 3 assigned keypoints, or an assignment equal to the one before (a workgroup-wide OR of the
//               threads' change flags), or the iteration count.
// No atomics; every sum's order is a function of keypoint indices only.  Arithmetic: f64, -ffp-contract=off.
#pragma once
#include "common.hip.h"
#include "overlap_kernels.hip.h"

#define SGTD_ALIGN_THREADS 256
#define SGTD_ALIGN_CAP 1024          // query keypoints whose assignment is held in LDS: 4 KB
#define SGTD_ALIGN_HEAD 9728         // bytes ahead of the tile: refine_tree's [9][128] + [64] doubles (the scan's words inside)

struct AlignParams {
  // the batch's candidates and their verification results
  const int *n_cand;
  const int *cand_frame;
  int cand_num;
  const double *score;
  const double *pose;                // the start pose: sgtd_verify's, or sgtd_refine_poses'
  // the query keypoints: xyz[3 i], label[i], query q's are q_off[q] .. q_off[q + 1]
  const float *q_xyz;
  const u32 *q_label;
  const long long *q_off;
  // the keypoint store's device copy
  const uint4 *kp;
  const u64 *f_word;                 // [n_ids]
  u32 n_ids;
  u32 hit_off, asg_off;              // byte offsets of the hit bytes and of the assignment in dynamic LDS
  double rr;
  int iterations;
  const u32 *order;                  // or NULL: the (query, candidate) indices in dispatch order (verify_order_keys_kernel)
  u32 n_blocks;
  // results, [nq * cand_num] each
  double *o_pose;                    // [.][12]
  int4 *fit;                         // n_fits, n_corr, stop, 0
  int4 *cnt;                         // [.][2]: sgtd_overlap's four counts before, after
  double *val;                       // [.][4]: overlap, rms before; overlap, rms after
  double *moments;                   // [.][15]
  int *assign;                       // candidate c of query q: cand_num * (q_off[q] - q_off[0]) + c * n_query_kp, n_query_kp entries
};

// dynamic LDS of a launch over a store whose longest frame has max_kp keypoints
inline size_t align_hit_off(int max_kp) { return (size_t)SGTD_ALIGN_HEAD + overlap_tile_slots(max_kp) * sizeof(uint4); }
inline size_t align_asg_off(int max_kp) { return align_hit_off(max_kp) + (((size_t)std::max(max_kp, 1) + 15) & ~(size_t)15); }
inline size_t align_lds_bytes(int max_kp) { return align_asg_off(max_kp) + (size_t)SGTD_ALIGN_CAP * sizeof(int); }

__global__ __launch_bounds__(SGTD_ALIGN_THREADS) void align_kernel(AlignParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char align_smem[];
  double *red = reinterpret_cast<double *>(align_smem);                         // [9][128]
  double *bc = red + 9 * 128;                                                   // [64]: totals, then the pose
  u32 *scan = reinterpret_cast<u32 *>(bc + 32);                                 // [<= 8] (behind the pose's 12)
  uint4 *tile = reinterpret_cast<uint4 *>(align_smem + SGTD_ALIGN_HEAD);
  unsigned char *hit = align_smem + P.hit_off;
  const int tid = threadIdx.x;
  const u32 blk = P.order ? P.order[blockIdx.x] : blockIdx.x;
  if (blk >= P.n_blocks) return;
  const int q = (int)(blk / (u32)P.cand_num), c = (int)(blk % (u32)P.cand_num);
  const double nan = __builtin_nan("");
  const long long q0 = P.q_off[q];
  const int nqk = (int)(P.q_off[q + 1] - q0);
  int *o_asg = P.assign + (size_t)(q0 - P.q_off[0]) * (size_t)P.cand_num + (size_t)c * (size_t)nqk;
  double *o_pose = P.o_pose + (size_t)blk * 12, *o_mom = P.moments + (size_t)blk * 15, *o_val = P.val + (size_t)blk * 4;
  if (c >= P.n_cand[q] || !(P.score[blk] >= 0.0)) {        // no verification result
    if (tid < 12) o_pose[tid] = 0.0;
    if (tid < 15) o_mom[tid] = nan;
    if (tid < 4) o_val[tid] = nan;
    if (tid < 2) P.cnt[(size_t)blk * 2 + tid] = make_int4(-1, -1, -1, -1);
    if (tid == 0) P.fit[blk] = make_int4(0, 0, -1, 0);
    for (int i = tid; i < nqk; i += SGTD_ALIGN_THREADS) o_asg[i] = -1;
    return;
  }
  double Rt[12], mom[15];
#pragma unroll
  for (int k = 0; k < 12; k++) Rt[k] = P.pose[(size_t)blk * 12 + k];
  const u32 frame = (u32)P.cand_frame[blk];
  const u64 word = frame < P.n_ids ? P.f_word[frame] : SGTD_OVERLAP_NONE;
  if (word == SGTD_OVERLAP_NONE) {                         // the frame has no stored keypoints: the start pose stands
    if (tid < 12) o_pose[tid] = Rt[tid];
    if (tid < 15) o_mom[tid] = nan;
    if (tid < 4) o_val[tid] = nan;
    if (tid < 2) P.cnt[(size_t)blk * 2 + tid] = make_int4(nqk, -1, 0, 0);
    if (tid == 0) P.fit[blk] = make_int4(0, 0, 1, 0);
    for (int i = tid; i < nqk; i += SGTD_ALIGN_THREADS) o_asg[i] = -1;
    return;
  }
  const int nf = (int)(word & 0xFFFFull);
  const uint4 *kp = P.kp + (size_t)(word >> 16);
  const double rr = P.rr;
  const bool in_lds = nqk <= SGTD_ALIGN_CAP;
  int *asg = in_lds ? reinterpret_cast<int *>(align_smem + P.asg_off) : o_asg;
  const int rounds = (nqk + SGTD_ALIGN_THREADS - 1) / SGTD_ALIGN_THREADS;
  const float *qx = P.q_xyz + (size_t)q0 * 3;
  const u32 *ql = P.q_label + (size_t)q0;

  u32 n_hit_q = 0, n_hit_f = 0, n_asg = 0;     // of the last walk
  double sum_m = 0.0;
  bool changed = true;
  // the assignment under Rt and, with it, sgtd_overlap's evaluation under Rt
  auto walk = [&](bool first) {
    __syncthreads();                           // the hit bytes' last readers are done
    for (int j = tid; j < nf; j += SGTD_ALIGN_THREADS) hit[j] = 0;
    double acc = 0.0;                          // accumulator `tid` of SUM(m_i over hit i)
    u32 nh = 0, na = 0;
    int ch = 0;
    for (int r = 0; r < rounds; r++) {
      const int i = r * SGTD_ALIGN_THREADS + tid;
      const bool active = i < nqk;
      double x[3] = {0.0, 0.0, 0.0};
      u32 lab = 0;
      if (active) {
        const double p[3] = {(double)qx[(size_t)i * 3], (double)qx[(size_t)i * 3 + 1], (double)qx[(size_t)i * 3 + 2]};
        lab = ql[i];
#pragma unroll
        for (int a = 0; a < 3; a++) x[a] = ((Rt[a * 3] * p[0] + Rt[a * 3 + 1] * p[1]) + Rt[a * 3 + 2] * p[2]) + Rt[9 + a];
      }
      double m = __builtin_inf();
      int bj = -1;
      overlap_walk<true>(kp, nf, true, tile, hit, active, x, lab, rr, m, bj);
      if (active) {
        if (m <= rr) { acc += m; nh++; }
        const int a = (bj >= 0 && m <= rr) ? bj : -1;
        if (!first && asg[i] != a) ch = 1;
        asg[i] = a;
        na += a >= 0 ? 1u : 0u;
      }
    }
    __syncthreads();
    u32 fh = 0;
    for (int j = tid; j < nf; j += SGTD_ALIGN_THREADS) fh += hit[j];
    (void)block_excl_scan(nh, scan, n_hit_q);
    (void)block_excl_scan(fh, scan, n_hit_f);
    (void)block_excl_scan(na, scan, n_asg);
    double s[1] = {acc};
    refine_tree<1>(s, red, bc);
    sum_m = s[0];
    changed = first || __syncthreads_or(ch) != 0;
  };
  auto store_eval = [&](int which) {
    if (tid == 0) {
      P.cnt[(size_t)blk * 2 + which] = make_int4(nqk, nf, (int)n_hit_q, (int)n_hit_f);
      o_val[which * 2] = nqk > 0 ? (double)n_hit_q / (double)nqk : nan;
      o_val[which * 2 + 1] = n_hit_q > 0 ? sqrt(sum_m / (double)n_hit_q) : nan;
    }
  };
  // f(p, w) for every assigned keypoint this thread owns, in ascending keypoint index
  auto for_my_pairs = [&](auto &&f) {
    for (int i = tid; i < nqk; i += SGTD_ALIGN_THREADS) {
      const int a = asg[i];
      if (a < 0) continue;
      const uint4 k = kp[a];
      const double p[3] = {(double)qx[(size_t)i * 3], (double)qx[(size_t)i * 3 + 1], (double)qx[(size_t)i * 3 + 2]};
      const double w[3] = {(double)__uint_as_float(k.x), (double)__uint_as_float(k.y), (double)__uint_as_float(k.z)};
      f(p, w);
    }
  };

  walk(true);
  store_eval(0);
  int n_fits = 0, n_corr = 0, stop = 0;
#pragma unroll
  for (int k = 0; k < 15; k++) mom[k] = nan;
  for (int it = 1; it <= P.iterations; it++) {
    if (n_asg < 3u) { stop = 1; break; }
    if (it >= 2 && !changed) { stop = 2; break; }
    const double cnt = (double)n_asg;
    double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for_my_pairs([&](const double (&p)[3], const double (&w)[3]) {
#pragma unroll
      for (int i = 0; i < 3; i++) { sums[i] += p[i]; sums[3 + i] += w[i]; }
    });
    refine_tree<6>(sums, red, bc);
#pragma unroll
    for (int i = 0; i < 6; i++) mom[i] = sums[i] / cnt;
    double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for_my_pairs([&](const double (&p)[3], const double (&w)[3]) {
      double dp[3], dw[3];
#pragma unroll
      for (int i = 0; i < 3; i++) { dp[i] = p[i] - mom[i]; dw[i] = w[i] - mom[3 + i]; }
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) H[i * 3 + j] += dp[i] * dw[j];
    });
    refine_tree<9>(H, red, bc);
#pragma unroll
    for (int i = 0; i < 9; i++) mom[6 + i] = H[i];
    if (tid == 0) refine_solve(H, mom, bc);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 12; k++) Rt[k] = bc[k];
    __syncthreads();
    n_fits++;
    n_corr = (int)n_asg;
    walk(false);
  }
  store_eval(1);
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 12; k++) o_pose[k] = Rt[k];
#pragma unroll
    for (int k = 0; k < 15; k++) o_mom[k] = mom[k];
    P.fit[blk] = make_int4(n_fits, n_corr, stop, 0);
  }
  if (in_lds)
    for (int i = tid; i < nqk; i += SGTD_ALIGN_THREADS) o_asg[i] = asg[i];
}
