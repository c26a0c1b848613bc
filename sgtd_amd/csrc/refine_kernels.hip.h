// refine_kernels.hip.h — least-squares refit of every verified candidate's relative pose over ALL its inlier pairs
// (sgtd_refine_poses; the rule is stated in include/sgtd_accel.h, DESIGN.md has the byte model).
//
// sgtd_verify's pose is the rigid motion of ONE triangle pair (candidate_verify's best hypothesis, STDesc.cpp:516-522,
// :549-571).  Its inlier set — tens to thousands of vertex correspondences per (query, candidate) — is already on the
// device as one flag byte per pair of the match list.  One 256-thread workgroup per (query, candidate):
//   gather      thread l owns the list positions j = l, l + 256, ... (the summation order of the rule: accumulator l).  It
//               reads their flag bytes and, for the flagged ones, the pair word and the 9 + 9 f32 vertex values of the query
//               descriptor and the table entry — 72 B of scattered reads per inlier pair, the expensive part — ONCE, into
//               LDS (structure of arrays: value k of slot s at lds[k * CAP + s], a thread's slots consecutive, the threads'
//               segments in thread order).  A set of more than SGTD_REFINE_CAP pairs stays in memory and is gathered by
//               every pass again.
//   fit         centroid sums, then the 3x3 covariance about the centroids, each as 256 per-thread accumulators combined
//               by the balanced tree acc[l] += acc[l + s], s = 128 ... 1 (s = 128, 64 through LDS, the rest as wave
//               shuffles: the same additions in the same order); thread 0 solves the 3x3 problem exactly as
//               triangle_solver does (svd3_dev, V U^T, the K correction).
//   re-select   (iterations > 1) the whole list streamed once more: every pair whose three vertices pass vertex_close
//               under the last pose; the flags go to the handle's own buffer (two halves, written alternately — the
//               previous set is needed to detect an unchanged one and to fall back on), never to sgtd_verify's.
//   residuals   of the final set under the refined pose and under sgtd_verify's, from the same LDS image.
// No atomics; every sum's order is a function of list positions only.  Arithmetic: f64, -ffp-contract=off.
#pragma once
#include "common.hip.h"
#include "verify_kernels.hip.h"

#define SGTD_REFINE_THREADS 256
#define SGTD_REFINE_CAP 896          // inlier pairs held in LDS: 896 * 72 B = 63 KB; with the reduction scratch two workgroups per CU
#define SGTD_REFINE_RED 9            // doubles reduced at once (the covariance)

struct RefineParams {
  // the batch's lists and sgtd_verify's results (VerifyParams' members of the same names)
  const u64 *pairs;
  const long long *pair_off;
  const u32 *q_pair_base;
  const int *n_cand;
  int cand_num;
  long long q_stride;
  const float *q_vertex;
  const float *t_vertex;
  const double *score;
  const double *v_pose;
  const unsigned char *v_inlier;     // set 0 (read only)
  // the handle's own flags: two halves of `flag_half` bytes, indexed like v_inlier
  unsigned char *flag;
  size_t flag_half;
  double thr2;
  int iterations;
  const u32 *order;                  // or NULL: the (query, candidate) indices in dispatch order (verify_order_keys_kernel)
  u32 n_blocks;
  // results, [nq * cand_num] each
  double *pose;                      // [.][12]
  double *rmse, *rmse_verify;
  int *n_pairs;
  double *moments;                   // [.][15]
};

inline size_t refine_lds_bytes() {
  return (size_t)SGTD_REFINE_CAP * 18 * sizeof(float) + (size_t)SGTD_REFINE_RED * 128 * sizeof(double) + 64 * sizeof(double);
}

// acc[l] += acc[l + s] for s = 128, 64, ..., 1 over the workgroup's 256 values of each of N quantities; the totals come
// back in every thread.  red: [N][128] doubles, bc: [>= N] doubles.
template <int N>
__device__ __forceinline__ void refine_tree(double (&v)[N], double *red, double *bc) {
  const int tid = threadIdx.x;
  if (tid >= 128) {
#pragma unroll
    for (int k = 0; k < N; k++) red[k * 128 + (tid - 128)] = v[k];
  }
  __syncthreads();
  if (tid < 128) {
#pragma unroll
    for (int k = 0; k < N; k++) v[k] += red[k * 128 + tid];
  }
  __syncthreads();
  if (tid >= 64 && tid < 128) {
#pragma unroll
    for (int k = 0; k < N; k++) red[k * 128 + (tid - 64)] = v[k];
  }
  __syncthreads();
  if (tid < 64) {
#pragma unroll
    for (int k = 0; k < N; k++) {
      double x = v[k] + red[k * 128 + tid];
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) x += __shfl_down(x, s);      // (lanes >= s add values nobody uses)
      if (tid == 0) bc[k] = x;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; k++) v[k] = bc[k];
  __syncthreads();
}

// the 3x3 solve (triangle_solver's, :558-569) of a fit with covariance H about the centroids mom = cp, cw:
// out[0..8] = rot row-major, out[9..11] = t
__device__ inline void refine_solve(const double (&H)[9], const double *mom, double *out) {
  double cov[3][3], U[3][3], V[3][3], UT[3][3], rot[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) cov[i][j] = H[i * 3 + j];
  svd3_dev(cov, U, V);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) UT[i][j] = U[j][i];
  mul3(V, UT, rot);
  const double det = rot[0][0] * (rot[1][1] * rot[2][2] - rot[1][2] * rot[2][1]) -
                     rot[0][1] * (rot[1][0] * rot[2][2] - rot[1][2] * rot[2][0]) +
                     rot[0][2] * (rot[1][0] * rot[2][1] - rot[1][1] * rot[2][0]);
  if (det < 0) {
    double K[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, -1}}, VK[3][3];
    mul3(V, K, VK);
    mul3(VK, UT, rot);
  }
  for (int r = 0; r < 3; r++) {
    for (int k = 0; k < 3; k++) out[r * 3 + k] = rot[r][k];
    out[9 + r] = -(rot[r][0] * mom[0] + rot[r][1] * mom[1] + rot[r][2] * mom[2]) + mom[3 + r];
  }
}

__global__ __launch_bounds__(SGTD_REFINE_THREADS) void refine_kernel(RefineParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char refine_smem[];
  float *rec = reinterpret_cast<float *>(refine_smem);                                        // [18][CAP]
  double *red = reinterpret_cast<double *>(refine_smem + (size_t)SGTD_REFINE_CAP * 18 * sizeof(float));   // [RED][128]
  double *bc = red + SGTD_REFINE_RED * 128;                                                   // [64]: totals, then the pose
  u32 *scan = reinterpret_cast<u32 *>(bc + 32);                                               // [<= 8] (behind the pose's 12)
  const int tid = threadIdx.x;
  const u32 blk = P.order ? P.order[blockIdx.x] : blockIdx.x;
  if (blk >= P.n_blocks) return;
  const int q = (int)(blk / (u32)P.cand_num), c = (int)(blk % (u32)P.cand_num);
  double *o_pose = P.pose + (size_t)blk * 12, *o_mom = P.moments + (size_t)blk * 15;
  if (c >= P.n_cand[q] || !(P.score[blk] >= 0.0)) {        // no verification result: zeros, NaN, 0 pairs
    const double nan = __builtin_nan("");
    if (tid < 12) o_pose[tid] = 0.0;
    if (tid < 15) o_mom[tid] = nan;
    if (tid == 0) { P.rmse[blk] = nan; P.rmse_verify[blk] = nan; P.n_pairs[blk] = 0; }
    return;
  }
  const long long *po = P.pair_off + (size_t)q * (P.cand_num + 1);
  const size_t base = (size_t)P.q_pair_base[q] + (size_t)po[c];
  const long long n_list = po[c + 1] - po[c];
  const u64 *pairs = P.pairs + base;
  const size_t qslot0 = (size_t)q * (size_t)P.q_stride;

  const unsigned char *cur = P.v_inlier + base;      // the current set's flags
  u32 n_set = 0;                                     // its pairs
  bool in_lds = false;
  u32 seg_lo = 0, seg_n = 0;                         // this thread's slots of the LDS image
  double Rt[12], mom[15];

  // the 18 vertex values of list position j: p = the query descriptor's A, B, C, w = the table entry's
  auto load_pair = [&](long long j, float (&v)[18]) {
    const u64 pr = pairs[j];
    const float *qv = P.q_vertex + (qslot0 + (size_t)(pr >> 32)) * 9, *tv = P.t_vertex + (size_t)(pr & 0xFFFFFFFFull) * 9;
#pragma unroll
    for (int k = 0; k < 9; k++) { v[k] = qv[k]; v[9 + k] = tv[k]; }
  };
  // f(v) for every pair of the current set this thread owns, in ascending list position
  auto for_my_pairs = [&](auto &&f) {
    float v[18];
    if (in_lds) {
      for (u32 s = seg_lo; s < seg_lo + seg_n; s++) {
#pragma unroll
        for (int k = 0; k < 18; k++) v[k] = rec[k * SGTD_REFINE_CAP + s];
        f(v);
      }
    } else {
      for (long long j = tid; j < n_list; j += SGTD_REFINE_THREADS)
        if (cur[j]) { load_pair(j, v); f(v); }
    }
  };

  for (int it = 1;; it++) {
    // ---- the current set into LDS (when it fits)
    u32 mine = 0;
    for (long long j = tid; j < n_list; j += SGTD_REFINE_THREADS) mine += cur[j] ? 1u : 0u;
    u32 tot;
    seg_lo = block_excl_scan(mine, scan, tot);
    seg_n = mine;
    n_set = tot;
    in_lds = tot <= SGTD_REFINE_CAP;
    if (in_lds) {
      u32 s = seg_lo;
      for (long long j = tid; j < n_list; j += SGTD_REFINE_THREADS)
        if (cur[j]) {
          float v[18];
          load_pair(j, v);
#pragma unroll
          for (int k = 0; k < 18; k++) rec[k * SGTD_REFINE_CAP + s] = v[k];
          s++;
        }
    }
    __syncthreads();
    // ---- centroids
    const double n3 = (double)(3ull * (unsigned long long)n_set);
    double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for_my_pairs([&](const float (&v)[18]) {
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
        for (int i = 0; i < 3; i++) { sums[i] += (double)v[a * 3 + i]; sums[3 + i] += (double)v[9 + a * 3 + i]; }
    });
    refine_tree<6>(sums, red, bc);
#pragma unroll
    for (int i = 0; i < 6; i++) mom[i] = sums[i] / n3;
    // ---- covariance about them
    double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for_my_pairs([&](const float (&v)[18]) {
#pragma unroll
      for (int a = 0; a < 3; a++) {
        double dp[3], dw[3];
#pragma unroll
        for (int i = 0; i < 3; i++) { dp[i] = (double)v[a * 3 + i] - mom[i]; dw[i] = (double)v[9 + a * 3 + i] - mom[3 + i]; }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 3; j++) H[i * 3 + j] += dp[i] * dw[j];
      }
    });
    refine_tree<9>(H, red, bc);
#pragma unroll
    for (int i = 0; i < 9; i++) mom[6 + i] = H[i];
    // ---- the 3x3 solve (triangle_solver's, :558-569) by thread 0
    if (tid == 0) refine_solve(H, mom, bc);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 12; k++) Rt[k] = bc[k];
    __syncthreads();
    if (it >= P.iterations) break;
    // ---- the next set: every pair of the list whose three vertices are close under this pose
    unsigned char *nxt = P.flag + (size_t)(it & 1) * P.flag_half + base;
    u32 cnt[2] = {0u, 0u};      // pairs of the next set, pairs whose flag changes
    for (long long j = tid; j < n_list; j += SGTD_REFINE_THREADS) {
      float v[18];
      load_pair(j, v);
      bool in = true;
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const double p[3] = {(double)v[a * 3], (double)v[a * 3 + 1], (double)v[a * 3 + 2]};
        const double w[3] = {(double)v[9 + a * 3], (double)v[9 + a * 3 + 1], (double)v[9 + a * 3 + 2]};
        in = in && vertex_close(Rt, p, w, P.thr2);
      }
      nxt[j] = in ? 1 : 0;
      cnt[0] += in ? 1u : 0u;
      cnt[1] += (in != (cur[j] != 0)) ? 1u : 0u;
    }
    u32 n_next, n_changed;
    (void)block_excl_scan(cnt[0], scan, n_next);
    (void)block_excl_scan(cnt[1], scan, n_changed);
    if (n_next < 4u || n_changed == 0u) break;      // the previous result stands (and its set is the LDS image)
    __threadfence_block();
    cur = nxt;
  }

  // ---- residuals of the final set: the refined pose, and sgtd_verify's
  double Vt[12];
  for (int k = 0; k < 12; k++) Vt[k] = P.v_pose[(size_t)blk * 12 + k];
  double ss[2] = {0.0, 0.0};
  for_my_pairs([&](const float (&v)[18]) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double p[3] = {(double)v[a * 3], (double)v[a * 3 + 1], (double)v[a * 3 + 2]};
      const double w[3] = {(double)v[9 + a * 3], (double)v[9 + a * 3 + 1], (double)v[9 + a * 3 + 2]};
#pragma unroll
      for (int m = 0; m < 2; m++) {
        const double *T = m ? Vt : Rt;
        const double px = (T[0] * p[0] + T[1] * p[1] + T[2] * p[2]) + T[9];
        const double py = (T[3] * p[0] + T[4] * p[1] + T[5] * p[2]) + T[10];
        const double pz = (T[6] * p[0] + T[7] * p[1] + T[8] * p[2]) + T[11];
        const double dx = px - w[0], dy = py - w[1], dz = pz - w[2];
        ss[m] += (dx * dx + dy * dy) + dz * dz;
      }
    }
  });
  refine_tree<2>(ss, red, bc);
  const double n3 = (double)(3ull * (unsigned long long)n_set);
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 12; k++) o_pose[k] = Rt[k];
#pragma unroll
    for (int k = 0; k < 15; k++) o_mom[k] = mom[k];
    P.rmse[blk] = sqrt(ss[0] / n3);
    P.rmse_verify[blk] = sqrt(ss[1] / n3);
    P.n_pairs[blk] = (int)n_set;
  }
}
