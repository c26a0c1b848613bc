// register_kernels.hip.h — sgtd_register_clouds: plane-regularised GICP of raw clouds, Levenberg-Marquardt per pair.
//
// The rule is the one include/sgtd_accel.h states at sgtd_register_clouds: all f64, every operation rounded once (the
// build's -ffp-contract=off), every sum in the order written there.  UNIT, ROT and M v are relax_kernels.hip.h's, svd3_dev
// and mul3 verify_kernels.hip.h's, the ordered sum's tree refine_kernels.hip.h's.  No floating-point atomics; the one
// atomic is the integer count of unfinished pairs.
//
//   reg_cov_kernel     a lane per point of a cloud some pair names: the cloud streams through LDS in tiles (broadcast
//                      reads), the lane keeps its k' best (d2, index) sorted in registers, holds back what beats its worst
//                      in a row of SGTD_REG_HOLD in LDS and inserts a row at a time; then mu, c, svd3 and C in the lane
//   reg_init_kernel    per pair: the state from init_pose; "no points"
//   reg_search_kernel  a workgroup per (tile of source points, slice of the target): x = R p + t, the slice streamed
//                      through LDS, the lane's minimum over (d2, j) of the slice (ascending j, strict <: ties to the
//                      lowest index)
//   reg_match_kernel   a lane per source point: the slices' minima combined in ascending slice order (exact under any
//                      split), the max_corr_dist test, M_i
//   reg_lin_kernel     a workgroup per pair: the 29 ordered sums of the linearisation; lane 0 counts the iteration and
//                      solves for the first trial
//   reg_trial_kernel   a workgroup per pair: the cost at the trial pose; lane 0 accepts, rejects (and solves for the next
//                      trial: no search is repeated) or ends the solve
//   reg_final_kernel   a workgroup per pair: n_matched and the fitness from the last pass's matches; the result rows
// The per-pair kernels read RegState and return at once when it leaves them nothing to do: a finished pair, or one whose
// phase is the other kernels'.  LDS: 8 KB of target tile (search, covariances), 12 KB of held candidates (covariances),
// 6.5 KB of reduction scratch (sums).
#pragma once
#include "refine_kernels.hip.h"
#include "relax_kernels.hip.h"

#define SGTD_REG_THREADS 128         // = SGTD_REG_SRC_TILE of the header: a lane per source point
#define SGTD_REG_W 256               // = SGTD_REG_SUM_W: accumulators of SUM, threads of the per-pair kernels
#define SGTD_REG_TILE 512            // = SGTD_REG_TGT_TILE: targets staged in LDS at once
#define SGTD_REG_K 32                // = SGTD_REG_MAX_K
#define SGTD_REG_HOLD 8              // candidates a lane holds back before its wave inserts (reg_cov_kernel)
#define SGTD_REG_NSUM 30            // 21 of H's lower triangle, 6 of b, the cost, the count, one spare

enum { REG_PHASE_LIN = 0, REG_PHASE_TRIAL = 1 };
enum { REG_CONVERGED = 0, REG_ITERATION_LIMIT = 1, REG_LM_FAILED = 2, REG_NO_CORRESPONDENCE = 3, REG_NO_POINTS = 4 };

struct RegState {
  double R[9], t[3];                 // the pose
  double Rt[9], tt[3];               // the trial pose
  double H[21], b[6], d[6];          // H: lower triangle, row a at a (a + 1) / 2
  double y0, lambda, nu, cost_first, cost_last;
  int iters, trials, phase, status, done, conv;
};

struct RegOptionsDev {
  int k, max_iterations, lm_max_trials;
  double max2, lambda_factor, rotation_eps, translation_eps, plane_eps;
};

struct RegParams {
  const float *pts;
  int stride;
  const long long *pt_off;           // [n_clouds + 1]
  const int *src, *tgt;              // [n_pairs]
  const int *src_off;                // [n_pairs + 1]: the pairs' source points back to back
  const int *tile_pair, *tile_first; // [n_tiles] source tiles: the pair, the first point within its source
  const int *ctile_cloud, *ctile_first;   // [n_ctiles] tiles of the named clouds
  int n_pairs, n_tiles, n_ctiles;
  int total_src;                     // source points of all pairs: the stride of the per-point streams
  int slice;                         // targets per slice
  double *cov;                       // [points of all clouds][9]
  double *part_d2;                   // [slices][total_src]
  int *part_j;
  double *md2;                       // [total_src]: the last pass's matches
  int *mj;
  double *M;                         // 9 streams of total_src
  RegState *st;
  int *unfinished;
  double *out_pose, *out_fitness, *out_cost;      // [n_pairs][12], [n_pairs], [n_pairs][2]
  int *out_matched, *out_iters, *out_status;      // [n_pairs]
  RegOptionsDev o;
};

__device__ __forceinline__ void reg_point(const RegParams &P, long long g, double *p) {
  const float *f = P.pts + (size_t)g * P.stride;
  p[0] = (double)f[0]; p[1] = (double)f[1]; p[2] = (double)f[2];
}

// the cloud's points [first, first + count) into the tile, x y z widened at the read
__device__ __forceinline__ void reg_stage(const RegParams &P, long long base, int first, int count, float4 *tile, int threads) {
  for (int k = threadIdx.x; k < count; k += threads) {
    const float *f = P.pts + (size_t)(base + first + k) * P.stride;
    tile[k] = make_float4(f[0], f[1], f[2], 0.f);
  }
}

__device__ __forceinline__ void reg_apply(const double *R, const double *t, const double *p, double *x) {
#pragma unroll
  for (int r = 0; r < 3; r++) x[r] = relax_mv(R, p, r) + t[r];
}

__global__ __launch_bounds__(SGTD_REG_THREADS) void reg_cov_kernel(RegParams P) {
  __shared__ float4 tile[SGTD_REG_TILE];
  __shared__ double hold_d[SGTD_REG_HOLD][SGTD_REG_THREADS];      // a row of candidates per lane, lane-contiguous
  __shared__ int hold_j[SGTD_REG_HOLD][SGTD_REG_THREADS];
  const int cloud = P.ctile_cloud[blockIdx.x];
  const long long base = P.pt_off[cloud];
  const int n = (int)(P.pt_off[cloud + 1] - base);
  const int i = P.ctile_first[blockIdx.x] + threadIdx.x;
  const bool active = i < n;
  const int kk = P.o.k < n ? P.o.k : n;
  const double inf = __builtin_inf();
  double p[3] = {0.0, 0.0, 0.0};
  if (active) reg_point(P, base + i, p);
  double bd[SGTD_REG_K];
  int bj[SGTD_REG_K];
#pragma unroll
  for (int s = 0; s < SGTD_REG_K; s++) { bd[s] = inf; bj[s] = 0x7FFFFFFF; }
  double worst = inf;
  int held = 0;
  // the lane's held candidates go into its sorted list, by the full (d2, index) order: one that is beaten by then falls
  // through and is dropped.  A wave runs this for all its lanes at once, so it is kept rare: only when a lane's row is full
  auto insert_held = [&]() {
    for (int b = 0; b < SGTD_REG_HOLD; b++) {
      double cd = inf;
      int cj = 0x7FFFFFFF;
      if (b < held) { cd = hold_d[b][threadIdx.x]; cj = hold_j[b][threadIdx.x]; }
#pragma unroll
      for (int s = 0; s < SGTD_REG_K; s++) {
        if (s < kk && (cd < bd[s] || (cd == bd[s] && cj < bj[s]))) {
          const double td = bd[s]; bd[s] = cd; cd = td;
          const int tj = bj[s]; bj[s] = cj; cj = tj;
        }
      }
    }
#pragma unroll
    for (int s = 0; s < SGTD_REG_K; s++)
      if (s == kk - 1) worst = bd[s];
    held = 0;
  };
  for (int first = 0; first < n; first += SGTD_REG_TILE) {
    const int count = n - first < SGTD_REG_TILE ? n - first : SGTD_REG_TILE;
    __syncthreads();
    reg_stage(P, base, first, count, tile, SGTD_REG_THREADS);
    __syncthreads();
    if (!active) continue;
    for (int k = 0; k < count; k++) {
      const float4 w = tile[k];
      const double dx = (double)w.x - p[0], dy = (double)w.y - p[1], dz = (double)w.z - p[2];
      const double dd = (dx * dx + dy * dy) + dz * dz;
      // (ascending index: an equal d2 does not beat the worst; NaN and +inf never do.  `worst` is the list's as of the last
      // insertion, so more may be held than the list will take)
      if (dd < worst) {
        hold_d[held][threadIdx.x] = dd;
        hold_j[held][threadIdx.x] = first + k;
        held++;
      }
      if (__any(held == SGTD_REG_HOLD)) insert_held();
    }
  }
  if (!active) return;
  insert_held();
  const double div = (double)kk;
  double mu[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < SGTD_REG_K; s++) {
    if (s < kk && bj[s] != 0x7FFFFFFF) {
      double q[3];
      reg_point(P, base + bj[s], q);
      for (int a = 0; a < 3; a++) mu[a] = mu[a] + q[a];
    }
  }
  for (int a = 0; a < 3; a++) mu[a] = mu[a] / div;
  double c[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
  for (int s = 0; s < SGTD_REG_K; s++) {
    if (s < kk && bj[s] != 0x7FFFFFFF) {
      double q[3];
      reg_point(P, base + bj[s], q);
      for (int a = 0; a < 3; a++) q[a] = q[a] - mu[a];
      for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) c[a][b] = c[a][b] + q[a] * q[b];
    }
  }
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) c[a][b] = c[a][b] / div;
  double U[3][3], V[3][3], VT[3][3], UD[3][3], C[3][3];
  svd3_dev(c, U, V);
  for (int b = 0; b < 3; b++) {      // (a completed column of U has no sign of its own: it takes V's)
    const double dot = (U[0][b] * V[0][b] + U[1][b] * V[1][b]) + U[2][b] * V[2][b];
    if (dot < 0.0)
      for (int a = 0; a < 3; a++) U[a][b] = -U[a][b];
  }
  const double D[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, P.o.plane_eps}};
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) VT[a][b] = V[b][a];
  mul3(U, D, UD);
  mul3(UD, VT, C);
  double *out = P.cov + (size_t)(base + i) * 9;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) out[a * 3 + b] = C[a][b];
}

__global__ __launch_bounds__(SGTD_REG_W) void reg_init_kernel(RegParams P, const double *init) {
  const int k = blockIdx.x * SGTD_REG_W + threadIdx.x;
  if (k >= P.n_pairs) return;
  RegState s;
  for (int a = 0; a < 9; a++) s.R[a] = init ? init[(size_t)k * 12 + a] : (a % 4 == 0 ? 1.0 : 0.0);
  for (int a = 0; a < 3; a++) s.t[a] = init ? init[(size_t)k * 12 + 9 + a] : 0.0;
  for (int a = 0; a < 9; a++) s.Rt[a] = s.R[a];
  for (int a = 0; a < 3; a++) s.tt[a] = s.t[a];
  for (int a = 0; a < 21; a++) s.H[a] = 0.0;
  for (int a = 0; a < 6; a++) { s.b[a] = 0.0; s.d[a] = 0.0; }
  s.y0 = 0.0; s.lambda = 0.0; s.nu = 2.0;
  s.cost_first = __builtin_nan(""); s.cost_last = s.cost_first;
  s.iters = 0; s.trials = 0; s.phase = REG_PHASE_LIN; s.conv = 0;
  const long long ns = P.pt_off[P.src[k] + 1] - P.pt_off[P.src[k]], nt = P.pt_off[P.tgt[k] + 1] - P.pt_off[P.tgt[k]];
  const bool empty = ns == 0 || nt == 0;
  s.status = empty ? REG_NO_POINTS : REG_ITERATION_LIMIT;
  s.done = empty ? 1 : 0;
  P.st[k] = s;
}

// final != 0: the pass behind the solve, for every pair at its pose
__global__ __launch_bounds__(SGTD_REG_THREADS) void reg_search_kernel(RegParams P, int final) {
  __shared__ float4 tile[SGTD_REG_TILE];
  const int pair = P.tile_pair[blockIdx.x];
  const RegState *st = P.st + pair;
  if (!final && (st->done || st->phase != REG_PHASE_LIN)) return;
  const long long sbase = P.pt_off[P.src[pair]], tbase = P.pt_off[P.tgt[pair]];
  const int ns = (int)(P.pt_off[P.src[pair] + 1] - sbase), nt = (int)(P.pt_off[P.tgt[pair] + 1] - tbase);
  const long long s0l = (long long)blockIdx.y * P.slice;
  if (s0l >= nt) return;
  const int s0 = (int)s0l, s1 = nt - s0 < P.slice ? nt : s0 + P.slice;
  const int i = P.tile_first[blockIdx.x] + threadIdx.x;
  const bool active = i < ns;
  double x[3] = {0.0, 0.0, 0.0};
  if (active) {
    double p[3];
    reg_point(P, sbase + i, p);
    reg_apply(st->R, st->t, p, x);
  }
  double best = __builtin_inf();
  int bj = -1;
  for (int first = s0; first < s1; first += SGTD_REG_TILE) {
    const int count = s1 - first < SGTD_REG_TILE ? s1 - first : SGTD_REG_TILE;
    __syncthreads();
    reg_stage(P, tbase, first, count, tile, SGTD_REG_THREADS);
    __syncthreads();
    if (!active) continue;
    for (int k = 0; k < count; k++) {
      const float4 w = tile[k];
      const double dx = (double)w.x - x[0], dy = (double)w.y - x[1], dz = (double)w.z - x[2];
      const double dd = (dx * dx + dy * dy) + dz * dz;
      if (dd < best) { best = dd; bj = first + k; }
    }
  }
  if (!active) return;
  const size_t g = (size_t)blockIdx.y * P.total_src + (size_t)(P.src_off[pair] + i);
  P.part_d2[g] = best;
  P.part_j[g] = bj;
}

__global__ __launch_bounds__(SGTD_REG_THREADS) void reg_match_kernel(RegParams P, int final) {
  const int pair = P.tile_pair[blockIdx.x];
  const RegState *st = P.st + pair;
  if (!final && (st->done || st->phase != REG_PHASE_LIN)) return;
  const long long sbase = P.pt_off[P.src[pair]], tbase = P.pt_off[P.tgt[pair]];
  const int ns = (int)(P.pt_off[P.src[pair] + 1] - sbase), nt = (int)(P.pt_off[P.tgt[pair] + 1] - tbase);
  const int i = P.tile_first[blockIdx.x] + threadIdx.x;
  if (i >= ns) return;
  const size_t g = (size_t)(P.src_off[pair] + i);
  const int slices = (int)(((long long)nt + P.slice - 1) / P.slice);
  double best = __builtin_inf();
  int bj = -1;
  for (int s = 0; s < slices; s++) {
    const double dd = P.part_d2[(size_t)s * P.total_src + g];
    if (dd < best) { best = dd; bj = P.part_j[(size_t)s * P.total_src + g]; }
  }
  const bool keep = best < P.o.max2;
  P.md2[g] = best;
  P.mj[g] = keep ? bj : -1;
  if (final || !keep) return;
  double R[3][3], CA[3][3], RC[3][3], S[3][3];
  const double *ca = P.cov + (size_t)(sbase + i) * 9, *cb = P.cov + (size_t)(tbase + bj) * 9;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) { R[r][c] = st->R[r * 3 + c]; CA[r][c] = ca[r * 3 + c]; }
  mul3(R, CA, RC);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) S[r][c] = cb[r * 3 + c] + ((RC[r][0] * R[c][0] + RC[r][1] * R[c][1]) + RC[r][2] * R[c][2]);
  double a[9];
  a[0] = S[1][1] * S[2][2] - S[1][2] * S[2][1]; a[1] = S[0][2] * S[2][1] - S[0][1] * S[2][2]; a[2] = S[0][1] * S[1][2] - S[0][2] * S[1][1];
  a[3] = S[1][2] * S[2][0] - S[1][0] * S[2][2]; a[4] = S[0][0] * S[2][2] - S[0][2] * S[2][0]; a[5] = S[0][2] * S[1][0] - S[0][0] * S[1][2];
  a[6] = S[1][0] * S[2][1] - S[1][1] * S[2][0]; a[7] = S[0][1] * S[2][0] - S[0][0] * S[2][1]; a[8] = S[0][0] * S[1][1] - S[0][1] * S[1][0];
  const double det = (S[0][0] * a[0] + S[0][1] * a[3]) + S[0][2] * a[6];
  for (int k = 0; k < 9; k++) P.M[(size_t)k * P.total_src + g] = a[k] / det;
}

// the pair ends
__device__ __forceinline__ void reg_end(RegState &s, const RegParams &P, int status) {
  s.status = status;
  s.done = 1;
  atomicSub(P.unfinished, 1);
}

// the next trial of the iteration: the damped solve and the trial pose; rejected at once while a pivot is not positive
__device__ inline void reg_next_trial(RegState &s, const RegParams &P) {
  for (;;) {
    if (s.trials >= P.o.lm_max_trials) { reg_end(s, P, REG_LM_FAILED); return; }
    s.trials++;
    double L[36];
    for (int a = 0; a < 36; a++) L[a] = 0.0;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; c++) {
      double v = s.H[c * (c + 1) / 2 + c] + s.lambda;
#pragma unroll
      for (int k = 0; k < c; k++) v = v - L[c * 6 + k] * L[c * 6 + k];
      ok = ok && v > 0.0;
      L[c * 6 + c] = sqrt(v);
#pragma unroll
      for (int rr = c + 1; rr < 6; rr++) {
        double v2 = s.H[rr * (rr + 1) / 2 + c];
#pragma unroll
        for (int k = 0; k < c; k++) v2 = v2 - L[rr * 6 + k] * L[c * 6 + k];
        L[rr * 6 + c] = v2 / L[c * 6 + c];
      }
    }
    if (!ok) { s.lambda = s.nu * s.lambda; s.nu = 2.0 * s.nu; continue; }
    double r[6], d[6];
    for (int a = 0; a < 6; a++) r[a] = -s.b[a];
    relax_solve(L, r, d);
    double q[4] = {1.0, 0.5 * d[0], 0.5 * d[1], 0.5 * d[2]}, dR[9];
    relax_unit(q);
    relax_rot(q, dR);
    for (int rr = 0; rr < 3; rr++) {
      for (int c = 0; c < 3; c++) s.Rt[rr * 3 + c] = (dR[rr * 3] * s.R[c] + dR[rr * 3 + 1] * s.R[3 + c]) + dR[rr * 3 + 2] * s.R[6 + c];
      s.tt[rr] = relax_mv(dR, s.t, rr) + d[3 + rr];
    }
    double mr = 0.0, mt = 0.0;
    for (int a = 0; a < 9; a++) {
      const double v = fabs(dR[a] - (a % 4 == 0 ? 1.0 : 0.0));
      mr = v > mr ? v : mr;
    }
    for (int a = 0; a < 3; a++) {
      const double v = fabs(d[3 + a]);
      mt = v > mt ? v : mt;
    }
    const double u = mr / P.o.rotation_eps, v = mt / P.o.translation_eps;
    s.conv = (v > u ? v : u) < 1.0 ? 1 : 0;
    for (int a = 0; a < 6; a++) s.d[a] = d[a];
    s.phase = REG_PHASE_TRIAL;
    return;
  }
}

// lane 0 behind a linearisation whose H, b and y0 are in s: the iteration is counted; "no correspondence", or the first
// trial's solve (lambda from H on the pair's first linearisation)
__device__ inline void reg_linearised(RegState &s, const RegParams &P, bool none) {
  s.iters = s.iters + 1;
  if (s.iters == 1) s.cost_first = s.y0;
  s.cost_last = s.y0;
  if (none) {
    reg_end(s, P, REG_NO_CORRESPONDENCE);
    return;
  }
  if (s.iters == 1) {
    double m = 0.0;
    for (int a = 0; a < 6; a++) {
      const double v = fabs(s.H[a * (a + 1) / 2 + a]);
      m = v > m ? v : m;
    }
    s.lambda = P.o.lambda_factor * m;
  }
  s.nu = 2.0;
  s.trials = 0;
  reg_next_trial(s, P);
}

// lane 0 behind a trial whose cost is yi: the trial is accepted, rejected (and the next one solved for) or ends the solve
__device__ inline void reg_tried(RegState &s, const RegParams &P, double yi) {
  double den = s.d[0] * (s.lambda * s.d[0] - s.b[0]);
  for (int a = 1; a < 6; a++) den = den + s.d[a] * (s.lambda * s.d[a] - s.b[a]);
  const double rho = (s.y0 - yi) / den;
  bool ended = false;
  if (!(rho >= 0.0)) {
    if (s.conv) ended = true;
    else {
      s.lambda = s.nu * s.lambda;
      s.nu = 2.0 * s.nu;
      reg_next_trial(s, P);
    }
  } else {
    for (int a = 0; a < 9; a++) s.R[a] = s.Rt[a];
    for (int a = 0; a < 3; a++) s.t[a] = s.tt[a];
    const double f = 2.0 * rho - 1.0, g = 1.0 - (f * f) * f, third = 1.0 / 3.0;
    s.lambda = s.lambda * (g > third ? g : third);
    ended = true;
  }
  if (ended) {
    if (s.conv) reg_end(s, P, REG_CONVERGED);
    else if (s.iters >= P.o.max_iterations) reg_end(s, P, REG_ITERATION_LIMIT);
    else s.phase = REG_PHASE_LIN;
  }
}

// one matched point's e = w_j - x_i under (R, t) and y = M_i e
__device__ __forceinline__ void reg_residual(const RegParams &P, const double *R, const double *t, long long sbase, long long tbase, int i, int j,
                                             size_t g, double *x, double *M, double *y, double *cost) {
  double p[3], w[3], e[3];
  reg_point(P, sbase + i, p);
  reg_point(P, tbase + j, w);
  reg_apply(R, t, p, x);
  for (int a = 0; a < 3; a++) e[a] = w[a] - x[a];
#pragma unroll
  for (int k = 0; k < 9; k++) M[k] = P.M[(size_t)k * P.total_src + g];
  for (int a = 0; a < 3; a++) y[a] = relax_mv(M, e, a);
  *cost = (e[0] * y[0] + e[1] * y[1]) + e[2] * y[2];
}

__global__ __launch_bounds__(SGTD_REG_W) void reg_lin_kernel(RegParams P) {
  __shared__ double red[6 * 128];
  __shared__ double bc[64];
  const int pair = blockIdx.x;
  RegState *st = P.st + pair;
  if (st->done || st->phase != REG_PHASE_LIN) return;
  const long long sbase = P.pt_off[P.src[pair]], tbase = P.pt_off[P.tgt[pair]];
  const int ns = (int)(P.pt_off[P.src[pair] + 1] - sbase), off = P.src_off[pair];
  double R[9], t[3];
  for (int a = 0; a < 9; a++) R[a] = st->R[a];
  for (int a = 0; a < 3; a++) t[a] = st->t[a];
  double acc[SGTD_REG_NSUM / 6][6];
#pragma unroll
  for (int c = 0; c < SGTD_REG_NSUM / 6; c++)
#pragma unroll
    for (int a = 0; a < 6; a++) acc[c][a] = 0.0;
#define REG_ACC(k, v) acc[(k) / 6][(k) % 6] = acc[(k) / 6][(k) % 6] + (v)
  for (int i = threadIdx.x; i < ns; i += SGTD_REG_W) {
    const size_t g = (size_t)(off + i);
    const int j = P.mj[g];
    if (j < 0) continue;
    double x[3], M[9], y[3], cost;
    reg_residual(P, R, t, sbase, tbase, i, j, g, x, M, y, &cost);
    const double A[3][3] = {{0.0, -x[2], x[1]}, {x[2], 0.0, -x[0]}, {-x[1], x[0], 0.0}};
    double MA[3][3];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) MA[r][c] = (M[r * 3] * A[0][c] + M[r * 3 + 1] * A[1][c]) + M[r * 3 + 2] * A[2][c];
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
      for (int b = 0; b < 3; b++) {
        if (b <= a) {
          REG_ACC(a * (a + 1) / 2 + b, (A[0][a] * MA[0][b] + A[1][a] * MA[1][b]) + A[2][a] * MA[2][b]);
          REG_ACC((3 + a) * (4 + a) / 2 + 3 + b, M[a * 3 + b]);
        }
        REG_ACC((3 + a) * (4 + a) / 2 + b, -MA[a][b]);
      }
      REG_ACC(21 + a, (A[0][a] * y[0] + A[1][a] * y[1]) + A[2][a] * y[2]);
      REG_ACC(24 + a, -y[a]);
    }
    REG_ACC(27, cost);
    REG_ACC(28, 1.0);
  }
#undef REG_ACC
#pragma unroll
  for (int c = 0; c < SGTD_REG_NSUM / 6; c++) refine_tree<6>(acc[c], red, bc);
  if (threadIdx.x != 0) return;
  RegState s = *st;
#pragma unroll
  for (int k = 0; k < 21; k++) s.H[k] = acc[k / 6][k % 6];
#pragma unroll
  for (int a = 0; a < 6; a++) s.b[a] = acc[(21 + a) / 6][(21 + a) % 6];
  s.y0 = acc[27 / 6][27 % 6];
  reg_linearised(s, P, acc[28 / 6][28 % 6] == 0.0);
  *st = s;
}

__global__ __launch_bounds__(SGTD_REG_W) void reg_trial_kernel(RegParams P) {
  __shared__ double red[128];
  __shared__ double bc[64];
  const int pair = blockIdx.x;
  RegState *st = P.st + pair;
  if (st->done || st->phase != REG_PHASE_TRIAL) return;
  const long long sbase = P.pt_off[P.src[pair]], tbase = P.pt_off[P.tgt[pair]];
  const int ns = (int)(P.pt_off[P.src[pair] + 1] - sbase), off = P.src_off[pair];
  double R[9], t[3];
  for (int a = 0; a < 9; a++) R[a] = st->Rt[a];
  for (int a = 0; a < 3; a++) t[a] = st->tt[a];
  double acc[1] = {0.0};
  for (int i = threadIdx.x; i < ns; i += SGTD_REG_W) {
    const size_t g = (size_t)(off + i);
    const int j = P.mj[g];
    if (j < 0) continue;
    double x[3], M[9], y[3], cost;
    reg_residual(P, R, t, sbase, tbase, i, j, g, x, M, y, &cost);
    acc[0] = acc[0] + cost;
  }
  refine_tree<1>(acc, red, bc);
  if (threadIdx.x != 0) return;
  RegState s = *st;
  reg_tried(s, P, acc[0]);
  *st = s;
}

__global__ __launch_bounds__(SGTD_REG_W) void reg_final_kernel(RegParams P) {
  __shared__ double red[2 * 128];
  __shared__ double bc[64];
  const int pair = blockIdx.x;
  const RegState *st = P.st + pair;
  const int ns = (int)(P.pt_off[P.src[pair] + 1] - P.pt_off[P.src[pair]]), off = P.src_off[pair];
  double acc[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < ns; i += SGTD_REG_W) {
    if (P.mj[off + i] < 0) continue;
    acc[0] = acc[0] + P.md2[off + i];
    acc[1] = acc[1] + 1.0;
  }
  refine_tree<2>(acc, red, bc);
  if (threadIdx.x != 0) return;
  for (int a = 0; a < 9; a++) P.out_pose[(size_t)pair * 12 + a] = st->R[a];
  for (int a = 0; a < 3; a++) P.out_pose[(size_t)pair * 12 + 9 + a] = st->t[a];
  P.out_fitness[pair] = acc[0] / acc[1];      // (0.0 / 0.0 without a match)
  P.out_cost[(size_t)pair * 2] = st->cost_first;
  P.out_cost[(size_t)pair * 2 + 1] = st->cost_last;
  P.out_matched[pair] = (int)acc[1];
  P.out_iters[pair] = st->iters;
  P.out_status[pair] = st->status;
}
