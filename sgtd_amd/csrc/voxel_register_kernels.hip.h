// voxel_register_kernels.hip.h — sgtd_register_voxels: voxelised GICP of clouds against maps of Gaussian voxels.
//
// The rule is the one include/sgtd_accel.h states at sgtd_register_voxels, on top of sgtd_register_clouds': all f64,
// every operation rounded once (the build's -ffp-contract=off), every sum in the order written there.  The covariances
// are reg_cov_kernel's, the state, the damped solve and the decisions register_kernels.hip.h's (RegState, reg_linearised,
// reg_tried, reg_next_trial, reg_end), the voxel heads scan_kernels.hip.h's.  No floating-point atomics.
//
//   vreg_keys_kernel    a lane per member point of every map, in map and member order: x = R p + t, q, the key; a point
//                       that enters no voxel gets the key n_maps << 48 and sorts behind every voxel
//   (radix_sort_pairs<u64>, stable; scan_heads_kernel / scan_voxels_kernel: the voxels' keys and first points)
//   vreg_ranges_kernel  a lane per map: the first voxel of the map (lower bound of map << 48)
//   vreg_voxel_kernel   a wave per voxel: VSUM of x and Cx over the run, lane l holding accumulator l; mean and cov
//   vreg_init_kernel    per pair: the state from init_pose; "no points"
//   vreg_corr_kernel    a lane per source point: x_i, q, per offset a binary search in the map's keys (they stay in L2);
//                       the voxel ids, and S, its cofactor inverse and Mw, go to per-correspondence streams
//   vreg_lin_kernel     a workgroup per pair: the 29 ordered sums over the points, a point's term summed over its
//                       correspondences first; lane 0 counts the iteration and solves for the first trial
//   vreg_trial_kernel   a workgroup per pair: the cost at the trial pose; lane 0 accepts, rejects or ends the solve
//   vreg_final_kernel   a workgroup per pair: n_corr, n_matched and the fitness from the last pass; the result rows
// LDS: 6.5 KB of reduction scratch in the per-pair kernels, none elsewhere.
#pragma once
#include "register_kernels.hip.h"
#include "scan_kernels.hip.h"

#define SGTD_VREG_W 64               // = SGTD_VREG_SUM_W: accumulators of VSUM, one per lane of the voxel's wave
#define SGTD_VREG_HALF 32768.0       // q lies in [-2^15, 2^15)

struct VregParams {
  const int *map_off;                // [n_maps + 1]
  const int *map_cloud;              // [n_members]
  const int *mem_map;                // [n_members]: the member's map
  const int *mem_pt_off;             // [n_members + 1]: the members' points back to back, in map and member order
  const double *map_pose;            // [n_members][12] or NULL (the identity)
  const int *tgt_map;                // [n_pairs]
  int n_maps, n_members, n_member_pts, mode;
  double res;
  const u64 *vkey;                   // [n_vox] ascending
  const u32 *vstart;                 // [n_vox + 1]: the voxel's first sorted point
  const u32 *order;                  // [n_member_pts]: member-point indices in sorted order
  u32 *map_vox;                      // [n_maps + 1]: the maps' voxel ranges
  u32 n_vox;
  double *vmean, *vcov;              // [n_vox][3], [n_vox][9]
  int *vid;                          // [total_src][mode]: the voxel within the map, -1 without one
  double *Mw;                        // [9][mode][total_src]
  int *out_corr;                     // [n_pairs]
};

__constant__ signed char vreg_off7[7][3] = {{0, 0, 0}, {1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};

__device__ __forceinline__ void vreg_offset(int mode, int o, int *d) {
  if (mode == 27) { d[0] = o / 9 - 1; d[1] = (o / 3) % 3 - 1; d[2] = o % 3 - 1; }
  else if (mode == 7) { d[0] = vreg_off7[o][0]; d[1] = vreg_off7[o][1]; d[2] = vreg_off7[o][2]; }
  else { d[0] = 0; d[1] = 0; d[2] = 0; }
}

// q of x; false: x enters no voxel
__device__ __forceinline__ bool vreg_coord(const double *x, double res, int *q) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double f = floor(x[a] / res - 0.5);
    const bool in = isfinite(x[a]) && f >= -SGTD_VREG_HALF && f < SGTD_VREG_HALF;
    q[a] = in ? (int)f : 0;
    ok = ok && in;
  }
  return ok;
}

__device__ __forceinline__ u64 vreg_key(int map, const int *q) {
  return ((u64)map << 48) | ((u64)(q[0] + 32768) << 32) | ((u64)(q[1] + 32768) << 16) | (u64)(q[2] + 32768);
}

// the member of member point i: the last one whose first point is not behind i (members without points are passed over)
__device__ __forceinline__ int vreg_member_of(const VregParams &V, int i) {
  int lo = 0, hi = V.n_members;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (V.mem_pt_off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void vreg_member_pose(const VregParams &V, int j, double *R, double *t) {
#pragma unroll
  for (int a = 0; a < 9; a++) R[a] = V.map_pose ? V.map_pose[(size_t)j * 12 + a] : (a % 4 == 0 ? 1.0 : 0.0);
#pragma unroll
  for (int a = 0; a < 3; a++) t[a] = V.map_pose ? V.map_pose[(size_t)j * 12 + 9 + a] : 0.0;
}

// G = (R C) R^T in sgtd_register_clouds' form, C the covariance of point g of the clouds
__device__ __forceinline__ void vreg_rotated_cov(const RegParams &P, const double *Rf, long long g, double G[3][3]) {
  double R[3][3], CA[3][3], RC[3][3];
  const double *ca = P.cov + (size_t)g * 9;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) { R[r][c] = Rf[r * 3 + c]; CA[r][c] = ca[r * 3 + c]; }
  mul3(R, CA, RC);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) G[r][c] = (RC[r][0] * R[c][0] + RC[r][1] * R[c][1]) + RC[r][2] * R[c][2];
}

__global__ __launch_bounds__(256) void vreg_keys_kernel(RegParams P, VregParams V, u64 *keys, u32 *vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= V.n_member_pts) return;
  const int j = vreg_member_of(V, i);
  double R[9], t[3], p[3], x[3];
  vreg_member_pose(V, j, R, t);
  reg_point(P, P.pt_off[V.map_cloud[j]] + (i - V.mem_pt_off[j]), p);
  reg_apply(R, t, p, x);
  int q[3];
  const bool ok = vreg_coord(x, V.res, q);
  keys[i] = ok ? vreg_key(V.mem_map[j], q) : (u64)V.n_maps << 48;
  vals[i] = (u32)i;
}

__global__ __launch_bounds__(256) void vreg_ranges_kernel(VregParams V) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m > V.n_maps) return;
  const u64 key = (u64)m << 48;
  u32 lo = 0, hi = V.n_vox;
  while (lo < hi) {
    const u32 mid = (lo + hi) >> 1;
    if (V.vkey[mid] < key) lo = mid + 1; else hi = mid;
  }
  V.map_vox[m] = lo;
}

__global__ __launch_bounds__(256) void vreg_voxel_kernel(RegParams P, VregParams V) {
  const u32 v = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (v >= V.n_vox) return;
  const u32 lane = lane_id();
  const u32 first = V.vstart[v], n = V.vstart[v + 1] - first;
  double a[12];
#pragma unroll
  for (int k = 0; k < 12; k++) a[k] = 0.0;
  for (u32 r = lane; r < n; r += SGTD_VREG_W) {
    const int i = (int)V.order[first + r];
    const int j = vreg_member_of(V, i);
    const long long g = P.pt_off[V.map_cloud[j]] + (i - V.mem_pt_off[j]);
    double R[9], t[3], p[3], x[3], G[3][3];
    vreg_member_pose(V, j, R, t);
    reg_point(P, g, p);
    reg_apply(R, t, p, x);
    vreg_rotated_cov(P, R, g, G);
#pragma unroll
    for (int k = 0; k < 3; k++) a[k] = a[k] + x[k];
#pragma unroll
    for (int k = 0; k < 9; k++) a[3 + k] = a[3 + k] + G[k / 3][k % 3];
  }
  const double div = (double)n;
#pragma unroll
  for (int k = 0; k < 12; k++) {
    double s = a[k];
#pragma unroll
    for (int w = SGTD_VREG_W / 2; w >= 1; w >>= 1) {
      const double u = __shfl_down(s, w, 64);
      if ((int)lane < w) s = s + u;
    }
    if (lane == 0) {
      if (k < 3) V.vmean[(size_t)v * 3 + k] = s / div;
      else V.vcov[(size_t)v * 9 + (k - 3)] = s / div;
    }
  }
}

__global__ __launch_bounds__(SGTD_REG_W) void vreg_init_kernel(RegParams P, VregParams V, const double *init) {
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
  const long long ns = P.pt_off[P.src[k] + 1] - P.pt_off[P.src[k]];
  const int m = V.tgt_map[k];
  const bool empty = ns == 0 || V.map_vox[m + 1] == V.map_vox[m];
  s.status = empty ? REG_NO_POINTS : REG_ITERATION_LIMIT;
  s.done = empty ? 1 : 0;
  P.st[k] = s;
}

// final != 0: the pass behind the solve, for every pair at its pose: the voxel ids alone
__global__ __launch_bounds__(SGTD_REG_THREADS) void vreg_corr_kernel(RegParams P, VregParams V, int final) {
  const int pair = P.tile_pair[blockIdx.x];
  const RegState *st = P.st + pair;
  if (!final && (st->done || st->phase != REG_PHASE_LIN)) return;
  const long long sbase = P.pt_off[P.src[pair]];
  const int ns = (int)(P.pt_off[P.src[pair] + 1] - sbase);
  const int i = P.tile_first[blockIdx.x] + threadIdx.x;
  if (i >= ns) return;
  const size_t g = (size_t)(P.src_off[pair] + i);
  const int m = V.tgt_map[pair];
  const u32 v0 = V.map_vox[m], v1 = V.map_vox[m + 1];
  double R[9], t[3], p[3], x[3], G[3][3];
  for (int a = 0; a < 9; a++) R[a] = st->R[a];
  for (int a = 0; a < 3; a++) t[a] = st->t[a];
  reg_point(P, sbase + i, p);
  reg_apply(R, t, p, x);
  int q[3];
  const bool ok = vreg_coord(x, V.res, q);
  if (ok && !final) vreg_rotated_cov(P, R, sbase + i, G);
  for (int o = 0; o < V.mode; o++) {
    int id = -1;
    if (ok) {
      int d[3], qo[3];
      vreg_offset(V.mode, o, d);
      bool in = true;
      for (int a = 0; a < 3; a++) {
        qo[a] = q[a] + d[a];
        in = in && qo[a] >= -32768 && qo[a] < 32768;
      }
      if (in) {
        const u64 key = vreg_key(m, qo);
        u32 lo = v0, hi = v1;
        while (lo < hi) {
          const u32 mid = (lo + hi) >> 1;
          if (V.vkey[mid] < key) lo = mid + 1; else hi = mid;
        }
        if (lo < v1 && V.vkey[lo] == key) id = (int)(lo - v0);
      }
    }
    V.vid[g * V.mode + o] = id;
    if (final || id < 0) continue;
    const u32 v = v0 + (u32)id;
    const double *cv = V.vcov + (size_t)v * 9;
    double S[3][3];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) S[r][c] = cv[r * 3 + c] + G[r][c];
    double a[9];
    a[0] = S[1][1] * S[2][2] - S[1][2] * S[2][1]; a[1] = S[0][2] * S[2][1] - S[0][1] * S[2][2]; a[2] = S[0][1] * S[1][2] - S[0][2] * S[1][1];
    a[3] = S[1][2] * S[2][0] - S[1][0] * S[2][2]; a[4] = S[0][0] * S[2][2] - S[0][2] * S[2][0]; a[5] = S[0][2] * S[1][0] - S[0][0] * S[1][2];
    a[6] = S[1][0] * S[2][1] - S[1][1] * S[2][0]; a[7] = S[0][1] * S[2][0] - S[0][0] * S[2][1]; a[8] = S[0][0] * S[1][1] - S[0][1] * S[1][0];
    const double det = (S[0][0] * a[0] + S[0][1] * a[3]) + S[0][2] * a[6];
    const double w = sqrt((double)(V.vstart[v + 1] - V.vstart[v]));
    for (int k = 0; k < 9; k++) V.Mw[((size_t)k * V.mode + o) * P.total_src + g] = w * (a[k] / det);
  }
}

// one correspondence's e = mean_v - x and y = Mw e
__device__ __forceinline__ void vreg_residual(const RegParams &P, const VregParams &V, u32 v, int o, size_t g, const double *x, double *M, double *y,
                                              double *cost) {
  double e[3];
  for (int a = 0; a < 3; a++) e[a] = V.vmean[(size_t)v * 3 + a] - x[a];
#pragma unroll
  for (int k = 0; k < 9; k++) M[k] = V.Mw[((size_t)k * V.mode + o) * P.total_src + g];
  for (int a = 0; a < 3; a++) y[a] = relax_mv(M, e, a);
  *cost = (e[0] * y[0] + e[1] * y[1]) + e[2] * y[2];
}

__global__ __launch_bounds__(SGTD_REG_W) void vreg_lin_kernel(RegParams P, VregParams V) {
  __shared__ double red[6 * 128];
  __shared__ double bc[64];
  const int pair = blockIdx.x;
  RegState *st = P.st + pair;
  if (st->done || st->phase != REG_PHASE_LIN) return;
  const long long sbase = P.pt_off[P.src[pair]];
  const int ns = (int)(P.pt_off[P.src[pair] + 1] - sbase), off = P.src_off[pair];
  const u32 v0 = V.map_vox[V.tgt_map[pair]];
  double R[9], t[3];
  for (int a = 0; a < 9; a++) R[a] = st->R[a];
  for (int a = 0; a < 3; a++) t[a] = st->t[a];
  double acc[SGTD_REG_NSUM / 6][6], term[SGTD_REG_NSUM];
#pragma unroll
  for (int c = 0; c < SGTD_REG_NSUM / 6; c++)
#pragma unroll
    for (int a = 0; a < 6; a++) acc[c][a] = 0.0;
#define VREG_TERM(k, v) term[k] = term[k] + (v)
  for (int i = threadIdx.x; i < ns; i += SGTD_REG_W) {
    const size_t g = (size_t)(off + i);
    double p[3], x[3];
    reg_point(P, sbase + i, p);
    reg_apply(R, t, p, x);
    const double A[3][3] = {{0.0, -x[2], x[1]}, {x[2], 0.0, -x[0]}, {-x[1], x[0], 0.0}};
#pragma unroll
    for (int k = 0; k < SGTD_REG_NSUM; k++) term[k] = 0.0;
    for (int o = 0; o < V.mode; o++) {
      const int id = V.vid[g * V.mode + o];
      if (id < 0) continue;
      double M[9], y[3], cost;
      vreg_residual(P, V, v0 + (u32)id, o, g, x, M, y, &cost);
      double MA[3][3];
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) MA[r][c] = (M[r * 3] * A[0][c] + M[r * 3 + 1] * A[1][c]) + M[r * 3 + 2] * A[2][c];
#pragma unroll
      for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int b = 0; b < 3; b++) {
          if (b <= a) {
            VREG_TERM(a * (a + 1) / 2 + b, (A[0][a] * MA[0][b] + A[1][a] * MA[1][b]) + A[2][a] * MA[2][b]);
            VREG_TERM((3 + a) * (4 + a) / 2 + 3 + b, M[a * 3 + b]);
          }
          VREG_TERM((3 + a) * (4 + a) / 2 + b, -MA[a][b]);
        }
        VREG_TERM(21 + a, (A[0][a] * y[0] + A[1][a] * y[1]) + A[2][a] * y[2]);
        VREG_TERM(24 + a, -y[a]);
      }
      VREG_TERM(27, cost);
      VREG_TERM(28, 1.0);
    }
    if (term[28] == 0.0) continue;
#pragma unroll
    for (int k = 0; k < SGTD_REG_NSUM; k++) acc[k / 6][k % 6] = acc[k / 6][k % 6] + term[k];
  }
#undef VREG_TERM
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

__global__ __launch_bounds__(SGTD_REG_W) void vreg_trial_kernel(RegParams P, VregParams V) {
  __shared__ double red[128];
  __shared__ double bc[64];
  const int pair = blockIdx.x;
  RegState *st = P.st + pair;
  if (st->done || st->phase != REG_PHASE_TRIAL) return;
  const long long sbase = P.pt_off[P.src[pair]];
  const int ns = (int)(P.pt_off[P.src[pair] + 1] - sbase), off = P.src_off[pair];
  const u32 v0 = V.map_vox[V.tgt_map[pair]];
  double R[9], t[3];
  for (int a = 0; a < 9; a++) R[a] = st->Rt[a];
  for (int a = 0; a < 3; a++) t[a] = st->tt[a];
  double acc[1] = {0.0};
  for (int i = threadIdx.x; i < ns; i += SGTD_REG_W) {
    const size_t g = (size_t)(off + i);
    double p[3], x[3], sum = 0.0;
    reg_point(P, sbase + i, p);
    reg_apply(R, t, p, x);
    bool any = false;
    for (int o = 0; o < V.mode; o++) {
      const int id = V.vid[g * V.mode + o];
      if (id < 0) continue;
      double M[9], y[3], cost;
      vreg_residual(P, V, v0 + (u32)id, o, g, x, M, y, &cost);
      sum = sum + cost;
      any = true;
    }
    if (any) acc[0] = acc[0] + sum;
  }
  refine_tree<1>(acc, red, bc);
  if (threadIdx.x != 0) return;
  RegState s = *st;
  reg_tried(s, P, acc[0]);
  *st = s;
}

__global__ __launch_bounds__(SGTD_REG_W) void vreg_final_kernel(RegParams P, VregParams V) {
  __shared__ double red[3 * 128];
  __shared__ double bc[64];
  const int pair = blockIdx.x;
  const RegState *st = P.st + pair;
  const long long sbase = P.pt_off[P.src[pair]];
  const int ns = (int)(P.pt_off[P.src[pair] + 1] - sbase), off = P.src_off[pair];
  const u32 v0 = V.map_vox[V.tgt_map[pair]];
  double R[9], t[3];
  for (int a = 0; a < 9; a++) R[a] = st->R[a];
  for (int a = 0; a < 3; a++) t[a] = st->t[a];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < ns; i += SGTD_REG_W) {
    const size_t g = (size_t)(off + i);
    double p[3], x[3], best = __builtin_inf();
    reg_point(P, sbase + i, p);
    reg_apply(R, t, p, x);
    int cnt = 0;
    for (int o = 0; o < V.mode; o++) {
      const int id = V.vid[g * V.mode + o];
      if (id < 0) continue;
      const double *mu = V.vmean + (size_t)(v0 + (u32)id) * 3;
      const double dx = mu[0] - x[0], dy = mu[1] - x[1], dz = mu[2] - x[2];
      const double dd = (dx * dx + dy * dy) + dz * dz;
      best = dd < best ? dd : best;
      cnt++;
    }
    if (cnt == 0) continue;
    acc[0] = acc[0] + best;
    acc[1] = acc[1] + 1.0;
    acc[2] = acc[2] + (double)cnt;
  }
  refine_tree<3>(acc, red, bc);
  if (threadIdx.x != 0) return;
  for (int a = 0; a < 9; a++) P.out_pose[(size_t)pair * 12 + a] = st->R[a];
  for (int a = 0; a < 3; a++) P.out_pose[(size_t)pair * 12 + 9 + a] = st->t[a];
  P.out_fitness[pair] = acc[0] / acc[1];      // (0.0 / 0.0 without a matched point)
  P.out_cost[(size_t)pair * 2] = st->cost_first;
  P.out_cost[(size_t)pair * 2 + 1] = st->cost_last;
  P.out_matched[pair] = (int)acc[1];
  V.out_corr[pair] = (int)acc[2];
  P.out_iters[pair] = st->iters;
  P.out_status[pair] = st->status;
}
