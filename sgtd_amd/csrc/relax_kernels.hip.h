// relax_kernels.hip.h — sgtd_relax_poses: Levenberg-Marquardt over a pose graph, the step by block-preconditioned CG.
//
// The rule is the one include/sgtd_accel.h states at sgtd_relax_poses: all f64, every operation rounded once (the
// build's -ffp-contract=off), every sum in the order written there; QUAT, ROT, SUM and MAX below are that comment's,
// inv() and mul() are consistency_kernels.hip.h's.  No floating-point atomics, no barrier between workgroups: every
// reduction is one workgroup of SGTD_RELAX_W threads (relax_ctl_kernel), which also takes every decision and keeps it in
// RelaxState; the other kernels read that state and return at once when it leaves them nothing to do.
//
//   relax_init_kernel     per node: pose0 -> (q, t, R = ROT(q)); per edge: inv(Z)
//   relax_edge_kernel     per edge: the residual and the cost terms at the current or the trial state; at the current
//                         state also the Jacobian blocks B, E_R, D_R and y = W r (structure of arrays, stride ms)
//   relax_setup_kernel    per node: g = J^T y and H_nn over the incident edges in ascending index (node -> edge CSR),
//                         the Cholesky factor of the damped block, r = -g, x = p = 0, z = M^-1 r
//   relax_cg_edge_kernel  per edge: y = W J p with p = z + beta p formed on the fly for both ends
//   relax_cg_node_kernel  per node: p = z + beta p (stored), Ap = J^T y + lambda H_nn p
//   relax_cg_update_kernel per node: x += alpha p, r -= alpha Ap, z = M^-1 r
//   relax_retract_kernel  per node: the trial state from x
//   relax_ctl_kernel      one workgroup: SUM / MAX and the decision of its mode
// Node vectors are [n][6] (dt, dtheta): element e = 6 node + a, which is SUM's order.  A node's state record is 16 f64:
// q (w, x, y, z), t, R row-major; two sets of records, RelaxState::cur names the current one, the other is the trial.
// The per-node and per-edge kernels are grid-stride loops: the host caps their grids (four workgroups a CU, or the
// SGTD_RELAX_MAX_BLOCKS hook), and no result depends on the grid.
#pragma once
#include "consistency_kernels.hip.h"

#define SGTD_RELAX_THREADS 256
#define SGTD_RELAX_W 1024            // = SGTD_RELAX_SUM_W of the header: accumulators of SUM, threads of relax_ctl_kernel
#define SGTD_RELAX_REC 16

enum { RELAX_CTL_COST0 = 0, RELAX_CTL_RZ0, RELAX_CTL_PQ, RELAX_CTL_RZ, RELAX_CTL_ACCEPT };

struct RelaxState {
  double cost, cost_before, lambda, rz, rz0, thr, alpha, beta;
  int outer, accepted, cg_total, cg_done, done, status, cur, pad;
};

struct RelaxParams {
  int n, m;
  size_t ms;                       // stream stride of the per-edge arrays
  double *state;                   // [2][n][SGTD_RELAX_REC]
  const unsigned char *held;       // [n]
  unsigned char *ok;               // [n] free and every pivot of its block positive
  const int *ei, *ej;              // [m]
  const double *wt, *wr;           // [m]
  double *iz;                      // 12 streams: inv(Z) rot (= A), t
  double *jac;                     // 27 streams: B, E_R, D_R
  double *y;                       // 6 streams
  double *csum;                    // [m] the edge's cost
  double *ec;                      // [2][m][2]: trans, rot per state set
  const int *off, *ent;            // node -> incident edges: ent = edge << 1 | side (0: the node is i, 1: j), ascending
  double *r, *x, *p, *z, *ap;      // [n][6]
  double *H, *L;                   // [n][36]
  RelaxState *st;
  double lmin, lmax, tol2, step_tol;
  int max_outer, all_held;
};

__device__ __forceinline__ void relax_unit(double *q) {
  const double nn = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
  const double s = sqrt(nn);
  for (int k = 0; k < 4; k++) q[k] = q[k] / s;
}

// QUAT: R row-major (9) -> q
__device__ __forceinline__ void relax_quat(const double *R, double *q) {
  const double tr = (R[0] + R[4]) + R[8];
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0) * 2.0;
    q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = sqrt(((1.0 + R[0]) - R[4]) - R[8]) * 2.0;
    q[0] = (R[7] - R[5]) / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    const double s = sqrt(((1.0 + R[4]) - R[0]) - R[8]) * 2.0;
    q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s;
  } else {
    const double s = sqrt(((1.0 + R[8]) - R[0]) - R[4]) * 2.0;
    q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s;
  }
  relax_unit(q);
}

// ROT
__device__ __forceinline__ void relax_rot(const double *q, double *R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// (M v)[r] and (M^T v)[r], M row-major 3x3: (m0 v0 + m1 v1) + m2 v2
__device__ __forceinline__ double relax_mv(const double *M, const double *v, int r) { return (M[r * 3] * v[0] + M[r * 3 + 1] * v[1]) + M[r * 3 + 2] * v[2]; }
__device__ __forceinline__ double relax_mtv(const double *M, const double *v, int r) { return (M[r] * v[0] + M[3 + r] * v[1]) + M[6 + r] * v[2]; }

__device__ __forceinline__ void relax_load(const double *soa, size_t ms, int first, int count, int k, double *out) {
#pragma unroll
  for (int s = 0; s < count; s++) out[s] = soa[(size_t)(first + s) * ms + k];
}

#define RELAX_GRID_LOOP(i, count) \
  for (int i = blockIdx.x * SGTD_RELAX_THREADS + threadIdx.x; i < (count); i += gridDim.x * SGTD_RELAX_THREADS)

__global__ __launch_bounds__(SGTD_RELAX_THREADS) void relax_init_kernel(RelaxParams P, const double *pose0, const double *meas) {
  RELAX_GRID_LOOP(v, P.n) {
    double R[9], rec[SGTD_RELAX_REC];
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) R[r * 3 + c] = pose0[(size_t)v * 12 + r * 4 + c];
      rec[4 + r] = pose0[(size_t)v * 12 + r * 4 + 3];
    }
    relax_quat(R, rec);
    relax_rot(rec, rec + 7);
    for (int k = 0; k < SGTD_RELAX_REC; k++) P.state[(size_t)v * SGTD_RELAX_REC + k] = rec[k];
  }
  RELAX_GRID_LOOP(k, P.m) {
    double Z[12], IZ[12];
    for (int s = 0; s < 12; s++) Z[s] = meas[(size_t)k * 12 + s];
    cons_inv(Z, IZ);
    for (int s = 0; s < 12; s++) P.iz[(size_t)s * P.ms + k] = IZ[s];
  }
}

// trial == 0: the current state, with the Jacobian blocks and y = W r; trial == 1: the trial state, costs only
__global__ __launch_bounds__(SGTD_RELAX_THREADS) void relax_edge_kernel(RelaxParams P, int trial) {
  if (P.st->done) return;
  const int set = P.st->cur ^ trial;
  const double *state = P.state + (size_t)set * P.n * SGTD_RELAX_REC;
  double *ec = P.ec + (size_t)set * P.m * 2;
  RELAX_GRID_LOOP(k, P.m) {
    const double *ri = state + (size_t)P.ei[k] * SGTD_RELAX_REC, *rj = state + (size_t)P.ej[k] * SGTD_RELAX_REC;
    double Xi[12], Xj[12], IXi[12], D[12], IZ[12], E[12];
    for (int s = 0; s < 9; s++) { Xi[s] = ri[7 + s]; Xj[s] = rj[7 + s]; }
    for (int s = 0; s < 3; s++) { Xi[9 + s] = ri[4 + s]; Xj[9 + s] = rj[4 + s]; }
    relax_load(P.iz, P.ms, 0, 12, k, IZ);
    cons_inv(Xi, IXi);
    cons_mul(IXi, Xj, D);
    cons_mul(IZ, D, E);
    double qe[4], rR[3];
    relax_quat(E, qe);
    const bool flip = qe[0] < 0.0;
    for (int r = 0; r < 3; r++) rR[r] = 2.0 * (flip ? -qe[1 + r] : qe[1 + r]);
    const double wt = P.wt[k], wr = P.wr[k];
    const double ct = wt * ((E[9] * E[9] + E[10] * E[10]) + E[11] * E[11]);
    const double cr = wr * ((rR[0] * rR[0] + rR[1] * rR[1]) + rR[2] * rR[2]);
    ec[(size_t)k * 2] = ct;
    ec[(size_t)k * 2 + 1] = cr;
    P.csum[k] = ct + cr;
    if (trial) continue;
    const double *A = IZ, *u = D + 9;
    for (int r = 0; r < 3; r++) {
      P.jac[(size_t)(r * 3 + 0) * P.ms + k] = A[r * 3 + 1] * u[2] - A[r * 3 + 2] * u[1];
      P.jac[(size_t)(r * 3 + 1) * P.ms + k] = A[r * 3 + 2] * u[0] - A[r * 3 + 0] * u[2];
      P.jac[(size_t)(r * 3 + 2) * P.ms + k] = A[r * 3 + 0] * u[1] - A[r * 3 + 1] * u[0];
    }
    for (int s = 0; s < 9; s++) {
      P.jac[(size_t)(9 + s) * P.ms + k] = E[s];
      P.jac[(size_t)(18 + s) * P.ms + k] = D[s];
    }
    for (int r = 0; r < 3; r++) {
      P.y[(size_t)r * P.ms + k] = wt * E[9 + r];
      P.y[(size_t)(3 + r) * P.ms + k] = wr * rR[r];
    }
  }
}

// one incident edge's share of J^T y
__device__ __forceinline__ void relax_contrib(const RelaxParams &P, int ent, double *c) {
  const int k = ent >> 1;
  double y[6];
  relax_load(P.y, P.ms, 0, 6, k, y);
  if ((ent & 1) == 0) {
    double A[9], B[9], DR[9];
    relax_load(P.iz, P.ms, 0, 9, k, A);
    relax_load(P.jac, P.ms, 0, 9, k, B);
    relax_load(P.jac, P.ms, 18, 9, k, DR);
    for (int r = 0; r < 3; r++) {
      c[r] = -relax_mtv(A, y, r);
      c[3 + r] = relax_mtv(B, y, r) - relax_mv(DR, y + 3, r);
    }
  } else {
    double ER[9];
    relax_load(P.jac, P.ms, 9, 9, k, ER);
    for (int r = 0; r < 3; r++) {
      c[r] = relax_mtv(ER, y, r);
      c[3 + r] = y[3 + r];
    }
  }
}

// z = M^-1 r through L (row-major 6x6, lower)
__device__ __forceinline__ void relax_solve(const double *L, const double *r, double *z) {
  double y[6];
#pragma unroll
  for (int a = 0; a < 6; a++) {
    double s = r[a];
#pragma unroll
    for (int k = 0; k < a; k++) s = s - L[a * 6 + k] * y[k];
    y[a] = s / L[a * 6 + a];
  }
#pragma unroll
  for (int a = 5; a >= 0; a--) {
    double s = y[a];
#pragma unroll
    for (int k = a + 1; k < 6; k++) s = s - L[k * 6 + a] * z[k];
    z[a] = s / L[a * 6 + a];
  }
}

__global__ __launch_bounds__(SGTD_RELAX_THREADS) void relax_setup_kernel(RelaxParams P) {
  if (P.st->done) return;
  const double lam = P.st->lambda;
  RELAX_GRID_LOOP(v, P.n) {
    double *r = P.r + (size_t)v * 6, *x = P.x + (size_t)v * 6, *p = P.p + (size_t)v * 6, *z = P.z + (size_t)v * 6;
    for (int a = 0; a < 6; a++) { x[a] = 0.0; p[a] = 0.0; }
    if (P.held[v]) {
      for (int a = 0; a < 6; a++) { r[a] = 0.0; z[a] = 0.0; }
      P.ok[v] = 0;
      continue;
    }
    double g[6], H[36];
    for (int a = 0; a < 6; a++) g[a] = 0.0;
    for (int a = 0; a < 36; a++) H[a] = 0.0;
    for (int at = P.off[v]; at < P.off[v + 1]; at++) {
      const int ent = P.ent[at], k = ent >> 1;
      double c[6];
      relax_contrib(P, ent, c);
      for (int a = 0; a < 6; a++) g[a] = g[a] + c[a];
      // the edge's 6x6 Jacobian with respect to this node, row by row
      const double wt = P.wt[k], wr = P.wr[k];
      double M0[9], M1[9];      // side 0: A and B, then D_R; side 1: E_R
      const bool is_i = (ent & 1) == 0;
      if (is_i) { relax_load(P.iz, P.ms, 0, 9, k, M0); relax_load(P.jac, P.ms, 0, 9, k, M1); }
      else relax_load(P.jac, P.ms, 9, 9, k, M0);
#pragma unroll
      for (int row = 0; row < 3; row++) {
        double J[6];
        for (int c3 = 0; c3 < 3; c3++) {
          J[c3] = is_i ? -M0[row * 3 + c3] : M0[row * 3 + c3];
          J[3 + c3] = is_i ? M1[row * 3 + c3] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
          for (int b = 0; b < 6; b++) H[a * 6 + b] = H[a * 6 + b] + (wt * J[a]) * J[b];
      }
      if (is_i) relax_load(P.jac, P.ms, 18, 9, k, M1);      // D_R
#pragma unroll
      for (int row = 0; row < 3; row++) {
        double J[6];
        for (int c3 = 0; c3 < 3; c3++) {
          J[c3] = 0.0;
          J[3 + c3] = is_i ? -M1[c3 * 3 + row] : (c3 == row ? 1.0 : 0.0);
        }
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
          for (int b = 0; b < 6; b++) H[a * 6 + b] = H[a * 6 + b] + (wr * J[a]) * J[b];
      }
    }
    // Cholesky of M = H + lambda H, column by column
    double L[36];
    for (int a = 0; a < 36; a++) L[a] = 0.0;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; c++) {
      double s = H[c * 6 + c] + lam * H[c * 6 + c];
#pragma unroll
      for (int k = 0; k < c; k++) s = s - L[c * 6 + k] * L[c * 6 + k];
      ok = ok && s > 0.0;
      L[c * 6 + c] = sqrt(s);
#pragma unroll
      for (int rr = c + 1; rr < 6; rr++) {
        double s2 = H[rr * 6 + c] + lam * H[rr * 6 + c];
#pragma unroll
        for (int k = 0; k < c; k++) s2 = s2 - L[rr * 6 + k] * L[c * 6 + k];
        L[rr * 6 + c] = s2 / L[c * 6 + c];
      }
    }
    double rv[6], zv[6];
    for (int a = 0; a < 6; a++) rv[a] = -g[a];
    relax_solve(L, rv, zv);
    for (int a = 0; a < 6; a++) { r[a] = rv[a]; z[a] = ok ? zv[a] : 0.0; }
    for (int a = 0; a < 36; a++) { P.H[(size_t)v * 36 + a] = H[a]; P.L[(size_t)v * 36 + a] = L[a]; }
    P.ok[v] = ok ? 1 : 0;
  }
}

__global__ __launch_bounds__(SGTD_RELAX_THREADS) void relax_cg_edge_kernel(RelaxParams P) {
  if (P.st->done || P.st->cg_done) return;
  const double beta = P.st->beta;
  RELAX_GRID_LOOP(k, P.m) {
    const size_t i = (size_t)P.ei[k] * 6, j = (size_t)P.ej[k] * 6;
    double pi[6], pj[6];
    for (int a = 0; a < 6; a++) { pi[a] = P.z[i + a] + beta * P.p[i + a]; pj[a] = P.z[j + a] + beta * P.p[j + a]; }
    double A[9], B[9], ER[9], DR[9];
    relax_load(P.iz, P.ms, 0, 9, k, A);
    relax_load(P.jac, P.ms, 0, 9, k, B);
    relax_load(P.jac, P.ms, 9, 9, k, ER);
    relax_load(P.jac, P.ms, 18, 9, k, DR);
    const double wt = P.wt[k], wr = P.wr[k];
    for (int r = 0; r < 3; r++) {
      const double et = (relax_mv(B, pi + 3, r) - relax_mv(A, pi, r)) + relax_mv(ER, pj, r);
      const double eR = pj[3 + r] - relax_mtv(DR, pi + 3, r);
      P.y[(size_t)r * P.ms + k] = wt * et;
      P.y[(size_t)(3 + r) * P.ms + k] = wr * eR;
    }
  }
}

__global__ __launch_bounds__(SGTD_RELAX_THREADS) void relax_cg_node_kernel(RelaxParams P) {
  if (P.st->done || P.st->cg_done) return;
  const double beta = P.st->beta, lam = P.st->lambda;
  RELAX_GRID_LOOP(v, P.n) {
    double *ap = P.ap + (size_t)v * 6, *p = P.p + (size_t)v * 6;
    if (P.held[v]) {
      for (int a = 0; a < 6; a++) ap[a] = 0.0;
      continue;
    }
    double pv[6], g[6];
    for (int a = 0; a < 6; a++) { pv[a] = P.z[(size_t)v * 6 + a] + beta * p[a]; g[a] = 0.0; }
    for (int at = P.off[v]; at < P.off[v + 1]; at++) {
      double c[6];
      relax_contrib(P, P.ent[at], c);
      for (int a = 0; a < 6; a++) g[a] = g[a] + c[a];
    }
    const double *H = P.H + (size_t)v * 36;
    for (int a = 0; a < 6; a++) {
      const double hp = ((((H[a * 6] * pv[0] + H[a * 6 + 1] * pv[1]) + H[a * 6 + 2] * pv[2]) + H[a * 6 + 3] * pv[3]) + H[a * 6 + 4] * pv[4]) + H[a * 6 + 5] * pv[5];
      ap[a] = g[a] + lam * hp;
      p[a] = pv[a];
    }
  }
}

__global__ __launch_bounds__(SGTD_RELAX_THREADS) void relax_cg_update_kernel(RelaxParams P) {
  if (P.st->done || P.st->cg_done) return;
  const double alpha = P.st->alpha;
  RELAX_GRID_LOOP(v, P.n) {
    if (P.held[v]) continue;      // (all of its vectors are 0)
    double rv[6], zv[6], L[36];
    for (int a = 0; a < 6; a++) {
      const size_t e = (size_t)v * 6 + a;
      P.x[e] = P.x[e] + alpha * P.p[e];
      rv[a] = P.r[e] - alpha * P.ap[e];
      P.r[e] = rv[a];
    }
    const bool ok = P.ok[v] != 0;
    for (int a = 0; a < 36; a++) L[a] = P.L[(size_t)v * 36 + a];
    relax_solve(L, rv, zv);
    for (int a = 0; a < 6; a++) P.z[(size_t)v * 6 + a] = ok ? zv[a] : 0.0;
  }
}

__global__ __launch_bounds__(SGTD_RELAX_THREADS) void relax_retract_kernel(RelaxParams P) {
  if (P.st->done) return;
  const int cur = P.st->cur;
  RELAX_GRID_LOOP(v, P.n) {
    const double *src = P.state + ((size_t)cur * P.n + v) * SGTD_RELAX_REC;
    double *dst = P.state + ((size_t)(cur ^ 1) * P.n + v) * SGTD_RELAX_REC;
    double rec[SGTD_RELAX_REC];
    for (int k = 0; k < SGTD_RELAX_REC; k++) rec[k] = src[k];
    if (P.ok[v]) {
      const double *x = P.x + (size_t)v * 6;
      const double h[3] = {0.5 * x[3], 0.5 * x[4], 0.5 * x[5]};
      const double w = rec[0], a = rec[1], b = rec[2], c = rec[3];
      double t2[3];
      for (int r = 0; r < 3; r++) t2[r] = relax_mv(rec + 7, x, r) + rec[4 + r];
      rec[0] = ((w - a * h[0]) - b * h[1]) - c * h[2];
      rec[1] = ((a + w * h[0]) + b * h[2]) - c * h[1];
      rec[2] = ((b + w * h[1]) + c * h[0]) - a * h[2];
      rec[3] = ((c + w * h[2]) + a * h[1]) - b * h[0];
      relax_unit(rec);
      for (int r = 0; r < 3; r++) rec[4 + r] = t2[r];
      relax_rot(rec, rec + 7);
    }
    for (int k = 0; k < SGTD_RELAX_REC; k++) dst[k] = rec[k];
  }
}

// the halving tree over the workgroup's SGTD_RELAX_W accumulators; every thread gets the result
template <bool MAX>
__device__ __forceinline__ double relax_tree(double acc, double *lds) {
  const int t = threadIdx.x;
  __syncthreads();      // (lds may still be read from the tree before)
  lds[t] = acc;
  __syncthreads();
  for (int s = SGTD_RELAX_W / 2; s >= 1; s >>= 1) {
    if (t < s) {
      const double a = lds[t], b = lds[t + s];
      lds[t] = MAX ? (b > a ? b : a) : a + b;
    }
    __syncthreads();
  }
  return lds[0];
}

__global__ __launch_bounds__(SGTD_RELAX_W) void relax_ctl_kernel(RelaxParams P, int mode) {
  __shared__ double lds[SGTD_RELAX_W];
  const RelaxState s = *P.st;
  if (s.done) return;
  if ((mode == RELAX_CTL_PQ || mode == RELAX_CTL_RZ) && s.cg_done) return;
  const int t = threadIdx.x;
  const long long n6 = (long long)P.n * 6;
  double acc = 0.0;
  if (mode == RELAX_CTL_COST0 || mode == RELAX_CTL_ACCEPT) {
    for (long long e = t; e < P.m; e += SGTD_RELAX_W) acc = acc + P.csum[e];
  } else {
    const double *u = mode == RELAX_CTL_PQ ? P.p : P.r, *v = mode == RELAX_CTL_PQ ? P.ap : P.z;
    for (long long e = t; e < n6; e += SGTD_RELAX_W) acc = acc + u[e] * v[e];
  }
  const double sum = relax_tree<false>(acc, lds);
  double maxd = 0.0;
  if (mode == RELAX_CTL_ACCEPT) {
    double m = 0.0;
    for (long long e = t; e < n6; e += SGTD_RELAX_W) {
      const double a = fabs(P.x[e]);
      m = a > m ? a : m;
    }
    maxd = relax_tree<true>(m, lds);
  }
  if (t != 0) return;
  RelaxState *st = P.st;
  switch (mode) {
    case RELAX_CTL_COST0:
      st->cost = sum;
      st->cost_before = sum;
      if (P.all_held) { st->status = 3; st->done = 1; }
      break;
    case RELAX_CTL_RZ0:
      st->rz = sum; st->rz0 = sum; st->thr = P.tol2 * sum; st->beta = 0.0; st->cg_done = 0;
      if (!(sum > 0.0)) { st->status = 0; st->done = 1; }
      break;
    case RELAX_CTL_PQ:
      if (!(sum > 0.0)) st->cg_done = 1;
      else st->alpha = s.rz / sum;
      break;
    case RELAX_CTL_RZ:
      st->cg_total = s.cg_total + 1;
      if (sum <= s.thr) st->cg_done = 1;
      else { st->beta = sum / s.rz; st->rz = sum; }
      break;
    case RELAX_CTL_ACCEPT: {
      int status = -1;
      if (sum < s.cost) {
        st->cur = s.cur ^ 1;
        st->cost = sum;
        st->accepted = s.accepted + 1;
        const double l = s.lambda / 3.0;
        st->lambda = l > P.lmin ? l : P.lmin;
        if (maxd <= P.step_tol) status = 0;
      } else {
        const double l = 3.0 * s.lambda;
        st->lambda = l;
        if (l > P.lmax) status = 2;
      }
      st->outer = s.outer + 1;
      if (status < 0 && s.outer + 1 >= P.max_outer) status = 1;
      if (status >= 0) { st->status = status; st->done = 1; }
      break;
    }
  }
}
