// consensus_kernels.hip.h — sgtd_pose_consensus: per query, the verified candidates grouped by the world pose they
// imply, the greedy mutually consistent set, and one fused pose.
//
// The rule is the one include/sgtd_accel.h states at sgtd_pose_consensus: all f64, every operation rounded once (the
// build's -ffp-contract=off), every sum in the order written there.  inv() and mul() are consistency_kernels.hip.h's,
// QUAT, UNIT and ROT relax_kernels.hip.h's.
//
//   consensus_kernel      one wave per query (one workgroup of 64 threads), lane k = candidate k.  A lane gathers its
//                         frame's pose B from the uploaded pose store, forms P = mul(B, T), inv(P) and QUAT(P's rotation),
//                         and leaves them with its score in LDS as streams of 64 (lane-major: conflict-free to write, one
//                         broadcast to read).  Pairs: a wave-uniform loop over l = 0 .. cn-1, lane k decides the pair
//                         (k, l) with the lower index first and sets bit l of its own row, so row k of the query's 64 x 64
//                         bit matrix lives in lane k's registers.  Greedy: on the masks, inside the wave: d(k) is a
//                         popcount, the pick the wave maximum of (d + 1) << 6 | (63 - k), its row a readlane; the clique
//                         shortcut takes the rest of P by its rank below the lane.  Fusion and figures: wave-uniform
//                         loops over the member bits in ascending order, every lane forming the same sums from the LDS
//                         streams; lane 0 stores the query's outputs, lane k < cn those of candidate k.
// No atomics, no global scratch, no early exit (the cross-lane steps need all 64 lanes); every output word is stored
// exactly once, those of invalid candidates and of queries without one included.
#pragma once
#include "relax_kernels.hip.h"

#define SGTD_CONSENSUS_STREAMS 29   // P 0..11, inv(P) 12..23, q 24..27, score 28; a pose: rot row-major (9), t (3)

struct ConsensusParams {
  const float *store;              // the pose store: 12 f32 per frame id
  const unsigned char *has;        // ... and whether the id has a pose
  u32 n_ids;
  const int *n_cand;               // [nq]
  const int *cand_frame;           // [nq * cn]
  const double *score;             // [nq * cn]
  const double *rel;               // [nq * cn * 12]
  int cn;                          // 1 .. 64
  double tt, min_trace;
  double *pose;                    // [nq * 12] row-major 3x4 [R | t]
  double *figs;                    // [nq * 3] support_score, spread_t2, spread_trace
  u64 *mask;                       // [nq]
  int *counts;                     // [nq * 3] n_valid, n_set, seed
  u64 *rows;                       // [nq * cn]
  int *degree, *pick;              // [nq * cn]
};

// the 64 bits of lane `src` (wave-uniform), in every lane
__device__ __forceinline__ u64 consensus_row_of(u64 v, int src) {
  const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)v, src), hi = (u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), src);
  return ((u64)hi << 32) | lo;
}

// grid: one workgroup (one wave) per query
__global__ __launch_bounds__(SGTD_WAVE) void consensus_kernel(ConsensusParams p) {
  __shared__ double s[SGTD_CONSENSUS_STREAMS][SGTD_WAVE];
  const int q = blockIdx.x, k = lane_id(), cn = p.cn;
  const size_t base = (size_t)q * cn;
  const double nan = __builtin_nan("");

  // ---- validity, P = mul(B, T), inv(P), QUAT
  double B[12], T[12], P[12], IP[12], quat[4];
  for (int i = 0; i < 12; i++) { B[i] = 0.0; T[i] = 0.0; }
  double sc = -1.0;
  bool ok = k < cn && k < p.n_cand[q];
  if (ok) {
    sc = p.score[base + k];
    ok = sc >= 0.0;
    for (int i = 0; i < 12; i++) T[i] = p.rel[(base + k) * 12 + i];
    const u32 f = (u32)p.cand_frame[base + k];
    if (f < p.n_ids && p.has[f]) cons_widen(p.store + (size_t)f * 12, B); else ok = false;
  }
  for (int i = 0; i < 12; i++) ok = ok && __builtin_isfinite(B[i]) && __builtin_isfinite(T[i]);
  cons_mul(B, T, P);
  cons_inv(P, IP);
  relax_quat(P, quat);
  for (int i = 0; i < 12; i++) { s[i][k] = P[i]; s[12 + i][k] = IP[i]; }
  for (int i = 0; i < 4; i++) s[24 + i][k] = quat[i];
  s[28][k] = sc;
  __syncthreads();
  const u64 valid = __ballot(ok);

  // ---- the rows: bit l of lane k = the decision of (min(k, l), max(k, l))
  u64 row = 0ull;
  for (int l = 0; l < cn; l++) {
    if (!((valid >> l) & 1ull)) continue;      // (wave-uniform)
    const bool k_lo = k < l;
    double x[12], y[12];                       // inv(P_lo), P_hi
    for (int i = 0; i < 12; i++) {
      const double pl = s[i][l], ipl = s[12 + i][l];
      x[i] = k_lo ? IP[i] : ipl;
      y[i] = k_lo ? pl : P[i];
    }
    double zt[3], zd[3];
    for (int r = 0; r < 3; r++) {
      zt[r] = ((x[r * 3 + 0] * y[9] + x[r * 3 + 1] * y[10]) + x[r * 3 + 2] * y[11]) + x[9 + r];
      zd[r] = (x[r * 3 + 0] * y[r] + x[r * 3 + 1] * y[3 + r]) + x[r * 3 + 2] * y[6 + r];
    }
    const double d2 = (zt[0] * zt[0] + zt[1] * zt[1]) + zt[2] * zt[2];
    const double tr = (zd[0] + zd[1]) + zd[2];
    const bool agree = ok && k != l && d2 <= p.tt && tr >= p.min_trace;
    row |= (u64)(agree ? 1 : 0) << l;
  }

  // ---- the greedy choice on the masks
  u64 pm = valid, members = 0ull;
  int n_set = 0, my_pick = -1, seed = -1;
  while (pm) {                                 // (wave-uniform)
    const bool in_p = ((pm >> k) & 1ull) != 0;
    const int psize = __popcll(pm);
    const u32 d = (u32)__popcll(row & pm);
    if (__ballot(in_p && (int)d == psize - 1) == pm) {
      // the rest of P is a clique: each round would take its lowest index
      if (in_p) my_pick = n_set + __popcll(pm & lanemask_lt());
      if (n_set == 0) seed = __builtin_ctzll(pm);
      members |= pm;
      n_set += psize;
      break;
    }
    const u32 key = wave_max_u32(in_p ? ((d + 1u) << 6) | (u32)(63 - k) : 0u);
    const int v = __builtin_amdgcn_readfirstlane(63 - (int)(key & 63u));
    if (k == v) my_pick = n_set;
    if (n_set == 0) seed = v;
    members |= 1ull << v;
    n_set++;
    pm &= consensus_row_of(row, v);
  }

  // ---- fusion over the members in ascending index
  double fused[12], support = 0.0, spread_t2 = nan, spread_tr = nan;
  for (int i = 0; i < 12; i++) fused[i] = nan;
  if (n_set > 0) {
    double ts[3] = {0.0, 0.0, 0.0}, Q[4] = {0.0, 0.0, 0.0, 0.0}, qs[4];
    for (int i = 0; i < 4; i++) qs[i] = s[24 + i][seed];
    for (u64 b = members; b; b &= b - 1) {
      const int m = __builtin_ctzll(b);
      for (int c = 0; c < 3; c++) ts[c] = ts[c] + s[9 + c][m];
      double qm[4];
      for (int i = 0; i < 4; i++) qm[i] = s[24 + i][m];
      const double dot = ((qm[0] * qs[0] + qm[1] * qs[1]) + qm[2] * qs[2]) + qm[3] * qs[3];
      for (int i = 0; i < 4; i++) Q[i] = Q[i] + (dot < 0.0 ? -qm[i] : qm[i]);
      support = support + s[28][m];
    }
    double that[3], R[9];
    for (int c = 0; c < 3; c++) that[c] = ts[c] / (double)n_set;
    relax_unit(Q);
    relax_rot(Q, R);
    bool first = true;
    for (u64 b = members; b; b &= b - 1) {
      const int m = __builtin_ctzll(b);
      double e[3], rr[3];
      for (int c = 0; c < 3; c++) {
        e[c] = s[9 + c][m] - that[c];
        rr[c] = (R[c * 3 + 0] * s[c * 3 + 0][m] + R[c * 3 + 1] * s[c * 3 + 1][m]) + R[c * 3 + 2] * s[c * 3 + 2][m];
      }
      const double e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
      const double tr = (rr[0] + rr[1]) + rr[2];
      spread_t2 = first ? e2 : (e2 > spread_t2 ? e2 : spread_t2);
      spread_tr = first ? tr : (tr < spread_tr ? tr : spread_tr);
      first = false;
    }
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) fused[r * 4 + c] = R[r * 3 + c];
      fused[r * 4 + 3] = that[r];
    }
  }

  // ---- outputs
  if (k == 0) {
    for (int i = 0; i < 12; i++) p.pose[(size_t)q * 12 + i] = fused[i];
    p.figs[(size_t)q * 3 + 0] = support;
    p.figs[(size_t)q * 3 + 1] = spread_t2;
    p.figs[(size_t)q * 3 + 2] = spread_tr;
    p.mask[q] = members;
    p.counts[(size_t)q * 3 + 0] = __popcll(valid);
    p.counts[(size_t)q * 3 + 1] = n_set;
    p.counts[(size_t)q * 3 + 2] = seed;
  }
  if (k < cn) {
    p.rows[base + k] = row;
    p.degree[base + k] = ok ? __popcll(row) : -1;
    p.pick[base + k] = my_pick;
  }
}
