// consistency_kernels.hip.h — sgtd_consistent_loops: pairwise consistency of loop closures and the greedy clique.
//
// The rule is the one include/sgtd_accel.h states at sgtd_consistent_loops: all f64, every operation rounded once (the
// build's -ffp-contract=off), the sums in the order written there.  inv() and mul() below are that comment's.
//
//   cons_prepare_kernel   one thread per edge: gathers B = pose of frame_b and A = pose_a row or pose of frame_a from the
//                         uploaded pose store, forms P = mul(B, T), marks validity, and writes P, inv(P), A, inv(A) as 48
//                         f64 streams of stride `ns` (structure of arrays): inv() depends on one edge only, so it is taken
//                         here once per edge, not once per pair.
//   cons_pair_kernel      the hot path.  A workgroup stages the 48 streams of SGTD_CONS_TILE columns in LDS and runs
//                         SGTD_CONS_ROWS rows over them; a wave owns a row i and 64 columns per step: lane l decides the
//                         pair (i, 64 w + l), the ballot is word w of row i, lane 0 stores it.  The pair is always taken
//                         with the lower index first (adj(i, j) = adj(j, i) = the decision of (min, max)): where a whole
//                         word lies above or below the diagonal the roles are wave-uniform, only the diagonal word
//                         selects per lane.  Every word of the n x words matrix is stored exactly once, columns >= n and
//                         invalid edges as 0: nothing relies on the buffer's earlier contents.
//   cons_init_kernel      P = the valid edges (bit mask), |P|, and the result arrays' defaults.
//   cons_count_kernel     one round's d(u) = popcount(row(u) & P) for every u in P: a wave per row (grid stride), its
//                         best (d, lowest u) folded into one 64-bit atomic maximum per wave; counts the u with
//                         d(u) = |P| - 1.  Round 0's d(u) is the edge's degree.
//   cons_select_kernel    one workgroup: the end (P empty), the clique shortcut (every d(u) = |P| - 1: the rest of P joins
//                         in ascending order), or the pick v and P &= row(v) with the new |P|.
// A round is count + select on one stream; both return at once when the state says the choice is complete, so rounds are
// enqueued in groups and the host looks at the state once per group.
#pragma once
#include "common.hip.h"

#define SGTD_CONS_THREADS 256
#define SGTD_CONS_TILE 128      // columns a workgroup of the pair pass stages (two row words)
#define SGTD_CONS_ROWS 64       // rows it runs over them (16 per wave)
#define SGTD_CONS_STREAMS 48    // P 0..11, inv(P) 12..23, A 24..35, inv(A) 36..47; a pose: rot row-major (9), t (3)
#define SGTD_CONS_SELECT_THREADS 512   // one thread per word of P: SGTD_MAX_LOOP_EDGES / 64

struct ConsState {
  u64 best;      // max over the round's u of (d(u) + 1) << 32 | ~u: the largest d, then the lowest index
  int psize;     // |P|
  int n_full;    // the round's u with d(u) == |P| - 1
  int n_set;     // |C|
  int round;     // rounds done
  int done;      // the choice is complete
  int pad;
};

// Y = inv(X)
__device__ __forceinline__ void cons_inv(const double *X, double *Y) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) Y[r * 3 + c] = X[c * 3 + r];
  for (int r = 0; r < 3; r++) Y[9 + r] = -((Y[r * 3 + 0] * X[9] + Y[r * 3 + 1] * X[10]) + Y[r * 3 + 2] * X[11]);
}

// Z = mul(X, Y)
__device__ __forceinline__ void cons_mul(const double *X, const double *Y, double *Z) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) Z[r * 3 + c] = (X[r * 3 + 0] * Y[c] + X[r * 3 + 1] * Y[3 + c]) + X[r * 3 + 2] * Y[6 + c];
    Z[9 + r] = ((X[r * 3 + 0] * Y[9] + X[r * 3 + 1] * Y[10]) + X[r * 3 + 2] * Y[11]) + X[9 + r];
  }
}

// the decision of a pair lo < hi from inv(P_lo), P_hi, inv(A_hi), A_lo.  Of Z = mul(U, V) only the diagonal and the
// translation are formed (the rule reads nothing else).  A NaN fails both comparisons.
__device__ __forceinline__ bool cons_decide(const double *ip_lo, const double *p_hi, const double *ia_hi, const double *a_lo,
                                            double tt, double min_trace) {
  double U[12], V[12];
  cons_mul(ip_lo, p_hi, U);
  cons_mul(ia_hi, a_lo, V);
  double zt[3], zd[3];
  for (int r = 0; r < 3; r++) {
    zt[r] = ((U[r * 3 + 0] * V[9] + U[r * 3 + 1] * V[10]) + U[r * 3 + 2] * V[11]) + U[9 + r];
    zd[r] = (U[r * 3 + 0] * V[r] + U[r * 3 + 1] * V[3 + r]) + U[r * 3 + 2] * V[6 + r];
  }
  const double d2 = (zt[0] * zt[0] + zt[1] * zt[1]) + zt[2] * zt[2];
  const double tr = (zd[0] + zd[1]) + zd[2];
  return d2 <= tt && tr >= min_trace;
}

struct ConsPrepareParams {
  const float *store;              // the pose store: 12 f32 per frame id
  const unsigned char *has;        // ... and whether the id has a pose
  u32 n_ids;
  const u32 *frame_a, *frame_b;    // frame_a: nullptr when pose_a is given without ids
  const double *rel;               // [n * 12]
  const float *pose_a;             // [n * 12] or nullptr
  int n;
  size_t ns;                       // stream stride
  double *soa;
  unsigned char *valid;
};

// a row-major 3x4 [R | t] in f32 -> rot (9), t (3) in f64
__device__ __forceinline__ void cons_widen(const float *m, double *X) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) X[r * 3 + c] = (double)m[r * 4 + c];
    X[9 + r] = (double)m[r * 4 + 3];
  }
}

__global__ __launch_bounds__(SGTD_CONS_THREADS) void cons_prepare_kernel(ConsPrepareParams p) {
  const int i = blockIdx.x * SGTD_CONS_THREADS + threadIdx.x;
  if (i >= p.n) return;
  double B[12], A[12], T[12], P[12], IP[12], IA[12];
  for (int k = 0; k < 12; k++) { B[k] = 0.0; A[k] = 0.0; T[k] = p.rel[(size_t)i * 12 + k]; }
  bool ok = true;
  const u32 fb = p.frame_b[i];
  if (fb < p.n_ids && p.has[fb]) cons_widen(p.store + (size_t)fb * 12, B); else ok = false;
  if (p.pose_a) {
    cons_widen(p.pose_a + (size_t)i * 12, A);
  } else {
    const u32 fa = p.frame_a[i];
    if (fa < p.n_ids && p.has[fa]) cons_widen(p.store + (size_t)fa * 12, A); else ok = false;
  }
  for (int k = 0; k < 12; k++) ok = ok && __builtin_isfinite(B[k]) && __builtin_isfinite(A[k]) && __builtin_isfinite(T[k]);
  cons_mul(B, T, P);
  cons_inv(P, IP);
  cons_inv(A, IA);
  for (int k = 0; k < 12; k++) {
    p.soa[(size_t)k * p.ns + i] = ok ? P[k] : 0.0;
    p.soa[(size_t)(12 + k) * p.ns + i] = ok ? IP[k] : 0.0;
    p.soa[(size_t)(24 + k) * p.ns + i] = ok ? A[k] : 0.0;
    p.soa[(size_t)(36 + k) * p.ns + i] = ok ? IA[k] : 0.0;
  }
  p.valid[i] = ok ? 1 : 0;
}

struct ConsPairParams {
  const double *soa;
  size_t ns;
  const unsigned char *valid;
  int n;
  u32 words;           // per row: ceil(n / 64)
  double tt, min_trace;
  u64 *rows;           // [n * words]
};

// grid: x = column tiles (ceil(words / 2)), y = row blocks (ceil(n / SGTD_CONS_ROWS))
__global__ __launch_bounds__(SGTD_CONS_THREADS) void cons_pair_kernel(ConsPairParams p) {
  __shared__ double tile[SGTD_CONS_STREAMS][SGTD_CONS_TILE];
  __shared__ unsigned char tile_valid[SGTD_CONS_TILE];
  const int c0 = blockIdx.x * SGTD_CONS_TILE;
  for (int x = threadIdx.x; x < SGTD_CONS_STREAMS * SGTD_CONS_TILE; x += SGTD_CONS_THREADS) {
    const int k = x / SGTD_CONS_TILE, c = x % SGTD_CONS_TILE, j = c0 + c;
    tile[k][c] = j < p.n ? p.soa[(size_t)k * p.ns + j] : 0.0;
  }
  if (threadIdx.x < SGTD_CONS_TILE) {
    const int j = c0 + (int)threadIdx.x;
    tile_valid[threadIdx.x] = j < p.n ? p.valid[j] : 0;
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / SGTD_WAVE)), lane = lane_id();
  for (int rr = wave; rr < SGTD_CONS_ROWS; rr += SGTD_CONS_THREADS / SGTD_WAVE) {
    const int i = blockIdx.y * SGTD_CONS_ROWS + rr;      // (wave-uniform)
    if (i >= p.n) break;
    const bool vi = p.valid[i] != 0;
    double ri[SGTD_CONS_STREAMS];
    if (vi)
#pragma unroll
      for (int k = 0; k < SGTD_CONS_STREAMS; k++) ri[k] = p.soa[(size_t)k * p.ns + i];
    for (int s = 0; s < SGTD_CONS_TILE / SGTD_WAVE; s++) {
      const u32 w = blockIdx.x * (SGTD_CONS_TILE / SGTD_WAVE) + s;
      if (w >= p.words) break;
      const int cs = c0 + s * SGTD_WAVE, c = s * SGTD_WAVE + lane, j = cs + lane;
      bool ok = false;
      if (vi) {
        double x0[12], x1[12];
        if (cs > i) {                                  // every column above the diagonal: the row is the lower index
#pragma unroll
          for (int k = 0; k < 12; k++) { x0[k] = tile[k][c]; x1[k] = tile[36 + k][c]; }
          ok = cons_decide(ri + 12, x0, x1, ri + 24, p.tt, p.min_trace);
        } else if (cs + SGTD_WAVE - 1 < i) {           // every column below it: the column is
#pragma unroll
          for (int k = 0; k < 12; k++) { x0[k] = tile[12 + k][c]; x1[k] = tile[24 + k][c]; }
          ok = cons_decide(x0, ri, ri + 36, x1, p.tt, p.min_trace);
        } else {                                       // the diagonal's word: by lane
          const bool col_lo = j < i;
          double y0[12], y1[12];
#pragma unroll
          for (int k = 0; k < 12; k++) {
            x0[k] = col_lo ? tile[12 + k][c] : ri[12 + k];       // inv(P_lo)
            y0[k] = col_lo ? ri[k] : tile[k][c];                 // P_hi
            x1[k] = col_lo ? ri[36 + k] : tile[36 + k][c];       // inv(A_hi)
            y1[k] = col_lo ? tile[24 + k][c] : ri[24 + k];       // A_lo
          }
          ok = cons_decide(x0, y0, x1, y1, p.tt, p.min_trace);
        }
        ok = ok && tile_valid[c] != 0 && j != i;
      }
      const u64 m = __ballot(ok);
      if (lane == 0) p.rows[(size_t)i * p.words + w] = m;
    }
  }
}

// grid: one wave per word of P.  st has been zeroed on the stream before.
__global__ __launch_bounds__(SGTD_CONS_THREADS) void cons_init_kernel(const unsigned char *valid, int n, u32 words, u64 *pmask,
                                                                      int *in_set, int *degree, int *pick, ConsState *st) {
  const u32 w = (blockIdx.x * SGTD_CONS_THREADS + threadIdx.x) / SGTD_WAVE;
  if (w >= words) return;      // (whole waves)
  const long long j = (long long)w * SGTD_WAVE + lane_id();
  const bool v = j < n && valid[j] != 0;
  if (j < n) { in_set[j] = 0; degree[j] = -1; pick[j] = -1; }
  const u64 m = __ballot(v);
  if (lane_id() == 0) {
    pmask[w] = m;
    if (m) atomicAdd(&st->psize, __popcll(m));
  }
}

__global__ __launch_bounds__(SGTD_CONS_THREADS) void cons_count_kernel(const u64 *rows, const u64 *pmask, int n, u32 words, int *degree,
                                                                       ConsState *st) {
  if (st->done) return;
  const int psize = st->psize, round = st->round;
  if (psize == 0) return;
  const int n_waves = gridDim.x * (SGTD_CONS_THREADS / SGTD_WAVE);
  const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * SGTD_CONS_THREADS + threadIdx.x) / SGTD_WAVE)), lane = lane_id();
  u64 best = 0;
  int full = 0;
  for (int u = wave; u < n; u += n_waves) {
    if (!((pmask[u >> 6] >> (u & 63)) & 1ull)) continue;     // (wave-uniform)
    u32 c = 0;
    for (u32 w = lane; w < words; w += SGTD_WAVE) c += (u32)__popcll(rows[(size_t)u * words + w] & pmask[w]);
    const u32 d = wave_sum(c);
    if (round == 0 && lane == 0) degree[u] = (int)d;
    const u64 key = ((u64)(d + 1) << 32) | (u64)(0xFFFFFFFFu - (u32)u);
    best = key > best ? key : best;
    full += (int)d == psize - 1;
  }
  if (lane == 0 && best) {
    atomicMax(&st->best, best);
    if (full) atomicAdd(&st->n_full, full);
  }
}

// one workgroup of SGTD_CONS_SELECT_THREADS: thread t owns word t of P
__global__ __launch_bounds__(SGTD_CONS_SELECT_THREADS) void cons_select_kernel(const u64 *rows, u64 *pmask, u32 words, int *in_set,
                                                                               int *pick, ConsState *st) {
  __shared__ u32 wave_tot[SGTD_CONS_SELECT_THREADS / SGTD_WAVE];
  if (st->done) return;
  const u32 t = threadIdx.x, wv = t / SGTD_WAVE;
  const u64 best = st->best;
  const int psize = st->psize, n_full = st->n_full, n_set = st->n_set;
  __syncthreads();      // (everyone has read the state before thread 0 writes it)
  if (psize == 0 || best == 0ull) {      // (P is empty; a round over a non-empty P always leaves a best)
    if (t == 0) st->done = 1;
    return;
  }
  const bool clique = n_full == psize;
  const u32 v = 0xFFFFFFFFu - (u32)(best & 0xFFFFFFFFull);
  u64 m = t < words ? pmask[t] : 0ull;
  if (!clique && t < words) m &= rows[(size_t)v * words + t];
  const u32 cnt = (u32)__popcll(m);
  const u32 incl = wave_incl_scan(cnt);
  if (lane_id() == SGTD_WAVE - 1) wave_tot[wv] = incl;
  __syncthreads();
  u32 before = 0, total = 0;
  for (u32 k = 0; k < SGTD_CONS_SELECT_THREADS / SGTD_WAVE; k++) {
    before += k < wv ? wave_tot[k] : 0;
    total += wave_tot[k];
  }
  if (clique) {
    // the rest of P is a clique: each round would take its lowest index and leave the others with d = |P| - 2
    u32 pos = (u32)n_set + before + incl - cnt;
    for (u64 b = m; b; b &= b - 1) {
      const u32 j = t * SGTD_WAVE + (u32)__builtin_ctzll(b);
      pick[j] = (int)pos++;
      in_set[j] = 1;
    }
    if (t < words) pmask[t] = 0ull;
    if (t == 0) { st->n_set = n_set + psize; st->psize = 0; st->round++; st->done = 1; }
    return;
  }
  if (t < words) pmask[t] = m;
  if (t == 0) {
    pick[v] = n_set;
    in_set[v] = 1;
    st->n_set = n_set + 1;
    st->psize = (int)total;
    st->round++;
    st->best = 0ull;
    st->n_full = 0;
    if (total == 0) st->done = 1;
  }
}
