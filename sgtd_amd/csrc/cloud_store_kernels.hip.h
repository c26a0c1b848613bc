// cloud_store_kernels.hip.h — sgtd_set_frame_clouds / sgtd_register_stored / sgtd_register_stored_loops: what the cloud
// store adds to register_kernels.hip.h, whose seven kernels run unchanged over the store's arena.
//
// The arena is one array of points (3 floats each) and one of covariances (9 doubles each); cloud c of the arena has the
// points pt_off[c] .. pt_off[c + 1].  The stored clouds ("slots") come first, in arrival order; a call's own clouds are
// packed behind the last slot for the length of the call.
//
//   store_pack_kernel     a lane per float: points of stride 3 or 4 (a device array: the caller's, or the host's points
//                         staged) into the arena's 3-float layout, from a given point on
//   store_compact_kernel  a lane per element (9 of the covariance, 3 of the point) of the live points: the live slots move
//                         to the front of NEW arrays in their order (never in place); the slot of an element by binary
//                         search over the slots' new first points
//   store_pairs_kernel    a wave per query of a verified batch: sgtd_register_stored_loops' pairs.  Lane c holds candidate
//                         c (candidate_num <= 64); its rank is the number of candidates with a result that come before it
//                         by (-score, index), counted over 64 shuffles (no sort, and stable by construction); the first
//                         max_per_query ranks are taken, and of those the ones whose frame has a slot are kept.  Pass 0
//                         leaves the count of kept candidates per query; the host scans the counts (device_scan); pass 1
//                         writes query q's rows from first[q] on in rank order: (query, candidate, frame, slot) and the
//                         start pose of the named stage.
// Every index that multiplies a point number is 64 bits wide: a store of 2^27 points has 2^30 covariance doubles and
// passes 2^31 bytes of points.  No atomics, no LDS.
#pragma once
#include "common.hip.h"

#define SGTD_STORE_THREADS 256
#define SGTD_STORE_NONE (-1)         // frame -> slot table: the frame has no cloud

__global__ __launch_bounds__(SGTD_STORE_THREADS) void store_pack_kernel(const float *src, int stride, long long n_points, float *dst) {
  const long long n = n_points * 3, step = (long long)gridDim.x * SGTD_STORE_THREADS;
  for (long long k = (long long)blockIdx.x * SGTD_STORE_THREADS + threadIdx.x; k < n; k += step) {
    const long long p = k / 3;
    dst[(size_t)k] = src[(size_t)p * stride + (size_t)(k - p * 3)];
  }
}

struct StoreMoveParams {
  const float *pts_in;
  const double *cov_in;
  float *pts_out;
  double *cov_out;
  const long long *from, *to;        // [n_live + 1]: a live slot's first point in the old and in the new arrays; to[n_live] = total
  int n_live;
  long long total;                   // live points
};

__global__ __launch_bounds__(SGTD_STORE_THREADS) void store_compact_kernel(StoreMoveParams P) {
  const long long n = P.total * 12, step = (long long)gridDim.x * SGTD_STORE_THREADS;
  for (long long k = (long long)blockIdx.x * SGTD_STORE_THREADS + threadIdx.x; k < n; k += step) {
    const long long g = k / 12;
    const int c = (int)(k - g * 12);
    // the last slot whose first new point is <= g: slots of no points share their first point with the next one
    int lo = 0, hi = P.n_live;
    while (hi - lo > 1) {
      const int mid = (lo + hi) / 2;
      if (P.to[mid] <= g) lo = mid; else hi = mid;
    }
    const long long s = P.from[lo] + (g - P.to[lo]);
    if (c < 9) P.cov_out[(size_t)g * 9 + c] = P.cov_in[(size_t)s * 9 + c];
    else P.pts_out[(size_t)g * 3 + (c - 9)] = P.pts_in[(size_t)s * 3 + (c - 9)];
  }
}

struct StorePairParams {
  const double *score;               // [nq][cand_num]: verify_score
  const int *n_cand, *cand_frame;    // [nq], [nq][cand_num]
  const double *pose;                // [nq][cand_num][12]: the named stage's relative poses
  const int *slot_of;                // [n_ids]: frame id -> slot, or SGTD_STORE_NONE
  u32 n_ids;
  int cand_num, nq, max_per_query;
  u32 *count;                        // [nq + 1] (the last stays 0: its scan is the total)
  const u32 *first;                  // [nq + 1]: the counts' exclusive scan (pass 1)
  int4 *rows;                        // [pairs]: query, candidate, frame, slot
  double *init;                      // [pairs][12]
};

__global__ __launch_bounds__(SGTD_STORE_THREADS) void store_pairs_kernel(StorePairParams P, int pass) {
  const int lane = threadIdx.x & 63, q = blockIdx.x * (SGTD_STORE_THREADS / 64) + (threadIdx.x >> 6);
  if (q >= P.nq) return;             // (a whole wave leaves)
  const size_t at = (size_t)q * P.cand_num + lane;
  const bool mine = lane < P.cand_num && lane < P.n_cand[q];
  const double s = mine ? P.score[at] : -1.0;
  const int valid = mine && s >= 0.0 ? 1 : 0;      // (NaN: no result)
  int rank = 0;
  for (int j = 0; j < P.cand_num; j++) {
    const double sj = __shfl(s, j, 64);
    const int vj = __shfl(valid, j, 64);
    if (vj && (sj > s || (sj == s && j < lane))) rank++;
  }
  int frame = 0, slot = SGTD_STORE_NONE;
  if (valid && rank < P.max_per_query) {
    frame = P.cand_frame[at];
    if ((u32)frame < P.n_ids) slot = P.slot_of[(u32)frame];
  }
  const int kept = slot != SGTD_STORE_NONE ? 1 : 0;
  if (pass == 0) {
    const unsigned long long m = __ballot(kept);
    if (lane == 0) P.count[q] = (u32)__popcll(m);
    return;
  }
  u32 pos = P.first[q];
  for (int j = 0; j < P.cand_num; j++) {
    const int kj = __shfl(kept, j, 64), rj = __shfl(rank, j, 64);
    if (kj && rj < rank) pos++;
  }
  if (!kept) return;
  P.rows[pos] = make_int4(q, lane, frame, slot);
  for (int a = 0; a < 12; a++) P.init[(size_t)pos * 12 + a] = P.pose[at * 12 + a];
}
