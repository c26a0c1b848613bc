// stored_local_kernels.hip.h — sgtd_register_stored_local_loops: the pairs of a verified batch, the local voxel maps of
// their candidate frames and the members' relative poses, formed on the device from the verification's results, the cloud
// store's frame -> slot table and the pose store (the rule: include/sgtd_accel.h).  The registration itself is
// voxel_register_kernels.hip.h's, over the cloud store's arena.
//
//   sl_eligible_kernel    a lane per frame id: eligible = a stored cloud, a stored pose, 12 finite floats; the translation
//                         widened to f64 as three streams (what the members kernel reads, coalesced); the map flags zeroed
//   sl_rows_kernel        store_pairs_kernel's wave per query (rank by (-score, index) over 64 shuffles) with the
//                         eligibility test.  Pass 0: the count of kept candidates per query, and flag[frame] = 1 (every
//                         writer stores the same word).  The host scans counts and flags (device_scan); pass 1 writes the
//                         rows (query, candidate, frame, map = the scan of the flags at the frame) and the start poses
//   sl_map_frames_kernel  a lane per frame id: map_frame[map_of[id]] = id where the flag is set: ascending frame id
//   sl_members_kernel     a workgroup per map, streaming the translations of every id (any number of ids: nothing is held
//                         in LDS but a 256-bin histogram).  Pass 0: the members in reach are counted; where max_members
//                         cuts, the (m - 1)-th smallest key (bits of d2, id) is found by a radix select, 12 passes of 8 bits
//                         from the top, each a histogram over the keys that share the digits chosen so far (d2 >= +0 is
//                         ordered by its bit pattern; the keys are distinct, so the threshold keeps exactly m - 1); the
//                         count, the members' points and the threshold are left per map.  Pass 1, once the host has turned
//                         the counts into offsets: the frame itself, then the kept ids in ascending order by ballot prefix
//                         sums over chunks of 256 ids (never by arrival); each member's slot, map and size
//   sl_poses_kernel       a lane per member: the identity written out for the map's own frame, mul(inv(T_j), T_i) with
//                         cons_inv / cons_mul for the others
// The only atomics are LDS integer adds into the histogram (counts: order-free).  All arithmetic on poses is f64, every
// operation rounded once (the build's -ffp-contract=off).
#pragma once
#include "cloud_store_kernels.hip.h"
#include "consistency_kernels.hip.h"

#define SGTD_SL_THREADS 256
#define SGTD_SL_CUT_ALL 0            // every member in reach is kept
#define SGTD_SL_CUT_KEY 1            // the members whose key is <= the threshold
#define SGTD_SL_CUT_NONE 2           // max_members == 1: the frame alone

struct StoredLocalParams {
  // the verified batch
  const double *score;               // [nq][cand_num]
  const int *n_cand, *cand_frame;    // [nq], [nq][cand_num]
  const double *pose;                // [nq][cand_num][12]: the named stage's relative poses
  int cand_num, nq, max_per_query;
  // the stores
  const int *slot_of;                // [n_ids]: frame id -> slot, or SGTD_STORE_NONE
  const float *pose_store;           // [n_ids][12]: row-major 3x4
  const unsigned char *has_pose;     // [n_ids]
  const long long *arena_off;        // the arena's offsets: slot s holds arena_off[s + 1] - arena_off[s] points
  u32 n_ids;                         // the ids both stores know: none beyond is eligible
  unsigned char *elig;               // [n_ids]
  double *trans;                     // [3][n_ids]
  // the rows
  u32 *count;                        // [nq + 1] (the last stays 0: its scan is the total)
  const u32 *first;                  // [nq + 1]: the counts' exclusive scan (pass 1)
  int4 *rows;                        // [rows]: query, candidate, frame, map
  double *init;                      // [rows][12]
  // the maps
  u32 *flag;                         // [n_ids + 1]: 1 where the frame is some row's (the last stays 0)
  const u32 *map_of;                 // [n_ids + 1]: the flags' exclusive scan; map_of[n_ids] = the number of maps
  u32 *map_frame;                    // [maps]
  double rr;
  int max_members;
  int *mem_count;                    // [maps]: members, the frame itself included
  long long *mem_pts;                // [maps]: their points
  int *mem_cut;                      // [maps]: SGTD_SL_CUT_*
  u64 *thr_d2;                       // [maps]: the threshold key
  u32 *thr_id;
  // the members (pass 1)
  const int *mem_off;                // [maps + 1]
  int *member, *mem_slot, *mem_map;  // [members]
  u32 *mem_size;                     // [members + 1] (the last stays 0: its scan is mem_pt_off)
  double *mem_pose;                  // [members][12]
};

__global__ __launch_bounds__(SGTD_SL_THREADS) void sl_eligible_kernel(StoredLocalParams P) {
  const u32 i = blockIdx.x * SGTD_SL_THREADS + threadIdx.x;
  if (i > P.n_ids) return;
  P.flag[i] = 0u;
  if (i == P.n_ids) return;
  bool ok = P.slot_of[i] != SGTD_STORE_NONE && P.has_pose[i] != 0;
  const float *m = P.pose_store + (size_t)i * 12;
  for (int k = 0; k < 12; k++) ok = ok && __builtin_isfinite(m[k]);
  P.elig[i] = ok ? 1 : 0;
  for (int r = 0; r < 3; r++) P.trans[(size_t)r * P.n_ids + i] = (double)m[r * 4 + 3];
}

__global__ __launch_bounds__(SGTD_SL_THREADS) void sl_rows_kernel(StoredLocalParams P, int pass) {
  const int lane = threadIdx.x & 63, q = blockIdx.x * (SGTD_SL_THREADS / 64) + (threadIdx.x >> 6);
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
  int frame = 0, kept = 0;
  if (valid && rank < P.max_per_query) {
    frame = P.cand_frame[at];
    if ((u32)frame < P.n_ids) kept = P.elig[(u32)frame];
  }
  if (pass == 0) {
    const unsigned long long m = __ballot(kept);
    if (lane == 0) P.count[q] = (u32)__popcll(m);
    if (kept) P.flag[(u32)frame] = 1u;
    return;
  }
  u32 pos = P.first[q];
  for (int j = 0; j < P.cand_num; j++) {
    const int kj = __shfl(kept, j, 64), rj = __shfl(rank, j, 64);
    if (kj && rj < rank) pos++;
  }
  if (!kept) return;
  P.rows[pos] = make_int4(q, lane, frame, (int)P.map_of[(u32)frame]);
  for (int a = 0; a < 12; a++) P.init[(size_t)pos * 12 + a] = P.pose[at * 12 + a];
}

__global__ __launch_bounds__(SGTD_SL_THREADS) void sl_map_frames_kernel(StoredLocalParams P) {
  const u32 i = blockIdx.x * SGTD_SL_THREADS + threadIdx.x;
  if (i < P.n_ids && P.flag[i]) P.map_frame[P.map_of[i]] = i;
}

// the sum of v over the workgroup's 256 threads, in every thread.  part: 256 long long of LDS.
__device__ __forceinline__ long long sl_block_sum(long long v, long long *part) {
  const int tid = threadIdx.x;
  part[tid] = v;
  __syncthreads();
  for (int w = SGTD_SL_THREADS / 2; w >= 1; w >>= 1) {
    if (tid < w) part[tid] += part[tid + w];
    __syncthreads();
  }
  const long long total = part[0];
  __syncthreads();
  return total;
}

// frame i against the map of frame j at (tx, ty, tz): in reach, and the bits of its d2
__device__ __forceinline__ bool sl_in_reach(const StoredLocalParams &P, u32 i, u32 j, double tx, double ty, double tz, u64 *bits) {
  if (i == j || !P.elig[i]) return false;
  const double dx = P.trans[i] - tx, dy = P.trans[(size_t)P.n_ids + i] - ty, dz = P.trans[(size_t)2 * P.n_ids + i] - tz;
  const double d2 = (dx * dx + dy * dy) + dz * dz;
  *bits = (u64)__double_as_longlong(d2);
  return d2 <= P.rr;
}

__device__ __forceinline__ bool sl_kept(int cut, u64 bits, u32 i, u64 thr_d2, u32 thr_id) {
  return cut == SGTD_SL_CUT_ALL || (cut == SGTD_SL_CUT_KEY && (bits < thr_d2 || (bits == thr_d2 && i <= thr_id)));
}

__global__ __launch_bounds__(SGTD_SL_THREADS) void sl_members_kernel(StoredLocalParams P, int pass) {
  __shared__ long long part[SGTD_SL_THREADS];
  __shared__ u32 hist[256];
  __shared__ u32 sel[2];
  __shared__ u32 wsum[SGTD_SL_THREADS / 64];
  const u32 m = blockIdx.x, tid = threadIdx.x;
  if (m >= P.map_of[P.n_ids]) return;      // (uniform: the grid is the host's upper bound of the maps)
  const u32 j = P.map_frame[m], n = P.n_ids;
  const double tx = P.trans[j], ty = P.trans[(size_t)n + j], tz = P.trans[(size_t)2 * n + j];
  if (pass == 0) {
    long long c = 0;
    for (u32 i = tid; i < n; i += SGTD_SL_THREADS) {
      u64 bits;
      if (sl_in_reach(P, i, j, tx, ty, tz, &bits)) c++;
    }
    const u32 others = (u32)sl_block_sum(c, part);
    int cut = SGTD_SL_CUT_ALL;
    u64 pre_hi = 0ull;
    u32 pre_lo = 0u;
    if (P.max_members > 0 && others > (u32)(P.max_members - 1)) {      // (uniform: every thread holds the same total)
      cut = P.max_members == 1 ? SGTD_SL_CUT_NONE : SGTD_SL_CUT_KEY;
      if (cut == SGTD_SL_CUT_KEY) {
        // the (max_members - 1)-th smallest of the distinct keys (bits of d2, id): digit 11 is the top byte of d2
        u64 mask_hi = 0ull;
        u32 mask_lo = 0u, remaining = (u32)(P.max_members - 1);
        for (int d = 11; d >= 0; d--) {
          hist[tid] = 0u;
          __syncthreads();
          for (u32 i = tid; i < n; i += SGTD_SL_THREADS) {
            u64 bits;
            if (!sl_in_reach(P, i, j, tx, ty, tz, &bits)) continue;
            if (((bits ^ pre_hi) & mask_hi) != 0ull || ((i ^ pre_lo) & mask_lo) != 0u) continue;
            const u32 digit = d >= 4 ? (u32)(bits >> ((d - 4) * 8)) & 0xFFu : (i >> (d * 8)) & 0xFFu;
            atomicAdd(&hist[digit], 1u);
          }
          __syncthreads();
          if (tid == 0) {
            u32 cum = 0u, D = 0u;
            while (D < 255u && cum + hist[D] < remaining) { cum += hist[D]; D++; }
            sel[0] = D; sel[1] = remaining - cum;
          }
          __syncthreads();
          const u32 D = sel[0];
          remaining = sel[1];
          if (d >= 4) { pre_hi |= (u64)D << ((d - 4) * 8); mask_hi |= 0xFFull << ((d - 4) * 8); }
          else { pre_lo |= D << (d * 8); mask_lo |= 0xFFu << (d * 8); }
          __syncthreads();      // (sel and hist are written again in the next pass)
        }
      }
    }
    // the members kept and their points; the frame's own come first
    long long cnt = 0, pts = 0;
    if (tid == 0) { const int s = P.slot_of[j]; cnt = 1; pts = P.arena_off[s + 1] - P.arena_off[s]; }
    for (u32 i = tid; i < n; i += SGTD_SL_THREADS) {
      u64 bits;
      if (!sl_in_reach(P, i, j, tx, ty, tz, &bits) || !sl_kept(cut, bits, i, pre_hi, pre_lo)) continue;
      const int s = P.slot_of[i];
      cnt++;
      pts += P.arena_off[s + 1] - P.arena_off[s];
    }
    cnt = sl_block_sum(cnt, part);
    pts = sl_block_sum(pts, part);
    if (tid == 0) { P.mem_count[m] = (int)cnt; P.mem_pts[m] = pts; P.mem_cut[m] = cut; P.thr_d2[m] = pre_hi; P.thr_id[m] = pre_lo; }
    return;
  }
  // pass 1: the list, ascending id behind the frame itself
  const int cut = P.mem_cut[m];
  const u64 thr_d2 = P.thr_d2[m];
  const u32 thr_id = P.thr_id[m];
  const size_t out = (size_t)P.mem_off[m];
  if (tid == 0) {
    const int s = P.slot_of[j];
    P.member[out] = (int)j; P.mem_slot[out] = s; P.mem_map[out] = (int)m;
    P.mem_size[out] = (u32)(P.arena_off[s + 1] - P.arena_off[s]);
  }
  const u32 lane = tid & 63u, wave = tid >> 6;
  u32 running = 1u;
  for (u32 base = 0; base < n; base += SGTD_SL_THREADS) {      // (uniform bounds: every thread reaches the barriers)
    const u32 i = base + tid;
    u64 bits = 0ull;
    const bool k = i < n && sl_in_reach(P, i, j, tx, ty, tz, &bits) && sl_kept(cut, bits, i, thr_d2, thr_id);
    const unsigned long long b = __ballot(k);
    if (lane == 0) wsum[wave] = (u32)__popcll(b);
    __syncthreads();
    u32 before = (u32)__popcll(b & ((1ull << lane) - 1ull)), total = 0u;
    for (u32 w = 0; w < SGTD_SL_THREADS / 64; w++) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    if (k) {
      const size_t e = out + running + before;
      const int s = P.slot_of[i];
      P.member[e] = (int)i; P.mem_slot[e] = s; P.mem_map[e] = (int)m;
      P.mem_size[e] = (u32)(P.arena_off[s + 1] - P.arena_off[s]);
    }
    running += total;
    __syncthreads();
  }
}

__global__ __launch_bounds__(SGTD_SL_THREADS) void sl_poses_kernel(StoredLocalParams P, int n_members) {
  const int e = blockIdx.x * SGTD_SL_THREADS + threadIdx.x;
  if (e >= n_members) return;
  const int m = P.mem_map[e];
  double *out = P.mem_pose + (size_t)e * 12;
  if (e == P.mem_off[m]) {
    for (int a = 0; a < 12; a++) out[a] = a < 9 && a % 4 == 0 ? 1.0 : 0.0;
    return;
  }
  double Tj[12], Ti[12], inv[12], M[12];
  cons_widen(P.pose_store + (size_t)P.map_frame[m] * 12, Tj);
  cons_widen(P.pose_store + (size_t)P.member[e] * 12, Ti);
  cons_inv(Tj, inv);
  cons_mul(inv, Ti, M);
  for (int a = 0; a < 12; a++) out[a] = M[a];
}
