// overlap_kernels.hip.h — keypoint overlap of every verified candidate (sgtd_overlap; the rule is stated in
// include/sgtd_accel.h, DESIGN.md has the LDS budget and the test count).
//
// Under a candidate's relative pose, how many of the query's semantic keypoints land within `radius` of a keypoint of
// the same label of the candidate's frame, and how many of the frame's keypoints are landed on?  The frame's keypoints
// come from the handle's keypoint store (sgtd_set_frame_keypoints): 16 B each (x, y, z as f32, the label), one 8-byte
// word per frame id (first keypoint << 16 | count; all ones: nothing stored).  One 256-thread workgroup per
// (query, candidate):
//   thread l owns the query keypoints i = l, l + 256, ... (the summation order of the rule: accumulator l); per round
//   of 256 it transforms its keypoint once (f64), then walks the frame's keypoints in LDS — tiles of
//   SGTD_OVERLAP_TILE, staged by the whole workgroup; every lane reads the same address, a broadcast — the label gates
//   the f64 squared distance; it keeps the running minimum and marks the frame keypoints it reaches with a plain
//   byte store of 1 into the frame's hit bytes (LDS, one per frame keypoint, all writers write the same value).
//   A frame of one tile is staged once; a longer one is staged again by every round of query keypoints.
// f64 vector arithmetic runs at the f32 rate on this chip, so there is no f32 pre-test: the walk is the rule itself.
// The sum of the hits' minima: per-thread accumulators, then refine_tree (two levels through LDS, six by wave
// shuffles).  No atomics.  Arithmetic: f64, -ffp-contract=off.
#pragma once
#include "common.hip.h"
#include "table_kernels.hip.h"
#include "refine_kernels.hip.h"

#define SGTD_OVERLAP_THREADS 256
#define SGTD_OVERLAP_TILE 1024       // frame keypoints staged at once: 16 KB
#define SGTD_OVERLAP_HEAD 1152       // bytes ahead of the tile: refine_tree's [128] + [8] doubles, the scan's words
#define SGTD_OVERLAP_NONE 0xFFFFFFFFFFFFFFFFull

struct OverlapParams {
  // the batch's candidates and their verification results
  const int *n_cand;
  const int *cand_frame;
  int cand_num;
  const double *score;
  const double *pose;                // sgtd_verify's, or sgtd_refine_poses'
  // the query keypoints: xyz[3 i], label[i], query q's are q_off[q] .. q_off[q + 1]
  const float *q_xyz;
  const u32 *q_label;
  const long long *q_off;
  // the keypoint store's device copy
  const uint4 *kp;
  const u64 *f_word;                 // [n_ids]
  u32 n_ids;
  u32 hit_off;                       // byte offset of the hit bytes in dynamic LDS (behind the tile)
  double rr;
  const u32 *order;                  // or NULL: the (query, candidate) indices in dispatch order (verify_order_keys_kernel)
  u32 n_blocks;
  // results, [nq * cand_num] each
  int4 *cnt;                         // n_query_kp, n_frame_kp, n_hit_query, n_hit_frame
  double2 *val;                      // overlap, rms
};

// dynamic LDS of a launch over a store whose longest frame has max_kp keypoints
inline size_t overlap_tile_slots(int max_kp) { return (size_t)std::min(std::max(max_kp, 1), SGTD_OVERLAP_TILE); }
inline size_t overlap_hit_off(int max_kp) { return (size_t)SGTD_OVERLAP_HEAD + overlap_tile_slots(max_kp) * sizeof(uint4); }
inline size_t overlap_lds_bytes(int max_kp) { return overlap_hit_off(max_kp) + (((size_t)std::max(max_kp, 1) + 15) & ~(size_t)15); }

// The walk of one round of 256 query keypoints over a frame's keypoints, tile by tile: this thread's keypoint (x, lab;
// `active`) against every frame keypoint.  m (+inf at the call) becomes the minimum of r2 over the keypoints of the
// label, the frame keypoints within reach get their hit byte.  ARG (sgtd_align_keypoints): bj (-1 at the call) becomes
// the lowest j that attains the minimum, -1 when no keypoint of the label has a non-NaN r2.  `stage` (uniform): stage
// the first tile too — off when a frame of one tile is still in `tile` from the round before.
template <bool ARG>
__device__ __forceinline__ void overlap_walk(const uint4 *kp, int nf, bool stage, uint4 *tile, unsigned char *hit, bool active,
                                             const double (&x)[3], u32 lab, double rr, double &m, int &bj) {
  const int tid = threadIdx.x;
  for (int t0 = 0; t0 < nf; t0 += SGTD_OVERLAP_TILE) {
    const int nt = min(SGTD_OVERLAP_TILE, nf - t0);
    if (stage || t0 > 0) {
      __syncthreads();                                     // the last tile's readers are done; the hit bytes are cleared
      for (int j = tid; j < nt; j += SGTD_OVERLAP_THREADS) tile[j] = kp[t0 + j];
      __syncthreads();
    }
    if (active) {
      // the label gates both comparisons; the distance itself is computed for every lane (the wave pays for it as
      // soon as one lane's label matches, and without a branch around it four keypoints' LDS reads are in flight)
      auto test = [&](const uint4 k, int j) {
        const double e0 = x[0] - (double)__uint_as_float(k.x), e1 = x[1] - (double)__uint_as_float(k.y),
                     e2 = x[2] - (double)__uint_as_float(k.z);
        const double r2 = (e0 * e0 + e1 * e1) + e2 * e2;
        const bool same = k.w == lab;
        if (ARG) {
          if (same && (r2 < m || (bj < 0 && r2 <= m))) { m = r2; bj = t0 + j; }      // (the first one, +inf included)
        } else {
          if (same && r2 < m) m = r2;
        }
        if (same && r2 <= rr) hit[t0 + j] = 1;
      };
      int j = 0;
      for (; j + 4 <= nt; j += 4) {
        const uint4 k0 = tile[j], k1 = tile[j + 1], k2 = tile[j + 2], k3 = tile[j + 3];
        test(k0, j); test(k1, j + 1); test(k2, j + 2); test(k3, j + 3);
      }
      for (; j < nt; j++) test(tile[j], j);
    }
  }
}

__global__ __launch_bounds__(SGTD_OVERLAP_THREADS) void overlap_kernel(OverlapParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char overlap_smem[];
  double *red = reinterpret_cast<double *>(overlap_smem);                       // [128]
  double *bc = red + 128;                                                       // [8]
  u32 *scan = reinterpret_cast<u32 *>(bc + 8);                                  // [<= 8]
  uint4 *tile = reinterpret_cast<uint4 *>(overlap_smem + SGTD_OVERLAP_HEAD);
  unsigned char *hit = overlap_smem + P.hit_off;
  const int tid = threadIdx.x;
  const u32 blk = P.order ? P.order[blockIdx.x] : blockIdx.x;
  if (blk >= P.n_blocks) return;
  const int q = (int)(blk / (u32)P.cand_num), c = (int)(blk % (u32)P.cand_num);
  const double nan = __builtin_nan("");
  if (c >= P.n_cand[q] || !(P.score[blk] >= 0.0)) {        // no verification result
    if (tid == 0) { P.cnt[blk] = make_int4(-1, -1, -1, -1); P.val[blk] = make_double2(nan, nan); }
    return;
  }
  const long long q0 = P.q_off[q];
  const int nqk = (int)(P.q_off[q + 1] - q0);
  const u32 frame = (u32)P.cand_frame[blk];
  const u64 word = frame < P.n_ids ? P.f_word[frame] : SGTD_OVERLAP_NONE;
  if (word == SGTD_OVERLAP_NONE) {                         // the frame has no stored keypoints
    if (tid == 0) { P.cnt[blk] = make_int4(nqk, -1, 0, 0); P.val[blk] = make_double2(nan, nan); }
    return;
  }
  const int nf = (int)(word & 0xFFFFull);
  const uint4 *kp = P.kp + (size_t)(word >> 16);
  double Rt[12];
#pragma unroll
  for (int k = 0; k < 12; k++) Rt[k] = P.pose[(size_t)blk * 12 + k];
  const double rr = P.rr;
  for (int j = tid; j < nf; j += SGTD_OVERLAP_THREADS) hit[j] = 0;

  double acc = 0.0;                  // accumulator `tid` of SUM(m_i over hit i)
  u32 n_hit = 0;
  const int rounds = (nqk + SGTD_OVERLAP_THREADS - 1) / SGTD_OVERLAP_THREADS;
  for (int r = 0; r < rounds; r++) {
    const int i = r * SGTD_OVERLAP_THREADS + tid;
    const bool active = i < nqk;
    double x[3] = {0.0, 0.0, 0.0};
    u32 lab = 0;
    if (active) {
      const float *pf = P.q_xyz + (size_t)(q0 + i) * 3;
      const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
      lab = P.q_label[(size_t)(q0 + i)];
#pragma unroll
      for (int a = 0; a < 3; a++) x[a] = ((Rt[a * 3] * p[0] + Rt[a * 3 + 1] * p[1]) + Rt[a * 3 + 2] * p[2]) + Rt[9 + a];
    }
    double m = __builtin_inf();
    int bj = -1;
    overlap_walk<false>(kp, nf, nf > SGTD_OVERLAP_TILE || r == 0, tile, hit, active, x, lab, rr, m, bj);   // (a frame of one tile is staged once)
    if (active && m <= rr) { acc += m; n_hit++; }
  }
  __syncthreads();
  u32 f_hit = 0;
  for (int j = tid; j < nf; j += SGTD_OVERLAP_THREADS) f_hit += hit[j];
  u32 n_hit_q, n_hit_f;
  (void)block_excl_scan(n_hit, scan, n_hit_q);
  (void)block_excl_scan(f_hit, scan, n_hit_f);
  double s[1] = {acc};
  refine_tree<1>(s, red, bc);
  if (tid == 0) {
    P.cnt[blk] = make_int4(nqk, nf, (int)n_hit_q, (int)n_hit_f);
    P.val[blk] = make_double2(nqk > 0 ? (double)n_hit_q / (double)nqk : nan, n_hit_q > 0 ? sqrt(s[0] / (double)n_hit_q) : nan);
  }
}
