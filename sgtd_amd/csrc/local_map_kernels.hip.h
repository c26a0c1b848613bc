// local_map_kernels.hip.h — sgtd_local_map_keypoints: posed, labelled scans to the keypoints of local maps (the rule:
// include/sgtd_accel.h; the reference's producer: src/sgtd/src/local_map.cpp:213-482).
//
//   members   one workgroup per anchor: the squared distance of every scan's translation to the anchor's in LDS, the
//             max_members cut by (d2, i) rank, then the member list in ascending scan index by a prefix sum over the
//             flags (never by arrival) and the merged size.  Run twice: counts first, the lists once the host has
//             turned the counts into offsets.
//   segments  per pass, one lane per (anchor, member): source offset, point count and M = mul(inv(T_j), T_i) in f64
//   gather    per pass: the merged cloud, xyz f32 at stride 3 and the labels.  A workgroup finds the segment its tile of
//             SGTD_SCAN_TILE merged points starts in once, then walks the segments; lanes read consecutive source points
//             (one 16-byte load a lane at stride 4); the anchor's own segment is a plain copy.
// The merged cloud then goes through scan_kernels.hip.h unchanged, one "scan" per anchor.  No atomics here.
#pragma once
#include "common.hip.h"
#include "consistency_kernels.hip.h"
#include "scan_kernels.hip.h"

#define SGTD_LM_THREADS 256
#define SGTD_LM_MAX_SCANS 4096      // == SGTD_SCAN_MAX_SCANS: what a workgroup's LDS holds
#define SGTD_LM_PER (SGTD_LM_MAX_SCANS / SGTD_LM_THREADS)

struct __attribute__((aligned(16))) LmSeg {
  long long src;      // first source point
  int plain, pad;     // the anchor's own points: copied as they are
  double M[12];       // R row-major, then t (the layout of cons_mul)
};

// exclusive prefix of v over the workgroup's 256 threads; *total = the sum.  part: 256 u32 of LDS.
__device__ __forceinline__ u32 lm_block_excl(u32 v, u32 *part, u32 *total) {
  const int tid = threadIdx.x;
  part[tid] = v;
  __syncthreads();
  for (int d = 1; d < SGTD_LM_THREADS; d <<= 1) {
    const u32 add = tid >= d ? part[tid - d] : 0u;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  const u32 incl = part[tid];
  *total = part[SGTD_LM_THREADS - 1];
  __syncthreads();
  return incl - v;
}

// mem_off == nullptr: only count[a] (members, the anchor included) and merged[a] (their points) are written
__global__ __launch_bounds__(SGTD_LM_THREADS) void lm_members_kernel(const float *pose12, const long long *pt_off, int n_scans, const int *anchors,
                                                                     double rr, int max_members, const long long *mem_off, int *member, int *count,
                                                                     long long *merged) {
  __shared__ double d2s[SGTD_LM_MAX_SCANS];
  __shared__ unsigned char in[SGTD_LM_MAX_SCANS], keep[SGTD_LM_MAX_SCANS];
  __shared__ u32 part[SGTD_LM_THREADS];
  __shared__ long long lsum[SGTD_LM_THREADS];
  const int a = blockIdx.x, tid = threadIdx.x;
  const int j = anchors[a];
  const double tx = (double)pose12[(size_t)j * 12 + 3], ty = (double)pose12[(size_t)j * 12 + 7], tz = (double)pose12[(size_t)j * 12 + 11];
  for (int i = tid; i < SGTD_LM_MAX_SCANS; i += SGTD_LM_THREADS) {
    double d2 = 0.0;
    bool m = false;
    if (i < n_scans && i != j) {
      const double dx = (double)pose12[(size_t)i * 12 + 3] - tx, dy = (double)pose12[(size_t)i * 12 + 7] - ty,
                   dz = (double)pose12[(size_t)i * 12 + 11] - tz;
      d2 = (dx * dx + dy * dy) + dz * dz;
      m = d2 <= rr;      // (NaN: not a member)
    }
    d2s[i] = d2;
    in[i] = m ? 1 : 0;
    keep[i] = m ? 1 : 0;
  }
  __syncthreads();
  if (max_members > 0) {
    u32 c = 0, others;
    for (int i = tid; i < n_scans; i += SGTD_LM_THREADS) c += in[i];
    lm_block_excl(c, part, &others);
    if (others > (u32)(max_members - 1)) {      // (uniform: every thread holds the same total)
      for (int i = tid; i < n_scans; i += SGTD_LM_THREADS) {
        if (!in[i]) continue;
        const double d = d2s[i];
        u32 rank = 0;
        for (int k = 0; k < n_scans; k++)
          if (in[k] && (d2s[k] < d || (d2s[k] == d && k < i))) rank++;
        keep[i] = rank < (u32)(max_members - 1) ? 1 : 0;
      }
      __syncthreads();
    }
  }
  // thread t owns the scans [t * PER, (t + 1) * PER): ascending order falls out of the prefix sum
  u32 c = 0, total;
  long long pts = tid == 0 ? pt_off[j + 1] - pt_off[j] : 0;
  for (int i = tid * SGTD_LM_PER; i < (tid + 1) * SGTD_LM_PER; i++)
    if (keep[i]) { c++; pts += pt_off[i + 1] - pt_off[i]; }
  const u32 excl = lm_block_excl(c, part, &total);
  lsum[tid] = pts;
  __syncthreads();
  for (int w = SGTD_LM_THREADS / 2; w >= 1; w >>= 1) {
    if (tid < w) lsum[tid] += lsum[tid + w];
    __syncthreads();
  }
  if (tid == 0) { count[a] = (int)total + 1; merged[a] = lsum[0]; }
  if (!mem_off) return;
  int *out = member + mem_off[a];
  if (tid == 0) out[0] = j;
  u32 at = 1 + excl;
  for (int i = tid * SGTD_LM_PER; i < (tid + 1) * SGTD_LM_PER; i++)
    if (keep[i]) out[at++] = i;
}

__device__ __forceinline__ void lm_pose(const float *p, double *X) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) X[r * 3 + c] = (double)p[r * 4 + c];
    X[9 + r] = (double)p[r * 4 + 3];
  }
}

// the pass's segments: the members mem_off[a0] .. mem_off[a0 + n_pass) of the call, n_seg of them; cnt gets n_seg + 1
// entries (the last 0) for the scan that turns them into the segments' first merged points
__global__ void lm_segments_kernel(const float *pose12, const long long *pt_off, const int *anchors, const long long *mem_off, const int *member,
                                   int a0, int n_pass, int n_seg, LmSeg *seg, u32 *cnt) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > n_seg) return;
  if (k == n_seg) { cnt[k] = 0; return; }
  const long long g = mem_off[a0] + k;
  int lo = a0 + 1, hi = a0 + n_pass;      // first a in (a0, a0 + n_pass] with mem_off[a] > g
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (mem_off[mid] > g) hi = mid; else lo = mid + 1;
  }
  const int a = lo - 1, j = anchors[a], i = member[g];
  LmSeg s;
  s.src = pt_off[i];
  s.plain = g == mem_off[a] ? 1 : 0;
  s.pad = 0;
  for (int q = 0; q < 12; q++) s.M[q] = 0.0;
  if (!s.plain) {
    double Tj[12], Ti[12], inv[12];
    lm_pose(pose12 + (size_t)j * 12, Tj);
    lm_pose(pose12 + (size_t)i * 12, Ti);
    cons_inv(Tj, inv);
    cons_mul(inv, Ti, s.M);
  }
  seg[k] = s;
  cnt[k] = (u32)(pt_off[i + 1] - pt_off[i]);
}

// start: n_seg + 1 first merged points of the segments (start[n_seg] = P, the pass's merged size)
template <int STRIDE, bool VEC>
__global__ __launch_bounds__(SGTD_LM_THREADS) void lm_gather_kernel(const float *pts, const u32 *labels, const LmSeg *seg, const u32 *start, int n_seg,
                                                                    u32 P, float *out_xyz, u32 *out_lab) {
  __shared__ int s_first;
  const int tid = threadIdx.x;
  const u32 base = blockIdx.x * (u32)SGTD_SCAN_TILE;
  if (base >= P) return;
  const u32 end = min(base + (u32)SGTD_SCAN_TILE, P);
  if (tid == 0) {
    int lo = 0, hi = n_seg - 1;      // the first k with start[k + 1] > base (one exists: base < P = start[n_seg])
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (start[mid + 1] > base) hi = mid; else lo = mid + 1;
    }
    s_first = lo;
  }
  __syncthreads();
  for (int k = __builtin_amdgcn_readfirstlane(s_first); k < n_seg; k++) {
    const u32 s = start[k];
    if (s >= end) break;
    const u32 lo = max(s, base), hi = min(start[k + 1], end);
    if (lo >= hi) continue;      // an empty scan
    const LmSeg *sg = seg + k;
    const long long src0 = sg->src - (long long)s;
    const bool plain = sg->plain != 0;
    double M[12];
    for (int q = 0; q < 12; q++) M[q] = sg->M[q];
    for (u32 i = lo + tid; i < hi; i += SGTD_LM_THREADS) {
      const size_t src = (size_t)(src0 + (long long)i);
      float x, y, z;
      if (VEC) {
        const float4 v = *reinterpret_cast<const float4 *>(pts + src * 4);
        x = v.x; y = v.y; z = v.z;
      } else {
        const float *p = pts + src * STRIDE;
        x = p[0]; y = p[1]; z = p[2];
      }
      if (!plain) {
        const double dx = (double)x, dy = (double)y, dz = (double)z;
        x = (float)(((M[0] * dx + M[1] * dy) + M[2] * dz) + M[9]);
        y = (float)(((M[3] * dx + M[4] * dy) + M[5] * dz) + M[10]);
        z = (float)(((M[6] * dx + M[7] * dy) + M[8] * dz) + M[11]);
      }
      float *o = out_xyz + (size_t)i * 3;
      o[0] = x; o[1] = y; o[2] = z;
      out_lab[i] = labels[src];
    }
  }
}
