// scan_kernels.hip.h — sgtd_scan_keypoints: labelled LiDAR scans to keypoints (the rule: include/sgtd_accel.h; the
// reference's producer: src/sgtd/src/get_json.cpp:41-343 over src/sgtd/include/cluster_manager.hpp:139-421).
//
// The whole batch goes through each pass together:
//   point     class, mode vote, r / pitch / azimuth per point; min / max of pitch and r per (scan, class): per tile in LDS
//             on the order-preserving integer image of the double, then one integer atomic per workgroup and value
//   rings     one lane per (scan, class): mode, width, height, the ring bounds
//   keys      (scan, class, pit, polar, azi) — or (scan, class, inst) in instance mode — per point; dropped points sort last
//   sort      table_kernels.hip.h's stable radix sort of (key, point): inside a voxel the points stay in index order
//   voxels    head flags + scan: the occupied voxels, their keys and first positions
//   links     searchKNN's neighbours of every voxel by binary search in the sorted voxel keys
//   components  min-hooking along the links + pointer jumping, in rounds; a round that hooks nothing ends them (the host
//             reads the flags once per group of rounds; later rounds of the group return at once)
//   clusters  count and smallest point index per component (integer atomics: add and min), size filter, a sort of the kept
//             roots by (scan, class, order), the keypoint offsets
//   regroup   a stable sort of the points by keypoint, then the fixed-order sum: a wave per small cluster, a workgroup
//             per large one, both the same 256 accumulators and fold
// Atomics touch integers only, where the result does not depend on arrival order (min, max, add).
#pragma once
#include "common.hip.h"

#define SGTD_SCAN_TILE 1024          // points per workgroup of the per-point passes (256 threads x 4)
#define SGTD_SCAN_NBR 26             // links kept per voxel
#define SGTD_SCAN_CELLS 1024         // ring bounds kept per (scan, class)
#define SGTD_SCAN_BIG 4096           // points from which a cluster's sum takes a workgroup
#define SGTD_SCAN_NONE 0xFFFFFFFFu
#define SGTD_SCAN_PI 3.14159265358979323846

struct ScanCfgDev {
  int node_label[32], min_seg[32];
  int min_inst, n_scans;
  double start_r, delta_r, delta_p, delta_a, min_range, max_range;
};

// order-preserving image of a double in u64 (no NaN reaches it)
__device__ __forceinline__ u64 scan_f64_image(double d) {
  const u64 b = (u64)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double scan_f64_of_image(u64 u) {
  return __longlong_as_double((long long)((u >> 63) ? (u & ~(1ull << 63)) : ~u));
}

// the scan of point i: the last s with pt_off[s] <= i (empty scans own nothing)
__device__ __forceinline__ int scan_of_point(const long long *pt_off, int n_scans, long long i) {
  int lo = 1, hi = n_scans;      // first s in [1, n_scans] with pt_off[s] > i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pt_off[mid] > i) hi = mid; else lo = mid + 1;
  }
  return lo - 1;
}

// mm: (minPitch, maxPitch, minPolar, maxPolar) images per (scan, class), from 0.0, 0.0, 5.0, 5.0 (cluster_manager.hpp:482-485)
__global__ void scan_init_kernel(u64 *mm, u32 *vote, int n_sc) {
  const int sc = blockIdx.x * blockDim.x + threadIdx.x;
  if (sc >= n_sc) return;
  mm[sc * 4 + 0] = scan_f64_image(0.0); mm[sc * 4 + 1] = scan_f64_image(0.0);
  mm[sc * 4 + 2] = scan_f64_image(5.0); mm[sc * 4 + 3] = scan_f64_image(5.0);
  vote[sc] = 0;
}

struct ScanPointParams {
  const float *pts; int stride; const u32 *labels; const long long *pt_off; long long n;
  u32 *sc_of; double *r, *pitch, *azimuth; u64 *mm; u32 *vote;
};

__global__ __launch_bounds__(256) void scan_point_kernel(ScanPointParams P, ScanCfgDev C) {
  __shared__ u64 lmm[32 * 4];
  __shared__ u32 lvote[32];
  const int tid = threadIdx.x;
  const long long base = (long long)blockIdx.x * SGTD_SCAN_TILE;
  const int s0 = scan_of_point(P.pt_off, C.n_scans, base);      // the tile's first scan: its values meet in LDS
  if (tid < 128) lmm[tid] = (tid & 1) ? 0ull : ~0ull;
  if (tid < 32) lvote[tid] = 0;
  __syncthreads();
  for (int k = 0; k < SGTD_SCAN_TILE / 256; k++) {
    const long long i = base + (long long)k * 256 + tid;
    if (i >= P.n) break;
    const int s = scan_of_point(P.pt_off, C.n_scans, i);
    const float *p = P.pts + (size_t)i * P.stride;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    const u32 lab = P.labels[i], sem = lab & 0xFFFFu, inst = lab >> 16;
    const bool kept = sem < 32u && C.node_label[sem & 31u] != 0 && isfinite(x) && isfinite(y) && isfinite(z);
    if (!kept) { P.sc_of[i] = SGTD_SCAN_NONE; continue; }
    const u32 sc = (u32)s * 32u + sem;
    P.sc_of[i] = sc;
    const double rr = norm3(x, y, z);
    double pitch = (asin(z / rr) * 180.0) / SGTD_SCAN_PI;
    if (pitch == 0.0) pitch = 0.0;      // (-0.0 is no new minimum: cluster_manager.hpp:200)
    const double a = atan2(y, x);
    const double azimuth = ((a > 0.0 ? a : a + 2.0 * SGTD_SCAN_PI) * 180.0) / SGTD_SCAN_PI;
    P.r[i] = rr; P.pitch[i] = pitch; P.azimuth[i] = azimuth;
    const u32 v = inst ? 2u : 1u;
    const bool in_range = !(rr >= C.max_range) && !(rr <= C.min_range);
    const u64 ip = scan_f64_image(pitch), ir = scan_f64_image(rr);
    if (s == s0) {
      atomicMax(&lvote[sem], v);
      if (in_range) {
        atomicMin(&lmm[sem * 4 + 0], ip); atomicMax(&lmm[sem * 4 + 1], ip);
        atomicMin(&lmm[sem * 4 + 2], ir); atomicMax(&lmm[sem * 4 + 3], ir);
      }
    } else {
      atomicMax(&P.vote[sc], v);
      if (in_range) {
        atomicMin(&P.mm[(size_t)sc * 4 + 0], ip); atomicMax(&P.mm[(size_t)sc * 4 + 1], ip);
        atomicMin(&P.mm[(size_t)sc * 4 + 2], ir); atomicMax(&P.mm[(size_t)sc * 4 + 3], ir);
      }
    }
  }
  __syncthreads();
  if (base >= P.n) return;
  if (tid < 128) {
    const u64 v = lmm[tid];
    const size_t g = (size_t)s0 * 128 + tid;
    if (tid & 1) { if (v != 0ull) atomicMax(&P.mm[g], v); }
    else if (v != ~0ull) atomicMin(&P.mm[g], v);
  }
  if (tid < 32 && lvote[tid]) atomicMax(&P.vote[(size_t)s0 * 32 + tid], lvote[tid]);
}

// grid: mode, polarNum, width, height; range: minPitch, maxPitch, minPolar, maxPolar; bounds [SGTD_SCAN_CELLS] per (scan, class)
__global__ void scan_rings_kernel(const u64 *mm, const u32 *vote, int n_sc, ScanCfgDev C, int *grid, double *range, double *bounds) {
  const int sc = blockIdx.x * blockDim.x + threadIdx.x;
  if (sc >= n_sc) return;
  const u32 v = vote[sc];
  const int mode = v == 0 ? 0 : (v == 2 ? 1 : 2);
  int polar_num = 0, width = 0, height = 0;
  double r4[4] = {0.0, 0.0, 0.0, 0.0};
  if (mode == 2) {
    for (int j = 0; j < 4; j++) r4[j] = scan_f64_of_image(mm[(size_t)sc * 4 + j]);
    width = (int)(round(360.0 / C.delta_a) + 1.0);
    height = (int)((r4[1] - r4[0]) / C.delta_p);
    double rg = r4[2];
    int step = 1;
    double *b = bounds + (size_t)sc * SGTD_SCAN_CELLS;
    while (rg <= r4[3] && polar_num < SGTD_SCAN_CELLS) {
      rg = rg + (C.start_r - (double)step * C.delta_r);
      b[polar_num] = rg;
      polar_num++; step++;
    }
  }
  grid[sc * 4 + 0] = mode; grid[sc * 4 + 1] = polar_num; grid[sc * 4 + 2] = width; grid[sc * 4 + 3] = height;
  for (int j = 0; j < 4; j++) range[(size_t)sc * 4 + j] = r4[j];
}

// key: scan << 38 | class << 33 | pit << 22 | polar << 11 | azi (voxel mode) or | inst (instance mode); dropped points
// carry the scan n_scans and sort behind everything
__device__ __forceinline__ u64 scan_drop_key(int n_scans) { return (u64)n_scans << 38; }

__global__ __launch_bounds__(256) void scan_keys_kernel(const u32 *sc_of, const u32 *labels, const double *r, const double *pitch, const double *azimuth,
                                                       const int *grid, const double *range, const double *bounds, ScanCfgDev C, long long n,
                                                       u64 *keys, u32 *vals) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  vals[i] = (u32)i;
  const u32 sc = sc_of[i];
  u64 key = scan_drop_key(C.n_scans);
  if (sc != SGTD_SCAN_NONE) {
    const int mode = grid[sc * 4];
    if (mode == 1) key = ((u64)sc << 33) | (u64)(labels[i] >> 16);
    else {
      const double rr = r[i];
      if (!(rr >= C.max_range) && !(rr <= C.min_range)) {
        const int pn = grid[sc * 4 + 1];
        const double *b = bounds + (size_t)sc * SGTD_SCAN_CELLS;
        int lo = 0, hi = pn;      // the first k with rr < b[k] (cluster_manager.hpp:259-264)
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (rr < b[mid]) hi = mid; else lo = mid + 1;
        }
        int polar = lo < pn ? lo : pn - 1;
        int pit = (int)round((pitch[i] - range[(size_t)sc * 4]) / C.delta_p);
        int azi = (int)round(azimuth[i] / C.delta_a);
        polar = min(max(polar, 0), 2047); pit = min(max(pit, 0), 2047); azi = min(max(azi, 0), 2047);
        key = ((u64)sc << 33) | ((u64)pit << 22) | ((u64)polar << 11) | (u64)azi;
      }
    }
  }
  keys[i] = key;
}

// counts[0] = live (not dropped) points; flags [n + 1], the last 0
__global__ void scan_heads_kernel(const u64 *keys, long long n, u64 drop, u32 *flags, u32 *counts) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p > n) return;
  if (p == n) { flags[p] = 0; return; }
  const u64 k = keys[p];
  const bool live = k < drop;
  flags[p] = (live && (p == 0 || keys[p - 1] != k)) ? 1u : 0u;
  if (live && (p == n - 1 || keys[p + 1] >= drop)) counts[0] = (u32)(p + 1);
}

// excl [n + 1]: the exclusive scan of flags (excl[n] = the number of voxels); vstart [voxels + 1]
__global__ void scan_voxels_kernel(const u64 *keys, const u32 *flags, const u32 *excl, long long n, const u32 *counts, u64 *vkey, u32 *vstart) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const u32 live = counts[0];
  if (p == 0) vstart[excl[n]] = live;
  if (p < live && flags[p]) { vkey[excl[p]] = keys[p]; vstart[excl[p]] = (u32)p; }
}

__device__ __forceinline__ u32 scan_find_voxel(const u64 *vkey, u32 n_vox, u64 key) {
  u32 lo = 0, hi = n_vox;
  while (lo < hi) {
    const u32 mid = (lo + hi) >> 1;
    if (vkey[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < n_vox && vkey[lo] == key) ? lo : SGTD_SCAN_NONE;
}

// the occupied voxels of searchKNN's set (cluster_manager.hpp:365-385; 300 read as width - 1) of every voxel-mode voxel
__global__ __launch_bounds__(256) void scan_links_kernel(const u64 *vkey, const u32 *n_vox_p, const int *grid, u32 *nbr, u32 *nbr_cnt, u32 *parent) {
  const u32 n_vox = *n_vox_p;
  const u32 v = blockIdx.x * 256u + threadIdx.x;
  if (v >= n_vox) return;
  parent[v] = v;
  const u64 key = vkey[v];
  const u32 sc = (u32)(key >> 33);
  u32 cnt = 0;
  if (grid[sc * 4] == 2) {
    const int pn = grid[sc * 4 + 1], width = grid[sc * 4 + 2], height = grid[sc * 4 + 3];
    const int pit = (int)((key >> 22) & 2047u), polar = (int)((key >> 11) & 2047u), azi = (int)(key & 2047u);
    for (int z = pit - 1; z <= pit + 1; z++) {
      if (z < 0 || z > height) continue;
      for (int y = polar - 1; y <= polar + 1; y++) {
        if (y < 0 || y > pn) continue;
        for (int x = azi - 1; x <= azi + 1; x++) {
          int ax = x;
          if (ax < 0) ax = width - 1;
          if (ax > width - 1) ax = width - 1;
          const u64 k = ((u64)sc << 33) | ((u64)z << 22) | ((u64)y << 11) | (u64)ax;
          if (k == key) continue;
          const u32 u = scan_find_voxel(vkey, n_vox, k);
          if (u != SGTD_SCAN_NONE && u != v && cnt < SGTD_SCAN_NBR) nbr[(size_t)v * SGTD_SCAN_NBR + cnt++] = u;
        }
      }
    }
  }
  nbr_cnt[v] = cnt;
}

// one round: every link whose ends have different parents hooks the larger parent under the smaller; changed[round] is set
// when any did.  parent[x] <= x always, so the parents form a forest whose roots are their trees' smallest voxels.
__global__ __launch_bounds__(256) void scan_hook_kernel(const u32 *n_vox_p, const u32 *nbr, const u32 *nbr_cnt, u32 *parent, u32 *changed, int round) {
  if (round > 0 && changed[round - 1] == 0) return;
  const u32 v = blockIdx.x * 256u + threadIdx.x;
  if (v >= *n_vox_p) return;
  const u32 cnt = nbr_cnt[v];
  const u32 pv = parent[v];
  bool ch = false;
  for (u32 j = 0; j < cnt; j++) {
    const u32 pu = parent[nbr[(size_t)v * SGTD_SCAN_NBR + j]];
    if (pu != pv) { atomicMin(&parent[max(pu, pv)], min(pu, pv)); ch = true; }
  }
  if (ch) changed[round] = 1;
}
// ... then every voxel points at its root (roots do not change here: a walk ends at one whatever the others have written)
__global__ __launch_bounds__(256) void scan_jump_kernel(const u32 *n_vox_p, u32 *parent, const u32 *changed, int round) {
  if (changed[round] == 0) return;
  const u32 v = blockIdx.x * 256u + threadIdx.x;
  if (v >= *n_vox_p) return;
  u32 p = parent[v], q;
  while ((q = parent[p]) != p) p = q;
  parent[v] = p;
}

// per component (at its root): points and smallest point index (the first point of a voxel is its smallest: the sort is stable)
__global__ void scan_component_kernel(const u32 *n_vox_p, const u32 *parent, const u32 *vstart, const u32 *vals, u32 *ccount, u32 *cmin) {
  const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= *n_vox_p) return;
  const u32 root = parent[v];
  atomicAdd(&ccount[root], vstart[v + 1] - vstart[v]);
  atomicMin(&cmin[root], vals[vstart[v]]);
}

// kept roots: (scan, class) << 32 | order — the smallest point index, or inst in instance mode; everything else sorts last
__global__ void scan_cluster_keys_kernel(const u32 *n_vox_p, const u64 *vkey, const u32 *parent, const u32 *ccount, const u32 *cmin, const int *grid,
                                         ScanCfgDev C, u64 *keys, u32 *vals) {
  const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= *n_vox_p) return;
  u64 k = (u64)C.n_scans << 37;
  if (parent[v] == v) {
    const u64 key = vkey[v];
    const u32 sc = (u32)(key >> 33), cnt = ccount[v];
    const bool inst = grid[sc * 4] == 1;
    const bool keep = inst ? (long long)cnt > (long long)C.min_inst : (long long)cnt >= (long long)C.min_seg[sc & 31u];
    if (keep) k = ((u64)sc << 32) | (u64)(inst ? (u32)(key & 0xFFFFu) : cmin[v]);
  }
  keys[v] = k;
  vals[v] = v;
}

// kp_off[s] = the first sorted cluster of scan s or later (kp_off[n_scans] = the number of keypoints)
__global__ void scan_offsets_kernel(const u64 *keys, const u32 *n_vox_p, int n_scans, long long *kp_off) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > n_scans) return;
  const u64 want = (u64)s << 37;
  u32 lo = 0, hi = *n_vox_p;
  while (lo < hi) {
    const u32 mid = (lo + hi) >> 1;
    if (keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  kp_off[s] = (long long)lo;
}

__global__ void scan_cluster_ids_kernel(const u64 *keys, const u32 *roots, u32 n_kept, const u32 *ccount, ScanCfgDev C, u32 *cl_of_root, u32 *kcount,
                                        int *n_points, u32 *label) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_kept) return;
  const u32 root = roots[j];
  cl_of_root[root] = j;
  kcount[j] = ccount[root];
  n_points[j] = (int)ccount[root];
  label[j] = (u32)C.node_label[(keys[j] >> 32) & 31u];
}

// per sorted position: the point's keypoint (n_kept: none) as the regroup key, and its index within its scan for the caller
__global__ void scan_point_clusters_kernel(const u64 *keys, const u32 *vals, const u32 *flags, const u32 *excl, const u32 *counts, const u32 *parent,
                                           const u32 *cl_of_root, const long long *kp_off, long long n, u32 n_kept, u32 *pkey, u32 *pval, int *cluster) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const u32 i = vals[p];
  u32 kp = SGTD_SCAN_NONE;
  if (p < counts[0]) kp = cl_of_root[parent[excl[p] + flags[p] - 1u]];
  pkey[i] = kp == SGTD_SCAN_NONE ? n_kept : kp;
  pval[i] = i;
  cluster[i] = kp == SGTD_SCAN_NONE ? -1 : (int)((long long)kp - kp_off[keys[p] >> 38]);
}

// The centre of every cluster: (float)(SUM / n), SUM over 256 accumulators (rank k of the cluster's points, in ascending
// point index, goes to accumulator k mod 256) folded acc[l] += acc[l + w], w = 128 .. 1.  A wave per cluster below
// SGTD_SCAN_BIG points (lane l holds accumulators l, l + 64, l + 128, l + 192), a workgroup per cluster from there on (one
// accumulator per thread): the same additions in the same order.
__global__ __launch_bounds__(256) void scan_sum_wave_kernel(const float *pts, int stride, const u32 *order, const u32 *cstart, const u32 *kcount, u32 n_kept,
                                                           float *xyz) {
  const u32 c = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (c >= n_kept) return;
  const u32 n = kcount[c];
  if (n >= SGTD_SCAN_BIG) return;
  const u32 lane = lane_id();
  const u32 *o = order + cstart[c];
  double a[4][3] = {};
  for (u32 k0 = 0; k0 < n; k0 += 256) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const u32 k = k0 + j * 64 + lane;
      if (k < n) {
        const float *p = pts + (size_t)o[k] * stride;
        a[j][0] += (double)p[0]; a[j][1] += (double)p[1]; a[j][2] += (double)p[2];
      }
    }
  }
#pragma unroll
  for (int d = 0; d < 3; d++) {
    a[0][d] += a[2][d]; a[1][d] += a[3][d];      // w = 128
    a[0][d] += a[1][d];                          // w = 64
    double s = a[0][d];
    for (int w = 32; w >= 1; w >>= 1) {
      const double t = __shfl_down(s, w, 64);
      if ((int)lane < w) s += t;
    }
    if (lane == 0) xyz[(size_t)c * 3 + d] = (float)(s / (double)n);
  }
}

__global__ __launch_bounds__(256) void scan_sum_block_kernel(const float *pts, int stride, const u32 *order, const u32 *cstart, const u32 *kcount, float *xyz) {
  __shared__ double acc[3][256];
  const u32 c = blockIdx.x, n = kcount[c];
  if (n < SGTD_SCAN_BIG) return;
  const u32 tid = threadIdx.x;
  const u32 *o = order + cstart[c];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (u32 k = tid; k < n; k += 256) {
    const float *p = pts + (size_t)o[k] * stride;
    a0 += (double)p[0]; a1 += (double)p[1]; a2 += (double)p[2];
  }
  acc[0][tid] = a0; acc[1][tid] = a1; acc[2][tid] = a2;
  __syncthreads();
  for (u32 w = 128; w >= 1; w >>= 1) {
    if (tid < w) { acc[0][tid] += acc[0][tid + w]; acc[1][tid] += acc[1][tid + w]; acc[2][tid] += acc[2][tid + w]; }
    __syncthreads();
  }
  if (tid < 3) xyz[(size_t)c * 3 + tid] = (float)(acc[tid][0] / (double)n);
}
