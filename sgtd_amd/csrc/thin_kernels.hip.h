// thin_kernels.hip.h — sgtd_thin_clouds: voxel-grid thinning of a batch of raw clouds (the rule: include/sgtd_accel.h;
// the reference's step: pcl's ApproximateVoxelGrid in semantic_graph_localization.cpp:357-358, 660; the host form:
// ingest.voxel_downsample).
//
// The whole batch goes through each pass together:
//   keys      per point: its cloud (dropped points carry the cloud n_clouds), its cell key cx << 42 | cy << 21 | cz
//             with every coordinate offset by SGTD_THIN_MAX_CELL to unsigned 21 bits; the drops are counted per cloud
//             (integer add)
//   sort      table_kernels.hip.h's stable radix sort of (key, point), twice: by the 63 bits of the cell key, then by the
//             cloud of the point each position holds.  16 cloud bits and 63 cell bits do not fit one u64; two stable
//             passes order by (cloud, cell), the dropped points last, and leave the points of a cell in index order
//   heads     a position starts a cell when its (cloud, cell) differs from its predecessor's: a flag per position, and a
//             flag at the point that position holds — the cell's smallest point index
//   scans     the exclusive scan of the position flags numbers the cells in key order and gives their first positions;
//             the scan of the point flags gives every cell its place by smallest point index, and — the clouds lie back
//             to back — out_off[s] is that scan at pt_off[s]
//   sums      a lane per cell walks its run: one sequential f64 sum per column in ascending point index
// No floating-point atomic anywhere; the only integer atomic is the add of the drop counts.
#pragma once
#include "common.hip.h"

#define SGTD_THIN_CELL_BITS 21
#define SGTD_THIN_DROP_KEY 0x7FFFFFFFFFFFFFFFull      // (the cell key of a dropped point; the corner cell has it too: the cloud tells them apart)

// the cloud of point i: the last s with pt_off[s] <= i (empty clouds own nothing)
__device__ __forceinline__ int thin_cloud_of_point(const long long *pt_off, int n_clouds, long long i) {
  int lo = 1, hi = n_clouds;      // first s in [1, n_clouds] with pt_off[s] > i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pt_off[mid] > i) hi = mid; else lo = mid + 1;
  }
  return lo - 1;
}

// key_pt / cl_pt: per point, kept for the heads; keys / vals: the sort's input; dropped [n_clouds * 2]: non-finite, out of range
__global__ __launch_bounds__(256) void thin_keys_kernel(const float *pts, int stride, const long long *pt_off, int n_clouds, long long n, double leaf,
                                                       u64 *key_pt, u32 *cl_pt, u64 *keys, u32 *vals, int *dropped) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = thin_cloud_of_point(pt_off, n_clouds, i);
  const float *p = pts + (size_t)i * stride;
  const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
  u64 key = SGTD_THIN_DROP_KEY;
  u32 cl = (u32)n_clouds;
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) atomicAdd(&dropped[s * 2], 1);
  else {
    const double lim = (double)(1 << 20);
    const double cx = floor(x / leaf), cy = floor(y / leaf), cz = floor(z / leaf);
    const bool in = cx >= -lim && cx < lim && cy >= -lim && cy < lim && cz >= -lim && cz < lim;
    if (!in) atomicAdd(&dropped[s * 2 + 1], 1);
    else {
      const u64 ux = (u64)((long long)cx + (1 << 20)), uy = (u64)((long long)cy + (1 << 20)), uz = (u64)((long long)cz + (1 << 20));
      key = (ux << (2 * SGTD_THIN_CELL_BITS)) | (uy << SGTD_THIN_CELL_BITS) | uz;
      cl = (u32)s;
    }
  }
  key_pt[i] = key; cl_pt[i] = cl;
  keys[i] = key; vals[i] = (u32)i;
}

// the second sort's keys: the cloud of the point every position holds
__global__ __launch_bounds__(256) void thin_cloud_keys_kernel(const u32 *vals, const u32 *cl_pt, long long n, u32 *ckeys) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p < n) ckeys[p] = cl_pt[vals[p]];
}

// flags [n + 1] per position and first [n + 1] per point, the last of each 0; counts[0] = the live (not dropped) points.
// first: zeroed on the stream by the caller.
__global__ __launch_bounds__(256) void thin_heads_kernel(const u32 *vals, const u64 *key_pt, const u32 *cl_pt, long long n, u32 n_clouds, u32 *flags,
                                                        u32 *first, u32 *counts) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p > n) return;
  if (p == n) { flags[p] = 0; return; }
  const u32 i = vals[p], cl = cl_pt[i];
  const bool live = cl < n_clouds;
  bool head = false;
  if (live) {
    head = p == 0;
    if (!head) {
      const u32 j = vals[p - 1];
      head = cl_pt[j] != cl || key_pt[j] != key_pt[i];
    }
    if (p == n - 1 || cl_pt[vals[p + 1]] >= n_clouds) counts[0] = (u32)(p + 1);
  }
  flags[p] = head ? 1u : 0u;
  if (head) first[i] = 1u;
}

// cstart [cells + 1]: the cells' first positions in key order, the live count behind them
__global__ __launch_bounds__(256) void thin_cells_kernel(const u32 *flags, const u32 *excl, long long n, const u32 *counts, u32 *cstart) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  if (p == 0) cstart[excl[n]] = counts[0];
  if (flags[p]) cstart[excl[p]] = (u32)p;
}

// out_off[s] = the cells whose smallest point lies before cloud s's first (out_off[n_clouds]: all of them)
__global__ void thin_offsets_kernel(const u32 *first_excl, const long long *pt_off, int n_clouds, long long *out_off) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s <= n_clouds) out_off[s] = (long long)first_excl[pt_off[s]];
}

// A lane per cell: column a of its output point = (float)(s_a / (double)count), s_a from +0.0 adding the cell's points in
// ascending point index (the order of its run: the sorts are stable).  The output row is the cell's place by smallest
// point index.  A cell that holds a whole cloud is walked by one lane: correct, and as slow as that is.
template <int STRIDE>
__global__ __launch_bounds__(256) void thin_sum_kernel(const float *pts, const u32 *vals, const u32 *cstart, const u32 *first_excl, const u32 *n_cells_p,
                                                      float *out) {
  const u32 c = blockIdx.x * 256u + threadIdx.x;
  if (c >= *n_cells_p) return;
  const u32 a = cstart[c], b = cstart[c + 1];
  double s[STRIDE];
#pragma unroll
  for (int k = 0; k < STRIDE; k++) s[k] = 0.0;
  for (u32 p = a; p < b; p++) {
    const float *q = pts + (size_t)vals[p] * STRIDE;
#pragma unroll
    for (int k = 0; k < STRIDE; k++) s[k] += (double)q[k];
  }
  const double cnt = (double)(b - a);
  float *o = out + (size_t)first_excl[vals[a]] * STRIDE;
#pragma unroll
  for (int k = 0; k < STRIDE; k++) o[k] = (float)(s[k] / cnt);
}
