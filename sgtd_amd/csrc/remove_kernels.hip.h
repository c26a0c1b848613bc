// remove_kernels.hip.h — sgtd_remove_frames: an order-preserving compaction of the table's cold store.
//
//   pass 1   remove_flag_kernel: every entry is tested against the removed set (a bitmap over the table's frame
//            span, in LDS), one 64-bit keep mask per wave and round (ballot) and one survivor count per tile; the
//            tile counts are scanned by device_scan (table_kernels.hip.h) into the tiles' output offsets
//   pass 2   remove_compact_kernel<W>: one field (W 32-bit words per entry) of one tile per workgroup, out of place:
//            16-byte loads into LDS, the survivors packed in LDS in their order (rank: the masks' popcounts and
//            v_mbcnt), 16-byte stores of the packed words.  The host runs it field by field, widest first, and swaps
//            the scratch with the field's buffer (sgtd_accel.hip, remove_frames)
//
// A tile is SGTD_RM_TILE entries: 4 rounds of 256 threads, entry r * 256 + threadIdx.x in round r, so that the masks
// of (round, wave) in that order list the tile's entries in insertion order.
#pragma once
#include "common.hip.h"

#define SGTD_RM_THREADS 256
#define SGTD_RM_ROUNDS 4
#define SGTD_RM_TILE (SGTD_RM_THREADS * SGTD_RM_ROUNDS)
#define SGTD_RM_MASKS (SGTD_RM_TILE / SGTD_WAVE)   // keep masks per tile

__device__ __forceinline__ bool rm_bit(const u32 *bits, u32 d) { return (bits[d >> 5] >> (d & 31u)) & 1u; }

// removed: bit f - lo for every frame id f to remove (span bits); keep_mask[t * SGTD_RM_MASKS + r * 4 + w]: the entries
// of round r, wave w of tile t that stay; tile_count[t]: how many stay in tile t; present: bit f - lo for every frame
// that has an entry (zeroed by the caller).  IN_LDS: the removed set is copied into dynamic LDS first (span / 8 bytes).
template <bool IN_LDS>
__global__ __launch_bounds__(SGTD_RM_THREADS) void remove_flag_kernel(const u32 *frame, long long n, const u32 *removed, u32 lo, u32 span,
                                                                      u64 *keep_mask, u32 *tile_count, u32 *present) {
  extern __shared__ u32 rm_lds[];
  __shared__ u32 wave_cnt[SGTD_RM_THREADS / SGTD_WAVE];
  const u32 *bits = removed;
  if (IN_LDS) {
    for (u32 w = threadIdx.x; w < (span + 31u) >> 5; w += SGTD_RM_THREADS) rm_lds[w] = removed[w];
    __syncthreads();
    bits = rm_lds;
  }
  const int lane = lane_id(), wid = threadIdx.x >> 6;
  const long long n_tiles = (n + SGTD_RM_TILE - 1) / SGTD_RM_TILE;
  for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    u32 cnt = 0;
#pragma unroll
    for (int r = 0; r < SGTD_RM_ROUNDS; r++) {
      const long long i = t * SGTD_RM_TILE + r * SGTD_RM_THREADS + threadIdx.x;
      const bool in = i < n;
      const u32 d = in ? frame[i] - lo : 0u;
      const bool inside = in && d < span;         // (every entry's frame lies in [lo, lo + span): the test only guards the bitmaps)
      const bool gone = inside && rm_bit(bits, d);
      const u64 m = __ballot(in && !gone);
      if (lane == 0) keep_mask[t * SGTD_RM_MASKS + r * (SGTD_RM_THREADS / SGTD_WAVE) + wid] = m;
      cnt += (u32)__popcll(m);
      // the frames that have entries: one atomic per run of equal frame ids in the wave
      const u32 prev = (u32)__shfl_up((int)d, 1);
      if (inside && (lane == 0 || prev != d)) atomicOr(present + (d >> 5), 1u << (d & 31u));
    }
    if (lane == 0) wave_cnt[wid] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      u32 s = 0;
#pragma unroll
      for (int w = 0; w < SGTD_RM_THREADS / SGTD_WAVE; w++) s += wave_cnt[w];
      tile_count[t] = s;
    }
    __syncthreads();
  }
}

// dst[k * W ..] = src[i * W ..] for the k-th surviving entry i, tile by tile (grid: one workgroup per tile).
// tile_off: the exclusive scan of tile_count.  src and dst are distinct buffers of at least 16-byte alignment.
template <int W>
__global__ __launch_bounds__(SGTD_RM_THREADS) void remove_compact_kernel(const u32 *__restrict__ src, u32 *__restrict__ dst, long long n,
                                                                         const u64 *__restrict__ keep_mask, const u32 *__restrict__ tile_off) {
  static_assert((SGTD_RM_TILE * W) % 4 == 0, "a tile's words come in whole 16-byte vectors");
  __shared__ uint4 lds_v[SGTD_RM_TILE * W / 4];
  __shared__ u64 msk[SGTD_RM_MASKS];
  __shared__ u32 before[SGTD_RM_MASKS + 1];
  u32 *lds = reinterpret_cast<u32 *>(lds_v);
  const long long t = blockIdx.x, e0 = t * SGTD_RM_TILE;
  const int ne = (int)min((long long)SGTD_RM_TILE, n - e0);
  const int nw = ne * W, nv = nw >> 2;
  // the tile's words into LDS: 16-byte loads (e0 * W words is a multiple of 4), the last partial vector word by word
  const u32 *s = src + e0 * W;
  for (int v = threadIdx.x; v < nv; v += SGTD_RM_THREADS) lds_v[v] = reinterpret_cast<const uint4 *>(s)[v];
  for (int w = nv * 4 + threadIdx.x; w < nw; w += SGTD_RM_THREADS) lds[w] = s[w];
  if (threadIdx.x < SGTD_RM_MASKS) msk[threadIdx.x] = keep_mask[t * SGTD_RM_MASKS + threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 a = 0;
    for (int k = 0; k < SGTD_RM_MASKS; k++) { before[k] = a; a += (u32)__popcll(msk[k]); }
    before[SGTD_RM_MASKS] = a;
  }
  // every thread takes its entries' words into registers, then the survivors go to their rank in the same LDS
  u32 val[SGTD_RM_ROUNDS][W];
#pragma unroll
  for (int r = 0; r < SGTD_RM_ROUNDS; r++) {
    const int j = r * SGTD_RM_THREADS + threadIdx.x;
#pragma unroll
    for (int k = 0; k < W; k++) val[r][k] = j < ne ? lds[j * W + k] : 0u;
  }
  __syncthreads();
  const int wid = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < SGTD_RM_ROUNDS; r++) {
    const int mi = r * (SGTD_RM_THREADS / SGTD_WAVE) + wid;
    const u64 m = msk[mi];
    if ((m >> lane_id()) & 1ull) {     // (a set bit names an entry inside the table: j < ne)
      const u32 at = before[mi] + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
#pragma unroll
      for (int k = 0; k < W; k++) lds[at * W + k] = val[r][k];
    }
  }
  __syncthreads();
  // the packed words out: scalar stores up to a 16-byte boundary of dst, 16-byte stores, scalar stores for the rest
  const u32 kw = before[SGTD_RM_MASKS] * W;
  const long long d0 = (long long)tile_off[t] * W;
  u32 *d = dst + d0;
  const u32 head = min((u32)((4 - (d0 & 3)) & 3), kw);
  const u32 nv_out = (kw - head) >> 2;
  if (threadIdx.x < head) d[threadIdx.x] = lds[threadIdx.x];
  for (u32 v = threadIdx.x; v < nv_out; v += SGTD_RM_THREADS) {
    const u32 w = head + v * 4;
    reinterpret_cast<uint4 *>(d + head)[v] = make_uint4(lds[w], lds[w + 1], lds[w + 2], lds[w + 3]);
  }
  for (u32 w = head + nv_out * 4 + threadIdx.x; w < kw; w += SGTD_RM_THREADS) d[w] = lds[w];
}
