// order_kernels.hip.h — the batch path's ordering chain (32-bit home keys) in eight launches behind the fill of the batch's counters:
//
//   order_begin_kernel     q_M and q_P cleared, the queries' prefix, n_valid                   (one workgroup)
//   (one fill)             the work block: tickets, digit histograms, tile state words
//   home_keys_hist_kernel  keys and values, the histogram of every 8-bit digit of every key, pos_of_slot = SGTD_NO_PASS
//   order_sort_pass_kernel one stable radix pass per digit: ticket, rank in LDS, decoupled look-back, runs written
//                          from the LDS image (one kernel where radix_hist + three scan launches + radix_scatter ran)
//   order_groups_kernel    gid, group_first, n_groups and pos_of_slot from ONE read of the sorted keys
//
// What the chain hands on is, value for value, what the launch train (sgtd_accel.hip order_descriptors) hands on: the
// sort is stable, so there is one right answer.
//
// Tiles and look-back.  A workgroup takes its tile number from a ticket when it starts, so a tile only ever waits for
// tiles whose workgroups are already running.  What a tile tells its successors is ONE word per digit (sort) or per tile
// (groups): status in the top two bits, the payload below, written and polled with relaxed agent-scope atomics — the
// payload is in the flag word, so no fence is needed (the per-XCD L2s are not coherent: a plain flag behind a fence is
// not seen).  The look-back is BOUNDED: after `max_polls` loads of state words a workgroup raises CTR_ORDER_GIVEUP in
// the batch's counters and exits; every later kernel of the chain returns at once when it finds the word set, and
// order_groups_kernel leaves the batch empty (n_valid = 0) with the work-buffer flag raised, so that everything behind
// the chain runs over nothing and sgtd_sync re-runs the batch with the launch train.  max_polls = 0: every tile but
// the first gives up (the tests' deterministic fallback).
#pragma once
#include "probe_kernels.hip.h"

#define SGTD_OS_THREADS 512
#define SGTD_OS_ITEMS 16
#define SGTD_OS_TILE (SGTD_OS_THREADS * SGTD_OS_ITEMS)        // keys of a sort tile: 8192 (64 KB of LDS image, two workgroups per CU)
#define SGTD_GI_THREADS 256
#define SGTD_GI_ITEMS 16
#define SGTD_GI_TILE (SGTD_GI_THREADS * SGTD_GI_ITEMS)        // sorted positions of a group-index tile: 4096
#define SGTD_ORDER_WINDOW 8                                     // state words a look-back loads at once
#define SGTD_ORDER_POLLS_DEFAULT (1u << 20)                     // a tile's turn comes after microseconds; this is a fraction of a second
#define SGTD_ORDER_MAX_KEYS (1ll << 30)                         // a state word counts in 30 bits

// the work block, in 32-bit words: tickets (one per sort pass, one for the group index) | four 256-bin digit histograms |
// the sort passes' state words, [pass][tile][digit] | the group index's state words (64-bit), [tile]
enum { OW_TICKET = 0, OW_GROUP_TICKET = 4, OW_HIST = 64, OW_STATE = OW_HIST + 4 * 256 };
__host__ __device__ __forceinline__ size_t order_sort_state_at(int pass, u32 tiles_cap) { return (size_t)OW_STATE + (size_t)pass * tiles_cap * 256; }
__host__ __device__ __forceinline__ size_t order_group_state_at(int passes, u32 tiles_cap) { return (order_sort_state_at(passes, tiles_cap) + 1) & ~(size_t)1; }
__host__ __device__ __forceinline__ size_t order_work_words(int passes, u32 tiles_cap, u32 gtiles_cap) { return order_group_state_at(passes, tiles_cap) + (size_t)gtiles_cap * 2; }

#define SGTD_ST_AGG 1u           // the tile's own count
#define SGTD_ST_INCL 2u          // the count of the tile and of every tile before it
#define SGTD_ST_MASK 0x3FFFFFFFu

__device__ __forceinline__ u32 order_ld(const u32 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void order_st(u32 *p, u32 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u64 order_ld64(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void order_st64(u64 *p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// what two of clear_batch's fills and query_prefix_kernel did: q_M and q_P zeroed, the exclusive prefix of the queries'
// descriptor counts and their total (the counter block keeps its fill: the host reads its flags whatever ran)
__global__ __launch_bounds__(256) void order_begin_kernel(const u32 *count, u32 *q_prefix, int n_queries, u32 *n_valid, u32 *q_M, unsigned long long *q_P) {
  __shared__ u32 lds[256 / SGTD_WAVE + 1];
  for (int q = threadIdx.x; q < n_queries; q += 256) { q_M[q] = 0u; q_P[q] = 0ull; }
  u32 carry = 0;
  for (int q0 = 0; q0 < n_queries; q0 += 256) {
    const int q = q0 + threadIdx.x;
    const u32 v = (q < n_queries) ? count[q] : 0;
    u32 tot;
    const u32 ex = block_excl_scan(v, lds, tot);
    if (q < n_queries) q_prefix[q] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *n_valid = carry;
}

// home_keys_kernel<u32>, grid-stride, and the keys' digit counts: four 256-bin histograms in LDS, added once per workgroup
// to hist[4][256] — no kernel reads the keys only to count them; and pos_of_slot's reset, which was a launch of its own
__global__ __launch_bounds__(256) void home_keys_hist_kernel(QueryView Q, const u32 *q_prefix, u32 *keys, u32 *vals, long long n_slots, int cbits, int sub_bits,
                                                             u32 *hist, u32 *pos_of_slot, size_t n_pass_slots) {
  __shared__ u32 h[4 * 256];
  for (int i = threadIdx.x; i < 4 * 256; i += 256) h[i] = 0u;
  __syncthreads();
  const u64 cmask = (1ull << cbits) - 1ull;
  const int ny = 1 << (sub_bits >> 1), nz = 1 << (sub_bits - (sub_bits >> 1));
  for (long long d = (long long)blockIdx.x * 256 + threadIdx.x; d < n_slots; d += (long long)gridDim.x * 256) {
    const int q = (int)(d / Q.stride);
    const u32 i = (u32)(d - (long long)q * Q.stride);
    if (i >= Q.count[q]) continue;
    const u64 code = label_code(Q.label[d * 3 + 0], Q.label[d * 3 + 1], Q.label[d * 3 + 2]);
    const double s0 = Q.side[d * 3 + 0], s1 = Q.side[d * 3 + 1], s2 = Q.side[d * 3 + 2];
    const u64 x = home_coord(s0, cmask), y = home_coord(s1, cmask), z = home_coord(s2, cmask);
    const double f1 = s1 - (double)(int)s1, f2 = s2 - (double)(int)s2;
    const u64 sub = (u64)min(max((int)(f1 * ny), 0), ny - 1) * nz + (u64)min(max((int)(f2 * nz), 0), nz - 1);
    const u32 key = (u32)(((((code << cbits | x) << cbits | y) << cbits) | z) << sub_bits | sub);
    const u32 idx = q_prefix[q] + i;
    keys[idx] = key;
    vals[idx] = (u32)d;
#pragma unroll
    for (int b = 0; b < 4; b++) atomicAdd(&h[b * 256 + ((key >> (8 * b)) & 255u)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4 * 256; i += 256)
    if (h[i]) atomicAdd(&hist[i], h[i]);
  // pos_of_slot = SGTD_NO_PASS everywhere (the launch train's 0xFF fill), 16 bytes a lane
  uint4 *p4 = reinterpret_cast<uint4 *>(pos_of_slot);
  const size_t n4 = n_pass_slots / 4, step = (size_t)gridDim.x * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (size_t i = first; i < n4; i += step) p4[i] = make_uint4(SGTD_NO_PASS, SGTD_NO_PASS, SGTD_NO_PASS, SGTD_NO_PASS);
  for (size_t i = n4 * 4 + first; i < n_pass_slots; i += step) pos_of_slot[i] = SGTD_NO_PASS;
}

// One stable radix pass over digit `pass` of the n_valid live keys.  Wave w of a tile owns its positions
// [w T / 8, (w + 1) T / 8) in rounds of 64: a key's place among the tile's keys of its digit is (keys of that digit in
// the waves before) + (in this wave's earlier rounds) + (among the round's lower lanes) — slot order, so the pass is stable.
__global__ __launch_bounds__(SGTD_OS_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void order_sort_pass_kernel(      // (two workgroups per CU: at most 128 registers)
const u32 *keys_in, const u32 *vals_in, u32 *keys_out, u32 *vals_out,
                                                                          const u32 *n_valid_p, long long n_cap, u32 *work, u32 tiles_cap, int pass,
                                                                          u32 max_polls, u32 *giveup) {
  constexpr int NW = SGTD_OS_THREADS / SGTD_WAVE;
  constexpr u32 PER_WAVE = SGTD_OS_TILE / NW;
  __shared__ u32 s_key[SGTD_OS_TILE], s_val[SGTD_OS_TILE];
  __shared__ u32 s_wcnt[NW][256];      // keys of (wave, digit) so far; after the ranking: of the waves before
  __shared__ u32 s_start[256];         // first place of a digit in the tile's sorted image
  __shared__ u32 s_gbase[256];         // (global position of the digit's first key of this tile) - s_start
  __shared__ u32 s_scan[NW + 1];
  __shared__ u32 s_tile, s_quit;
  const u32 tid = threadIdx.x, wid = tid >> 6, lane = tid & 63u;
  const u32 nv = (u32)min((long long)*n_valid_p, n_cap);
  const u32 ntiles = min((nv + SGTD_OS_TILE - 1u) / SGTD_OS_TILE, tiles_cap);
  if (blockIdx.x >= ntiles) return;      // (exactly ntiles workgroups take a ticket)
  if (tid == 0) { s_tile = atomicAdd(&work[OW_TICKET + pass], 1u); s_quit = order_ld(giveup); }
  for (u32 i = tid; i < NW * 256u; i += SGTD_OS_THREADS) (&s_wcnt[0][0])[i] = 0u;
  __syncthreads();
  const u32 tile = s_tile;
  if (s_quit || tile >= ntiles) return;
  u32 *state = work + order_sort_state_at(pass, tiles_cap);
  const u32 base = tile * SGTD_OS_TILE, n_tile = min((u32)SGTD_OS_TILE, nv - base);
  const int shift = 8 * pass;
  u32 key[SGTD_OS_ITEMS], place[SGTD_OS_ITEMS];
#pragma unroll
  for (int r = 0; r < SGTD_OS_ITEMS; r++) {
    const u32 i = wid * PER_WAVE + (u32)r * SGTD_WAVE + lane;
    key[r] = i < n_tile ? keys_in[base + i] : 0xFFFFFFFFu;
  }
#pragma unroll
  for (int r = 0; r < SGTD_OS_ITEMS; r++) {
    const u32 i = wid * PER_WAVE + (u32)r * SGTD_WAVE + lane;
    const bool valid = i < n_tile;
    const u32 digit = (key[r] >> shift) & 255u;
    u32 rank, count;
    wave_group_rank<8>(digit, valid, rank, count);
    const u32 have = s_wcnt[wid][digit];
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0) s_wcnt[wid][digit] = have + count;
    __builtin_amdgcn_wave_barrier();
    place[r] = have + rank;
  }
  __syncthreads();
  // digit `tid`: the waves' counts to their exclusive prefix, the tile's count to its successors
  u32 cnt = 0;
  if (tid < 256u) {
#pragma unroll
    for (int w = 0; w < NW; w++) { const u32 t = s_wcnt[w][tid]; s_wcnt[w][tid] = cnt; cnt += t; }
    order_st(&state[(size_t)tile * 256 + tid], ((tile == 0 ? SGTD_ST_INCL : SGTD_ST_AGG) << 30) | cnt);
  }
  u32 tot;
  const u32 start = block_excl_scan(cnt, s_scan, tot);
  const u32 gstart = block_excl_scan(tid < 256u ? work[OW_HIST + pass * 256 + tid] : 0u, s_scan, tot);      // the digit's first key of the whole batch
  // keys of the digit in the tiles before: back over their state words to the first inclusive one
  u32 before = 0;
  bool quit = false;
  if (tid < 256u && tile > 0) {
    // (a window of words is loaded at once and taken in order up to the first empty one: the tiles that start together
    // publish their own counts together, and a walk back over them one load at a time is one memory latency per tile)
    u32 polls = max_polls, idle = 0, t = tile;      // tiles [0, t) are still to be counted
    bool done = false;
    while (!done) {
      if (polls == 0) { quit = true; break; }
      polls -= min(polls, (u32)SGTD_ORDER_WINDOW);
      u32 s[SGTD_ORDER_WINDOW];
#pragma unroll
      for (int w = 0; w < SGTD_ORDER_WINDOW; w++) s[w] = (u32)w < t ? order_ld(&state[(size_t)(t - 1u - (u32)w) * 256 + tid]) : 0u;
      const u32 t0 = t;
      bool stop = false;
#pragma unroll
      for (int w = 0; w < SGTD_ORDER_WINDOW; w++) {
        if (stop || (u32)w >= t0) continue;
        if ((s[w] >> 30) == 0u) { stop = true; continue; }
        before += s[w] & SGTD_ST_MASK;
        t = t0 - 1u - (u32)w;
        if ((s[w] >> 30) == SGTD_ST_INCL || t == 0u) { done = true; stop = true; }
      }
      if (t == t0) {      // the nearest word is still empty
        if ((++idle & 255u) == 0u && order_ld(giveup)) { quit = true; break; }
        __builtin_amdgcn_s_sleep(2);
      }
    }
    if (quit) { order_st(giveup, 1u); s_quit = 1u; }
    else order_st(&state[(size_t)tile * 256 + tid], (SGTD_ST_INCL << 30) | (before + cnt));
  }
  if (tid < 256u) { s_start[tid] = start; s_gbase[tid] = gstart + before - start; }
  __syncthreads();
  if (s_quit) return;
  // the tile's sorted image in LDS (the values are loaded here: sixteen registers fewer through the ranking and the look-back), then
  // every digit's run to consecutive addresses
  u32 val[SGTD_OS_ITEMS];
#pragma unroll
  for (int r = 0; r < SGTD_OS_ITEMS; r++) {
    const u32 i = wid * PER_WAVE + (u32)r * SGTD_WAVE + lane;
    val[r] = i < n_tile ? vals_in[base + i] : 0u;
  }
#pragma unroll
  for (int r = 0; r < SGTD_OS_ITEMS; r++) {
    const u32 i = wid * PER_WAVE + (u32)r * SGTD_WAVE + lane;
    if (i < n_tile) {
      const u32 digit = (key[r] >> shift) & 255u;
      const u32 at = s_start[digit] + s_wcnt[wid][digit] + place[r];
      s_key[at] = key[r];
      s_val[at] = val[r];
    }
  }
  __syncthreads();
  for (u32 j = tid; j < n_tile; j += SGTD_OS_THREADS) {
    const u32 k = s_key[j];
    const u32 g = s_gbase[(k >> shift) & 255u] + j;
    if (g < nv) { keys_out[g] = k; vals_out[g] = s_val[j]; }      // (always, while the histograms count the same keys)
  }
}

// inclusive running maximum over the lanes (wave_incl_scan's steps with max for +; 0 is the identity)
__device__ __forceinline__ u32 wave_incl_max_scan(u32 v) {
  int x = (int)v;
#define SGTD_MAX_STEP(ctrl, rows) { const u32 o = (u32)__builtin_amdgcn_update_dpp(0, x, ctrl, rows, 0xf, false); x = (int)((u32)x > o ? (u32)x : o); }
  SGTD_MAX_STEP(0x111, 0xf) SGTD_MAX_STEP(0x112, 0xf) SGTD_MAX_STEP(0x114, 0xf) SGTD_MAX_STEP(0x118, 0xf)
  SGTD_MAX_STEP(0x142, 0xa) SGTD_MAX_STEP(0x143, 0xc)
#undef SGTD_MAX_STEP
  return (u32)x;
}

__device__ __forceinline__ bool order_group_head(u32 key, u32 key_before, int cbits, int sub_bits) {      // group_heads_kernel's rule
  const u32 a = key >> sub_bits, b = key_before >> sub_bits;
  const u32 cmask = (1u << cbits) - 1u;
  return (a != b) || ((a & cmask) == cmask) || (((a >> cbits) & cmask) == cmask) || (((a >> (2 * cbits)) & cmask) == cmask);
}

// The group index from the sorted keys, over the live positions only: position p heads a group where p = 0 or
// group_heads_kernel's rule holds between keys p - 1 and p.  With H(p) the heads in 0 .. p and F(p) the last head at or
// before p: gid[p] = H(p) - 1, group_first[gid] = p at a head, n_groups = H(n_valid - 1), and the pass slot of a leader
// (pass_slots_kernel's rule) from gid and F.  A tile's state word carries the pair (heads, last head position + 1), so a
// group that began tiles ago still knows its first position.
__global__ __launch_bounds__(SGTD_GI_THREADS) void order_groups_kernel(const u32 *keys, u32 *n_valid_p, u32 *gid, u32 *group_first, u32 *n_groups,
                                                                       u32 *pos_of_slot, u32 slot_cap, long long n_cap, u32 *ticket, u64 *state,
                                                                       u32 tiles_cap, int cbits, int sub_bits, int pair, u32 max_polls, u32 *giveup,
                                                                       int *overflow) {
  constexpr int NW = SGTD_GI_THREADS / SGTD_WAVE;
  __shared__ u32 s_scan[NW + 1], s_max[NW];
  __shared__ u32 s_tile, s_quit, s_heads, s_last;
  const u32 tid = threadIdx.x, wid = tid >> 6, lane = tid & 63u;
  const u32 nv = (u32)min((long long)*n_valid_p, n_cap);
  if (order_ld(giveup)) {      // a sort pass gave up: the batch is left empty and flagged, sgtd_sync runs it again
    if (blockIdx.x == 0 && tid == 0) { order_st(n_valid_p, 0u); order_st(n_groups, 0u); order_st(reinterpret_cast<u32 *>(overflow), 1u); }
    return;
  }
  if (nv == 0) { if (blockIdx.x == 0 && tid == 0) *n_groups = 0u; return; }
  const u32 ntiles = min((nv + SGTD_GI_TILE - 1u) / SGTD_GI_TILE, tiles_cap);
  if (blockIdx.x >= ntiles) return;
  if (tid == 0) { s_tile = atomicAdd(ticket, 1u); s_quit = 0u; }
  __syncthreads();
  const u32 tile = s_tile;
  if (tile >= ntiles) return;
  const u32 p0 = tile * SGTD_GI_TILE + tid * SGTD_GI_ITEMS;
  const bool full = (tile + 1u) * SGTD_GI_TILE <= nv;
  u32 k[SGTD_GI_ITEMS];
  if (full) {
    const uint4 *src = reinterpret_cast<const uint4 *>(keys + p0);
#pragma unroll
    for (int j = 0; j < SGTD_GI_ITEMS / 4; j++) { const uint4 w = src[j]; k[4 * j] = w.x; k[4 * j + 1] = w.y; k[4 * j + 2] = w.z; k[4 * j + 3] = w.w; }
  } else {
#pragma unroll
    for (int j = 0; j < SGTD_GI_ITEMS; j++) k[j] = p0 + j < nv ? keys[p0 + j] : 0u;
  }
  u32 before = (p0 > 0 && p0 < nv) ? keys[p0 - 1] : 0u;
  u32 heads = 0, mine = 0, last = 0;      // bit j: position p0 + j heads a group; their number; the last one's position + 1
#pragma unroll
  for (int j = 0; j < SGTD_GI_ITEMS; j++) {
    const u32 p = p0 + j;
    const bool h = p < nv && (p == 0 || order_group_head(k[j], before, cbits, sub_bits));
    before = k[j];
    if (h) { heads |= 1u << j; mine++; last = p + 1u; }
  }
  u32 tile_heads;
  const u32 ex_heads = block_excl_scan(mine, s_scan, tile_heads);
  const u32 inc_last = wave_incl_max_scan(last);
  if (lane == SGTD_WAVE - 1) s_max[wid] = inc_last;
  __syncthreads();
  u32 ex_last = (u32)__shfl_up((int)inc_last, 1);
  if (lane == 0) ex_last = 0;
  u32 tile_last = 0;
#pragma unroll
  for (int w = 0; w < NW; w++) { const u32 m = s_max[w]; if ((u32)w < wid) ex_last = max(ex_last, m); tile_last = max(tile_last, m); }
  // the pair of the tiles before (thread 0): back to the first inclusive word
  if (tid == 0) {
    u32 c_heads = 0, c_last = 0;
    bool quit = false;
    if (tile > 0) {
      order_st64(&state[tile], ((u64)SGTD_ST_AGG << 62) | ((u64)tile_heads << 31) | (u64)tile_last);
      u32 polls = max_polls, idle = 0, t = tile;      // tiles [0, t) are still to be counted (windows: order_sort_pass_kernel)
      bool done = false;
      while (!done) {
        if (polls == 0) { quit = true; break; }
        polls -= min(polls, (u32)SGTD_ORDER_WINDOW);
        u64 s[SGTD_ORDER_WINDOW];
#pragma unroll
        for (int w = 0; w < SGTD_ORDER_WINDOW; w++) s[w] = (u32)w < t ? order_ld64(&state[t - 1u - (u32)w]) : 0ull;
        const u32 t0 = t;
        bool stop = false;
#pragma unroll
        for (int w = 0; w < SGTD_ORDER_WINDOW; w++) {
          if (stop || (u32)w >= t0) continue;
          if ((s[w] >> 62) == 0ull) { stop = true; continue; }
          c_heads += (u32)(s[w] >> 31) & 0x7FFFFFFFu;
          if (c_last == 0) c_last = (u32)s[w] & 0x7FFFFFFFu;
          t = t0 - 1u - (u32)w;
          if ((u32)(s[w] >> 62) == SGTD_ST_INCL || t == 0u) { done = true; stop = true; }
        }
        if (t == t0) {      // the nearest word is still empty
          if ((++idle & 255u) == 0u && order_ld(giveup)) { quit = true; break; }
          __builtin_amdgcn_s_sleep(2);
        }
      }
    }
    if (quit) {
      order_st(giveup, 1u); order_st(n_valid_p, 0u); order_st(n_groups, 0u); order_st(reinterpret_cast<u32 *>(overflow), 1u);
      s_quit = 1u;
    } else {
      order_st64(&state[tile], ((u64)SGTD_ST_INCL << 62) | ((u64)(c_heads + tile_heads) << 31) | (u64)(tile_last ? tile_last : c_last));
    }
    s_heads = c_heads; s_last = c_last;
  }
  __syncthreads();
  if (s_quit) return;
  u32 H = s_heads + ex_heads, F = ex_last ? ex_last : s_last;      // heads before p0, last head before p0 (+ 1)
  u32 g[SGTD_GI_ITEMS];
#pragma unroll
  for (int j = 0; j < SGTD_GI_ITEMS; j++) {
    const u32 p = p0 + j;
    if ((heads >> j) & 1u) { H++; F = p + 1u; }
    g[j] = H - 1u;
    if (p < nv) {
      if (((heads >> j) & 1u) && H <= nv) group_first[H - 1u] = p;      // (H <= p + 1 always)
      if (!pair) pos_of_slot[p] = p;
      else {
        const u32 f = F - 1u;
        if (((p - f) % SGTD_PAIR) == 0u) {
          const u32 s = (H - 1u) + (f + SGTD_PAIR - 1u) / SGTD_PAIR + (p - f) / SGTD_PAIR;
          if (s < slot_cap) pos_of_slot[s] = p;
        }
      }
      if (p == nv - 1u) *n_groups = H;
    }
  }
  if (full) {
    uint4 *dst = reinterpret_cast<uint4 *>(gid + p0);
#pragma unroll
    for (int j = 0; j < SGTD_GI_ITEMS / 4; j++) dst[j] = make_uint4(g[4 * j], g[4 * j + 1], g[4 * j + 2], g[4 * j + 3]);
  } else {
#pragma unroll
    for (int j = 0; j < SGTD_GI_ITEMS; j++) if (p0 + j < nv) gid[p0 + j] = g[j];
  }
}
