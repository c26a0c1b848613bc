// filter_kernels.hip.h — sgtd_set_frame_filter: the match records of frames a query may not see leave its lists.
//
// One pass right after resolve_undecided_kernel (sgtd_accel.hip, plan_and_sweep), only when the batch has a filter.
// Every later stage already skips dead records (votes, top-k, the match lists, verification, the one-frame path), so
// the sweep and the vote and list passes run unchanged.
//
//   filter_records_kernel<IN_LDS>       a record whose local frame (rec >> id_bits) has no bit in its query's row becomes
//                                       SGTD_DEAD_ID; the query's match count loses the killed records (one atomic per
//                                       wave).  Records already dead stay dead and are not counted again.
//   filter_compact_kernel<IN_LDS>       the diagnostic build (rec_cell / rec_dis beside the records): the list is compacted
//                                       in place instead, in order, and its length shrinks — the rough list
//                                       (rough_gather_kernel) reads every record of a list and never sees dead ones.  The
//                                       votes pass counts the shorter lists, so q_M is not touched.
//
// Grid: wg_per_q workgroups of SGTD_FILT_THREADS per query (query blockIdx.x / wg_per_q).  A wave takes 64 consecutive
// descriptor slots of its query at a time, loads their list heads in one coalesced read, and walks the lists one by
// one with the next list's first 256 records in flight while it tests the current one.  The query's row (bit f for
// local frame f of the table, n_words 64-bit words) is staged in LDS once per workgroup; beyond 64 KB (2^19 frames) it
// is read from memory.
#pragma once
#include "common.hip.h"
#include "probe_kernels.hip.h"

#define SGTD_FILT_THREADS 256
#define SGTD_FILT_WAVES (SGTD_FILT_THREADS / SGTD_WAVE)

// is local frame f allowed by `row`?  (f < span is part of the test: a dead record's frame lies beyond every span)
__device__ __forceinline__ bool filt_allowed(const u64 *row, u32 span, u32 f) { return f < span && ((row[f >> 6] >> (f & 63u)) & 1ull); }

template <bool IN_LDS>
__device__ __forceinline__ const u64 *filt_stage_row(const u64 *rows, int n_rows, u32 n_words, int q, u64 *lds) {
  const u64 *row = rows + (size_t)(n_rows == 1 ? 0 : q) * n_words;
  if (!IN_LDS) return row;
  for (u32 w = threadIdx.x; w < n_words; w += SGTD_FILT_THREADS) lds[w] = row[w];
  __syncthreads();
  return lds;
}

template <bool IN_LDS>
__global__ __launch_bounds__(SGTD_FILT_THREADS) void filter_records_kernel(QueryView Q, ProbeBuffers B, const u64 *rows, int n_rows,
                                                                          u32 n_words, u32 span, int wg_per_q, u32 *q_M) {
  extern __shared__ u64 filt_lds[];
  if (B.overflow()[0]) return;      // the batch is re-run (list lengths may exceed what was stored): leave it
  const int q = blockIdx.x / wg_per_q, part = blockIdx.x % wg_per_q;
  const u64 *row = filt_stage_row<IN_LDS>(rows, n_rows, n_words, q, filt_lds);
  const int lane = lane_id(), wave = part * SGTD_FILT_WAVES + (threadIdx.x >> 6), n_waves = wg_per_q * SGTD_FILT_WAVES;
  const u32 cnt = Q.count[q], id_bits = B.id_bits;
  const uint2 *list = B.list + (long long)q * Q.stride;
  u32 killed = 0;
  // the four records of a quad tested, the dead written back where one changed
  auto test = [&](uint4 &r, u32 *at, u32 valid) {
    u32 w[4] = {r.x, r.y, r.z, r.w};
    bool changed = false;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if ((u32)i < valid && w[i] != SGTD_DEAD_ID && !filt_allowed(row, span, w[i] >> id_bits)) {
        w[i] = SGTD_DEAD_ID;
        changed = true;
        killed++;
      }
    }
    if (changed) *reinterpret_cast<uint4 *>(at) = make_uint4(w[0], w[1], w[2], w[3]);
  };
  for (u32 d0 = (u32)wave * SGTD_WAVE; d0 < cnt; d0 += (u32)n_waves * SGTD_WAVE) {
    const u32 n_here = min((u32)SGTD_WAVE, cnt - d0);
    const uint2 head = (u32)lane < n_here ? list[d0 + lane] : make_uint2(0u, 0u);
    // the first quad of each lane in list j: lane's quad of the list's first 256 records
    auto first = [&](u32 j, uint4 &r) {
      const u32 g = (u32)__builtin_amdgcn_readlane((int)head.x, j), m = (u32)__builtin_amdgcn_readlane((int)head.y, j);
      if ((u32)lane * 4u < m) r = *reinterpret_cast<const uint4 *>(B.rec_at(g) + lane * 4);
    };
    uint4 nxt = make_uint4(0u, 0u, 0u, 0u);
    first(0, nxt);
    for (u32 j = 0; j < n_here; j++) {
      uint4 cur = nxt;
      if (j + 1 < n_here) first(j + 1, nxt);
      const u32 g = (u32)__builtin_amdgcn_readlane((int)head.x, j), m = (u32)__builtin_amdgcn_readlane((int)head.y, j);
      u32 *base = B.rec_at(g);
      if ((u32)lane * 4u < m) test(cur, base + lane * 4, min(4u, m - (u32)lane * 4u));
      for (u32 k = (u32)lane + SGTD_WAVE; k * 4u < m; k += SGTD_WAVE) {      // lists beyond 256 records
        uint4 r = *reinterpret_cast<const uint4 *>(base + k * 4);
        test(r, base + k * 4, min(4u, m - k * 4u));
      }
    }
  }
  const u32 total = wave_sum(killed);
  if (lane == 0 && total) atomicSub(&q_M[q], total);
}

template <bool IN_LDS>
__global__ __launch_bounds__(SGTD_FILT_THREADS) void filter_compact_kernel(QueryView Q, ProbeBuffers B, const u64 *rows, int n_rows,
                                                                          u32 n_words, u32 span, int wg_per_q) {
  extern __shared__ u64 filt_lds[];
  if (B.overflow()[0]) return;
  const int q = blockIdx.x / wg_per_q, part = blockIdx.x % wg_per_q;
  const u64 *row = filt_stage_row<IN_LDS>(rows, n_rows, n_words, q, filt_lds);
  const int lane = lane_id(), wave = part * SGTD_FILT_WAVES + (threadIdx.x >> 6), n_waves = wg_per_q * SGTD_FILT_WAVES;
  const u32 cnt = Q.count[q], id_bits = B.id_bits;
  uint2 *list = B.list + (long long)q * Q.stride;
  for (u32 d = (u32)wave; d < cnt; d += (u32)n_waves) {
    const uint2 lp = list[d];
    const size_t p0 = B.rec_index(lp.x);
    u32 out = 0;
    // 64 records per step, all read before any is written; a kept record moves to out + its rank (never beyond
    // where it was read), so the next step's reads are untouched
    for (u32 j0 = 0; j0 < lp.y; j0 += SGTD_WAVE) {
      const u32 j = j0 + (u32)lane;
      const bool in = j < lp.y;
      const u32 r = in ? B.rec[p0 + j] : SGTD_DEAD_ID;
      const unsigned char c = in ? B.rec_cell[p0 + j] : 0;
      const double dis = in ? B.rec_dis[p0 + j] : 0.0;
      const bool keep = in && (r == SGTD_DEAD_ID || filt_allowed(row, span, r >> id_bits));
      const u64 m = __ballot(keep);
      if (keep) {
        const size_t at = p0 + out + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
        B.rec[at] = r;
        B.rec_cell[at] = c;
        B.rec_dis[at] = dis;
      }
      out += (u32)__popcll(m);
    }
    if (lane == 0 && out != lp.y) list[d].y = out;
  }
}
