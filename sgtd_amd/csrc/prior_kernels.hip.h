// prior_kernels.hip.h — sgtd_set_position_prior: the batch's frame-filter rows built on the device from the map poses.
//
// Runs in reserve_select (sgtd_accel.hip) where prepare_filter would upload host rows, only when the batch has a prior.  It writes the
// rows filter_records_kernel / filter_compact_kernel read (filter_kernels.hip.h: bit f of row r = local frame f of
// the table's span allowed to query r), so the filter pass and everything after it run unchanged.
//
//   prior_rows_kernel       one wave per (row, 64-frame word): lane l tests local frame word * 64 + l against the row's
//                           prior, one ballot makes the word, lane 0 stores it — ANDed with the re-based filter row
//                           when a filter is set too.  Frames beyond the span are never allowed (the last word's high
//                           bits stay clear).
//
// The test (include/sgtd_accel.h): frame f is allowed by (c, rr = r*r) iff it has a pose, the tested coordinates of its
// translation are finite, and d2 <= rr with dx = (double)t[0] - c.x, ..., d2 = (dx*dx + dy*dy) + dz*dz, all f64 and
// built with -ffp-contract=off (dims 2 has no dz term).
#pragma once
#include "common.hip.h"

#define SGTD_PRIOR_THREADS 256

// pos: (t0, t1, t2, has pose) per local frame of the span; prm: (cx, cy, cz, rr) per prior row (one for every row when
// prm_rows == 1); base: the re-based filter rows (nullptr: no filter), one for every row when base_rows == 1.
__global__ __launch_bounds__(SGTD_PRIOR_THREADS) void prior_rows_kernel(const float4 *pos, u32 span, u32 words, const double4 *prm,
                                                                        int prm_rows, int dims, const u64 *base, int base_rows,
                                                                        int n_rows, u64 *rows) {
  const long long wv = ((long long)blockIdx.x * SGTD_PRIOR_THREADS + threadIdx.x) / SGTD_WAVE;
  if (wv >= (long long)n_rows * words) return;      // (whole waves)
  const int r = (int)(wv / words);
  const u32 w = (u32)(wv % words), f = w * SGTD_WAVE + (u32)lane_id();
  bool in = false;
  if (f < span) {
    const float4 p = pos[f];
    const double4 c = prm[prm_rows == 1 ? 0 : r];
    if (p.w != 0.f) {
      const double dx = (double)p.x - c.x, dy = (double)p.y - c.y;
      double d2 = dx * dx + dy * dy;
      bool fin = __builtin_isfinite(p.x) && __builtin_isfinite(p.y);
      if (dims == 3) {
        const double dz = (double)p.z - c.z;
        d2 = d2 + dz * dz;
        fin = fin && __builtin_isfinite(p.z);
      }
      in = fin && d2 <= c.w;
    }
  }
  u64 m = __ballot(in);
  if (lane_id() == 0) {
    if (base) m &= base[(size_t)(base_rows == 1 ? 0 : r) * words + w];
    rows[(size_t)r * words + w] = m;
  }
}
