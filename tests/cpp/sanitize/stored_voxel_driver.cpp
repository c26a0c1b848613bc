// stored_voxel_driver.cpp — the host bookkeeping of sgtd_register_stored_voxels (sgtd_accel.hip) under ASan + UBSan,
// against hip_stub.cpp.  "Device" memory is host memory there and no kernel runs, so the launch hook below does on the host
// what the call's bookkeeping shows in: the store's own kernels (pack, compact), a covariance that names its point where
// reg_cov_kernel would have written one, and of the voxel run the keys (one voxel per distinct first coordinate of a map's
// member points, read through map_cloud, mem_pt_off and the arena's offsets exactly as vreg_keys_kernel reads them), the
// voxel heads, the maps' ranges and result rows that name their source and their map.  The driver keeps a model of the
// store (frame -> points) and compares every map's voxels with it: members looked up by slot on a store with dead slots,
// after a compaction and after a growth that the call's own tail causes, a frame in several maps and twice in one, empty
// maps and members, map and member offsets, every cap and error path with the earlier results kept, two "devices" behind
// one handle.  Every copy the engine makes is checked by the sanitizer against the real size of the allocation; at the end
// no device block is left.
// What it does not reach: of sgtd_register_stored_local_loops only the returns that come before a verified batch is asked
// for (SGTD_ERR_INVALID, SGTD_ERR_STATE, a multi-device handle's SGTD_ERR_UNSUPPORTED).  The stand-in cannot produce a
// verified batch, so that call's host bookkeeping behind it (the offsets into its two device buffers, the rows and member
// offsets it assembles, the caps on what was formed) runs only on the device, in tests/test_gpu_register_stored_local_loops.py,
// and its SGTD_ERR_UNSUPPORTED for formed rows or maps beyond a cap is not exercised anywhere.
// Compiled for the host only; tests/test_stored_voxel_sanitize.py builds and runs it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include <stdint.h>

#include "../../../include/sgtd_accel.h"
// the kernels' argument structs come with the kernels themselves: in a namespace of their own here, so that this file's
// copies of the host-side launch stubs do not collide with the engine's
namespace kernels_of_the_engine {
#include "../../../sgtd_amd/csrc/build_kernel.hip.h"       // (the engine's own include order: the headers lean on each other)
#include "../../../sgtd_amd/csrc/common.hip.h"
#include "../../../sgtd_amd/csrc/table_kernels.hip.h"
#include "../../../sgtd_amd/csrc/probe_kernels.hip.h"
#include "../../../sgtd_amd/csrc/select_kernels.hip.h"
#include "../../../sgtd_amd/csrc/verify_kernels.hip.h"
#include "../../../sgtd_amd/csrc/refine_kernels.hip.h"
#include "../../../sgtd_amd/csrc/relax_kernels.hip.h"
#include "../../../sgtd_amd/csrc/register_kernels.hip.h"
#include "../../../sgtd_amd/csrc/voxel_register_kernels.hip.h"
#include "../../../sgtd_amd/csrc/cloud_store_kernels.hip.h"
}  // namespace kernels_of_the_engine
namespace K = kernels_of_the_engine;
using K::u32;
using K::u64;

extern "C" {
typedef void (*launch_hook_t)(const char *name, void **args, void *user);
void sgtd_stub_set_launch_hook(launch_hook_t h, void *user);
size_t sgtd_stub_device_blocks();
}

#define REQUIRE(x) do { if (!(x)) { fprintf(stderr, "stored_voxel_driver: %s failed at line %d\n", #x, __LINE__); exit(1); } } while (0)
static sgtd_handle g_h = nullptr;
#define OK(call) do { const int st_ = (call); if (st_ != SGTD_OK) { fprintf(stderr, "stored_voxel_driver: %s = %d at line %d (%s)\n", #call, st_, __LINE__, g_h ? sgtd_last_error(g_h) : ""); exit(1); } } while (0)

namespace {
int g_compactions = 0, g_cov_points = 0, g_key_points = 0;

// `kernel` is the function the (mangled) name names: reg_init_kernel is not vreg_init_kernel
bool names(const char *name, const char *kernel) {
  const char *at = strstr(name, kernel);
  return at && at > name && at[-1] >= '0' && at[-1] <= '9';
}

void hook(const char *name, void **args, void *) {
  if (names(name, "store_pack_kernel")) {
    const float *src = *static_cast<const float **>(args[0]);
    const int stride = *static_cast<int *>(args[1]);
    const long long n = *static_cast<long long *>(args[2]);
    float *dst = *static_cast<float **>(args[3]);
    for (long long i = 0; i < n; i++)
      for (int a = 0; a < 3; a++) dst[i * 3 + a] = src[i * stride + a];
  } else if (names(name, "store_compact_kernel")) {
    const K::StoreMoveParams &P = *static_cast<const K::StoreMoveParams *>(args[0]);
    for (int s = 0; s < P.n_live; s++)
      for (long long g = P.to[s]; g < P.to[s + 1]; g++) {
        const long long f = P.from[s] + (g - P.to[s]);
        for (int a = 0; a < 3; a++) P.pts_out[g * 3 + a] = P.pts_in[f * 3 + a];
        for (int a = 0; a < 9; a++) P.cov_out[g * 9 + a] = P.cov_in[f * 9 + a];
      }
    g_compactions++;
  } else if (names(name, "reg_cov_kernel")) {
    // a covariance that names its point
    const K::RegParams &P = *static_cast<const K::RegParams *>(args[0]);
    for (int b = 0; b < P.n_ctiles; b++) {
      const long long base = P.pt_off[P.ctile_cloud[b]], n = P.pt_off[P.ctile_cloud[b] + 1] - base;
      REQUIRE(P.ctile_first[b] < n);
      for (long long i = P.ctile_first[b]; i < std::min<long long>(n, P.ctile_first[b] + 128); i++) {
        double *c = P.cov + (base + i) * 9;
        c[0] = (double)P.pts[(base + i) * P.stride];
        c[1] = 77.0;
        g_cov_points++;
      }
    }
  } else if (names(name, "vreg_keys_kernel")) {
    // member point i of the maps, found the way the kernel finds it; its covariance came with the store
    const K::RegParams &P = *static_cast<const K::RegParams *>(args[0]);
    const K::VregParams &V = *static_cast<const K::VregParams *>(args[1]);
    u64 *keys = *static_cast<u64 **>(args[2]);
    u32 *vals = *static_cast<u32 **>(args[3]);
    REQUIRE(V.mem_pt_off[V.n_members] == V.n_member_pts);
    for (int j = 0; j < V.n_members; j++) {
      REQUIRE(V.mem_map[j] >= 0 && V.mem_map[j] < V.n_maps && V.map_off[V.mem_map[j]] <= j && j < V.map_off[V.mem_map[j] + 1]);
      const long long first = P.pt_off[V.map_cloud[j]];
      REQUIRE(P.pt_off[V.map_cloud[j] + 1] - first == V.mem_pt_off[j + 1] - V.mem_pt_off[j]);
      for (int i = V.mem_pt_off[j]; i < V.mem_pt_off[j + 1]; i++) {
        const long long g = first + (i - V.mem_pt_off[j]);
        const float x = P.pts[g * P.stride];
        REQUIRE(P.cov[g * 9] == (double)x && P.cov[g * 9 + 1] == 77.0);
        keys[i] = ((u64)V.mem_map[j] << 48) | (u64)(u32)x;
        vals[i] = (u32)i;
        g_key_points++;
      }
    }
  } else if (names(name, "radix_scatter_kernel")) {
    // a pass of the sort: the pairs move to the other buffers as they are (scan_voxels_kernel below sorts them)
    const long long n = *static_cast<long long *>(args[4]);
    memcpy(*static_cast<u64 **>(args[2]), *static_cast<const u64 **>(args[0]), (size_t)n * sizeof(u64));
    memcpy(*static_cast<u32 **>(args[3]), *static_cast<const u32 **>(args[1]), (size_t)n * sizeof(u32));
  } else if (names(name, "scan_voxels_kernel")) {
    // (the sort did not run: the keys are sorted here) the runs' keys, first points and count
    u64 *keys = *static_cast<u64 **>(args[0]);
    u32 *excl = *static_cast<u32 **>(args[2]);
    const long long n = *static_cast<long long *>(args[3]);
    u64 *vkey = *static_cast<u64 **>(args[5]);
    u32 *vstart = *static_cast<u32 **>(args[6]);
    std::sort(keys, keys + n);
    u32 nv = 0;
    for (long long i = 0; i < n; i++)
      if (i == 0 || keys[i] != keys[i - 1]) { vkey[nv] = keys[i]; vstart[nv] = (u32)i; nv++; }
    vstart[nv] = (u32)n;
    excl[n] = nv;
  } else if (names(name, "vreg_voxel_kernel")) {
    const K::VregParams &V = *static_cast<const K::VregParams *>(args[1]);
    for (u32 v = 0; v < V.n_vox; v++) V.vmean[(size_t)v * 3] = (double)(u32)(V.vkey[v] & 0xFFFFFFFFull);
  } else if (names(name, "vreg_ranges_kernel")) {
    const K::VregParams &V = *static_cast<const K::VregParams *>(args[0]);
    for (int m = 0; m <= V.n_maps; m++) {
      u32 lo = 0;
      while (lo < V.n_vox && V.vkey[lo] < ((u64)m << 48)) lo++;
      V.map_vox[m] = lo;
    }
  } else if (names(name, "vreg_trial_kernel") || names(name, "reg_trial_kernel")) {
    *static_cast<const K::RegParams *>(args[0])->unfinished = 0;
  } else if (names(name, "vreg_final_kernel")) {
    // a row that names its source's first point and size, and its map's voxels
    const K::RegParams &P = *static_cast<const K::RegParams *>(args[0]);
    const K::VregParams &V = *static_cast<const K::VregParams *>(args[1]);
    for (int k = 0; k < P.n_pairs; k++) {
      const long long s0 = P.pt_off[P.src[k]], ns = P.pt_off[P.src[k] + 1] - s0;
      P.out_pose[(size_t)k * 12] = ns ? (double)P.pts[s0 * 3] : -1.0;
      P.out_pose[(size_t)k * 12 + 1] = ns ? P.cov[s0 * 9] : -1.0;      // (the source's covariance was computed)
      P.out_matched[k] = (int)ns;
      P.out_iters[k] = (int)(V.map_vox[V.tgt_map[k] + 1] - V.map_vox[V.tgt_map[k]]);
      P.out_status[k] = k;
      V.out_corr[k] = V.tgt_map[k];
    }
  }
}

// a cloud of n points of `stride` floats whose first coordinate names (tag, point); the fourth float must never be read
std::vector<float> cloud(int tag, int n, int stride = 3) {
  std::vector<float> v((size_t)n * stride, 1e30f);
  for (int i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) v[(size_t)i * stride + a] = (float)(tag * 1000 + i) + 0.25f * a;
  return v;
}

struct Model {
  std::map<uint32_t, std::vector<float>> clouds;      // frame -> the first coordinate of every point
  int k = 5;
  double eps = 1e-3;

  void set(const std::vector<uint32_t> &frames, const std::vector<int> &sizes, int tag, int stride = 3) {
    std::vector<int64_t> off(1, 0);
    std::vector<float> pts;
    for (size_t i = 0; i < frames.size(); i++) {
      const std::vector<float> c = cloud(tag + (int)i, sizes[i], stride);
      pts.insert(pts.end(), c.begin(), c.end());
      off.push_back(off.back() + sizes[i]);
      std::vector<float> &m = clouds[frames[i]];
      m.clear();
      for (int p = 0; p < sizes[i]; p++) m.push_back(c[(size_t)p * stride]);
    }
    if (pts.empty()) pts.assign(4, 0.f);      // (a non-NULL array: NULL forgets)
    OK(sgtd_set_frame_clouds(g_h, frames.data(), off.data(), pts.data(), stride, (int64_t)frames.size(), k, eps, 0));
  }
  void forget(const std::vector<uint32_t> &frames) {
    OK(sgtd_set_frame_clouds(g_h, frames.data(), nullptr, nullptr, 3, (int64_t)frames.size(), 0, 0.0, 0));
    for (uint32_t f : frames) clouds.erase(f);
  }
  sgtd_voxel_register_options options() const {
    sgtd_voxel_register_options o;
    sgtd_default_voxel_register_options(&o);
    o.k_neighbors = k; o.plane_eps = eps; o.neighbor_mode = 7;
    return o;
  }
};

struct Call {
  std::vector<int> sizes;                    // the call's clouds
  std::vector<std::vector<uint32_t>> maps;   // the maps' member frames
  std::vector<int32_t> src, tgt;
};

// what the getters must say of a call: per map the sorted distinct first coordinates of its members' points
void verify_results(const Model &M, const Call &c) {
  const int n = (int)c.src.size(), n_maps = (int)c.maps.size();
  std::vector<size_t> voxels((size_t)n_maps);
  for (int m = 0; m < n_maps; m++) {
    std::set<float> want;
    for (uint32_t f : c.maps[(size_t)m]) want.insert(M.clouds.at(f).begin(), M.clouds.at(f).end());
    voxels[(size_t)m] = want.size();
    int64_t nv = -1;
    OK(sgtd_result_stored_voxel_map(g_h, m, nullptr, nullptr, nullptr, nullptr, 0, &nv));
    REQUIRE(nv == (int64_t)want.size());
    std::vector<double> mean((size_t)nv * 3 + 1, -5.0), cov((size_t)nv * 9 + 1, -5.0);
    std::vector<int32_t> coord((size_t)nv * 3 + 1, -5), cnt((size_t)nv + 1, -5);
    OK(sgtd_result_stored_voxel_map(g_h, m, coord.data(), cnt.data(), mean.data(), cov.data(), nv, &nv));
    REQUIRE(mean.back() == -5.0 && cov.back() == -5.0 && coord.back() == -5 && cnt.back() == -5);
    size_t v = 0, points = 0, members = 0;
    for (float x : want) REQUIRE(mean[3 * v++] == (double)x);
    for (int64_t i = 0; i < nv; i++) points += (size_t)cnt[(size_t)i];
    for (uint32_t f : c.maps[(size_t)m]) members += M.clouds.at(f).size();
    REQUIRE(points == members);
    if (nv > 1) {      // one short: the count still reported, the first entries written
      int64_t need = 0;
      std::vector<double> part((size_t)nv * 3, -5.0);
      REQUIRE(sgtd_result_stored_voxel_map(g_h, m, nullptr, nullptr, part.data(), nullptr, nv - 1, &need) == SGTD_ERR_CAPACITY && need == nv);
      REQUIRE(part[(size_t)(nv - 2) * 3] == mean[(size_t)(nv - 2) * 3] && part[(size_t)(nv - 1) * 3] == -5.0);
    }
  }
  int64_t m64 = 0;
  REQUIRE(sgtd_result_stored_voxel_map(g_h, n_maps, nullptr, nullptr, nullptr, nullptr, 0, &m64) == SGTD_ERR_INVALID);
  REQUIRE(sgtd_result_stored_voxel_map(g_h, -1, nullptr, nullptr, nullptr, nullptr, 0, &m64) == SGTD_ERR_INVALID);
  std::vector<double> pose((size_t)n * 12 + 1, -5.0), fit((size_t)n + 1), cost((size_t)n * 2 + 1);
  std::vector<int32_t> matched((size_t)n + 1), corr((size_t)n + 1), iters((size_t)n + 1), status((size_t)n + 1);
  OK(sgtd_result_stored_voxel_registered(g_h, pose.data(), fit.data(), cost.data(), matched.data(), corr.data(), iters.data(), status.data()));
  REQUIRE(pose.back() == -5.0);
  for (int k = 0; k < n; k++) {
    const int s = c.src[(size_t)k], ns = c.sizes[(size_t)s];
    REQUIRE(matched[(size_t)k] == ns && corr[(size_t)k] == c.tgt[(size_t)k] && status[(size_t)k] == k);
    REQUIRE(iters[(size_t)k] == (int)voxels[(size_t)c.tgt[(size_t)k]]);
    REQUIRE(pose[(size_t)k * 12] == (ns ? (double)((500 + s) * 1000) : -1.0) && pose[(size_t)k * 12 + 1] == pose[(size_t)k * 12]);
    int64_t need = -1;
    OK(sgtd_result_stored_voxel_matches(g_h, k, nullptr, 0, &need));
    REQUIRE(need == (int64_t)ns * 7);
    std::vector<int32_t> vox((size_t)need + 1, -7);
    OK(sgtd_result_stored_voxel_matches(g_h, k, vox.data(), need, &need));
    REQUIRE(vox.back() == -7);
    if (need > 1) REQUIRE(sgtd_result_stored_voxel_matches(g_h, k, vox.data(), need - 1, &need) == SGTD_ERR_CAPACITY);
  }
  REQUIRE(sgtd_result_stored_voxel_matches(g_h, n, nullptr, 0, &m64) == SGTD_ERR_INVALID);
  REQUIRE(sgtd_result_stored_voxel_matches(g_h, 0, nullptr, -1, &m64) == SGTD_ERR_INVALID);
}

void stored_voxel_call(const Model &M, const Call &c, int stride, bool device, bool poses) {
  std::vector<int64_t> off(1, 0);
  std::vector<float> pts;
  for (size_t i = 0; i < c.sizes.size(); i++) {
    const std::vector<float> cl = cloud(500 + (int)i, c.sizes[i], stride);
    pts.insert(pts.end(), cl.begin(), cl.end());
    off.push_back(off.back() + c.sizes[i]);
  }
  if (pts.empty()) pts.assign(4, 0.f);
  float *arg = pts.data();
  void *dev = nullptr;
  if (device) {
    REQUIRE(hipMalloc(&dev, pts.size() * sizeof(float)) == hipSuccess);
    memcpy(dev, pts.data(), pts.size() * sizeof(float));
    arg = static_cast<float *>(dev);
  }
  std::vector<int32_t> map_off(1, 0);
  std::vector<uint32_t> map_frame;
  for (const auto &m : c.maps) { map_frame.insert(map_frame.end(), m.begin(), m.end()); map_off.push_back((int32_t)map_frame.size()); }
  std::vector<double> map_pose;
  if (poses)
    for (size_t j = 0; j < map_frame.size(); j++)
      for (int a = 0; a < 12; a++) map_pose.push_back(a % 4 == 0 && a < 9 ? 1.0 : 0.0);
  const sgtd_voxel_register_options o = M.options();
  const int covs = g_cov_points;
  OK(sgtd_register_stored_voxels(g_h, &o, arg, stride, off.data(), (int)c.sizes.size(), map_off.data(), map_frame.data(),
                                 poses ? map_pose.data() : nullptr, (int)c.maps.size(), c.src.data(), c.tgt.data(), nullptr, (int)c.src.size(),
                                 device ? 1 : 0));
  if (dev) REQUIRE(hipFree(dev) == hipSuccess);
  // covariances: of the call's clouds that some pair names, and of nothing else
  std::set<int32_t> named(c.src.begin(), c.src.end());
  int want = 0;
  for (int32_t s : named) want += c.sizes[(size_t)s];
  REQUIRE(g_cov_points - covs == want);
  verify_results(M, c);
}
}  // namespace

int main() {
  setenv("SGTD_CLOUD_STORE_INIT_POINTS", "64", 1);
  sgtd_stub_set_launch_hook(hook, nullptr);
  sgtd_config cfg;
  sgtd_default_config(&cfg);
  cfg.max_frame_n = 1000;
  OK(sgtd_create(&cfg, &g_h));
  Model M;
  int64_t n64 = 0;

  // ---- before anything has run
  REQUIRE(sgtd_result_stored_voxel_registered(g_h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SGTD_ERR_STATE);
  REQUIRE(sgtd_result_stored_voxel_map(g_h, 0, nullptr, nullptr, nullptr, nullptr, 0, &n64) == SGTD_ERR_STATE);
  REQUIRE(sgtd_result_stored_voxel_matches(g_h, 0, nullptr, 0, &n64) == SGTD_ERR_STATE);
  REQUIRE(sgtd_stored_voxel_register_stage_ms(g_h, nullptr, nullptr, nullptr, nullptr, nullptr) == SGTD_ERR_STATE);
  // a store without a frame: a call with no member is a run
  stored_voxel_call(M, Call{{3}, {{}}, {0}, {0}}, 3, false, false);

  // ---- a store with dead slots: overwritten and forgotten frames lie between the members
  M.set({3, 7, 9, 12}, {10, 0, 30, 6}, 1);
  M.set({7}, {50}, 6);             // larger: the arena grows, slot 1 dies
  M.set({9, 20}, {4, 17}, 8);      // slot of 9 dies
  M.forget({12});
  const Call mixed{{5, 0, 130, 2},
                   {{3}, {9, 7}, {}, {20, 3, 20, 7}, {7, 7}},      // one frame, two, none, a frame twice, a frame in several maps
                   {0, 2, 1, 2, 0, 0, 3},
                   {0, 3, 1, 1, 2, 4, 3}};
  stored_voxel_call(M, mixed, 3, false, false);
  stored_voxel_call(M, mixed, 4, true, true);
  // ---- a tail larger than the arena: it grows inside the call, the slots are renumbered behind the members' lookup
  const int before = g_compactions;
  stored_voxel_call(M, Call{{9000, 4}, {{20, 9}, {3}}, {0, 1, 1}, {0, 1, 0}}, 4, false, true);
  REQUIRE(g_compactions > before);
  stored_voxel_call(M, mixed, 3, false, false);
  // no pair is a run (the maps are built), and so is no map
  stored_voxel_call(M, Call{{3}, {{7}, {3, 9}}, {}, {}}, 3, false, false);
  stored_voxel_call(M, Call{{3}, {}, {}, {}}, 3, false, false);

  // ---- the error paths: the earlier results are kept
  {
    const Call kept{{6, 7}, {{20}, {3, 7}}, {1, 0}, {0, 1}};
    stored_voxel_call(M, kept, 3, false, false);
    const std::vector<float> pts = cloud(90, 10);
    const int64_t off[3] = {0, 4, 10}, off_first[3] = {1, 4, 10}, off_down[3] = {0, 6, 4}, off_big[2] = {0, (1 << 17) + 1};
    const int32_t map_off[3] = {0, 1, 3}, map_off_first[3] = {1, 1, 3}, map_off_down[3] = {0, 2, 1};
    const uint32_t map_frame[3] = {20, 3, 7}, map_none[3] = {20, 12, 7}, map_far[3] = {20, 3, 4000000000u};
    const int32_t src[2] = {0, 1}, src_bad[2] = {0, 2}, tgt[2] = {1, 0}, tgt_bad[2] = {1, 2}, neg[2] = {-1, 0};
    const sgtd_voxel_register_options o = M.options();
    auto call = [&](const sgtd_voxel_register_options *opt, const float *p, int stride, const int64_t *po, int nc, const int32_t *mo, const uint32_t *mf,
                    const double *mp, int nm, const int32_t *s, const int32_t *t, const double *init, int n) {
      return sgtd_register_stored_voxels(g_h, opt, p, stride, po, nc, mo, mf, mp, nm, s, t, init, n, 0);
    };
    REQUIRE(call(&o, pts.data(), 3, off, 2, map_off, map_frame, nullptr, 2, src, tgt, nullptr, -1) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, off, 2, map_off, map_frame, nullptr, -1, src, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, off, -1, map_off, map_frame, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, off, 2, map_off, map_frame, nullptr, 2, nullptr, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, off, 2, map_off, map_frame, nullptr, 2, src, nullptr, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, off, 2, nullptr, map_frame, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, off, 2, map_off, nullptr, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, nullptr, 3, off, 2, map_off, map_frame, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, nullptr, 2, map_off, map_frame, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    for (int stride : {2, 5}) REQUIRE(call(&o, pts.data(), stride, off, 2, map_off, map_frame, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, off_first, 2, map_off, map_frame, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, off_down, 2, map_off, map_frame, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, off, 2, map_off_first, map_frame, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, off, 2, map_off_down, map_frame, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, off, 2, map_off, map_frame, nullptr, 2, src_bad, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, off, 2, map_off, map_frame, nullptr, 2, neg, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, off, 2, map_off, map_frame, nullptr, 2, src, tgt_bad, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, off, 2, map_off, map_frame, nullptr, 2, src, neg, nullptr, 2) == SGTD_ERR_INVALID);
    std::vector<double> poses(36, 0.0);
    poses[17] = (double)NAN;
    REQUIRE(call(&o, pts.data(), 3, off, 2, map_off, map_frame, poses.data(), 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    REQUIRE(call(&o, pts.data(), 3, off, 2, map_off, map_frame, nullptr, 2, src, tgt, poses.data(), 2) == SGTD_ERR_INVALID);
    // a member without a stored cloud: a forgotten frame, an id beyond the table
    REQUIRE(call(&o, pts.data(), 3, off, 2, map_off, map_none, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID && strstr(sgtd_last_error(g_h), "frame 12 "));
    REQUIRE(call(&o, pts.data(), 3, off, 2, map_off, map_far, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID && strstr(sgtd_last_error(g_h), "frame 4000000000 "));
    // the options, and the store's settings
    sgtd_voxel_register_options other = o;
    other.neighbor_mode = 6;
    REQUIRE(call(&other, pts.data(), 3, off, 2, map_off, map_frame, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    other = o; other.voxel_resolution = 0.0;
    REQUIRE(call(&other, pts.data(), 3, off, 2, map_off, map_frame, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    other = o; other.max_iterations = 0;
    REQUIRE(call(&other, pts.data(), 3, off, 2, map_off, map_frame, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_INVALID);
    other = o; other.k_neighbors = M.k + 1;
    REQUIRE(call(&other, pts.data(), 3, off, 2, map_off, map_frame, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_STATE);
    other = o; other.plane_eps = 0.5;
    REQUIRE(call(&other, pts.data(), 3, off, 2, map_off, map_frame, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_STATE);
    REQUIRE(call(nullptr, pts.data(), 3, off, 2, map_off, map_frame, nullptr, 2, src, tgt, nullptr, 2) == SGTD_ERR_STATE);      // (k_neighbors 20)
    // the caps, from the offsets and counts alone
    REQUIRE(call(&o, pts.data(), 3, off_big, 1, map_off, map_frame, nullptr, 2, src, tgt, nullptr, 1) == SGTD_ERR_UNSUPPORTED && strstr(sgtd_last_error(g_h), "points a cloud"));
    {
      const std::vector<int32_t> many(SGTD_VREG_MAX_MAPS + 2, 0);
      REQUIRE(call(&o, pts.data(), 3, off, 2, many.data(), map_frame, nullptr, SGTD_VREG_MAX_MAPS + 1, src, tgt, nullptr, 2) == SGTD_ERR_UNSUPPORTED &&
              strstr(sgtd_last_error(g_h), "SGTD_VREG_MAX_MAPS"));
      const int n_mem = SGTD_VREG_MAX_MEMBER_POINTS / 50 + 1;      // (frame 7 holds 50 points)
      const std::vector<uint32_t> members((size_t)n_mem, 7u);
      const int32_t one_map[2] = {0, n_mem};
      REQUIRE(call(&o, pts.data(), 3, off, 2, one_map, members.data(), nullptr, 1, src, neg + 1, nullptr, 1) == SGTD_ERR_UNSUPPORTED &&
              strstr(sgtd_last_error(g_h), "SGTD_VREG_MAX_MEMBER_POINTS"));
      const int64_t full[2] = {0, 1 << 17};
      const int n_src = SGTD_VREG_MAX_CORR / 27 / (1 << 17) + 1;
      const std::vector<int32_t> zeros((size_t)n_src, 0);
      other = o; other.neighbor_mode = 27;
      REQUIRE(call(&other, pts.data(), 3, full, 1, map_off, map_frame, nullptr, 2, zeros.data(), zeros.data(), nullptr, n_src) == SGTD_ERR_UNSUPPORTED &&
              strstr(sgtd_last_error(g_h), "SGTD_VREG_MAX_CORR"));
    }
    verify_results(M, kept);
    // the loops form: its argument errors, no verified batch, and its getters after the explicit form
    REQUIRE(sgtd_register_stored_local_loops(g_h, &o, pts.data(), 3, off, -1, SGTD_START_VERIFY, 5.0, 0, 0) == SGTD_ERR_INVALID);
    for (int start : {-1, 3}) REQUIRE(sgtd_register_stored_local_loops(g_h, &o, pts.data(), 3, off, 4, start, 5.0, 0, 0) == SGTD_ERR_INVALID);
    for (double radius : {-1.0, (double)NAN, (double)INFINITY})
      REQUIRE(sgtd_register_stored_local_loops(g_h, &o, pts.data(), 3, off, 4, SGTD_START_VERIFY, radius, 0, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_register_stored_local_loops(g_h, &o, pts.data(), 3, off, 4, SGTD_START_VERIFY, 5.0, -1, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_register_stored_local_loops(g_h, &o, pts.data(), 2, off, 4, SGTD_START_VERIFY, 5.0, 0, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_register_stored_local_loops(g_h, &o, pts.data(), 3, nullptr, 4, SGTD_START_VERIFY, 5.0, 0, 0) == SGTD_ERR_INVALID);
    other = o; other.neighbor_mode = 5;
    REQUIRE(sgtd_register_stored_local_loops(g_h, &other, pts.data(), 3, off, 4, SGTD_START_VERIFY, 5.0, 0, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_register_stored_local_loops(g_h, &o, pts.data(), 3, off, 4, SGTD_START_VERIFY, 5.0, 0, 0) == SGTD_ERR_STATE && strstr(sgtd_last_error(g_h), "sgtd_verify"));
    REQUIRE(sgtd_result_stored_local_pairs(g_h, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &n64) == SGTD_ERR_STATE);
    REQUIRE(sgtd_result_stored_local_maps(g_h, nullptr, nullptr, nullptr, nullptr, 0, 0, &n64, &n64) == SGTD_ERR_STATE);
    REQUIRE(sgtd_result_stored_local_pairs(g_h, nullptr, nullptr, nullptr, nullptr, nullptr, -1, &n64) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_result_stored_local_maps(g_h, nullptr, nullptr, nullptr, nullptr, -1, 0, &n64, &n64) == SGTD_ERR_INVALID);
    verify_results(M, kept);
    // sgtd_register_stored's results and this call's do not touch each other
    sgtd_register_options d;
    sgtd_default_register_options(&d);
    d.k_neighbors = M.k;
    const uint32_t frame = 20;
    REQUIRE(sgtd_result_stored_registered(g_h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SGTD_ERR_STATE);
    OK(sgtd_register_stored(g_h, &d, pts.data(), 3, off, 2, src, &frame, nullptr, 1, 0));
    verify_results(M, kept);
    stored_voxel_call(M, mixed, 3, false, false);
    OK(sgtd_result_stored_registered(g_h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  }

  // ---- two "devices" behind one handle: the store and the call's results live on the first
  {
    const int devices[2] = {0, 0};
    sgtd_handle single = g_h, multi = nullptr;
    OK(sgtd_create_multi(&cfg, devices, 2, &multi));
    g_h = multi;
    Model G;
    G.set({4, 5}, {20, 70}, 100);
    stored_voxel_call(G, Call{{12, 3}, {{5, 4}, {4}}, {0, 0, 1}, {1, 0, 0}}, 3, false, true);
    const std::vector<float> pts = cloud(90, 10);
    const int64_t off[2] = {0, 10};
    REQUIRE(sgtd_register_stored_local_loops(g_h, nullptr, pts.data(), 3, off, 4, SGTD_START_VERIFY, 5.0, 0, 0) == SGTD_ERR_UNSUPPORTED &&
            strstr(sgtd_last_error(g_h), "multi-device"));
    OK(sgtd_destroy(multi));
    g_h = single;
    stored_voxel_call(M, mixed, 3, false, false);
  }

  // ---- forget all: a store with other settings works
  OK(sgtd_set_frame_clouds(g_h, nullptr, nullptr, nullptr, 3, 0, 0, 0.0, 0));
  M.clouds.clear();
  M.k = 9; M.eps = 0.01;
  M.set({0, 999}, {64, 65}, 120);
  stored_voxel_call(M, Call{{1}, {{999, 0}}, {0}, {0}}, 3, false, false);
  OK(sgtd_destroy(g_h));
  g_h = nullptr;
  REQUIRE(sgtd_stub_device_blocks() == 0);
  printf("stored voxel maps under the sanitizers: ok (%d compactions, %d covariances, %d member points)\n", g_compactions, g_cov_points, g_key_points);
  return 0;
}
