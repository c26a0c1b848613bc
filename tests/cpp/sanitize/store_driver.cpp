// store_driver.cpp — the cloud store's host bookkeeping (sgtd_set_frame_clouds, sgtd_register_stored, the error paths of
// sgtd_register_stored_loops: sgtd_accel.hip) under ASan + UBSan, against hip_stub.cpp.  "Device" memory is host memory there
// and no kernel runs, so the launch hook below does on the host what the store's own kernels would (store_pack_kernel,
// store_compact_kernel), leaves a covariance that names its point where reg_cov_kernel would have written one, ends the solves
// and writes result rows that name their target.  The driver keeps a model of the store (frame -> points) beside the handle and
// compares every frame's stored cloud with it after every step: set, overwrite (larger, smaller, empty), an id twice in a call,
// forget, growth and compaction from a first capacity of 64 points, a failed growth that must leave the store as it was, stored
// calls whose tail makes the arena grow, every argument error with the store and the earlier results intact, forget-all,
// destroy.  Every copy the engine makes is checked by the sanitizer against the real size of the allocation; at the end no
// device block is left.  Compiled for the host only; tests/test_store_sanitize.py builds and runs it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
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
#include "../../../sgtd_amd/csrc/cloud_store_kernels.hip.h"
}  // namespace kernels_of_the_engine
namespace K = kernels_of_the_engine;

extern "C" {
typedef void (*launch_hook_t)(const char *name, void **args, void *user);
void sgtd_stub_set_launch_hook(launch_hook_t h, void *user);
size_t sgtd_stub_device_bytes();
size_t sgtd_stub_device_blocks();
}

#define REQUIRE(x) do { if (!(x)) { fprintf(stderr, "store_driver: %s failed at line %d\n", #x, __LINE__); exit(1); } } while (0)
static sgtd_handle g_h = nullptr;
#define OK(call) do { const int st_ = (call); if (st_ != SGTD_OK) { fprintf(stderr, "store_driver: %s = %d at line %d (%s)\n", #call, st_, __LINE__, g_h ? sgtd_last_error(g_h) : ""); exit(1); } } while (0)

namespace {
int g_compactions = 0, g_packs = 0, g_cov_tiles = 0;

// `kernel` is the function the (mangled) name names
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
    g_packs++;
  } else if (names(name, "store_compact_kernel")) {
    const K::StoreMoveParams &P = *static_cast<const K::StoreMoveParams *>(args[0]);
    REQUIRE(P.to[P.n_live] == P.total);
    for (int s = 0; s < P.n_live; s++)
      for (long long g = P.to[s]; g < P.to[s + 1]; g++) {
        const long long f = P.from[s] + (g - P.to[s]);
        for (int a = 0; a < 3; a++) P.pts_out[g * 3 + a] = P.pts_in[f * 3 + a];
        for (int a = 0; a < 9; a++) P.cov_out[g * 9 + a] = P.cov_in[f * 9 + a];
      }
    g_compactions++;
  } else if (names(name, "reg_cov_kernel")) {
    // a covariance that names its point and the settings
    const K::RegParams &P = *static_cast<const K::RegParams *>(args[0]);
    for (int b = 0; b < P.n_ctiles; b++) {
      const long long base = P.pt_off[P.ctile_cloud[b]], n = P.pt_off[P.ctile_cloud[b] + 1] - base;
      REQUIRE(P.ctile_first[b] < n);
      for (long long i = P.ctile_first[b]; i < std::min<long long>(n, P.ctile_first[b] + 128); i++) {
        double *c = P.cov + (base + i) * 9;
        for (int a = 0; a < 3; a++) c[a] = (double)P.pts[(base + i) * P.stride + a];
        c[3] = (double)P.o.k; c[4] = P.o.plane_eps;
      }
    }
    g_cov_tiles += P.n_ctiles;
  } else if (names(name, "reg_trial_kernel")) {
    *static_cast<const K::RegParams *>(args[0])->unfinished = 0;
  } else if (names(name, "reg_final_kernel")) {
    // a row that names its source's and its target's first point, and their sizes
    const K::RegParams &P = *static_cast<const K::RegParams *>(args[0]);
    for (int k = 0; k < P.n_pairs; k++) {
      const long long s0 = P.pt_off[P.src[k]], ns = P.pt_off[P.src[k] + 1] - s0, t0 = P.pt_off[P.tgt[k]], nt = P.pt_off[P.tgt[k] + 1] - t0;
      P.out_pose[(size_t)k * 12] = ns ? (double)P.pts[s0 * 3] : -1.0;
      P.out_pose[(size_t)k * 12 + 1] = nt ? (double)P.pts[t0 * 3] : -1.0;
      P.out_pose[(size_t)k * 12 + 2] = nt ? P.cov[t0 * 9 + 1] : -1.0;      // (the target's covariance came with it)
      P.out_matched[k] = (int)ns; P.out_iters[k] = (int)nt; P.out_status[k] = k;
    }
  }
}

// a cloud of n points of `stride` floats whose coordinates name (tag, point, axis); the fourth float must never be read
std::vector<float> cloud(int tag, int n, int stride = 3) {
  std::vector<float> v((size_t)n * stride, 1e30f);
  for (int i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) v[(size_t)i * stride + a] = (float)(tag * 1000 + i) + 0.25f * a;
  return v;
}

struct Model {
  std::map<uint32_t, std::vector<float>> clouds;      // frame -> x y z per point
  int k = 5;
  double eps = 1e-3;

  void verify() const {
    int64_t nf = 0, np = 0, bytes = 0;
    int32_t k_ = 0;
    double eps_ = 0.0;
    OK(sgtd_frame_clouds_info(g_h, &nf, &np, &bytes, &k_, &eps_));
    size_t pts = 0;
    for (const auto &c : clouds) pts += c.second.size() / 3;
    REQUIRE(nf == (int64_t)clouds.size() && np == (int64_t)pts && bytes >= (int64_t)pts * 84);
    for (uint32_t f = 0; f < 1000; f++) {
      int64_t n = 0;
      OK(sgtd_result_frame_cloud(g_h, f, nullptr, nullptr, 0, &n));
      const auto it = clouds.find(f);
      if (it == clouds.end()) { REQUIRE(n == -1); continue; }
      REQUIRE(n == (int64_t)it->second.size() / 3);
      std::vector<float> xyz((size_t)n * 3 + 1, -5.f);
      std::vector<double> cov((size_t)n * 9 + 1, -5.0);
      OK(sgtd_result_frame_cloud(g_h, f, xyz.data(), cov.data(), n, &n));
      REQUIRE(std::equal(it->second.begin(), it->second.end(), xyz.begin()) && xyz.back() == -5.f && cov.back() == -5.0);
      for (int64_t i = 0; i < n; i++) {
        for (int a = 0; a < 3; a++) REQUIRE(cov[(size_t)i * 9 + a] == (double)xyz[(size_t)i * 3 + a]);
        REQUIRE(cov[(size_t)i * 9 + 3] == (double)k && cov[(size_t)i * 9 + 4] == eps);
      }
      if (n > 1) {      // one short: the count still reported, the first entries written
        int64_t m = 0;
        std::vector<float> part((size_t)n * 3, -5.f);
        REQUIRE(sgtd_result_frame_cloud(g_h, f, part.data(), nullptr, n - 1, &m) == SGTD_ERR_CAPACITY && m == n);
        REQUIRE(std::equal(part.begin(), part.end() - 3, xyz.begin()) && part[(size_t)n * 3 - 1] == -5.f);
      }
    }
  }

  // one set call: frames, their sizes (tag = a number that makes the coordinates this call's), stride, host or "device" points
  void set(const std::vector<uint32_t> &frames, const std::vector<int> &sizes, int tag, int stride = 3, bool device = false) {
    std::vector<int64_t> off(1, 0);
    std::vector<float> pts;
    for (size_t i = 0; i < frames.size(); i++) {
      const std::vector<float> c = cloud(tag + (int)i, sizes[i], stride);
      pts.insert(pts.end(), c.begin(), c.end());
      off.push_back(off.back() + sizes[i]);
      std::vector<float> &m = clouds[frames[i]];
      m.clear();
      for (int p = 0; p < sizes[i]; p++) m.insert(m.end(), c.begin() + (size_t)p * stride, c.begin() + (size_t)p * stride + 3);
    }
    if (pts.empty()) pts.assign(4, 0.f);      // (a non-NULL array: NULL forgets)
    float *arg = pts.data();
    void *dev = nullptr;
    if (device) {
      REQUIRE(hipMalloc(&dev, pts.size() * sizeof(float)) == hipSuccess);
      memcpy(dev, pts.data(), pts.size() * sizeof(float));
      arg = static_cast<float *>(dev);
    }
    OK(sgtd_set_frame_clouds(g_h, frames.data(), off.data(), arg, stride, (int64_t)frames.size(), k, eps, device ? 1 : 0));
    if (dev) REQUIRE(hipFree(dev) == hipSuccess);
    verify();
  }

  void forget(const std::vector<uint32_t> &frames) {
    OK(sgtd_set_frame_clouds(g_h, frames.data(), nullptr, nullptr, 3, (int64_t)frames.size(), 0, 0.0, 0));
    for (uint32_t f : frames) clouds.erase(f);
    verify();
  }
};

// a stored call of `sizes.size()` clouds whose pair k registers cloud src[k] onto frame tgt[k]; the rows name what they saw
void stored_call(const Model &M, const std::vector<int> &sizes, const std::vector<int32_t> &src, const std::vector<uint32_t> &tgt, int stride, bool device) {
  std::vector<int64_t> off(1, 0);
  std::vector<float> pts;
  for (size_t i = 0; i < sizes.size(); i++) {
    const std::vector<float> c = cloud(500 + (int)i, sizes[i], stride);
    pts.insert(pts.end(), c.begin(), c.end());
    off.push_back(off.back() + sizes[i]);
  }
  if (pts.empty()) pts.assign(4, 0.f);
  float *arg = pts.data();
  void *dev = nullptr;
  if (device) {
    REQUIRE(hipMalloc(&dev, pts.size() * sizeof(float)) == hipSuccess);
    memcpy(dev, pts.data(), pts.size() * sizeof(float));
    arg = static_cast<float *>(dev);
  }
  sgtd_register_options o;
  sgtd_default_register_options(&o);
  o.k_neighbors = M.k; o.plane_eps = M.eps;
  const int n = (int)src.size();
  OK(sgtd_register_stored(g_h, &o, arg, stride, off.data(), (int)sizes.size(), src.data(), tgt.data(), nullptr, n, device ? 1 : 0));
  if (dev) REQUIRE(hipFree(dev) == hipSuccess);
  std::vector<double> pose((size_t)n * 12 + 1, -5.0), fit((size_t)n + 1), cost((size_t)n * 2 + 1);
  std::vector<int32_t> matched((size_t)n + 1), iters((size_t)n + 1), status((size_t)n + 1);
  OK(sgtd_result_stored_registered(g_h, pose.data(), fit.data(), cost.data(), matched.data(), iters.data(), status.data()));
  for (int k = 0; k < n; k++) {
    const std::vector<float> &t = M.clouds.at(tgt[(size_t)k]);
    REQUIRE(matched[(size_t)k] == sizes[(size_t)src[(size_t)k]] && iters[(size_t)k] == (int)t.size() / 3 && status[(size_t)k] == k);
    REQUIRE(pose[(size_t)k * 12] == (sizes[(size_t)src[(size_t)k]] ? (double)((500 + src[(size_t)k]) * 1000) : -1.0));
    REQUIRE(pose[(size_t)k * 12 + 1] == (t.empty() ? -1.0 : (double)t[0]) && pose[(size_t)k * 12 + 2] == (t.empty() ? -1.0 : (double)t[1]));
  }
  // the call's covariances: of the clouds some pair names, from the copy outside the arena
  std::vector<unsigned char> named(sizes.size(), 0);
  for (int32_t s : src) named[(size_t)s] = 1;
  for (size_t c = 0; c < sizes.size(); c++) {
    int64_t m = -1;
    OK(sgtd_result_stored_covariances(g_h, (int)c, nullptr, 0, &m));
    REQUIRE(m == (named[c] ? sizes[c] : 0));
    std::vector<double> cov((size_t)m * 9 + 1, -5.0);
    OK(sgtd_result_stored_covariances(g_h, (int)c, cov.data(), m, &m));
    for (int64_t i = 0; i < m; i++) REQUIRE(cov[(size_t)i * 9] == (double)((500 + (int)c) * 1000 + i) && cov[(size_t)i * 9 + 3] == (double)M.k);
    REQUIRE(cov.back() == -5.0);
  }
  for (int k = 0; k < n; k++) {
    int64_t m = -1;
    OK(sgtd_result_stored_matches(g_h, k, nullptr, nullptr, 0, &m));
    REQUIRE(m == sizes[(size_t)src[(size_t)k]]);
    std::vector<int32_t> j((size_t)m + 1, -7);
    std::vector<double> d2((size_t)m + 1, -7.0);
    OK(sgtd_result_stored_matches(g_h, k, j.data(), d2.data(), m, &m));
    REQUIRE(j.back() == -7 && d2.back() == -7.0);
  }
  int64_t m = 0;
  REQUIRE(sgtd_result_stored_pairs(g_h, nullptr, nullptr, nullptr, nullptr, 0, &m) == SGTD_ERR_STATE);
  REQUIRE(sgtd_result_stored_matches(g_h, n, nullptr, nullptr, 0, &m) == SGTD_ERR_INVALID);
  REQUIRE(sgtd_result_stored_covariances(g_h, (int)sizes.size(), nullptr, 0, &m) == SGTD_ERR_INVALID);
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
  int64_t bytes0 = -1, bytes = 0, n64 = 0;

  // ---- before anything is stored
  M.verify();
  OK(sgtd_frame_clouds_info(g_h, nullptr, nullptr, &bytes0, nullptr, nullptr));
  REQUIRE(bytes0 == 0);
  REQUIRE(sgtd_result_stored_registered(g_h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SGTD_ERR_STATE);
  REQUIRE(sgtd_result_stored_covariances(g_h, 0, nullptr, 0, &n64) == SGTD_ERR_STATE && sgtd_result_stored_matches(g_h, 0, nullptr, nullptr, 0, &n64) == SGTD_ERR_STATE);
  REQUIRE(sgtd_stored_register_stage_ms(g_h, nullptr, nullptr, nullptr, nullptr) == SGTD_ERR_STATE);
  M.forget({3, 4});      // (nothing to forget is fine)

  // ---- set, overwrite, forget; growth and compaction from 64 points
  M.set({3, 7, 9}, {10, 0, 30}, 1);
  OK(sgtd_frame_clouds_info(g_h, nullptr, nullptr, &bytes0, nullptr, nullptr));
  REQUIRE(g_compactions == 0 && bytes0 > 0);
  M.set({7}, {50}, 2);                       // larger: the arena grows (the live slots move to new arrays)
  OK(sgtd_frame_clouds_info(g_h, nullptr, nullptr, &bytes, nullptr, nullptr));
  REQUIRE(bytes > bytes0 && g_compactions == 1);
  M.set({7}, {5}, 3, 4);                     // smaller, stride 4
  M.set({7}, {0}, 4);                        // empty: the frame still has a cloud
  M.set({7, 12, 7}, {8, 3, 21}, 5, 4, true); // an id twice in a call: the last wins; "device" points
  M.forget({3, 100});                        // one that has a cloud, one that never had
  M.set({3}, {129}, 8);
  const int before = g_compactions;
  for (int r = 0; r < 12; r++) M.set({(uint32_t)(20 + r % 3), 9}, {40 + r, 17}, 10 + 2 * r, r % 2 ? 4 : 3, r % 3 == 0);
  REQUIRE(g_compactions > before);           // dead points outnumbered the live ones
  M.forget({20, 21, 22, 9, 12, 7});          // nearly everything dies: a compaction without growth
  M.set({1, 2}, {2, 3}, 40);

  // ---- a growth that fails leaves the store as it was
  {
    // 400 clouds of 2^17 points need more than the stand-in's 6 GB: the second of the new arrays cannot be had, and the
    // points ("device" memory) are never read
    std::vector<uint32_t> ids(400);
    std::vector<int64_t> off(401);
    for (int i = 0; i <= 400; i++) { off[(size_t)i] = (int64_t)i << 17; if (i < 400) ids[(size_t)i] = 100 + (uint32_t)i; }
    void *dev = nullptr;
    REQUIRE(hipMalloc(&dev, 64) == hipSuccess);
    const size_t blocks = sgtd_stub_device_blocks(), held = sgtd_stub_device_bytes();
    REQUIRE(sgtd_set_frame_clouds(g_h, ids.data(), off.data(), static_cast<float *>(dev), 3, 400, M.k, M.eps, 1) == SGTD_ERR_HIP);
    REQUIRE(strstr(sgtd_last_error(g_h), "cloud store") && sgtd_stub_device_blocks() == blocks && sgtd_stub_device_bytes() == held);
    REQUIRE(hipFree(dev) == hipSuccess);
    M.verify();
    M.set({2}, {5000}, 60);
  }

  // ---- the argument errors: the store stays as it is
  {
    const std::vector<float> pts = cloud(70, 10);
    const uint32_t ids[2] = {5, 6}, far_id = 1000;
    const int64_t off[3] = {0, 4, 10}, off_first[3] = {1, 4, 10}, off_down[3] = {0, 6, 4}, off_big[2] = {0, (1 << 17) + 1};
    REQUIRE(sgtd_set_frame_clouds(g_h, ids, off, pts.data(), 3, -1, M.k, M.eps, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_set_frame_clouds(g_h, nullptr, off, pts.data(), 3, 2, M.k, M.eps, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_set_frame_clouds(g_h, ids, nullptr, pts.data(), 3, 2, M.k, M.eps, 0) == SGTD_ERR_INVALID);
    for (int stride : {2, 5}) REQUIRE(sgtd_set_frame_clouds(g_h, ids, off, pts.data(), stride, 2, M.k, M.eps, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_set_frame_clouds(g_h, ids, off_first, pts.data(), 3, 2, M.k, M.eps, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_set_frame_clouds(g_h, ids, off_down, pts.data(), 3, 2, M.k, M.eps, 0) == SGTD_ERR_INVALID);
    for (int k : {2, 33}) REQUIRE(sgtd_set_frame_clouds(g_h, ids, off, pts.data(), 3, 2, k, M.eps, 0) == SGTD_ERR_INVALID);
    for (double eps : {0.0, -1.0, (double)NAN, (double)INFINITY}) REQUIRE(sgtd_set_frame_clouds(g_h, ids, off, pts.data(), 3, 2, M.k, eps, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_set_frame_clouds(g_h, &far_id, off, pts.data(), 3, 1, M.k, M.eps, 0) == SGTD_ERR_FRAME_LIMIT);
    REQUIRE(sgtd_set_frame_clouds(g_h, &far_id, nullptr, nullptr, 3, 1, 0, 0.0, 0) == SGTD_ERR_FRAME_LIMIT);
    REQUIRE(sgtd_set_frame_clouds(g_h, ids, off_big, pts.data(), 3, 1, M.k, M.eps, 0) == SGTD_ERR_UNSUPPORTED && strstr(sgtd_last_error(g_h), "points a cloud"));
    REQUIRE(sgtd_set_frame_clouds(g_h, ids, off, pts.data(), 3, 2, M.k + 1, M.eps, 0) == SGTD_ERR_STATE);
    REQUIRE(sgtd_set_frame_clouds(g_h, ids, off, pts.data(), 3, 2, M.k, 2 * M.eps, 0) == SGTD_ERR_STATE);
    OK(sgtd_set_frame_clouds(g_h, ids, off, pts.data(), 3, 0, M.k, M.eps, 0));      // (n == 0 with ids: nothing)
    REQUIRE(sgtd_result_frame_cloud(g_h, 1, nullptr, nullptr, -1, &n64) == SGTD_ERR_INVALID);
    M.verify();
  }

  // ---- stored calls: the tail behind the slots, on a store with dead slots and after a growth the tail itself causes
  M.set({30, 31, 32}, {130, 0, 600}, 80);
  stored_call(M, {5, 0, 130}, {0, 2, 1, 2, 0}, {30, 32, 30, 31, 1}, 3, false);
  stored_call(M, {9000, 4}, {0, 1}, {32, 2}, 4, true);      // (a tail larger than the arena: it grows, the slots are renumbered)
  M.verify();
  stored_call(M, {3}, {}, {}, 3, false);                    // no pair is a run
  {
    // what a failed call keeps: the results of the call before it
    stored_call(M, {6, 7}, {1, 0}, {30, 1}, 3, false);
    const std::vector<float> pts = cloud(90, 10);
    const int64_t off[3] = {0, 4, 10}, off_big[2] = {0, (1 << 17) + 1};
    const int32_t src[2] = {0, 1}, src_bad[2] = {0, 2};
    const uint32_t tgt[2] = {30, 1}, tgt_none[2] = {30, 33};
    sgtd_register_options o;
    sgtd_default_register_options(&o);
    o.k_neighbors = M.k;
    REQUIRE(sgtd_register_stored(g_h, &o, pts.data(), 3, off, 2, src, tgt, nullptr, -1, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_register_stored(g_h, &o, pts.data(), 3, off, 2, nullptr, tgt, nullptr, 2, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_register_stored(g_h, &o, pts.data(), 3, off, 2, src, nullptr, nullptr, 2, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_register_stored(g_h, &o, pts.data(), 3, off, 2, src_bad, tgt, nullptr, 2, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_register_stored(g_h, &o, nullptr, 3, off, 2, src, tgt, nullptr, 2, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_register_stored(g_h, &o, pts.data(), 6, off, 2, src, tgt, nullptr, 2, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_register_stored(g_h, &o, pts.data(), 3, off, 2, src, tgt_none, nullptr, 2, 0) == SGTD_ERR_INVALID && strstr(sgtd_last_error(g_h), "frame 33"));
    REQUIRE(sgtd_register_stored(g_h, &o, pts.data(), 3, off_big, 1, src, tgt, nullptr, 1, 0) == SGTD_ERR_UNSUPPORTED && strstr(sgtd_last_error(g_h), "points a cloud"));
    sgtd_register_options other = o;
    other.k_neighbors = M.k + 1;
    REQUIRE(sgtd_register_stored(g_h, &other, pts.data(), 3, off, 2, src, tgt, nullptr, 2, 0) == SGTD_ERR_STATE);
    other = o; other.plane_eps = 0.5;
    REQUIRE(sgtd_register_stored(g_h, &other, pts.data(), 3, off, 2, src, tgt, nullptr, 2, 0) == SGTD_ERR_STATE);
    other = o; other.max_iterations = 0;
    REQUIRE(sgtd_register_stored(g_h, &other, pts.data(), 3, off, 2, src, tgt, nullptr, 2, 0) == SGTD_ERR_INVALID);
    int32_t matched[2] = {0, 0};
    OK(sgtd_result_stored_registered(g_h, nullptr, nullptr, nullptr, matched, nullptr, nullptr));
    REQUIRE(matched[0] == 7 && matched[1] == 6);
    // the loops form without a verified batch, and its argument errors
    REQUIRE(sgtd_register_stored_loops(g_h, &o, pts.data(), 3, off, 4, SGTD_START_VERIFY, 0) == SGTD_ERR_STATE && strstr(sgtd_last_error(g_h), "sgtd_verify"));
    REQUIRE(sgtd_register_stored_loops(g_h, &o, pts.data(), 3, off, -1, SGTD_START_VERIFY, 0) == SGTD_ERR_INVALID);
    for (int start : {-1, 3}) REQUIRE(sgtd_register_stored_loops(g_h, &o, pts.data(), 3, off, 4, start, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_register_stored_loops(g_h, &o, pts.data(), 2, off, 4, SGTD_START_VERIFY, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_register_stored_loops(g_h, &o, pts.data(), 3, nullptr, 4, SGTD_START_VERIFY, 0) == SGTD_ERR_INVALID);
    REQUIRE(sgtd_register_stored_loops(g_h, &other, pts.data(), 3, off, 4, SGTD_START_VERIFY, 0) == SGTD_ERR_INVALID);
    OK(sgtd_result_stored_registered(g_h, nullptr, nullptr, nullptr, matched, nullptr, nullptr));
    REQUIRE(matched[0] == 7 && matched[1] == 6);
    M.verify();
  }

  // ---- two "devices" behind one handle: the store lives on the first
  {
    const int devices[2] = {0, 0};
    sgtd_handle single = g_h, multi = nullptr;
    OK(sgtd_create_multi(&cfg, devices, 2, &multi));
    g_h = multi;
    Model G;
    G.set({4, 5}, {20, 70}, 100);
    stored_call(G, {12}, {0, 0}, {5, 4}, 3, false);
    const std::vector<float> pts = cloud(90, 10);
    const int64_t off[2] = {0, 10};
    REQUIRE(sgtd_register_stored_loops(g_h, nullptr, pts.data(), 3, off, 4, SGTD_START_VERIFY, 0) == SGTD_ERR_UNSUPPORTED && strstr(sgtd_last_error(g_h), "multi-device"));
    OK(sgtd_destroy(multi));
    g_h = single;
    M.verify();
  }

  // ---- forget all: no frames, no device memory, no settings; a store with other settings works
  OK(sgtd_set_frame_clouds(g_h, nullptr, nullptr, nullptr, 3, 0, 0, 0.0, 0));
  M.clouds.clear();
  M.verify();
  int32_t k_now = -1;
  OK(sgtd_frame_clouds_info(g_h, nullptr, nullptr, &bytes, &k_now, nullptr));
  REQUIRE(bytes == 0 && k_now == 0);
  M.k = 9; M.eps = 0.01;
  M.set({0, 999}, {64, 65}, 120);
  stored_call(M, {1}, {0}, {999}, 3, false);
  OK(sgtd_destroy(g_h));
  g_h = nullptr;
  REQUIRE(sgtd_stub_device_blocks() == 0);
  printf("cloud store under the sanitizers: ok (%d packs, %d compactions, %d covariance tiles)\n", g_packs, g_compactions, g_cov_tiles);
  return 0;
}
