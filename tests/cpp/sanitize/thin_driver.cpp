// thin_driver.cpp — the host code of sgtd_thin_clouds and its getters (sgtd_accel.hip) under ASan + UBSan, against
// hip_stub.cpp.  "Device" memory is host memory there and no kernel runs, so the launch hook below does on the host what
// the call's kernels would if every finite point were a cell of its own and every other point were dropped
// (thin_keys_kernel: the drop counts; thin_offsets_kernel: out_off = the finite points before pt_off; thin_sum_kernel: the
// finite points as they are): enough for the call to size, fill and hand out its output, so that every copy the host
// code makes is checked by the sanitizer against the real size of the allocation.  Covered: the getters before a run,
// every argument error with the earlier results intact, both caps, an empty batch, empty clouds, host and "device"
// input, stride 3 and 4, a larger call after a smaller one, capacity one short, every output NULL, the timed form, a
// view, and one handle through a shrinking size, a batch with every point dropped (K = 0), a growing size, a change of
// stride and 256 clouds; destroy with no device block left.  Compiled for the host only, the way
// tests/test_store_sanitize.py builds store_driver.cpp; tests/test_thin_sanitize.py builds and runs it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <stdint.h>

#include "../../../include/sgtd_accel.h"

extern "C" {
typedef void (*launch_hook_t)(const char *name, void **args, void *user);
void sgtd_stub_set_launch_hook(launch_hook_t h, void *user);
size_t sgtd_stub_device_blocks();
}

#define REQUIRE(x) do { if (!(x)) { fprintf(stderr, "thin_driver: %s failed at line %d\n", #x, __LINE__); exit(1); } } while (0)
static sgtd_handle g_h = nullptr;
#define OK(call) do { const int st_ = (call); if (st_ != SGTD_OK) { fprintf(stderr, "thin_driver: %s = %d at line %d (%s)\n", #call, st_, __LINE__, g_h ? sgtd_last_error(g_h) : ""); exit(1); } } while (0)

namespace {
int g_sums = 0;
// the call being run, as thin_keys_kernel was handed it
const float *g_pts = nullptr;
const long long *g_off = nullptr;
int g_stride = 0, g_clouds = 0;

bool finite_point(const float *p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

// `kernel` is the function the (mangled) name names
bool names(const char *name, const char *kernel) {
  const char *at = strstr(name, kernel);
  return at && at > name && at[-1] >= '0' && at[-1] <= '9';
}

void hook(const char *name, void **args, void *) {
  if (names(name, "thin_keys_kernel")) {
    g_pts = *static_cast<const float **>(args[0]);
    g_stride = *static_cast<int *>(args[1]);
    g_off = *static_cast<const long long **>(args[2]);
    g_clouds = *static_cast<int *>(args[3]);
    int *dropped = *static_cast<int **>(args[10]);
    for (int s = 0; s < g_clouds; s++)
      for (long long i = g_off[s]; i < g_off[s + 1]; i++)
        if (!finite_point(g_pts + i * g_stride)) dropped[s * 2]++;
  } else if (names(name, "thin_offsets_kernel")) {
    const long long *pt_off = *static_cast<const long long **>(args[1]);
    const int n_clouds = *static_cast<int *>(args[2]);
    long long *out_off = *static_cast<long long **>(args[3]);
    REQUIRE(pt_off == g_off && n_clouds == g_clouds);
    long long kept = 0;
    for (int s = 0; s <= n_clouds; s++) {
      out_off[s] = kept;
      for (long long i = pt_off[s]; s < n_clouds && i < pt_off[s + 1]; i++) kept += finite_point(g_pts + i * g_stride);
    }
  } else if (names(name, "thin_sum_kernel")) {
    const float *pts = *static_cast<const float **>(args[0]);
    float *out = *static_cast<float **>(args[5]);
    const int stride = strstr(name, "Li4E") ? 4 : 3;
    REQUIRE(pts == g_pts && stride == g_stride);
    for (long long i = 0; i < g_off[g_clouds]; i++)
      if (finite_point(pts + i * stride)) {
        std::memcpy(out, pts + i * stride, stride * sizeof(float));
        out += stride;
      }
    g_sums++;
  }
}

std::vector<float> cloud(int tag, long long n, int stride) {
  std::vector<float> v((size_t)n * stride);
  for (size_t i = 0; i < v.size(); i++) v[i] = (float)(tag * 100000) + 0.5f * (float)i;
  return v;
}

// what the hook makes of a call: the finite points, their offsets, the drop counts
struct Want {
  std::vector<float> pts;
  std::vector<int64_t> off;
  std::vector<int32_t> dropped;
};

Want want_of(const std::vector<float> &pts, const std::vector<int64_t> &off, int stride) {
  Want w;
  const int S = (int)off.size() - 1;
  w.off.assign((size_t)S + 1, 0);
  w.dropped.assign((size_t)S * 2, 0);
  for (int s = 0; s < S; s++) {
    for (int64_t i = off[(size_t)s]; i < off[(size_t)s + 1]; i++) {
      const float *p = pts.data() + (size_t)i * stride;
      if (finite_point(p)) w.pts.insert(w.pts.end(), p, p + stride);
      else w.dropped[(size_t)s * 2]++;
    }
    w.off[(size_t)s + 1] = (int64_t)(w.pts.size() / (size_t)stride);
  }
  return w;
}

void expect(sgtd_handle h, const std::vector<float> &raw, const std::vector<int64_t> &raw_off, int stride) {
  const Want w = want_of(raw, raw_off, stride);
  const std::vector<float> &pts = w.pts;
  const std::vector<int64_t> &off = w.off;
  const int S = (int)off.size() - 1;
  int64_t n = -1;
  std::vector<int64_t> got_off((size_t)S + 1, -1);
  std::vector<int32_t> dropped((size_t)S * 2 + 1, -1);
  OK(sgtd_result_thinned(h, got_off.data(), nullptr, dropped.data(), 0, &n));
  REQUIRE(n == off.back() && got_off == off);
  for (int s = 0; s < S * 2; s++) REQUIRE(dropped[(size_t)s] == w.dropped[(size_t)s]);
  REQUIRE(dropped[(size_t)S * 2] == -1);
  std::vector<float> out((size_t)n * stride + 1, -7.f);
  OK(sgtd_result_thinned(h, nullptr, out.data(), nullptr, n, nullptr));
  REQUIRE((n == 0 || std::memcmp(out.data(), pts.data(), (size_t)n * stride * sizeof(float)) == 0) && out.back() == -7.f);
  if (n > 0) {
    std::fill(out.begin(), out.end(), -7.f);
    REQUIRE(sgtd_result_thinned(h, nullptr, out.data(), nullptr, n - 1, &n) == SGTD_ERR_CAPACITY && n == off.back());
    REQUIRE(std::memcmp(out.data(), pts.data(), (size_t)(n - 1) * stride * sizeof(float)) == 0 && out[(size_t)(n - 1) * stride] == -7.f);
  }
  const float *d = nullptr;
  int st = 0;
  int64_t m = -1;
  OK(sgtd_thinned_device_view(h, &d, &st, &m));
  REQUIRE(d && st == stride && m == n);
  REQUIRE(n == 0 || std::memcmp(d, pts.data(), (size_t)n * stride * sizeof(float)) == 0);
  OK(sgtd_thinned_device_view(h, nullptr, nullptr, nullptr));
  OK(sgtd_result_thinned(h, nullptr, nullptr, nullptr, 0, nullptr));
}
}  // namespace

int main() {
  sgtd_stub_set_launch_hook(hook, nullptr);
  sgtd_config cfg;
  sgtd_default_config(&cfg);
  sgtd_handle h = nullptr, view = nullptr;
  OK(sgtd_create(&cfg, &h));
  g_h = h;
  OK(sgtd_create(&cfg, &view));
  OK(sgtd_attach_table(view, h));
  int64_t n = 5;
  float ms[3] = {-1.f, -1.f, -1.f};
  // before a run
  for (sgtd_handle x : {h, view}) {
    REQUIRE(sgtd_result_thinned(x, nullptr, nullptr, nullptr, 0, &n) == SGTD_ERR_STATE && n == 5);
    REQUIRE(sgtd_thinned_device_view(x, nullptr, nullptr, &n) == SGTD_ERR_STATE);
    REQUIRE(sgtd_thin_stage_ms(x, ms, ms + 1, ms + 2) == SGTD_ERR_STATE);
  }
  // an empty batch, empty clouds
  const std::vector<int64_t> none = {0}, empties = {0, 0, 0};
  OK(sgtd_thin_clouds(h, nullptr, 3, none.data(), 0, 0.25, 0));
  expect(h, {}, none, 3);
  OK(sgtd_thin_clouds(h, nullptr, 4, empties.data(), 2, 0.25, 1));
  expect(h, {}, empties, 4);
  // host input, stride 3, then a larger call with stride 4 from "device" memory
  const std::vector<int64_t> off_a = {0, 40, 40, 41, 300};
  const std::vector<float> a = cloud(1, 300, 3);
  OK(sgtd_thin_clouds(h, a.data(), 3, off_a.data(), 4, 0.25, 0));
  expect(h, a, off_a, 3);
  const std::vector<int64_t> off_b = {0, 5000, 20000};
  const std::vector<float> b = cloud(2, 20000, 4);
  OK(sgtd_thin_clouds(h, b.data(), 4, off_b.data(), 2, 0.5, 1));
  expect(h, b, off_b, 4);
  // the argument errors and the caps keep these results
  const std::vector<int64_t> falls = {0, 300, 200}, from_one = {1, 200, 300};
  std::vector<int64_t> many((size_t)SGTD_REG_MAX_CLOUDS + 2, 0);
  const std::vector<int64_t> lots = {0, (int64_t)SGTD_SCAN_MAX_POINTS + 1};
  REQUIRE(sgtd_thin_clouds(nullptr, a.data(), 3, off_a.data(), 4, 0.25, 0) == SGTD_ERR_INVALID);
  REQUIRE(sgtd_thin_clouds(h, a.data(), 2, off_a.data(), 4, 0.25, 0) == SGTD_ERR_INVALID);
  REQUIRE(sgtd_thin_clouds(h, a.data(), 5, off_a.data(), 4, 0.25, 0) == SGTD_ERR_INVALID);
  REQUIRE(sgtd_thin_clouds(h, a.data(), 3, off_a.data(), -1, 0.25, 0) == SGTD_ERR_INVALID);
  REQUIRE(sgtd_thin_clouds(h, nullptr, 3, off_a.data(), 4, 0.25, 0) == SGTD_ERR_INVALID);
  REQUIRE(sgtd_thin_clouds(h, a.data(), 3, nullptr, 4, 0.25, 0) == SGTD_ERR_INVALID);
  REQUIRE(sgtd_thin_clouds(h, a.data(), 3, falls.data(), 2, 0.25, 0) == SGTD_ERR_INVALID);
  REQUIRE(sgtd_thin_clouds(h, a.data(), 3, from_one.data(), 2, 0.25, 0) == SGTD_ERR_INVALID);
  for (double leaf : {0.0, -1.0, (double)NAN, (double)INFINITY, -(double)INFINITY})
    REQUIRE(sgtd_thin_clouds(h, a.data(), 3, off_a.data(), 4, leaf, 0) == SGTD_ERR_INVALID);
  REQUIRE(sgtd_thin_clouds(h, a.data(), 3, many.data(), SGTD_REG_MAX_CLOUDS + 1, 0.25, 0) == SGTD_ERR_UNSUPPORTED);
  REQUIRE(sgtd_thin_clouds(h, a.data(), 3, lots.data(), 1, 0.25, 0) == SGTD_ERR_UNSUPPORTED);
  REQUIRE(sgtd_result_thinned(h, nullptr, nullptr, nullptr, -1, &n) == SGTD_ERR_INVALID);
  expect(h, b, off_b, 4);
  // timed; a smaller call after the larger one; the view's own results
  OK(sgtd_set_timing(h, 1));
  OK(sgtd_thin_clouds(h, a.data(), 3, off_a.data(), 4, 0.25, 0));
  OK(sgtd_thin_stage_ms(h, ms, ms + 1, ms + 2));
  OK(sgtd_thin_stage_ms(h, nullptr, nullptr, nullptr));
  OK(sgtd_set_timing(h, 0));
  expect(h, a, off_a, 3);
  g_h = view;
  OK(sgtd_thin_clouds(view, b.data(), 4, off_b.data(), 2, 0.5, 0));
  expect(view, b, off_b, 4);
  g_h = h;
  expect(h, a, off_a, 3);
  REQUIRE(g_sums == 4);
  // one handle, call after call: a small call after a large one, every point dropped (nothing kept: no sum runs), a
  // larger call than any before, another stride, 256 clouds
  const std::vector<int64_t> off_c = {0, 4, 10};
  const std::vector<float> c = cloud(3, 10, 3);
  OK(sgtd_thin_clouds(h, b.data(), 4, off_b.data(), 2, 0.5, 0));
  expect(h, b, off_b, 4);
  OK(sgtd_thin_clouds(h, c.data(), 3, off_c.data(), 2, 0.25, 0));
  expect(h, c, off_c, 3);
  const std::vector<int64_t> off_d = {0, 100, 100, 250};
  std::vector<float> d = cloud(4, 250, 3);
  for (size_t i = 0; i < 250; i++) d[i * 3 + i % 3] = i % 2 ? NAN : INFINITY;
  OK(sgtd_thin_clouds(h, d.data(), 3, off_d.data(), 3, 0.25, 0));
  expect(h, d, off_d, 3);
  REQUIRE(g_sums == 6);
  OK(sgtd_result_thinned(h, nullptr, nullptr, nullptr, 0, &n));
  REQUIRE(n == 0);
  const std::vector<int64_t> off_e = {0, 1, 29999, 30000};
  std::vector<float> e = cloud(5, 30000, 3);
  e[0] = NAN;                                // the first point dropped
  e[(size_t)29999 * 3 + 2] = -INFINITY;      // and the last
  OK(sgtd_thin_clouds(h, e.data(), 3, off_e.data(), 3, 0.25, 1));
  expect(h, e, off_e, 3);
  std::vector<int64_t> off_f(257);
  for (size_t s = 0; s <= 256; s++) off_f[s] = (int64_t)(s * 3 - (s > 100 ? 3 : 0) + (s == 256 ? 3 : 0));      // cloud 100 empty, cloud 255 of six points
  std::vector<float> f = cloud(6, off_f[256], 4);
  for (int64_t i = 0; i < off_f[256]; i += 7) f[(size_t)i * 4 + 1] = NAN;
  f[(size_t)(off_f[256] - 1) * 4] = INFINITY;
  OK(sgtd_thin_clouds(h, f.data(), 4, off_f.data(), 256, 0.5, 0));
  expect(h, f, off_f, 4);
  REQUIRE(g_sums == 8);
  OK(sgtd_destroy(view));
  OK(sgtd_destroy(h));
  REQUIRE(sgtd_stub_device_blocks() == 0);
  printf("thin_clouds under the sanitizers: ok\n");
  return 0;
}
