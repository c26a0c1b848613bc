// localize.cpp — the reference node's main loop (src/sgtd/src/semantic_graph_localization.cpp:
// 376-458 map construction, 506-520 query loading, 567-646 + 716-745 query loop and metrics)
// on the C ABI alone: graph-JSON directories in, localization statistics out.  No ROS, no PCL,
// no GICP (enable_gicp = false); BASE2OUSTER = identity.
//
//   localize <map_dir | map.cache> <query_dir | query.cache> [batch=256] [icp_threshold=0.4] [prior_radius] [--refine N]
//   --refine N (anywhere on the line): sgtd_refine_poses(h, N) after the verification — the relative pose of SearchLoop's
//   choice refitted over all its inlier pairs — and a second set of error lines for the refined poses (off by default)
//   --overlap RADIUS [--min-overlap X] (anywhere on the line): the map's keypoints are stored on the handle
//   (sgtd_set_frame_keypoints), sgtd_overlap(h, RADIUS) runs after the verification and the detection is
//   sgtd_search_loop_overlap's — the best-scored candidate among those whose keypoint overlap reaches X (default 0.4) —
//   in place of sgtd_search_loop's; one more line counts what the gate accepted, rejected and moved (off by default)
//   --align RADIUS[,ITER] (anywhere on the line): the map's keypoints are stored on the handle, sgtd_align_keypoints(h,
//   RADIUS, ITER) (default 10 iterations; from the refined pose with --refine) runs after the verification, and one more
//   set of lines accounts sgtd_search_loop_aligned's choice (overlap_after >= 0.4, the lowest rms_after) with its aligned
//   world pose (off by default)
//   prior_radius: restrict every query to the map frames within that many metres (x, y) of its ground-truth position
//   (sgtd_set_frame_poses + sgtd_set_position_prior), as a localizer with odometry would, and report how many map
//   frames a query was allowed on average (the LOCALIZE_PER_FRAME calls below run without it)
//   LOCALIZE_DEFAULT_MALLOC=1: do not tune glibc's allocator (see main)
//   LOCALIZE_PER_FRAME=n: additionally run the first n queries the way the reference node does —
//   one BuildSingleScanSTD + SearchLoop call per frame through the STDescManager adapter
//   (semantic_graph_localization.cpp:590-601) — and report the time per frame
//
// Map frames take the sorted file order here (the reference uses the unsorted directory order,
// quirk 13: pass an explicit order if a run must be reproduced); queries are sorted (:386).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <malloc.h>
#include <string>
#include <vector>

#include "sgtd_accel.h"
#include "sgtd/STDescManager.hpp"

namespace fs = std::filesystem;

struct Mat4 {
  float m[4][4];
};
static Mat4 from_row(const float *p) {   // 12 floats, row-major 3x4 (:723-733)
  Mat4 r{};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) r.m[i][j] = p[i * 4 + j];
  r.m[3][3] = 1.f;
  return r;
}
static Mat4 mul(const Mat4 &a, const Mat4 &b) {
  Mat4 r{};
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      float s = 0;
      for (int k = 0; k < 4; k++) s += a.m[i][k] * b.m[k][j];
      r.m[i][j] = s;
    }
  return r;
}
static Mat4 rigid_inverse(const Mat4 &a) {   // poses are rigid: R^T, -R^T t
  Mat4 r{};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) r.m[i][j] = a.m[j][i];
  for (int i = 0; i < 3; i++) r.m[i][3] = -(r.m[i][0] * a.m[0][3] + r.m[i][1] * a.m[1][3] + r.m[i][2] * a.m[2][3]);
  r.m[3][3] = 1.f;
  return r;
}
// utility.hpp:109-123
static void compute_adj_rpe(const Mat4 &gt, const Mat4 &lo, double &t_e, double &r_e) {
  const Mat4 d = mul(rigid_inverse(lo), gt);
  t_e = std::sqrt((double)d.m[0][3] * d.m[0][3] + (double)d.m[1][3] * d.m[1][3] + (double)d.m[2][3] * d.m[2][3]);
  const double c = std::fmin(std::fmax(((double)d.m[0][0] + d.m[1][1] + d.m[2][2] - 1) / 2, -1.0), 1.0);
  r_e = std::fabs(std::acos(c)) / M_PI * 180;
}

static std::vector<std::string> list_json(const char *dir) {
  std::vector<std::string> v;
  if (!fs::is_directory(dir)) {
    std::fprintf(stderr, "not a directory: %s\n", dir);
    std::exit(2);
  }
  for (auto &e : fs::recursive_directory_iterator(dir))
    if (e.is_regular_file() && e.path().extension() == ".json") v.push_back(e.path().string());
  std::sort(v.begin(), v.end());
  return v;
}

#define OK(call)                                                                          \
  do {                                                                                    \
    const int st_ = (call);                                                               \
    if (st_ != SGTD_OK) {                                                                 \
      std::fprintf(stderr, "%s failed: %s\n", #call, sgtd_strerror(st_));                 \
      return 1;                                                                           \
    }                                                                                     \
  } while (0)

struct Graphs {
  sgtd_graph_batch *b = nullptr;
  int n = 0;
  const float *xyz = nullptr, *poses = nullptr;
  const uint32_t *label = nullptr;
  const int64_t *off = nullptr;
};
// a directory of graph-JSON files, or ONE graph-batch cache file (sgtd_graphs_save_cache, sgtd_amd/ingest.py write_cache)
static int load_any(const char *path, Graphs &g);
static int load(const std::vector<std::string> &files, Graphs &g) {
  std::vector<const char *> p;
  for (auto &s : files) p.push_back(s.c_str());
  const int st = sgtd_graphs_load(p.data(), (int)p.size(), 16, &g.b);
  if (st != SGTD_OK) {
    std::fprintf(stderr, "%s\n", sgtd_graphs_error(g.b));
    return st;
  }
  return sgtd_graphs_view(g.b, &g.n, nullptr, &g.xyz, &g.label, &g.off, &g.poses);
}

static int load_any(const char *path, Graphs &g) {
  if (fs::is_regular_file(path)) {
    const int st = sgtd_graphs_load_cache(path, &g.b);
    if (st != SGTD_OK) {
      std::fprintf(stderr, "%s\n", sgtd_graphs_error(g.b));
      return st;
    }
    return sgtd_graphs_view(g.b, &g.n, nullptr, &g.xyz, &g.label, &g.off, &g.poses);
  }
  return load(list_json(path), g);
}

int main(int argc, char **argv) {
  int refine = 0;                                            // --refine N, taken out of the positional arguments
  for (int i = 1; i < argc; i++)
    if (!std::strcmp(argv[i], "--refine")) {
      refine = i + 1 < argc ? std::atoi(argv[i + 1]) : 0;
      if (refine < 1) { std::fprintf(stderr, "--refine needs a number of iterations >= 1\n"); return 2; }
      for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
      argc -= 2;
      break;
    }
  double overlap_radius = -1.0, min_overlap = 0.4;           // --overlap RADIUS, --min-overlap X, taken out likewise
  bool min_overlap_given = false;
  for (int i = 1; i < argc;) {
    const bool ov = !std::strcmp(argv[i], "--overlap"), mo = !std::strcmp(argv[i], "--min-overlap");
    if (!ov && !mo) { i++; continue; }
    char *end = nullptr;
    const double v = i + 1 < argc ? std::strtod(argv[i + 1], &end) : -1.0;
    if (i + 1 >= argc || end == argv[i + 1] || *end || !(v >= 0.0) || std::isinf(v)) {
      std::fprintf(stderr, "%s needs a number >= 0\n", argv[i]);
      return 2;
    }
    if (ov) overlap_radius = v; else { min_overlap = v; min_overlap_given = true; }
    for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
    argc -= 2;
  }
  const bool use_overlap = overlap_radius >= 0.0;
  double align_radius = -1.0;                                // --align RADIUS[,ITER], taken out likewise
  int align_iter = 10;
  for (int i = 1; i < argc;) {
    if (std::strcmp(argv[i], "--align")) { i++; continue; }
    char *end = nullptr;
    const double v = i + 1 < argc ? std::strtod(argv[i + 1], &end) : -1.0;
    long it = 10;
    bool ok = i + 1 < argc && end != argv[i + 1] && v >= 0.0 && !std::isinf(v);
    if (ok && *end == ',') {
      char *e2 = nullptr;
      it = std::strtol(end + 1, &e2, 10);
      ok = e2 != end + 1 && !*e2 && it >= 1 && it <= 1000000;
    } else if (ok && *end) ok = false;
    if (!ok) { std::fprintf(stderr, "--align needs RADIUS[,ITER]: a number >= 0 and an iteration count >= 1\n"); return 2; }
    align_radius = v; align_iter = (int)it;
    for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
    argc -= 2;
  }
  const bool use_align = align_radius >= 0.0;
  if (min_overlap_given && !use_overlap) { std::fprintf(stderr, "--min-overlap comes with --overlap RADIUS\n"); return 2; }
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <map_dir | map.cache> <query_dir | query.cache> [batch] [icp_threshold] [prior_radius] [--refine N] "
                         "[--overlap RADIUS [--min-overlap X]] [--align RADIUS[,ITER]]\n", argv[0]);
    return 2;
  }
  // SearchLoop hands back ~130 MB of std::pair<STDesc, STDesc> per frame (the reference's own result
  // type): with glibc's defaults every one of those vectors is a fresh mmap — page faults on the way in,
  // munmap on the way out.  Keeping freed memory in the heap takes about a quarter off the per-frame
  // time (measured 25.1 -> 16.7 ms); the reference's node gets the same from the environment
  // (MALLOC_MMAP_THRESHOLD_=33554432 MALLOC_TRIM_THRESHOLD_=1073741824 MALLOC_TOP_PAD_=268435456).
  // LOCALIZE_DEFAULT_MALLOC=1 leaves the allocator alone.
  if (!std::getenv("LOCALIZE_DEFAULT_MALLOC")) {
    mallopt(M_MMAP_THRESHOLD, 32 << 20);
    mallopt(M_TRIM_THRESHOLD, 1 << 30);
    mallopt(M_TOP_PAD, 256 << 20);
  }
  const int batch = argc > 3 ? std::atoi(argv[3]) : 256;
  const double icp_threshold = argc > 4 ? std::atof(argv[4]) : 0.4;   // SG_localization.yaml:89
  const bool use_prior = argc > 5;
  const double prior_radius = use_prior ? std::atof(argv[5]) : 0.0;
  auto t0 = std::chrono::steady_clock::now();
  Graphs map, qs;
  OK(load_any(argv[1], map));
  OK(load_any(argv[2], qs));
  auto t1 = std::chrono::steady_clock::now();

  sgtd_config cfg;
  sgtd_default_config(&cfg);                                 // SG_localization.yaml:74-89
  if (map.n + 1 > cfg.max_frame_n) cfg.max_frame_n = map.n + 1;
  sgtd_handle h = nullptr;
  // SGTD_DEVICES=0,1,...: the table sharded over several GPUs of this node behind the one handle
  std::vector<int> devices;
  if (const char *dv = std::getenv("SGTD_DEVICES"))
    for (const char *p = dv; *p;) { devices.push_back(std::atoi(p)); while (*p && *p != ',') p++; if (*p == ',') p++; }
  if (devices.empty()) devices.push_back(0);
  OK(sgtd_create_multi(&cfg, devices.data(), (int)devices.size(), &h));
  OK(sgtd_add_frames(h, map.xyz, map.label, map.off, map.n, 0));   // :419-458
  OK(sgtd_finalize(h));
  if (use_prior) {                                           // map frame i has global id i (first_frame_id 0)
    std::vector<uint32_t> ids(map.n);
    for (int i = 0; i < map.n; i++) ids[i] = (uint32_t)i;
    OK(sgtd_set_frame_poses(h, ids.data(), map.poses, map.n));
  }
  if (use_overlap || use_align) {                            // the map's keypoints, under the ids the frames were added with
    std::vector<uint32_t> ids(map.n);
    for (int i = 0; i < map.n; i++) ids[i] = (uint32_t)i;
    OK(sgtd_set_frame_keypoints(h, ids.data(), map.off, map.xyz, map.label, map.n));
  }
  long ov_accepted = 0, ov_rejected = 0, ov_moved = 0;       // --overlap: the gated choice against sgtd_search_loop's
  double ov_sum = 0;
  std::vector<int32_t> plain_cand(batch), plain_frame(batch);
  std::vector<double> best_overlap(batch);
  long al_chosen = 0, al_moved = 0, al_score_num = 0;        // --align: sgtd_search_loop_aligned's choice, its aligned pose
  double al_err_t = 0, al_err_r = 0, al_rms_b = 0, al_rms_a = 0;
  std::vector<int32_t> al_cand(batch), al_frame(batch);
  std::vector<double> al_pose((size_t)cfg.candidate_num * 12), al_rb(cfg.candidate_num), al_ra(cfg.candidate_num);
  long allowed_sum = 0;                                      // (query, map frame) pairs the priors allowed
  std::vector<double> prior_c, prior_r;
  auto t2 = std::chrono::steady_clock::now();

  const int cn = cfg.candidate_num;
  long total_num = 0, detected = 0, score_num = 0, test_10 = 0;
  std::vector<long> STD_num(cn, 0);
  double err_t = 0, err_r = 0;
  long ref_score_num = 0;                                    // --refine: the same accounting with the refined poses
  double ref_err_t = 0, ref_err_r = 0, ref_rmse = 0, ver_rmse = 0;
  std::vector<double> ref_pose((size_t)cn * 12), ref_rmse_v(cn), ver_rmse_v(cn);
  std::vector<int32_t> n_cand(batch), cand_frame((size_t)batch * cn), best_cand(batch), best_frame(batch);
  std::vector<double> best_score(batch), score(cn), pose((size_t)cn * 12);
  for (int q0 = 0; q0 < qs.n; q0 += batch) {                 // :567-745, `batch` queries per call
    const int nb = std::min(batch, qs.n - q0);
    std::vector<int64_t> off(nb + 1);
    for (int i = 0; i <= nb; i++) off[i] = qs.off[q0 + i] - qs.off[q0];
    if (use_prior) {                                         // each query's ground-truth (x, y), one row per query
      prior_c.assign((size_t)nb * 2, 0.0);
      prior_r.assign(nb, prior_radius);
      for (int i = 0; i < nb; i++) {
        const float *qp = qs.poses + (size_t)(q0 + i) * 12;
        prior_c[(size_t)i * 2] = qp[3];
        prior_c[(size_t)i * 2 + 1] = qp[7];
        for (int f = 0; f < map.n; f++) {                    // (the rule of sgtd_set_position_prior, dims 2)
          const float *mp = map.poses + (size_t)f * 12;
          const double dx = (double)mp[3] - prior_c[(size_t)i * 2], dy = (double)mp[7] - prior_c[(size_t)i * 2 + 1];
          allowed_sum += std::isfinite(mp[3]) && std::isfinite(mp[7]) && dx * dx + dy * dy <= prior_radius * prior_radius;
        }
      }
      OK(sgtd_set_position_prior(h, prior_c.data(), prior_r.data(), nb, 2));
    }
    auto tb0 = std::chrono::steady_clock::now();
    OK(sgtd_query_frames(h, qs.xyz + 3 * qs.off[q0], qs.label + qs.off[q0], off.data(), nb, 0));
    OK(sgtd_sync(h));
    auto tb1 = std::chrono::steady_clock::now();
    OK(sgtd_verify(h));
    OK(sgtd_search_loop(h, icp_threshold, best_cand.data(), best_frame.data(), best_score.data()));
    OK(sgtd_result_candidates(h, n_cand.data(), cand_frame.data(), nullptr, nullptr));
    if (use_overlap) {
      plain_cand = best_cand; plain_frame = best_frame;
      OK(sgtd_overlap(h, overlap_radius, 0, nullptr, nullptr, nullptr));
      OK(sgtd_search_loop_overlap(h, icp_threshold, min_overlap, best_cand.data(), best_frame.data(), best_score.data(), best_overlap.data()));
      for (int i = 0; i < nb; i++) {
        if (best_frame[i] > 0) { ov_accepted++; ov_sum += best_overlap[i]; }
        if (plain_frame[i] > 0 && !(best_frame[i] > 0)) ov_rejected++;
        if (plain_frame[i] > 0 && best_frame[i] > 0 && plain_cand[i] != best_cand[i]) ov_moved++;
      }
    }
    if (refine) OK(sgtd_refine_poses(h, refine));
    if (use_align) {
      OK(sgtd_align_keypoints(h, align_radius, align_iter, refine ? SGTD_ALIGN_REFINED : 0, nullptr, nullptr, nullptr));
      OK(sgtd_search_loop_aligned(h, 0.4, 0.0, al_cand.data(), al_frame.data(), nullptr, nullptr));
      for (int i = 0; i < nb; i++) {
        if (!(al_frame[i] > 0)) continue;
        al_chosen++;
        if (al_cand[i] != best_cand[i]) al_moved++;
        OK(sgtd_result_aligned(h, i, al_pose.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, al_rb.data(), nullptr, al_ra.data(), nullptr));
        const double *r = &al_pose[(size_t)al_cand[i] * 12];
        Mat4 nt{};
        for (int a = 0; a < 3; a++) {
          for (int b = 0; b < 3; b++) nt.m[a][b] = (float)r[a * 3 + b];
          nt.m[a][3] = (float)r[9 + a];
        }
        nt.m[3][3] = 1.f;
        double te, re;
        compute_adj_rpe(from_row(qs.poses + (size_t)(q0 + i) * 12), mul(from_row(map.poses + (size_t)al_frame[i] * 12), nt), te, re);
        if (te < 5 && re < 10) { al_score_num++; al_err_t += te; al_err_r += re; }
        al_rms_b += al_rb[al_cand[i]]; al_rms_a += al_ra[al_cand[i]];
      }
    }
    auto tb2 = std::chrono::steady_clock::now();
    if (std::getenv("LOCALIZE_VERBOSE"))
      std::printf("  batch at %d: select %.1f ms, verify + choice %.1f ms\n", q0,
                  std::chrono::duration<double, std::milli>(tb1 - tb0).count(), std::chrono::duration<double, std::milli>(tb2 - tb1).count());
    for (int i = 0; i < nb; i++) {
      total_num++;
      if (!(best_frame[i] > 0)) continue;                    // search_result.first > 0 (:606-620)
      detected++;
      const Mat4 gt = from_row(qs.poses + (size_t)(q0 + i) * 12);
      OK(sgtd_result_verify(h, i, score.data(), pose.data()));
      std::vector<int> order(n_cand[i]);
      for (int k = 0; k < n_cand[i]; k++) order[k] = k;
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return (int)score[a] > (int)score[b]; });   // :12-14, int member
      for (int rank = 0; rank < n_cand[i]; rank++) {         // :621-645
        double te, re;
        compute_adj_rpe(gt, from_row(map.poses + (size_t)cand_frame[(size_t)i * cn + order[rank]] * 12), te, re);
        if (te < 10) { test_10++; STD_num[rank]++; break; }
      }
      Mat4 nt{};                                             // new_trans (:716-720)
      const double *p = &pose[(size_t)best_cand[i] * 12];
      for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) nt.m[a][b] = (float)p[a * 3 + b];
        nt.m[a][3] = (float)p[9 + a];
      }
      nt.m[3][3] = 1.f;
      double te, re;
      compute_adj_rpe(gt, mul(from_row(map.poses + (size_t)best_frame[i] * 12), nt), te, re);   // :733-735
      if (te < 5 && re < 10) { score_num++; err_t += te; err_r += re; }
      if (refine) {                                          // the refined pose of the same candidate in place of loop_transform
        OK(sgtd_result_refined(h, i, ref_pose.data(), ref_rmse_v.data(), ver_rmse_v.data(), nullptr, nullptr));
        const double *r = &ref_pose[(size_t)best_cand[i] * 12];
        for (int a = 0; a < 3; a++) {
          for (int b = 0; b < 3; b++) nt.m[a][b] = (float)r[a * 3 + b];
          nt.m[a][3] = (float)r[9 + a];
        }
        compute_adj_rpe(gt, mul(from_row(map.poses + (size_t)best_frame[i] * 12), nt), te, re);
        if (te < 5 && re < 10) { ref_score_num++; ref_err_t += te; ref_err_r += re; }
        ref_rmse += ref_rmse_v[best_cand[i]];
        ver_rmse += ver_rmse_v[best_cand[i]];
      }
    }
  }
  auto t3 = std::chrono::steady_clock::now();
  auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  std::printf("map frames %d, queries %ld: loops %ld, success(5m,10deg) %ld (%.4f), candidate<10m %ld, top-1 hit %ld\n", map.n,
              total_num, detected, score_num, total_num ? (double)score_num / total_num : 0.0, test_10, STD_num[0]);
  if (use_prior)
    std::printf("position prior %.2f m: %.1f map frames allowed per query (%ld in all)\n", prior_radius,
                total_num ? (double)allowed_sum / total_num : 0.0, allowed_sum);
  std::printf("mean errors of the successes: %.4f m, %.4f deg\n", score_num ? err_t / score_num : 0.0, score_num ? err_r / score_num : 0.0);
  if (refine) {
    std::printf("refined poses (%d iteration%s): success(5m,10deg) %ld (%.4f)\n", refine, refine == 1 ? "" : "s", ref_score_num,
                total_num ? (double)ref_score_num / total_num : 0.0);
    std::printf("mean errors of the successes, refined: %.4f m, %.4f deg\n", ref_score_num ? ref_err_t / ref_score_num : 0.0,
                ref_score_num ? ref_err_r / ref_score_num : 0.0);
    std::printf("mean inlier rmse of the chosen candidates: %.4f m refined, %.4f m under the verification's pose\n",
                detected ? ref_rmse / detected : 0.0, detected ? ver_rmse / detected : 0.0);
  }
  if (use_overlap)
    std::printf("keypoint overlap (radius %.2f m, min %.2f): accepted %ld, rejected %ld, moved to another candidate %ld, mean overlap of the accepted %.4f\n",
                overlap_radius, min_overlap, ov_accepted, ov_rejected, ov_moved, ov_accepted ? ov_sum / ov_accepted : 0.0);
  if (use_align) {
    std::printf("keypoint alignment (radius %.2f m, %d iteration%s, overlap >= 0.40): chosen %ld, another candidate than SearchLoop's %ld, success(5m,10deg) %ld (%.4f)\n",
                align_radius, align_iter, align_iter == 1 ? "" : "s", al_chosen, al_moved, al_score_num, total_num ? (double)al_score_num / total_num : 0.0);
    std::printf("mean errors of the successes, aligned: %.4f m, %.4f deg; mean keypoint rms of the chosen %.4f m before, %.4f m after\n",
                al_score_num ? al_err_t / al_score_num : 0.0, al_score_num ? al_err_r / al_score_num : 0.0,
                al_chosen ? al_rms_b / al_chosen : 0.0, al_chosen ? al_rms_a / al_chosen : 0.0);
  }
  std::printf("time: load %.1f ms, map build %.1f ms, queries %.1f ms (%.3f ms per query incl. verification), %d device(s)\n", ms(t0, t1), ms(t1, t2),
              ms(t2, t3), total_num ? ms(t2, t3) / total_num : 0.0, sgtd_device_count(h));
  if (const char *pf = std::getenv("LOCALIZE_PER_FRAME")) {
    // the reference's own call pattern: one frame per call, host containers in and out
    const int n_pf = std::min(std::atoi(pf), qs.n);
    sgtd::ConfigSetting cs;
    cs.icp_threshold_ = icp_threshold;
    cs.max_frame_n_ = cfg.max_frame_n;
    cs.device_ids_ = devices;
    sgtd::STDescManager mgr(cs);
    OK(sgtd_add_frames(mgr.handle(), map.xyz, map.label, map.off, map.n, 0));   // the map, batched (the per-frame form is tests/cpp/test_manager.cpp)
    OK(sgtd_current_frame_id(mgr.handle(), &mgr.current_frame_id_));
    OK(sgtd_finalize(mgr.handle()));
    double ms_build = 0, ms_search = 0, ms_selector = 0, ms_best_only = 0;
    long same = 0, pairs = 0, list_pairs = 0, same_best = 0;
    std::vector<int32_t> bf(1);
    for (int i = 0; i < n_pf; i++) {
      std::vector<sgtd::PointXYZL> cloud;
      for (int64_t k = qs.off[i]; k < qs.off[i + 1]; k++) cloud.push_back({qs.xyz[3 * k], qs.xyz[3 * k + 1], qs.xyz[3 * k + 2], qs.label[k]});
      auto a = std::chrono::steady_clock::now();
      std::vector<sgtd::STDesc> stds;
      mgr.BuildSingleScanSTD(cloud, stds);                                  // :592
      auto b = std::chrono::steady_clock::now();
      std::pair<int, double> search_result(-1, 0);
      std::pair<sgtd::Vec3, sgtd::Mat3> loop_transform;
      std::vector<std::pair<sgtd::STDesc, sgtd::STDesc>> loop_std_pair;
      std::vector<sgtd::LOOP_RESULT> match_result_list;
      mgr.SearchLoop(stds, search_result, loop_transform, loop_std_pair, match_result_list);   // :601
      auto c = std::chrono::steady_clock::now();
      OK(mgr.last_status());
      ms_build += std::chrono::duration<double, std::milli>(b - a).count();
      ms_search += std::chrono::duration<double, std::milli>(c - b).count();
      // the batched run above must have chosen the same frame for this query
      std::vector<int64_t> off1 = {0, qs.off[i + 1] - qs.off[i]};
      OK(sgtd_query_frames(h, qs.xyz + 3 * qs.off[i], qs.label + qs.off[i], off1.data(), 1, 0));
      OK(sgtd_verify(h));
      OK(sgtd_search_loop(h, icp_threshold, nullptr, bf.data(), nullptr));
      same += bf[0] == search_result.first;
      pairs += (long)loop_std_pair.size();
      // the other drop-in: candidate_selector alone (:318-460), every match list as pair<STDesc, STDesc> — what a
      // node that keeps its own candidate_verify calls
      auto d0 = std::chrono::steady_clock::now();
      std::vector<sgtd::STDMatchList> candidate_matcher_vec;
      mgr.candidate_selector(stds, candidate_matcher_vec);
      auto d1 = std::chrono::steady_clock::now();
      OK(mgr.last_status());
      ms_selector += std::chrono::duration<double, std::milli>(d1 - d0).count();
      for (const auto &ml : candidate_matcher_vec) list_pairs += (long)ml.match_list_.size();
      // ... and SearchLoop with only the best candidate's loop_std_pair built (sgtd_shim::fill_policy() = 1: an opt-in
      // deviation, adapter/STDesc_shim.hpp): same choice, same list for the chosen frame
      {
        const sgtd_shim::SearchTiming keep = sgtd_shim::search_timing();     // (the by-part report below is the default policy's)
        sgtd_shim::fill_policy() = 1;
        auto e0 = std::chrono::steady_clock::now();
        std::vector<sgtd::STDesc> stds2;
        mgr.BuildSingleScanSTD(cloud, stds2);
        std::pair<int, double> r2(-1, 0);
        std::pair<sgtd::Vec3, sgtd::Mat3> t2;
        std::vector<std::pair<sgtd::STDesc, sgtd::STDesc>> lp2;
        std::vector<sgtd::LOOP_RESULT> mr2;
        mgr.SearchLoop(stds2, r2, t2, lp2, mr2);
        auto e1 = std::chrono::steady_clock::now();
        sgtd_shim::fill_policy() = 0;
        sgtd_shim::search_timing() = keep;
        OK(mgr.last_status());
        ms_best_only += std::chrono::duration<double, std::milli>(e1 - e0).count();
        same_best += r2.first == search_result.first && lp2.size() == loop_std_pair.size() && mr2.size() == match_result_list.size();
      }
    }
    std::printf("per-frame calls through STDescManager (%d frames): %.3f ms per frame = BuildSingleScanSTD %.3f + SearchLoop %.3f; "
                "%ld/%d agree with the batched run, %.1f inlier pairs per loop\n",
                n_pf, (ms_build + ms_search) / n_pf, ms_build / n_pf, ms_search / n_pf, same, n_pf, (double)pairs / n_pf);
    std::printf("candidate_selector alone: %.3f ms per frame for %.0f pairs in the match lists\n", ms_selector / n_pf, (double)list_pairs / n_pf);
    std::printf("with only the best candidate's loop_std_pair built (SGTD_SHIM_FILL=best): %.3f ms per frame; %ld/%d the same choice and list\n",
                ms_best_only / n_pf, same_best, n_pf);
    const sgtd_shim::SearchTiming &tm = sgtd_shim::search_timing();
    if (tm.calls)
      std::printf("SearchLoop by part (ms per frame): select %.3f, verify %.3f, inlier pairs and their entries %.3f, host fill of loop_std_pair %.3f\n",
                  tm.select / tm.calls, tm.verify / tm.calls, tm.inliers / tm.calls, tm.fill / tm.calls);
  }
  sgtd_destroy(h);
  sgtd_graphs_free(map.b);
  sgtd_graphs_free(qs.b);
  return 0;
}
