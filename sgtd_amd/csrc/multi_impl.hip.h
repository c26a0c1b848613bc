// multi_impl.hip.h — implementation of multi.hip.h, included at the end of sgtd_accel.hip: the
// single-device entry points are defined above it; every shard is an ordinary engine.
#pragma once
namespace multi {

static inline Group *G(sgtd_engine *e) { return e->grp; }

#define MCHK(call)                     \
  do {                                 \
    int _r = (call);                   \
    if (_r != SGTD_OK) {               \
      e->err = "device shard: " + std::string(sgtd_last_error(c)); \
      return _r;                       \
    }                                  \
  } while (0)

// as sgtd_accel.hip's two, for the group's own flags
static void stale_stages(Group *g) { g->refined = false; g->overlapped = false; g->aligned = false; }
static void new_results(Group *g, bool verified) { g->verified = verified; stale_stages(g); }

// A stage on a verified batch, on every owner: the state checks with the texts of the single-device entry points (`stage`:
// the entry point's name; refined_flag: the name of the flag that asks for the refit's poses, or NULL), the stage's
// results (*done) gone while the devices run
template <class Call>
static int fan_out(sgtd_engine *e, const char *stage, const char *refined_flag, bool *done, Call call) {
  Group *g = G(e);
  if (!g->batch_valid || !g->verified) return needs(e, stage, "sgtd_verify");
  if (refined_flag && !g->refined) return needs(e, refined_flag, "sgtd_refine_poses");
  *done = false;
  for (sgtd_engine *c : g->dev) MCHK(call(c));
  *done = true;
  return SGTD_OK;
}

// a stage's getter of query q on a group: the stage has run on the pending batch (`missing` says what has not), q is one
// of its queries
static int group_result_ready(sgtd_engine *e, int q, bool done, const char *missing) {
  Group *g = G(e);
  if (!g->batch_valid || !g->verified || !done) { e->err = missing; return SGTD_ERR_STATE; }
  return (q < 0 || q >= g->nq) ? SGTD_ERR_INVALID : SGTD_OK;
}

// Query q's merged candidates, each from the device that owns it: fetch(c, s) brings what owner s (the engine c) has for
// the query, once, before copy(s, ks, k) first copies from it: the owner's slot ks to the merged slot k
template <class Fetch, class Copy>
static int gather(sgtd_engine *e, int q, Fetch fetch, Copy copy) {
  Group *g = G(e);
  const int cn = e->cfg.candidate_num;
  std::vector<char> have((size_t)g->n, 0);
  for (int k = 0; k < g->n_cand[q]; k++) {
    const size_t i = (size_t)q * cn + k;
    const int s = g->owner[i];
    if (!have[(size_t)s]) {
      sgtd_engine *c = g->dev[s];
      MCHK(fetch(c, s));
      have[(size_t)s] = 1;
    }
    copy(s, g->owner_slot[i], k);
  }
  return SGTD_OK;
}

int create(const sgtd_config *cfg, const int *device_ids, int n_dev, sgtd_handle *out) {
  if (!cfg || !out || !device_ids || n_dev < 1 || n_dev > 64) return SGTD_ERR_INVALID;
  *out = nullptr;
  sgtd_engine *e = new sgtd_engine();
  e->cfg = *cfg;
  e->grp = new Group();
  Group *g = e->grp;
  g->n = n_dev;
  g->current_frame_id = cfg->first_frame_id;
  if (cfg->first_frame_id % (SGTD_SHARD_BLOCK * (u32)n_dev) != 0) { delete g; delete e; return SGTD_ERR_INVALID; }
  for (int s = 0; s < n_dev; s++) {
    sgtd_config c = *cfg;
    c.device_id = device_ids[s];
    c.first_frame_id = local_of(cfg->first_frame_id, n_dev);
    sgtd_handle h = nullptr;
    const int st = sgtd_create(&c, &h);
    if (st != SGTD_OK) {
      for (sgtd_engine *d : g->dev) sgtd_destroy(d);
      delete g; delete e;
      return st;
    }
    g->dev.push_back(h);
  }
  *out = e;
  return SGTD_OK;
}

int destroy(sgtd_engine *e) {
  for (sgtd_engine *d : G(e)->dev) sgtd_destroy(d);
  delete e->grp;
  delete e;
  return SGTD_OK;
}

// BuildSingleScanSTD of one frame: any device will do; stamped with the GLOBAL frame id
int build(sgtd_engine *e, const float *xyz, const uint32_t *label, int n, sgtd_desc_soa *out, int64_t capacity, int64_t *n_out) {
  if (!out || !n_out || n < 0 || (n > 0 && (!xyz || !label))) return SGTD_ERR_INVALID;
  Group *g = G(e);
  sgtd_engine *c = g->dev[shard_of(g->current_frame_id, g->n)];
  MCHK(sgtd_build(c, xyz, label, n, out, capacity, n_out));
  if (out->frame)
    for (int64_t i = 0; i < *n_out; i++) out->frame[i] = g->current_frame_id;
  return SGTD_OK;
}

// AddSTDescs: the frame goes to the owner of the current global id; descriptors must carry
// that id (what BuildSingleScanSTD stamped, STDesc.cpp:305) — it becomes the owner's local id
int add(sgtd_engine *e, const sgtd_desc_soa *d, int64_t n) {
  if (n < 0 || (n > 0 && (!d || !d->side || !d->label || !d->frame))) return SGTD_ERR_INVALID;
  Group *g = G(e);
  const u32 gid = g->current_frame_id;
  if ((uint64_t)gid >= (uint64_t)e->cfg.max_frame_n) return SGTD_ERR_FRAME_LIMIT;
  const int s = shard_of(gid, g->n);
  sgtd_engine *c = g->dev[s];
  std::vector<uint32_t> lf((size_t)std::max<int64_t>(n, 1));
  for (int64_t i = 0; i < n; i++) {
    if (d->frame[i] != gid) { e->err = "multi-device tables take descriptors stamped with the current frame id"; return SGTD_ERR_UNSUPPORTED; }
    lf[(size_t)i] = local_of(gid, g->n);
  }
  if (n == 0) {   // an empty frame (d may be NULL): the owner only advances its frame counter
    MCHK(sgtd_add(c, nullptr, 0));
  } else {
    sgtd_desc_soa t = *d;
    t.frame = lf.data();
    MCHK(sgtd_add(c, &t, n));
  }
  g->current_frame_id++;
  g->batch_valid = false;
  return SGTD_OK;
}

int add_frames(sgtd_engine *e, const float *xyz, const uint32_t *label, const int64_t *kp_off, int n_frames, int device_ptrs) {
  if (n_frames < 0 || !kp_off) return SGTD_ERR_INVALID;
  if (n_frames == 0) return SGTD_OK;
  Group *g = G(e);
  if (device_ptrs) { e->err = "multi-device tables take host pointers"; return SGTD_ERR_UNSUPPORTED; }
  if ((uint64_t)g->current_frame_id + (uint64_t)n_frames > (uint64_t)e->cfg.max_frame_n) return SGTD_ERR_FRAME_LIMIT;
  int k = 0;
  while (k < n_frames) {   // runs of frames with one owner (to the end of its block)
    const u32 gid = g->current_frame_id;
    const int run = std::min<int>(n_frames - k, (int)(SGTD_SHARD_BLOCK - gid % SGTD_SHARD_BLOCK));
    sgtd_engine *c = g->dev[shard_of(gid, g->n)];
    MCHK(sgtd_add_frames(c, xyz, label, kp_off + k, run, 0));
    g->current_frame_id += (u32)run;
    k += run;
  }
  g->batch_valid = false;
  return SGTD_OK;
}

int finalize(sgtd_engine *e) {
  for (sgtd_engine *c : G(e)->dev) MCHK(sgtd_finalize(c));
  return SGTD_OK;
}

// every global id goes to its owner as the owner's local id; entry ids keep their shard << 40 form (each shard's
// insertion indices are renumbered densely on the shard)
int remove_frames(sgtd_engine *e, const uint32_t *frame_ids, int64_t n, int64_t *n_removed) {
  if (n < 0 || (n > 0 && !frame_ids)) return SGTD_ERR_INVALID;
  Group *g = G(e);
  std::vector<std::vector<uint32_t>> loc(g->n);
  for (int64_t i = 0; i < n; i++) loc[shard_of(frame_ids[i], g->n)].push_back(local_of(frame_ids[i], g->n));
  int64_t total = 0;
  for (int s = 0; s < g->n; s++) {
    if (loc[s].empty()) continue;
    sgtd_engine *c = g->dev[s];
    int64_t r = 0;
    MCHK(sgtd_remove_frames(c, loc[s].data(), (int64_t)loc[s].size(), &r));
    total += r;
  }
  if (total > 0) g->batch_valid = false;
  if (n_removed) *n_removed = total;
  return SGTD_OK;
}

// every shard gets the rows sliced to its own frames in its local ids.  A shard holds whole blocks of SGTD_SHARD_BLOCK
// (64) frames, global block b as its local block b / n: each of its blocks is one word of its rows, read from the global
// row at bit b * 64 - frame_lo.  A shard without a frame in [frame_lo, frame_lo + n_frames) allows nothing.
int set_frame_filter(sgtd_engine *e, uint32_t frame_lo, uint32_t n_frames, const uint64_t *rows, int n_rows) {
  Group *g = G(e);
  if (n_rows == 0) {
    for (sgtd_engine *c : g->dev) MCHK(sgtd_set_frame_filter(c, 0, 0, nullptr, 0));
    e->filt.reset();
    return SGTD_OK;
  }
  auto F = std::make_shared<FrameFilter>();
  F->lo = frame_lo; F->n = n_frames; F->n_rows = n_rows;      // (the group's own copy: the row count for filter_fits)
  e->filt = std::move(F);
  static_assert(SGTD_SHARD_BLOCK == 64, "a shard's block is one word of its rows");
  const size_t words = ((size_t)n_frames + 63) / 64;
  const u64 b_first = frame_lo / SGTD_SHARD_BLOCK, b_last = ((u64)frame_lo + n_frames - 1) / SGTD_SHARD_BLOCK;
  std::vector<uint64_t> loc;
  std::vector<u64> clean((size_t)n_rows * words);      // the caller's rows with the bits beyond n_frames cleared
  for (int r = 0; r < n_rows; r++)
    for (size_t w = 0; w < words; w++) {
      u64 v = rows[(size_t)r * words + w];
      if (w == words - 1 && n_frames % 64) v &= (1ull << (n_frames % 64)) - 1ull;
      clean[(size_t)r * words + w] = v;
    }
  for (int s = 0; s < g->n; s++) {
    sgtd_engine *c = g->dev[s];
    // the shard's first and last block inside the range
    u64 b0 = b_first + ((u64)s + g->n - b_first % g->n) % g->n;
    if (b0 > b_last) {
      const std::vector<uint64_t> none((size_t)n_rows, 0u);
      MCHK(sgtd_set_frame_filter(c, 0, 1, none.data(), n_rows));
      continue;
    }
    const u64 b1 = b_last - ((b_last + g->n - s) % g->n);
    const u64 lb0 = b0 / g->n, n_blocks = b1 / g->n - lb0 + 1;
    loc.assign((size_t)n_rows * n_blocks, 0u);
    for (int r = 0; r < n_rows; r++)
      for (u64 k = 0; k < n_blocks; k++) {
        const u64 b = (lb0 + k) * g->n + s;
        loc[(size_t)r * n_blocks + k] = row_bits_at(clean.data() + (size_t)r * words, words, (long long)(b * SGTD_SHARD_BLOCK) - (long long)frame_lo);
      }
    MCHK(sgtd_set_frame_filter(c, (uint32_t)(lb0 * SGTD_SHARD_BLOCK), (uint32_t)(n_blocks * SGTD_SHARD_BLOCK), loc.data(), n_rows));
  }
  return SGTD_OK;
}

// every shard keeps the poses of its own frames under their local ids (the group keeps them under the global ids for
// sgtd_result_world_poses); the checks ran in sgtd_set_frame_poses
int set_frame_poses(sgtd_engine *e, const uint32_t *frame_ids, const float *pose12, int64_t n) {
  Group *g = G(e);
  if (n == 0) {
    for (sgtd_engine *c : g->dev) MCHK(sgtd_set_frame_poses(c, frame_ids, pose12, 0));
    return SGTD_OK;
  }
  std::vector<std::vector<uint32_t>> loc(g->n);
  std::vector<std::vector<float>> rows(g->n);
  for (int64_t i = 0; i < n; i++) {
    const int s = shard_of(frame_ids[i], g->n);
    loc[s].push_back(local_of(frame_ids[i], g->n));
    if (pose12) rows[s].insert(rows[s].end(), pose12 + (size_t)i * 12, pose12 + (size_t)i * 12 + 12);
  }
  for (int s = 0; s < g->n; s++) {
    if (loc[s].empty()) continue;
    sgtd_engine *c = g->dev[s];
    MCHK(sgtd_set_frame_poses(c, loc[s].data(), pose12 ? rows[s].data() : nullptr, (int64_t)loc[s].size()));
  }
  return SGTD_OK;
}

// every shard keeps the keypoints of its own frames under their local ids (the group keeps them under the global ids,
// as it keeps the poses); the checks ran in sgtd_set_frame_keypoints
int set_frame_keypoints(sgtd_engine *e, const uint32_t *frame_ids, const int64_t *kp_off, const float *xyz, const uint32_t *label, int64_t n) {
  Group *g = G(e);
  if (n == 0) {
    for (sgtd_engine *c : g->dev) MCHK(sgtd_set_frame_keypoints(c, frame_ids, kp_off, xyz, label, 0));
    return SGTD_OK;
  }
  std::vector<std::vector<uint32_t>> loc(g->n), lab(g->n);
  std::vector<std::vector<int64_t>> off(g->n);
  std::vector<std::vector<float>> pts(g->n);
  for (int s = 0; s < g->n; s++) off[s].push_back(0);
  for (int64_t i = 0; i < n; i++) {
    const int s = shard_of(frame_ids[i], g->n);
    loc[s].push_back(local_of(frame_ids[i], g->n));
    if (xyz) {
      pts[s].insert(pts[s].end(), xyz + (size_t)kp_off[i] * 3, xyz + (size_t)kp_off[i + 1] * 3);
      lab[s].insert(lab[s].end(), label + (size_t)kp_off[i], label + (size_t)kp_off[i + 1]);
      off[s].push_back((int64_t)lab[s].size());
    }
  }
  static const float no_xyz[3] = {0.f, 0.f, 0.f};      // (a shard whose frames are all empty still stores them: not NULL)
  static const uint32_t no_label[1] = {0u};
  for (int s = 0; s < g->n; s++) {
    if (loc[s].empty()) continue;
    sgtd_engine *c = g->dev[s];
    MCHK(sgtd_set_frame_keypoints(c, loc[s].data(), off[s].data(), xyz ? (pts[s].empty() ? no_xyz : pts[s].data()) : nullptr,
                                  lab[s].empty() ? no_label : lab[s].data(), (int64_t)loc[s].size()));
  }
  return SGTD_OK;
}

// the prior goes to every shard as it is (it tests each shard's own positions); the group keeps it for prior_fits
int set_position_prior(sgtd_engine *e, const double *center, const double *radius, int n_rows, int dims) {
  for (sgtd_engine *c : G(e)->dev) MCHK(sgtd_set_position_prior(c, center, radius, n_rows, dims));
  return SGTD_OK;
}

int query_frames(sgtd_engine *e, const float *xyz, const uint32_t *label, const int64_t *kp_off, int n_queries, int device_ptrs) {
  if (n_queries <= 0 || !kp_off || !xyz || !label) return SGTD_ERR_INVALID;
  CHK(filter_fits(e, n_queries));
  CHK(prior_fits(e, n_queries));
  Group *g = G(e);
  if (device_ptrs) { e->err = "multi-device tables take host pointers"; return SGTD_ERR_UNSUPPORTED; }
  // every device builds the query descriptors itself and sweeps its shard; the calls only
  // enqueue, so the devices run concurrently
  for (sgtd_engine *c : g->dev) MCHK(sgtd_query_frames(c, xyz, label, kp_off, n_queries, 0));
  g->nq = n_queries; g->batch_valid = true; g->merged = false; new_results(g, false);
  return SGTD_OK;
}

int query_descs(sgtd_engine *e, const sgtd_desc_soa *q, int64_t nq) {
  if (nq < 0 || (nq > 0 && (!q || !q->side || !q->label || !q->frame))) return SGTD_ERR_INVALID;
  CHK(filter_fits(e, 1));
  CHK(prior_fits(e, 1));
  Group *g = G(e);
  std::vector<uint32_t> lf((size_t)std::max<int64_t>(nq, 1));
  for (int s = 0; s < g->n; s++) {
    sgtd_engine *c = g->dev[s];
    // the frame test (:373) compares ids: a query id that names a map frame of this shard
    // becomes that frame's local id, any other id a value no local frame has
    for (int64_t i = 0; i < nq; i++) {
      const u32 f = q->frame[i];
      lf[(size_t)i] = (f < g->current_frame_id && shard_of(f, g->n) == s) ? local_of(f, g->n) : 0xFFFFFFFEu;
    }
    sgtd_desc_soa t = *q;
    t.frame = lf.data();
    MCHK(sgtd_query_descs(c, &t, nq));
  }
  g->nq = 1; g->batch_valid = true; g->merged = false; new_results(g, false);
  return SGTD_OK;
}

// gathers the local candidate tables and merges them (STDesc.cpp:423-433 on the union)
int merge(sgtd_engine *e) {
  Group *g = G(e);
  if (!g->batch_valid) return SGTD_ERR_STATE;
  if (g->merged) return SGTD_OK;
  const int cn = e->cfg.candidate_num, nq = g->nq, n = g->n;
  std::vector<std::vector<int>> nc(n), cf(n), cv(n);
  std::vector<std::vector<int64_t>> po(n);
  for (int s = 0; s < n; s++) {
    sgtd_engine *c = g->dev[s];
    nc[s].resize(nq); cf[s].resize((size_t)nq * cn); cv[s].resize((size_t)nq * cn); po[s].resize((size_t)nq * (cn + 1));
    MCHK(sgtd_result_candidates(c, nc[s].data(), cf[s].data(), cv[s].data(), po[s].data()));
  }
  g->n_cand.assign(nq, 0);
  g->cand_frame.assign((size_t)nq * cn, -1); g->cand_votes.assign((size_t)nq * cn, 0);
  g->owner.assign((size_t)nq * cn, -1); g->owner_slot.assign((size_t)nq * cn, -1);
  g->pair_off.assign((size_t)nq * (cn + 1), 0);
  struct Item { long long votes; u32 frame; int s, k; };
  std::vector<Item> items;
  for (int q = 0; q < nq; q++) {
    items.clear();
    for (int s = 0; s < n; s++)
      for (int k = 0; k < nc[s][q]; k++) {
        const size_t i = (size_t)q * cn + k;
        if (cv[s][i] >= 5) items.push_back({cv[s][i], global_of(s, (u32)cf[s][i], n), s, k});
      }
    std::sort(items.begin(), items.end(), [](const Item &a, const Item &b) {
      return a.votes != b.votes ? a.votes > b.votes : a.frame < b.frame;
    });
    const int m = (int)std::min<size_t>(items.size(), (size_t)cn);
    g->n_cand[q] = m;
    long long acc = 0;
    for (int k = 0; k <= cn; k++) {
      g->pair_off[(size_t)q * (cn + 1) + k] = acc;
      if (k < m) {
        const Item &it = items[k];
        const size_t i = (size_t)q * cn + k;
        g->cand_frame[i] = (int)it.frame; g->cand_votes[i] = (int)it.votes; g->owner[i] = it.s; g->owner_slot[i] = it.k;
        acc += po[it.s][(size_t)q * (cn + 1) + it.k + 1] - po[it.s][(size_t)q * (cn + 1) + it.k];
      }
    }
  }
  g->merged = true;
  return SGTD_OK;
}

int result_candidates(sgtd_engine *e, int32_t *n_cand, int32_t *cand_frame, int32_t *cand_votes, int64_t *pair_off) {
  CHK(merge(e));
  Group *g = G(e);
  const int cn = e->cfg.candidate_num, nq = g->nq;
  if (n_cand) std::memcpy(n_cand, g->n_cand.data(), nq * sizeof(int));
  if (cand_frame) std::memcpy(cand_frame, g->cand_frame.data(), (size_t)nq * cn * sizeof(int));
  if (cand_votes) std::memcpy(cand_votes, g->cand_votes.data(), (size_t)nq * cn * sizeof(int));
  if (pair_off)
    for (size_t i = 0; i < (size_t)nq * (cn + 1); i++) pair_off[i] = g->pair_off[i];
  return SGTD_OK;
}

// query q's merged candidate count and global frame ids
int candidates_of(sgtd_engine *e, int q, int *n_cand, int *cand_frame) {
  CHK(merge(e));
  Group *g = G(e);
  if (q < 0 || q >= g->nq) return SGTD_ERR_INVALID;
  const int cn = e->cfg.candidate_num;
  *n_cand = g->n_cand[(size_t)q];
  std::memcpy(cand_frame, g->cand_frame.data() + (size_t)q * cn, (size_t)cn * sizeof(int));
  return SGTD_OK;
}

// match lists of query q in the merged candidate order, each fetched from its owner
int result_pairs(sgtd_engine *e, int q, int32_t *q_idx, int64_t *db_entry, int64_t capacity, int64_t *n_pairs) {
  if (!n_pairs) return SGTD_ERR_INVALID;
  CHK(merge(e));
  Group *g = G(e);
  if (q < 0 || q >= g->nq) return SGTD_ERR_INVALID;
  const int cn = e->cfg.candidate_num;
  const int64_t total = g->pair_off[(size_t)q * (cn + 1) + cn];
  *n_pairs = total;
  if (total > capacity) return SGTD_ERR_CAPACITY;
  std::vector<std::vector<int32_t>> qi(g->n);
  std::vector<std::vector<int64_t>> en(g->n), off(g->n);
  return gather(e, q, [&](sgtd_engine *c, int s) {   // the owner's lists of this query
    off[s].resize((size_t)g->nq * (cn + 1));
    MCHK(sgtd_result_candidates(c, nullptr, nullptr, nullptr, off[s].data()));
    const int64_t ts = off[s][(size_t)q * (cn + 1) + cn];
    qi[s].resize((size_t)std::max<int64_t>(ts, 1)); en[s].resize((size_t)std::max<int64_t>(ts, 1));
    int64_t got = 0;
    MCHK(sgtd_result_pairs(c, q, qi[s].data(), en[s].data(), ts, &got));
    return (int)SGTD_OK;
  }, [&](int s, int ks, int k) {
    const int64_t lo = off[s][(size_t)q * (cn + 1) + ks], hi = off[s][(size_t)q * (cn + 1) + ks + 1];
    int64_t o = g->pair_off[(size_t)q * (cn + 1) + k];
    for (int64_t r = lo; r < hi; r++, o++) {
      if (q_idx) q_idx[o] = qi[s][(size_t)r];
      if (db_entry) db_entry[o] = ((int64_t)s << SGTD_ENTRY_SHARD_SHIFT) | en[s][(size_t)r];
    }
  });
}

int fetch_entries(sgtd_engine *e, const int64_t *db_entry, int64_t n, sgtd_desc_soa *out) {
  if (n < 0 || (n > 0 && (!db_entry || !out))) return SGTD_ERR_INVALID;
  Group *g = G(e);
  // runs of one owner are fetched together; frame ids come back global
  int64_t i = 0;
  std::vector<int64_t> loc;
  while (i < n) {
    const int s = (int)(db_entry[i] >> SGTD_ENTRY_SHARD_SHIFT);
    if (s < 0 || s >= g->n) return SGTD_ERR_INVALID;
    int64_t j = i;
    loc.clear();
    while (j < n && (int)(db_entry[j] >> SGTD_ENTRY_SHARD_SHIFT) == s) { loc.push_back(db_entry[j] & ((1ll << SGTD_ENTRY_SHARD_SHIFT) - 1)); j++; }
    sgtd_desc_soa t;
    t.side = out->side ? out->side + 3 * i : nullptr; t.angle = out->angle ? out->angle + 3 * i : nullptr;
    t.center = out->center ? out->center + 3 * i : nullptr; t.vertex = out->vertex ? out->vertex + 9 * i : nullptr;
    t.label = out->label ? out->label + 3 * i : nullptr; t.frame = out->frame ? out->frame + i : nullptr;
    t.node_id = out->node_id ? out->node_id + 3 * i : nullptr;
    sgtd_engine *c = g->dev[s];
    MCHK(sgtd_fetch_entries(c, loc.data(), j - i, &t));
    if (t.frame)
      for (int64_t k = 0; k < j - i; k++) t.frame[k] = global_of(s, t.frame[k], g->n);
    i = j;
  }
  return SGTD_OK;
}

int result_query_desc_count(sgtd_engine *e, int q, int64_t *n) { sgtd_engine *c = G(e)->dev[0]; MCHK(sgtd_result_query_desc_count(c, q, n)); return SGTD_OK; }

int result_query_descs(sgtd_engine *e, int q, sgtd_desc_soa *out, int64_t capacity, int64_t *n_out) {
  Group *g = G(e);
  sgtd_engine *c = g->dev[0];
  MCHK(sgtd_result_query_descs(c, q, out, capacity, n_out));
  if (out->frame)
    for (int64_t i = 0; i < *n_out; i++) out->frame[i] = g->current_frame_id;   // :592: every query descriptor carries F
  return SGTD_OK;
}

int result_votes(sgtd_engine *e, int q, uint32_t *votes, int64_t capacity, uint32_t *frame_lo, int64_t *n) {
  Group *g = G(e);
  if (!n || !g->batch_valid || q < 0 || q >= g->nq) return SGTD_ERR_INVALID;
  const u32 lo = e->cfg.first_frame_id;
  const int64_t span = std::max<int64_t>((int64_t)g->current_frame_id - lo, 1);
  *n = span;
  if (frame_lo) *frame_lo = lo;
  if (!votes) return SGTD_OK;
  if (span > capacity) return SGTD_ERR_CAPACITY;
  std::fill(votes, votes + span, 0u);
  std::vector<uint32_t> lv;
  for (int s = 0; s < g->n; s++) {
    sgtd_engine *c = g->dev[s];
    uint32_t llo = 0; int64_t ln = 0;
    MCHK(sgtd_result_votes(c, q, nullptr, 0, &llo, &ln));
    lv.assign((size_t)ln, 0u);
    MCHK(sgtd_result_votes(c, q, lv.data(), ln, &llo, &ln));
    for (int64_t k = 0; k < ln; k++) {
      const u32 gf = global_of(s, llo + (u32)k, g->n);
      if (lv[(size_t)k] && gf >= lo && gf - lo < (u32)span) votes[gf - lo] = lv[(size_t)k];
    }
  }
  return SGTD_OK;
}

int verify(sgtd_engine *e) {
  Group *g = G(e);
  CHK(merge(e));
  stale_stages(g);
  for (sgtd_engine *c : g->dev) MCHK(sgtd_verify(c));   // every owner verifies its local candidates
  g->verified = true;
  return SGTD_OK;
}

int result_verify(sgtd_engine *e, int q, double *score, double *pose) {
  Group *g = G(e);
  if (!g->verified || q < 0 || q >= g->nq) return SGTD_ERR_INVALID;
  const int cn = e->cfg.candidate_num;
  std::vector<std::vector<double>> ss(g->n), pp(g->n);
  for (int k = 0; k < cn; k++) {
    if (score) score[k] = -1.0;
    if (pose) std::fill(pose + (size_t)k * 12, pose + (size_t)k * 12 + 12, 0.0);
  }
  return gather(e, q, [&](sgtd_engine *c, int s) {
    ss[s].resize(cn); pp[s].resize((size_t)cn * 12);
    return sgtd_result_verify(c, q, ss[s].data(), pp[s].data());
  }, [&](int s, int ks, int k) {
    if (score) score[k] = ss[s][ks];
    if (pose) std::copy(pp[s].begin() + (size_t)ks * 12, pp[s].begin() + (size_t)ks * 12 + 12, pose + (size_t)k * 12);
  });
}

// every owner refits the poses of its local candidates
int refine_poses(sgtd_engine *e, int iterations) {
  return fan_out(e, "sgtd_refine_poses", nullptr, &G(e)->refined, [&](sgtd_engine *c) { return sgtd_refine_poses(c, iterations); });
}

// the refined results of query q's merged candidates
int result_refined(sgtd_engine *e, int q, double *pose, double *rmse, double *rmse_verify, int32_t *n_pairs, double *moments) {
  Group *g = G(e);
  CHK(group_result_ready(e, q, g->refined, kNoRefined));
  const int cn = e->cfg.candidate_num;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  struct Owned { std::vector<double> pose, rmse, rmse_v, mom; std::vector<int32_t> np; };
  std::vector<Owned> own(g->n);
  for (int k = 0; k < cn; k++) {
    if (pose) std::fill(pose + (size_t)k * 12, pose + (size_t)k * 12 + 12, 0.0);
    if (rmse) rmse[k] = nan;
    if (rmse_verify) rmse_verify[k] = nan;
    if (n_pairs) n_pairs[k] = 0;
    if (moments) std::fill(moments + (size_t)k * 15, moments + (size_t)k * 15 + 15, nan);
  }
  return gather(e, q, [&](sgtd_engine *c, int s) {
    Owned &o = own[s];
    o.pose.resize((size_t)cn * 12); o.rmse.resize(cn); o.rmse_v.resize(cn); o.mom.resize((size_t)cn * 15); o.np.resize(cn);
    return sgtd_result_refined(c, q, o.pose.data(), o.rmse.data(), o.rmse_v.data(), o.np.data(), o.mom.data());
  }, [&](int s, int ks, int k) {
    const Owned &o = own[s];
    if (pose) std::copy(o.pose.begin() + (size_t)ks * 12, o.pose.begin() + (size_t)ks * 12 + 12, pose + (size_t)k * 12);
    if (rmse) rmse[k] = o.rmse[ks];
    if (rmse_verify) rmse_verify[k] = o.rmse_v[ks];
    if (n_pairs) n_pairs[k] = o.np[ks];
    if (moments) std::copy(o.mom.begin() + (size_t)ks * 15, o.mom.begin() + (size_t)ks * 15 + 15, moments + (size_t)k * 15);
  });
}

int nq_of(sgtd_engine *e, int *nq) {
  Group *g = G(e);
  if (!g->batch_valid) return SGTD_ERR_STATE;
  *nq = g->nq;
  return SGTD_OK;
}

int has_overlap(sgtd_engine *e) {
  Group *g = G(e);
  return g->batch_valid && g->verified && g->overlapped;
}

// every owner computes the overlap of its local candidates (the checks ran in sgtd_overlap)
int overlap(sgtd_engine *e, double radius, int flags, const float *q_xyz, const uint32_t *q_label, const int64_t *q_kp_off) {
  return fan_out(e, "sgtd_overlap", (flags & SGTD_OVERLAP_REFINED) ? "SGTD_OVERLAP_REFINED" : nullptr, &G(e)->overlapped,
                 [&](sgtd_engine *c) { return sgtd_overlap(c, radius, flags, q_xyz, q_label, q_kp_off); });
}

// the overlap results of query q's merged candidates
int result_overlap(sgtd_engine *e, int q, int32_t *n_query_kp, int32_t *n_frame_kp, int32_t *n_hit_query, int32_t *n_hit_frame, double *overlap, double *rms) {
  Group *g = G(e);
  CHK(group_result_ready(e, q, g->overlapped, kNoOverlap));
  const int cn = e->cfg.candidate_num;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  struct Owned { std::vector<int32_t> c[4]; std::vector<double> ov, rms; };
  std::vector<Owned> own(g->n);
  int32_t *out[4] = {n_query_kp, n_frame_kp, n_hit_query, n_hit_frame};
  for (int k = 0; k < cn; k++) {
    for (int a = 0; a < 4; a++) if (out[a]) out[a][k] = -1;
    if (overlap) overlap[k] = nan;
    if (rms) rms[k] = nan;
  }
  return gather(e, q, [&](sgtd_engine *c, int s) {
    Owned &o = own[s];
    for (int a = 0; a < 4; a++) o.c[a].resize(cn);
    o.ov.resize(cn); o.rms.resize(cn);
    return sgtd_result_overlap(c, q, o.c[0].data(), o.c[1].data(), o.c[2].data(), o.c[3].data(), o.ov.data(), o.rms.data());
  }, [&](int s, int ks, int k) {
    const Owned &o = own[s];
    for (int a = 0; a < 4; a++) if (out[a]) out[a][k] = o.c[a][ks];
    if (overlap) overlap[k] = o.ov[ks];
    if (rms) rms[k] = o.rms[ks];
  });
}

int has_aligned(sgtd_engine *e) {
  Group *g = G(e);
  return g->batch_valid && g->verified && g->aligned;
}

// every owner aligns its local candidates (the checks ran in sgtd_align_keypoints)
int align_keypoints(sgtd_engine *e, double radius, int iterations, int flags, const float *q_xyz, const uint32_t *q_label, const int64_t *q_kp_off) {
  return fan_out(e, "sgtd_align_keypoints", (flags & SGTD_ALIGN_REFINED) ? "SGTD_ALIGN_REFINED" : nullptr, &G(e)->aligned,
                 [&](sgtd_engine *c) { return sgtd_align_keypoints(c, radius, iterations, flags, q_xyz, q_label, q_kp_off); });
}

// the aligned results of query q's merged candidates
int result_aligned(sgtd_engine *e, int q, double *pose, int32_t *n_fits, int32_t *n_corr, int32_t *stop, int32_t *counts_before, int32_t *counts_after,
                   double *overlap_before, double *rms_before, double *overlap_after, double *rms_after, double *moments) {
  Group *g = G(e);
  CHK(group_result_ready(e, q, g->aligned, kNoAligned));
  const int cn = e->cfg.candidate_num;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  struct Owned { std::vector<double> pose, mom, val[4]; std::vector<int32_t> fit[3], cnt[2]; };
  std::vector<Owned> own(g->n);
  int32_t *fit[3] = {n_fits, n_corr, stop}, *cnt[2] = {counts_before, counts_after};
  double *val[4] = {overlap_before, rms_before, overlap_after, rms_after};
  for (int k = 0; k < cn; k++) {
    if (pose) std::fill(pose + (size_t)k * 12, pose + (size_t)k * 12 + 12, 0.0);
    if (moments) std::fill(moments + (size_t)k * 15, moments + (size_t)k * 15 + 15, nan);
    for (int a = 0; a < 3; a++) if (fit[a]) fit[a][k] = a == 2 ? -1 : 0;
    for (int a = 0; a < 2; a++) if (cnt[a]) std::fill(cnt[a] + (size_t)k * 4, cnt[a] + (size_t)k * 4 + 4, -1);
    for (int a = 0; a < 4; a++) if (val[a]) val[a][k] = nan;
  }
  return gather(e, q, [&](sgtd_engine *c, int s) {
    Owned &o = own[s];
    o.pose.resize((size_t)cn * 12); o.mom.resize((size_t)cn * 15);
    for (int a = 0; a < 4; a++) o.val[a].resize(cn);
    for (int a = 0; a < 3; a++) o.fit[a].resize(cn);
    for (int a = 0; a < 2; a++) o.cnt[a].resize((size_t)cn * 4);
    return sgtd_result_aligned(c, q, o.pose.data(), o.fit[0].data(), o.fit[1].data(), o.fit[2].data(), o.cnt[0].data(), o.cnt[1].data(),
                               o.val[0].data(), o.val[1].data(), o.val[2].data(), o.val[3].data(), o.mom.data());
  }, [&](int s, int ks, int k) {
    const Owned &o = own[s];
    if (pose) std::copy(o.pose.begin() + (size_t)ks * 12, o.pose.begin() + (size_t)ks * 12 + 12, pose + (size_t)k * 12);
    if (moments) std::copy(o.mom.begin() + (size_t)ks * 15, o.mom.begin() + (size_t)ks * 15 + 15, moments + (size_t)k * 15);
    for (int a = 0; a < 3; a++) if (fit[a]) fit[a][k] = o.fit[a][ks];
    for (int a = 0; a < 2; a++) if (cnt[a]) std::copy(o.cnt[a].begin() + (size_t)ks * 4, o.cnt[a].begin() + (size_t)ks * 4 + 4, cnt[a] + (size_t)k * 4);
    for (int a = 0; a < 4; a++) if (val[a]) val[a][k] = o.val[a][ks];
  });
}

int result_aligned_pairs(sgtd_engine *e, int q, int cand, int32_t *frame_kp, int64_t capacity, int64_t *n) {
  Group *g = G(e);
  CHK(group_result_ready(e, q, g->aligned, kNoAligned));
  if (cand < 0 || cand >= g->n_cand[q]) return SGTD_ERR_INVALID;
  const size_t i = (size_t)q * e->cfg.candidate_num + cand;
  sgtd_engine *c = g->dev[g->owner[i]];
  MCHK(sgtd_result_aligned_pairs(c, q, g->owner_slot[i], frame_kp, capacity, n));
  return SGTD_OK;
}

int result_inliers(sgtd_engine *e, int q, int cand, int32_t *idx, int64_t capacity, int64_t *n) {
  Group *g = G(e);
  if (!g->verified || q < 0 || q >= g->nq || cand < 0 || cand >= g->n_cand[q]) return SGTD_ERR_INVALID;
  const size_t i = (size_t)q * e->cfg.candidate_num + cand;
  sgtd_engine *c = g->dev[g->owner[i]];
  MCHK(sgtd_result_inliers(c, q, g->owner_slot[i], idx, capacity, n));
  return SGTD_OK;
}

// inlier pairs of every merged candidate of query q: each candidate's from its owner, entry ids with the owner in the upper bits
int result_inlier_pairs(sgtd_engine *e, int q, int64_t *cand_off, int32_t *q_idx, int64_t *db_entry, int64_t capacity, int64_t *n_pairs) {
  Group *g = G(e);
  if (!n_pairs || !cand_off || !g->verified || q < 0 || q >= g->nq) return SGTD_ERR_INVALID;
  const int cn = e->cfg.candidate_num;
  std::vector<std::vector<int32_t>> qi(g->n);
  std::vector<std::vector<int64_t>> en(g->n), off(g->n);
  int64_t o = 0;
  bool fits = true;
  for (int k = 0; k <= cn; k++) cand_off[k] = 0;
  CHK(gather(e, q, [&](sgtd_engine *c, int s) {   // the owner's inlier pairs of this query: how many, then the pairs
    off[s].resize((size_t)cn + 1);
    int64_t ns = 0;
    const int st = sgtd_result_inlier_pairs(c, q, off[s].data(), nullptr, nullptr, 0, &ns);
    if (st != SGTD_OK && st != SGTD_ERR_CAPACITY) return st;
    qi[s].resize((size_t)std::max<int64_t>(ns, 1)); en[s].resize((size_t)std::max<int64_t>(ns, 1));
    return sgtd_result_inlier_pairs(c, q, off[s].data(), qi[s].data(), en[s].data(), ns, &ns);
  }, [&](int s, int ks, int k) {
    cand_off[k] = o;
    for (int64_t r = off[s][(size_t)ks]; r < off[s][(size_t)ks + 1]; r++, o++) {
      if (o < capacity) {
        if (q_idx) q_idx[o] = qi[s][(size_t)r];
        if (db_entry) db_entry[o] = ((int64_t)s << SGTD_ENTRY_SHARD_SHIFT) | en[s][(size_t)r];
      } else fits = false;
    }
  }));
  for (int k = g->n_cand[q]; k <= cn; k++) cand_off[k] = o;
  *n_pairs = o;
  return fits ? SGTD_OK : SGTD_ERR_CAPACITY;
}

// SearchLoop's choice on the merged list (STDesc.cpp:105-146)
int search_loop(sgtd_engine *e, double icp_threshold, int32_t *best_cand, int32_t *best_frame, double *best_score) {
  Group *g = G(e);
  if (!g->verified) return SGTD_ERR_INVALID;
  const int cn = e->cfg.candidate_num;
  std::vector<double> score(cn);
  for (int q = 0; q < g->nq; q++) {
    CHK(result_verify(e, q, score.data(), nullptr));
    double best = 0; int arg = -1;
    for (int k = 0; k < g->n_cand[q]; k++)
      if (score[k] > best) { best = score[k]; arg = k; }
    const bool ok = arg >= 0 && best > icp_threshold;
    if (best_cand) best_cand[q] = ok ? arg : -1;
    if (best_frame) best_frame[q] = ok ? g->cand_frame[(size_t)q * cn + arg] : -1;
    if (best_score) best_score[q] = ok ? best : 0.0;
  }
  return SGTD_OK;
}

int sync(sgtd_engine *e) {
  for (sgtd_engine *c : G(e)->dev) MCHK(sgtd_sync(c));
  return SGTD_OK;
}

int get_stats(sgtd_engine *e, sgtd_stats *out) {
  Group *g = G(e);
  sgtd_stats t{};
  for (int s = 0; s < g->n; s++) {
    sgtd_engine *c = g->dev[s];
    sgtd_stats x;
    MCHK(sgtd_get_stats(c, &x));
    t.n_entries += x.n_entries; t.n_buckets += x.n_buckets; t.n_frames += x.n_frames;
    t.last_queries = x.last_queries; t.last_D = x.last_D;
    t.last_P += x.last_P; t.last_M += x.last_M; t.last_P_swept += x.last_P_swept;
    t.hbm_bytes_table += x.hbm_bytes_table;
    t.overflowed |= x.overflowed;
    t.select_form = x.select_form;
    t.batches_total = x.batches_total; t.overflow_launches_total += x.overflow_launches_total;
    t.reruns_total += x.reruns_total; t.rewrites_total += x.rewrites_total; t.order_giveups_total += x.order_giveups_total;
    t.list_moves_total += x.list_moves_total; t.last_list_moves += x.last_list_moves;
    t.ms_total = std::max(t.ms_total, x.ms_total);
    if (s == 0) { t.ms_consistency_pairs = x.ms_consistency_pairs; t.ms_consistency_greedy = x.ms_consistency_greedy; t.consistency_rounds = x.consistency_rounds; }   // (sgtd_consistent_loops runs on the first device)
  }
  if (g->merged) {
    const int cn = e->cfg.candidate_num;
    for (int q = 0; q < g->nq; q++) t.last_cand_pairs += g->pair_off[(size_t)q * (cn + 1) + cn];
  }
  *out = t;
  return SGTD_OK;
}

int max_batch(sgtd_engine *e, int n_keypoints, int64_t *max_queries) {
  int64_t best = -1;
  for (sgtd_engine *c : G(e)->dev) {
    int64_t m = 0;
    MCHK(sgtd_max_batch(c, n_keypoints, &m));
    best = best < 0 ? m : std::min(best, m);
  }
  *max_queries = best;
  return SGTD_OK;
}

u32 current_frame_id(sgtd_engine *e) { return G(e)->current_frame_id; }
int device_count(sgtd_engine *e) { return G(e)->n; }
sgtd_engine *device_handle(sgtd_engine *e, int k) { return (k >= 0 && k < G(e)->n) ? G(e)->dev[k] : nullptr; }

#undef MCHK
}  // namespace multi
