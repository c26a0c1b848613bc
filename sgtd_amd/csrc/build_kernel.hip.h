// build_kernel.hip.h — BuildSingleScanSTD (src/sgtd/src/STDesc.cpp:174-315)
// for a batch of frames, one workgroup per frame.
//
//   stage 0  keypoints (xyz f32 + label) -> LDS                (16 B/keypoint)
//   stage 1  exact k-NN in LDS: f32 ((dx*dx)+dy*dy)+dz*dz, ascending, ties ->
//            lower index (stands in for pcl::KdTreeFLANN, :183-192); selection by
//            sorting and merging networks on (distance, index) keys in registers
//   stage 2  triplet enumeration t = i*C(K-1,2) + (m,n) in the reference's
//            loop order (:189-194): sides, length filter (:204-208), 3-step
//            strict-'>' sort (:220-243), millimetre key (:244-248)
//   stage 3  first-wins dedup (:249-251,307): open-addressing table in LDS
//            holding the minimum t per key (atomicCAS + atomicMin)
//   stage 4  ordered compaction (winner bitmap + prefix popcount -> the winners'
//            list in rank order) and descriptor fill (:253-308) of the listed
//            triplets at out[frame_slot*stride + rank]
#pragma once
#include <utility>
#include "common.hip.h"

struct DescArrays {
  double *side, *angle, *center;  // [cap*3]
  float *vertex;                  // [cap*9]  A,B,C xyz
  int *label;                     // [cap*3]
  u32 *frame;                     // [cap]
  int *node_id;                   // [cap*3]
  QueryRec *qrec;                 // [cap] sweep record (query descriptors only; may be null)
};

#define SGTD_BUILD_THREADS 1024
#ifdef SGTD_EXP_PHASE
__device__ unsigned long long g_bphase[8];
#define BPH(i) do { if (tid == 0) { const unsigned long long _n = __builtin_readcyclecounter(); atomicAdd(&g_bphase[i], _n - bph_t); bph_t = _n; } } while (0)
#else
#define BPH(i) do { } while (0)
#endif
#define SGTD_TRI_INVALID 0xFFFFFFFFFFFFFFFFull
#define SGTD_SLOT_EMPTY 0xFFFFFFFFu

struct Tri {
  double a, b, c;     // sorted ascending
  int va, vb, vc;     // vertex A,B,C as 0/1/2 = p1/p2/p3
  bool valid;
};

// |p - q| as the reference computes it (:198-203): f32 subtraction, then
// pow(double,2) (exact), two rounded f64 adds, correctly rounded sqrt
__device__ __forceinline__ double side_len(const float4 &p, const float4 &q) {
  double dx = (double)(p.x - q.x), dy = (double)(p.y - q.y), dz = (double)(p.z - q.z);
  return sqrt(dx * dx + dy * dy + dz * dz);
}

__device__ __forceinline__ Tri make_triangle(const float4 &p1, const float4 &p2,
                                             const float4 &p3, const DevCfg &cfg) {
  Tri t;
  double a = side_len(p1, p2), b = side_len(p1, p3), c = side_len(p3, p2);
  t.valid = !(a > cfg.max_len || b > cfg.max_len || c > cfg.max_len ||
              a < cfg.min_len || b < cfg.min_len || c < cfg.min_len);
  // side identities 0:(p1,p2) 1:(p1,p3) 2:(p2,p3) stand for l1,l2,l3 (:213-218);
  // two different sides share vertex index (u+v-1): {0,1}->p1 {0,2}->p2 {1,2}->p3
  int sa = 0, sb = 1, sc = 2;
  double tmp; int ti;
  if (a > b) { tmp = a; a = b; b = tmp; ti = sa; sa = sb; sb = ti; }
  if (b > c) { tmp = b; b = c; c = tmp; ti = sb; sb = sc; sc = ti; }
  if (a > b) { tmp = a; a = b; b = tmp; ti = sa; sa = sb; sb = ti; }
  t.a = a; t.b = b; t.c = c;
  t.va = sa + sb - 1;  // shared by shortest and middle side  (:253-265)
  t.vb = sa + sc - 1;  // shared by shortest and longest      (:266-278)
  t.vc = sb + sc - 1;  // shared by middle and longest        (:279-291)
  return t;
}

// millimetre dedup key: (int64_t)(float)(side*1000) per side (:244-248), 21 bits each
__host__ __device__ __forceinline__ u64 pack_milli_key(u64 x, u64 y, u64 z) { return (x << 42) | (y << 21) | z; }
__device__ __forceinline__ u64 milli_key(const Tri &t) {
  float kx = (float)(t.a * 1000.0), ky = (float)(t.b * 1000.0), kz = (float)(t.c * 1000.0);
  u64 x = (u64)(long long)kx, y = (u64)(long long)ky, z = (u64)(long long)kz;
  return pack_milli_key(x, y, z);
}

// ---- k-NN selection: compare-exchange networks on 64-bit keys, generated and checked at compile time
// key = (f32 bits of d) << 32 | j.  d is a sum of squares: never negative, never -0, so its bit pattern orders like
// its value, and the key order is (smaller distance, then lower index).
// An empty slot holds (+inf bits) << 32 | 0.  A candidate at d = +inf or NaN (bits above +inf's, whatever the sign;
// knn_key takes them down to +inf's) has a key >= that placeholder, and a list starts with as many placeholders as it
// has slots: such a candidate never comes before one of them, so the slot reads index 0 — what a selection by
// `d < best` gives, which is never true for such a d.
#define SGTD_KNN_EMPTY 0x7F80000000000000ull

struct CexNet {                 // compare-exchanges in order: min -> lo[c], max -> hi[c], lo[c] < hi[c]
  int n_cex;
  unsigned char lo[64], hi[64];
};

// sorting network of n inputs: the 29-exchange network for 10 (the fewest known), else Batcher's odd-even merge sort
// of the next power of two with the exchanges that touch a pad position (a +inf that never moves) dropped
constexpr CexNet knn_sort_net(int n) {
  CexNet t{};
  if (n == 10) {
    const unsigned char net[29][2] = {{0, 8}, {1, 9}, {2, 7}, {3, 5}, {4, 6}, {0, 2}, {1, 4}, {5, 8}, {7, 9}, {0, 3},
                                      {2, 4}, {5, 7}, {6, 9}, {0, 1}, {3, 6}, {8, 9}, {1, 5}, {2, 3}, {4, 8}, {6, 7},
                                      {1, 2}, {3, 5}, {4, 6}, {7, 8}, {2, 3}, {4, 5}, {6, 7}, {3, 4}, {5, 6}};
    for (int c = 0; c < 29; c++) { t.lo[c] = net[c][0]; t.hi[c] = net[c][1]; }
    t.n_cex = 29;
    return t;
  }
  for (int p = 1; p < n; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j + k < n; j += 2 * k)
        for (int i = 0; i < k && i + j + k < n; i++)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
            t.lo[t.n_cex] = (unsigned char)(i + j);
            t.hi[t.n_cex] = (unsigned char)(i + j + k);
            t.n_cex++;
          }
  return t;
}

// sorts m[k] = min(best[k], batch[n-1-k]) of two ascending lists: m rises, then falls.  Read from its far end and
// followed by -inf pads up to a power of two it is bitonic, and the bitonic merger in DESCENDING order leaves the pads
// where they are: wire w is m[n-1-w], exchanges that touch a pad are dropped, m comes out ascending.
constexpr CexNet knn_merge_net(int n) {
  CexNet t{};
  int p = 1;
  while (p < n) p *= 2;
  for (int k = p / 2; k >= 1; k /= 2)
    for (int w = 0; w + k < n; w++)
      if ((w & k) == 0) {
        t.lo[t.n_cex] = (unsigned char)(n - 1 - w - k);
        t.hi[t.n_cex] = (unsigned char)(n - 1 - w);
        t.n_cex++;
      }
  return t;
}

// 0-1 principle, 64 inputs per word: wire w of input x carries bit w of x
constexpr bool knn_sort_net_sorts(const CexNet &t, int n) {
  const u64 low[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
                      0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
  const int words = n > 6 ? 1 << (n - 6) : 1;
  for (int word = 0; word < words; word++) {
    u64 v[SGTD_MAX_K] = {};
    for (int w = 0; w < n; w++) v[w] = w < 6 ? low[w] : (((word >> (w - 6)) & 1) ? ~0ull : 0ull);
    for (int c = 0; c < t.n_cex; c++) {
      const u64 a = v[t.lo[c]], b = v[t.hi[c]];
      v[t.lo[c]] = a & b;
      v[t.hi[c]] = a | b;
    }
    for (int w = 0; w + 1 < n; w++)
      if (v[w] & ~v[w + 1]) return false;
  }
  return true;
}

// every pair of sorted 0-1 lists, n of best (za zeros first) and b <= n of a batch (zb zeros first; it stands for a
// list of n that ends in n - b ones): the merge step leaves min(za + zb, n) zeros, then ones
constexpr bool knn_merge_net_merges(const CexNet &t, int n, int b) {
  for (int za = 0; za <= n; za++)
    for (int zb = 0; zb <= b; zb++) {
      int v[SGTD_MAX_K] = {};
      for (int k = 0; k < n; k++) {
        const int x = k >= za, y = (n - 1 - k) >= zb;
        v[k] = x < y ? x : y;
      }
      for (int c = 0; c < t.n_cex; c++) {
        const int x = v[t.lo[c]], y = v[t.hi[c]];
        v[t.lo[c]] = x < y ? x : y;
        v[t.hi[c]] = x < y ? y : x;
      }
      const int z = za + zb < n ? za + zb : n;
      for (int k = 0; k < n; k++)
        if (v[k] != (k >= z)) return false;
    }
  return true;
}

// KM slots of the best list; candidates come B at a time.  B = KM up to the shipped 10; the two larger lists take a
// part of a list at a time, for the registers: 2 * (KM + B) of keys beside the candidates' coordinates in flight
// (12: as many instructions per candidate as with B = KM; 16: a fifth more)
template <int KM>
struct KnnNets {
  static constexpr int B = KM > 12 ? KM / 4 : KM > 10 ? KM / 2 : KM;
  static constexpr CexNet sort = knn_sort_net(B);
  static constexpr CexNet merge = knn_merge_net(KM);
  static_assert(KM <= SGTD_MAX_K && knn_sort_net_sorts(sort, B), "the sorting network does not sort");
  static_assert(knn_merge_net_merges(merge, KM, B), "the merge network does not merge");
};

// One exchange is two instructions.  A key's distance word is at most +inf's bits (knn_key), so as an f64 bit pattern
// the key is a finite number >= +0 (exponent field <= 0x7F8; small distances make denormals, which f64 instructions
// keep), and such numbers order like their bit patterns: v_min_f64 / v_max_f64 hand back one operand or the other,
// bit for bit.  As integers an exchange would be a 64-bit compare and four selects.
__device__ __forceinline__ u64 knn_min(u64 a, u64 b) {
  u64 r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ u64 knn_max(u64 a, u64 b) {
  u64 r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ u64 knn_key(float d, int j) {
  const u32 bits = __float_as_uint(d);
  return ((u64)(bits < 0x7F800000u ? bits : 0x7F800000u) << 32) | (u32)j;
}
template <int LO, int HI>
__device__ __forceinline__ void knn_cex(u64 *v) {
  const u64 a = v[LO], b = v[HI];
  v[LO] = knn_min(a, b);
  v[HI] = knn_max(a, b);
}
template <int KM, size_t... C>
__device__ __forceinline__ void knn_sort(u64 *v, std::index_sequence<C...>) {
  (knn_cex<KnnNets<KM>::sort.lo[C], KnnNets<KM>::sort.hi[C]>(v), ...);
}
// best (KM keys), batch (B keys): ascending.  best <- the KM smallest of both, ascending
template <int KM, size_t... C>
__device__ __forceinline__ void knn_merge(u64 *best, const u64 *batch, std::index_sequence<C...>) {
#pragma unroll
  for (int k = 0; k < KnnNets<KM>::B; k++) best[KM - 1 - k] = knn_min(best[KM - 1 - k], batch[k]);
  (knn_cex<KnnNets<KM>::merge.lo[C], KnnNets<KM>::merge.hi[C]>(best), ...);
}

// The thread index as a value the compiler knows nothing about, taken anew by every stage: what a stage derives from
// it (its loops' first addresses) is then computed in that stage and not kept in registers through all the others,
// where the k-NN stage needs them for its keys.
__device__ __forceinline__ void stage_tid(int &tid) {
  asm volatile("" : "+v"(tid));
  __builtin_assume(tid >= 0 && tid < SGTD_BUILD_THREADS);
}

struct BuildParams {
  const float *xyz;        // [total_kp*3]
  const u32 *label;        // [total_kp]
  const long long *kp_off; // [n_frames+1] device
  int n_frames;
  u32 frame_id0;
  int frame_id_step;       // 1: frame k gets frame_id0+k (map), 0: all frame_id0 (queries)
  long long out_stride;    // descriptor slots per frame
  u32 *out_count;          // [n_frames]
  int max_n;               // largest keypoint count in the batch (LDS layout)
  int max_slots;           // pow2 >= max_n*tpi + 1
  // global fallback for the dedup tables (LDS_DEDUP == false): per block
  u64 *ws_keys;            // [gridDim.x * max_n*tpi]
  u32 *ws_slots;           // [gridDim.x * max_slots]
};

// KM = slots of the k-NN best list and its networks, the smallest of {4, 8, 10, 12, 16} that holds
// descriptor_near_num (the shipped configuration is 10)
template <bool LDS_DEDUP, int KM>
__global__ __launch_bounds__(SGTD_BUILD_THREADS) void build_frames_kernel(
    BuildParams P, DevCfg cfg, DescArrays out) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int K = cfg.K, tpi = cfg.tpi;
  const int max_t = P.max_n * tpi;
  const int max_words = (max_t + 31) / 32;
  // LDS carve (all offsets multiples of 16 bytes)
  float4 *pts = reinterpret_cast<float4 *>(smem);
  size_t off = (size_t)P.max_n * 16;
  unsigned short *knn = reinterpret_cast<unsigned short *>(smem + off);
  off += (((size_t)P.max_n * K * 2) + 15) & ~(size_t)15;
  unsigned char *mn = smem + off;
  off += (((size_t)tpi * 2) + 15) & ~(size_t)15;
  u32 *winbits = reinterpret_cast<u32 *>(smem + off);
  off += (((size_t)max_words * 4) + 15) & ~(size_t)15;
  u32 *wordpre = reinterpret_cast<u32 *>(smem + off);
  off += (((size_t)(max_words + 1) * 4) + 15) & ~(size_t)15;
  u64 *keys;
  u32 *slots;
  if (LDS_DEDUP) {
    keys = reinterpret_cast<u64 *>(smem + off);
    off += (size_t)max_t * 8;
    slots = reinterpret_cast<u32 *>(smem + off);
  } else {
    keys = P.ws_keys + (size_t)blockIdx.x * max_t;
    slots = P.ws_slots + (size_t)blockIdx.x * P.max_slots;
  }
  int tid = threadIdx.x;

  // (m,n) rank pairs in loop order m = 1..K-2, n = m+1..K-1 (:193-194)
  if (tid == 0) {
    int k = 0;
    for (int m = 1; m < K - 1; m++)
      for (int n = m + 1; n < K; n++) {
        mn[2 * k] = (unsigned char)m;
        mn[2 * k + 1] = (unsigned char)n;
        k++;
      }
  }

  for (int f = blockIdx.x; f < P.n_frames; f += gridDim.x) {
    const long long kp0 = P.kp_off[f];
    const int n = (int)(P.kp_off[f + 1] - kp0);
    __syncthreads();
    if (n < K) {  // the reference indexes K neighbours regardless (UB): no descriptors
      if (tid == 0) P.out_count[f] = 0;
      continue;
    }
    const int T = n * tpi;
    int nslots = 64;
    while (nslots < T + 1) nslots <<= 1;
    const int nwords = (T + 31) / 32;

#ifdef SGTD_EXP_PHASE
    unsigned long long bph_t = __builtin_readcyclecounter();
#endif
    stage_tid(tid);
    // ---- stage 0: keypoints -> LDS
    for (int i = tid; i < n; i += SGTD_BUILD_THREADS) {
      float4 p;
      p.x = P.xyz[(kp0 + i) * 3 + 0];
      p.y = P.xyz[(kp0 + i) * 3 + 1];
      p.z = P.xyz[(kp0 + i) * 3 + 2];
      p.w = __uint_as_float(P.label[kp0 + i]);
      pts[i] = p;
    }
    for (int s = tid; s < nslots; s += SGTD_BUILD_THREADS) slots[s] = SGTD_SLOT_EMPTY;
    for (int w = tid; w < nwords; w += SGTD_BUILD_THREADS) winbits[w] = 0;
    __syncthreads();

    BPH(0);
    stage_tid(tid);
    // ---- stage 1: k-NN by selection networks in registers, on keys (distance bits, index): the
    // key order is (smaller distance, then lower index), whatever order the candidates come in.
    // Candidates go through B at a time: the batch is sorted by a network, then merged with the
    // best list (knn_merge).  Four threads share a keypoint: each selects among a quarter of the
    // candidates, parts 1..3 park their K best in the (not yet live) dedup-key area and part 0
    // merges the three sorted lists into its own.
    const int parts = (3 * K <= tpi) ? 4 : 1;   // the parking area is T*8 bytes = n*tpi*8
    const int per_pass = SGTD_BUILD_THREADS / parts;
    constexpr int B = KnnNets<KM>::B;
    constexpr auto sort_seq = std::make_index_sequence<KnnNets<KM>::sort.n_cex>();
    constexpr auto merge_seq = std::make_index_sequence<KnnNets<KM>::merge.n_cex>();
    for (int i0 = 0; i0 < n; i0 += per_pass) {
      const int i = i0 + tid / parts, part = tid % parts;
      u64 best[KM];
#pragma unroll
      for (int k = 0; k < KM; k++) best[k] = SGTD_KNN_EMPTY;
      if (i < n) {
        const float4 q = pts[i];
        const int j_lo = (int)((long long)n * part / parts), j_hi = (int)((long long)n * (part + 1) / parts);
        auto key_of = [&](int j) {
          const float4 p = pts[j];
          float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
          float d = dx * dx;   // FLANN L2_Simple accumulation order
          d += dy * dy;
          d += dz * dz;
          return knn_key(d, j);
        };
        int j0 = j_lo;
        for (; j0 + B <= j_hi; j0 += B) {
          u64 batch[B];
#pragma unroll
          for (int b = 0; b < B; b++) batch[b] = key_of(j0 + b);
          knn_sort<KM>(batch, sort_seq);
          knn_merge<KM>(best, batch, merge_seq);
        }
        if (j0 < j_hi) {   // the tail, padded with empty slots
          u64 batch[B];
#pragma unroll
          for (int b = 0; b < B; b++) {
            const u64 key = key_of(j0 + b < j_hi ? j0 + b : j_hi - 1);
            batch[b] = j0 + b < j_hi ? key : SGTD_KNN_EMPTY;
          }
          knn_sort<KM>(batch, sort_seq);
          knn_merge<KM>(best, batch, merge_seq);
        }
        if (part > 0) {
#pragma unroll
          for (int k = 0; k < KM; k++)
            if (k < K) keys[((size_t)i * 3 + (part - 1)) * K + k] = best[k];
        }
      }
      if (parts > 1) {
        if (!LDS_DEDUP) __threadfence_block();
        __syncthreads();
        if (i < n && part == 0) {
          for (int pp = 0; pp < 3; pp++) {   // the sorted lists of parts 1, 2, 3, B keys at a time
#pragma unroll
            for (int k0 = 0; k0 < KM; k0 += B) {
              u64 batch[B];
#pragma unroll
              for (int b = 0; b < B; b++)
                batch[b] = k0 + b < K ? keys[((size_t)i * 3 + pp) * K + k0 + b] : SGTD_KNN_EMPTY;
              knn_merge<KM>(best, batch, merge_seq);
            }
          }
        }
      }
      if (i < n && part == 0) {
#pragma unroll
        for (int k = 0; k < KM; k++)
          if (k < K) knn[i * K + k] = (unsigned short)(u32)best[k];
      }
      if (parts > 1) __syncthreads();   // the parking area is reused by the next pass
    }
    __syncthreads();

    BPH(1);
    stage_tid(tid);
    // ---- stage 2: keys of all triplets
    for (int t = tid; t < T; t += SGTD_BUILD_THREADS) {
      const int i = t / tpi, r = t - i * tpi;
      const int m = mn[2 * r], nn = mn[2 * r + 1];
      Tri tr = make_triangle(pts[i], pts[knn[i * K + m]], pts[knn[i * K + nn]], cfg);
      keys[t] = tr.valid ? milli_key(tr) : SGTD_TRI_INVALID;
    }
    if (!LDS_DEDUP) __threadfence_block();
    __syncthreads();

    BPH(2);
    stage_tid(tid);
    // ---- stage 3: first-wins dedup, slot value = min t of its key
    for (int t = tid; t < T; t += SGTD_BUILD_THREADS) {
      const u64 key = keys[t];
      if (key == SGTD_TRI_INVALID) continue;
      u32 h = (u32)mix64(key) & (u32)(nslots - 1);
      while (true) {
        u32 cur = atomicCAS(&slots[h], SGTD_SLOT_EMPTY, (u32)t);
        if (cur == SGTD_SLOT_EMPTY) break;
        if (keys[cur] == key) { atomicMin(&slots[h], (u32)t); break; }
        h = (h + 1) & (u32)(nslots - 1);
      }
    }
    __syncthreads();
    for (int s = tid; s < nslots; s += SGTD_BUILD_THREADS) {
      u32 v = slots[s];
      if (v != SGTD_SLOT_EMPTY) atomicOr(&winbits[v >> 5], 1u << (v & 31));
    }
    __syncthreads();
    // exclusive prefix of popcounts over the winner bitmap (wave 0)
    if (tid < SGTD_WAVE) {
      u32 carry = 0;
      for (int w0 = 0; w0 < nwords; w0 += SGTD_WAVE) {
        int w = w0 + tid;
        u32 c = (w < nwords) ? __popc(winbits[w]) : 0;
        u32 inc = wave_incl_scan(c);
        if (w < nwords) wordpre[w] = carry + inc - c;
        carry += __shfl(inc, SGTD_WAVE - 1);
      }
      if (tid == 0) { wordpre[nwords] = carry; P.out_count[f] = carry; }
    }
    __syncthreads();
    // the winners' triplet indices in rank order, in the key array (dead since the dedup): the fill
    // then runs on full waves instead of skipping the losers' lanes
    u32 *winners = reinterpret_cast<u32 *>(keys);
    for (int t = tid; t < T; t += SGTD_BUILD_THREADS) {
      const u32 word = winbits[t >> 5];
      if ((word >> (t & 31)) & 1u) winners[wordpre[t >> 5] + __popc(word & ((1u << (t & 31)) - 1u))] = (u32)t;
    }
    if (!LDS_DEDUP) __threadfence_block();
    __syncthreads();

    BPH(3);
    stage_tid(tid);
    // ---- stage 4: descriptor fill in (i,m,n) order of the surviving triplets
    const u32 frame_id = P.frame_id0 + (u32)(P.frame_id_step * f);
    const u32 n_win = wordpre[nwords];
    for (u32 rank = tid; rank < n_win; rank += SGTD_BUILD_THREADS) {
      const int t = (int)winners[rank];
      const int i = t / tpi, r = t - i * tpi;
      const int m = mn[2 * r], nn = mn[2 * r + 1];
      float4 p[3];
      p[0] = pts[i]; p[1] = pts[knn[i * K + m]]; p[2] = pts[knn[i * K + nn]];
      const Tri tr = make_triangle(p[0], p[1], p[2], cfg);
      const float4 A = tr.va == 0 ? p[0] : (tr.va == 1 ? p[1] : p[2]);
      const float4 B = tr.vb == 0 ? p[0] : (tr.vb == 1 ? p[1] : p[2]);
      const float4 C = tr.vc == 0 ? p[0] : (tr.vc == 1 ? p[1] : p[2]);
      const size_t o = (size_t)f * P.out_stride + rank;
      const double a = tr.a, b = tr.b, c = tr.c;
      out.side[o * 3 + 0] = cfg.scale * a;
      out.side[o * 3 + 1] = cfg.scale * b;
      out.side[o * 3 + 2] = cfg.scale * c;
      out.angle[o * 3 + 0] = fabs((b * b + c * c - a * a) / (2 * b * c));  // :299-301
      out.angle[o * 3 + 1] = fabs((a * a + c * c - b * b) / (2 * a * c));
      out.angle[o * 3 + 2] = fabs((a * a + b * b - c * c) / (2 * a * b));
      out.center[o * 3 + 0] = (((double)A.x + (double)B.x) + (double)C.x) / 3;  // :296
      out.center[o * 3 + 1] = (((double)A.y + (double)B.y) + (double)C.y) / 3;
      out.center[o * 3 + 2] = (((double)A.z + (double)B.z) + (double)C.z) / 3;
      out.vertex[o * 9 + 0] = A.x; out.vertex[o * 9 + 1] = A.y; out.vertex[o * 9 + 2] = A.z;
      out.vertex[o * 9 + 3] = B.x; out.vertex[o * 9 + 4] = B.y; out.vertex[o * 9 + 5] = B.z;
      out.vertex[o * 9 + 6] = C.x; out.vertex[o * 9 + 7] = C.y; out.vertex[o * 9 + 8] = C.z;
      // vertex_attached_ holds the u32 label as a double; (int) of it is what
      // AddSTDescs / candidate_selector use (:158-160,362-364)
      out.label[o * 3 + 0] = (int)(double)__float_as_uint(A.w);
      out.label[o * 3 + 1] = (int)(double)__float_as_uint(B.w);
      out.label[o * 3 + 2] = (int)(double)__float_as_uint(C.w);
      out.frame[o] = frame_id;
      if (out.qrec) write_query_rec(out.qrec + o, cfg.scale * a, cfg.scale * b, cfg.scale * c, cfg.rough, frame_id);
      out.node_id[o * 3 + 0] = i; out.node_id[o * 3 + 1] = m; out.node_id[o * 3 + 2] = nn;
    }
#ifdef SGTD_EXP_PHASE
    __syncthreads();
    BPH(4);
#endif
  }
}

// LDS bytes the kernel carves for a batch whose largest frame has max_n keypoints
static inline size_t build_lds_bytes(int max_n, int K, int tpi, bool lds_dedup, int max_slots) {
  size_t max_t = (size_t)max_n * tpi, words = (max_t + 31) / 32;
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  size_t b = (size_t)max_n * 16 + up((size_t)max_n * K * 2) + up((size_t)tpi * 2) +
             up(words * 4) + up((words + 1) * 4);
  if (lds_dedup) b += max_t * 8 + (size_t)max_slots * 4;
  return b;
}
