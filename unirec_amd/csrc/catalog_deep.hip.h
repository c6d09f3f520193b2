// The selection kernels of ur_catalog_deep_select (include/unirec_hip_deep.h): lists of up to 1024 items per user.  Included by
// catalog.hip, where the scoring launches live; the total order, the exclude rule and the tile size are those of catalog_select.hip.h.
//
// What differs from catalog_select_kernel:
//   * the merge is deferred.  Survivors of successive tiles pile up behind the list in an LDS buffer of DEEP_CAP entries, and list +
//     survivors are sorted only when the buffer could not take one more tile in which EVERY score passes (m + SEL_TILE > DEEP_CAP: the
//     worst case, not the average), and at the end of the workgroup's segment.  Between merges the threshold (the list's K-th entry as of
//     the last merge) is stale; a stale threshold is a weaker one, so it admits every item the fresh one would and the merged list is
//     the same.  At K = 1024 and random scores a user takes about K (1 + ln(N / K)) = 8 000 insertions over 1 000 tiles of a million-row
//     catalogue: a merge per tile with a survivor is ~1 000 sorts of 2048 entries, a deferred merge one sort of 4096 per ~3 000 survivors.
//   * G workgroups share a user's chunk row, each on a contiguous run of tiles with a list of its own in the workspace; a last kernel
//     merges the G lists and adds the G counts.  64 users alone would occupy a quarter of the compute units.
// LDS: 2 x 4 x DEEP_CAP = 32 KB per workgroup of 256 threads, five workgroups per compute unit of 160 KB.  The sort's compare-exchange
// pairs are dealt one per thread and step (pair p -> i = p with a zero bit inserted at the stride's position, q = i | stride), so no
// thread idles; at strides >= 32 a wave's 64 pairs are 64 consecutive words on either side (conflict-free), below that a ds_read_b32
// half-wave lands two-way on the 32 banks.
#pragma once
#include "catalog_select.hip.h"
#include "unirec_hip_deep.h"

namespace {

constexpr int DEEP_CAP = 4096;                 // entries of the sweep's LDS buffer, a power of two
constexpr int DEEP_MERGE_MAX = 2048;           // entries of the final merge: two lists, a power of two
static_assert(UR_CATALOG_DEEP_TOPK_MAX + SEL_TILE <= DEEP_CAP, "a list and one tile in which every score passes must fit the buffer");
static_assert(2 * UR_CATALOG_DEEP_TOPK_MAX <= DEEP_MERGE_MAX, "two lists must fit the final merge");

// bitonic sort of ks / ki [0, P) under the total order, best first; P a power of two >= 2; 256 threads.  The caller has made the P
// entries visible (a barrier); the sort ends on a barrier.
__device__ __forceinline__ void deep_sort(float* ks, int* ki, int P, int tid) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = tid; p < (P >> 1); p += 256) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), q = i | j;
        const float si = ks[i], sq = ks[q];
        const int ii = ki[i], iq = ki[q];
        const bool up = (i & k) == 0;                              // this pair ends in list order (best first)
        if (up ? sel_before(sq, iq, si, ii) : sel_before(si, ii, sq, iq)) { ks[i] = sq; ki[i] = iq; ks[q] = si; ki[q] = ii; }
      }
      __syncthreads();
    }
  }
}

// Workgroup (b, g) = blockIdx.x = b G + g folds the scores chunk[b][g seg_len .. (g + 1) seg_len) (catalogue rows c0 + ..; seg_len a
// multiple of SEL_TILE) into its running list (list_score / list_index [B, G, K]: sorted, empty slots = (-inf, SEL_EMPTY)) and into
// count[b][g] = #{non-excluded n of its segments so far : s_bn > ref[b]}.
__global__ __launch_bounds__(256) void catalog_deep_sweep_kernel(const float* __restrict__ chunk, long ld, int c0, int len, int K, int G,
                                                                 long seg_len, float* __restrict__ list_score, int* __restrict__ list_index,
                                                                 int* __restrict__ count, const long* __restrict__ gt,
                                                                 const float* __restrict__ ref, const long* __restrict__ exclude, int E,
                                                                 int first) {
  __shared__ float ks[DEEP_CAP];
  __shared__ int ki[DEEP_CAP];
  __shared__ int n_surv[3];      // survivor counter of tile t = n_surv[t % 3] (see the sweep)
  __shared__ int part[4];
  const int b = blockIdx.x / G, g = blockIdx.x - b * G, tid = threadIdx.x;
  const long s0 = (long)g * seg_len;
  const int t_begin = (int)(s0 < (long)len ? s0 : (long)len);
  const int t_end = (int)(s0 + seg_len < (long)len ? s0 + seg_len : (long)len);
  if (!first && t_begin >= t_end) return;                          // nothing of this chunk is ours: list and count stay (uniform)
  const float ninf = -__builtin_inff();
  const long slot = (long)blockIdx.x * K;
  for (int i = tid; i < K; i += 256) {
    ks[i] = first ? ninf : list_score[slot + i];
    ki[i] = first ? SEL_EMPTY : list_index[slot + i];
  }
  if (tid == 0) n_surv[0] = 0;
  __syncthreads();
  float thr_s = ks[K - 1];
  int thr_i = ki[K - 1];
  const bool has_gt = gt != nullptr;
  const long gb = has_gt ? gt[b] : -1L;
  const float rf = has_gt ? ref[b] : 0.f;
  const long* ex = E > 0 ? exclude + (long)b * E : nullptr;
  const float* row = chunk + (long)b * ld;
  int cnt = 0;
  int m = K;                     // entries of the buffer in use: the list and the survivors since the last merge (uniform)
  // One barrier per tile without a merge: a thread may start appending to the next tile's counter while another still reads this
  // tile's, so the counters rotate.  Thread 0 clears the NEXT tile's counter during this tile's sweep: that counter was last read
  // two tiles ago, before the previous tile's barrier, and is first added to after this tile's.
  int cur = 0;
  for (int t0 = t_begin; t0 < t_end; t0 += SEL_TILE) {
    const int nxt = cur == 2 ? 0 : cur + 1;
    if (tid == 0) n_surv[nxt] = 0;
#pragma unroll
    for (int j = 0; j < SEL_TILE / 256; ++j) {
      const int n = t0 + j * 256 + tid;
      if (n < t_end) {
        const float s = row[n];
        const int idx = c0 + n;
        const bool pass = sel_before(s, idx, thr_s, thr_i);
        const bool above = has_gt && s > rf;
        if (pass || above) {
          const bool out = E > 0 && (long)idx != gb && sel_excluded(ex, E, (long)idx);
          if (!out) {
            cnt += above ? 1 : 0;
            if (pass) {
              const int pos = m + atomicAdd(&n_surv[cur], 1);        // < m + SEL_TILE <= DEEP_CAP
              ks[pos] = s; ki[pos] = idx;
            }
          }
        }
      }
    }
    __syncthreads();
    m += n_surv[cur];                                                // uniform
    cur = nxt;
    const bool last = t0 + SEL_TILE >= t_end;
    if (m > K && (last || m + SEL_TILE > DEEP_CAP)) {
      int P = 2;
      while (P < m) P <<= 1;
      for (int i = m + tid; i < P; i += 256) { ks[i] = ninf; ki[i] = SEL_EMPTY; }
      __syncthreads();
      deep_sort(ks, ki, P, tid);
      thr_s = ks[K - 1]; thr_i = ki[K - 1];
      m = K;
    }
  }
  for (int i = tid; i < K; i += 256) {
    list_score[slot + i] = ks[i];
    list_index[slot + i] = ki[i];
  }
  if (has_gt) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) part[wave] = cnt;
    __syncthreads();
    if (tid == 0) count[blockIdx.x] = (first ? 0 : count[blockIdx.x]) + part[0] + part[1] + part[2] + part[3];
  }
}

// One workgroup per user, after the last chunk: the G sorted lists of the user merged under the total order, one at a time behind
// the running result (a sort of 2 K entries each), the first K written out with empty slots as (-1, -inf); rank = 1 + the G counts.
__global__ __launch_bounds__(256) void catalog_deep_merge_kernel(const float* __restrict__ list_score, const int* __restrict__ list_index,
                                                                 const int* __restrict__ count, int K, int G, float* __restrict__ topk_score,
                                                                 int* __restrict__ topk_index, int* __restrict__ rank) {
  __shared__ float ks[DEEP_MERGE_MAX];
  __shared__ int ki[DEEP_MERGE_MAX];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long base = (long)b * G * K;
  for (int i = tid; i < K; i += 256) { ks[i] = list_score[base + i]; ki[i] = list_index[base + i]; }
  int P = 2;
  while (P < 2 * K) P <<= 1;
  for (int g = 1; g < G; ++g) {
    for (int i = tid; i < K; i += 256) { ks[K + i] = list_score[base + (long)g * K + i]; ki[K + i] = list_index[base + (long)g * K + i]; }
    for (int i = 2 * K + tid; i < P; i += 256) { ks[i] = -__builtin_inff(); ki[i] = SEL_EMPTY; }
    __syncthreads();
    deep_sort(ks, ki, P, tid);
  }
  __syncthreads();
  for (int i = tid; i < K; i += 256) {
    topk_score[(long)b * K + i] = ks[i];
    topk_index[(long)b * K + i] = ki[i] == SEL_EMPTY ? -1 : ki[i];
  }
  if (rank != nullptr && tid == 0) {
    int r = 1;
    for (int g = 0; g < G; ++g) r += count[b * G + g];
    rank[b] = r;
  }
}

// workgroups per user's chunk row.  The workspace is laid out for deep_segments_cap (catalog_layout.hip.h);
// the launch takes no more than that, than ~4 workgroups per compute unit in all, and than the chunk has tiles.  Measured at a million
// rows and K = 1000 (docs/lab_notes.md section 37): 2 is the best count at 512 users and 8 at 64; 16 at 64 users is 4 % slower again
// (every list is filled, written back per chunk and merged at the end), so the library stops at DEEP_SEGMENTS_AUTO.
static_assert(DEEP_SEGMENTS_AUTO <= UR_CATALOG_DEEP_SEGMENTS_MAX, "the library's own choice is one a caller may force");
int deep_segments(int32_t segments, int32_t B, int64_t rows) {
  if (segments > 0) return segments;
  int64_t g = deep_segments_cap(0, B);
  const int64_t by_cu = 4 * (int64_t)ur_device_cu_count() / (B > 0 ? B : 1), tiles = rows / SEL_TILE;
  if (g > by_cu) g = by_cu;
  if (g > tiles) g = tiles;
  return g < 1 ? 1 : (int)g;
}

// ---- the sorting launch of the long re-ranks (ur_catalog_deep_rerank, ur_catalog_funnel_rerank in catalog_coarse.hip; ur_catalog_fp8_rerank
// in catalog_fp8.hip) ------------------------------------------------------------------------------------------------------------------
// One workgroup per user loads its K_in (score, index) pairs into LDS, pads them to the next power of two with empty slots, sorts them
// with deep_sort and writes the first k.  The scoring launches that feed it are described where they live.
constexpr int DR_SLOTS = UR_CATALOG_DEEP_TOPK_MAX;
constexpr int DR_GRID_Y_MAX = 65535;
static_assert((DR_SLOTS & (DR_SLOTS - 1)) == 0 && DR_SLOTS >= UR_CATALOG_TOPK_MAX, "the sort takes a power of two; the short lists are a subset");
__global__ __launch_bounds__(256) void catalog_deep_rerank_sort_kernel(const float* __restrict__ score, const int* __restrict__ index, int K_in,
                                                                       int k, int* __restrict__ topk_index, float* __restrict__ topk_score,
                                                                       long N) {
  __shared__ float ks[DR_SLOTS];
  __shared__ int ki[DR_SLOTS];
  const int b = blockIdx.x, tid = threadIdx.x;
  int P = 2;
  while (P < K_in) P <<= 1;                                              // <= DR_SLOTS: K_in <= UR_CATALOG_DEEP_TOPK_MAX is checked
  for (int i = tid; i < P; i += 256) {
    float s = -__builtin_inff();
    int id = SEL_EMPTY;
    if (i < K_in) {
      const int g = index[(long)b * K_in + i];
      if (g >= 0 && (long)g < N) { s = score[(long)b * K_in + i]; id = g; }
    }
    ks[i] = s; ki[i] = id;
  }
  __syncthreads();
  deep_sort(ks, ki, P, tid);
  for (int i = tid; i < k; i += 256) {
    topk_score[(long)b * k + i] = ks[i];
    topk_index[(long)b * k + i] = ki[i] == SEL_EMPTY ? -1 : ki[i];
  }
}

}  // namespace
