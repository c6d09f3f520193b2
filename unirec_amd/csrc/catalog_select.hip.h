// What the catalogue translation units share (catalog.hip: the exact scorers and the softmax loss; catalog_coarse.hip: the bf16-MFMA
// shortlist pass and the exact re-rank): the catalogue element loads, the row norms, the total order of the lists and the streaming
// selection kernel with its chunk-size rule.  Everything here has internal linkage; each unit compiles its own copy of the same text.
#pragma once
#include "common.hip.h"
#include "unirec_hip.h"

namespace {

// Catalogue element loads: the kernels below are templated on the stored type CT (float or bf16_t) and differ in nothing but these.
// bf16 -> f32 is a 16-bit shift, exact, so a bf16 catalogue scores bit for bit as its .float() copy does.
__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 load4(const bf16_t* p) {
  const uint2 v = *reinterpret_cast<const uint2*>(p);
  return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u));
}

template <typename CT>
__global__ void row_inv_norm_kernel(const CT* __restrict__ x, float* __restrict__ inv, long rows, int D) {
  const long row = (long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const CT* p = x + row * D;
  float s = 0.f;
  for (int d = lane * 4; d < D; d += 256) {
    const float4 v = load4(p + d);
    s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  s = wave_sum(s);
  if (lane == 0) inv[row] = 1.0f / fmaxf(sqrtf(s), 1e-12f);
}

// The total order of the lists: score descending, index ascending.  An empty slot is (-inf, SEL_EMPTY): it follows every item.
constexpr int SEL_TILE = 1024;                 // scores per sweep step: 4 per thread
constexpr int SEL_SORT_MAX = 2048;             // >= UR_CATALOG_TOPK_MAX + SEL_TILE, a power of two
constexpr int SEL_EMPTY = 0x7fffffff;
static_assert(UR_CATALOG_TOPK_MAX + SEL_TILE <= SEL_SORT_MAX, "list + one tile of survivors must fit the sort buffer");
__device__ __forceinline__ bool sel_before(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }
// n in the ascending row ex[0..E)?
__device__ __forceinline__ bool sel_excluded(const long* __restrict__ ex, int E, long n) {
  int lo = 0, hi = E;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ex[mid] < n) lo = mid + 1; else hi = mid;
  }
  return lo < E && ex[lo] == n;
}

// One workgroup per user folds one chunk of scores (chunk[b][0..len), catalogue rows c0 .. c0+len) into the user's running list
// (topk_score / topk_index [B,K]: sorted, empty slots = (-inf, -1)) and into rank[b] = 1 + #{non-excluded n : s_bn > ref[b]}.
// Per tile every score is compared with the list's K-th entry; what passes and is not excluded is appended behind the list in LDS
// through an LDS counter, and a tile that appended anything is merged by a bitonic sort of list + survivors under the total order
// (so the result does not depend on the order of the appends).  A tile without survivors costs its read and compares.
__global__ __launch_bounds__(256) void catalog_select_kernel(const float* __restrict__ chunk, long ld, int c0, int len, int K,
                                                             float* __restrict__ topk_score, int* __restrict__ topk_index,
                                                             const long* __restrict__ gt, const float* __restrict__ ref, int* __restrict__ rank,
                                                             const long* __restrict__ exclude, int E, int first) {
  __shared__ float ks[SEL_SORT_MAX];
  __shared__ int ki[SEL_SORT_MAX];
  __shared__ int n_surv[3];      // survivor counter of tile t = n_surv[t % 3] (see the sweep)
  __shared__ int part[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float ninf = -__builtin_inff();
  if (tid < K) {
    float s = ninf;
    int i = SEL_EMPTY;
    if (!first) {
      s = topk_score[(long)b * K + tid];
      i = topk_index[(long)b * K + tid];
      if (i < 0) i = SEL_EMPTY;
    }
    ks[tid] = s; ki[tid] = i;
  }
  if (tid == 0) n_surv[0] = 0;
  __syncthreads();
  float thr_s = ks[K - 1];
  int thr_i = ki[K - 1];
  const bool has_gt = gt != nullptr;
  const long g = has_gt ? gt[b] : -1L;
  const float rf = has_gt ? ref[b] : 0.f;
  const long* ex = E > 0 ? exclude + (long)b * E : nullptr;
  const float* row = chunk + (long)b * ld;
  int cnt = 0;
  // One barrier per tile without survivors: a thread may start appending to the next tile's counter while another still reads this
  // tile's, so the counters rotate.  Thread 0 clears the NEXT tile's counter during this tile's sweep: that counter was last read
  // two tiles ago, before the previous tile's barrier, and is first added to after this tile's.
  int cur = 0;
  for (int t0 = 0; t0 < len; t0 += SEL_TILE) {
    const int nxt = cur == 2 ? 0 : cur + 1;
    if (tid == 0) n_surv[nxt] = 0;
#pragma unroll
    for (int j = 0; j < SEL_TILE / 256; ++j) {
      const int n = t0 + j * 256 + tid;
      if (n < len) {
        const float s = row[n];
        const int idx = c0 + n;
        const bool pass = sel_before(s, idx, thr_s, thr_i);
        const bool above = has_gt && s > rf;
        if (pass || above) {
          const bool out = E > 0 && (long)idx != g && sel_excluded(ex, E, (long)idx);
          if (!out) {
            cnt += above ? 1 : 0;
            if (pass) {
              const int pos = K + atomicAdd(&n_surv[cur], 1);          // < K + SEL_TILE <= SEL_SORT_MAX
              ks[pos] = s; ki[pos] = idx;
            }
          }
        }
      }
    }
    __syncthreads();
    const int m = K + n_surv[cur];                                // uniform
    cur = nxt;
    if (m > K) {
      int P = 2;
      while (P < m) P <<= 1;
      for (int i = m + tid; i < P; i += 256) { ks[i] = ninf; ki[i] = SEL_EMPTY; }
      __syncthreads();
      for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int i = tid; i < P; i += 256) {
            const int q = i ^ j;
            if (q > i) {
              const float si = ks[i], sq = ks[q];
              const int ii = ki[i], iq = ki[q];
              const bool up = (i & k) == 0;                        // this pair ends in list order (best first)
              if (up ? sel_before(sq, iq, si, ii) : sel_before(si, ii, sq, iq)) { ks[i] = sq; ki[i] = iq; ks[q] = si; ki[q] = ii; }
            }
          }
          __syncthreads();
        }
      }
      thr_s = ks[K - 1]; thr_i = ki[K - 1];
    }
  }
  if (tid < K) {
    topk_score[(long)b * K + tid] = ks[tid];
    topk_index[(long)b * K + tid] = ki[tid] == SEL_EMPTY ? -1 : ki[tid];
  }
  if (has_gt) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) part[wave] = cnt;
    __syncthreads();
    if (tid == 0) rank[b] = (first ? 1 : rank[b]) + part[0] + part[1] + part[2] + part[3];
  }
}

// rows per chunk of the streaming mode: the caller's figure, or a chunk buffer [B, rows] near 64 MB (so that it can stay in the
// Infinity Cache between the scoring and the selection launch); never more than N rounded up to the selection tile
static int64_t catalog_chunk_rows(int64_t chunk_rows, int32_t B, int64_t N) {
  const int64_t n_up = (N + SEL_TILE - 1) / SEL_TILE * SEL_TILE;
  int64_t r = chunk_rows;
  if (r <= 0) r = ((int64_t)64 << 20) / (4 * (int64_t)(B > 0 ? B : 1)) / SEL_TILE * SEL_TILE;
  if (r > n_up) r = n_up;
  if (r > ((int64_t)1 << 30)) r = (int64_t)1 << 30;           // the selection kernel indexes a chunk with an int
  if (r < SEL_TILE) r = SEL_TILE;
  return r;
}

}  // namespace
