// What the catalogue translation units share (catalog.hip: the exact scorers and the softmax loss; catalog_coarse.hip: the bf16-MFMA
// shortlist pass and the exact re-rank).  Device side: the catalogue element loads, the row norms, the total order of the lists and the
// streaming selection kernel.  Host side: the argument checks every entry point makes (catalog_call), the f32 / bf16 dispatch and the
// chunk loop; the workspaces are in catalog_layout.hip.h.  Everything here has internal linkage; each unit compiles its own copy of
// the same text.
#pragma once
#include "common.hip.h"
#include "unirec_hip.h"
#include "unirec_hip_funnel.h"
#include "catalog_layout.hip.h"

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

// The row norms of L prefixes in one read (ur_catalog_prefix_norms, and the norm planes of ur_catalog_mrl_softmax).
// row_inv_norm_kernel's chain: lane j adds the squares of its pieces at d = 4 j + 256 i in ascending i.  The sum a lane holds after its
// last piece below dims[l] is that chain on the slice [:dims[l]] (dims are multiples of 4: a piece lies wholly on one side of a
// boundary), so the lane keeps it as plane l's snapshot; a lane with no piece below the boundary keeps 0, as the short loop does.  Each
// snapshot is folded by the same wave_sum and finished by the same expression.
struct prefix_dims {
  int d[UR_FUNNEL_MAX_DIMS];
};
template <typename CT>
__global__ void row_prefix_inv_norm_kernel(const CT* __restrict__ x, long ld, float* __restrict__ inv, long rows, prefix_dims dims, int L) {
  const long row = (long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const CT* p = x + row * ld;
  const int D = dims.d[L - 1];
  float s = 0.f;
  float snap[UR_FUNNEL_MAX_DIMS];
#pragma unroll
  for (int l = 0; l < UR_FUNNEL_MAX_DIMS; ++l) snap[l] = 0.f;
  for (int d = lane * 4; d < D; d += 256) {
    const float4 v = load4(p + d);
    s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
#pragma unroll
    for (int l = 0; l < UR_FUNNEL_MAX_DIMS; ++l)
      if (l < L && d < dims.d[l]) snap[l] = s;
  }
#pragma unroll
  for (int l = 0; l < UR_FUNNEL_MAX_DIMS; ++l) {
    if (l < L) {                                                       // (uniform)
      const float t = wave_sum(snap[l]);
      if (lane == 0) inv[(long)l * rows + row] = 1.0f / fmaxf(sqrtf(t), 1e-12f);
    }
  }
}

// The total order of the lists: score descending, index ascending.  An empty slot is (-inf, SEL_EMPTY): it follows every item.
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

// ---- host side --------------------------------------------------------------------------------------------------------------------
// What every catalogue entry point takes and checks the same way; each fills it from its own argument struct (a field it does not
// have stays zero, which passes).  K, segments, temperature and the outputs are the entry point's own business.
struct catalog_call {
  const char* who;
  int32_t B;
  int64_t N;
  int32_t D, E;
  int64_t chunk_rows;
  int32_t catalog_bf16, scorer;
  const void *gt, *rank, *exclude, *user, *catalog, *cat_inv_norm, *workspace;
  int64_t workspace_bytes;
};

// the checks of the sizes and flags, all before the size query answers.  d_mult: what D must be a multiple of; n_min: the smallest
// catalogue (0 or 1); gt_needed: the entry point has no rank output and takes gt_index unconditionally (checked with the operands)
int catalog_check_sizes(const catalog_call& c, int d_mult, int64_t n_min, bool gt_needed) {
  UR_REQUIRE(c.B >= 0, "%s: need B >= 0 (got %d)", c.who, c.B);
  UR_REQUIRE(c.N >= n_min && c.N <= (int64_t)INT32_MAX, "%s: need %lld <= N <= INT32_MAX (got %lld)", c.who, (long long)n_min, (long long)c.N);
  UR_REQUIRE(c.D > 0 && (c.D % d_mult) == 0 && c.D <= 2048, "%s: D must be a positive multiple of %d and <= 2048 (got %d)", c.who, d_mult, c.D);
  UR_REQUIRE(c.chunk_rows >= 0 && (c.chunk_rows % SEL_TILE) == 0, "%s: chunk_rows must be 0 or a positive multiple of %d (got %lld)", c.who,
             SEL_TILE, (long long)c.chunk_rows);
  UR_REQUIRE(c.E >= 0 && (c.E == 0 || c.exclude), "%s: E > 0 needs exclude", c.who);
  UR_REQUIRE(gt_needed || (c.gt != nullptr) == (c.rank != nullptr), "%s: gt_index and rank go together", c.who);
  UR_REQUIRE(c.catalog_bf16 == 0 || c.catalog_bf16 == 1, "%s: catalog_bf16 must be 0 or 1 (got %d)", c.who, c.catalog_bf16);
  UR_REQUIRE(c.scorer >= 0 && c.scorer <= UR_CATALOG_SCORER_MFMA, "%s: scorer must be 0 (the library chooses), 1 (vector) or 2 (f32 MFMA) (got %d)",
             c.who, c.scorer);
  return 0;
}

// the checks of a call that brings its workspace (`need` bytes, from the layout): the workspace, then -- unless B == 0, when the call
// is a no-op that needs no buffer -- the operands
int catalog_check_buffers(const catalog_call& c, int64_t need, bool gt_needed) {
  UR_REQUIRE(UR_ALIGNED16(c.workspace) && c.workspace_bytes >= need, "%s: workspace must be 16-byte aligned and hold %lld bytes (got %lld)", c.who,
             (long long)need, (long long)c.workspace_bytes);
  if (c.B == 0) return 0;
  UR_REQUIRE(c.user && (c.N == 0 || (c.catalog && c.cat_inv_norm)) && (!gt_needed || c.gt), "%s: user / catalog / cat_inv_norm / gt_index: null pointer",
             c.who);
  UR_REQUIRE(UR_ALIGNED16(c.user) && UR_ALIGNED16(c.catalog), "%s: user and catalog must be 16-byte aligned", c.who);
  return 0;
}

// f(catalogue as const float* or const bf16_t*): the one place the catalog_bf16 flag becomes a type
template <typename F>
int catalog_dispatch(bool bf16, const void* catalog, F&& f) {
  return bf16 ? f((const bf16_t*)catalog) : f((const float*)catalog);
}

// body(c0, len, first) per chunk of `rows` catalogue rows, until one returns non-zero.  N == 0 still makes one pass, with len == 0:
// the selection launch of that pass writes the empty lists.
template <typename F>
int catalog_for_each_chunk(int64_t N, int64_t rows, F&& body) {
  int64_t c0 = 0;
  do {
    const int64_t len = N - c0 < rows ? N - c0 : rows;
    const int rc = body(c0, len, (int)(c0 == 0));
    if (rc != 0) return rc;
    c0 += rows;
  } while (c0 < N);
  return 0;
}

}  // namespace
