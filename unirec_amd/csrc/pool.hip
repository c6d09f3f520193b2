// The pooling family (include/unirec_hip_pool.h): the decoder's final RMSNorm fused with a mask-aware pooling rule (masked mean / last
// valid token), forward and backward.  HBM-bound row reductions: one wave owns a row (D <= 2048: the row sits in registers, 16 bytes per
// lane and load), its two reductions are wave-64 shuffles, rows whose pooling weight is 0 are never loaded.  No floating-point atomics:
// every sum has one fixed order (the header states it).  gfx950 only.
#include "common.hip.h"
#include "unirec_hip.h"
#include "unirec_hip_pool.h"

namespace {

constexpr int PN_SLICES = UR_POOL_NORM_SLICES;
constexpr int PN_WAVES = 4;             // waves (= rows in flight) per block
constexpr int PN_BWD_BLOCKS = 1024;     // grid cap of the backward: from 4096 rows on, a wave strides over rows

__device__ __forceinline__ void un8(const uint4& u, float (&f)[8]) {
  f[0] = bf_lo(u.x); f[1] = bf_hi(u.x); f[2] = bf_lo(u.y); f[3] = bf_hi(u.y);
  f[4] = bf_lo(u.z); f[5] = bf_hi(u.z); f[6] = bf_lo(u.w); f[7] = bf_hi(u.w);
}
__device__ __forceinline__ uint4 pk8(const float (&f)[8]) {
  return make_uint4(pack_bf2(f[0], f[1]), pack_bf2(f[2], f[3]), pack_bf2(f[4], f[5]), pack_bf2(f[6], f[7]));
}
__device__ __forceinline__ void ld8f(const float* p, float (&f)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
__device__ __forceinline__ void st8f(float* p, const float (&f)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// Lane l owns the elements 8 (l + 64 i) .. + 7 of a row, i < NCH; chunks at or beyond D hold zeros and are never stored.
template <int NCH>
__device__ __forceinline__ void pn_load_row(const bf16_t* rowp, int lane, int D, uint4 (&raw)[NCH]) {
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int e0 = (lane + i * 64) * 8;
    raw[i] = e0 < D ? *reinterpret_cast<const uint4*>(rowp + e0) : make_uint4(0u, 0u, 0u, 0u);
  }
}
template <int NCH>
__device__ __forceinline__ void pn_load_f32(const float* p, int lane, int D, float (&f)[NCH][8]) {
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int e0 = (lane + i * 64) * 8;
    if (e0 < D) {
      ld8f(p + e0, f[i]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[i][e] = 0.f;
    }
  }
}
// v = the row in f32; returns rstd = rsqrt(mean(x^2) + eps)
template <int NCH>
__device__ __forceinline__ float pn_rstd(const uint4 (&raw)[NCH], float (&v)[NCH][8], int D, float eps) {
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    un8(raw[i], v[i]);
#pragma unroll
    for (int e = 0; e < 8; ++e) q += v[i][e] * v[i][e];
  }
  return rsqrtf(wave_sum(q) / (float)D + eps);
}
// acc += w * (x * rstd) for one row
template <int NCH>
__device__ __forceinline__ void pn_accumulate(const uint4 (&raw)[NCH], const float (&ww)[NCH][8], float (&acc)[NCH][8], int D, float eps) {
  float v[NCH][8];
  const float rs = pn_rstd<NCH>(raw, v, D, eps);
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[i][e] += ww[i][e] * (v[i][e] * rs);
}

// the last valid position of a mask row (-1: none); every lane returns it
__device__ __forceinline__ int pn_last_valid(const uint8_t* m, int S, int lane) {
  int best = -1;
  for (int s = lane; s < S; s += 64)
    if (m[s]) best = s;
  return wave_max_i(best);
}

// ---- MASKED_MEAN forward, stage 1: block (b, slice) sums y over the valid rows of its slice.  Wave v takes the rows v, v + 4, .. of the
// slice, two per trip so that two rows' loads are in flight; the waves are added 0 + 1 + 2 + 3 through LDS.  Every (b, slice) slot of
// `part` and `cnt` is written, the empty slices with zeros.
template <int NCH>
__global__ __launch_bounds__(PN_WAVES * 64) void pn_mean_stage1(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                               const uint8_t* __restrict__ mask, float* __restrict__ part,
                                                               int* __restrict__ cnt, int S, int D, int per, float eps) {
  __shared__ __attribute__((aligned(16))) float red[PN_WAVES - 1][NCH * 64 * 8];
  __shared__ int nred[PN_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long b = blockIdx.x / PN_SLICES;
  const int sl = blockIdx.x % PN_SLICES;
  const int s0 = sl * per, s1 = min(S, s0 + per);
  const bf16_t* xb = x + b * S * D;
  const uint8_t* mb = mask ? mask + b * S : nullptr;
  float ww[NCH][8], acc[NCH][8];
  pn_load_f32<NCH>(w, lane, D, ww);
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;
  int n = 0;
  for (int s = s0 + wave; s < s1; s += 2 * PN_WAVES) {
    const int t = s + PN_WAVES;
    const bool va = !mb || mb[s] != 0;
    const bool vb = t < s1 && (!mb || mb[t] != 0);
    uint4 ra[NCH], rb[NCH];
    if (va) pn_load_row<NCH>(xb + (long)s * D, lane, D, ra);
    if (vb) pn_load_row<NCH>(xb + (long)t * D, lane, D, rb);
    if (va) { pn_accumulate<NCH>(ra, ww, acc, D, eps); ++n; }
    if (vb) { pn_accumulate<NCH>(rb, ww, acc, D, eps); ++n; }
  }
  nred[wave] = n;
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) st8f(&red[wave - 1][(i * 64 + lane) * 8], acc[i]);
  }
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int k = 0; k < PN_WAVES - 1; ++k)
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      float r[8];
      ld8f(&red[k][(i * 64 + lane) * 8], r);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[i][e] += r[e];
    }
  float* o = part + (long)blockIdx.x * D;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int e0 = (lane + i * 64) * 8;
    if (e0 < D) st8f(o + e0, acc[i]);
  }
  if (lane == 0) cnt[blockIdx.x] = nred[0] + nred[1] + nred[2] + nred[3];
}

// stage 2: pooled[b, d] = (slice 0 + slice 1 + .. + slice 15) / n_b ; n_b = 0 gives zeros.  One thread per four columns.
__global__ __launch_bounds__(256) void pn_mean_stage2(const float* __restrict__ part, const int* __restrict__ cnt, float* __restrict__ out,
                                                      long BD4, int D4) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BD4) return;
  const long b = i / D4;
  const int c = (int)(i - b * D4);
  int n = 0;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < PN_SLICES; ++k) {
    n += cnt[b * PN_SLICES + k];
    const float4 p = *reinterpret_cast<const float4*>(part + ((b * PN_SLICES + k) * D4 + c) * 4);
    s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
  }
  if (n > 0) {
    const float fn = (float)n;
    s.x /= fn; s.y /= fn; s.z /= fn; s.w /= fn;
  } else {
    s = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  *reinterpret_cast<float4*>(out + i * 4) = s;
}

// ---- LAST forward: one wave per sample finds s*, normalises that row and writes it in f32
template <int NCH>
__global__ __launch_bounds__(64) void pn_last_fwd(const bf16_t* __restrict__ x, const float* __restrict__ w, const uint8_t* __restrict__ mask,
                                                  float* __restrict__ out, int S, int D, float eps) {
  const int lane = threadIdx.x;
  const long b = blockIdx.x;
  const int sstar = mask ? pn_last_valid(mask + b * S, S, lane) : S - 1;
  float acc[NCH][8];
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;
  if (sstar >= 0) {
    uint4 raw[NCH];
    float ww[NCH][8], v[NCH][8];
    pn_load_row<NCH>(x + (b * S + sstar) * D, lane, D, raw);
    pn_load_f32<NCH>(w, lane, D, ww);
    const float rs = pn_rstd<NCH>(raw, v, D, eps);
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[i][e] = ww[i][e] * (v[i][e] * rs);
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int e0 = (lane + i * 64) * 8;
    if (e0 < D) st8f(out + b * D + e0, acc[i]);
  }
}

// ---- backward.  meta[b] (one wave per sample): MASKED_MEAN n_b, LAST s* (-1: none)
__global__ __launch_bounds__(64) void pn_meta_kernel(const uint8_t* __restrict__ mask, int* __restrict__ meta, int S, int mode) {
  const int lane = threadIdx.x;
  const uint8_t* m = mask + (long)blockIdx.x * S;
  int r;
  if (mode == UR_POOL_LAST) {
    r = pn_last_valid(m, S, lane);
  } else {
    int n = 0;
    for (int s = lane; s < S; s += 64) n += m[s] != 0;
    r = wave_sum_i(n);
  }
  if (lane == 0) meta[blockIdx.x] = r;
}

// One wave per row, grid-stride.  meta == NULL: no mask (n_b = S, s* = S - 1).
template <int NCH>
__global__ __launch_bounds__(PN_WAVES * 64) void pn_bwd_kernel(const float* __restrict__ dpool, const bf16_t* __restrict__ x,
                                                              const float* __restrict__ w, const uint8_t* __restrict__ mask,
                                                              const int* __restrict__ meta, bf16_t* __restrict__ dx, long M, int S, int D,
                                                              float eps, int mode) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long row = (long)blockIdx.x * PN_WAVES + wave; row < M; row += (long)gridDim.x * PN_WAVES) {
    const long b = row / S;
    const int s = (int)(row - b * S);
    float c;
    if (mode == UR_POOL_LAST) {
      c = s == (meta ? meta[b] : S - 1) ? 1.f : 0.f;
    } else {
      c = (!mask || mask[row] != 0) ? 1.f / (float)(meta ? meta[b] : S) : 0.f;
    }
    bf16_t* drow = dx + row * D;
    if (c == 0.f) {                     // wave-uniform: the row is neither read nor computed
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int e0 = (lane + i * 64) * 8;
        if (e0 < D) *reinterpret_cast<uint4*>(drow + e0) = make_uint4(0u, 0u, 0u, 0u);
      }
      continue;
    }
    uint4 raw[NCH];
    float g[NCH][8], ww[NCH][8], xh[NCH][8];
    pn_load_row<NCH>(x + row * D, lane, D, raw);
    pn_load_f32<NCH>(dpool + b * D, lane, D, g);
    pn_load_f32<NCH>(w, lane, D, ww);
    const float rs = pn_rstd<NCH>(raw, xh, D, eps);
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) { g[i][e] *= ww[i][e]; xh[i][e] *= rs; t += g[i][e] * xh[i][e]; }
    const float m = wave_sum(t) / (float)D;
    const float k = c * rs;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int e0 = (lane + i * 64) * 8;
      if (e0 < D) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = k * (g[i][e] - xh[i][e] * m);
        *reinterpret_cast<uint4*>(drow + e0) = pk8(o);
      }
    }
  }
}

inline int pn_nch(int D) { const int c = ur_cdiv(D, 512); return c <= 1 ? 1 : (c <= 2 ? 2 : 4); }
inline bool pn_mode_ok(int mode) { return mode == UR_POOL_MASKED_MEAN || mode == UR_POOL_LAST; }
inline int64_t pn_ws_bytes(int64_t B, int64_t D, int mode) {
  // MASKED_MEAN: slice sums [B][SLICES][D] f32, then slice counts [B][SLICES] int (the backward's B ints fit in front); LAST: B ints
  return mode == UR_POOL_MASKED_MEAN ? B * PN_SLICES * (D + 1) * (int64_t)sizeof(float) : B * (int64_t)sizeof(int);
}

}  // namespace

#define UR_PN_DISPATCH(D, CALL)                     \
  switch (pn_nch(D)) {                              \
    case 1: { constexpr int NCH = 1; CALL; } break; \
    case 2: { constexpr int NCH = 2; CALL; } break; \
    default: { constexpr int NCH = 4; CALL; } break; \
  }

// the checks the two calls share (everything but their own pointers)
#define UR_PN_CHECK_SHAPE(who)                                                                                                      \
  UR_REQUIRE(pn_mode_ok(mode), who ": unknown mode %d (UR_POOL_MASKED_MEAN = 1, UR_POOL_LAST = 2)", mode);                           \
  UR_REQUIRE(D > 0 && (D % 8) == 0 && D <= 2048, who ": need D %% 8 == 0 and 0 < D <= 2048 (D=%d)", D);                              \
  UR_REQUIRE(S > 0 && B >= 0, who ": need S > 0 and B >= 0 (B=%d, S=%d)", B, S);                                                     \
  UR_REQUIRE(eps >= 0.f, who ": eps must be >= 0 (got %g)", (double)eps);                                                            \
  if (B == 0) return 0
#define UR_PN_CHECK_WORKSPACE(who)                                                                                                  \
  UR_REQUIRE(workspace && UR_ALIGNED16(workspace), who ": workspace is null or not 16-byte aligned");                               \
  UR_REQUIRE(workspace_bytes >= pn_ws_bytes(B, D, mode), who ": workspace too small (%lld bytes, ur_pool_norm_workspace_bytes says %lld)", \
             (long long)workspace_bytes, (long long)pn_ws_bytes(B, D, mode))

extern "C" int64_t ur_pool_norm_workspace_bytes(int32_t B, int32_t D, int32_t mode) {
  if (!pn_mode_ok(mode) || B < 0 || D <= 0 || (D % 8) != 0 || D > 2048) {
    snprintf(g_ur_err, sizeof(g_ur_err), "ur_pool_norm_workspace_bytes: bad argument (B=%d, D=%d, mode=%d)", B, D, mode);
    return -1;
  }
  return pn_ws_bytes(B, D, mode);
}

extern "C" int ur_pool_norm_fwd(const void* x, const float* w, const uint8_t* mask, float* pooled, int32_t B, int32_t S, int32_t D,
                                float eps, int32_t mode, void* workspace, int64_t workspace_bytes, void* stream) {
  UR_PN_CHECK_SHAPE("ur_pool_norm_fwd");
  UR_REQUIRE(x && w && pooled, "ur_pool_norm_fwd: null pointer (x, w and pooled are required)");
  UR_REQUIRE(UR_ALIGNED16(x) && UR_ALIGNED16(w) && UR_ALIGNED16(pooled), "ur_pool_norm_fwd: x, w and pooled must be 16-byte aligned");
  UR_PN_CHECK_WORKSPACE("ur_pool_norm_fwd");
  hipStream_t st = (hipStream_t)stream;
  if (mode == UR_POOL_LAST) {
    UR_PN_DISPATCH(D, hipLaunchKernelGGL((pn_last_fwd<NCH>), dim3(B), dim3(64), 0, st, (const bf16_t*)x, w, mask, pooled, S, D, eps));
    UR_CHECK_LAUNCH("ur_pool_norm_fwd(last)");
    return 0;
  }
  float* part = (float*)workspace;
  int* cnt = (int*)(part + (size_t)B * PN_SLICES * D);
  const int per = ur_cdiv(S, PN_SLICES);
  UR_PN_DISPATCH(D, hipLaunchKernelGGL((pn_mean_stage1<NCH>), dim3((unsigned)B * PN_SLICES), dim3(PN_WAVES * 64), 0, st, (const bf16_t*)x, w,
                                       mask, part, cnt, S, D, per, eps));
  UR_CHECK_LAUNCH("ur_pool_norm_fwd(stage1)");
  const long BD4 = (long)B * (D / 4);
  hipLaunchKernelGGL(pn_mean_stage2, dim3(ur_cdiv(BD4, 256)), dim3(256), 0, st, (const float*)part, (const int*)cnt, pooled, BD4, D / 4);
  UR_CHECK_LAUNCH("ur_pool_norm_fwd(stage2)");
  return 0;
}

extern "C" int ur_pool_norm_bwd(const float* d_pooled, const void* x, const float* w, const uint8_t* mask, void* dx, int32_t B, int32_t S,
                                int32_t D, float eps, int32_t mode, void* workspace, int64_t workspace_bytes, void* stream) {
  UR_PN_CHECK_SHAPE("ur_pool_norm_bwd");
  UR_REQUIRE(d_pooled && x && w && dx, "ur_pool_norm_bwd: null pointer (d_pooled, x, w and dx are required)");
  UR_REQUIRE(UR_ALIGNED16(d_pooled) && UR_ALIGNED16(x) && UR_ALIGNED16(w) && UR_ALIGNED16(dx),
             "ur_pool_norm_bwd: d_pooled, x, w and dx must be 16-byte aligned");
  UR_PN_CHECK_WORKSPACE("ur_pool_norm_bwd");
  hipStream_t st = (hipStream_t)stream;
  int* meta = nullptr;
  if (mask) {
    meta = (int*)workspace;
    hipLaunchKernelGGL(pn_meta_kernel, dim3(B), dim3(64), 0, st, mask, meta, S, mode);
    UR_CHECK_LAUNCH("ur_pool_norm_bwd(meta)");
  }
  const long M = (long)B * S;
  const long blocks = (M + PN_WAVES - 1) / PN_WAVES;
  const dim3 grid((unsigned)(blocks < PN_BWD_BLOCKS ? blocks : PN_BWD_BLOCKS));
  UR_PN_DISPATCH(D, hipLaunchKernelGGL((pn_bwd_kernel<NCH>), grid, dim3(PN_WAVES * 64), 0, st, d_pooled, (const bf16_t*)x, w, mask,
                                       (const int*)meta, (bf16_t*)dx, M, S, D, eps, mode));
  UR_CHECK_LAUNCH("ur_pool_norm_bwd");
  return 0;
}
