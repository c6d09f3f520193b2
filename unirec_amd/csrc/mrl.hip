// Matryoshka head (include/unirec_hip_mrl.h): the candidate scores, the InfoNCE loss and its gradient on K nested prefixes of the
// embedding, with ONE read of the candidates per direction.  A prefix dot product is a running sum: the score kernel keeps each lane's
// sums across the prefix boundaries and folds a snapshot at every boundary; the backward keeps one accumulator per plane that covers a
// feature.  The expressions are those of csrc/loss.hip (cos_scores_kernel, infonce_row_kernel, mean_kernel, infonce_bwd_stage1/2),
// restated here term by term so that plane k has the bits of those kernels on the contiguous slice [..., :d_k].  All arithmetic f32.
// gfx950 only.
#include "common.hip.h"
#include "unirec_hip_mrl.h"

namespace {

constexpr float NORM_EPS = 1e-12f;   // F.normalize eps
constexpr int KMAX = UR_MRL_MAX_DIMS;
constexpr int CHUNKS = UR_MRL_BWD_CHUNKS;

struct Dims { int K; int d[KMAX]; };              // by value: uniform, lives in scalar registers
struct Weights { float v[KMAX]; };

// scores[k][b][j] = cos(user[b][:d_k], cand(b,j)[:d_k]); one wave per candidate row, each element loaded once.
__global__ __launch_bounds__(256) void mrl_scores_kernel(const float* __restrict__ user, const float* __restrict__ pos,
                                                         const float* __restrict__ neg, float* __restrict__ scores,
                                                         float* __restrict__ inv_norm, int B, int N, Dims dims) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = dims.d[dims.K - 1];
  const long total = (long)B * (N + 1);
  for (long row = (long)blockIdx.x * 4 + wave; row < total; row += (long)gridDim.x * 4) {
    const int b = (int)(row / (N + 1)), j = (int)(row - (long)b * (N + 1));
    const float* c = (j == 0) ? pos + (long)b * D : neg + ((long)b * N + (j - 1)) * D;
    const float* u = user + (long)b * D;
    float dot = 0.f, cc = 0.f, uu = 0.f;
    int d = lane * 4;
    for (int k = 0; k < dims.K; ++k) {
      const int dk = dims.d[k];
      for (; d < dk; d += 256) {
        const float4 cv = *reinterpret_cast<const float4*>(c + d), uv = *reinterpret_cast<const float4*>(u + d);
        dot += cv.x * uv.x + cv.y * uv.y + cv.z * uv.z + cv.w * uv.w;
        cc += cv.x * cv.x + cv.y * cv.y + cv.z * cv.z + cv.w * cv.w;
        uu += uv.x * uv.x + uv.y * uv.y + uv.z * uv.z + uv.w * uv.w;
      }
      const float sdot = wave_sum(dot), scc = wave_sum(cc), suu = wave_sum(uu);      // the snapshot: the running sums go on
      if (lane == 0) {
        const float ic = 1.0f / fmaxf(sqrtf(scc), NORM_EPS), iu = 1.0f / fmaxf(sqrtf(suu), NORM_EPS);
        scores[(long)k * total + row] = sdot * ic * iu;
        inv_norm[(long)k * total + row] = ic;
      }
    }
  }
}

// per (sample, plane): loss_b = -s0/tau + logsumexp_{valid j}(s_j/tau); w[k][b][j] = d loss_b / d (s_j)  (already / tau)
__global__ __launch_bounds__(256) void mrl_row_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ nmask,
                                                      float* __restrict__ row_loss, float* __restrict__ w, int B, int N, int bpad,
                                                      float inv_tau) {
  __shared__ float red[4];
  const int b = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long plane = (long)k * B * (N + 1);
  const float* s = scores + plane + (long)b * (N + 1);
  float mx = -__builtin_huge_valf();
  for (int j = tid; j <= N; j += 256) {
    const bool valid = (j == 0) || nmask == nullptr || nmask[(long)b * N + (j - 1)];
    if (valid) mx = fmaxf(mx, s[j] * inv_tau);
  }
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int j = tid; j <= N; j += 256) {
    const bool valid = (j == 0) || nmask == nullptr || nmask[(long)b * N + (j - 1)];
    if (valid) sum += __expf(s[j] * inv_tau - mx);
  }
  sum = wave_sum(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  sum = red[0] + red[1] + red[2] + red[3];
  const float lse = mx + logf(sum);
  if (tid == 0) row_loss[(long)k * bpad + b] = -s[0] * inv_tau + lse;
  for (int j = tid; j <= N; j += 256) {
    const bool valid = (j == 0) || nmask == nullptr || nmask[(long)b * N + (j - 1)];
    float p = valid ? __expf(s[j] * inv_tau - lse) : 0.f;
    if (j == 0) p -= 1.0f;
    w[plane + (long)b * (N + 1) + j] = p * inv_tau;
  }
}

// wave k: plane_loss[k] = mean_b row_loss[k][b]; then loss = sum_k weights[k] * plane_loss[k], ascending k, zero weights left out
__global__ void mrl_mean_kernel(const float* __restrict__ row_loss, float* __restrict__ plane_loss, float* __restrict__ loss, int n,
                                int bpad, int K, Weights wt) {
  __shared__ float pl[KMAX];
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* x = row_loss + (long)k * bpad;
  float s = 0.f;
  for (int i = lane; i < n; i += 64) s += x[i];
  s = wave_sum(s);
  if (lane == 0) { pl[k] = s / (float)n; plane_loss[k] = pl[k]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int q = 0; q < K; ++q)
      if (wt.v[q] != 0.f) acc = fmaf(wt.v[q], pl[q], acc);
    loss[0] = acc;
  }
}

// part[b][chunk][off_k + d] = sum_{j in chunk} w[k][b][j] * inv_norm[k][b][j] * cand(b,j)[d] for every plane k with d < d_k
// (off_k = d_0 + .. + d_{k-1}); each candidate float4 is loaded once and feeds the accumulators of all those planes.
__global__ __launch_bounds__(256) void mrl_bwd_stage1(const float* __restrict__ pos, const float* __restrict__ neg,
                                                      const float* __restrict__ w, const float* __restrict__ inv_norm,
                                                      float* __restrict__ part, int B, int N, int per, Dims dims, int sumd) {
  const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x;
  const int D = dims.d[dims.K - 1];
  const int j0 = ch * per, j1 = min(N + 1, j0 + per);
  const long total = (long)B * (N + 1);
  for (int d = tid * 4; d < D; d += 1024) {
    float4 acc[KMAX];
    bool on[KMAX];                                  // plane k covers this feature
#pragma unroll
    for (int k = 0; k < KMAX; ++k) { acc[k] = make_float4(0.f, 0.f, 0.f, 0.f); on[k] = k < dims.K && d < dims.d[k]; }
    for (int j = j0; j < j1; ++j) {
      const float* c = (j == 0) ? pos + (long)b * D : neg + ((long)b * N + (j - 1)) * D;
      const float4 cv = *reinterpret_cast<const float4*>(c + d);
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < dims.K) {                           // uniform: the coefficient is a scalar load
          const float coef = w[(long)k * total + (long)b * (N + 1) + j] * inv_norm[(long)k * total + (long)b * (N + 1) + j];
          if (on[k]) { acc[k].x += coef * cv.x; acc[k].y += coef * cv.y; acc[k].z += coef * cv.z; acc[k].w += coef * cv.w; }
        }
      }
    }
    float* out = part + ((long)b * CHUNKS + ch) * sumd + d;
    int off = 0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (on[k]) *reinterpret_cast<float4*>(out + off) = acc[k];
      if (k < dims.K) off += dims.d[k];
    }
  }
}

// du[b][d] = sum_{k : d < d_k} weights[k] * gscale * ( sum_chunks part_k - uhat_k * sum_j w_kj s_kj ) / max(||u[:d_k]||, eps)
__global__ __launch_bounds__(256) void mrl_bwd_stage2(const float* __restrict__ user, const float* __restrict__ scores,
                                                      const float* __restrict__ w, const float* __restrict__ part,
                                                      float* __restrict__ du, int B, int N, Dims dims, int sumd, Weights wt, float gscale) {
  __shared__ float red[KMAX][8];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = dims.d[dims.K - 1];
  const long total = (long)B * (N + 1);
  {
    float uu = 0.f;
    int d = tid;
    for (int k = 0; k < dims.K; ++k) {
      float ws = 0.f;
      const long base = (long)k * total + (long)b * (N + 1);
      for (int j = tid; j <= N; j += 256) ws += w[base + j] * scores[base + j];
      for (; d < dims.d[k]; d += 256) { const float u = user[(long)b * D + d]; uu += u * u; }
      const float sws = wave_sum(ws), suu = wave_sum(uu);       // uu: the snapshot at the boundary, the running sum goes on
      if (lane == 0) { red[k][wave] = sws; red[k][4 + wave] = suu; }
    }
  }
  __syncthreads();
  for (int d = tid; d < D; d += 256) {
    const float ud = user[(long)b * D + d];
    float acc = 0.f;
    int off = 0;
    for (int k = 0; k < dims.K; ++k) {
      if (d < dims.d[k] && wt.v[k] != 0.f) {
        const float ws = red[k][0] + red[k][1] + red[k][2] + red[k][3];
        const float uu = red[k][4] + red[k][5] + red[k][6] + red[k][7];
        const float iu = 1.0f / fmaxf(sqrtf(uu), NORM_EPS);
        float s = 0.f;
        for (int c = 0; c < CHUNKS; ++c) s += part[((long)b * CHUNKS + c) * sumd + off + d];
        // gscale * iu * (s - ud * iu * ws) as infonce_bwd_stage2 is compiled: the subtraction contracts with the product by ws.  Spelt
        // out, because beside the weighted sum below the compiler would pair the products instead and round s - (..) twice.
        const float g = (gscale * iu) * fmaf(-(ud * iu), ws, s);
        acc = fmaf(wt.v[k], g, acc);
      }
      off += dims.d[k];
    }
    du[(long)b * D + d] = acc;
  }
}

// ---- host: the checks both entry points share ---------------------------------------------------------------------------------------
int check_dims(const char* who, int K, const int32_t* d, int D, int B, int N, Dims* out, int64_t* sumd) {
  UR_REQUIRE(K >= 1 && K <= KMAX, "%s: K must be in 1..%d (got %d)", who, KMAX, K);
  int64_t s = 0;
  for (int k = 0; k < K; ++k) {
    UR_REQUIRE(d[k] > 0 && (d[k] % 4) == 0, "%s: dims[%d] must be a positive multiple of 4 (got %d)", who, k, d[k]);
    UR_REQUIRE(k == 0 || d[k] > d[k - 1], "%s: dims must be strictly ascending (dims[%d] = %d after %d)", who, k, d[k], d[k - 1]);
    out->d[k] = d[k];
    s += d[k];
  }
  for (int k = K; k < KMAX; ++k) out->d[k] = 0;
  out->K = K;
  UR_REQUIRE(d[K - 1] == D, "%s: the last of dims must equal D (got %d, D %d)", who, d[K - 1], D);
  UR_REQUIRE(B >= 0 && N >= 0, "%s: need B >= 0 and N >= 0 (got B %d, N %d)", who, B, N);
  *sumd = s;
  return 0;
}

int check_operands(const char* who, const float* user, const float* pos, const float* neg, int N, const float* scores, const float* inv) {
  UR_REQUIRE(user && pos && (N == 0 || neg) && scores && inv, "%s: null pointer (user, pos, neg, scores, cand_inv_norm)", who);
  UR_REQUIRE(UR_ALIGNED16(user) && UR_ALIGNED16(pos) && (!neg || UR_ALIGNED16(neg)), "%s: user, pos and neg must be 16-byte aligned", who);
  return 0;
}

void launch_scores(const float* user, const float* pos, const float* neg, float* scores, float* inv, int B, int N, const Dims& dims,
                   hipStream_t st) {
  const long rows = (long)B * (N + 1);
  long g = (rows + 3) / 4; if (g > 256 * 16) g = 256 * 16;
  hipLaunchKernelGGL(mrl_scores_kernel, dim3((int)g), dim3(256), 0, st, user, pos, neg, scores, inv, B, N, dims);
}

inline int64_t pad4(int64_t n) { return (n + 3) / 4 * 4; }

}  // namespace

extern "C" int ur_mrl_scores(const ur_mrl_scores_t* a, void* stream) {
  UR_REQUIRE(a, "ur_mrl_scores: null argument struct");
  Dims dims; int64_t sumd;
  if (int rc = check_dims("ur_mrl_scores", a->K, a->dims, a->D, a->B, a->N, &dims, &sumd)) return rc;
  if (a->B == 0) return 0;
  if (int rc = check_operands("ur_mrl_scores", a->user, a->pos, a->neg, a->N, a->scores, a->cand_inv_norm)) return rc;
  launch_scores(a->user, a->pos, a->neg, a->scores, a->cand_inv_norm, a->B, a->N, dims, (hipStream_t)stream);
  UR_CHECK_LAUNCH("ur_mrl_scores");
  return 0;
}

extern "C" int ur_mrl_infonce(ur_mrl_infonce_t* a, void* stream) {
  UR_REQUIRE(a, "ur_mrl_infonce: null argument struct");
  Dims dims; int64_t sumd;
  if (int rc = check_dims("ur_mrl_infonce", a->K, a->dims, a->D, a->B, a->N, &dims, &sumd)) return rc;
  const int B = a->B, N = a->N, K = a->K;
  Weights wt;
  bool any = false;
  for (int k = 0; k < KMAX; ++k) wt.v[k] = 0.f;
  for (int k = 0; k < K; ++k) {
    const float v = a->weights[k];
    UR_REQUIRE(v >= 0.f && v <= 3.0e38f, "ur_mrl_infonce: weights[%d] must be finite and >= 0 (got %g)", k, (double)v);
    wt.v[k] = v;
    any = any || v > 0.f;
  }
  UR_REQUIRE(any, "ur_mrl_infonce: weights must hold at least one positive entry");
  UR_REQUIRE(a->temperature > 0.f && a->temperature <= 3.0e38f, "ur_mrl_infonce: temperature must be positive and finite (got %g)",
             (double)a->temperature);
  // row_loss [K][bpad] + w [K][B][N+1] + part [B][CHUNKS][sumd]
  const int64_t bpad = pad4(B), wn = pad4((int64_t)K * B * (N + 1));
  const int64_t need = (int64_t)sizeof(float) * ((int64_t)K * bpad + wn + (int64_t)B * CHUNKS * sumd);
  if (!a->workspace) {
    a->workspace_bytes = need;
    return 0;
  }
  if (B == 0) return 0;
  if (int rc = check_operands("ur_mrl_infonce", a->user, a->pos, a->neg, N, a->scores, a->cand_inv_norm)) return rc;
  UR_REQUIRE(a->plane_loss && a->loss, "ur_mrl_infonce: null pointer (plane_loss, loss)");
  UR_REQUIRE(UR_ALIGNED16(a->workspace) && a->workspace_bytes >= need,
             "ur_mrl_infonce: workspace must be 16-byte aligned and hold %lld bytes (got %lld)", (long long)need, (long long)a->workspace_bytes);
  UR_REQUIRE(!a->d_user || UR_ALIGNED16(a->d_user), "ur_mrl_infonce: d_user must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  float* row_loss = (float*)a->workspace;
  float* w = row_loss + (int64_t)K * bpad;
  float* part = w + wn;
  launch_scores(a->user, a->pos, a->neg, a->scores, a->cand_inv_norm, B, N, dims, st);
  UR_CHECK_LAUNCH("ur_mrl_infonce(scores)");
  hipLaunchKernelGGL(mrl_row_kernel, dim3(B, K), dim3(256), 0, st, (const float*)a->scores, a->neg_mask, row_loss, w, B, N, (int)bpad,
                     1.0f / a->temperature);
  UR_CHECK_LAUNCH("ur_mrl_infonce(row)");
  hipLaunchKernelGGL(mrl_mean_kernel, dim3(1), dim3(64 * K), 0, st, (const float*)row_loss, a->plane_loss, a->loss, B, (int)bpad, K, wt);
  UR_CHECK_LAUNCH("ur_mrl_infonce(mean)");
  if (a->d_user) {
    const int per = ur_cdiv(N + 1, CHUNKS);
    hipLaunchKernelGGL(mrl_bwd_stage1, dim3(CHUNKS, B), dim3(256), 0, st, a->pos, a->neg, (const float*)w, (const float*)a->cand_inv_norm,
                       part, B, N, per, dims, (int)sumd);
    UR_CHECK_LAUNCH("ur_mrl_infonce(bwd1)");
    hipLaunchKernelGGL(mrl_bwd_stage2, dim3(B), dim3(256), 0, st, a->user, (const float*)a->scores, (const float*)w, (const float*)part,
                       a->d_user, B, N, dims, (int)sumd, wt, a->grad_scale / (float)B);
    UR_CHECK_LAUNCH("ur_mrl_infonce(bwd2)");
  }
  return 0;
}
