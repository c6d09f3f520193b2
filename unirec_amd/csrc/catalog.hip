// Data-path kernels either side of the hot path, gfx950 only.  All HBM-bound.
//
//   ur_gather_rows    : out[i] = src[idx[i]] (a zero row for idx < 0): the packed replacement of the reference's
//                       per-sample torch.stack of cached tensors --
//                       training/train_item_individual_token_joint.py:557-577 (_get_history_qformer_inputs: history
//                       slot -> [F,1024] field vectors + [F] mask, zero padding for missing items / empty slots),
//                       :246-255 (history item query tokens), models/qformer_utils.py:150-155 (__getitem__).
//                       f32 rows may leave as bf16 (the dtype the Q-Former kernels consume) in the same pass, and bf16 rows
//                       as f32 (a bf16 catalogue's rows for the f32 InfoNCE kernels; a 16-bit shift, exact for every pattern).
//   ur_catalog_scores : scores[b][n] = cos(user_b, item_n) over a SHARED catalogue [N,D] f32 with
//                       F.normalize(p=2, eps=1e-12) semantics (training/train_item_individual_token_joint.py:408-415,
//                       evaluation over pool = all items); the catalogue is read once per 16 users.
//   ur_rank_of_index  : rank_b = 1 + #{n : s_bn > s_b,gt_b}  (:416-417: position of the positive in the descending
//                       argsort; ties resolved for the positive, as ur_mrr_rank).
//   ur_catalog_scores with a ur_catalog_select_t: streaming retrieval.  The host loop scores the catalogue a chunk of rows at a
//                       time (the same kernel on a row range) and catalog_select_kernel folds each chunk into a running
//                       top-K list and a count of scores above the ground truth's, per-user exclusion lists filtered out.
//                       Here the catalogue may be bf16 (widened exactly on load) and a chunk may be scored on the f32 matrix cores
//                       (catalog_scores_mfma_kernel: the vector kernel's fmaf chains and sum tree, so the same score bits).
//   ur_catalog_deep_select (include/unirec_hip_deep.h): the same streaming retrieval with lists of up to 1024 items.  The chunks are
//                       scored by the launches of select mode; the selection kernels are those of catalog_deep.hip.h.
#include <utility>
#include "common.hip.h"
#include "unirec_hip.h"
#include "unirec_hip_loss.h"
#include "unirec_hip_mrl_loss.h"
#include "unirec_hip_deep.h"
#include "catalog_select.hip.h"
#include "catalog_deep.hip.h"

namespace {

// one wave per output row; 16-byte pieces
template <int SRC_BYTES, bool TO_BF16, bool TO_F32 = false>
__global__ void gather_rows_kernel(const char* __restrict__ src, const long* __restrict__ idx, char* __restrict__ out,
                                   long row_elems, long n_out, long n_src) {
  const long row = (long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (row >= n_out) return;
  const int lane = threadIdx.x & 63;
  const long s = idx[row];
  const bool valid = s >= 0 && s < n_src;
  constexpr int EPP = 16 / SRC_BYTES;                   // source elements per 16-byte piece
  const long pieces = row_elems / EPP;                  // host guarantees divisibility
  const char* sp = src + (valid ? s : 0) * row_elems * SRC_BYTES;
  if (TO_F32) {                                         // bf16 -> f32: one source piece -> its 2 adjacent 16-byte output pieces,
    char* op = out + row * row_elems * 4;               // so a wave's stores cover whole contiguous 128-byte lines
    for (long p = lane; p < pieces; p += 64) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (valid) v = *reinterpret_cast<const uint4*>(sp + p * 16);
      *reinterpret_cast<uint4*>(op + p * 32) = make_uint4(v.x << 16, v.x & 0xffff0000u, v.y << 16, v.y & 0xffff0000u);
      *reinterpret_cast<uint4*>(op + p * 32 + 16) = make_uint4(v.z << 16, v.z & 0xffff0000u, v.w << 16, v.w & 0xffff0000u);
    }
  } else if (TO_BF16) {                                 // f32 -> bf16: 2 source pieces -> one 16-byte output piece
    char* op = out + row * row_elems * 2;
    for (long p = lane; p < pieces / 2; p += 64) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
      if (valid) { a = *reinterpret_cast<const float4*>(sp + p * 32); b = *reinterpret_cast<const float4*>(sp + p * 32 + 16); }
      *reinterpret_cast<uint4*>(op + p * 16) = make_uint4(pack_bf2(a.x, a.y), pack_bf2(a.z, a.w), pack_bf2(b.x, b.y), pack_bf2(b.z, b.w));
    }
  } else {
    char* op = out + row * row_elems * SRC_BYTES;
    for (long p = lane; p < pieces; p += 64) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (valid) v = *reinterpret_cast<const uint4*>(sp + p * 16);
      *reinterpret_cast<uint4*>(op + p * 16) = v;
    }
  }
}
// narrow rows (masks: F bytes per item): one thread per output element
__global__ void gather_bytes_kernel(const uint8_t* __restrict__ src, const long* __restrict__ idx, uint8_t* __restrict__ out,
                                    long row_bytes, long n_out, long n_src) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out * row_bytes) return;
  const long row = i / row_bytes, c = i - row * row_bytes;
  const long s = idx[row];
  out[i] = (s >= 0 && s < n_src) ? src[s * row_bytes + c] : (uint8_t)0;
}

// scores[b][n] = (u_b . c_n) * inv_u[b] * inv_c[n], f32 FMA.  Block = 256 threads = 4 waves; a block owns 16 users
// (their vectors staged once in LDS) and walks catalogue rows, one row per wave per step: each lane holds 4-element
// pieces of the row and accumulates 16 dot products, reduced across the wave at the end of the row.
constexpr int CU_USERS = 16;
// (the body: uld / cld = the row strides of user and cat in elements, D for the contiguous kernel; only the first D components of a
// row are read, so with strides above D this is the kernel on a prefix of rows read in place -- catalog_scores_prefix_kernel)
template <typename CT>
__device__ __forceinline__ void catalog_scores_body(const float* __restrict__ user, long uld, const float* __restrict__ inv_u,
                                                    const CT* __restrict__ cat, long cld, const float* __restrict__ inv_c,
                                                    float* __restrict__ scores, int B, long N, int D, long rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) float us[];      // [CU_USERS][D]
  const int b0 = blockIdx.y * CU_USERS;
  const int nb = min(CU_USERS, B - b0);
  for (int i = threadIdx.x * 4; i < CU_USERS * D; i += 256 * 4) {
    const int u = i / D, d = i - u * D;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (u < nb) v = *reinterpret_cast<const float4*>(user + (long)(b0 + u) * uld + d);
    *reinterpret_cast<float4*>(us + i) = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long r0 = (long)blockIdx.x * rows_per_block, r1 = min(N, r0 + rows_per_block);
  for (long n = r0 + wave; n < r1; n += 4) {
    float acc[CU_USERS];
#pragma unroll
    for (int u = 0; u < CU_USERS; ++u) acc[u] = 0.f;
    const CT* cp = cat + n * cld;
    for (int d = lane * 4; d < D; d += 256) {
      const float4 c = load4(cp + d);
#pragma unroll
      for (int u = 0; u < CU_USERS; ++u) {
        const float4 x = *reinterpret_cast<const float4*>(us + u * D + d);
        acc[u] = fmaf(c.x, x.x, fmaf(c.y, x.y, fmaf(c.z, x.z, fmaf(c.w, x.w, acc[u]))));
      }
    }
    const float ic = inv_c[n];
#pragma unroll
    for (int u = 0; u < CU_USERS; ++u) {
      const float s = wave_sum(acc[u]);
      if (lane == 0 && u < nb) scores[(long)(b0 + u) * N + n] = s * inv_u[b0 + u] * ic;
    }
  }
}
template <typename CT>
__global__ __launch_bounds__(256) void catalog_scores_kernel(const float* __restrict__ user, const float* __restrict__ inv_u,
                                                             const CT* __restrict__ cat, const float* __restrict__ inv_c,
                                                             float* __restrict__ scores, int B, long N, int D, long rows_per_block) {
  catalog_scores_body<CT>(user, (long)D, inv_u, cat, (long)D, inv_c, scores, B, N, D, rows_per_block);
}
template <typename CT>
__global__ __launch_bounds__(256) void catalog_scores_prefix_kernel(const float* __restrict__ user, long uld, const float* __restrict__ inv_u,
                                                                    const CT* __restrict__ cat, long cld, const float* __restrict__ inv_c,
                                                                    float* __restrict__ scores, int B, long N, int D, long rows_per_block) {
  catalog_scores_body<CT>(user, uld, inv_u, cat, cld, inv_c, scores, B, N, D, rows_per_block);
}

__global__ void rank_of_index_kernel(const float* __restrict__ scores, const long* __restrict__ gt, int* __restrict__ rank, long N) {
  const int b = blockIdx.x;
  const float* s = scores + (long)b * N;
  const long g = min(max(gt[b], 0L), N - 1);
  const float ref = s[g];
  int cnt = 0;
  for (long n = threadIdx.x; n < N; n += blockDim.x) cnt += (s[n] > ref) ? 1 : 0;
  __shared__ int part[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) part[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) rank[b] = 1 + part[0] + part[1] + part[2] + part[3];
}

// ---- streaming selection (ur_catalog_select_t) -------------------------------------------------------------------------
// s_b,gt for the rank count, before any chunk is scored: one wave per user runs catalog_scores_kernel's dot product on row gt[b]
// (the same lane -> element map, the same fmaf chain, the same wave_sum and the same two multiplies), so ref[b] has the bits that
// kernel writes for that row.
template <typename CT>
__device__ __forceinline__ void catalog_gt_score_body(const float* __restrict__ user, long uld, const float* __restrict__ inv_u,
                                                      const CT* __restrict__ cat, long cld, const float* __restrict__ inv_c,
                                                      const long* __restrict__ gt, float* __restrict__ ref, int B, long N, int D) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const long g = min(max(gt[b], 0L), N - 1);
  const CT* cp = cat + g * cld;
  const float* up = user + (long)b * uld;
  float acc = 0.f;
  for (int d = lane * 4; d < D; d += 256) {
    const float4 c = load4(cp + d);
    const float4 x = *reinterpret_cast<const float4*>(up + d);
    acc = fmaf(c.x, x.x, fmaf(c.y, x.y, fmaf(c.z, x.z, fmaf(c.w, x.w, acc))));
  }
  const float ic = inv_c[g];
  const float s = wave_sum(acc);
  if (lane == 0) ref[b] = s * inv_u[b] * ic;
}
template <typename CT>
__global__ __launch_bounds__(256) void catalog_gt_score_kernel(const float* __restrict__ user, const float* __restrict__ inv_u,
                                                               const CT* __restrict__ cat, const float* __restrict__ inv_c,
                                                               const long* __restrict__ gt, float* __restrict__ ref, int B, long N, int D) {
  catalog_gt_score_body<CT>(user, (long)D, inv_u, cat, (long)D, inv_c, gt, ref, B, N, D);
}
// (the same on the first D components of rows uld / cld elements apart)
template <typename CT>
__global__ __launch_bounds__(256) void catalog_gt_score_prefix_kernel(const float* __restrict__ user, long uld, const float* __restrict__ inv_u,
                                                                      const CT* __restrict__ cat, long cld, const float* __restrict__ inv_c,
                                                                      const long* __restrict__ gt, float* __restrict__ ref, int B, long N, int D) {
  catalog_gt_score_body<CT>(user, uld, inv_u, cat, cld, inv_c, gt, ref, B, N, D);
}

// ---- f32-MFMA scorer ---------------------------------------------------------------------------------------------------------
// The same scores as catalog_scores_kernel, bit for bit, on v_mfma_f32_16x16x4_f32 (a k-ordered f32 fmaf chain from the C input, one
// rounding per product).  The vector kernel's score of (user u, row n) is: per lane l a chain p_l over the 4-element pieces at
// d = 4l + 256j (j = 0, 1, ...; inside a piece w, z, y, x), then wave_sum's balanced tree over the 64 lanes (pairs 32 apart first),
// then (v * inv_u) * inv_c.  Here "lane l" becomes chain c: for one c the pieces j = 0 .. J-1 are the K dimension (4 per MFMA, k = 0
// .. 3 <-> w, z, y, x) of a [16 users] x [16 rows] product from C = 0, which yields p_c of all 256 pairs at once.  A piece that lies
// past D is skipped (the condition is wave-uniform), as the lane's loop ends there; a chain without pieces stays +0.
// A workgroup = 4 waves owns 16 UT users (vectors staged once in LDS, in operand order) and walks groups of 16 RT rows; all four
// waves work on the same UT x RT tiles, wave w on the 16 chains c = w + 4t.  Visiting t in 4-bit bit-reversed order completes the
// tree's pairs as they arrive (5 pending tiles at most); what is left per wave is the subtree y_w of the lanes = w mod 4, and the
// last two levels, (y_0 + y_2) + (y_1 + y_3), go through LDS, wave w finishing tile w.  The catalogue operand is loaded straight
// from global memory in operand layout (lane = (row, k)), two chains ahead; the four waves touch the same 64 bytes of a row together.
constexpr int MF_TILES = 4;                    // 16x16 output tiles per wave (UT x RT) = waves per workgroup
__host__ __device__ constexpr int mf_bitrev4(int i) { return ((i & 1) << 3) | ((i & 2) << 1) | ((i & 4) >> 1) | ((i & 8) >> 3); }
__host__ __device__ constexpr int mf_trailing_ones(int i) { return (i & 1) ? 1 + mf_trailing_ones(i >> 1) : 0; }
__host__ __device__ constexpr size_t mf_lds_bytes(int D, bool wide) {
  return ((size_t)((D + 255) / 256) * (wide ? 1 : 2) * 64 * 64 + 4 * MF_TILES * 64 * 4) * sizeof(float);
}

// the wave's element of a catalogue row for one MFMA: lane (row, k) takes element 3 - k of a 4-element piece.  f32: that dword.
// bf16: the aligned dword that holds the element and its neighbour, widened by a shift or a mask (half-word loads were 11 % slower, docs/lab_notes.md section 22).
template <typename CT> struct mf_row;
template <> struct mf_row<float> {
  const float* p = nullptr;
  mf_row() = default;
  __device__ __forceinline__ mf_row(const float* row, int k) : p(row + (3 - k)) {}
  __device__ __forceinline__ float at(int off) const { return p[off]; }                 // off: element offset of the piece in the row
};
template <> struct mf_row<bf16_t> {
  const uint32_t* p = nullptr;
  bool hi = false;
  mf_row() = default;
  __device__ __forceinline__ mf_row(const bf16_t* row, int k) : p(reinterpret_cast<const uint32_t*>(row) + ((3 - k) >> 1)), hi((3 - k) & 1) {}
  __device__ __forceinline__ float at(int off) const {
    const uint32_t v = p[off >> 1];
    return __uint_as_float(hi ? (v & 0xffff0000u) : (v << 16));
  }
};

// WIDE: D > 1024 (16 users per workgroup, 8 pieces per chain at most).  FULL: D = 256 JMAX, so every chain has every piece and the
// conditions below fold away; the code is one straight line per row group.
// (the body: uld / cld = the row strides of user and cat, D for the contiguous kernel.  With strides above D it scores the first D
// components of rows read in place -- catalog_scores_mfma_prefix_kernel: a piece at or past D is skipped by the conditions below, never
// loaded as an operand, so what lies behind the prefix in a row reaches no result.)
template <typename CT, bool WIDE, bool FULL>
__device__ __forceinline__ void catalog_scores_mfma_body(const float* __restrict__ user, long uld, const float* __restrict__ inv_u,
                                                         const CT* __restrict__ cat, long cld, const float* __restrict__ inv_c,
                                                         float* __restrict__ scores, int B, long N, int D, long rows_per_block, int ub) {
  constexpr int UT = WIDE ? 1 : 2, RT = MF_TILES / UT, JMAX = WIDE ? 8 : 4;
  extern __shared__ __attribute__((aligned(16))) float us[];       // [64 chains][J][UT][k 4][user 16] | exchange [4 waves][MF_TILES][64] f32x4
  const int J = (D + 255) >> 8;
  f32x4* ex = reinterpret_cast<f32x4*>(us + J * UT * 64 * 64);
  const int ug = blockIdx.x % ub;
  const long rb = blockIdx.x / ub;
  const int b0 = ug * 16 * UT;
  const int nb = min(16 * UT, B - b0);
  const int D4 = D >> 2;
  for (int i = threadIdx.x; i < 16 * UT * D4; i += 256) {
    const int u = i / D4, d = (i - u * D4) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (u < nb) v = *reinterpret_cast<const float4*>(user + (long)(b0 + u) * uld + d);
    float* q = us + (((((d & 255) >> 2) * J + (d >> 8)) * UT + (u >> 4)) << 6) + (u & 15);
    q[0] = v.w; q[16] = v.z; q[32] = v.y; q[48] = v.x;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, col = lane & 15, k = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long r0 = rb * rows_per_block, r1 = min(N, r0 + rows_per_block);
  for (long n0 = r0; n0 < r1; n0 += 16 * RT) {
    mf_row<CT> bp[RT];                           // a row past the end is read as the last one and never stored
#pragma unroll
    for (int r = 0; r < RT; ++r) bp[r] = mf_row<CT>(cat + min(n0 + r * 16 + col, N - 1) * cld, k);
    float bq[3][JMAX][RT];
    f32x4 st[5][MF_TILES];                       // st[s]: a finished subtree of 2^s chains waiting for its sibling
#pragma unroll
    for (int i = -2; i < 16; ++i) {
      if (i + 2 < 16) {
        const int t = mf_bitrev4(i + 2);
#pragma unroll
        for (int j = 0; j < JMAX; ++j)
#pragma unroll
          for (int r = 0; r < RT; ++r)
            bq[(i + 2) % 3][j][r] = bp[r].at((FULL || 4 * w + 16 * t + 256 * j < D) ? 4 * w + 16 * t + 256 * j : 0);   // (a piece past D: unused)
      }
      if (i >= 0) {
        const int c = w + 4 * mf_bitrev4(i);
        f32x4 acc[MF_TILES];
#pragma unroll
        for (int x = 0; x < MF_TILES; ++x) acc[x] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
          if (FULL || 4 * c + 256 * j < D) {
            const float* ap = us + (((c * J + j) * UT) << 6) + lane;
#pragma unroll
            for (int t = 0; t < UT; ++t) {
              const float a = ap[t * 64];
#pragma unroll
              for (int r = 0; r < RT; ++r)
                acc[t * RT + r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bq[i % 3][j][r], acc[t * RT + r], 0, 0, 0);
            }
          }
        }
        const int lvl = mf_trailing_ones(i);
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (s < lvl) {
#pragma unroll
            for (int x = 0; x < MF_TILES; ++x) acc[x] = st[s][x] + acc[x];
          }
#pragma unroll
        for (int x = 0; x < MF_TILES; ++x) st[lvl][x] = acc[x];
      }
    }
    __syncthreads();                             // the previous group's exchange has been read
#pragma unroll
    for (int x = 0; x < MF_TILES; ++x) ex[(w * MF_TILES + x) * 64 + lane] = st[4][x];
    __syncthreads();
    const f32x4 v = (ex[(0 * MF_TILES + w) * 64 + lane] + ex[(2 * MF_TILES + w) * 64 + lane]) +
                    (ex[(1 * MF_TILES + w) * 64 + lane] + ex[(3 * MF_TILES + w) * 64 + lane]);
    const int ut = w / RT;
    const long n = n0 + (w % RT) * 16 + col;     // C/D layout: column = lane & 15 (row of the catalogue), row = 4 (lane >> 4) + reg (user)
    if (n < N) {
      const float ic = inv_c[n];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int u = ut * 16 + k * 4 + e;
        if (u < nb) scores[(long)(b0 + u) * N + n] = v[e] * inv_u[b0 + u] * ic;
      }
    }
  }
}
template <typename CT, bool WIDE, bool FULL>
__global__ __launch_bounds__(256) void catalog_scores_mfma_kernel(const float* __restrict__ user, const float* __restrict__ inv_u,
                                                                  const CT* __restrict__ cat, const float* __restrict__ inv_c,
                                                                  float* __restrict__ scores, int B, long N, int D, long rows_per_block, int ub) {
  catalog_scores_mfma_body<CT, WIDE, FULL>(user, (long)D, inv_u, cat, (long)D, inv_c, scores, B, N, D, rows_per_block, ub);
}
template <typename CT, bool WIDE, bool FULL>
__global__ __launch_bounds__(256) void catalog_scores_mfma_prefix_kernel(const float* __restrict__ user, long uld, const float* __restrict__ inv_u,
                                                                         const CT* __restrict__ cat, long cld, const float* __restrict__ inv_c,
                                                                         float* __restrict__ scores, int B, long N, int D, long rows_per_block,
                                                                         int ub) {
  catalog_scores_mfma_body<CT, WIDE, FULL>(user, uld, inv_u, cat, cld, inv_c, scores, B, N, D, rows_per_block, ub);
}

// ---- one scoring pass for several prefixes (ur_catalog_mrl_softmax) -------------------------------------------------------------------
// catalog_scores_mfma_kernel for up to MG_PLANES nested prefixes d_0 < .. < d_{NP-1} <= 1024 of the rows at once: plane p's scores, bit
// for bit what that kernel writes at width d_p.  The chain of c runs over ascending pieces j as there; its value after the last piece
// below d_p IS plane p's chain (a piece 4c + 256j lies wholly on one side of d_p), so at that point -- a wave-uniform condition -- the
// accumulator enters plane p's own tree of pending subtrees, by the same counter in the same bit-reversed order; a chain with no piece
// below d_p enters as +0, the idle lane of the vector kernel (a chain is never -0: it starts from +0).  So the MFMAs are those of ONE
// pass at width d_{NP-1}, not of NP passes; what is paid per plane is the tree's adds and the epilogue.  NP trees do not fit beside
// four output tiles: a wave keeps UT = 2 user tiles of ONE 16-row tile (2 f32x4 per pending subtree and plane), a workgroup steps 16
// rows.  The last two tree levels go through the same LDS exchange, two planes per round: wave w finishes (plane w / 2, tile w % 2).
// Three planes is what the register file takes: with four the trees spill to scratch (profiles/catalog_mrl_softmax_resource_usage.txt).
constexpr int MG_PLANES = 3;
// f(integral_constant<int, 0>), f(<1>), ... in order: a loop whose index is a compile-time constant of each iteration
template <typename F, int... I>
__device__ __forceinline__ void mf_steps(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
struct mf_group {
  int d[MG_PLANES];                              // the prefixes, ascending; entries past NP unused
};
template <typename CT, int NP>
__global__ __launch_bounds__(256) void catalog_scores_mfma_group_kernel(const float* __restrict__ user, long uld, const float* __restrict__ inv_u,
                                                                        const CT* __restrict__ cat, long cld, const float* __restrict__ inv_c, long icld,
                                                                        float* __restrict__ scores, long sld, int B, long N, mf_group g,
                                                                        long rows_per_block, int ub) {
  // plane p: user norms inv_u + p B, row norms inv_c + p icld, scores + p sld (each [B][N])
  constexpr int UT = 2, JMAX = 4;
  extern __shared__ __attribute__((aligned(16))) float us[];       // [64 chains][J][UT][k 4][user 16] | exchange [4 waves][MF_TILES][64] f32x4
  const int D = g.d[NP - 1];
  const int J = (D + 255) >> 8;
  f32x4* ex = reinterpret_cast<f32x4*>(us + J * UT * 64 * 64);
  const int ug = blockIdx.x % ub;
  const long rb = blockIdx.x / ub;
  const int b0 = ug * 16 * UT;
  const int nb = min(16 * UT, B - b0);
  const int D4 = D >> 2;
  for (int i = threadIdx.x; i < 16 * UT * D4; i += 256) {
    const int u = i / D4, d = (i - u * D4) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (u < nb) v = *reinterpret_cast<const float4*>(user + (long)(b0 + u) * uld + d);
    float* q = us + (((((d & 255) >> 2) * J + (d >> 8)) * UT + (u >> 4)) << 6) + (u & 15);
    q[0] = v.w; q[16] = v.z; q[32] = v.y; q[48] = v.x;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, col = lane & 15, k = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long r0 = rb * rows_per_block, r1 = min(N, r0 + rows_per_block);
  for (long n0 = r0; n0 < r1; n0 += 16) {
    const mf_row<CT> bp(cat + min(n0 + col, N - 1) * cld, k);       // a row past the end is read as the last one and never stored
    float bq[3][JMAX];
    f32x4 st[NP][5][UT];                         // st[p][s]: plane p's finished subtree of 2^s chains waiting for its sibling
    // step i - 2 of the 18: the loads of chain i, the products and the tree step of chain i - 2.  The step index is a template argument
    // (mf_steps calls the 18 in order): the tree level of a chain is a constant of its step, in straight-line code.
    const auto step = [&](auto index) __attribute__((always_inline)) {
      constexpr int i = decltype(index)::value - 2;
      if constexpr (i + 2 < 16) {
        constexpr int t = mf_bitrev4(i + 2);
#pragma unroll
        for (int j = 0; j < JMAX; ++j) bq[(i + 2) % 3][j] = bp.at(4 * w + 16 * t + 256 * j < D ? 4 * w + 16 * t + 256 * j : 0);   // (a piece past D: unused)
      }
      if constexpr (i >= 0) {
        const int c = w + 4 * mf_bitrev4(i);
        constexpr int lvl = mf_trailing_ones(i);
        f32x4 acc[UT], snap[NP][UT];             // snap[p]: the chain after its last piece below d_p; +0 without one
#pragma unroll
        for (int x = 0; x < UT; ++x) acc[x] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
          for (int x = 0; x < UT; ++x) snap[p][x] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
          if (4 * c + 256 * j < D) {
            const float* ap = us + (((c * J + j) * UT) << 6) + lane;
#pragma unroll
            for (int x = 0; x < UT; ++x) acc[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[x * 64], bq[i % 3][j], acc[x], 0, 0, 0);
#pragma unroll
            for (int p = 0; p < NP - 1; ++p)
              if (4 * c + 256 * j < g.d[p] && !(4 * c + 256 * (j + 1) < g.d[p])) {      // the chain's last piece below d_p (wave-uniform)
#pragma unroll
                for (int x = 0; x < UT; ++x) snap[p][x] = acc[x];
              }
          }
        }
#pragma unroll
        for (int x = 0; x < UT; ++x) snap[NP - 1][x] = acc[x];      // (d_{NP-1} = D: every piece that was multiplied)
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
          for (int x = 0; x < UT; ++x) {
            f32x4 v = snap[p][x];
#pragma unroll
            for (int s = 0; s < 4; ++s)
              if (s < lvl) v = st[p][s][x] + v;
            st[p][lvl][x] = v;
          }
      }
    };
    mf_steps(step, std::make_integer_sequence<int, 18>{});
#pragma unroll
    for (int p0 = 0; p0 < NP; p0 += 2) {
      __syncthreads();                           // the previous exchange has been read
#pragma unroll
      for (int pp = 0; pp < 2; ++pp)
        if (p0 + pp < NP) {
#pragma unroll
          for (int x = 0; x < UT; ++x) ex[(w * MF_TILES + pp * UT + x) * 64 + lane] = st[p0 + pp][4][x];
        }
      __syncthreads();
      const int p = p0 + (w >> 1), ut = w & 1;   // wave w finishes item w of the round: (plane, user tile)
      const long n = n0 + col;                   // C/D layout: column = lane & 15 (row of the catalogue), row = 4 (lane >> 4) + reg (user)
      if (p < NP && n < N) {
        const f32x4 v = (ex[(0 * MF_TILES + w) * 64 + lane] + ex[(2 * MF_TILES + w) * 64 + lane]) +
                        (ex[(1 * MF_TILES + w) * 64 + lane] + ex[(3 * MF_TILES + w) * 64 + lane]);
        const float ic = inv_c[p * icld + n];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int u = ut * 16 + k * 4 + e;
          if (u < nb) scores[p * sld + (long)(b0 + u) * N + n] = v[e] * inv_u[(long)p * B + b0 + u] * ic;
        }
      }
    }
  }
}

// ---- full-catalogue softmax loss (ur_catalog_softmax, include/unirec_hip_loss.h) ---------------------------------------------------
// Both passes stream the catalogue through the chunk buffer with the scoring launches of select mode.  Every kernel here reduces in
// a fixed order (a thread's strided sequence, wave_sum's tree, the four waves in index order) and nothing is added atomically.
// z_bn is the ROUNDED f32 product s_bn * (1 / tau) wherever it is formed (csm_z: a multiply that is never contracted into the
// subtraction that follows it -- fused, z - max would be the product's rounding residue instead of 0 for the maximum itself), so the
// maximum, the ground truth's z and the exponents agree to the bit and a one-term sum gives exactly 0.
__device__ __forceinline__ float csm_z(float s, float inv_tau) {
#pragma clang fp contract(off)
  return s * inv_tau;
}
//
// item n is excluded for the user of exclusion row ex[0..E) and ground truth g: select mode's rule and its search.  Most of a chunk
// lies outside [first non-negative entry, last entry]: those scores skip the search.
__device__ __forceinline__ bool csm_excluded(const long* __restrict__ ex, int E, long g, long n) {
  return E > 0 && n != g && n <= ex[E - 1] && sel_excluded(ex, E, n);
}
__device__ __forceinline__ float csm_block_sum(float v, float* red) {      // red: 4 floats of LDS; every thread gets the sum
  v = wave_sum(v);
  __syncthreads();                                                          // (red may still be read from the previous reduction)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float csm_block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// Pass 1 and the weights of pass 2 split a user's chunk row over CSM_SEGS workgroups (a few users would otherwise occupy a few compute
// units): segment j owns the rows [j seg, (j + 1) seg) of every chunk and its own running slot [b][j], carried across the chunks in the
// stream's order; the slots of a user are merged in index order at the end.  seg is fixed by the chunk size, so a (shorter) last
// chunk leaves its trailing segments without rows: those keep their slots (or, on the first chunk, initialise them).
// (CSM_SEGS sizes the workspace: catalog_layout.hip.h)

// Pass 1, one workgroup per (user, segment) and chunk: slot (m, l) <- the running maximum and sum_n exp(z_bn - m) over the segment's
// rows seen so far (chunk[b][0..len) = s_bn of catalogue rows c0 .. c0+len).  Two sweeps over the rows (just written: cache
// resident): their maximum, then the sum against max(m, that maximum); the old sum is rescaled once per chunk.
__global__ __launch_bounds__(256) void catalog_softmax_fold_kernel(const float* __restrict__ chunk, long ld, int c0, int len, int seg,
                                                                   const long* __restrict__ gt, const long* __restrict__ exclude, int E,
                                                                   float inv_tau, float* __restrict__ m_run, float* __restrict__ l_run, int first) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int slot = b * CSM_SEGS + blockIdx.y;
  const int n0 = blockIdx.y * seg, n1 = min(len, n0 + seg);
  const float ninf = -__builtin_inff();
  if (n0 >= n1) {                                                           // (uniform)
    if (first && tid == 0) { m_run[slot] = ninf; l_run[slot] = 0.f; }
    return;
  }
  const long g = gt[b];
  const long* ex = E > 0 ? exclude + (long)b * E : nullptr;
  const float* row = chunk + (long)b * ld;
  float mx = ninf;
  for (int n = n0 + tid; n < n1; n += 256)
    if (!csm_excluded(ex, E, g, (long)c0 + n)) mx = fmaxf(mx, csm_z(row[n], inv_tau));
  mx = csm_block_max(mx, red);
  const float m_old = first ? ninf : m_run[slot];
  const float l_old = first ? 0.f : l_run[slot];
  const float m_new = fmaxf(m_old, mx);
  float sum = 0.f;
  if (mx > ninf)                                                            // (uniform; rows that are all excluded add nothing)
    for (int n = n0 + tid; n < n1; n += 256)
      if (!csm_excluded(ex, E, g, (long)c0 + n)) sum += expf(csm_z(row[n], inv_tau) - m_new);
  sum = csm_block_sum(sum, red);
  if (tid == 0) {
    m_run[slot] = m_new;
    l_run[slot] = (m_old > ninf ? l_old * expf(m_old - m_new) : 0.f) + sum;
  }
}

// (m_b, l_b) = the user's CSM_SEGS slots merged in index order; lse_b = m_b + log l_b, row_loss_b = -z_b,g + lse_b (z_b,g from
// catalog_gt_score_kernel's ref: the bits the chunk holds for row g), loss = their mean in a fixed order.  One wave.
__global__ __launch_bounds__(64) void catalog_softmax_finish_kernel(const float* __restrict__ m_run, const float* __restrict__ l_run,
                                                                    const float* __restrict__ ref, float inv_tau, float* __restrict__ lse,
                                                                    float* __restrict__ row_loss, float* __restrict__ loss, int B) {
  float s = 0.f;
  for (int b = threadIdx.x; b < B; b += 64) {
    float m = -__builtin_inff();
    for (int j = 0; j < CSM_SEGS; ++j) m = fmaxf(m, m_run[b * CSM_SEGS + j]);
    float l = 0.f;
    for (int j = 0; j < CSM_SEGS; ++j) {
      const float lj = l_run[b * CSM_SEGS + j];
      if (lj > 0.f) l += lj * expf(m_run[b * CSM_SEGS + j] - m);             // (an empty slot is (-inf, 0))
    }
    const float v = m + logf(l);
    const float r = v - csm_z(ref[b], inv_tau);
    lse[b] = v;
    row_loss[b] = r;
    s += r;
  }
  s = wave_sum(s);
  if (threadIdx.x == 0) loss[0] = s / (float)B;
}

// Pass 2, one workgroup per (user, segment) and chunk: chunk[b][n] <- w_bn * ic_n in place (w_bn = (exp(z_bn - lse_b) - [n == g_b]) / tau,
// 0 for an excluded n) and slot t[b][j] += sum_n w_bn s_bn.
__global__ __launch_bounds__(256) void catalog_softmax_weight_kernel(float* __restrict__ chunk, long ld, int c0, int len, int seg,
                                                                     const float* __restrict__ inv_c, const long* __restrict__ gt,
                                                                     const long* __restrict__ exclude, int E, float inv_tau,
                                                                     const float* __restrict__ lse, float* __restrict__ t_run, int first) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int slot = b * CSM_SEGS + blockIdx.y;
  const int n0 = blockIdx.y * seg, n1 = min(len, n0 + seg);
  if (n0 >= n1) {                                                           // (uniform)
    if (first && tid == 0) t_run[slot] = 0.f;
    return;
  }
  const long g = gt[b];
  const long* ex = E > 0 ? exclude + (long)b * E : nullptr;
  float* row = chunk + (long)b * ld;
  const float ls = lse[b];
  float t = 0.f;
  for (int n = n0 + tid; n < n1; n += 256) {
    const long idx = (long)c0 + n;
    const float s = row[n];
    float w = 0.f;
    if (!csm_excluded(ex, E, g, idx)) {
      float p = expf(csm_z(s, inv_tau) - ls);
      if (idx == g) p -= 1.0f;
      w = p * inv_tau;
    }
    t = fmaf(w, s, t);
    row[n] = w * inv_c[idx];
  }
  t = csm_block_sum(t, red);
  if (tid == 0) t_run[slot] = (first ? 0.f : t_run[slot]) + t;
}

// Pass 2, the gradient product of one chunk: slab[z] [B,D] (+)= W [B x rows of split z] . C [those rows x D] on v_mfma_f32_16x16x4_f32,
// the catalogue-row axis as K (W = the chunk after catalog_softmax_weight_kernel, leading dimension ld; C = the chunk's rows, bf16
// widened exactly on load).  A workgroup = 4 waves owns CSM_USERS users x 256 columns and the rows [z rps, (z+1) rps) of the chunk; wave w
// owns 64 of the columns as four 16-column tiles, tile t holding the columns d0 + 4 c + t (c = the MFMA column), so that a lane
// loads its four tiles' operands of a row as one 16-byte piece and stores its results as 16-byte pieces.  One step takes 16 rows:
// lane (user u, q = lane >> 4) brings W[u][n0 + 4q + j] and lane (q, c) the piece of row n0 + 4q + j for j = 0 .. 3, i.e. the K index
// of MFMA j is q <-> row n0 + 4q + j -- an order of the sum, fixed by (rps, the chunk rows) alone.  A row past the split's end
// enters as zeros on both sides.  Users past B and columns past D are computed on clamped addresses and never stored (an output
// element depends on its own user and column only).  The slabs are accumulated across chunks by the stream's order: the first chunk
// stores, later chunks add; a split without rows in a later (shorter) chunk leaves its slab alone.
// (CSM_UT and CSM_USERS size the workspace: catalog_layout.hip.h)
// (the body: cld = the row stride of cat in elements, D for the contiguous kernel.  With cld above D the product runs over the first D
// columns of rows read in place -- catalog_softmax_grad_prefix_kernel: the slabs are [B,D], and the column clamp min(d, D - 4) keeps
// every load below D, where the row's live data behind the prefix begins.)
template <typename CT>
__device__ __forceinline__ void catalog_softmax_grad_body(const float* __restrict__ wchunk, long ld, int len, const CT* __restrict__ cat, long cld,
                                                          float* __restrict__ slabs, int B, int D, int rps, int first) {
  const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
  const int wave = threadIdx.x >> 6;
  const int b0 = blockIdx.x * CSM_USERS;
  const int d0 = blockIdx.y * 256 + wave * 64;
  if (d0 >= D) return;                                                      // (wave-uniform; the kernel has no barrier)
  const int r0 = blockIdx.z * rps, r1 = min(len, r0 + rps);
  if (r0 >= r1 && !first) return;
  const int d = d0 + 4 * col;
  const CT* cp = cat + min(d, D - 4);
  const float* wp[CSM_UT];
#pragma unroll
  for (int t = 0; t < CSM_UT; ++t) wp[t] = wchunk + (long)min(b0 + t * 16 + col, B - 1) * ld;
  f32x4 acc[CSM_UT][4];
#pragma unroll
  for (int t = 0; t < CSM_UT; ++t)
#pragma unroll
    for (int x = 0; x < 4; ++x) acc[t][x] = f32x4{0.f, 0.f, 0.f, 0.f};
  int n0 = r0;
  for (; n0 + 16 <= r1; n0 += 16) {
    float a[CSM_UT][4];
    float4 c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + 4 * q + j;
      c[j] = load4(cp + (long)n * cld);
#pragma unroll
      for (int t = 0; t < CSM_UT; ++t) a[t][j] = wp[t][n];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int t = 0; t < CSM_UT; ++t) {
        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][j], c[j].x, acc[t][0], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][j], c[j].y, acc[t][1], 0, 0, 0);
        acc[t][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][j], c[j].z, acc[t][2], 0, 0, 0);
        acc[t][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][j], c[j].w, acc[t][3], 0, 0, 0);
      }
  }
  if (n0 < r1) {                                                            // the ragged last step of the split
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + 4 * q + j;
      const bool in = n < r1;
      const int ns = in ? n : r1 - 1;
      float4 c = load4(cp + (long)ns * cld);
      if (!in) c = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int t = 0; t < CSM_UT; ++t) {
        const float a = in ? wp[t][ns] : 0.f;
        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, c.x, acc[t][0], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, c.y, acc[t][1], 0, 0, 0);
        acc[t][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, c.z, acc[t][2], 0, 0, 0);
        acc[t][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, c.w, acc[t][3], 0, 0, 0);
      }
    }
  }
  if (d >= D) return;
  float* slab = slabs + (long)blockIdx.z * B * D;
#pragma unroll
  for (int t = 0; t < CSM_UT; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) {                                           // C/D layout: column = lane & 15, row (user) = 4 (lane >> 4) + register
      const int u = b0 + t * 16 + 4 * q + e;
      if (u < B) {
        float4* o = reinterpret_cast<float4*>(slab + (long)u * D + d);
        float4 v = make_float4(acc[t][0][e], acc[t][1][e], acc[t][2][e], acc[t][3][e]);
        if (!first) { const float4 p = *o; v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w; }
        *o = v;
      }
    }
}
template <typename CT>
__global__ __launch_bounds__(256) void catalog_softmax_grad_kernel(const float* __restrict__ wchunk, long ld, int len, const CT* __restrict__ cat,
                                                                   float* __restrict__ slabs, int B, int D, int rps, int first) {
  catalog_softmax_grad_body<CT>(wchunk, ld, len, cat, (long)D, slabs, B, D, rps, first);
}
template <typename CT>
__global__ __launch_bounds__(256) void catalog_softmax_grad_prefix_kernel(const float* __restrict__ wchunk, long ld, int len, const CT* __restrict__ cat,
                                                                          long cld, float* __restrict__ slabs, int B, int D, int rps, int first) {
  catalog_softmax_grad_body<CT>(wchunk, ld, len, cat, cld, slabs, B, D, rps, first);
}

// d_user[b] = gscale * iu_b * (sum_z slab[z][b] - u_b * iu_b * t_b), the slabs and the slots of t_b added in index order
__global__ __launch_bounds__(256) void catalog_softmax_duser_kernel(const float* __restrict__ user, const float* __restrict__ inv_u,
                                                                    const float* __restrict__ t_run, const float* __restrict__ slabs,
                                                                    float* __restrict__ d_user, int B, int D, int nslab, float gscale) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= (long)B * D) return;
  const int b = (int)(i / D);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int z = 0; z < nslab; ++z) {
    const float4 p = *reinterpret_cast<const float4*>(slabs + (long)z * B * D + i);
    s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
  }
  float t = 0.f;
  for (int j = 0; j < CSM_SEGS; ++j) t += t_run[b * CSM_SEGS + j];
  const float iu = inv_u[b], k = iu * t, gs = gscale * iu;
  const float4 u = *reinterpret_cast<const float4*>(user + i);
  *reinterpret_cast<float4*>(d_user + i) = make_float4(gs * (s.x - u.x * k), gs * (s.y - u.y * k), gs * (s.z - u.z * k), gs * (s.w - u.w * k));
}

// Context MLP, first layer: h1[n][j] = gelu(b1[j] + sum_f W1[j][f] * feat_f(n)), bf16 out.
//   KIND 0: TimestampEncoder features, models/mwne.py:525-565 (9 = secular + 4 sin/cos pairs, all in f32 as the
//           reference computes them from timestamps.float()).
//   KIND 1: GeoCoordinateEncoder features, models/mwne.py:586-607 (lat/lon degrees -> unit-sphere x, y, z).
// The 9- / 3-wide contraction stays on the vector units in f32 (exact features, no padding to an MFMA k-step); the
// second Linear (2H -> H) is an ordinary ur_gemm.
template <int KIND>
__global__ void context_mlp1_kernel(const float* __restrict__ in, const float* __restrict__ W1, const float* __restrict__ b1,
                                    bf16_t* __restrict__ out, long n, int H2) {
  const long row = blockIdx.x;
  if (row >= n) return;
  constexpr int NF = KIND == 0 ? 9 : 3;
  float f[NF];
  if (KIND == 0) {
    const float x = in[row];
    const float year = 31557600.0f, day = 86400.0f, two_pi = 6.283185307179586f;
    f[0] = x / year;
    float r = fmodf(x, day); if (r < 0.f) r += day;              // torch `%` is a floor-mod
    const float day_phase = r / day;
    f[1] = sinf(two_pi * day_phase); f[2] = cosf(two_pi * day_phase);
    const float week_phase = ((x / day) + 4.0f) / 7.0f;
    f[3] = sinf(two_pi * week_phase); f[4] = cosf(two_pi * week_phase);
    float ry = fmodf(x, year); if (ry < 0.f) ry += year;
    const float year_phase = ry / year;
    f[5] = sinf(two_pi * year_phase); f[6] = cosf(two_pi * year_phase);
    const float month_phase = year_phase * 12.0f;
    f[7] = sinf(two_pi * month_phase); f[8] = cosf(two_pi * month_phase);
  } else {
    const float d2r = 0.017453292519943295f;
    const float lat = in[2 * row] * d2r, lon = in[2 * row + 1] * d2r;
    f[0] = cosf(lat) * cosf(lon); f[1] = cosf(lat) * sinf(lon); f[2] = sinf(lat);
  }
  for (int j = threadIdx.x; j < H2; j += blockDim.x) {
    float a = b1[j];
#pragma unroll
    for (int k = 0; k < NF; ++k) a = fmaf(W1[(long)j * NF + k], f[k], a);
    out[row * H2 + j] = f2bf(gelu_erf_f(a));
  }
}

}  // namespace

extern "C" int ur_gather_rows(const void* src, int32_t src_kind, void* out, int32_t out_kind, const int64_t* idx, int64_t row_elems,
                              int64_t n_out, int64_t n_src, void* stream) {
  UR_REQUIRE(n_out >= 0 && n_src >= 0 && row_elems > 0, "ur_gather_rows: bad sizes");
  UR_REQUIRE((src_kind == UR_KIND_U8 || src_kind == UR_KIND_BF16 || src_kind == UR_KIND_F32) &&
             (out_kind == src_kind || (src_kind == UR_KIND_F32 && out_kind == UR_KIND_BF16) ||
              (src_kind == UR_KIND_BF16 && out_kind == UR_KIND_F32)),
             "ur_gather_rows: kinds must match, or f32 -> bf16, or bf16 -> f32");
  if (n_out == 0) return 0;
  UR_REQUIRE(src && out && idx, "ur_gather_rows: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (src_kind == UR_KIND_U8) {
    const long total = n_out * row_elems;
    hipLaunchKernelGGL(gather_bytes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const uint8_t*)src, (const long*)idx,
                       (uint8_t*)out, (long)row_elems, (long)n_out, (long)n_src);
  } else {
    UR_REQUIRE(UR_ALIGNED16(src) && UR_ALIGNED16(out), "ur_gather_rows: rows must be 16-byte aligned");
    const dim3 grid((unsigned)((n_out + 3) / 4)), block(256);
    if (src_kind == UR_KIND_BF16 && out_kind == UR_KIND_F32) {
      UR_REQUIRE((row_elems % 8) == 0, "ur_gather_rows: bf16 -> f32 rows must be multiples of 8 elements");
      hipLaunchKernelGGL((gather_rows_kernel<2, false, true>), grid, block, 0, st, (const char*)src, (const long*)idx, (char*)out, (long)row_elems, (long)n_out, (long)n_src);
    } else if (src_kind == UR_KIND_BF16) {
      UR_REQUIRE((row_elems % 8) == 0, "ur_gather_rows: bf16 rows must be multiples of 8 elements");
      hipLaunchKernelGGL((gather_rows_kernel<2, false>), grid, block, 0, st, (const char*)src, (const long*)idx, (char*)out, (long)row_elems, (long)n_out, (long)n_src);
    } else if (out_kind == UR_KIND_F32) {
      UR_REQUIRE((row_elems % 4) == 0, "ur_gather_rows: f32 rows must be multiples of 4 elements");
      hipLaunchKernelGGL((gather_rows_kernel<4, false>), grid, block, 0, st, (const char*)src, (const long*)idx, (char*)out, (long)row_elems, (long)n_out, (long)n_src);
    } else {
      UR_REQUIRE((row_elems % 8) == 0, "ur_gather_rows: f32 -> bf16 rows must be multiples of 8 elements");
      hipLaunchKernelGGL((gather_rows_kernel<4, true>), grid, block, 0, st, (const char*)src, (const long*)idx, (char*)out, (long)row_elems, (long)n_out, (long)n_src);
    }
  }
  UR_CHECK_LAUNCH("ur_gather_rows");
  return 0;
}

// the vector scoring launch of both modes: rows [0,N) of `catalog` / `cat_inv_norm` into scores [B][N] (leading dimension N);
// who = the entry point the launch is made for, named in a failure
template <typename CT>
static int launch_catalog_scores(const float* user, const float* user_inv_norm, const CT* catalog, const float* cat_inv_norm,
                                 float* scores, int32_t B, int64_t N, int32_t D, hipStream_t st, const char* who) {
  const int ub = ur_cdiv(B, CU_USERS);
  long blocks_x = 2048 / ub;                                  // ~8 workgroups per CU in all
  if (blocks_x < 1) blocks_x = 1;
  long rpb = (N + blocks_x - 1) / blocks_x;
  rpb = (rpb + 3) / 4 * 4;
  blocks_x = (N + rpb - 1) / rpb;
  const size_t smem = (size_t)CU_USERS * D * sizeof(float);
  static std::atomic<uint64_t> attr_set{0};   // per device
  UR_ONCE_PER_DEVICE(attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&catalog_scores_kernel<CT>), hipFuncAttributeMaxDynamicSharedMemorySize, CU_USERS * 2048 * 4);
    if (e != hipSuccess) UR_FAIL((int)e, "%s: hipFuncSetAttribute failed: %s", who, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(catalog_scores_kernel<CT>, dim3((unsigned)blocks_x, (unsigned)ub), dim3(256), smem, st, user, user_inv_norm, catalog,
                     cat_inv_norm, scores, (int)B, (long)N, (int)D, (long)rpb);
  UR_CHECK_LAUNCH(who);
  return 0;
}

// the f32-MFMA scoring launch of the streaming mode: the same arguments, the same scores
template <typename CT>
static int launch_catalog_scores_mfma(const float* user, const float* user_inv_norm, const CT* catalog, const float* cat_inv_norm,
                                      float* scores, int32_t B, int64_t N, int32_t D, hipStream_t st, const char* who) {
  const bool wide = D > 1024;
  const int ub = ur_cdiv(B, wide ? 16 : 32);
  const int group = wide ? 16 * MF_TILES : 16 * MF_TILES / 2;      // rows per step of a workgroup
  long blocks_x = 1024 / ub;                                  // one workgroup per CU at a time (LDS): ~4 rounds
  if (blocks_x < 1) blocks_x = 1;
  long rpb = (N + blocks_x - 1) / blocks_x;
  rpb = (rpb + group - 1) / group * group;
  blocks_x = (N + rpb - 1) / rpb;
  void (*kernel)(const float*, const float*, const CT*, const float*, float*, int, long, int, long, int) =
      wide ? (D == 2048 ? catalog_scores_mfma_kernel<CT, true, true> : catalog_scores_mfma_kernel<CT, true, false>)
           : (D == 1024 ? catalog_scores_mfma_kernel<CT, false, true> : catalog_scores_mfma_kernel<CT, false, false>);
  static std::atomic<uint64_t> attr_set[4];   // per device, one per kernel
  UR_ONCE_PER_DEVICE(attr_set[2 * wide + (D == 1024 || D == 2048)]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mf_lds_bytes(2048, true));
    if (e != hipSuccess) UR_FAIL((int)e, "%s: hipFuncSetAttribute failed: %s", who, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks_x * ub)), dim3(256), mf_lds_bytes(D, wide), st, user, user_inv_norm, catalog, cat_inv_norm,
                     scores, (int)B, (long)N, (int)D, (long)rpb, ub);
  UR_CHECK_LAUNCH(who);
  return 0;
}

// The two launches above on the first D components of rows read in place (user rows uld, catalogue rows cld elements apart): the grids,
// the rows per workgroup and the LDS of the contiguous launch at width D, so a pair has the bits that launch gives on the contiguous
// slices.  With both strides equal to D they ARE the contiguous launches.
template <typename CT>
static int launch_catalog_scores_prefix(const float* user, long uld, const float* user_inv_norm, const CT* catalog, long cld, const float* cat_inv_norm,
                                        float* scores, int32_t B, int64_t N, int32_t D, hipStream_t st, const char* who) {
  if (uld == D && cld == D) return launch_catalog_scores<CT>(user, user_inv_norm, catalog, cat_inv_norm, scores, B, N, D, st, who);
  const int ub = ur_cdiv(B, CU_USERS);
  long blocks_x = 2048 / ub;
  if (blocks_x < 1) blocks_x = 1;
  long rpb = (N + blocks_x - 1) / blocks_x;
  rpb = (rpb + 3) / 4 * 4;
  blocks_x = (N + rpb - 1) / rpb;
  const size_t smem = (size_t)CU_USERS * D * sizeof(float);
  static std::atomic<uint64_t> attr_set{0};   // per device
  UR_ONCE_PER_DEVICE(attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&catalog_scores_prefix_kernel<CT>), hipFuncAttributeMaxDynamicSharedMemorySize, CU_USERS * 2048 * 4);
    if (e != hipSuccess) UR_FAIL((int)e, "%s: hipFuncSetAttribute failed: %s", who, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(catalog_scores_prefix_kernel<CT>, dim3((unsigned)blocks_x, (unsigned)ub), dim3(256), smem, st, user, uld, user_inv_norm, catalog,
                     cld, cat_inv_norm, scores, (int)B, (long)N, (int)D, (long)rpb);
  UR_CHECK_LAUNCH(who);
  return 0;
}
template <typename CT>
static int launch_catalog_scores_mfma_prefix(const float* user, long uld, const float* user_inv_norm, const CT* catalog, long cld,
                                             const float* cat_inv_norm, float* scores, int32_t B, int64_t N, int32_t D, hipStream_t st, const char* who) {
  if (uld == D && cld == D) return launch_catalog_scores_mfma<CT>(user, user_inv_norm, catalog, cat_inv_norm, scores, B, N, D, st, who);
  const bool wide = D > 1024;
  const int ub = ur_cdiv(B, wide ? 16 : 32);
  const int group = wide ? 16 * MF_TILES : 16 * MF_TILES / 2;
  long blocks_x = 1024 / ub;
  if (blocks_x < 1) blocks_x = 1;
  long rpb = (N + blocks_x - 1) / blocks_x;
  rpb = (rpb + group - 1) / group * group;
  blocks_x = (N + rpb - 1) / rpb;
  void (*kernel)(const float*, long, const float*, const CT*, long, const float*, float*, int, long, int, long, int) =
      wide ? catalog_scores_mfma_prefix_kernel<CT, true, false>                // (a prefix is narrower than its row: never 2048)
           : (D == 1024 ? catalog_scores_mfma_prefix_kernel<CT, false, true> : catalog_scores_mfma_prefix_kernel<CT, false, false>);
  static std::atomic<uint64_t> attr_set[3];   // per device, one per kernel
  UR_ONCE_PER_DEVICE(attr_set[wide ? 2 : (D == 1024)]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mf_lds_bytes(2048, true));
    if (e != hipSuccess) UR_FAIL((int)e, "%s: hipFuncSetAttribute failed: %s", who, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks_x * ub)), dim3(256), mf_lds_bytes(D, wide), st, user, uld, user_inv_norm, catalog, cld, cat_inv_norm,
                     scores, (int)B, (long)N, (int)D, (long)rpb, ub);
  UR_CHECK_LAUNCH(who);
  return 0;
}

// one launch of the group scorer: np (2 .. MG_PLANES) prefixes d[0] < .. < d[np-1] <= 1024 of rows [0,N); plane p reads inv_u + p B and
// inv_c + p icld and writes scores + p sld, leading dimension N
template <typename CT>
static int launch_catalog_scores_mfma_group(const float* user, long uld, const float* inv_u, const CT* catalog, long cld, const float* inv_c, long icld,
                                            float* scores, long sld, int32_t B, int64_t N, const int* d, int np, hipStream_t st, const char* who) {
  mf_group g{};
  for (int p = 0; p < np; ++p) g.d[p] = d[p];
  const int D = d[np - 1];
  const int ub = ur_cdiv(B, 32);
  long blocks_x = 1024 / ub;                                  // one workgroup per CU at a time (LDS): ~4 rounds
  if (blocks_x < 1) blocks_x = 1;
  long rpb = (N + blocks_x - 1) / blocks_x;
  rpb = (rpb + 15) / 16 * 16;
  blocks_x = (N + rpb - 1) / rpb;
  void (*kernel)(const float*, long, const float*, const CT*, long, const float*, long, float*, long, int, long, mf_group, long, int) =
      np == 2 ? catalog_scores_mfma_group_kernel<CT, 2> : catalog_scores_mfma_group_kernel<CT, 3>;
  static_assert(MG_PLANES == 3, "one kernel per group size");
  static std::atomic<uint64_t> attr_set[MG_PLANES + 1];   // per device, one per kernel
  UR_ONCE_PER_DEVICE(attr_set[np]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mf_lds_bytes(1024, false));
    if (e != hipSuccess) UR_FAIL((int)e, "%s: hipFuncSetAttribute failed: %s", who, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks_x * ub)), dim3(256), mf_lds_bytes(D, false), st, user, uld, inv_u, catalog, cld, inv_c, icld, scores,
                     sld, (int)B, (long)N, g, (long)rpb, ub);
  UR_CHECK_LAUNCH(who);
  return 0;
}

// which scorer the streaming mode runs when the caller leaves the choice to the library (select.scorer == 0).  Both give the same
// bits, so this is a matter of time alone: docs/lab_notes.md section 22 has the measurements behind it.
// Measured at D = 1024 only (the embedding width of this project): the MFMA scorer wins at every sampled (B, N) on an f32 catalogue
// and at B = 64 and 512 on a bf16 one; at B = 8 on bf16 the two are within 2 %.  Other widths have not been timed and stay on the
// vector scorer.
static bool catalog_default_is_mfma(int32_t B, int32_t D, bool bf16) { return D == 1024 && (B > CU_USERS || !bf16); }
// the one place the `scorer` field of an argument struct becomes a kernel choice
static bool catalog_use_mfma(const catalog_call& c) {
  return c.scorer == UR_CATALOG_SCORER_MFMA || (c.scorer == 0 && catalog_default_is_mfma(c.B, c.D, c.catalog_bf16 == 1));
}

// The two steps the exact streams (select, deep, softmax) share, after every check; inv_u = where the call keeps the user norms.
// Before the first chunk: the user norms, the catalogue norms unless the caller brought them, the ground-truth scores into ref.
template <typename CT>
static int catalog_prologue(const catalog_call& c, const CT* catalog, float* inv_u, int32_t cat_norm_ready, float* ref, hipStream_t st) {
  const float* user = (const float*)c.user;
  float* inv_c = (float*)c.cat_inv_norm;
  hipLaunchKernelGGL(row_inv_norm_kernel<float>, dim3((unsigned)((c.B + 3) / 4)), dim3(256), 0, st, user, inv_u, (long)c.B, (int)c.D);
  if (!cat_norm_ready && c.N > 0)
    hipLaunchKernelGGL(row_inv_norm_kernel<CT>, dim3((unsigned)((c.N + 3) / 4)), dim3(256), 0, st, catalog, inv_c, (long)c.N, (int)c.D);
  if (c.gt && c.N > 0)
    hipLaunchKernelGGL(catalog_gt_score_kernel<CT>, dim3((unsigned)((c.B + 3) / 4)), dim3(256), 0, st, user, (const float*)inv_u, catalog,
                       (const float*)inv_c, (const long*)c.gt, ref, (int)c.B, (long)c.N, (int)c.D);
  UR_CHECK_LAUNCH(c.who);
  return 0;
}

// the scores of catalogue rows [c0, c0 + len) into chunk [B][len]; an empty chunk (N == 0) launches nothing
template <typename CT>
static int catalog_score_chunk(const catalog_call& c, const CT* catalog, const float* inv_u, int64_t c0, int64_t len, float* chunk, hipStream_t st) {
  if (len <= 0) return 0;
  const float* user = (const float*)c.user;
  const float* inv_c = (const float*)c.cat_inv_norm + c0;
  return catalog_use_mfma(c) ? launch_catalog_scores_mfma<CT>(user, inv_u, catalog + c0 * c.D, inv_c, chunk, c.B, len, c.D, st, c.who)
                             : launch_catalog_scores<CT>(user, inv_u, catalog + c0 * c.D, inv_c, chunk, c.B, len, c.D, st, c.who);
}

// the launches of the streaming mode, after every check
template <typename CT>
static int catalog_stream(const catalog_call& c, const CT* catalog, float* inv_u, int32_t cat_norm_ready, const ur_catalog_select_t* select,
                          const select_plan& p, hipStream_t st) {
  char* ws = (char*)select->workspace;
  float* chunk = (float*)(ws + p.chunk);
  float* ref = (float*)(ws + p.ref);
  if (const int rc = catalog_prologue(c, catalog, inv_u, cat_norm_ready, ref, st)) return rc;
  return catalog_for_each_chunk(c.N, p.rows, [&](int64_t c0, int64_t len, int first) {
    if (const int rc = catalog_score_chunk(c, catalog, inv_u, c0, len, chunk, st)) return rc;
    hipLaunchKernelGGL(catalog_select_kernel, dim3((unsigned)c.B), dim3(256), 0, st, (const float*)chunk, (long)len, (int)c0, (int)len, select->K,
                       select->topk_score, select->topk_index, (const long*)c.gt, (const float*)ref, select->rank, (const long*)select->exclude,
                       select->E, first);
    UR_CHECK_LAUNCH(c.who);
    return 0;
  });
}

extern "C" int ur_catalog_scores(const float* user, const float* catalog, float* scores, float* user_inv_norm, float* cat_inv_norm,
                                 int32_t cat_norm_ready, int32_t B, int64_t N, int32_t D, ur_catalog_select_t* select, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!select) {
    UR_REQUIRE(B >= 0 && N >= 0 && D > 0 && (D % 4) == 0 && D <= 2048, "ur_catalog_scores: need D %% 4 == 0 and D <= 2048 (got %d)", D);
    if (B == 0 || N == 0) return 0;
    UR_REQUIRE(user && catalog && scores && user_inv_norm && cat_inv_norm, "ur_catalog_scores: null pointer");
    UR_REQUIRE(UR_ALIGNED16(user) && UR_ALIGNED16(catalog), "ur_catalog_scores: operands must be 16-byte aligned");
    hipLaunchKernelGGL(row_inv_norm_kernel<float>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, user, user_inv_norm, (long)B, (int)D);
    if (!cat_norm_ready)
      hipLaunchKernelGGL(row_inv_norm_kernel<float>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, catalog, cat_inv_norm, (long)N, (int)D);
    return launch_catalog_scores<float>(user, user_inv_norm, catalog, cat_inv_norm, scores, B, N, D, st, "ur_catalog_scores");
  }
  // ---- streaming selection: every check before any launch ----
  const catalog_call c{"ur_catalog_scores", B, N, D, select->E, select->chunk_rows, select->catalog_bf16, select->scorer, select->gt_index,
                       select->rank, select->exclude, user, catalog, cat_inv_norm, select->workspace, select->workspace_bytes};
  if (const int rc = catalog_check_sizes(c, 4, 0, false)) return rc;
  UR_REQUIRE(select->K >= 1 && select->K <= UR_CATALOG_TOPK_MAX, "ur_catalog_scores: select.K must be 1 .. %d (got %d)", UR_CATALOG_TOPK_MAX, select->K);
  const select_plan p = select_layout(B, N, select->chunk_rows);
  if (!select->workspace) {
    select->workspace_bytes = p.need;
    return 0;
  }
  if (const int rc = catalog_check_buffers(c, p.need, false)) return rc;
  if (B == 0) return 0;
  UR_REQUIRE(select->topk_index && select->topk_score && user_inv_norm, "ur_catalog_scores: select.topk_index / topk_score / user_inv_norm are null");
  return catalog_dispatch(c.catalog_bf16 == 1, catalog, [&](auto* cat) {
    return catalog_stream(c, cat, user_inv_norm, cat_norm_ready, select, p, st);
  });
}

// ---- ur_catalog_deep_select (include/unirec_hip_deep.h) --------------------------------------------------------------------------
// the launches, after every check: select mode's norms, reference score and scoring launches; the deep selection kernels
template <typename CT>
static int catalog_deep_stream(const catalog_call& c, const ur_catalog_deep_t* a, const CT* catalog, const deep_plan& p, hipStream_t st) {
  char* ws = (char*)a->workspace;
  float* chunk = (float*)(ws + p.chunk);
  float* ref = (float*)(ws + p.ref);
  float* list_score = (float*)(ws + p.list_score);
  int* list_index = (int*)(ws + p.list_index);
  int* count = (int*)(ws + p.count);
  const long* gt = (const long*)a->gt_index;
  const int B = a->B, K = a->K;
  const int G = deep_segments(a->segments, B, p.rows);             // <= p.gw, what the workspace holds
  const int64_t tiles = p.rows / SEL_TILE;
  const long seg_len = (long)((tiles + G - 1) / G) * SEL_TILE;
  float* inv_u = (float*)(ws + p.inv_u);
  if (const int rc = catalog_prologue(c, catalog, inv_u, a->cat_norm_ready, ref, st)) return rc;
  const int swept = catalog_for_each_chunk(c.N, p.rows, [&](int64_t c0, int64_t len, int first) {
    if (const int rc = catalog_score_chunk(c, catalog, inv_u, c0, len, chunk, st)) return rc;
    hipLaunchKernelGGL(catalog_deep_sweep_kernel, dim3((unsigned)((int64_t)B * G)), dim3(256), 0, st, (const float*)chunk, (long)len, (int)c0,
                       (int)len, K, G, seg_len, list_score, list_index, count, gt, (const float*)ref, (const long*)a->exclude, (int)a->E, first);
    UR_CHECK_LAUNCH(c.who);
    return 0;
  });
  if (swept != 0) return swept;
  hipLaunchKernelGGL(catalog_deep_merge_kernel, dim3((unsigned)B), dim3(256), 0, st, (const float*)list_score, (const int*)list_index,
                     (const int*)count, K, G, a->topk_score, a->topk_index, a->rank);
  UR_CHECK_LAUNCH(c.who);
  return 0;
}

extern "C" int ur_catalog_deep_select(ur_catalog_deep_t* a, void* stream) {
  UR_REQUIRE(a, "ur_catalog_deep_select: null argument struct");
  const catalog_call c{"ur_catalog_deep_select", a->B, a->N, a->D, a->E, a->chunk_rows, a->catalog_bf16, a->scorer, a->gt_index, a->rank,
                       a->exclude, a->user, a->catalog, a->cat_inv_norm, a->workspace, a->workspace_bytes};
  if (const int rc = catalog_check_sizes(c, 4, 0, false)) return rc;
  UR_REQUIRE(a->K >= 1 && a->K <= UR_CATALOG_DEEP_TOPK_MAX, "ur_catalog_deep_select: K must be 1 .. %d (got %d)", UR_CATALOG_DEEP_TOPK_MAX, a->K);
  UR_REQUIRE(a->segments >= 0 && a->segments <= UR_CATALOG_DEEP_SEGMENTS_MAX, "ur_catalog_deep_select: segments must be 0 .. %d (got %d)",
             UR_CATALOG_DEEP_SEGMENTS_MAX, a->segments);
  const deep_plan p = deep_layout(a->B, a->N, a->K, a->chunk_rows, a->segments);
  if (!a->workspace) {
    a->workspace_bytes = p.need;
    return 0;
  }
  if (const int rc = catalog_check_buffers(c, p.need, false)) return rc;
  if (a->B == 0) return 0;
  UR_REQUIRE(a->topk_index && a->topk_score, "ur_catalog_deep_select: topk_index / topk_score are null");
  return catalog_dispatch(c.catalog_bf16 == 1, a->catalog, [&](auto* cat) { return catalog_deep_stream(c, a, cat, p, (hipStream_t)stream); });
}

// ---- ur_catalog_softmax (include/unirec_hip_loss.h) ------------------------------------------------------------------------------
// the launches, after every check: pass 1 folds every chunk into the running (m, l) and finishes the loss; pass 2 (with d_user) scores
// the chunks again, turns them into weights, accumulates the gradient slabs and finishes d_user
template <typename CT>
static int catalog_softmax_stream(const catalog_call& c, const ur_catalog_softmax_t* a, const CT* catalog, const catalog_softmax_plan& p,
                                  hipStream_t st) {
  const int32_t B = a->B, D = a->D, E = a->E;
  char* ws = (char*)a->workspace;
  float* chunk = (float*)(ws + p.chunk);
  float* inv_u = (float*)(ws + p.inv_u);
  float* ref = (float*)(ws + p.ref);
  float* m_run = (float*)(ws + p.m_run);
  float* l_run = (float*)(ws + p.l_run);
  float* t_run = (float*)(ws + p.t_run);
  float* slabs = (float*)(ws + p.slabs);
  const long* gt = (const long*)a->gt_index;
  const long* ex = (const long*)a->exclude;
  const float inv_tau = 1.0f / a->temperature;
  if (const int rc = catalog_prologue(c, catalog, inv_u, a->cat_norm_ready, ref, st)) return rc;
  const int folded = catalog_for_each_chunk(c.N, p.rows, [&](int64_t c0, int64_t len, int first) {
    if (const int rc = catalog_score_chunk(c, catalog, inv_u, c0, len, chunk, st)) return rc;
    hipLaunchKernelGGL(catalog_softmax_fold_kernel, dim3((unsigned)B, CSM_SEGS), dim3(256), 0, st, (const float*)chunk, (long)len, (int)c0, (int)len,
                       p.seg, gt, ex, E, inv_tau, m_run, l_run, first);
    UR_CHECK_LAUNCH(c.who);
    return 0;
  });
  if (folded != 0) return folded;
  hipLaunchKernelGGL(catalog_softmax_finish_kernel, dim3(1), dim3(64), 0, st, (const float*)m_run, (const float*)l_run, (const float*)ref, inv_tau,
                     a->lse, a->row_loss, a->loss, (int)B);
  UR_CHECK_LAUNCH(c.who);
  if (!a->d_user) return 0;
  const int weighted = catalog_for_each_chunk(c.N, p.rows, [&](int64_t c0, int64_t len, int first) {
    if (const int rc = catalog_score_chunk(c, catalog, inv_u, c0, len, chunk, st)) return rc;
    hipLaunchKernelGGL(catalog_softmax_weight_kernel, dim3((unsigned)B, CSM_SEGS), dim3(256), 0, st, chunk, (long)len, (int)c0, (int)len, p.seg,
                       (const float*)a->cat_inv_norm, gt, ex, E, inv_tau, (const float*)a->lse, t_run, first);
    hipLaunchKernelGGL(catalog_softmax_grad_kernel<CT>, dim3((unsigned)ur_cdiv(B, CSM_USERS), (unsigned)ur_cdiv(D, 256), (unsigned)p.nsplit),
                       dim3(256), 0, st, (const float*)chunk, (long)len, (int)len, catalog + c0 * D, slabs, (int)B, (int)D, p.rps, first);
    UR_CHECK_LAUNCH(c.who);
    return 0;
  });
  if (weighted != 0) return weighted;
  hipLaunchKernelGGL(catalog_softmax_duser_kernel, dim3((unsigned)(((long)B * D / 4 + 255) / 256)), dim3(256), 0, st, a->user, (const float*)inv_u,
                     (const float*)t_run, (const float*)slabs, a->d_user, (int)B, (int)D, p.nsplit, a->grad_scale / (float)B);
  UR_CHECK_LAUNCH(c.who);
  return 0;
}

extern "C" int ur_catalog_softmax(ur_catalog_softmax_t* a, void* stream) {
  UR_REQUIRE(a, "ur_catalog_softmax: null argument struct");
  const catalog_call c{"ur_catalog_softmax", a->B, a->N, a->D, a->E, a->chunk_rows, a->catalog_bf16, a->scorer, a->gt_index, nullptr,
                       a->exclude, a->user, a->catalog, a->cat_inv_norm, a->workspace, a->workspace_bytes};
  if (const int rc = catalog_check_sizes(c, 4, 1, true)) return rc;
  UR_REQUIRE(a->temperature > 0.f && a->temperature <= 3.0e38f, "ur_catalog_softmax: temperature must be positive and finite (got %g)", (double)a->temperature);
  const catalog_softmax_plan p = catalog_softmax_layout(a->B, a->N, a->D, a->chunk_rows, a->d_user != nullptr);
  if (!a->workspace) {
    a->workspace_bytes = p.need;
    return 0;
  }
  if (const int rc = catalog_check_buffers(c, p.need, true)) return rc;
  if (a->B == 0) return 0;
  UR_REQUIRE(a->loss && a->row_loss && a->lse, "ur_catalog_softmax: loss / row_loss / lse: null pointer");
  UR_REQUIRE(!a->d_user || UR_ALIGNED16(a->d_user), "ur_catalog_softmax: d_user must be 16-byte aligned");
  return catalog_dispatch(c.catalog_bf16 == 1, a->catalog, [&](auto* cat) { return catalog_softmax_stream(c, a, cat, p, (hipStream_t)stream); });
}

// ---- ur_catalog_mrl_softmax (include/unirec_hip_mrl_loss.h) ------------------------------------------------------------------------
// The stream above on K prefixes of the rows, read in place.  Every plane runs the launches of ur_catalog_softmax at width d_k with the
// row stride D (the *_prefix kernels share their bodies with the contiguous ones; the fold, finish and weight kernels are the unchanged
// ones on the plane's part of the chunk buffer, its norm plane and its slots), so plane k has the bits of that call on the contiguous
// slices -- except that the MFMA scores of up to MG_PLANES planes come from one pass of catalog_scores_mfma_group_kernel.  What the
// planes share besides: one read of the catalogue for all K norm planes, the chunk loop, and the last kernel.
static_assert(CSM_MRL_MAX == UR_MRL_MAX_DIMS && UR_FUNNEL_MAX_DIMS == UR_MRL_MAX_DIMS, "one limit for the prefixes of every family");
struct mrl_softmax_planes {
  int d[UR_MRL_MAX_DIMS];
  float w[UR_MRL_MAX_DIMS];
  long slab[UR_MRL_MAX_DIMS];                  // plane k's slabs, as a float offset from the first plane's
  int nslab[UR_MRL_MAX_DIMS];
};

namespace {
// loss = sum_k w_k plane_loss[k]: fmaf from 0 in ascending k, a plane of weight 0 skipped.  One thread.
__global__ void catalog_mrl_loss_kernel(const float* __restrict__ plane_loss, mrl_softmax_planes pl, int K, float* __restrict__ loss) {
  float s = 0.f;
  for (int k = 0; k < K; ++k)
    if (pl.w[k] > 0.f) s = fmaf(pl.w[k], plane_loss[k], s);
  loss[0] = s;
}

// d_user[b][d] = sum_{k : d < d_k} w_k g_k[b][d]: g_k is catalog_softmax_duser_kernel's expression on plane k's slabs [nslab_k][B][d_k],
// slots t [k][B][CSM_SEGS] and user norm inv_u[k][b]; the sum is fmaf from 0 in ascending k, a plane of weight 0 skipped.
__global__ __launch_bounds__(256) void catalog_mrl_duser_kernel(const float* __restrict__ user, const float* __restrict__ inv_u,
                                                                const float* __restrict__ t_run, const float* __restrict__ slabs,
                                                                float* __restrict__ d_user, int B, int D, mrl_softmax_planes pl, int K, float gscale) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= (long)B * D) return;
  const int b = (int)(i / D), d = (int)(i - (long)b * D);
  const float4 u = *reinterpret_cast<const float4*>(user + i);
  float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = 0; p < K; ++p) {
    const int dk = pl.d[p];
    if (d >= dk || !(pl.w[p] > 0.f)) continue;
    const float* sl = slabs + pl.slab[p] + (long)b * dk + d;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int z = 0; z < pl.nslab[p]; ++z) {
      const float4 q = *reinterpret_cast<const float4*>(sl + (long)z * B * dk);
      s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w;
    }
    float t = 0.f;
    for (int j = 0; j < CSM_SEGS; ++j) t += t_run[((long)p * B + b) * CSM_SEGS + j];
    const float iu = inv_u[(long)p * B + b], k = iu * t, gs = gscale * iu;
    const float4 g = make_float4(gs * (s.x - u.x * k), gs * (s.y - u.y * k), gs * (s.z - u.z * k), gs * (s.w - u.w * k));
    const float w = pl.w[p];
    out = make_float4(fmaf(w, g.x, out.x), fmaf(w, g.y, out.y), fmaf(w, g.z, out.z), fmaf(w, g.w, out.w));
  }
  *reinterpret_cast<float4*>(d_user + i) = out;
}
}  // namespace

template <typename CT>
static int catalog_mrl_softmax_stream(const catalog_call& c, const ur_catalog_mrl_softmax_t* a, const CT* catalog, const catalog_mrl_softmax_plan& p,
                                      hipStream_t st) {
  const int32_t B = a->B, D = a->D, E = a->E, K = a->K;
  const int64_t N = a->N;
  char* ws = (char*)a->workspace;
  float* chunk = (float*)(ws + p.chunk);
  float* inv_u = (float*)(ws + p.inv_u);
  float* ref = (float*)(ws + p.ref);
  float* m_run = (float*)(ws + p.m_run);
  float* l_run = (float*)(ws + p.l_run);
  float* t_run = (float*)(ws + p.t_run);
  float* slabs = (float*)(ws + p.slabs[0]);
  const long* gt = (const long*)a->gt_index;
  const long* ex = (const long*)a->exclude;
  const float* user = a->user;
  float* inv_c = a->cat_inv_norm;
  const float inv_tau = 1.0f / a->temperature;
  const bool mfma = catalog_use_mfma(c);                        // by the call's (B, D), for every plane: the bits do not depend on it
  prefix_dims dims{};
  mrl_softmax_planes pl{};
  for (int k = 0; k < K; ++k) {
    dims.d[k] = pl.d[k] = a->dims[k];
    pl.w[k] = a->weights[k];
    pl.slab[k] = (long)((p.slabs[k] - p.slabs[0]) / 4);
    pl.nslab[k] = p.nsplit[k];
  }
  // the norms of every prefix, users and catalogue, one read each; the ground-truth scores per plane
  hipLaunchKernelGGL(row_prefix_inv_norm_kernel<float>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, user, (long)D, inv_u, (long)B, dims, (int)K);
  if (!a->cat_norm_ready)
    hipLaunchKernelGGL(row_prefix_inv_norm_kernel<CT>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, catalog, (long)D, inv_c, (long)N, dims, (int)K);
  for (int k = 0; k < K; ++k)
    hipLaunchKernelGGL(catalog_gt_score_prefix_kernel<CT>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, user, (long)D, (const float*)(inv_u + (long)k * B),
                       catalog, (long)D, (const float*)(inv_c + (long)k * N), gt, ref + (long)k * B, (int)B, (long)N, (int)pl.d[k]);
  UR_CHECK_LAUNCH(c.who);
  // the scores of rows [c0, c0 + len) on every plane.  MFMA: runs of up to MG_PLANES planes no wider than 1024 take one pass of the group
  // scorer; a plane left alone, or wider than 1024, takes the stride-aware single-plane launch.  Vector: one launch per plane.
  const auto score_planes = [&](int64_t c0, int64_t len) {
    for (int k = 0; k < K;) {
      float* out = chunk + (long)k * B * p.rows;
      const float* iu = inv_u + (long)k * B;
      const float* ic = inv_c + (long)k * N + c0;
      int np = 1;
      while (mfma && k + np < K && np < MG_PLANES && pl.d[k + np] <= 1024) ++np;
      const int rc = np > 1 ? launch_catalog_scores_mfma_group<CT>(user, (long)D, iu, catalog + c0 * D, (long)D, ic, (long)N, out, (long)B * p.rows, B, len,
                                                                   pl.d + k, np, st, c.who)
                     : mfma ? launch_catalog_scores_mfma_prefix<CT>(user, (long)D, iu, catalog + c0 * D, (long)D, ic, out, B, len, pl.d[k], st, c.who)
                            : launch_catalog_scores_prefix<CT>(user, (long)D, iu, catalog + c0 * D, (long)D, ic, out, B, len, pl.d[k], st, c.who);
      if (rc != 0) return rc;
      k += np;
    }
    return 0;
  };
  const int folded = catalog_for_each_chunk(N, p.rows, [&](int64_t c0, int64_t len, int first) {
    if (const int rc = score_planes(c0, len)) return rc;
    for (int k = 0; k < K; ++k)
      hipLaunchKernelGGL(catalog_softmax_fold_kernel, dim3((unsigned)B, CSM_SEGS), dim3(256), 0, st, (const float*)(chunk + (long)k * B * p.rows), (long)len,
                         (int)c0, (int)len, p.seg, gt, ex, E, inv_tau, m_run + (long)k * B * CSM_SEGS, l_run + (long)k * B * CSM_SEGS, first);
    UR_CHECK_LAUNCH(c.who);
    return 0;
  });
  if (folded != 0) return folded;
  for (int k = 0; k < K; ++k)
    hipLaunchKernelGGL(catalog_softmax_finish_kernel, dim3(1), dim3(64), 0, st, (const float*)(m_run + (long)k * B * CSM_SEGS),
                       (const float*)(l_run + (long)k * B * CSM_SEGS), (const float*)(ref + (long)k * B), inv_tau, a->lse + (long)k * B,
                       a->row_loss + (long)k * B, a->plane_loss + k, (int)B);
  hipLaunchKernelGGL(catalog_mrl_loss_kernel, dim3(1), dim3(1), 0, st, (const float*)a->plane_loss, pl, (int)K, a->loss);
  UR_CHECK_LAUNCH(c.who);
  if (!a->d_user) return 0;
  const int weighted = catalog_for_each_chunk(N, p.rows, [&](int64_t c0, int64_t len, int first) {
    if (const int rc = score_planes(c0, len)) return rc;
    for (int k = 0; k < K; ++k) {
      float* wk = chunk + (long)k * B * p.rows;
      const int dk = pl.d[k];
      hipLaunchKernelGGL(catalog_softmax_weight_kernel, dim3((unsigned)B, CSM_SEGS), dim3(256), 0, st, wk, (long)len, (int)c0, (int)len, p.seg,
                         (const float*)(inv_c + (long)k * N), gt, ex, E, inv_tau, (const float*)(a->lse + (long)k * B), t_run + (long)k * B * CSM_SEGS,
                         first);
      const dim3 grid((unsigned)ur_cdiv(B, CSM_USERS), (unsigned)ur_cdiv(dk, 256), (unsigned)p.nsplit[k]);
      if (dk == D)
        hipLaunchKernelGGL(catalog_softmax_grad_kernel<CT>, grid, dim3(256), 0, st, (const float*)wk, (long)len, (int)len, catalog + c0 * D,
                           slabs + pl.slab[k], (int)B, (int)D, p.rps[k], first);
      else
        hipLaunchKernelGGL(catalog_softmax_grad_prefix_kernel<CT>, grid, dim3(256), 0, st, (const float*)wk, (long)len, (int)len, catalog + c0 * D, (long)D,
                           slabs + pl.slab[k], (int)B, dk, p.rps[k], first);
    }
    UR_CHECK_LAUNCH(c.who);
    return 0;
  });
  if (weighted != 0) return weighted;
  hipLaunchKernelGGL(catalog_mrl_duser_kernel, dim3((unsigned)(((long)B * D / 4 + 255) / 256)), dim3(256), 0, st, user, (const float*)inv_u,
                     (const float*)t_run, (const float*)slabs, a->d_user, (int)B, (int)D, pl, (int)K, a->grad_scale / (float)B);
  UR_CHECK_LAUNCH(c.who);
  return 0;
}

extern "C" int ur_catalog_mrl_softmax(ur_catalog_mrl_softmax_t* a, void* stream) {
  UR_REQUIRE(a, "ur_catalog_mrl_softmax: null argument struct");
  const catalog_call c{"ur_catalog_mrl_softmax", a->B, a->N, a->D, a->E, a->chunk_rows, a->catalog_bf16, a->scorer, a->gt_index, nullptr,
                       a->exclude, a->user, a->catalog, a->cat_inv_norm, a->workspace, a->workspace_bytes};
  if (const int rc = catalog_check_sizes(c, 4, 1, true)) return rc;
  const int32_t K = a->K;
  UR_REQUIRE(K >= 1 && K <= UR_MRL_MAX_DIMS, "ur_catalog_mrl_softmax: K must be 1 .. %d (got %d)", UR_MRL_MAX_DIMS, K);
  const int mult = a->catalog_bf16 == 1 ? 8 : 4;
  bool any = false;
  for (int k = 0; k < K; ++k) {
    const int32_t d = a->dims[k];
    UR_REQUIRE(d > 0 && (d % mult) == 0, "ur_catalog_mrl_softmax: dims[%d] must be a positive multiple of %d (got %d)", k, mult, d);
    UR_REQUIRE(k == 0 || d > a->dims[k - 1], "ur_catalog_mrl_softmax: dims must be strictly ascending (dims[%d] = %d after %d)", k, d, a->dims[k - 1]);
    const float w = a->weights[k];
    UR_REQUIRE(w >= 0.f && w <= 3.0e38f, "ur_catalog_mrl_softmax: weights[%d] must be finite and >= 0 (got %g)", k, (double)w);
    any = any || w > 0.f;
  }
  UR_REQUIRE(a->dims[K - 1] == a->D, "ur_catalog_mrl_softmax: the last of dims must equal D (got %d, D %d)", a->dims[K - 1], a->D);
  UR_REQUIRE(any, "ur_catalog_mrl_softmax: weights must hold at least one positive entry");
  UR_REQUIRE(a->temperature > 0.f && a->temperature <= 3.0e38f, "ur_catalog_mrl_softmax: temperature must be positive and finite (got %g)",
             (double)a->temperature);
  const catalog_mrl_softmax_plan p = catalog_mrl_softmax_layout(a->B, a->N, K, a->dims, a->chunk_rows, a->d_user != nullptr);
  if (!a->workspace) {
    a->workspace_bytes = p.need;
    return 0;
  }
  if (const int rc = catalog_check_buffers(c, p.need, true)) return rc;
  if (a->B == 0) return 0;
  UR_REQUIRE(a->plane_loss && a->loss && a->row_loss && a->lse, "ur_catalog_mrl_softmax: plane_loss / loss / row_loss / lse: null pointer");
  UR_REQUIRE(!a->d_user || UR_ALIGNED16(a->d_user), "ur_catalog_mrl_softmax: d_user must be 16-byte aligned");
  return catalog_dispatch(c.catalog_bf16 == 1, a->catalog, [&](auto* cat) { return catalog_mrl_softmax_stream(c, a, cat, p, (hipStream_t)stream); });
}

extern "C" int ur_rank_of_index(const float* scores, const int64_t* gt_index, int32_t* rank, int32_t B, int64_t N, void* stream) {
  UR_REQUIRE(B >= 0 && N > 0, "ur_rank_of_index: bad sizes");
  if (B == 0) return 0;
  UR_REQUIRE(scores && gt_index && rank, "ur_rank_of_index: null pointer");
  hipLaunchKernelGGL(rank_of_index_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, scores, (const long*)gt_index, rank, (long)N);
  UR_CHECK_LAUNCH("ur_rank_of_index");
  return 0;
}

extern "C" int ur_context_mlp1(const float* in, int32_t kind, const float* W1, const float* b1, void* out, int64_t n, int32_t H2, void* stream) {
  UR_REQUIRE((kind == 0 || kind == 1) && n >= 0 && H2 > 0, "ur_context_mlp1: kind must be 0 (timestamp) or 1 (lat/lon), n >= 0");
  if (n == 0) return 0;
  UR_REQUIRE(in && W1 && b1 && out, "ur_context_mlp1: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (kind == 0) hipLaunchKernelGGL((context_mlp1_kernel<0>), dim3((unsigned)n), dim3(256), 0, st, in, W1, b1, (bf16_t*)out, (long)n, (int)H2);
  else hipLaunchKernelGGL((context_mlp1_kernel<1>), dim3((unsigned)n), dim3(256), 0, st, in, W1, b1, (bf16_t*)out, (long)n, (int)H2);
  UR_CHECK_LAUNCH("ur_context_mlp1");
  return 0;
}
