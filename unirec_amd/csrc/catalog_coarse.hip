// Two-stage retrieval (include/unirec_hip_coarse.h), gfx950 only.
//
//   ur_catalog_coarse_select : an APPROXIMATE shortlist over a bf16 catalogue.  The users are rounded to bf16 once; per chunk of rows
//                              catalog_scores_bf16_kernel writes s~_bn = ((u~_b . c_n) * iu~_b) * ic_n on v_mfma_f32_16x16x32_bf16 into
//                              the chunk buffer and catalog_select_kernel (catalog_select.hip.h, the kernel of ur_catalog_scores' select
//                              mode, unchanged) folds it into the lists and the rank counts.
//   ur_catalog_rerank        : the EXACT scores of a shortlist, catalog_scores_kernel's own chain per (user, slot), sorted per user.
//
// Long two-stage retrieval (include/unirec_hip_coarse_deep.h), the same two halves with lists of up to 1024 items:
//
//   ur_catalog_coarse_deep_select : the cast, norms, diagonal launch and chunk launches of ur_catalog_coarse_select, each chunk folded by
//                                   catalog_deep_sweep_kernel and the lists joined by catalog_deep_merge_kernel (catalog_deep.hip.h, the
//                                   kernels of ur_catalog_deep_select, unchanged; this unit compiles its own copy as catalog.hip does).
//   ur_catalog_deep_rerank        : the same chain per (user, slot) in a launch of its own, one wave per pair, then one workgroup per
//                                   user sorts up to 1024 pairs.
//
// Funnel retrieval (include/unirec_hip_funnel.h), the long two-stage pair on prefixes of the embedding, read in place with a row stride:
//
//   ur_catalog_prefix_norms  : the row-norm chain with a snapshot per prefix boundary, one read of the catalogue for all planes.
//   ur_catalog_funnel_select : a strided cast of the user prefix, catalog_scores_bf16_prefix_kernel (the coarse scorer with a catalogue
//                              row stride) and the sweep / merge kernels of catalog_deep.hip.h, unchanged.
//   ur_catalog_funnel_rerank : the scoring launch of ur_catalog_deep_rerank with both strides, then its sorting launch, unchanged.
//
// The headers hold the definitions in full; the comments here are about the placement.
#include "common.hip.h"
#include "unirec_hip.h"
#include "unirec_hip_coarse.h"
#include "unirec_hip_coarse_deep.h"
#include "unirec_hip_funnel.h"
#include "unirec_hip_mrl.h"
#include "catalog_select.hip.h"
#include "catalog_deep.hip.h"

namespace {

// ---- the coarse scorer ------------------------------------------------------------------------------------------------------------
// A workgroup = CC_WAVES waves owns 16 UT users and a range of catalogue rows.  A = users (row = user), B = catalogue rows (column =
// row n), K = the embedding axis: lane l of v_mfma_f32_16x16x32_bf16 holds A[l & 15][8 (l >> 4) + j] and B[8 (l >> 4) + j][l & 15],
// j = 0 .. 7, and C[4 (l >> 4) + e][l & 15], e = 0 .. 3.
//   Users: the bf16 copy is staged once in LDS in operand order, us[step s][user tile t][lane][8]: a wave's ds_read_b128 of one operand
//   is 1024 contiguous bytes.  The staged row is padded with zeros to a multiple of 32 elements.
//   Catalogue: rows are K-contiguous, so the lane's operand of step s is the 16 bytes at row n, element 32 s + 8 (l >> 4): straight from
//   global memory, no LDS (an element is used once per user group).  A lane whose 8 elements lie past D takes zeros (D % 8 == 0: a
//   lane's piece is wholly inside or wholly outside).
//   A wave takes CC_RT 16-row tiles per step and all UT user tiles.  The K steps s = 0, 1, .. of an output tile are dealt to NC chains,
//   step s to chain s % NC, each chain ascending from C = 0, and the chains are added at the end, c0 + c1 (NC = 2, D <= 1024) or
//   (c0 + c2) + (c1 + c3) (NC = 4, D > 1024) -- the order of the sum is fixed by D alone.  One chain over all of D = 2048 (64 dependent
//   f32 additions) measured 4.4 x the error of the exact scorer's lane chains + tree and missed the tests' bound; 16 steps per chain at
//   most keep it inside.  UT CC_RT NC = 16 independent accumulators keep the matrix pipe busy between dependent steps, and an A
//   operand read from LDS serves CC_RT MFMAs.
// User group: UT = 4 (64 users) for D <= 1024, UT = 2 (32 users) above: 128 KB of LDS at D = 1024 and at D = 2048, one workgroup of 8
// waves per compute unit there.  The alternative, 32 users and two workgroups per CU, doubles the times the catalogue is read (once per
// user group); the catalogue bytes are what this kernel waits for (2 KB per row against 64 x 1024 MACs at a matrix rate that finishes them
// in a fraction of the load's time), so the larger group was chosen and the latency is covered by 8 waves with unrolled loads in flight.
// Blocks of the same row range and different user groups are adjacent in the grid (the user group is the fast index), so the re-reads
// of a row range run together and meet in the L2 / Infinity Cache.
//   Diagonal mode (gt != NULL): "row" n is the virtual row of user n, catalogue row gt[n]; a workgroup visits the virtual rows of its own
//   users only and stores the diagonal, ref[b] = s~_b,gt[b] -- the same instructions in the same order as the chunk pass runs for that
//   pair, hence the same bits.
constexpr int CC_WAVES = 8;
constexpr int CC_RT = 2;
constexpr int CC_ROWS = CC_WAVES * CC_RT * 16;          // catalogue rows per workgroup step
constexpr int CC_ACCS = 16;                             // 16x16 accumulators of a wave: UT x CC_RT tiles x NC chains
constexpr int CC_LDS_MAX = 128 * 1024;
__host__ __device__ constexpr int cc_steps(int D) { return (D + 31) >> 5; }
__host__ __device__ constexpr size_t cc_lds_bytes(int D, int ut) { return (size_t)cc_steps(D) * ut * 64 * 16; }
static_assert(cc_lds_bytes(1024, 4) <= CC_LDS_MAX && cc_lds_bytes(2048, 2) <= CC_LDS_MAX, "the user group must fit the LDS budget");
static_assert(UR_COARSE_USER_GROUP == 16 * 4, "the header documents the user group of D <= 1024");

template <int UT>
__global__ __launch_bounds__(CC_WAVES * 64) void catalog_scores_bf16_kernel(const bf16_t* __restrict__ user, const float* __restrict__ inv_u,
                                                                           const bf16_t* __restrict__ cat, const float* __restrict__ inv_c,
                                                                           float* __restrict__ scores, long ld, const long* __restrict__ gt,
                                                                           float* __restrict__ ref, int B, long N, int D, long rows_per_block,
                                                                           int ub) {
  constexpr int NC = CC_ACCS / (UT * CC_RT);                       // chains of the K axis
  static_assert(NC == 2 || NC == 4, "the epilogue adds two or four chains");
  extern __shared__ __attribute__((aligned(16))) bf16_t cus[];     // [steps][UT][64 lanes][8]
  const int S = cc_steps(D);
  const int ug = blockIdx.x % ub;
  const long rb = blockIdx.x / ub;
  const int b0 = ug * 16 * UT;
  const int nb = min(16 * UT, B - b0);
  const int P = S * 4;                                             // 8-element pieces of a padded row
  // 64 threads = 16 users x 4 consecutive pieces: 64-byte runs of a user's row in, 1024 contiguous bytes of LDS out
  for (int i = threadIdx.x; i < 16 * UT * P; i += CC_WAVES * 64) {
    const int ul = i & 15, p = (i >> 4) % P, ut = (i >> 4) / P;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (p * 8 < D) v = *reinterpret_cast<const uint4*>(user + (long)min(b0 + ut * 16 + ul, B - 1) * D + p * 8);
    *reinterpret_cast<uint4*>(cus + ((((p >> 2) * UT + ut) * 64 + ul + 16 * (p & 3)) << 3)) = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, col = lane & 15, kq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool diag = gt != nullptr;
  const long r0 = diag ? (long)b0 : rb * rows_per_block;
  const long r1 = diag ? (long)(b0 + nb) : min(N, r0 + rows_per_block);
  const int S_full = D >> 5;
  const bf16_t* ap = cus + (lane << 3);
  for (long n0 = r0 + w * 16 * CC_RT; n0 < r1; n0 += CC_ROWS) {
    const bf16_t* bp[CC_RT];                     // a row past the end is read as the last one and never stored
    long crow[CC_RT];
#pragma unroll
    for (int r = 0; r < CC_RT; ++r) {
      const long n = min(n0 + r * 16 + col, r1 - 1);
      crow[r] = diag ? min(max(gt[n], 0L), N - 1) : n;
      bp[r] = cat + crow[r] * D + 8 * kq;
    }
    f32x4 acc[NC][UT][CC_RT];
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int t = 0; t < UT; ++t)
#pragma unroll
        for (int r = 0; r < CC_RT; ++r) acc[j][t][r] = f32x4{0.f, 0.f, 0.f, 0.f};
    // step s of chain j: PART = the K step that ends short (lanes past D bring zeros; the staged users are padded)
    auto step = [&](int s, f32x4 (&c)[UT][CC_RT], bool part) {
      const bool in = !part || 32 * s + 8 * kq < D;
      bf16x8 b[CC_RT];
#pragma unroll
      for (int r = 0; r < CC_RT; ++r) {
        b[r] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (in) b[r] = *reinterpret_cast<const bf16x8*>(bp[r] + 32 * s);
      }
#pragma unroll
      for (int t = 0; t < UT; ++t) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(ap + ((s * UT + t) << 9));
#pragma unroll
        for (int r = 0; r < CC_RT; ++r) c[t][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[r], c[t][r], 0, 0, 0);
      }
    };
    int s0 = 0;
    for (; s0 + NC <= S_full; s0 += NC) {
#pragma unroll
      for (int j = 0; j < NC; ++j) step(s0 + j, acc[j], false);
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {               // the last, incomplete round: step s still goes to chain s % NC (wave-uniform conditions)
      if (s0 + j < S_full) step(s0 + j, acc[j], false);
      else if (s0 + j == S_full && S_full < S) step(s0 + j, acc[j], true);
    }
#pragma unroll
    for (int t = 0; t < UT; ++t)
#pragma unroll
      for (int r = 0; r < CC_RT; ++r) {
        if (NC == 2) acc[0][t][r] = acc[0][t][r] + acc[1][t][r];
        else acc[0][t][r] = (acc[0][t][r] + acc[2 % NC][t][r]) + (acc[1][t][r] + acc[3 % NC][t][r]);
      }
#pragma unroll
    for (int r = 0; r < CC_RT; ++r) {
      const long n = n0 + r * 16 + col;          // C/D layout: column = lane & 15 (row of the catalogue), row = 4 (lane >> 4) + reg (user)
      if (n < r1) {
        const float ic = inv_c[crow[r]];
#pragma unroll
        for (int t = 0; t < UT; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int u = t * 16 + kq * 4 + e;
            if (u < nb) {
              const float v = acc[0][t][r][e] * inv_u[b0 + u] * ic;
              if (!diag) scores[(long)(b0 + u) * ld + n] = v;
              else if ((long)(b0 + u) == n) ref[n] = v;
            }
          }
      }
    }
  }
}

// ---- the exact re-rank ------------------------------------------------------------------------------------------------------------
// One workgroup = 4 waves per user.  Wave w scores the slots w, w + 4, ..: catalog_scores_kernel's dot product on (user b, row
// index[b][slot]) -- the same lane -> element map, the same fmaf chain, the same wave_sum and the same two multiplies, as
// catalog_gt_score_kernel does for one row per user -- so the score has the bits that kernel writes for the pair.  An index outside
// [0, N) is an empty slot (-inf, SEL_EMPTY).  Then a bitonic sort of the 128 slots under the total order of the lists; the first k leave.
constexpr int RR_SLOTS = UR_CATALOG_TOPK_MAX;
static_assert((RR_SLOTS & (RR_SLOTS - 1)) == 0 && RR_SLOTS <= 256, "the sort takes a power of two, one pair per thread at most");
template <typename CT>
__global__ __launch_bounds__(256) void catalog_rerank_kernel(const float* __restrict__ user, const float* __restrict__ inv_u,
                                                             const CT* __restrict__ cat, const float* __restrict__ inv_c,
                                                             const int* __restrict__ index, int K_in, int k, int* __restrict__ topk_index,
                                                             float* __restrict__ topk_score, long N, int D) {
  __shared__ float ks[RR_SLOTS];
  __shared__ int ki[RR_SLOTS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const float* up = user + (long)b * D;
  const float iu = inv_u[b];
  for (int slot = wave; slot < RR_SLOTS; slot += 4) {
    float s = -__builtin_inff();
    int id = SEL_EMPTY;
    const int g = slot < K_in ? index[(long)b * K_in + slot] : -1;       // (wave-uniform)
    if (g >= 0 && (long)g < N) {
      const CT* cp = cat + (long)g * D;
      float acc = 0.f;
      for (int d = lane * 4; d < D; d += 256) {
        const float4 c = load4(cp + d);
        const float4 x = *reinterpret_cast<const float4*>(up + d);
        acc = fmaf(c.x, x.x, fmaf(c.y, x.y, fmaf(c.z, x.z, fmaf(c.w, x.w, acc))));
      }
      const float ic = inv_c[g];
      s = wave_sum(acc) * iu * ic;
      id = g;
    }
    if (lane == 0) { ks[slot] = s; ki[slot] = id; }
  }
  __syncthreads();
  for (int kk = 2; kk <= RR_SLOTS; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      const int i = tid, q = i ^ j;
      if (i < RR_SLOTS && q > i) {
        const float si = ks[i], sq = ks[q];
        const int ii = ki[i], iq = ki[q];
        const bool up_ = (i & kk) == 0;                                 // this pair ends in list order (best first)
        if (up_ ? sel_before(sq, iq, si, ii) : sel_before(si, ii, sq, iq)) { ks[i] = sq; ki[i] = iq; ks[q] = si; ki[q] = ii; }
      }
      __syncthreads();
    }
  }
  if (tid < k) {
    topk_score[(long)b * k + tid] = ks[tid];
    topk_index[(long)b * k + tid] = ki[tid] == SEL_EMPTY ? -1 : ki[tid];
  }
}

// ---- the exact re-rank of a long shortlist (ur_catalog_deep_rerank) -----------------------------------------------------------------
// catalog_rerank_kernel gives one workgroup per user every slot: at 1024 slots a wave would walk 256 rows one after the other, each a
// dependent fetch through index[], and 64 users would occupy a quarter of the compute units.  Here the scoring is a launch of its own,
// one wave per (user, slot): workgroup (x, y) = slots 4 x .. 4 x + 3 of the users y, y + gridDim.y, ..; the chain is the one above, so
// the bits are.  A wave writes its score (-inf for an empty slot) to score[b][slot]; the pairing with index[b][slot] is positional.
// Then one workgroup per user loads its K_in pairs into LDS (2 x 4 x 1024 = 8 KB), pads them to the next power of two with empty slots
// and sorts them with the bitonic helper of catalog_deep.hip.h (one compare-exchange pair per thread and step); the first k leave.
// Neither launch's result depends on its grid: a score is a function of its pair, a list of its user's pairs.
// (DR_SLOTS, DR_GRID_Y_MAX and the sorting kernel, catalog_deep_rerank_sort_kernel, are in catalog_deep.hip.h: ur_catalog_fp8_rerank of
// catalog_fp8.hip runs the same sorting launch)
template <typename CT>
__global__ __launch_bounds__(256) void catalog_deep_rerank_score_kernel(const float* __restrict__ user, const float* __restrict__ inv_u,
                                                                        const CT* __restrict__ cat, const float* __restrict__ inv_c,
                                                                        const int* __restrict__ index, int K_in, float* __restrict__ score,
                                                                        int B, long N, int D) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (slot >= K_in) return;                                              // (wave-uniform; no barrier in this kernel)
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float* up = user + (long)b * D;
    const float iu = inv_u[b];
    float s = -__builtin_inff();
    const int g = index[(long)b * K_in + slot];                          // (wave-uniform)
    if (g >= 0 && (long)g < N) {
      const CT* cp = cat + (long)g * D;
      float acc = 0.f;
      for (int d = lane * 4; d < D; d += 256) {
        const float4 c = load4(cp + d);
        const float4 x = *reinterpret_cast<const float4*>(up + d);
        acc = fmaf(c.x, x.x, fmaf(c.y, x.y, fmaf(c.z, x.z, fmaf(c.w, x.w, acc))));
      }
      const float ic = inv_c[g];
      s = wave_sum(acc) * iu * ic;
    }
    if (lane == 0) score[(long)b * K_in + slot] = s;
  }
}

// one launch of the coarse scorer: rows [0,N) of `cat` / `inv_c` into scores [B][ld], or (gt != NULL) the diagonal into ref [B]
int launch_catalog_scores_bf16(const bf16_t* user, const float* inv_u, const bf16_t* cat, const float* inv_c, float* scores, long ld,
                               const long* gt, float* ref, int32_t B, int64_t N, int32_t D, hipStream_t st) {
  const bool wide = D > 1024;
  const int ut = wide ? 2 : 4;
  const int ub = ur_cdiv(B, 16 * ut);
  long blocks_x = 1, rpb = N;
  if (!gt) {
    blocks_x = 512 / ub;                                        // ~2 rounds of one workgroup per CU; a workgroup stages its users once
    if (blocks_x < 1) blocks_x = 1;
    rpb = (N + blocks_x - 1) / blocks_x;
    rpb = (rpb + CC_ROWS - 1) / CC_ROWS * CC_ROWS;
    blocks_x = (N + rpb - 1) / rpb;
  }
  void (*kernel)(const bf16_t*, const float*, const bf16_t*, const float*, float*, long, const long*, float*, int, long, int, long, int) =
      wide ? catalog_scores_bf16_kernel<2> : catalog_scores_bf16_kernel<4>;
  static std::atomic<uint64_t> attr_set[2];   // per device, one per kernel
  UR_ONCE_PER_DEVICE(attr_set[wide]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, CC_LDS_MAX);
    if (e != hipSuccess) UR_FAIL((int)e, "ur_catalog_coarse_select: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks_x * ub)), dim3(CC_WAVES * 64), cc_lds_bytes(D, ut), st, user, inv_u, cat, inv_c, scores, ld,
                     gt, ref, (int)B, (long)N, (int)D, rpb, ub);
  UR_CHECK_LAUNCH("ur_catalog_coarse_select");
  return 0;
}

}  // namespace

extern "C" int ur_catalog_coarse_select(ur_catalog_coarse_t* a, void* stream) {
  UR_REQUIRE(a, "ur_catalog_coarse_select: null argument struct");
  const catalog_call c{"ur_catalog_coarse_select", a->B, a->N, a->D, a->E, a->chunk_rows, a->catalog_bf16, 0, a->gt_index, a->rank, a->exclude,
                       a->user, a->catalog, a->cat_inv_norm, a->workspace, a->workspace_bytes};
  if (const int rc = catalog_check_sizes(c, 8, 0, false)) return rc;
  const int32_t B = a->B, D = a->D, K = a->K, E = a->E;
  const int64_t N = a->N;
  UR_REQUIRE(K >= 1 && K <= UR_CATALOG_TOPK_MAX, "ur_catalog_coarse_select: K must be 1 .. %d (got %d)", UR_CATALOG_TOPK_MAX, K);
  UR_REQUIRE(a->catalog_bf16 == 1, "ur_catalog_coarse_select: catalog_bf16 must be 1, the coarse scorer reads a bf16 catalogue only (got %d)",
             a->catalog_bf16);
  const coarse_plan p = coarse_layout(B, N, D, a->chunk_rows);
  if (!a->workspace) {
    a->workspace_bytes = p.need;
    return 0;
  }
  if (const int rc = catalog_check_buffers(c, p.need, false)) return rc;
  if (B == 0) return 0;
  UR_REQUIRE(a->topk_index && a->topk_score, "ur_catalog_coarse_select: topk_index / topk_score are null");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)a->workspace;
  bf16_t* ubf = (bf16_t*)(ws + p.user);
  float* inv_u = (float*)(ws + p.inv_u);
  float* ref = (float*)(ws + p.ref);
  float* chunk = (float*)(ws + p.chunk);
  const bf16_t* cat = (const bf16_t*)a->catalog;
  const long* gt = (const long*)a->gt_index;
  int rc = ur_cast_f32_to_bf16(a->user, ubf, (int64_t)B * D, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(row_inv_norm_kernel<bf16_t>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, (const bf16_t*)ubf, inv_u, (long)B, (int)D);
  if (!a->cat_norm_ready && N > 0)
    hipLaunchKernelGGL(row_inv_norm_kernel<bf16_t>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, cat, a->cat_inv_norm, (long)N, (int)D);
  UR_CHECK_LAUNCH("ur_catalog_coarse_select");
  if (gt && N > 0) {
    rc = launch_catalog_scores_bf16(ubf, inv_u, cat, a->cat_inv_norm, nullptr, 0, gt, ref, B, N, D, st);
    if (rc != 0) return rc;
  }
  return catalog_for_each_chunk(N, p.rows, [&](int64_t c0, int64_t len, int first) {
    if (len > 0) {
      const int rc = launch_catalog_scores_bf16(ubf, inv_u, cat + c0 * D, a->cat_inv_norm + c0, chunk, (long)len, nullptr, nullptr, B, len, D, st);
      if (rc != 0) return rc;
    }
    hipLaunchKernelGGL(catalog_select_kernel, dim3((unsigned)B), dim3(256), 0, st, (const float*)chunk, (long)len, (int)c0, (int)len, (int)K,
                       a->topk_score, a->topk_index, gt, (const float*)ref, a->rank, (const long*)a->exclude, (int)E, first);
    UR_CHECK_LAUNCH("ur_catalog_coarse_select");
    return 0;
  });
}

extern "C" int ur_catalog_rerank(ur_catalog_rerank_t* a, void* stream) {
  UR_REQUIRE(a, "ur_catalog_rerank: null argument struct");
  const int32_t B = a->B, D = a->D;
  const int64_t N = a->N;
  UR_REQUIRE(B >= 0, "ur_catalog_rerank: need B >= 0 (got %d)", B);
  UR_REQUIRE(N >= 1 && N <= (int64_t)INT32_MAX, "ur_catalog_rerank: need 1 <= N <= INT32_MAX (got %lld)", (long long)N);
  UR_REQUIRE(a->catalog_bf16 == 0 || a->catalog_bf16 == 1, "ur_catalog_rerank: catalog_bf16 must be 0 or 1 (got %d)", a->catalog_bf16);
  const bool bf16 = a->catalog_bf16 == 1;
  UR_REQUIRE(D > 0 && (D % (bf16 ? 8 : 4)) == 0 && D <= 2048,
             "ur_catalog_rerank: D must be a positive multiple of %d and <= 2048 (got %d)", bf16 ? 8 : 4, D);
  UR_REQUIRE(a->K_in >= 1 && a->K_in <= UR_CATALOG_TOPK_MAX, "ur_catalog_rerank: K_in must be 1 .. %d (got %d)", UR_CATALOG_TOPK_MAX, a->K_in);
  UR_REQUIRE(a->k >= 1 && a->k <= a->K_in, "ur_catalog_rerank: k must be 1 .. K_in = %d (got %d)", a->K_in, a->k);
  ws_carver carve;                                             // the workspace: inv_u [B], nothing else
  const int64_t inv_u_at = carve.take((int64_t)B * 4), need = carve.need();
  if (!a->workspace) {
    a->workspace_bytes = need;
    return 0;
  }
  UR_REQUIRE(UR_ALIGNED16(a->workspace) && a->workspace_bytes >= need,
             "ur_catalog_rerank: workspace must be 16-byte aligned and hold %lld bytes (got %lld)", (long long)need, (long long)a->workspace_bytes);
  if (B == 0) return 0;
  UR_REQUIRE(a->index && a->topk_index && a->topk_score, "ur_catalog_rerank: index / topk_index / topk_score are null");
  UR_REQUIRE(a->user && a->catalog && a->cat_inv_norm, "ur_catalog_rerank: user / catalog / cat_inv_norm: null pointer");
  UR_REQUIRE(UR_ALIGNED16(a->user) && UR_ALIGNED16(a->catalog), "ur_catalog_rerank: user and catalog must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  float* inv_u = (float*)((char*)a->workspace + inv_u_at);
  hipLaunchKernelGGL(row_inv_norm_kernel<float>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, a->user, inv_u, (long)B, (int)D);
  return catalog_dispatch(bf16, a->catalog, [&](auto* cat) {
    using CT = std::remove_const_t<std::remove_pointer_t<decltype(cat)>>;
    if (!a->cat_norm_ready)
      hipLaunchKernelGGL(row_inv_norm_kernel<CT>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, cat, a->cat_inv_norm, (long)N, (int)D);
    hipLaunchKernelGGL(catalog_rerank_kernel<CT>, dim3((unsigned)B), dim3(256), 0, st, a->user, (const float*)inv_u, cat,
                       (const float*)a->cat_inv_norm, a->index, (int)a->K_in, (int)a->k, a->topk_index, a->topk_score, (long)N, (int)D);
    UR_CHECK_LAUNCH("ur_catalog_rerank");
    return 0;
  });
}

// ---- include/unirec_hip_coarse_deep.h ---------------------------------------------------------------------------------------------
extern "C" int ur_catalog_coarse_deep_select(ur_catalog_coarse_deep_t* a, void* stream) {
  UR_REQUIRE(a, "ur_catalog_coarse_deep_select: null argument struct");
  const catalog_call c{"ur_catalog_coarse_deep_select", a->B, a->N, a->D, a->E, a->chunk_rows, a->catalog_bf16, 0, a->gt_index, a->rank,
                       a->exclude, a->user, a->catalog, a->cat_inv_norm, a->workspace, a->workspace_bytes};
  if (const int rc = catalog_check_sizes(c, 8, 0, false)) return rc;
  const int32_t B = a->B, D = a->D, K = a->K, E = a->E;
  const int64_t N = a->N;
  UR_REQUIRE(K >= 1 && K <= UR_CATALOG_DEEP_TOPK_MAX, "ur_catalog_coarse_deep_select: K must be 1 .. %d (got %d)", UR_CATALOG_DEEP_TOPK_MAX, K);
  UR_REQUIRE(a->catalog_bf16 == 1,
             "ur_catalog_coarse_deep_select: catalog_bf16 must be 1, the coarse scorer reads a bf16 catalogue only (got %d)", a->catalog_bf16);
  UR_REQUIRE(a->segments >= 0 && a->segments <= UR_CATALOG_DEEP_SEGMENTS_MAX, "ur_catalog_coarse_deep_select: segments must be 0 .. %d (got %d)",
             UR_CATALOG_DEEP_SEGMENTS_MAX, a->segments);
  const coarse_deep_plan p = coarse_deep_layout(B, N, D, K, a->chunk_rows, a->segments);
  if (!a->workspace) {
    a->workspace_bytes = p.need;
    return 0;
  }
  if (const int rc = catalog_check_buffers(c, p.need, false)) return rc;
  if (B == 0) return 0;
  UR_REQUIRE(a->topk_index && a->topk_score, "ur_catalog_coarse_deep_select: topk_index / topk_score are null");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)a->workspace;
  bf16_t* ubf = (bf16_t*)(ws + p.user);
  float* inv_u = (float*)(ws + p.inv_u);
  float* ref = (float*)(ws + p.ref);
  float* chunk = (float*)(ws + p.chunk);
  float* list_score = (float*)(ws + p.list_score);
  int* list_index = (int*)(ws + p.list_index);
  int* count = (int*)(ws + p.count);
  const bf16_t* cat = (const bf16_t*)a->catalog;
  const long* gt = (const long*)a->gt_index;
  const int G = deep_segments(a->segments, B, p.rows);             // <= p.gw, what the workspace holds
  const int64_t tiles = p.rows / SEL_TILE;
  const long seg_len = (long)((tiles + G - 1) / G) * SEL_TILE;
  // the sequence of ur_catalog_coarse_select: cast, norms, the diagonal launch, then the chunks
  int rc = ur_cast_f32_to_bf16(a->user, ubf, (int64_t)B * D, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(row_inv_norm_kernel<bf16_t>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, (const bf16_t*)ubf, inv_u, (long)B, (int)D);
  if (!a->cat_norm_ready && N > 0)
    hipLaunchKernelGGL(row_inv_norm_kernel<bf16_t>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, cat, a->cat_inv_norm, (long)N, (int)D);
  UR_CHECK_LAUNCH(c.who);
  if (gt && N > 0) {
    rc = launch_catalog_scores_bf16(ubf, inv_u, cat, a->cat_inv_norm, nullptr, 0, gt, ref, B, N, D, st);
    if (rc != 0) return rc;
  }
  rc = catalog_for_each_chunk(N, p.rows, [&](int64_t c0, int64_t len, int first) {
    if (len > 0) {
      const int rc = launch_catalog_scores_bf16(ubf, inv_u, cat + c0 * D, a->cat_inv_norm + c0, chunk, (long)len, nullptr, nullptr, B, len, D, st);
      if (rc != 0) return rc;
    }
    hipLaunchKernelGGL(catalog_deep_sweep_kernel, dim3((unsigned)((int64_t)B * G)), dim3(256), 0, st, (const float*)chunk, (long)len, (int)c0,
                       (int)len, (int)K, G, seg_len, list_score, list_index, count, gt, (const float*)ref, (const long*)a->exclude, (int)E, first);
    UR_CHECK_LAUNCH(c.who);
    return 0;
  });
  if (rc != 0) return rc;
  hipLaunchKernelGGL(catalog_deep_merge_kernel, dim3((unsigned)B), dim3(256), 0, st, (const float*)list_score, (const int*)list_index,
                     (const int*)count, (int)K, G, a->topk_score, a->topk_index, a->rank);
  UR_CHECK_LAUNCH(c.who);
  return 0;
}

extern "C" int ur_catalog_deep_rerank(ur_catalog_deep_rerank_t* a, void* stream) {
  UR_REQUIRE(a, "ur_catalog_deep_rerank: null argument struct");
  const int32_t B = a->B, D = a->D;
  const int64_t N = a->N;
  UR_REQUIRE(B >= 0, "ur_catalog_deep_rerank: need B >= 0 (got %d)", B);
  UR_REQUIRE(N >= 1 && N <= (int64_t)INT32_MAX, "ur_catalog_deep_rerank: need 1 <= N <= INT32_MAX (got %lld)", (long long)N);
  UR_REQUIRE(a->catalog_bf16 == 0 || a->catalog_bf16 == 1, "ur_catalog_deep_rerank: catalog_bf16 must be 0 or 1 (got %d)", a->catalog_bf16);
  const bool bf16 = a->catalog_bf16 == 1;
  UR_REQUIRE(D > 0 && (D % (bf16 ? 8 : 4)) == 0 && D <= 2048,
             "ur_catalog_deep_rerank: D must be a positive multiple of %d and <= 2048 (got %d)", bf16 ? 8 : 4, D);
  UR_REQUIRE(a->K_in >= 1 && a->K_in <= UR_CATALOG_DEEP_TOPK_MAX, "ur_catalog_deep_rerank: K_in must be 1 .. %d (got %d)",
             UR_CATALOG_DEEP_TOPK_MAX, a->K_in);
  UR_REQUIRE(a->k >= 1 && a->k <= a->K_in, "ur_catalog_deep_rerank: k must be 1 .. K_in = %d (got %d)", a->K_in, a->k);
  const deep_rerank_plan p = deep_rerank_layout(B, a->K_in);
  if (!a->workspace) {
    a->workspace_bytes = p.need;
    return 0;
  }
  UR_REQUIRE(UR_ALIGNED16(a->workspace) && a->workspace_bytes >= p.need,
             "ur_catalog_deep_rerank: workspace must be 16-byte aligned and hold %lld bytes (got %lld)", (long long)p.need,
             (long long)a->workspace_bytes);
  if (B == 0) return 0;
  UR_REQUIRE(a->index && a->topk_index && a->topk_score, "ur_catalog_deep_rerank: index / topk_index / topk_score are null");
  UR_REQUIRE(a->user && a->catalog && a->cat_inv_norm, "ur_catalog_deep_rerank: user / catalog / cat_inv_norm: null pointer");
  UR_REQUIRE(UR_ALIGNED16(a->user) && UR_ALIGNED16(a->catalog), "ur_catalog_deep_rerank: user and catalog must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  float* inv_u = (float*)((char*)a->workspace + p.inv_u);
  float* score = (float*)((char*)a->workspace + p.score);
  const int K_in = a->K_in;
  hipLaunchKernelGGL(row_inv_norm_kernel<float>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, a->user, inv_u, (long)B, (int)D);
  return catalog_dispatch(bf16, a->catalog, [&](auto* cat) {
    using CT = std::remove_const_t<std::remove_pointer_t<decltype(cat)>>;
    if (!a->cat_norm_ready)
      hipLaunchKernelGGL(row_inv_norm_kernel<CT>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, cat, a->cat_inv_norm, (long)N, (int)D);
    hipLaunchKernelGGL(catalog_deep_rerank_score_kernel<CT>, dim3((unsigned)((K_in + 3) / 4), (unsigned)(B < DR_GRID_Y_MAX ? B : DR_GRID_Y_MAX)),
                       dim3(256), 0, st, a->user, (const float*)inv_u, cat, (const float*)a->cat_inv_norm, a->index, K_in, score, (int)B, (long)N,
                       (int)D);
    hipLaunchKernelGGL(catalog_deep_rerank_sort_kernel, dim3((unsigned)B), dim3(256), 0, st, (const float*)score, a->index, K_in, (int)a->k,
                       a->topk_index, a->topk_score, (long)N);
    UR_CHECK_LAUNCH("ur_catalog_deep_rerank");
    return 0;
  });
}

// ---- include/unirec_hip_funnel.h --------------------------------------------------------------------------------------------------
namespace {

static_assert(UR_FUNNEL_MAX_DIMS == UR_MRL_MAX_DIMS, "a funnel takes the prefixes a Matryoshka head trains");
static_assert(UR_FUNNEL_USER_GROUP == UR_COARSE_USER_GROUP, "the prefix scorer keeps the user groups of the contiguous one");

// (the row norms of L prefixes in one read, row_prefix_inv_norm_kernel, are in catalog_select.hip.h: the Matryoshka softmax loss of
// catalog.hip takes them too)

// user [B, ldu] f32 -> out [B, dim] bf16, nearest even: the bits ur_cast_f32_to_bf16 gives on the contiguous copy user[:, :dim]
__global__ void cast_prefix_kernel(const float* __restrict__ user, long ldu, bf16_t* __restrict__ out, int B, int dim) {
  const int P = dim >> 3;
  const long total = (long)B * P, stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long b = i / P;
    const int p = (int)(i - b * P);
    const float* s = user + b * ldu + p * 8;
    const float4 lo = *reinterpret_cast<const float4*>(s), hi = *reinterpret_cast<const float4*>(s + 4);
    *reinterpret_cast<uint4*>(out + b * dim + p * 8) =
        make_uint4(pack_bf2(lo.x, lo.y), pack_bf2(lo.z, lo.w), pack_bf2(hi.x, hi.y), pack_bf2(hi.z, hi.w));
  }
}

// ---- the prefix scorer ------------------------------------------------------------------------------------------------------------
// catalog_scores_bf16_kernel on the first D components of catalogue rows that are `cld` elements apart.  The users arrive as the
// contiguous bf16 block [B, D] the entry point cast, so the staging, the operand layout, the chains (step s to chain s % NC, NC by D
// alone) and the epilogue are that kernel's, instruction for instruction: a pair has the bits the contiguous kernel gives it on the
// copy.  What differs is the catalogue side of a lane's address, row * cld, and what lies behind the prefix: elements D .. cld - 1 of
// a row are live data, so the K step that ends short is masked by D -- a lane whose 8 elements start at or past D loads nothing and
// brings zeros, wherever the row ends.  A lane reads 16 bytes at row * cld + 32 s + 8 kq only when 32 s + 8 kq + 8 <= D <= cld.
// A wave's load of one step touches 16 rows x 64 bytes: whole 64-byte pieces of rows cld apart (cld % 8 == 0 keeps them 16-byte
// aligned); consecutive steps walk each row's prefix front to back.
template <int UT, int NC>
__global__ __launch_bounds__(CC_WAVES * 64) void catalog_scores_bf16_prefix_kernel(const bf16_t* __restrict__ user, const float* __restrict__ inv_u,
                                                                                  const bf16_t* __restrict__ cat, long cld,
                                                                                  const float* __restrict__ inv_c, float* __restrict__ scores,
                                                                                  long ld, const long* __restrict__ gt, float* __restrict__ ref,
                                                                                  int B, long N, int D, long rows_per_block, int ub) {
  static_assert(NC == 2 || NC == 4, "the epilogue adds two or four chains");
  extern __shared__ __attribute__((aligned(16))) bf16_t cus[];     // [steps][UT][64 lanes][8]
  const int S = cc_steps(D);
  const int ug = blockIdx.x % ub;
  const long rb = blockIdx.x / ub;
  const int b0 = ug * 16 * UT;
  const int nb = min(16 * UT, B - b0);
  const int P = S * 4;                                             // 8-element pieces of a padded row
  for (int i = threadIdx.x; i < 16 * UT * P; i += CC_WAVES * 64) {
    const int ul = i & 15, p = (i >> 4) % P, ut = (i >> 4) / P;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (p * 8 < D) v = *reinterpret_cast<const uint4*>(user + (long)min(b0 + ut * 16 + ul, B - 1) * D + p * 8);
    *reinterpret_cast<uint4*>(cus + ((((p >> 2) * UT + ut) * 64 + ul + 16 * (p & 3)) << 3)) = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, col = lane & 15, kq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool diag = gt != nullptr;
  const long r0 = diag ? (long)b0 : rb * rows_per_block;
  const long r1 = diag ? (long)(b0 + nb) : min(N, r0 + rows_per_block);
  const int S_full = D >> 5;
  const bf16_t* ap = cus + (lane << 3);
  for (long n0 = r0 + w * 16 * CC_RT; n0 < r1; n0 += CC_ROWS) {
    const bf16_t* bp[CC_RT];                     // a row past the end is read as the last one and never stored
    long crow[CC_RT];
#pragma unroll
    for (int r = 0; r < CC_RT; ++r) {
      const long n = min(n0 + r * 16 + col, r1 - 1);
      crow[r] = diag ? min(max(gt[n], 0L), N - 1) : n;
      bp[r] = cat + crow[r] * cld + 8 * kq;
    }
    f32x4 acc[NC][UT][CC_RT];
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int t = 0; t < UT; ++t)
#pragma unroll
        for (int r = 0; r < CC_RT; ++r) acc[j][t][r] = f32x4{0.f, 0.f, 0.f, 0.f};
    // step s of chain j: PART = the K step that ends short of 32 elements -- masked by D, the prefix, not by the row's end
    auto step = [&](int s, f32x4 (&c)[UT][CC_RT], bool part) {
      const bool in = !part || 32 * s + 8 * kq < D;
      bf16x8 b[CC_RT];
#pragma unroll
      for (int r = 0; r < CC_RT; ++r) {
        b[r] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (in) b[r] = *reinterpret_cast<const bf16x8*>(bp[r] + 32 * s);
      }
#pragma unroll
      for (int t = 0; t < UT; ++t) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(ap + ((s * UT + t) << 9));
#pragma unroll
        for (int r = 0; r < CC_RT; ++r) c[t][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[r], c[t][r], 0, 0, 0);
      }
    };
    int s0 = 0;
    for (; s0 + NC <= S_full; s0 += NC) {
#pragma unroll
      for (int j = 0; j < NC; ++j) step(s0 + j, acc[j], false);
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {               // the last, incomplete round: step s still goes to chain s % NC (wave-uniform conditions)
      if (s0 + j < S_full) step(s0 + j, acc[j], false);
      else if (s0 + j == S_full && S_full < S) step(s0 + j, acc[j], true);
    }
#pragma unroll
    for (int t = 0; t < UT; ++t)
#pragma unroll
      for (int r = 0; r < CC_RT; ++r) {
        if (NC == 2) acc[0][t][r] = acc[0][t][r] + acc[1][t][r];
        else acc[0][t][r] = (acc[0][t][r] + acc[2 % NC][t][r]) + (acc[1][t][r] + acc[3 % NC][t][r]);
      }
#pragma unroll
    for (int r = 0; r < CC_RT; ++r) {
      const long n = n0 + r * 16 + col;
      if (n < r1) {
        const float ic = inv_c[crow[r]];
#pragma unroll
        for (int t = 0; t < UT; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int u = t * 16 + kq * 4 + e;
            if (u < nb) {
              const float v = acc[0][t][r][e] * inv_u[b0 + u] * ic;
              if (!diag) scores[(long)(b0 + u) * ld + n] = v;
              else if ((long)(b0 + u) == n) ref[n] = v;
            }
          }
      }
    }
  }
}

// one launch of the prefix scorer, the grid of launch_catalog_scores_bf16: rows [0,N) of `cat` (stride cld) / `inv_c` into scores [B][ld],
// or (gt != NULL) the diagonal into ref [B].  The user group is a function of dim alone.
int launch_catalog_scores_bf16_prefix(const bf16_t* user, const float* inv_u, const bf16_t* cat, long cld, const float* inv_c, float* scores,
                                      long ld, const long* gt, float* ref, int32_t B, int64_t N, int32_t dim, hipStream_t st) {
  const bool wide = dim > 1024;
  const int ut = wide ? 2 : 4;
  static_assert(UR_FUNNEL_USER_GROUP == 16 * 4, "the header documents the user group of dim <= 1024");
  const int ub = ur_cdiv(B, 16 * ut);
  long blocks_x = 1, rpb = N;
  if (!gt) {
    blocks_x = 512 / ub;
    if (blocks_x < 1) blocks_x = 1;
    rpb = (N + blocks_x - 1) / blocks_x;
    rpb = (rpb + CC_ROWS - 1) / CC_ROWS * CC_ROWS;
    blocks_x = (N + rpb - 1) / rpb;
  }
  void (*kernel)(const bf16_t*, const float*, const bf16_t*, long, const float*, float*, long, const long*, float*, int, long, int, long, int) =
      wide ? catalog_scores_bf16_prefix_kernel<2, 4> : catalog_scores_bf16_prefix_kernel<4, 2>;
  static std::atomic<uint64_t> attr_set[2];   // per device, one per kernel
  UR_ONCE_PER_DEVICE(attr_set[wide]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, CC_LDS_MAX);
    if (e != hipSuccess) UR_FAIL((int)e, "ur_catalog_funnel_select: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks_x * ub)), dim3(CC_WAVES * 64), cc_lds_bytes(dim, ut), st, user, inv_u, cat, cld, inv_c, scores,
                     ld, gt, ref, (int)B, (long)N, (int)dim, rpb, ub);
  UR_CHECK_LAUNCH("ur_catalog_funnel_select");
  return 0;
}

// the scoring launch of ur_catalog_deep_rerank with the two row strides; the chain runs over d < D
template <typename CT>
__global__ __launch_bounds__(256) void catalog_funnel_rerank_score_kernel(const float* __restrict__ user, long ldu, const float* __restrict__ inv_u,
                                                                          const CT* __restrict__ cat, long cld, const float* __restrict__ inv_c,
                                                                          const int* __restrict__ index, int K_in, float* __restrict__ score,
                                                                          int B, long N, int D) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (slot >= K_in) return;                                              // (wave-uniform; no barrier in this kernel)
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float* up = user + (long)b * ldu;
    const float iu = inv_u[b];
    float s = -__builtin_inff();
    const int g = index[(long)b * K_in + slot];                          // (wave-uniform)
    if (g >= 0 && (long)g < N) {
      const CT* cp = cat + (long)g * cld;
      float acc = 0.f;
      for (int d = lane * 4; d < D; d += 256) {
        const float4 c = load4(cp + d);
        const float4 x = *reinterpret_cast<const float4*>(up + d);
        acc = fmaf(c.x, x.x, fmaf(c.y, x.y, fmaf(c.z, x.z, fmaf(c.w, x.w, acc))));
      }
      const float ic = inv_c[g];
      s = wave_sum(acc) * iu * ic;
    }
    if (lane == 0) score[(long)b * K_in + slot] = s;
  }
}

template <typename CT>
void launch_prefix_norm(const CT* x, long ld, float* inv, long rows, int dim, hipStream_t st) {
  prefix_dims dims{};
  dims.d[0] = dim;
  hipLaunchKernelGGL(row_prefix_inv_norm_kernel<CT>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, ld, inv, rows, dims, 1);
}

}  // namespace

extern "C" int ur_catalog_prefix_norms(const ur_catalog_prefix_norms_t* a, void* stream) {
  UR_REQUIRE(a, "ur_catalog_prefix_norms: null argument struct");
  UR_REQUIRE(a->catalog_bf16 == 0 || a->catalog_bf16 == 1, "ur_catalog_prefix_norms: catalog_bf16 must be 0 or 1 (got %d)", a->catalog_bf16);
  const bool bf16 = a->catalog_bf16 == 1;
  const int mult = bf16 ? 8 : 4;
  const int64_t N = a->N;
  UR_REQUIRE(N >= 0 && N <= (int64_t)INT32_MAX, "ur_catalog_prefix_norms: need 0 <= N <= INT32_MAX (got %lld)", (long long)N);
  UR_REQUIRE(a->L >= 1 && a->L <= UR_FUNNEL_MAX_DIMS, "ur_catalog_prefix_norms: L must be 1 .. %d (got %d)", UR_FUNNEL_MAX_DIMS, a->L);
  UR_REQUIRE(a->ld > 0 && (a->ld % mult) == 0, "ur_catalog_prefix_norms: ld must be a positive multiple of %d (got %lld)", mult, (long long)a->ld);
  prefix_dims dims{};
  for (int l = 0; l < a->L; ++l) {
    const int32_t d = a->dims[l];
    UR_REQUIRE(d > 0 && (d % mult) == 0 && d <= 2048, "ur_catalog_prefix_norms: dims[%d] must be a positive multiple of %d and <= 2048 (got %d)", l,
               mult, d);
    UR_REQUIRE((int64_t)d <= a->ld, "ur_catalog_prefix_norms: dims[%d] = %d exceeds ld = %lld", l, d, (long long)a->ld);
    UR_REQUIRE(l == 0 || d > a->dims[l - 1], "ur_catalog_prefix_norms: dims must be strictly ascending (dims[%d] = %d after %d)", l, d,
               a->dims[l - 1]);
    dims.d[l] = d;
  }
  if (N == 0) return 0;
  UR_REQUIRE(a->catalog && a->inv, "ur_catalog_prefix_norms: catalog / inv: null pointer");
  UR_REQUIRE(UR_ALIGNED16(a->catalog), "ur_catalog_prefix_norms: catalog must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  return catalog_dispatch(bf16, a->catalog, [&](auto* cat) {
    using CT = std::remove_const_t<std::remove_pointer_t<decltype(cat)>>;
    hipLaunchKernelGGL(row_prefix_inv_norm_kernel<CT>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, cat, (long)a->ld, a->inv, (long)N, dims,
                       (int)a->L);
    UR_CHECK_LAUNCH("ur_catalog_prefix_norms");
    return 0;
  });
}

extern "C" int ur_catalog_funnel_select(ur_catalog_funnel_select_t* a, void* stream) {
  UR_REQUIRE(a, "ur_catalog_funnel_select: null argument struct");
  const catalog_call c{"ur_catalog_funnel_select", a->B, a->N, 8 /* dim has its own checks below */, a->E, a->chunk_rows, a->catalog_bf16, 0,
                       a->gt_index, a->rank, a->exclude, a->user, a->catalog, a->cat_inv_norm, a->workspace, a->workspace_bytes};
  if (const int rc = catalog_check_sizes(c, 8, 0, false)) return rc;
  const int32_t B = a->B, dim = a->dim, K = a->K, E = a->E;
  const int64_t N = a->N, cld = a->ld, ldu = a->ldu;
  UR_REQUIRE(dim > 0 && (dim % 8) == 0 && dim <= 2048, "ur_catalog_funnel_select: dim must be a positive multiple of 8 and <= 2048 (got %d)", dim);
  UR_REQUIRE(cld >= dim, "ur_catalog_funnel_select: ld must be at least dim = %d (got %lld)", dim, (long long)cld);
  UR_REQUIRE(ldu >= dim, "ur_catalog_funnel_select: ldu must be at least dim = %d (got %lld)", dim, (long long)ldu);
  UR_REQUIRE((cld % 8) == 0, "ur_catalog_funnel_select: ld must be a multiple of 8, every bf16 row 16-byte aligned (got %lld)", (long long)cld);
  UR_REQUIRE((ldu % 4) == 0, "ur_catalog_funnel_select: ldu must be a multiple of 4, every f32 row 16-byte aligned (got %lld)", (long long)ldu);
  UR_REQUIRE(K >= 1 && K <= UR_CATALOG_DEEP_TOPK_MAX, "ur_catalog_funnel_select: K must be 1 .. %d (got %d)", UR_CATALOG_DEEP_TOPK_MAX, K);
  UR_REQUIRE(a->catalog_bf16 == 1, "ur_catalog_funnel_select: catalog_bf16 must be 1, the coarse scorer reads a bf16 catalogue only (got %d)",
             a->catalog_bf16);
  UR_REQUIRE(a->segments >= 0 && a->segments <= UR_CATALOG_DEEP_SEGMENTS_MAX, "ur_catalog_funnel_select: segments must be 0 .. %d (got %d)",
             UR_CATALOG_DEEP_SEGMENTS_MAX, a->segments);
  const coarse_deep_plan p = funnel_select_layout(B, N, dim, K, a->chunk_rows, a->segments);
  if (!a->workspace) {
    a->workspace_bytes = p.need;
    return 0;
  }
  if (const int rc = catalog_check_buffers(c, p.need, false)) return rc;
  if (B == 0) return 0;
  UR_REQUIRE(a->topk_index && a->topk_score, "ur_catalog_funnel_select: topk_index / topk_score are null");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)a->workspace;
  bf16_t* ubf = (bf16_t*)(ws + p.user);
  float* inv_u = (float*)(ws + p.inv_u);
  float* ref = (float*)(ws + p.ref);
  float* chunk = (float*)(ws + p.chunk);
  float* list_score = (float*)(ws + p.list_score);
  int* list_index = (int*)(ws + p.list_index);
  int* count = (int*)(ws + p.count);
  const bf16_t* cat = (const bf16_t*)a->catalog;
  const long* gt = (const long*)a->gt_index;
  const int G = deep_segments(a->segments, B, p.rows);             // <= p.gw, what the workspace holds
  const int64_t tiles = p.rows / SEL_TILE;
  const long seg_len = (long)((tiles + G - 1) / G) * SEL_TILE;
  // the sequence of ur_catalog_coarse_deep_select: cast, norms, the diagonal launch, the chunks, the merge
  const long pieces = (long)B * (dim >> 3);
  hipLaunchKernelGGL(cast_prefix_kernel, dim3((unsigned)(pieces < 256L * 2048 ? (pieces + 255) / 256 : 2048)), dim3(256), 0, st, a->user, (long)ldu,
                     ubf, (int)B, (int)dim);
  hipLaunchKernelGGL(row_inv_norm_kernel<bf16_t>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, (const bf16_t*)ubf, inv_u, (long)B, (int)dim);
  if (!a->cat_norm_ready && N > 0) launch_prefix_norm(cat, (long)cld, a->cat_inv_norm, (long)N, dim, st);
  UR_CHECK_LAUNCH(c.who);
  int rc = 0;
  if (gt && N > 0) {
    rc = launch_catalog_scores_bf16_prefix(ubf, inv_u, cat, (long)cld, a->cat_inv_norm, nullptr, 0, gt, ref, B, N, dim, st);
    if (rc != 0) return rc;
  }
  rc = catalog_for_each_chunk(N, p.rows, [&](int64_t c0, int64_t len, int first) {
    if (len > 0) {
      const int rc = launch_catalog_scores_bf16_prefix(ubf, inv_u, cat + c0 * cld, (long)cld, a->cat_inv_norm + c0, chunk, (long)len, nullptr,
                                                       nullptr, B, len, dim, st);
      if (rc != 0) return rc;
    }
    hipLaunchKernelGGL(catalog_deep_sweep_kernel, dim3((unsigned)((int64_t)B * G)), dim3(256), 0, st, (const float*)chunk, (long)len, (int)c0,
                       (int)len, (int)K, G, seg_len, list_score, list_index, count, gt, (const float*)ref, (const long*)a->exclude, (int)E, first);
    UR_CHECK_LAUNCH(c.who);
    return 0;
  });
  if (rc != 0) return rc;
  hipLaunchKernelGGL(catalog_deep_merge_kernel, dim3((unsigned)B), dim3(256), 0, st, (const float*)list_score, (const int*)list_index,
                     (const int*)count, (int)K, G, a->topk_score, a->topk_index, a->rank);
  UR_CHECK_LAUNCH(c.who);
  return 0;
}

extern "C" int ur_catalog_funnel_rerank(ur_catalog_funnel_rerank_t* a, void* stream) {
  UR_REQUIRE(a, "ur_catalog_funnel_rerank: null argument struct");
  const int32_t B = a->B, dim = a->dim;
  const int64_t N = a->N, cld = a->ld, ldu = a->ldu;
  UR_REQUIRE(B >= 0, "ur_catalog_funnel_rerank: need B >= 0 (got %d)", B);
  UR_REQUIRE(N >= 1 && N <= (int64_t)INT32_MAX, "ur_catalog_funnel_rerank: need 1 <= N <= INT32_MAX (got %lld)", (long long)N);
  UR_REQUIRE(a->catalog_bf16 == 0 || a->catalog_bf16 == 1, "ur_catalog_funnel_rerank: catalog_bf16 must be 0 or 1 (got %d)", a->catalog_bf16);
  const bool bf16 = a->catalog_bf16 == 1;
  const int mult = bf16 ? 8 : 4;
  UR_REQUIRE(dim > 0 && (dim % mult) == 0 && dim <= 2048, "ur_catalog_funnel_rerank: dim must be a positive multiple of %d and <= 2048 (got %d)",
             mult, dim);
  UR_REQUIRE(cld >= dim && (cld % mult) == 0, "ur_catalog_funnel_rerank: ld must be at least dim = %d and a multiple of %d (got %lld)", dim, mult,
             (long long)cld);
  UR_REQUIRE(ldu >= dim && (ldu % 4) == 0, "ur_catalog_funnel_rerank: ldu must be at least dim = %d and a multiple of 4 (got %lld)", dim,
             (long long)ldu);
  UR_REQUIRE(a->K_in >= 1 && a->K_in <= UR_CATALOG_DEEP_TOPK_MAX, "ur_catalog_funnel_rerank: K_in must be 1 .. %d (got %d)",
             UR_CATALOG_DEEP_TOPK_MAX, a->K_in);
  UR_REQUIRE(a->k >= 1 && a->k <= a->K_in, "ur_catalog_funnel_rerank: k must be 1 .. K_in = %d (got %d)", a->K_in, a->k);
  const deep_rerank_plan p = funnel_rerank_layout(B, a->K_in);
  if (!a->workspace) {
    a->workspace_bytes = p.need;
    return 0;
  }
  UR_REQUIRE(UR_ALIGNED16(a->workspace) && a->workspace_bytes >= p.need,
             "ur_catalog_funnel_rerank: workspace must be 16-byte aligned and hold %lld bytes (got %lld)", (long long)p.need,
             (long long)a->workspace_bytes);
  if (B == 0) return 0;
  UR_REQUIRE(a->index && a->topk_index && a->topk_score, "ur_catalog_funnel_rerank: index / topk_index / topk_score are null");
  UR_REQUIRE(a->user && a->catalog && a->cat_inv_norm, "ur_catalog_funnel_rerank: user / catalog / cat_inv_norm: null pointer");
  UR_REQUIRE(UR_ALIGNED16(a->user) && UR_ALIGNED16(a->catalog), "ur_catalog_funnel_rerank: user and catalog must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  float* inv_u = (float*)((char*)a->workspace + p.inv_u);
  float* score = (float*)((char*)a->workspace + p.score);
  const int K_in = a->K_in;
  launch_prefix_norm(a->user, (long)ldu, inv_u, (long)B, dim, st);
  return catalog_dispatch(bf16, a->catalog, [&](auto* cat) {
    using CT = std::remove_const_t<std::remove_pointer_t<decltype(cat)>>;
    if (!a->cat_norm_ready) launch_prefix_norm(cat, (long)cld, a->cat_inv_norm, (long)N, dim, st);
    hipLaunchKernelGGL(catalog_funnel_rerank_score_kernel<CT>, dim3((unsigned)((K_in + 3) / 4), (unsigned)(B < DR_GRID_Y_MAX ? B : DR_GRID_Y_MAX)),
                       dim3(256), 0, st, a->user, (long)ldu, (const float*)inv_u, cat, (long)cld, (const float*)a->cat_inv_norm, a->index, K_in,
                       score, (int)B, (long)N, (int)dim);
    hipLaunchKernelGGL(catalog_deep_rerank_sort_kernel, dim3((unsigned)B), dim3(256), 0, st, (const float*)score, a->index, K_in, (int)a->k,
                       a->topk_index, a->topk_score, (long)N);
    UR_CHECK_LAUNCH("ur_catalog_funnel_rerank");
    return 0;
  });
}
