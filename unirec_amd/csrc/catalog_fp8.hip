// FP8 catalogues (include/unirec_fp8.h), gfx950 only: a resident catalogue of one e4m3fn byte per element.
//
//   ur_catalog_fp8_quantize : one wave per row reads an f32 / bf16 row once and writes its codes, its power-of-two scale and the inverse
//                             norm of the code values (the row-norm chain of catalog_select.hip.h on the decoded row).
//   ur_catalog_fp8_select   : an APPROXIMATE shortlist over the codes.  The users are quantised by the same kernel; per chunk of rows
//                             catalog_scores_fp8_kernel widens the codes in registers (exactly) and writes s8_bn = ((q_b . c_n) * iu8_b)
//                             * inv_n on v_mfma_f32_16x16x32_bf16 into the chunk buffer -- v_mfma_f32_16x16x32_fp8_fp8 was built first and
//                             measured: it truncates the products of a K step and misses the header's bound (docs/lab_notes.md section
//                             43) -- and catalog_deep_sweep_kernel / catalog_deep_merge_kernel (catalog_deep.hip.h, unchanged;
//                             this unit compiles its own copy as catalog.hip and catalog_coarse.hip do) fold and join the lists.
//   ur_catalog_fp8_rerank   : the scoring launch of ur_catalog_deep_rerank with the codes widened as they are read, then its sorting
//                             launch, unchanged.
//
// The header holds the definitions in full; the comments here are about the placement.
#include "common.hip.h"
#include "unirec_hip.h"
#include "unirec_fp8.h"
#include "catalog_select.hip.h"
#include "catalog_deep.hip.h"
#include "catalog_fp8_codec.hip.h"

namespace {

// 16 code bytes, the operands of two K steps, widened to bf16: v_cvt_pk_f32_fp8 (OCP e4m3 on gfx950; exact, subnormals included)
// gives two f32 per instruction, and an e4m3 value has three mantissa bits, so the upper half of the f32 IS its bf16: v_perm_b32 packs
// two of them.  Element j of `lo` is byte j, element j of `hi` byte 8 + j.
__device__ __forceinline__ uint32_t widen2(uint32_t w, bool upper) {
  typedef __attribute__((ext_vector_type(2))) float f2_t;
  const f2_t f = upper ? __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true) : __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  return __builtin_amdgcn_perm(__float_as_uint(f[1]), __float_as_uint(f[0]), 0x07060302u);
}
__device__ __forceinline__ void widen16(const uint4 v, bf16x8& lo, bf16x8& hi) {
  typedef __attribute__((ext_vector_type(4))) uint32_t u4_t;
  const u4_t a = {widen2(v.x, false), widen2(v.x, true), widen2(v.y, false), widen2(v.y, true)};
  const u4_t b = {widen2(v.z, false), widen2(v.z, true), widen2(v.w, false), widen2(v.w, true)};
  lo = __builtin_bit_cast(bf16x8, a);
  hi = __builtin_bit_cast(bf16x8, b);
}

// four codes of a row, widened exactly: what load4 is to the f32 and bf16 catalogues
__device__ __forceinline__ float4 load4(const uint8_t* p) {
  const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
  return make_float4(fp8_decode(v & 0xffu), fp8_decode((v >> 8) & 0xffu), fp8_decode((v >> 16) & 0xffu), fp8_decode(v >> 24));
}

// ---- the quantiser ----------------------------------------------------------------------------------------------------------------
// One wave per row, four rows per workgroup.  Lane l holds the 4-element pieces at d = 4 l + 256 i, i = 0 .. 7 (D <= 2048), in
// registers: the element map of row_inv_norm_kernel, so that the norm of the code values is that kernel's chain on the decoded row --
// the squares of e4m3 values are exact in f32, so the bits do not depend on how the compiler fuses the sum.  A wave's load of one i is
// 1024 contiguous bytes of an f32 row; its store of one i is 256 contiguous code bytes.
constexpr int Q_PIECES = 8;
static_assert(Q_PIECES * 256 >= 2048, "a lane holds its pieces of the widest row");
template <typename ST>
__global__ __launch_bounds__(256) void catalog_fp8_quantize_kernel(const ST* __restrict__ src, long ld, uint8_t* __restrict__ codes,
                                                                   float* __restrict__ scale, float* __restrict__ inv, long rows, int D) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                                               // (wave-uniform; no barrier in this kernel)
  const int lane = threadIdx.x & 63;
  const ST* p = src + row * ld;
  float4 v[Q_PIECES];
  uint32_t amax = 0;                                                     // the bits of max |x|: non-negative floats order as integers
#pragma unroll
  for (int i = 0; i < Q_PIECES; ++i) {
    const int d = lane * 4 + 256 * i;
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (d < D) {
      v[i] = load4(p + d);
      amax = max(max(amax, __float_as_uint(v[i].x) & 0x7fffffffu), max(__float_as_uint(v[i].y) & 0x7fffffffu, __float_as_uint(v[i].z) & 0x7fffffffu));
      amax = max(amax, __float_as_uint(v[i].w) & 0x7fffffffu);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = max(amax, (uint32_t)__shfl_xor((int)amax, o, 64));
  const int e = fp8_row_exponent(amax);
  const float up = fp8_pow2(e);
  uint8_t* cp = codes + row * D;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < Q_PIECES; ++i) {
    const int d = lane * 4 + 256 * i;
    if (d < D) {
      const uint32_t cx = fp8_encode(v[i].x * up), cy = fp8_encode(v[i].y * up), cz = fp8_encode(v[i].z * up), cw = fp8_encode(v[i].w * up);
      *reinterpret_cast<uint32_t*>(cp + d) = cx | (cy << 8) | (cz << 16) | (cw << 24);
      const float4 q = make_float4(fp8_decode(cx), fp8_decode(cy), fp8_decode(cz), fp8_decode(cw));
      s += q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    }
  }
  s = wave_sum(s);
  if (lane == 0) {
    inv[row] = 1.0f / fmaxf(sqrtf(s), 1e-12f);
    scale[row] = fp8_pow2(-e);
  }
}

template <typename ST>
void launch_catalog_fp8_quantize(const ST* src, long ld, uint8_t* codes, float* scale, float* inv, int64_t rows, int32_t D, hipStream_t st) {
  hipLaunchKernelGGL(catalog_fp8_quantize_kernel<ST>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, src, ld, codes, scale, inv, (long)rows,
                     (int)D);
}

// ---- the fp8 scorer ---------------------------------------------------------------------------------------------------------------
// catalog_scores_bf16_kernel (catalog_coarse.hip) over code rows.  A workgroup = CF_WAVES waves owns 16 UT users and a range of
// catalogue rows.  A = users (row = user), B = catalogue rows (column = row n), K = the embedding axis: lane l of
// v_mfma_f32_16x16x32_bf16 holds eight bf16 of A[l & 15] and of B[.][l & 15], the K positions 8 (l >> 4) + j, j = 0 .. 7, and
// C[4 (l >> 4) + e][l & 15], e = 0 .. 3.
//   Why not v_mfma_f32_16x16x32_fp8_fp8: the first form of this kernel fed it the bytes as they are.  It does not add the 32 products of
//   a step as f32 numbers -- it aligns them to the largest and drops what lies below about 2^-14 of it (448 * 448 + 12 came back as
//   200704 + 8) -- and missed the header's bound 34-fold at D = 16.  The codes are widened instead: every e4m3 value is a bf16 value, the
//   products are exact in f32 and the bf16 instruction adds them as the coarse scorer's does.  The catalogue still moves one byte per
//   element; the widening is two vector instructions per two elements, beside CF_RT x UT MFMAs per 16 elements.
//   A lane's unit is 16 code bytes, the operands of TWO K steps: pair p covers elements 64 p .. 64 p + 63, lane quarter q = l >> 4 takes
//   the 16 bytes at 64 p + 16 q, the low eight for step 2 p and the high eight for step 2 p + 1 -- on the user side and on the catalogue
//   side alike, so every product pairs the same element of both rows.  D % 16 == 0: a lane's unit is wholly inside or wholly outside.
//   Users: the codes are widened once and staged in LDS in operand order, us[pair p][user tile t][half h][lane][8 bf16]: a wave's
//   ds_read_b128 of one operand is 1024 contiguous bytes.  The staged row is padded with zeros to a multiple of 64.
//   Catalogue: the lane's unit of pair p is the 16 bytes at row n, element 64 p + 16 q, straight from global memory, no LDS: one
//   global_load_dwordx4 feeds two MFMAs per user tile, and a wave's load touches 16 rows x 64 bytes, whole 64-byte pieces.
//   Chains: step s goes to chain s % NC, each chain ascending from C = 0, and the chains are added at the end, c0 + c1 (NC = 2,
//   D <= 1024) or (c0 + c2) + (c1 + c3) (NC = 4, D > 1024): the coarse scorer's order, fixed by D alone.  With NC = 2 a pair feeds
//   chains 0 and 1; with NC = 4 pair p feeds chains 2 (p & 1) and 2 (p & 1) + 1.  The pair that ends short of D brings zeros in the
//   lanes past D (and the staged users are padded), in both of its steps.
// User group: UT = 4 (64 users) for D <= 1024, UT = 2 (32 users) above -- the accumulator budget of the bf16 kernel, UT x CF_RT x NC = 16
// tiles -- at 128 KB of LDS in both cases, as there.
//   Diagonal mode (gt != NULL): "row" n is the virtual row of user n, catalogue row gt[n]; a workgroup visits the virtual rows of its own
//   users only and stores the diagonal, ref[b] = s8_b,gt[b] -- the same instructions in the same order as the chunk pass runs for that
//   pair, hence the same bits.
constexpr int CF_WAVES = 8;
constexpr int CF_RT = 2;
constexpr int CF_ROWS = CF_WAVES * CF_RT * 16;          // catalogue rows per workgroup step
constexpr int CF_ACCS = 16;                             // 16x16 accumulators of a wave: UT x CF_RT tiles x NC chains
constexpr int CF_LDS_MAX = 128 * 1024;
__host__ __device__ constexpr int cf_pairs(int D) { return (D + 63) >> 6; }
__host__ __device__ constexpr size_t cf_lds_bytes(int D, int ut) { return (size_t)cf_pairs(D) * ut * 2 * 64 * 16; }
static_assert(cf_lds_bytes(1024, 4) <= CF_LDS_MAX && cf_lds_bytes(2048, 2) <= CF_LDS_MAX, "the user group must fit the LDS budget");
static_assert(UR_FP8_USER_GROUP == 16 * 4, "the header documents the user group of D <= 1024");

template <int UT>
__global__ __launch_bounds__(CF_WAVES * 64) void catalog_scores_fp8_kernel(const uint8_t* __restrict__ user, const float* __restrict__ inv_u,
                                                                          const uint8_t* __restrict__ cat, const float* __restrict__ inv_c,
                                                                          float* __restrict__ scores, long ld, const long* __restrict__ gt,
                                                                          float* __restrict__ ref, int B, long N, int D, long rows_per_block,
                                                                          int ub) {
  constexpr int NC = CF_ACCS / (UT * CF_RT);                       // chains of the K axis
  constexpr int NP = NC / 2;                                       // pairs per round of the chains
  static_assert(NC == 2 || NC == 4, "the epilogue adds two or four chains");
  extern __shared__ __attribute__((aligned(16))) bf16_t cus[];     // [pairs][UT][2 halves][64 lanes][8]
  const int P2 = cf_pairs(D);
  const int ug = blockIdx.x % ub;
  const long rb = blockIdx.x / ub;
  const int b0 = ug * 16 * UT;
  const int nb = min(16 * UT, B - b0);
  const int P = P2 * 4;                                            // 16-byte units of a padded row
  // 64 threads = 16 users x 4 consecutive units: 64-byte runs of a user's row in, two runs of 1024 contiguous bytes of LDS out
  for (int i = threadIdx.x; i < 16 * UT * P; i += CF_WAVES * 64) {
    const int ul = i & 15, p = (i >> 4) % P, ut = (i >> 4) / P;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (p * 16 < D) v = *reinterpret_cast<const uint4*>(user + (long)min(b0 + ut * 16 + ul, B - 1) * D + p * 16);
    bf16x8 lo, hi;
    widen16(v, lo, hi);
    bf16_t* at = cus + (((((p >> 2) * UT + ut) * 2) * 64 + ul + 16 * (p & 3)) << 3);
    *reinterpret_cast<bf16x8*>(at) = lo;
    *reinterpret_cast<bf16x8*>(at + 512) = hi;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, col = lane & 15, kq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool diag = gt != nullptr;
  const long r0 = diag ? (long)b0 : rb * rows_per_block;
  const long r1 = diag ? (long)(b0 + nb) : min(N, r0 + rows_per_block);
  const int P_full = D >> 6;
  const bf16_t* ap = cus + (lane << 3);
  for (long n0 = r0 + w * 16 * CF_RT; n0 < r1; n0 += CF_ROWS) {
    const uint8_t* bp[CF_RT];                    // a row past the end is read as the last one and never stored
    long crow[CF_RT];
#pragma unroll
    for (int r = 0; r < CF_RT; ++r) {
      const long n = min(n0 + r * 16 + col, r1 - 1);
      crow[r] = diag ? min(max(gt[n], 0L), N - 1) : n;
      bp[r] = cat + crow[r] * D + 16 * kq;
    }
    f32x4 acc[NC][UT][CF_RT];
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int t = 0; t < UT; ++t)
#pragma unroll
        for (int r = 0; r < CF_RT; ++r) acc[j][t][r] = f32x4{0.f, 0.f, 0.f, 0.f};
    // pair p = steps 2 p (chain c0) and 2 p + 1 (chain c1); PART = the pair that ends short (lanes past D bring zeros)
    auto pair = [&](int p, f32x4 (&c0)[UT][CF_RT], f32x4 (&c1)[UT][CF_RT], bool part) {
      const bool in = !part || 64 * p + 16 * kq < D;
      bf16x8 b0[CF_RT], b1[CF_RT];
#pragma unroll
      for (int r = 0; r < CF_RT; ++r) {
        uint4 v = make_uint4(0, 0, 0, 0);                      // (the zero code widens to zero)
        if (in) v = *reinterpret_cast<const uint4*>(bp[r] + 64 * p);
        widen16(v, b0[r], b1[r]);
      }
#pragma unroll
      for (int t = 0; t < UT; ++t) {
        const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(ap + ((p * UT + t) << 10));
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(ap + ((p * UT + t) << 10) + 512);
#pragma unroll
        for (int r = 0; r < CF_RT; ++r) c0[t][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0[r], c0[t][r], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < CF_RT; ++r) c1[t][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1[r], c1[t][r], 0, 0, 0);
      }
    };
    int p0 = 0;
    for (; p0 + NP <= P_full; p0 += NP) {
#pragma unroll
      for (int j = 0; j < NP; ++j) pair(p0 + j, acc[2 * j], acc[2 * j + 1], false);
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {               // the last, incomplete round: step s still goes to chain s % NC (wave-uniform conditions)
      if (p0 + j < P_full) pair(p0 + j, acc[2 * j], acc[2 * j + 1], false);
      else if (p0 + j == P_full && P_full < P2) pair(p0 + j, acc[2 * j], acc[2 * j + 1], true);
    }
#pragma unroll
    for (int t = 0; t < UT; ++t)
#pragma unroll
      for (int r = 0; r < CF_RT; ++r) {
        if (NC == 2) acc[0][t][r] = acc[0][t][r] + acc[1][t][r];
        else acc[0][t][r] = (acc[0][t][r] + acc[2 % NC][t][r]) + (acc[1][t][r] + acc[3 % NC][t][r]);
      }
#pragma unroll
    for (int r = 0; r < CF_RT; ++r) {
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

// one launch of the fp8 scorer, the grid of the bf16 one: rows [0,N) of `cat` / `inv_c` into scores [B][ld], or (gt != NULL) the
// diagonal into ref [B]
int launch_catalog_scores_fp8(const uint8_t* user, const float* inv_u, const uint8_t* cat, const float* inv_c, float* scores, long ld,
                              const long* gt, float* ref, int32_t B, int64_t N, int32_t D, hipStream_t st) {
  const bool wide = D > 1024;
  const int ut = wide ? 2 : 4;
  const int ub = ur_cdiv(B, 16 * ut);
  long blocks_x = 1, rpb = N;
  if (!gt) {
    blocks_x = 512 / ub;                                        // ~2 rounds of one workgroup per CU; a workgroup stages its users once
    if (blocks_x < 1) blocks_x = 1;
    rpb = (N + blocks_x - 1) / blocks_x;
    rpb = (rpb + CF_ROWS - 1) / CF_ROWS * CF_ROWS;
    blocks_x = (N + rpb - 1) / rpb;
  }
  void (*kernel)(const uint8_t*, const float*, const uint8_t*, const float*, float*, long, const long*, float*, int, long, int, long, int) =
      wide ? catalog_scores_fp8_kernel<2> : catalog_scores_fp8_kernel<4>;
  static std::atomic<uint64_t> attr_set[2];   // per device, one per kernel
  UR_ONCE_PER_DEVICE(attr_set[wide]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, CF_LDS_MAX);
    if (e != hipSuccess) UR_FAIL((int)e, "ur_catalog_fp8_select: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks_x * ub)), dim3(CF_WAVES * 64), cf_lds_bytes(D, ut), st, user, inv_u, cat, inv_c, scores, ld,
                     gt, ref, (int)B, (long)N, (int)D, rpb, ub);
  UR_CHECK_LAUNCH("ur_catalog_fp8_select");
  return 0;
}

// the scoring launch of ur_catalog_deep_rerank (catalog_deep_rerank_score_kernel, catalog_coarse.hip) over code rows: one wave per
// (user, slot), the same lane -> element map, fmaf chain, wave_sum and two multiplies, so the score has the bits that kernel gives the
// pair on the f32 catalogue codes.float()
__global__ __launch_bounds__(256) void catalog_fp8_rerank_score_kernel(const float* __restrict__ user, const float* __restrict__ inv_u,
                                                                       const uint8_t* __restrict__ cat, const float* __restrict__ inv_c,
                                                                       const int* __restrict__ index, int K_in, float* __restrict__ score, int B,
                                                                       long N, int D) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (slot >= K_in) return;                                              // (wave-uniform; no barrier in this kernel)
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float* up = user + (long)b * D;
    const float iu = inv_u[b];
    float s = -__builtin_inff();
    const int g = index[(long)b * K_in + slot];                          // (wave-uniform)
    if (g >= 0 && (long)g < N) {
      const uint8_t* cp = cat + (long)g * D;
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

}  // namespace

extern "C" int ur_catalog_fp8_quantize(ur_catalog_fp8_quantize_t* a, void* stream) {
  UR_REQUIRE(a, "ur_catalog_fp8_quantize: null argument struct");
  UR_REQUIRE(a->src_bf16 == 0 || a->src_bf16 == 1, "ur_catalog_fp8_quantize: src_bf16 must be 0 or 1 (got %d)", a->src_bf16);
  UR_REQUIRE(a->N >= 0 && a->N <= (int64_t)INT32_MAX, "ur_catalog_fp8_quantize: need 0 <= N <= INT32_MAX (got %lld)", (long long)a->N);
  UR_REQUIRE(a->D > 0 && (a->D % 16) == 0 && a->D <= 2048, "ur_catalog_fp8_quantize: D must be a positive multiple of 16 and <= 2048 (got %d)",
             a->D);
  UR_REQUIRE(a->ld >= a->D && (a->ld % 4) == 0, "ur_catalog_fp8_quantize: ld must be at least D = %d and a multiple of 4 (got %lld)", a->D,
             (long long)a->ld);
  if (a->N == 0) return 0;
  UR_REQUIRE(a->src && a->codes && a->scale && a->inv, "ur_catalog_fp8_quantize: src / codes / scale / inv: null pointer");
  UR_REQUIRE(UR_ALIGNED16(a->src) && UR_ALIGNED16(a->codes), "ur_catalog_fp8_quantize: src and codes must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (a->src_bf16) launch_catalog_fp8_quantize((const bf16_t*)a->src, (long)a->ld, a->codes, a->scale, a->inv, a->N, a->D, st);
  else launch_catalog_fp8_quantize((const float*)a->src, (long)a->ld, a->codes, a->scale, a->inv, a->N, a->D, st);
  UR_CHECK_LAUNCH("ur_catalog_fp8_quantize");
  return 0;
}

extern "C" int ur_catalog_fp8_select(ur_catalog_fp8_select_t* a, void* stream) {
  UR_REQUIRE(a, "ur_catalog_fp8_select: null argument struct");
  const catalog_call c{"ur_catalog_fp8_select", a->B, a->N, a->D, a->E, a->chunk_rows, 0, 0, a->gt_index, a->rank, a->exclude, a->user, a->codes,
                       a->cat_inv_norm, a->workspace, a->workspace_bytes};
  if (const int rc = catalog_check_sizes(c, 16, 0, false)) return rc;
  const int32_t B = a->B, D = a->D, K = a->K, E = a->E;
  const int64_t N = a->N;
  UR_REQUIRE(K >= 1 && K <= UR_CATALOG_DEEP_TOPK_MAX, "ur_catalog_fp8_select: K must be 1 .. %d (got %d)", UR_CATALOG_DEEP_TOPK_MAX, K);
  UR_REQUIRE(a->segments >= 0 && a->segments <= UR_CATALOG_DEEP_SEGMENTS_MAX, "ur_catalog_fp8_select: segments must be 0 .. %d (got %d)",
             UR_CATALOG_DEEP_SEGMENTS_MAX, a->segments);
  const fp8_select_plan p = fp8_select_layout(B, N, D, K, a->chunk_rows, a->segments);
  if (!a->workspace) {
    a->workspace_bytes = p.need;
    return 0;
  }
  if (const int rc = catalog_check_buffers(c, p.need, false)) return rc;
  if (B == 0) return 0;
  UR_REQUIRE(a->topk_index && a->topk_score, "ur_catalog_fp8_select: topk_index / topk_score are null");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)a->workspace;
  uint8_t* q = (uint8_t*)(ws + p.user);
  float* inv_u = (float*)(ws + p.inv_u);
  float* scale_u = (float*)(ws + p.scale_u);
  float* ref = (float*)(ws + p.ref);
  float* chunk = (float*)(ws + p.chunk);
  float* list_score = (float*)(ws + p.list_score);
  int* list_index = (int*)(ws + p.list_index);
  int* count = (int*)(ws + p.count);
  const uint8_t* cat = a->codes;
  const long* gt = (const long*)a->gt_index;
  const int G = deep_segments(a->segments, B, p.rows);             // <= p.gw, what the workspace holds
  const int64_t tiles = p.rows / SEL_TILE;
  const long seg_len = (long)((tiles + G - 1) / G) * SEL_TILE;
  // the sequence of ur_catalog_coarse_deep_select: the users' codes and norms, the diagonal launch, then the chunks
  launch_catalog_fp8_quantize(a->user, (long)D, q, scale_u, inv_u, (int64_t)B, D, st);
  UR_CHECK_LAUNCH(c.who);
  int rc = 0;
  if (gt && N > 0) {
    rc = launch_catalog_scores_fp8(q, inv_u, cat, a->cat_inv_norm, nullptr, 0, gt, ref, B, N, D, st);
    if (rc != 0) return rc;
  }
  rc = catalog_for_each_chunk(N, p.rows, [&](int64_t c0, int64_t len, int first) {
    if (len > 0) {
      const int rc = launch_catalog_scores_fp8(q, inv_u, cat + c0 * D, a->cat_inv_norm + c0, chunk, (long)len, nullptr, nullptr, B, len, D, st);
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

extern "C" int ur_catalog_fp8_rerank(ur_catalog_fp8_rerank_t* a, void* stream) {
  UR_REQUIRE(a, "ur_catalog_fp8_rerank: null argument struct");
  const int32_t B = a->B, D = a->D;
  const int64_t N = a->N;
  UR_REQUIRE(B >= 0, "ur_catalog_fp8_rerank: need B >= 0 (got %d)", B);
  UR_REQUIRE(N >= 1 && N <= (int64_t)INT32_MAX, "ur_catalog_fp8_rerank: need 1 <= N <= INT32_MAX (got %lld)", (long long)N);
  UR_REQUIRE(D > 0 && (D % 16) == 0 && D <= 2048, "ur_catalog_fp8_rerank: D must be a positive multiple of 16 and <= 2048 (got %d)", D);
  UR_REQUIRE(a->K_in >= 1 && a->K_in <= UR_CATALOG_DEEP_TOPK_MAX, "ur_catalog_fp8_rerank: K_in must be 1 .. %d (got %d)", UR_CATALOG_DEEP_TOPK_MAX,
             a->K_in);
  UR_REQUIRE(a->k >= 1 && a->k <= a->K_in, "ur_catalog_fp8_rerank: k must be 1 .. K_in = %d (got %d)", a->K_in, a->k);
  const deep_rerank_plan p = fp8_rerank_layout(B, a->K_in);
  if (!a->workspace) {
    a->workspace_bytes = p.need;
    return 0;
  }
  UR_REQUIRE(UR_ALIGNED16(a->workspace) && a->workspace_bytes >= p.need,
             "ur_catalog_fp8_rerank: workspace must be 16-byte aligned and hold %lld bytes (got %lld)", (long long)p.need,
             (long long)a->workspace_bytes);
  if (B == 0) return 0;
  UR_REQUIRE(a->index && a->topk_index && a->topk_score, "ur_catalog_fp8_rerank: index / topk_index / topk_score are null");
  UR_REQUIRE(a->user && a->codes && a->cat_inv_norm, "ur_catalog_fp8_rerank: user / codes / cat_inv_norm: null pointer");
  UR_REQUIRE(UR_ALIGNED16(a->user) && UR_ALIGNED16(a->codes), "ur_catalog_fp8_rerank: user and codes must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  float* inv_u = (float*)((char*)a->workspace + p.inv_u);
  float* score = (float*)((char*)a->workspace + p.score);
  const int K_in = a->K_in;
  hipLaunchKernelGGL(row_inv_norm_kernel<float>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, a->user, inv_u, (long)B, (int)D);
  hipLaunchKernelGGL(catalog_fp8_rerank_score_kernel, dim3((unsigned)((K_in + 3) / 4), (unsigned)(B < DR_GRID_Y_MAX ? B : DR_GRID_Y_MAX)), dim3(256),
                     0, st, a->user, (const float*)inv_u, a->codes, a->cat_inv_norm, a->index, K_in, score, (int)B, (long)N, (int)D);
  hipLaunchKernelGGL(catalog_deep_rerank_sort_kernel, dim3((unsigned)B), dim3(256), 0, st, (const float*)score, a->index, K_in, (int)a->k,
                     a->topk_index, a->topk_score, (long)N);
  UR_CHECK_LAUNCH("ur_catalog_fp8_rerank");
  return 0;
}
