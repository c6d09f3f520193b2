// The adapter family (include/unirec_hip_adapter.h): ur_lora_merge folds one projection's LoRA adapter into its frozen weight,
// out = W + scale * B A, from the f32 masters, in one pass over W (HBM-bound: W is read once, each output written once; the rank-r
// slices of A and B are staged once per tile in LDS).  peft's merge_adapter / merge_and_unload arithmetic, fixed to one fmaf chain per
// element in ascending k so the bits do not depend on the launch shape.  gfx950 only.
#include "common.hip.h"
#include "unirec_hip.h"
#include "unirec_hip_adapter.h"

namespace {

constexpr int MG_TO = 64;        // rows of W per tile: 16 row groups x 4 rows
constexpr int MG_TI = 128;       // columns of W per tile: 16 column lanes x 8 columns (two 16-byte f32 chunks, one 16-byte bf16 chunk)
constexpr int MG_THREADS = 256;
constexpr int MG_BPAD = 4;       // floats of padding per staged B row: the four row groups of a wave read 4 * (R + 4) floats apart,
                                 // i.e. 16 banks apart for every R in {8, 16, 32, 64}: their 16-byte reads share no bank

// One tile per loop trip.  Thread (rg, cl) owns rows rg*4 .. rg*4+3 and columns cl*8 .. cl*8+7 of the tile: its W values are in
// flight while the A / B slices are staged.  As holds A[k][tile columns] with the two 16-byte chunks of a lane's eight columns in
// separate halves of the row (chunk q of the row sits at (q & 1) * 64 + (q >> 1) * 4), so the sixteen column lanes read 256 contiguous
// bytes per instruction; the row groups of a wave read the same A addresses (broadcast).
template <int R>
__global__ __launch_bounds__(MG_THREADS) void lora_merge_kernel(const float* W, long ldw, const float* __restrict__ A, const float* __restrict__ B,
                                                                float scale, float* out_f32, long ld_f32, bf16_t* __restrict__ out_bf16,
                                                                long ld_bf16, int out_rows, int in_cols, int tiles_i, long ntiles) {
  __shared__ __attribute__((aligned(16))) float As[R * MG_TI];
  __shared__ __attribute__((aligned(16))) float Bs[MG_TO * (R + MG_BPAD)];
  const int tid = threadIdx.x, cl = tid & 15, rg = tid >> 4;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int row0 = (int)(t / tiles_i) * MG_TO, col0 = (int)(t % tiles_i) * MG_TI;
    const int col = col0 + cl * 8;
    const bool col_ok = col < in_cols;            // in_cols % 8 == 0: a lane's eight columns are inside or outside together
    // ---- W: 4 rows x 2 x 16 bytes per lane, issued first
    float4 w[4][2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = row0 + rg * 4 + j;
      w[j][0] = w[j][1] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (col_ok && o < out_rows) {
        const float4* src = reinterpret_cast<const float4*>(W + (size_t)o * ldw + col);
        w[j][0] = src[0];
        w[j][1] = src[1];
      }
    }
    // ---- stage A [R, tile columns] and B [tile rows, R]; out-of-range parts are zeros (never stored from)
    for (int idx = tid; idx < R * (MG_TI / 4); idx += MG_THREADS) {
      const int k = idx / (MG_TI / 4), q = idx % (MG_TI / 4), c = col0 + q * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < in_cols) v = *reinterpret_cast<const float4*>(A + (size_t)k * in_cols + c);
      *reinterpret_cast<float4*>(&As[k * MG_TI + (q & 1) * (MG_TI / 2) + (q >> 1) * 4]) = v;
    }
    for (int idx = tid; idx < MG_TO * (R / 4); idx += MG_THREADS) {
      const int row = idx / (R / 4), kq = idx % (R / 4), o = row0 + row;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (o < out_rows) v = *reinterpret_cast<const float4*>(B + (size_t)o * R + kq * 4);
      *reinterpret_cast<float4*>(&Bs[row * (R + MG_BPAD) + kq * 4]) = v;
    }
    __syncthreads();
    // ---- acc[o,i] = fmaf(B[o,k], A[k,i], acc) for k ascending: one chain per element
    float acc[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[j][c] = 0.f;
#pragma unroll 2
    for (int kq = 0; kq < R / 4; ++kq) {
      float4 b4[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) b4[j] = *reinterpret_cast<const float4*>(&Bs[(rg * 4 + j) * (R + MG_BPAD) + kq * 4]);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const float4 a0 = *reinterpret_cast<const float4*>(&As[(kq * 4 + kk) * MG_TI + cl * 4]);
        const float4 a1 = *reinterpret_cast<const float4*>(&As[(kq * 4 + kk) * MG_TI + MG_TI / 2 + cl * 4]);
        const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float b = kk == 0 ? b4[j].x : (kk == 1 ? b4[j].y : (kk == 2 ? b4[j].z : b4[j].w));
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[j][c] = __builtin_fmaf(b, a[c], acc[j][c]);
        }
      }
    }
    // ---- w = fmaf(scale, acc, W): 16-byte stores; in place the lane overwrites exactly what it read
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = row0 + rg * 4 + j;
      if (!(col_ok && o < out_rows)) continue;
      const float wv[8] = {w[j][0].x, w[j][0].y, w[j][0].z, w[j][0].w, w[j][1].x, w[j][1].y, w[j][1].z, w[j][1].w};
      float m[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) m[c] = __builtin_fmaf(scale, acc[j][c], wv[c]);
      if (out_f32) {
        float4* dst = reinterpret_cast<float4*>(out_f32 + (size_t)o * ld_f32 + col);
        dst[0] = make_float4(m[0], m[1], m[2], m[3]);
        dst[1] = make_float4(m[4], m[5], m[6], m[7]);
      }
      if (out_bf16) {
        uint4 pk;
        pk.x = pack_bf2(m[0], m[1]); pk.y = pack_bf2(m[2], m[3]); pk.z = pack_bf2(m[4], m[5]); pk.w = pack_bf2(m[6], m[7]);
        *reinterpret_cast<uint4*>(out_bf16 + (size_t)o * ld_bf16 + col) = pk;
      }
    }
    __syncthreads();      // the next tile restages As / Bs
  }
}

// [lo, hi) byte ranges
struct byte_range { uintptr_t lo, hi; };
inline byte_range range_of(const void* p, int64_t rows, int64_t ld, int64_t cols, int64_t elem) {
  const uintptr_t lo = (uintptr_t)p;
  return {lo, lo + (uintptr_t)(((rows - 1) * ld + cols) * elem)};
}
inline bool overlap(byte_range a, byte_range b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace

extern "C" int ur_lora_merge(ur_lora_merge_t* a, void* stream) {
  UR_REQUIRE(a, "ur_lora_merge: null argument struct");
  const int R = a->rank;
  const int64_t O = a->out_rows, I = a->in_cols;
  UR_REQUIRE(R == 8 || R == 16 || R == 32 || R == 64, "ur_lora_merge: rank must be 8, 16, 32 or 64 (got %d)", R);
  UR_REQUIRE(O >= 0 && I >= 0 && (O % 8) == 0 && (I % 8) == 0, "ur_lora_merge: out_rows and in_cols must be non-negative multiples of 8 (got %lld, %lld)",
             (long long)O, (long long)I);
  if (O == 0 || I == 0) return 0;
  UR_REQUIRE(a->W && a->A && a->B, "ur_lora_merge: null pointer (W, A and B are required)");
  UR_REQUIRE(a->out_f32 || a->out_bf16, "ur_lora_merge: both outputs are null (out_f32, out_bf16: give at least one)");
  UR_REQUIRE(UR_ALIGNED16(a->W) && UR_ALIGNED16(a->A) && UR_ALIGNED16(a->B) && UR_ALIGNED16(a->out_f32) && UR_ALIGNED16(a->out_bf16),
             "ur_lora_merge: W, A, B, out_f32 and out_bf16 must be 16-byte aligned");
  UR_REQUIRE(a->ldw >= I && (a->ldw % 4) == 0, "ur_lora_merge: ldw must be >= in_cols and a multiple of 4 (got %lld)", (long long)a->ldw);
  UR_REQUIRE(!a->out_f32 || (a->ld_f32 >= I && (a->ld_f32 % 4) == 0), "ur_lora_merge: ld_f32 must be >= in_cols and a multiple of 4 (got %lld)",
             (long long)a->ld_f32);
  UR_REQUIRE(!a->out_bf16 || (a->ld_bf16 >= I && (a->ld_bf16 % 8) == 0), "ur_lora_merge: ld_bf16 must be >= in_cols and a multiple of 8 (got %lld)",
             (long long)a->ld_bf16);
  const byte_range rw = range_of(a->W, O, a->ldw, I, 4), ra = range_of(a->A, R, I, I, 4), rb = range_of(a->B, O, R, R, 4);
  if (a->out_bf16) {
    const byte_range r16 = range_of(a->out_bf16, O, a->ld_bf16, I, 2);
    UR_REQUIRE(!overlap(r16, rw) && !overlap(r16, ra) && !overlap(r16, rb), "ur_lora_merge: out_bf16 aliases an input (W, A or B)");
    UR_REQUIRE(!a->out_f32 || !overlap(r16, range_of(a->out_f32, O, a->ld_f32, I, 4)), "ur_lora_merge: out_bf16 aliases out_f32");
  }
  if (a->out_f32) {
    const byte_range r32 = range_of(a->out_f32, O, a->ld_f32, I, 4);
    const bool in_place = a->out_f32 == a->W && a->ld_f32 == a->ldw;
    UR_REQUIRE(in_place || !overlap(r32, rw), "ur_lora_merge: out_f32 overlaps W without being W itself (in place needs the same pointer and row stride)");
    UR_REQUIRE(!overlap(r32, ra) && !overlap(r32, rb), "ur_lora_merge: out_f32 aliases A or B");
  }
  const int tiles_i = ur_cdiv(I, MG_TI);
  const long ntiles = (long)ur_cdiv(O, MG_TO) * tiles_i;
  const long cap = (long)ur_device_cu_count() * 8;
  const dim3 grid((unsigned)(ntiles < cap ? ntiles : cap)), block(MG_THREADS);
  hipStream_t st = (hipStream_t)stream;
#define UR_MERGE_LAUNCH(RANK)                                                                                                          \
  hipLaunchKernelGGL(lora_merge_kernel<RANK>, grid, block, 0, st, a->W, (long)a->ldw, a->A, a->B, a->scale, a->out_f32, (long)a->ld_f32, \
                     (bf16_t*)a->out_bf16, (long)a->ld_bf16, (int)O, (int)I, tiles_i, ntiles)
  switch (R) {
    case 8: UR_MERGE_LAUNCH(8); break;
    case 16: UR_MERGE_LAUNCH(16); break;
    case 32: UR_MERGE_LAUNCH(32); break;
    default: UR_MERGE_LAUNCH(64); break;
  }
#undef UR_MERGE_LAUNCH
  UR_CHECK_LAUNCH("ur_lora_merge");
  return 0;
}
