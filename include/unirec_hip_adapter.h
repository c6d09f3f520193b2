/* unirec_hip_adapter.h -- the adapter family of libunirec_hip.so: what is done with LoRA adapters AFTER training.  A third header with
 * the conventions of include/unirec_hip.h and include/unirec_hip_loss.h (plain device pointers and sizes, the caller owns every buffer,
 * every call takes the HIP stream and synchronises nothing, 0 ok / < 0 invalid argument / > 0 hipError_t, ur_last_error() for the
 * text).  The ABI version is the one of unirec_hip.h (UR_ABI_VERSION, 21 since this header exists).
 *
 * ur_lora_merge: folds one projection's adapter into its frozen weight, out = W + scale * B A, in ONE pass over W.  All inputs are
 *   the f32 masters (W [out,in] with row stride ldw; A [r,in] and B [out,r] dense); the arithmetic is fixed, so the result does not
 *   depend on the launch shape:
 *
 *     acc = 0 ;  for k = 0 .. r-1 (ascending): acc = fmaf(B[o,k], A[k,i], acc)
 *     w   = fmaf(scale, acc, W[o,i])
 *     out_f32[o,i] = w ;  out_bf16[o,i] = round-to-nearest-even(w)
 *
 *   No atomics, no split over k: two calls give the same bits.  Either output may be NULL, not both.  out_f32 may BE W (the same
 *   pointer and the same row stride: the merge in place -- every element is read and written by the one lane that owns it); any other
 *   overlap of an output with W, A, B or the other output is refused.
 *   Checks (all before any launch): rank in {8, 16, 32, 64}; out_rows >= 0, in_cols >= 0, both multiples of 8; then out_rows == 0 or
 *   in_cols == 0 returns 0 and writes nothing; every pointer given 16-byte aligned, W / A / B non-null; ldw >= in_cols and
 *   ldw % 4 == 0, ld_f32 likewise, ld_bf16 >= in_cols and ld_bf16 % 8 == 0 (every row 16-byte aligned: the kernel moves 16 bytes per
 *   load and store); the overlaps above.  scale is any finite or non-finite float, of either sign. */
#ifndef UNIREC_HIP_ADAPTER_H
#define UNIREC_HIP_ADAPTER_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  const float* W;            /* [out_rows, in_cols] f32, row stride ldw: the frozen master */
  int64_t ldw;
  const float* A;            /* [rank, in_cols] f32, dense: lora_A.weight */
  const float* B;            /* [out_rows, rank] f32, dense: lora_B.weight */
  int32_t rank;              /* 8, 16, 32 or 64 */
  float scale;               /* lora_alpha / r (or lora_alpha / sqrt(r)); negative subtracts */
  float* out_f32;            /* [out_rows, in_cols] f32, row stride ld_f32, or NULL; may be W itself (in place) */
  int64_t ld_f32;
  uint16_t* out_bf16;        /* [out_rows, in_cols] bf16, row stride ld_bf16, or NULL */
  int64_t ld_bf16;
  int32_t out_rows;
  int32_t in_cols;
} ur_lora_merge_t;

int ur_lora_merge(ur_lora_merge_t* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
