/* unirec_fp8.h -- FP8 catalogues of libunirec_hip.so: a resident [N, D] catalogue at ONE byte per element (OCP e4m3fn codes with a
 * power-of-two scale per row), an APPROXIMATE shortlist pass over it (codes widened in registers, v_mfma_f32_16x16x32_bf16), and the exact re-rank of a shortlist
 * against the quantised rows.  An eleventh header with the conventions of include/unirec_hip.h and the family headers beside it (plain
 * device pointers and sizes, the caller owns every buffer including the workspace, every call takes the HIP stream and synchronises
 * nothing, 0 ok / < 0 invalid argument / > 0 hipError_t, ur_last_error() for the text, every check before any launch and every refusal
 * naming the field, no device allocation, no environment variable, two calls give the same bits, no floating-point atomics).  The ABI
 * version is the one of unirec_hip.h (UR_ABI_VERSION, 30 since this header exists).  Every older entry point is untouched: its kernels,
 * launches, limits and bits stay.
 *
 * The format.  codes [N, D]: one byte per element, the bit pattern of the OCP 8-bit float e4m3fn (1 sign, 4 exponent bits of bias 7,
 *   3 mantissa bits, subnormals, no infinities, 0x7f / 0xff the only NaNs, largest finite value 448) -- torch.float8_e4m3fn, NOT the
 *   e4m3fnuz form of gfx942.  Rows are contiguous; D is a positive multiple of 16 and at most 2048.  Two f32 planes [N] go with it:
 *   scale, a power of two per row, and inv, the inverse norm of the row's code values.
 *   Row scale.  a = max_d |x_nd| (a bf16 source is widened exactly).  a == 0 or a not finite: e = 0.  Otherwise a = m 2^x with m in
 *   [0.5, 1) (frexp) and e = 9 - x if m <= 0.875, else 8 - x: the largest e with a 2^e <= 448.  e is clamped to [-64, 64];
 *   scale[n] = 2^-e.  Decoding, codes.float() * scale[:, None], is exact.
 *   Codes.  code_nd = the e4m3fn nearest to the f32 product x_nd 2^e, ties to the even code, into the subnormals (multiples of 2^-9),
 *   the sign of a zero kept: what torch.tensor(x * 2^e, dtype=float32).to(torch.float8_e4m3fn) gives on the CPU.  |x 2^e| <= 448, so
 *   nothing saturates.  The rule defines the codes; the library rounds in integer arithmetic and uses no convert instruction.
 *   Non-finite inputs are outside the contract.
 *   Norm.  inv[n] = 1 / max(|codes[n].float()|, 1e-12) over the UNSCALED code values, with the bits the row-norm kernel of
 *   ur_catalog_scores writes for the f32 row codes[n].float(): lane l of 64 adds x^2 + y^2 + z^2 + w^2 of its 4-element pieces at
 *   d = 4 l + 256 i in ascending i, the xor-shuffle sum over the lanes (32, 16, .. 1), sqrtf, fmaxf, one division (the chain
 *   include/unirec_hip_funnel.h spells out).  A cosine does not see a positive row scale: no scorer below reads `scale`.
 *
 * ur_catalog_fp8_quantize: src [N, ld] f32, or bf16 when src_bf16 == 1, row stride ld >= D elements -> codes, scale, inv as above.
 *   One wave per row reads the row once; no workspace.  ur_catalog_fp8_select runs the same kernel on the users.
 *   Checks: src_bf16 in {0, 1}, 0 <= N <= INT32_MAX, D a positive multiple of 16 and <= 2048, ld >= D and a multiple of 4; then N == 0
 *   returns 0; then src / codes / scale / inv non-null, src and codes 16-byte aligned.
 *
 * ur_catalog_fp8_select: the long coarse select of include/unirec_hip_coarse_deep.h over codes -- the K best items per user under the
 *   score s8 and the rank of gt_index under s8, streamed in chunks, K up to UR_CATALOG_DEEP_TOPK_MAX = 1024.
 *   Score.  The users are quantised by the rule above into the workspace: codes q_b and iu8_b, the inverse norm of q_b's values.
 *   s8_bn = ((q_b . c_n) * iu8_b) * inv_n with inv = cat_inv_norm, always an input here (the plane ur_catalog_fp8_quantize wrote).  The
 *   codes of both sides are widened to bf16 in registers -- exact: an e4m3 value has three mantissa bits -- and the dot product runs
 *   on v_mfma_f32_16x16x32_bf16 in K steps of 32 elements.  A lane loads 16 code bytes of a row, the operands of two steps: steps 2 p
 *   and 2 p + 1 together cover elements 64 p .. 64 p + 63, step 2 p + h holding the eight elements at 64 p + 16 q + 8 h of each
 *   quarter q = 0 .. 3, for users and rows alike.  Step s goes to chain s mod NC, NC = 2 for D <= 1024 and 4 above, each chain
 *   ascending from 0; the chains are added as c0 + c1 or (c0 + c2) + (c1 + c3): the order is fixed by D alone.  A step that ends short
 *   of D brings zeros.
 *   Accuracy.  The products of two e4m3 values are exact in f32; what rounds is the order of at most D f32 additions and the two
 *   multiplies, so |s8 - exact| <= ((D + 2) 2^-23 sum_d |q_bd c_nd|) iu8_b inv_n + 2^-22 |s8| (tests/test_gpu_catalog_fp8.py holds every
 *   score to it; worst err / bound measured 0.04).
 *   Why not v_mfma_f32_16x16x32_fp8_fp8, which takes the bytes as they are: it was built first and measured (docs/lab_notes.md, "FP8
 *   catalogues").  That instruction does not add the 32 products of a step as f32 numbers: it aligns them to the largest product of the
 *   step and drops what lies below about 2^-14 of it (448 * 448 next to x y: 12 arrives as 8, anything below 8 as 0).  It missed the
 *   bound above 34-fold at D = 16 and 5.5-fold at D = 48, and 4 x the error of the bf16 scorer on the same operands at every width.
 *   The catalogue is read at one byte per element either way.
 *   s8_b,g comes from the scorer's diagonal mode before the first chunk: the same instructions in the same order as the chunk pass
 *   runs for that pair.  The score of a pair does not depend on B, N, chunk_rows, segments or the pair's position.
 *   Selection.  The sweep and merge kernels of ur_catalog_deep_select, unchanged: the strict total order score descending, index
 *   ascending; exclude rows sorted ascending, negative entries empty, a user's own gt_index is never excluded; with fewer than K
 *   candidates the tail is (-1, -inf).  rank_b = 1 + #{kept n != g_b : s8_bn > s8_b,g}.  The outputs are a pure function of the scores.
 *   Workspace: q [B,D] bytes | iu8 [B] f32 | user scales [B] f32 | s8_b,g [B] f32 | chunk [B, rows] f32 | list scores [B, Gw, K] f32 |
 *   list indices [B, Gw, K] int32 | counts [B, Gw] int32, each part rounded up to 16 bytes; Gw = segments if > 0, else
 *   min(max(1024 / B, 1), 8), and rows = chunk_rows, or a chunk buffer near 64 MB, never more than N rounded up to 1024 (both as in
 *   unirec_hip_deep.h); nothing of size B x N.
 *   Checks (those of ur_catalog_coarse_deep_select): B >= 0, 0 <= N <= INT32_MAX, D a positive multiple of 16 and <= 2048, chunk_rows 0
 *   or a positive multiple of 1024, E == 0 or exclude != NULL, gt_index and rank both or neither, K in 1..UR_CATALOG_DEEP_TOPK_MAX,
 *   segments in 0..UR_CATALOG_DEEP_SEGMENTS_MAX; then the size query; then the workspace (16-byte aligned, at least what the query
 *   reports); then B == 0 returns 0; then topk_index / topk_score non-null, user / codes / cat_inv_norm non-null (codes and cat_inv_norm
 *   may be NULL when N == 0) and user / codes 16-byte aligned.
 *
 * ur_catalog_fp8_rerank: ur_catalog_deep_rerank over codes -- the EXACT scores of a shortlist of up to 1024 items against the quantised
 *   rows.  One wave per (user, slot) widens the codes exactly and runs the exact scorer's chain against the UNROUNDED f32 user (lane l
 *   the 4-element pieces at d = 4 l + 256 j, w, z, y, x inside a piece, fmaf from 0, the xor-shuffle sum, then (v * iu_b) * inv_n); the
 *   sorting launch of ur_catalog_deep_rerank then runs unchanged.  Index and score bits are those of ur_catalog_deep_rerank on the f32
 *   catalogue codes.float().  cat_inv_norm is an input (the plane ur_catalog_fp8_quantize wrote).
 *   Workspace: iu [B] f32 | scores [B, K_in] f32, each part rounded up to 16 bytes.
 *   Checks: B >= 0, 1 <= N <= INT32_MAX, D a positive multiple of 16 and <= 2048, K_in in 1..UR_CATALOG_DEEP_TOPK_MAX, k in 1..K_in;
 *   then the size query; the workspace; B == 0 returns 0; then index / topk_index / topk_score / user / codes / cat_inv_norm non-null
 *   and user / codes 16-byte aligned.
 *
 * Size query (select and rerank): with workspace == NULL the call checks the sizes, writes the bytes it needs into workspace_bytes and
 *   returns 0 without launching anything; a refused query leaves workspace_bytes alone. */
#ifndef UNIREC_FP8_H
#define UNIREC_FP8_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UR_FP8_USER_GROUP 64    /* users a workgroup of the fp8 scorer stages in LDS for D <= 1024 (half of it above) */

typedef struct {
  const void* src;           /* [N,ld] f32, or bf16 when src_bf16 == 1 */
  int32_t src_bf16;          /* 0 / 1; anything else is rejected */
  int64_t N;
  int32_t D;                 /* a positive multiple of 16, <= 2048 */
  int64_t ld;                /* elements between rows of src: >= D, a multiple of 4 */
  uint8_t* codes;            /* [N,D] out: e4m3fn bit patterns */
  float* scale;              /* [N] out: 2^-e */
  float* inv;                /* [N] out: the inverse norm of the row's code values */
} ur_catalog_fp8_quantize_t;

typedef struct {
  const float* user;         /* [B,D] f32 */
  const uint8_t* codes;      /* [N,D] e4m3fn */
  const float* cat_inv_norm; /* [N] in: ur_catalog_fp8_quantize's inv */
  int32_t B;
  int64_t N;
  int32_t D;                 /* a positive multiple of 16, <= 2048 */
  int32_t K;                 /* list length, 1..UR_CATALOG_DEEP_TOPK_MAX (1024) */
  int32_t* topk_index;       /* [B,K] out */
  float* topk_score;         /* [B,K] out: the scores s8 */
  const int64_t* gt_index;   /* [B] or NULL */
  int32_t* rank;             /* [B] out, with gt_index */
  const int64_t* exclude;    /* [B,E] or NULL; every row sorted ascending, negative entries = empty slots */
  int32_t E;
  int64_t chunk_rows;        /* catalogue rows scored per chunk; 0 = the library chooses (a chunk buffer near 64 MB) */
  int32_t segments;          /* workgroups that share a user's chunk row; 0 = the library chooses.  The outputs do not depend on it */
  void* workspace;           /* 16-byte aligned; NULL = size query */
  int64_t workspace_bytes;   /* in: bytes at workspace; out (size query): bytes needed */
} ur_catalog_fp8_select_t;

typedef struct {
  const float* user;         /* [B,D] f32 */
  const uint8_t* codes;      /* [N,D] e4m3fn */
  const float* cat_inv_norm; /* [N] in: ur_catalog_fp8_quantize's inv */
  int32_t B;
  int64_t N;
  int32_t D;
  const int32_t* index;      /* [B,K_in]; entries outside [0,N) are empty slots */
  int32_t K_in;              /* 1..UR_CATALOG_DEEP_TOPK_MAX (1024) */
  int32_t k;                 /* 1..K_in */
  int32_t* topk_index;       /* [B,k] out */
  float* topk_score;         /* [B,k] out: the exact scores against the quantised rows */
  void* workspace;           /* 16-byte aligned; NULL = size query */
  int64_t workspace_bytes;   /* in: bytes at workspace; out (size query): bytes needed */
} ur_catalog_fp8_rerank_t;

int ur_catalog_fp8_quantize(ur_catalog_fp8_quantize_t* args, void* stream);
int ur_catalog_fp8_select(ur_catalog_fp8_select_t* args, void* stream);
int ur_catalog_fp8_rerank(ur_catalog_fp8_rerank_t* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
