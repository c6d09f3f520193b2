/* unirec_hip_coarse.h -- the two-stage retrieval family of libunirec_hip.so: an explicitly APPROXIMATE shortlist pass over a bf16
 * catalogue on v_mfma_f32_16x16x32_bf16, and the exact f32 re-rank of a shortlist.  A sixth header with the conventions of
 * include/unirec_hip.h, include/unirec_hip_loss.h, include/unirec_hip_adapter.h, include/unirec_hip_pool.h and include/unirec_hip_mrl.h
 * (plain device pointers and sizes, the caller owns every buffer including the workspace, every call takes the HIP stream and
 * synchronises nothing, 0 ok / < 0 invalid argument / > 0 hipError_t, ur_last_error() for the text, no device allocation, no environment
 * variable).  The ABI version is the one of unirec_hip.h (UR_ABI_VERSION, 25 since this header exists).  ur_catalog_scores and
 * ur_catalog_softmax are untouched: their scorer field still takes 0, 1 or 2 only.
 *
 * Coarse score.  u~_b is u_b rounded to bf16 (nearest even; ur_cast_f32_to_bf16), c_n the bf16 catalogue row,
 *
 *     iu~_b = 1 / max(|u~_b|, 1e-12)        the row-norm kernel of ur_catalog_scores run on u~ (f32 sums of the widened elements)
 *     ic_n  = 1 / max(|c_n|, 1e-12)          the catalogue's inverse norm, as ur_catalog_scores computes it for a bf16 catalogue
 *     A_bn  = sum_d u~_bd * c_nd             f32, accumulated by the bf16 MFMA from C = 0
 *     s~_bn = (A_bn * iu~_b) * ic_n
 *
 *   the cosine of the ROUNDED user with the row: the quantity ur_catalog_scores computes in f32 fmaf chains for the user u~.  It differs
 *   from the exact score of u_b by the rounding of the user (at most 2^-8 of a cosine) and by the order of an f32 sum.
 *   Order of the sum: K steps of 32 elements, s = 0, 1, .. ceil(D / 32) - 1, each one v_mfma_f32_16x16x32_bf16; step s belongs to chain
 *   s mod NC, NC = 2 for D <= 1024 and 4 above; a chain takes its steps in ascending order from C = 0, each step's C input the chain's
 *   previous result, and the chains are added at the end as c0 + c1, or (c0 + c2) + (c1 + c3); inside a step the order is the
 *   instruction's own.  (A single chain of 64 steps at D = 2048 measured 4.4 x the error of the exact scorer's sum, past the bound of
 *   the tests; no chain is longer than 16 steps now.)  The order is fixed by D alone: it does not depend on
 *   B, on the position of the user in the batch, on the position of the row in a tile, a workgroup or a chunk, or on chunk_rows.
 *   A K step that runs past D reads zeros on both sides.  Rows past N and users past B are computed on clamped addresses and never stored.
 *   bf16 subnormal inputs are OUTSIDE the tested contract (the matrix cores may flush them); infinities and NaNs are unspecified, as in
 *   select mode.
 *
 * ur_catalog_coarse_select: the K best items per user under s~ and the rank of gt_index under s~, streamed in chunks.
 *   The users are cast once; per chunk of chunk_rows rows catalog_scores_bf16_kernel writes s~ into a chunk buffer [B, rows] f32 and the
 *   selection kernel of ur_catalog_scores' select mode, unchanged, folds it into the lists: the same total order (score descending, index
 *   ascending), the same exclude rule (sorted rows, negative entries empty, a user's own gt_index is never excluded), K <= UR_CATALOG_TOPK_MAX
 *   and the same tail (index -1, score -inf).  rank_b = 1 + #{kept n != g_b : s~_bn > s~_b,g}; s~_b,g is computed before the first chunk by
 *   the same kernel on row g_b (its diagonal mode), so it has the bits a chunk holds for that pair and g_b never counts against itself.
 *   A workgroup (8 waves) stages UR_COARSE_USER_GROUP = 64 users (32 when D > 1024) in LDS in A-operand order -- 128 KB at D = 1024, one
 *   workgroup per compute unit: the catalogue is re-read once per 64 users rather than once per 32, and it is the catalogue bytes that
 *   bound this kernel -- and walks catalogue rows, 32 per wave and step; a lane's 16-byte global load is the eight consecutive k of the B
 *   operand, so the catalogue goes through no LDS.
 *   Workspace: u~ [B,D] bf16 | iu~ [B] f32 | s~_b,g [B] f32 | chunk [B, rows] f32 (each part rounded up to 16 bytes); nothing of size
 *   B x N.  cat_inv_norm [N] is written unless cat_norm_ready.
 *   Checks (all before any launch, each message names the field): B >= 0, 0 <= N <= INT32_MAX, D a positive multiple of 8 and <= 2048,
 *   K in 1..UR_CATALOG_TOPK_MAX, chunk_rows 0 or a positive multiple of 1024, E == 0 or exclude != NULL, gt_index and rank both or
 *   neither, catalog_bf16 == 1 (an f32 catalogue is refused: this path reads bf16 rows only); then the size query; then the workspace
 *   (16-byte aligned, at least what the query reports); then B == 0 returns 0; then topk_index / topk_score non-null, user / catalog /
 *   cat_inv_norm non-null (catalog and cat_inv_norm may be NULL when N == 0) and user / catalog 16-byte aligned.
 *
 * ur_catalog_rerank: the EXACT scores of a shortlist.  index [B, K_in] int32 (an entry outside [0, N), -1 for instance, is an empty
 *   slot).  One wave per (user, slot) runs the chain of ur_catalog_scores on that pair -- lane l the 4-element pieces at d = 4 l + 256 j
 *   (w, z, y, x inside a piece, fmaf from 0), the xor-shuffle sum over the 64 lanes (32, 16, .. 1), then (v * iu_b) * ic_n with iu of the
 *   UNROUNDED f32 user -- so the score has the bits ur_catalog_scores writes for the pair, for an f32 catalogue and for a bf16 one
 *   (widened exactly).  One workgroup per user then sorts its at most 128 pairs in LDS under the total order above and writes the first
 *   k; empty slots stay at the tail as (-1, -inf).  A duplicated index is scored and listed twice.  No floating-point atomics; two calls
 *   give the same bits.
 *   Workspace: iu [B] f32.  cat_inv_norm [N] is written unless cat_norm_ready.
 *   Checks (all before any launch): B >= 0, 1 <= N <= INT32_MAX, D a positive multiple of 4 (8 for a bf16 catalogue) and <= 2048,
 *   K_in in 1..UR_CATALOG_TOPK_MAX, k in 1..K_in, catalog_bf16 in {0, 1}; then the size query; the workspace; B == 0 returns 0; then index /
 *   topk_index / topk_score / user / catalog / cat_inv_norm non-null and user / catalog 16-byte aligned.
 *
 * Size query (both calls): with workspace == NULL the call checks the sizes, writes the bytes it needs into workspace_bytes and returns
 *   0 without launching anything. */
#ifndef UNIREC_HIP_COARSE_H
#define UNIREC_HIP_COARSE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UR_COARSE_USER_GROUP 64

typedef struct {
  const float* user;         /* [B,D] f32 */
  const void* catalog;       /* [N,D] bf16 */
  int32_t catalog_bf16;      /* must be 1 */
  float* cat_inv_norm;       /* [N]: in when cat_norm_ready, else out */
  int32_t cat_norm_ready;
  int32_t B;
  int64_t N;
  int32_t D;                 /* a positive multiple of 8, <= 2048 */
  int32_t K;                 /* list length, 1..UR_CATALOG_TOPK_MAX */
  int32_t* topk_index;       /* [B,K] out */
  float* topk_score;         /* [B,K] out: the coarse scores s~ */
  const int64_t* gt_index;   /* [B] or NULL */
  int32_t* rank;             /* [B] out, with gt_index */
  const int64_t* exclude;    /* [B,E] or NULL; every row sorted ascending, negative entries = empty slots */
  int32_t E;
  int64_t chunk_rows;        /* catalogue rows scored per chunk; 0 = the library chooses (a chunk buffer near 64 MB) */
  void* workspace;           /* 16-byte aligned; NULL = size query */
  int64_t workspace_bytes;   /* in: bytes at workspace; out (size query): bytes needed */
} ur_catalog_coarse_t;

typedef struct {
  const float* user;         /* [B,D] f32 */
  const void* catalog;       /* [N,D] f32, or bf16 when catalog_bf16 == 1 */
  int32_t catalog_bf16;      /* 0 / 1; anything else is rejected */
  float* cat_inv_norm;       /* [N]: in when cat_norm_ready, else out */
  int32_t cat_norm_ready;
  int32_t B;
  int64_t N;
  int32_t D;
  const int32_t* index;      /* [B,K_in]; entries outside [0,N) are empty slots */
  int32_t K_in;              /* 1..UR_CATALOG_TOPK_MAX */
  int32_t k;                 /* 1..K_in */
  int32_t* topk_index;       /* [B,k] out */
  float* topk_score;         /* [B,k] out: the exact scores */
  void* workspace;           /* 16-byte aligned; NULL = size query */
  int64_t workspace_bytes;   /* in: bytes at workspace; out (size query): bytes needed */
} ur_catalog_rerank_t;

int ur_catalog_coarse_select(ur_catalog_coarse_t* args, void* stream);
int ur_catalog_rerank(ur_catalog_rerank_t* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
