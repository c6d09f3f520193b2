/* unirec_hip_coarse_deep.h -- long two-stage retrieval of libunirec_hip.so: the APPROXIMATE bf16-MFMA shortlist pass of
 * include/unirec_hip_coarse.h feeding the long-list selection of include/unirec_hip_deep.h, and the exact f32 re-rank of a shortlist of
 * up to UR_CATALOG_DEEP_TOPK_MAX = 1024 items.  An eighth header with the conventions of include/unirec_hip.h, include/unirec_hip_loss.h,
 * include/unirec_hip_adapter.h, include/unirec_hip_pool.h, include/unirec_hip_mrl.h, include/unirec_hip_coarse.h and
 * include/unirec_hip_deep.h (plain device pointers and sizes, the caller owns every buffer including the workspace, every call takes the
 * HIP stream and synchronises nothing, 0 ok / < 0 invalid argument / > 0 hipError_t, ur_last_error() for the text, no device allocation,
 * no environment variable).  The ABI version is the one of unirec_hip.h (UR_ABI_VERSION, 27 since this header exists).
 * ur_catalog_coarse_select, ur_catalog_rerank (K, K_in <= UR_CATALOG_TOPK_MAX = 128) and ur_catalog_deep_select are untouched: their
 * limits, kernels, launches and bits stay.
 *
 * ur_catalog_coarse_deep_select: the K best items per user under the coarse score s~ and the rank of gt_index under s~, streamed in
 *   chunks, K up to 1024.
 *   Score.  s~_bn of unirec_hip_coarse.h, bit for bit: the users are cast once by ur_cast_f32_to_bf16 and normed by the row-norm kernel
 *   on u~, the chunks are scored by the launch ur_catalog_coarse_select uses (catalog_scores_bf16_kernel), and s~_b,g comes from that
 *   launch's diagonal mode before the first chunk -- the same sequence ur_catalog_coarse_select runs.
 *   Selection.  The sweep and merge kernels of ur_catalog_deep_select, unchanged: the strict total order score descending, index
 *   ascending; exclude rows sorted ascending, negative entries empty, a user's own gt_index is never excluded; with fewer than K
 *   candidates the tail is (-1, -inf).  rank_b = 1 + #{kept n != g_b : s~_bn > s~_b,g}.
 *   Purity.  The order is strict and the rank an integer count, so the outputs are a pure function of the coarse scores: they do not
 *   depend on chunk_rows, on segments, on B or on the position of a user in the batch.  For K <= 128 they equal
 *   ur_catalog_coarse_select's in every bit; for larger K the first 128 entries and the rank equal those of K = 128.  Two calls give
 *   the same bits; no floating-point atomics.
 *   Workspace: u~ [B,D] bf16 | iu~ [B] f32 | s~_b,g [B] f32 | chunk [B, rows] f32 | list scores [B, Gw, K] f32 | list indices
 *   [B, Gw, K] int32 | counts [B, Gw] int32, each part rounded up to 16 bytes; Gw = segments if > 0, else min(max(1024 / B, 1), 8), and
 *   rows = chunk_rows, or a chunk buffer near 64 MB, never more than N rounded up to 1024 (both as in unirec_hip_deep.h); nothing of
 *   size B x N.  cat_inv_norm [N] is written unless cat_norm_ready.
 *   Checks (all before any launch, each message names the field): B >= 0, 0 <= N <= INT32_MAX, D a positive multiple of 8 and <= 2048,
 *   chunk_rows 0 or a positive multiple of 1024, E == 0 or exclude != NULL, gt_index and rank both or neither, K in
 *   1..UR_CATALOG_DEEP_TOPK_MAX, catalog_bf16 == 1 (an f32 catalogue is refused: this path reads bf16 rows only), segments in
 *   0..UR_CATALOG_DEEP_SEGMENTS_MAX; then the size query; then the workspace (16-byte aligned, at least what the query reports); then
 *   B == 0 returns 0; then topk_index / topk_score non-null, user / catalog / cat_inv_norm non-null (catalog and cat_inv_norm may be NULL
 *   when N == 0) and user / catalog 16-byte aligned.
 *
 * ur_catalog_deep_rerank: the EXACT scores of a shortlist of up to 1024 items.  index [B, K_in] int32 (an entry outside [0, N), -1 for
 *   instance, is an empty slot).
 *   Score of a pair.  One wave per (user, slot) runs the chain of ur_catalog_scores / ur_catalog_rerank -- lane l the 4-element pieces
 *   at d = 4 l + 256 j (w, z, y, x inside a piece, fmaf from 0), the xor-shuffle sum over the 64 lanes (32, 16, .. 1), then
 *   (v * iu_b) * ic_n with iu of the UNROUNDED f32 user -- so the score has the bits ur_catalog_scores writes for the pair, for an f32
 *   catalogue and for a bf16 one (widened exactly).
 *   Order.  The total order above; empty slots stay at the tail as (-1, -inf); a duplicated index is scored and listed twice.  No
 *   floating-point atomics; two calls give the same bits; for K_in <= 128 the outputs equal ur_catalog_rerank's in every bit.
 *   Launches.  A scoring launch, one wave per (user, slot) -- workgroups of four waves, ceil(K_in / 4) per user, so that 64 users fill
 *   the device and no wave waits on more than one row -- writes [B, K_in] f32 into the workspace; then one workgroup per user sorts its
 *   pairs, padded to the next power of two with empty slots, in 8 KB of LDS and writes the first k.  The result does not depend on the
 *   grid of either launch.
 *   Workspace: iu [B] f32 | scores [B, K_in] f32, each part rounded up to 16 bytes.  cat_inv_norm [N] is written unless cat_norm_ready.
 *   Checks (all before any launch): B >= 0, 1 <= N <= INT32_MAX, catalog_bf16 in {0, 1}, D a positive multiple of 4 (8 for a bf16
 *   catalogue) and <= 2048, K_in in 1..UR_CATALOG_DEEP_TOPK_MAX, k in 1..K_in; then the size query; the workspace; B == 0 returns 0; then
 *   index / topk_index / topk_score / user / catalog / cat_inv_norm non-null and user / catalog 16-byte aligned.
 *
 * Size query (both calls): with workspace == NULL the call checks the sizes, writes the bytes it needs into workspace_bytes and returns
 *   0 without launching anything; a refused query leaves workspace_bytes alone. */
#ifndef UNIREC_HIP_COARSE_DEEP_H
#define UNIREC_HIP_COARSE_DEEP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  const float* user;         /* [B,D] f32 */
  const void* catalog;       /* [N,D] bf16 */
  int32_t catalog_bf16;      /* must be 1 */
  float* cat_inv_norm;       /* [N]: in when cat_norm_ready, else out */
  int32_t cat_norm_ready;
  int32_t B;
  int64_t N;
  int32_t D;                 /* a positive multiple of 8, <= 2048 */
  int32_t K;                 /* list length, 1..UR_CATALOG_DEEP_TOPK_MAX (1024) */
  int32_t* topk_index;       /* [B,K] out */
  float* topk_score;         /* [B,K] out: the coarse scores s~ */
  const int64_t* gt_index;   /* [B] or NULL */
  int32_t* rank;             /* [B] out, with gt_index */
  const int64_t* exclude;    /* [B,E] or NULL; every row sorted ascending, negative entries = empty slots */
  int32_t E;
  int64_t chunk_rows;        /* catalogue rows scored per chunk; 0 = the library chooses (a chunk buffer near 64 MB) */
  int32_t segments;          /* workgroups that share a user's chunk row; 0 = the library chooses.  The outputs do not depend on it */
  void* workspace;           /* 16-byte aligned; NULL = size query */
  int64_t workspace_bytes;   /* in: bytes at workspace; out (size query): bytes needed */
} ur_catalog_coarse_deep_t;

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
  int32_t K_in;              /* 1..UR_CATALOG_DEEP_TOPK_MAX (1024) */
  int32_t k;                 /* 1..K_in */
  int32_t* topk_index;       /* [B,k] out */
  float* topk_score;         /* [B,k] out: the exact scores */
  void* workspace;           /* 16-byte aligned; NULL = size query */
  int64_t workspace_bytes;   /* in: bytes at workspace; out (size query): bytes needed */
} ur_catalog_deep_rerank_t;

int ur_catalog_coarse_deep_select(ur_catalog_coarse_deep_t* args, void* stream);
int ur_catalog_deep_rerank(ur_catalog_deep_rerank_t* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
