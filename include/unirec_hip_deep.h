/* unirec_hip_deep.h -- long exact retrieval lists of libunirec_hip.so: the streaming selection of ur_catalog_scores' select mode with
 * lists of up to UR_CATALOG_DEEP_TOPK_MAX = 1024 items per user.  A seventh header with the conventions of include/unirec_hip.h,
 * include/unirec_hip_loss.h, include/unirec_hip_adapter.h, include/unirec_hip_pool.h, include/unirec_hip_mrl.h and
 * include/unirec_hip_coarse.h (plain device pointers and sizes, the caller owns every buffer including the workspace, every call takes
 * the HIP stream and synchronises nothing, 0 ok / < 0 invalid argument / > 0 hipError_t, ur_last_error() for the text, no device
 * allocation, no environment variable).  The ABI version is the one of unirec_hip.h (UR_ABI_VERSION, 26 since this header exists).
 * ur_catalog_scores, its select mode (K <= UR_CATALOG_TOPK_MAX = 128) and the two-stage family are untouched.
 *
 * ur_catalog_deep_select: the K best items per user and the rank of gt_index, streamed in chunks; nothing of size B x N exists.
 *   Scores.  s_bn is the score of ur_catalog_scores, bit for bit: per chunk of rows the same scoring kernels run through the same launch
 *   functions as in select mode -- the vector scorer (scorer 1), the f32-MFMA scorer (scorer 2), the library's choice between them
 *   (scorer 0: select mode's rule), a bf16 catalogue widened exactly as it is read.  The coarse bf16-MFMA scorer is not reachable here.
 *   Lists.  topk_index[b] holds the first K items, among those not excluded for user b, of the strict total order score descending,
 *   index ascending; topk_score[b] their scores; with fewer than K candidates the tail is (-1, -inf).  exclude follows select mode: rows
 *   sorted ascending, negative entries are empty slots, duplicates allowed, a user's own gt_index is never excluded.
 *   Rank.  rank[b] = 1 + #{non-excluded n : s_bn > s_b,g}, s_b,g from catalog_gt_score_kernel as in select mode.
 *   Uniqueness.  A strict total order has one top-K and the count is an integer, so the outputs are a pure function of the scores: they
 *   do not depend on chunk_rows, on B, on segments or on when the kernel merges.  For K <= 128 they equal select mode's in every bit.
 *   Two calls give the same bits.  No floating-point atomics (an integer LDS counter hands out the survivor slots).
 *
 *   Selection.  A chunk row of a user is cut into G segments of whole 1024-score tiles; one workgroup per (user, segment) keeps its own
 *   running list [K] in the workspace across the chunks.  Per tile a score is compared with the list's K-th entry AS OF THE LAST MERGE;
 *   what passes and is not excluded is appended behind the list in an LDS buffer of 4096 entries (32 KB).  The workgroup merges -- a bitonic
 *   sort of list + survivors under the total order -- only when the buffer could not take a whole further tile in which every score
 *   passes, and at the end of its segment.  A stale threshold admits more survivors, never fewer, so the list after a merge is the one
 *   a merge per tile would give.  After the last chunk one workgroup per user merges the G lists under the same order and adds the G
 *   integer counts into the rank.  G: segments if > 0; else min(4 CUs / B, 1024 / B, 8, tiles of a chunk), at least 1.
 *   Workspace: chunk [B, rows] f32 | s_b,g [B] f32 | 1/|u_b| [B] f32 | list scores [B, Gw, K] f32 | list indices [B, Gw, K] int32 |
 *   counts [B, Gw] int32, each part rounded up to 16 bytes, Gw = segments if > 0, else min(max(1024 / B, 1), 8) -- a function of the
 *   sizes alone, so the size query needs no device.  rows = chunk_rows, or a chunk buffer near 64 MB; never more than N rounded up to
 *   1024.  cat_inv_norm [N] is written unless cat_norm_ready.
 *   Checks (all before any launch, each message names the field): B >= 0, 0 <= N <= INT32_MAX, D a positive multiple of 4 and <= 2048,
 *   K in 1..UR_CATALOG_DEEP_TOPK_MAX, chunk_rows 0 or a positive multiple of 1024, E == 0 or exclude != NULL, gt_index and rank both or
 *   neither, catalog_bf16 in {0, 1}, scorer in {0, 1, 2}, segments in 0..UR_CATALOG_DEEP_SEGMENTS_MAX; then the size query; then the
 *   workspace (16-byte aligned, at least what the query reports); then B == 0 returns 0; then topk_index / topk_score non-null, user /
 *   catalog / cat_inv_norm non-null (catalog and cat_inv_norm may be NULL when N == 0) and user / catalog 16-byte aligned.
 *
 * Size query: with workspace == NULL the call checks the sizes, writes the bytes it needs into workspace_bytes and returns 0 without
 *   launching anything; a refused query leaves workspace_bytes alone. */
#ifndef UNIREC_HIP_DEEP_H
#define UNIREC_HIP_DEEP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UR_CATALOG_DEEP_TOPK_MAX 1024
#define UR_CATALOG_DEEP_SEGMENTS_MAX 16

typedef struct {
  const float* user;         /* [B,D] f32 */
  const void* catalog;       /* [N,D] f32, or bf16 when catalog_bf16 == 1 */
  int32_t catalog_bf16;      /* 0 / 1; anything else is rejected */
  int32_t scorer;            /* 0 the library chooses, 1 vector, 2 f32 MFMA: ur_catalog_select_t.scorer (UR_CATALOG_SCORER_*) */
  float* cat_inv_norm;       /* [N]: in when cat_norm_ready, else out */
  int32_t cat_norm_ready;
  int32_t B;
  int64_t N;
  int32_t D;                 /* a positive multiple of 4, <= 2048 */
  int32_t K;                 /* list length, 1..UR_CATALOG_DEEP_TOPK_MAX */
  int32_t* topk_index;       /* [B,K] out */
  float* topk_score;         /* [B,K] out */
  const int64_t* gt_index;   /* [B] or NULL */
  int32_t* rank;             /* [B] out, with gt_index */
  const int64_t* exclude;    /* [B,E] or NULL; every row sorted ascending, negative entries = empty slots */
  int32_t E;
  int64_t chunk_rows;        /* catalogue rows scored per chunk; 0 = the library chooses (a chunk buffer near 64 MB) */
  int32_t segments;          /* workgroups that share a user's chunk row; 0 = the library chooses.  The outputs do not depend on it */
  void* workspace;           /* 16-byte aligned; NULL = size query */
  int64_t workspace_bytes;   /* in: bytes at workspace; out (size query): bytes needed */
} ur_catalog_deep_t;

int ur_catalog_deep_select(ur_catalog_deep_t* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
