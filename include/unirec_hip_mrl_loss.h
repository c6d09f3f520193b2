/* unirec_hip_mrl_loss.h -- the Matryoshka form of the full-catalogue softmax loss of libunirec_hip.so: ur_catalog_softmax
 * (include/unirec_hip_loss.h) on K nested prefixes of the embedding in one call, the resident [N,D] catalogue and the [B,D] user block
 * read in place with their row stride D -- no contiguous [N,d_k] copy.  It is the training side of what include/unirec_hip_funnel.h
 * deploys.  A tenth header with the conventions of include/unirec_hip_loss.h (plain device pointers and sizes, the caller owns every
 * buffer including the workspace, a NULL workspace is a size query, every check runs before any launch and names its field, every
 * call takes the HIP stream and synchronises nothing, 0 ok / < 0 invalid argument / > 0 hipError_t, ur_last_error() for the text).  The
 * ABI version is the one of unirec_hip.h (UR_ABI_VERSION, 29 since this header exists).  Every older entry point is untouched.
 *
 * ur_catalog_mrl_softmax: with plane k = ur_catalog_softmax on the first d_k = dims[k] components of every user and catalogue row,
 *   every prefix renormalised (iu_k, ic_k = the inverse norms of the prefixes),
 *
 *     plane_loss[k] = mean_b row_loss[k][b]
 *     loss          = sum_k weights[k] * plane_loss[k]          fmaf(weights[k], plane_loss[k], loss) from 0, ascending k
 *     d_user[b][d]  = sum_{k : d < d_k} weights[k] * g_k[b][d]  fmaf(weights[k], g_k[b][d], .) from 0, ascending k
 *
 *   g_k = the d_user of ur_catalog_softmax on the slice (grad_scale / B included).  A plane of weight 0 is still computed -- its
 *   row_loss, lse and plane_loss are written -- and contributes exactly nothing to both sums: it is skipped, not multiplied by 0
 *   (ur_mrl_infonce's rule).  gt_index, exclude / E, temperature, grad_scale, chunk_rows and scorer are shared by all planes and keep
 *   the meaning and the checks they have in ur_catalog_softmax_t.
 *
 *   The bit contract, at equal explicit chunk_rows, for f32 and bf16 catalogues and both scorers: row_loss[k], lse[k], plane_loss[k]
 *   and cat_inv_norm[k] equal, in every bit, what ur_catalog_softmax returns (row_loss, lse, loss, cat_inv_norm) on the contiguous
 *   copies user[:, :d_k] and catalog[:, :d_k]; with weights one-hot at plane k, loss and d_user[:, :d_k] equal that call's and
 *   d_user[:, d_k:] is zero; with K = 1, dims = {D}, weights = {1} every output equals ur_catalog_softmax's on the same buffers.
 *   So plane k's score is the exact scorer's per-lane chain over the 4-element pieces d = 4 l + 256 j below d_k, the same 64-way tree,
 *   then (v * iu_k) * ic_k; its fold uses the segment size of the chunk rows; its gradient product uses the row splits of (B, d_k,
 *   rows).  There are no floating-point atomics and every reduction runs in a fixed order: two calls give the same bits.  What lies
 *   behind d_k in a row is live data of the same row; no result of plane k depends on it.
 *
 *   Sequence.  The user prefix norms inv_u [K][B] (the row-norm chain with a snapshot per prefix, the kernel of
 *   ur_catalog_prefix_norms); cat_inv_norm [K][N] by that kernel in one read of the catalogue unless cat_norm_ready; the ground-truth
 *   scores ref [K][B].  Pass 1 per chunk: the scores of every plane into its [B][rows] part of the chunk buffer, then the fold kernel
 *   per plane; the finish kernel per plane; the weighted loss.  Pass 2 (d_user != NULL) per chunk: the scores again, then per plane
 *   the weight kernel and the gradient product on the plane's own slabs; a last kernel forms every g_k and the weighted sum.
 *   Scoring.  MFMA scorer (scorer 2, or 0 where the library chooses it by (B, D) as ur_catalog_softmax does): runs of up to three
 *   consecutive planes no wider than 1024 take ONE pass of a group kernel -- the chain of c runs over ascending pieces, its value after
 *   the last piece below d_k is plane k's chain and enters plane k's own tree there, so the products are those of one pass at the run's
 *   widest prefix; a plane left alone or wider than 1024 takes the single-plane MFMA kernel with the row strides.  Vector scorer
 *   (scorer 1): one launch per plane of the vector kernel with the row strides, prefix d_k as its D -- the independent route to the same
 *   bits.
 *   chunk_rows == 0: the library chooses rows so that the K score planes [K][B][rows] together stay near the 64 MB chunk buffer:
 *   rows = (64 MB / (4 K B)) rounded down to a multiple of 1024, at least 1024, never more than N rounded up to 1024.
 *   Workspace: scores [K][B][rows] f32 | inv_u [K][B] | ref [K][B] | m, l, t: [K][B][16] each | for k = 0 .. K-1: slabs
 *   [nsplit_k][B][d_k] (with d_user only; nsplit_k = the row splits ur_catalog_softmax takes at (B, d_k, rows)), each part rounded up
 *   to 16 bytes.  Nothing of size B x N and nothing of size N x d.
 *   Checks (all before any launch, each message names the field): B >= 0; 1 <= N <= INT32_MAX; D a positive multiple of 4, <= 2048;
 *   chunk_rows 0 or a positive multiple of 1024; E == 0 or exclude != NULL; catalog_bf16 in {0, 1}; scorer in {0, 1, 2}; K in
 *   1..UR_MRL_MAX_DIMS; dims positive multiples of 4 (8 for a bf16 catalogue), strictly ascending, the last equal to D; weights finite
 *   and >= 0 with at least one > 0; temperature > 0 and finite; then the size query; then the workspace (16-byte aligned, at least what
 *   the query reports); then B == 0 returns 0; then user / catalog / cat_inv_norm / gt_index non-null, user and catalog 16-byte aligned,
 *   plane_loss / loss / row_loss / lse non-null, d_user NULL or 16-byte aligned.  gt_index outside [0,N) and NaN scores are unspecified.
 *   Size query: with workspace == NULL the call checks the sizes, writes the bytes it needs into workspace_bytes and returns 0 without
 *   launching anything; a refused query leaves workspace_bytes alone. */
#ifndef UNIREC_HIP_MRL_LOSS_H
#define UNIREC_HIP_MRL_LOSS_H
#include <stdint.h>
#include "unirec_hip_mrl.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  const float* user;         /* [B,D] f32 */
  const void* catalog;       /* [N,D] f32, or bf16 when catalog_bf16 == 1 */
  int32_t catalog_bf16;      /* 0 / 1; anything else is rejected */
  float* cat_inv_norm;       /* [K,N], plane k the norms of prefix dims[k]: in when cat_norm_ready, else out */
  int32_t cat_norm_ready;
  const int64_t* gt_index;   /* [B] */
  const int64_t* exclude;    /* [B,E] or NULL; every row sorted ascending, negative entries = empty slots, duplicates allowed */
  int32_t E;                 /* row length of exclude (0 = no exclusion) */
  float temperature;         /* > 0 */
  float grad_scale;
  int32_t K;                 /* number of prefixes, 1..UR_MRL_MAX_DIMS */
  int32_t dims[UR_MRL_MAX_DIMS];      /* strictly ascending multiples of 4 (8 for bf16), the last == D; entries past K are ignored */
  float weights[UR_MRL_MAX_DIMS];     /* finite, >= 0, at least one > 0 */
  float* plane_loss;         /* [K] out */
  float* loss;               /* [1] out */
  float* row_loss;           /* [K,B] out */
  float* lse;                /* [K,B] out */
  float* d_user;             /* [B,D] out, or NULL: forward only (no second pass) */
  int32_t B;
  int64_t N;
  int32_t D;
  int64_t chunk_rows;        /* catalogue rows scored per chunk; 0 = the library chooses (K score planes near 64 MB together) */
  int32_t scorer;            /* 0: the library chooses; 1: vector; 2: f32 MFMA (UR_CATALOG_SCORER_*) */
  void* workspace;           /* 16-byte aligned; NULL = size query */
  int64_t workspace_bytes;   /* in: bytes at workspace; out (size query): bytes needed */
} ur_catalog_mrl_softmax_t;

int ur_catalog_mrl_softmax(ur_catalog_mrl_softmax_t* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
