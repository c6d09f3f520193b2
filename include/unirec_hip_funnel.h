/* unirec_hip_funnel.h -- funnel retrieval of libunirec_hip.so: the long two-stage retrieval of include/unirec_hip_coarse_deep.h run on
 * PREFIXES of the embedding, read in place from the resident [N, ld] catalogue with its row stride -- no contiguous [N, dim] copy.  It is
 * the deployment side of a Matryoshka-trained model (include/unirec_hip_mrl.h): shortlist on a narrow prefix, re-rank the survivors on
 * wider ones.  A ninth header with the conventions of the eight before it (plain device pointers and sizes, the caller owns every buffer
 * including the workspace, every call takes the HIP stream and synchronises nothing, 0 ok / < 0 invalid argument / > 0 hipError_t,
 * ur_last_error() for the text, no device allocation, no environment variable).  The ABI version is the one of unirec_hip.h
 * (UR_ABI_VERSION, 28 since this header exists).  Every older entry point is untouched: its kernels, launches, limits and bits stay.
 *
 * Strides.  catalog is [N, ld] and user [B, ldu], row-major, in elements; only the first dim components of a row are read, and
 * whatever lies behind them in the row is live data that no result depends on.  With dim == ld == ldu the operands are the contiguous
 * ones of the older calls.
 *
 * ur_catalog_prefix_norms: inv[l][n] = 1 / max(|catalog[n, :dims[l]]|, 1e-12) for L prefixes of every row, catalog f32 or bf16.
 *   Plane l holds, bit for bit, what the row-norm kernel of ur_catalog_scores (and of every call of this family) computes for the
 *   contiguous slice catalog[:, :dims[l]]: lane j of a wave adds the squares of its 4-element pieces at d = 4 j + 256 i in ascending i,
 *   the 64 lanes are folded by xor shuffles (32, 16, .. 1), then 1 / max(sqrt(.), 1e-12).
 *   ONE pass was built: a wave reads its row once up to dims[L-1]; the lane's chain runs over ascending d, so its partial sum after the
 *   last piece below a boundary dims[l] is already the chain of that prefix -- the lane keeps that snapshot per plane and the same fold
 *   is applied to each snapshot.  The catalogue is read once for all L planes.
 *   Checks (all before any launch, each message names the field): catalog_bf16 in {0, 1}; 0 <= N <= INT32_MAX; L in
 *   1..UR_MRL_MAX_DIMS; ld a positive multiple of 4 (8 for a bf16 catalogue); dims strictly ascending, every one a positive multiple of
 *   4 (8 for bf16), at most ld and at most 2048; then N == 0 returns 0; then catalog / inv non-null and catalog 16-byte aligned.
 *   No workspace.
 *
 * ur_catalog_funnel_select: ur_catalog_coarse_deep_select over the first dim components of a bf16 [N, ld] catalogue and of an f32
 *   [B, ldu] user block.  EVERY output -- the lists, the coarse score bits, the rank and the norms written -- equals, in every bit, what
 *   ur_catalog_coarse_deep_select returns on the contiguous copies user[:, :dim] and catalog[:, :dim], for any chunk_rows, segments,
 *   gt_index, exclude and cat_norm_ready.
 *   Sequence.  The user prefix is cast to bf16 (nearest even) into the workspace as a contiguous [B, dim] block and normed there by the
 *   row-norm kernel; cat_inv_norm [N] is the prefix's plane, written (the kernel of ur_catalog_prefix_norms, one plane) unless
 *   cat_norm_ready; the diagonal launch; then per chunk the prefix scorer and the sweep kernel, and the merge kernel at the end
 *   (catalog_deep_sweep_kernel / catalog_deep_merge_kernel, unchanged).
 *   Scorer.  catalog_scores_bf16_prefix_kernel: the coarse scorer of include/unirec_hip_coarse.h with a catalogue row stride.  The order
 *   of the sum is the one that header fixes, by dim alone: K steps of 32 elements, step s to chain s mod NC, NC = 2 for dim <= 1024 and
 *   4 above, the chains added as c0 + c1 or (c0 + c2) + (c1 + c3).  The K step that ends short is masked by dim: a lane whose 8
 *   elements lie at or past dim brings zeros and does not load -- the elements there are live data of the same row, not padding.
 *   User group: 64 users per workgroup for dim <= 1024, 32 above (UR_FUNNEL_USER_GROUP and half of it) -- a function of dim alone, and
 *   the groups of the contiguous scorer.  Diagonal mode keeps its rule: the same instructions in the same order as the chunk pass runs
 *   for that pair.
 *   Workspace: that of ur_catalog_coarse_deep_select with D = dim: u~ [B,dim] bf16 | iu~ [B] f32 | s~_b,g [B] f32 | chunk [B, rows] f32
 *   | list scores [B, Gw, K] f32 | list indices [B, Gw, K] int32 | counts [B, Gw] int32, each part rounded up to 16 bytes; Gw = segments
 *   if > 0, else min(max(1024 / B, 1), 8); rows = chunk_rows, or a chunk buffer near 64 MB, never more than N rounded up to 1024.  Nothing
 *   of size B x N and nothing of size N x dim.
 *   Checks (all before any launch, each message names the field): B >= 0, 0 <= N <= INT32_MAX, dim a positive multiple of 8 and <= 2048,
 *   ld >= dim, ldu >= dim, ld a multiple of 8 (every row stays 16-byte aligned), ldu a multiple of 4, chunk_rows 0 or a positive
 *   multiple of 1024, E == 0 or exclude != NULL, gt_index and rank both or neither, K in 1..UR_CATALOG_DEEP_TOPK_MAX, catalog_bf16 == 1,
 *   segments in 0..UR_CATALOG_DEEP_SEGMENTS_MAX; then the size query; then the workspace (16-byte aligned, at least what the query
 *   reports); then B == 0 returns 0; then topk_index / topk_score non-null, user / catalog / cat_inv_norm non-null (catalog and
 *   cat_inv_norm may be NULL when N == 0) and user / catalog 16-byte aligned.
 *
 * ur_catalog_funnel_rerank: ur_catalog_deep_rerank over the first dim components: catalog [N, ld] f32 or bf16, user [B, ldu] f32,
 *   K_in and k up to UR_CATALOG_DEEP_TOPK_MAX, cat_inv_norm the prefix's plane (in, or written unless cat_norm_ready).  The index and
 *   score bits are those of ur_catalog_deep_rerank on the contiguous slices user[:, :dim], catalog[:, :dim]; with dim == ld == ldu they
 *   are that call's on the same buffers.  One wave per (user, slot) runs the exact scorer's chain over d < dim, iu_b the norm of the
 *   unrounded user prefix; then the sorting launch of ur_catalog_deep_rerank, unchanged.
 *   Workspace: iu [B] f32 | scores [B, K_in] f32, each part rounded up to 16 bytes.
 *   Checks (all before any launch): B >= 0, 1 <= N <= INT32_MAX, catalog_bf16 in {0, 1}, dim a positive multiple of 4 (8 for a bf16
 *   catalogue) and <= 2048, ld >= dim and a multiple of 4 (8 for bf16), ldu >= dim and a multiple of 4, K_in in
 *   1..UR_CATALOG_DEEP_TOPK_MAX, k in 1..K_in; then the size query; the workspace; B == 0 returns 0; then index / topk_index /
 *   topk_score / user / catalog / cat_inv_norm non-null and user / catalog 16-byte aligned.
 *
 * Size query (select and re-rank): with workspace == NULL the call checks the sizes, writes the bytes it needs into workspace_bytes and
 *   returns 0 without launching anything; a refused query leaves workspace_bytes alone. */
#ifndef UNIREC_HIP_FUNNEL_H
#define UNIREC_HIP_FUNNEL_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UR_FUNNEL_MAX_DIMS 8       /* = UR_MRL_MAX_DIMS (include/unirec_hip_mrl.h) */
#define UR_FUNNEL_USER_GROUP 64    /* users a workgroup of the prefix scorer stages for dim <= 1024; half of it above */

typedef struct {
  const void* catalog;       /* [N,ld] f32, or bf16 when catalog_bf16 == 1 */
  int32_t catalog_bf16;      /* 0 / 1; anything else is rejected */
  int64_t N;
  int64_t ld;                /* row stride in elements, a multiple of 4 (8 for bf16) */
  int32_t L;                 /* number of prefixes, 1..UR_FUNNEL_MAX_DIMS */
  int32_t dims[UR_FUNNEL_MAX_DIMS];   /* strictly ascending multiples of 4 (8 for bf16), <= ld, <= 2048; entries past L are ignored */
  float* inv;                /* [L,N] out */
} ur_catalog_prefix_norms_t;

typedef struct {
  const float* user;         /* [B,ldu] f32 */
  const void* catalog;       /* [N,ld] bf16 */
  int32_t catalog_bf16;      /* must be 1 */
  float* cat_inv_norm;       /* [N], the plane of this prefix: in when cat_norm_ready, else out */
  int32_t cat_norm_ready;
  int32_t B;
  int64_t N;
  int32_t dim;               /* the prefix: a positive multiple of 8, <= 2048 */
  int64_t ld;                /* catalogue row stride in elements: >= dim, a multiple of 8 */
  int64_t ldu;               /* user row stride in elements: >= dim, a multiple of 4 */
  int32_t K;                 /* list length, 1..UR_CATALOG_DEEP_TOPK_MAX (1024) */
  int32_t* topk_index;       /* [B,K] out */
  float* topk_score;         /* [B,K] out: the coarse scores s~ of the prefix */
  const int64_t* gt_index;   /* [B] or NULL */
  int32_t* rank;             /* [B] out, with gt_index */
  const int64_t* exclude;    /* [B,E] or NULL; every row sorted ascending, negative entries = empty slots */
  int32_t E;
  int64_t chunk_rows;        /* catalogue rows scored per chunk; 0 = the library chooses (a chunk buffer near 64 MB) */
  int32_t segments;          /* workgroups that share a user's chunk row; 0 = the library chooses.  The outputs do not depend on it */
  void* workspace;           /* 16-byte aligned; NULL = size query */
  int64_t workspace_bytes;   /* in: bytes at workspace; out (size query): bytes needed */
} ur_catalog_funnel_select_t;

typedef struct {
  const float* user;         /* [B,ldu] f32 */
  const void* catalog;       /* [N,ld] f32, or bf16 when catalog_bf16 == 1 */
  int32_t catalog_bf16;      /* 0 / 1; anything else is rejected */
  float* cat_inv_norm;       /* [N], the plane of this prefix: in when cat_norm_ready, else out */
  int32_t cat_norm_ready;
  int32_t B;
  int64_t N;
  int32_t dim;               /* the prefix: a positive multiple of 4 (8 for bf16), <= 2048 */
  int64_t ld;                /* catalogue row stride in elements: >= dim, a multiple of 4 (8 for bf16) */
  int64_t ldu;               /* user row stride in elements: >= dim, a multiple of 4 */
  const int32_t* index;      /* [B,K_in]; entries outside [0,N) are empty slots */
  int32_t K_in;              /* 1..UR_CATALOG_DEEP_TOPK_MAX (1024) */
  int32_t k;                 /* 1..K_in */
  int32_t* topk_index;       /* [B,k] out */
  float* topk_score;         /* [B,k] out: the exact scores of the prefix */
  void* workspace;           /* 16-byte aligned; NULL = size query */
  int64_t workspace_bytes;   /* in: bytes at workspace; out (size query): bytes needed */
} ur_catalog_funnel_rerank_t;

int ur_catalog_prefix_norms(const ur_catalog_prefix_norms_t* args, void* stream);
int ur_catalog_funnel_select(ur_catalog_funnel_select_t* args, void* stream);
int ur_catalog_funnel_rerank(ur_catalog_funnel_rerank_t* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
