/* unirec_hip_loss.h -- the loss family of libunirec_hip.so that arrived after include/unirec_hip.h's table of entry points was
 * frozen by its tests: a second header with the same conventions (plain device pointers and sizes, the caller owns every buffer
 * including the workspace, every call takes the HIP stream and synchronises nothing, 0 ok / < 0 invalid argument / > 0 hipError_t,
 * ur_last_error() for the text).  The ABI version is the one of unirec_hip.h (UR_ABI_VERSION, 20 since this header exists).
 *
 * ur_catalog_softmax: the softmax loss of the joint step over the WHOLE resident catalogue, streamed in chunks -- cross-entropy of
 *   each user's ground-truth row against all N rows under the cosine scores of ur_catalog_scores, and its gradient with respect to the
 *   user embeddings (the catalogue is frozen).  All f32 on the device; for user b with ground truth g_b and exclusion row X_b (negative
 *   entries and an entry equal to g_b are ignored: seen items leave, the user's own ground truth never does -- select mode's rule):
 *
 *     s_bn   = (u_b . c_n) * iu_b * ic_n          iu = 1 / max(|u_b|, 1e-12), ic likewise: the bits ur_catalog_scores writes
 *     z_bn   = s_bn * (1 / temperature)           over n in [0,N) \ X_b
 *     lse_b  = log sum_n exp(z_bn)                running maximum: no overflow at any temperature
 *     row_loss_b = -z_b,g + lse_b ;  loss = mean_b row_loss_b
 *     w_bn   = (exp(z_bn - lse_b) - [n == g_b]) / temperature      (0 for excluded n)
 *     G_b    = sum_n w_bn * ic_n * c_n ;  t_b = sum_n w_bn * s_bn
 *     d_user_b = grad_scale / B * iu_b * (G_b - u_b * iu_b * t_b)
 *
 *   (ur_infonce_fwd_bwd's loss and gradient with the candidate set replaced by the catalogue.)
 *   Pass 1 scores the catalogue chunk_rows rows at a time into the workspace with the scoring kernels of select mode (scorer and
 *   catalog_bf16 as in ur_catalog_select_t: the same score bits for both scorers and for a bf16 catalogue and its f32 copy) and folds
 *   each chunk into running (maximum, sum) pairs per user (one per sixteenth of the chunk row, merged in index order at the end).
 *   Pass 2 runs only when d_user != NULL: it scores each chunk again, turns it into
 *   w * ic in place and adds W [B x rows] . C [rows x D] on v_mfma_f32_16x16x4_f32 into per-workgroup [B,D] slabs of the workspace,
 *   which a last kernel adds in index order.  Nothing of size B*N exists; there are no floating-point atomics and every reduction
 *   runs in a fixed order, so two calls give the same bits.  cat_inv_norm [N] is written unless cat_norm_ready.
 *   Checks (all before any launch): D % 4 == 0, D <= 2048, 1 <= N <= INT32_MAX, temperature > 0, chunk_rows 0 or a positive multiple
 *   of 1024, E == 0 or exclude != NULL, catalog_bf16 in {0, 1}, scorer in {0, 1, 2}, user / catalog / workspace 16-byte aligned.
 *   gt_index outside [0,N) and NaN scores are unspecified, as in select mode.
 *   Size query: with workspace == NULL the call checks the sizes, writes the bytes it needs for (B, N, D, chunk_rows, d_user given
 *   or not) into workspace_bytes and returns 0 without launching anything. */
#ifndef UNIREC_HIP_LOSS_H
#define UNIREC_HIP_LOSS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  const float* user;         /* [B,D] f32 */
  const void* catalog;       /* [N,D] f32, or bf16 when catalog_bf16 == 1 */
  int32_t catalog_bf16;      /* 0 / 1; anything else is rejected */
  float* cat_inv_norm;       /* [N]: in when cat_norm_ready, else out */
  int32_t cat_norm_ready;
  const int64_t* gt_index;   /* [B] */
  const int64_t* exclude;    /* [B,E] or NULL; every row sorted ascending, negative entries = empty slots, duplicates allowed */
  int32_t E;                 /* row length of exclude (0 = no exclusion) */
  float temperature;         /* > 0 */
  float grad_scale;
  float* loss;               /* [1] out */
  float* row_loss;           /* [B] out */
  float* lse;                /* [B] out */
  float* d_user;             /* [B,D] out, or NULL: forward only (no second pass) */
  int32_t B;
  int64_t N;
  int32_t D;
  int64_t chunk_rows;        /* catalogue rows scored per chunk; 0 = the library chooses (a chunk buffer near 64 MB) */
  int32_t scorer;            /* 0: the library chooses; 1: vector; 2: f32 MFMA (UR_CATALOG_SCORER_*) */
  void* workspace;           /* 16-byte aligned; NULL = size query */
  int64_t workspace_bytes;   /* in: bytes at workspace; out (size query): bytes needed */
} ur_catalog_softmax_t;

int ur_catalog_softmax(ur_catalog_softmax_t* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
