/* unirec_hip_mrl.h -- the Matryoshka family of libunirec_hip.so: the candidate scores and the InfoNCE loss of the joint head on K nested
 * prefixes of the embedding at once.  A fifth header with the conventions of include/unirec_hip.h, include/unirec_hip_loss.h,
 * include/unirec_hip_adapter.h and include/unirec_hip_pool.h (plain device pointers and sizes, the caller owns every buffer including
 * the workspace, every call takes the HIP stream and synchronises nothing, 0 ok / < 0 invalid argument / > 0 hipError_t,
 * ur_last_error() for the text, no device allocation, no environment variable).  The ABI version is the one of unirec_hip.h
 * (UR_ABI_VERSION, 24 since this header exists).
 *
 * Operands.  user [B,D], pos [B,D], neg [B,N,D] f32, 16-byte aligned (neg may be NULL when N == 0).  dims d_0 < d_1 < .. < d_{K-1} = D,
 * 1 <= K <= UR_MRL_MAX_DIMS, every d_k a positive multiple of 4.  Plane k is the head of unirec_hip.h on the first d_k components:
 * candidate j of sample b is pos_b for j = 0 and neg_{b,j-1} for j >= 1, and with x[:d] the first d components of x
 *
 *     scores[k][b][j]        = (u_b[:d_k] . c_bj[:d_k]) * ic * iu,    ic = 1 / max(|c_bj[:d_k]|, 1e-12), iu likewise (F.normalize's floor)
 *     cand_inv_norm[k][b][j] = ic
 *
 * ur_mrl_scores reads every candidate element ONCE for all K planes: one wave per candidate row; lane l adds its elements
 *   4 l + 256 i .. + 3 in ascending order into running sums that it keeps across the prefix boundaries, and at each boundary d_k the 64
 *   lanes' sums so far are folded by xor shuffles (32, 16, .. 1).  That is the chain and the fold of ur_cosine_scores on the contiguous
 *   slice [..., :d_k]: plane k has that call's bits.
 *
 * ur_mrl_infonce runs the scores above (scores and cand_inv_norm are outputs of the call), then per plane the loss of
 *   ur_infonce_fwd_bwd on that plane's scores, and their weighted sum with its gradient:
 *
 *     plane_loss[k] = mean_b( -s_b0 / tau + logsumexp over {0} U valid negatives of s_bj / tau )       s = scores[k]
 *     loss          = sum_k weights[k] * plane_loss[k]      fmaf(weights[k], plane_loss[k], loss) from 0 in ascending k
 *     d_user[b][d]  = sum_{k : d < d_k} weights[k] * g_k[b][d]                fmaf(weights[k], g_k, .) from 0 in ascending k
 *     g_k[b][d]     = grad_scale / B * iu_k * (S_k[d] - u[d] * iu_k * sum_j w_kj s_kj),   S_k[d] = sum_j w_kj ic_kj c_bj[d],
 *     w_kj          = (softmax_j(s_k / tau) - [j == 0]) / tau    (0 for masked negatives)
 *
 *   A plane with weights[k] == 0 is still computed (its plane_loss is written) and is left out of both sums, so it contributes exactly
 *   nothing.  neg_mask [B,N] uint8 (nonzero = valid) or NULL = every negative valid.  d_user == NULL: no backward.
 *   The backward sweeps the candidates ONCE for all planes: the thread that owns the float4 at feature d in segment m
 *   (d_{m-1} <= d < d_m) keeps one accumulator per plane k >= m; the candidates are cut into UR_MRL_BWD_CHUNKS chunks of
 *   ceil((N + 1) / UR_MRL_BWD_CHUNKS), added in chunk order.  With a single plane (dims = {D}, weights = {1}) every output has the bits
 *   of ur_cosine_scores + ur_infonce_fwd_bwd; with weights one-hot at plane k, loss and d_user[:, :d_k] have the bits of that pair run
 *   on the contiguous slices [..., :d_k], and d_user[:, d_k:] is zero.  There are no floating-point atomics and every reduction runs in
 *   a fixed order: two calls give the same bits.
 *   Workspace: row losses [K][B] + w [K][B][N+1] + partial sums [B][UR_MRL_BWD_CHUNKS][sum_k d_k], in floats (each part rounded up to
 *   16 bytes).  Size query: with workspace == NULL the call checks the sizes, writes the bytes it needs into workspace_bytes and returns 0
 *   without launching anything.
 *
 * Checks (all before any launch, each message names the field): K in 1..UR_MRL_MAX_DIMS; dims positive multiples of 4, strictly ascending,
 *   the last equal to D; B >= 0, N >= 0; ur_mrl_infonce: weights finite and >= 0 with at least one positive, temperature > 0; then the
 *   size query; then B == 0 returns 0 and writes nothing; then the pointers non-null and user / pos / neg / workspace 16-byte aligned;
 *   workspace_bytes at least what the size query reports. */
#ifndef UNIREC_HIP_MRL_H
#define UNIREC_HIP_MRL_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UR_MRL_MAX_DIMS 8
#define UR_MRL_BWD_CHUNKS 16

typedef struct {
  const float* user;         /* [B,D] f32 */
  const float* pos;          /* [B,D] f32 */
  const float* neg;          /* [B,N,D] f32 (NULL allowed when N == 0) */
  int32_t B;
  int32_t N;
  int32_t D;
  int32_t K;                 /* number of prefixes, 1..UR_MRL_MAX_DIMS */
  int32_t dims[UR_MRL_MAX_DIMS];   /* d_0 < .. < d_{K-1} = D, multiples of 4; entries past K are ignored */
  float* scores;             /* [K][B][N+1] out */
  float* cand_inv_norm;      /* [K][B][N+1] out */
} ur_mrl_scores_t;

typedef struct {
  const float* user;         /* [B,D] f32 */
  const float* pos;          /* [B,D] f32 */
  const float* neg;          /* [B,N,D] f32 (NULL allowed when N == 0) */
  const uint8_t* neg_mask;   /* [B,N] nonzero = valid, or NULL: every negative is valid */
  int32_t B;
  int32_t N;
  int32_t D;
  int32_t K;
  int32_t dims[UR_MRL_MAX_DIMS];
  float weights[UR_MRL_MAX_DIMS];  /* finite, >= 0, at least one > 0; entries past K are ignored */
  float temperature;         /* > 0 */
  float grad_scale;
  float* scores;             /* [K][B][N+1] out */
  float* cand_inv_norm;      /* [K][B][N+1] out */
  float* plane_loss;         /* [K] out */
  float* loss;               /* [1] out */
  float* d_user;             /* [B,D] out, or NULL: forward only */
  void* workspace;           /* 16-byte aligned; NULL = size query */
  int64_t workspace_bytes;   /* in: bytes at workspace; out (size query): bytes needed */
} ur_mrl_infonce_t;

int ur_mrl_scores(const ur_mrl_scores_t* args, void* stream);
int ur_mrl_infonce(ur_mrl_infonce_t* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
