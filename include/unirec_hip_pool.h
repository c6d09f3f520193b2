/* unirec_hip_pool.h -- the pooling family of libunirec_hip.so: the final RMSNorm of the decoder fused with a pooling rule that looks at
 * the attention mask.  A fourth header with the conventions of include/unirec_hip.h, include/unirec_hip_loss.h and
 * include/unirec_hip_adapter.h (plain device pointers and sizes, the caller owns every buffer, every call takes the HIP stream and
 * synchronises nothing, 0 ok / < 0 invalid argument / > 0 hipError_t, ur_last_error() for the text).  The ABI version is the one of
 * unirec_hip.h (UR_ABI_VERSION, 22 since this header exists).  The default pooling of the product -- the mean over all S positions,
 * padding included -- stays ur_rmsnorm_fwd + ur_mean_pool_fwd of unirec_hip.h; this family serves the two other rules.
 *
 * Operands.  x [B,S,D] bf16: the last layer's output.  w [D] f32: the final norm weight.  mask [B,S] uint8, nonzero = valid; a NULL
 * mask means every position is valid (and gives the bits an explicit all-ones mask gives).  eps >= 0.
 *
 * Pooling weights c[b,s]:
 *   UR_POOL_MASKED_MEAN   c[b,s] = (mask[b,s] != 0) / n_b,   n_b = the number of valid positions of sample b
 *   UR_POOL_LAST          c[b,s] = 1 at s* = max{s : mask[b,s] != 0}, 0 elsewhere.  For a contiguous left-padded or right-padded mask
 *                         that is the usual last-token pooling; it is also right for a batch that mixes both sides and for masks with holes.
 *   A sample with NO valid position gives a zero row of `pooled` and a zero gradient: the product's rule (a mean over nothing and
 *   a last token of nothing have no value; zeros keep a batch with an empty sample finite).
 *
 * ur_pool_norm_fwd:  pooled[b,d] = sum_s c[b,s] y[b,s,d],   y[s,d] = x[s,d] * rstd_s * w[d],   rstd_s = rsqrt(mean_d(x[s,:]^2) + eps),
 *   everything in f32 (y is never rounded to bf16), pooled f32 [B,D].  Rows with c = 0 are NOT LOADED: any bit pattern in them (NaN,
 *   Inf) leaves the output bits unchanged.  The reduction order is fixed and there are no floating-point atomics: two calls give the same
 *   bits.  Per row: lane l of a wave sums the squares of its elements 8 (l + 64 i) .. + 7 in ascending order, the 64 lanes are folded by
 *   xor shuffles (32, 16, .. 1).  MASKED_MEAN: S is cut into UR_POOL_NORM_SLICES slices of ceil(S / UR_POOL_NORM_SLICES) positions; in a
 *   slice, wave v of four adds its valid rows v, v + 4, .. in ascending order, the waves are added 0 + 1 + 2 + 3, the slices in ascending
 *   order, and the sum is divided by n_b.  LAST reads B rows.
 *
 * ur_pool_norm_bwd:  with g = d_pooled[b,:] (f32; the base model is frozen: there is no d w)
 *     dx[s,d] = c_s * rstd_s * (g_d w_d - x[s,d] * rstd_s^2 * (1/D) * sum_j g_j w_j x[s,j]),  rounded to nearest even into bf16 [B,S,D].
 *   rstd is recomputed from the row in the same pass (no rstd tensor crosses the ABI).  Rows with c = 0 are written as +0 without being
 *   read.  The kernel writes EVERY row of dx: no memset is needed.
 *
 * Workspace: ur_pool_norm_workspace_bytes(B, D, mode) bytes serve either call of that mode (MASKED_MEAN: the slice sums and counts of
 *   the forward; both modes: one int per sample for the backward).  It returns -1 for arguments the calls would refuse.
 * Checks (all before any launch): mode is one of the two; D > 0, D % 8 == 0, D <= 2048; S > 0; B >= 0; eps >= 0; then B == 0 returns 0
 *   and writes nothing; x, w and pooled / d_pooled, dx non-null and 16-byte aligned (mask: any alignment, may be NULL); the workspace
 *   non-null, 16-byte aligned and at least ur_pool_norm_workspace_bytes(B, D, mode) bytes. */
#ifndef UNIREC_HIP_POOL_H
#define UNIREC_HIP_POOL_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UR_POOL_MASKED_MEAN 1
#define UR_POOL_LAST 2
#define UR_POOL_NORM_SLICES 16      /* slices of S in the MASKED_MEAN forward */

int64_t ur_pool_norm_workspace_bytes(int32_t B, int32_t D, int32_t mode);
int ur_pool_norm_fwd(const void* x, const float* w, const uint8_t* mask, float* pooled, int32_t B, int32_t S, int32_t D, float eps,
                     int32_t mode, void* workspace, int64_t workspace_bytes, void* stream);
int ur_pool_norm_bwd(const float* d_pooled, const void* x, const float* w, const uint8_t* mask, void* dx, int32_t B, int32_t S,
                     int32_t D, float eps, int32_t mode, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
