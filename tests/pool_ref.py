"""Float64 restatement of the pooling family (include/unirec_hip_pool.h: ur_pool_norm_fwd / ur_pool_norm_bwd), forward and backward,
the ulp count the forward is held to, and the cases of the fixture tests/golden/pool_tiny.npz.

Semantics.  x [B,S,D] (the last layer's output), w [D] (the final norm weight), mask [B,S] (nonzero = valid; None = all valid):
    masked_mean   c[b,s] = (mask[b,s] != 0) / n_b,  n_b = the number of valid positions of sample b
    last          c[b,s] = 1 at s* = max{s : mask[b,s] != 0}, 0 elsewhere
    a sample with no valid position has c = 0 everywhere: a zero row, a zero gradient
    rstd_s = rsqrt(mean_d(x[s,:]^2) + eps) ;  y[s,d] = x[s,d] * rstd_s * w[d] ;  pooled[b,d] = sum_s c[b,s] y[b,s,d]
    dx[s,d] = c_s * rstd_s * (g_d w_d - x[s,d] * rstd_s^2 * (1/D) * sum_j g_j w_j x[s,j]),   g = d_pooled[b,:]
Rows with c = 0 never enter a product here (their x is replaced by zeros first), as the kernels never load them."""
import torch

from oracle import weights as W
from tests.golden import cases

F64 = torch.float64
MODES = ("masked_mean", "last")
SLICES = 16            # UR_POOL_NORM_SLICES
WAVES = 4              # rows of a slice in flight in the masked-mean forward


def pool_weights(mask, B, S, mode, dtype=F64):
    """c [B,S]"""
    valid = torch.ones(B, S, dtype=torch.bool) if mask is None else torch.as_tensor(mask).reshape(B, S) != 0
    if mode == "masked_mean":
        n = valid.sum(1, keepdim=True)
        return torch.where(valid, 1.0 / n.clamp_min(1).to(dtype), torch.zeros((), dtype=dtype))
    if mode == "last":
        pos = torch.arange(S).expand(B, S)
        last = torch.where(valid, pos, torch.full_like(pos, -1)).amax(1, keepdim=True)
        return ((pos == last) & valid).to(dtype)
    raise ValueError(mode)


def pool(h, mask, mode):
    """pooled [B,D] of ALREADY normalised hidden states h [B,S,D] (what oracle.qwen3_ref.qwen3_forward returns), differentiable:
    the oracle's pooling step under `mode` (in place of its .mean(dim=1))."""
    B, S, _ = h.shape
    c = pool_weights(mask, B, S, mode, h.dtype)
    return (torch.where(c[..., None] != 0, h, torch.zeros((), dtype=h.dtype)) * c[..., None]).sum(1)


def _live(x, c, dtype):
    return torch.where(c[..., None] != 0, torch.as_tensor(x).detach().cpu().to(dtype), torch.zeros((), dtype=dtype))


def pool_norm_fwd(x, w, eps, mask, mode, dtype=F64):
    """(pooled [B,D], T [B,D]) with T = sum_s |c_s y_sd|, the scale the forward's error is measured in"""
    B, S, _ = x.shape
    c = pool_weights(mask, B, S, mode, dtype)
    xx = _live(x, c, dtype)
    rstd = torch.rsqrt((xx * xx).mean(-1, keepdim=True) + eps)
    y = xx * rstd * torch.as_tensor(w).detach().cpu().to(dtype)
    cy = torch.where(c[..., None] != 0, c[..., None] * y, torch.zeros((), dtype=dtype))
    return cy.sum(1), cy.abs().sum(1)


def pool_norm_bwd(d_pooled, x, w, eps, mask, mode, dtype=F64):
    """dx [B,S,D] by the closed formula above"""
    B, S, D = x.shape
    c = pool_weights(mask, B, S, mode, dtype)
    xx = _live(x, c, dtype)
    rstd = torch.rsqrt((xx * xx).mean(-1, keepdim=True) + eps)
    gw = (torch.as_tensor(d_pooled).detach().cpu().to(dtype) * torch.as_tensor(w).detach().cpu().to(dtype))[:, None, :]      # [B,1,D]
    dot = (gw * xx).sum(-1, keepdim=True)
    dx = c[..., None] * rstd * (gw - xx * rstd * rstd * dot / D)
    return torch.where(c[..., None] != 0, dx, torch.zeros((), dtype=dtype))


# ---- the forward's error bound, in f32 ulps of T ---------------------------------------------------------------------------------------
def nch(D):
    """16-byte chunks of a row per lane (the kernels' template parameter)"""
    k = -(-D // 512)
    return 1 if k <= 1 else (2 if k <= 2 else 4)


def fwd_ulps(D, S, mode, n_valid):
    """First-order count of f32 roundings (unit roundoff u = 2^-24 <= one ulp of T / T) between the exact pooled value and the kernel's,
    relative to T = sum_s |c_s y_sd|, from the kernels' own operation order (csrc/pool.hip):
      sum of squares of a row   1 (the square) + 8 NCH - 1 (a lane's adds, ascending) + 6 (xor-shuffle levels)         = 8 NCH + 6
      mean + eps                2 (the division by D, the add);  rsqrt halves the relative error of its argument: (8 NCH + 8) / 2
      v_rsq_f32                 1 ulp = 2 u
      y = w * (x * rstd)        2
    so every y carries 4 NCH + 8 roundings; sum_s |c_s y_s| = T turns them into (4 NCH + 8) u T.  LAST adds nothing.  MASKED_MEAN
    adds the sums: a wave's rows of a slice, ceil(ceil(S / 16) / 4) - 1 adds (the first lands on 0), 3 for the four waves, 15 for the
    sixteen slices, each relative to a partial sum of magnitude <= n T (the division by n_b, one more rounding, comes last) -- but
    an add with a zero operand is exact, so a sample with n valid rows pays at most n - 1 of them, and n = 1 pays neither an add nor
    the division (x / 1)."""
    per_y = 4 * nch(D) + 8
    if mode == "last" or n_valid <= 1:
        return per_y
    per = -(-S // SLICES)
    adds = (-(-per // WAVES) - 1) + (WAVES - 1) + (SLICES - 1)
    return per_y + min(n_valid - 1, adds) + 1


def fwd_bound(T, D, S, mode, n_valid):
    """[B,D] absolute bound: fwd_ulps f32 ulps of T (n_valid [B])"""
    from tests import ref64
    ulps = torch.tensor([fwd_ulps(D, S, mode, int(n)) for n in n_valid], dtype=F64)[:, None]
    return ulps * ref64.f32_ulp(T)


# ---- the fixture tests/golden/pool_tiny.npz (tests/golden/make_golden_pool.py) ---------------------------------------------------------
# The decoder alone at the _TINYQ shape on one left-padded and one right-padded batch (B 3, S 40; sample 0 unpadded, the others padded
# by up to 30 %: every row keeps a valid token).  Inputs are regenerated from the seeds; the file holds outputs only.
POOL_CASES = {
    "left": dict(kind="qwen", seed=61, B=3, S=40, pad_side="left", qwen=cases._TINYQ),
    "right": dict(kind="qwen", seed=62, B=3, S=40, pad_side="right", qwen=cases._TINYQ),
}


def pool_case_inputs(side):
    """(x [B,S,D] f32, attention_mask [B,S] int64, r [B,D] f32): the decoder's inputs_embeds, the mask and the weights of the scalar
    loss = sum(pooled * r) whose gradient the fixture stores"""
    case = POOL_CASES[side]
    x, am = cases.qwen_inputs(case)
    r = W.normal("pool/r", (case["B"], case["qwen"]["D"]), case["seed"], std=1.0)
    assert (am.sum(1) > 0).all()
    return x, am, r

