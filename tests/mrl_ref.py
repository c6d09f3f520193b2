"""Float64 restatement of the Matryoshka family (include/unirec_hip_mrl.h: ur_mrl_scores / ur_mrl_infonce) and the seeded inputs of the
fixture tests/golden/mrl_tiny.npz.

Every term is the head's own reference (tests/ref64.py) on a prefix: plane k of the scores is ref64.cosine_scores on
user[:, :d_k], pos[:, :d_k], neg[..., :d_k] (each prefix renormalised), plane k of the loss is ref64.infonce on them, and

    loss   = sum_k weights[k] * plane_loss[k]
    d_user = sum_k weights[k] * pad(d_user_k)         d_user_k [B, d_k] zero-padded to D

``dtype=torch.float32`` re-evaluates the same formula in float32: the yardstick of ref64.assert_f32_close.  Plain torch on the CPU.
"""
import numpy as np
import torch

from tests import ref64

F64 = torch.float64

# the fixture (tests/golden/make_golden_mrl.py): the reference's InfoNCELoss on the slices
MRL_DIMS = (4, 12, 32)
MRL_WEIGHTS = {"ones": (1.0, 1.0, 1.0), "mixed": (0.5, 0.0, 2.0)}
MRL_CASES = {"masked": dict(B=3, N=7, D=32, mask=True, seed=4101), "plain": dict(B=2, N=5, D=32, mask=False, seed=4102)}
MRL_TAU = 0.07


def mrl_case_inputs(name):
    """(user [B,D], pos [B,D], neg [B,N,D] f32, neg_mask bool [B,N] or None) of fixture case `name`, from its seed; a mask keeps at
    least one valid negative per row"""
    c = MRL_CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    user = torch.randn(c["B"], c["D"], generator=g)
    pos = torch.randn(c["B"], c["D"], generator=g)
    neg = torch.randn(c["B"], c["N"], c["D"], generator=g)
    mask = None
    if c["mask"]:
        mask = torch.rand(c["B"], c["N"], generator=g) > 0.4
        mask[torch.arange(c["B"]), torch.randint(0, c["N"], (c["B"],), generator=g)] = True
    return user, pos, neg, mask


def scores(user, pos, neg, dims, dtype=F64):
    """[K, B, 1 + N]: plane k = ref64.cosine_scores on the first dims[k] components"""
    return torch.stack([ref64.cosine_scores(user[:, :d], pos[:, :d], neg[..., :d], dtype) for d in dims])


def ranks(plane_scores, neg_mask=None):
    """[K, B]: ref64.mrr_rank of every plane"""
    return torch.stack([ref64.mrr_rank(s, neg_mask) for s in plane_scores])


def plane_terms(user, pos, neg, neg_mask, dims, tau, grad_scale=1.0, dtype=F64):
    """(plane_loss [K], g [K, B, D]) in `dtype`: ref64.infonce on every prefix, its gradient zero-padded to D"""
    assert dims[-1] == user.shape[1]
    plane, g = [], torch.zeros((len(dims),) + tuple(user.shape), dtype=dtype)
    for k, d in enumerate(dims):
        l, gk = ref64.infonce(user[:, :d], pos[:, :d], neg[..., :d], neg_mask, tau, grad_scale, dtype)
        plane.append(l)
        g[k, :, :d] = gk
    return torch.stack(plane), g


def combine(plane_loss, g, weights):
    """(loss, d_user) = the weighted sums of plane_terms' outputs, in their dtype"""
    lam = torch.tensor(weights, dtype=plane_loss.dtype)
    assert lam.shape == plane_loss.shape
    return (lam * plane_loss).sum(), (lam[:, None, None] * g).sum(0)


def infonce(user, pos, neg, neg_mask, dims, weights, tau, grad_scale=1.0, dtype=F64):
    """(loss, plane_loss [K], d_user [B, D]) in `dtype`"""
    plane, g = plane_terms(user, pos, neg, neg_mask, dims, tau, grad_scale, dtype)
    loss, du = combine(plane, g, weights)
    return loss, plane, du


def fixture_keys():
    return sorted(f"{c}/{k}" for c in MRL_CASES for k in ["plane_loss"] + [f"{w}/{q}" for w in MRL_WEIGHTS for q in ("loss", "d_user")])


def load_fixture(golden_dir):
    import os
    return dict(np.load(os.path.join(golden_dir, "mrl_tiny.npz")))
