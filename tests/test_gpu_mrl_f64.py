"""GPU: the Matryoshka family (include/unirec_hip_mrl.h: ur_mrl_scores / ur_mrl_infonce) against the float64 restatement of
tests/mrl_ref.py (held to the reference's own loss in tests/test_mrl_host.py) and, plane by plane and bit for bit, against the kernels of
the head on contiguous slices.

Shapes: every boundary the kernels have is crossed.
  dims (64, 128, 256, 512, 1024)   boundaries inside the first 256-element sweep of a wave (lanes 16 and 32 idle below them) and on sweep ends
       (4, 260, 1020, 1024)        lane 1, a boundary in the second sweep, a 4-wide last segment
       (4, 8)                      the smallest legal case
       (1024,)                     K = 1
       eight dims up to 2048       K = 8 and D > 1024: the backward's feature stride wraps
  (B, N) (1, 0) no negatives; (2, 1) one; (3, 14): N + 1 < 16 leaves backward chunks empty; (65, 37): B past the 64-lane mean;
       (2, 10000) at D = 8: 20002 rows against the 16384 the score launch covers at once.
  masks: none, random, exactly one valid negative per row, all invalid.

Criteria.  Scores, inverse norms, plane_loss, loss and d_user by ref64.assert_f32_close (8 e32 + 2^-20 scale, e32 from the f32 run of
the same reference; the loss's scale is |loss| + 1).  A row without a valid negative has an exact gradient of 0; it is held to the bound
tests/test_gpu_head_primitives.py::test_infonce_fwd_bwd derives for one plane, summed over the planes:
sum_k weights[k] 2^-22 gscale / (B |u[:d_k]| tau^2).  Each test prints its worst error / bound as "[ratio] ...".

Temperature.  0.07 where the narrowest prefix is 64 wide or more.  The dims cases that start at 4 run the loss AND gradient at 1.0, as
test_infonce_fwd_bwd runs its D = 4 rows with a single valid negative: on 4 components the cosines fill [-1, 1], at tau = 0.07 the
logits span +-14 and most rows saturate (p_0 -> 1).  The kernels form p_0 - 1 from exp(z_0 - lse), whose absolute floor 2^-24 / tau is
the very term the no-valid-negative bound above is made of; a saturated row is such a row in all but name, and no criterion relative
to its own vanishing gradient holds for it in f32 -- in ur_infonce_fwd_bwd, whose arithmetic this family restates bit for bit, no more
than here.  At tau = 0.07 those cases are still held on plane_loss and loss."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import mrl_ref, ref64  # noqa: E402
from unirec_amd import _lib, hip  # noqa: E402

# entry point of include/unirec_hip_mrl.h -> its float64 tests (tests/test_mrl_host.py holds this dict to the header)
COVERS = {
    "ur_mrl_scores": ["test_mrl_scores_float64"],
    "ur_mrl_infonce": ["test_mrl_infonce_float64"],
}

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
TAU = float(torch.tensor(0.07, dtype=F32))

DIMS = {
    "sweep": (64, 128, 256, 512, 1024),
    "odd": (4, 260, 1020, 1024),
    "tiny": (4, 8),
    "single": (1024,),
    "eight": (4, 64, 256, 520, 1024, 1028, 2044, 2048),
}
BN = [(1, 0), (2, 1), (3, 14), (65, 37)]
CASES = [(name, B, N) for name in DIMS for B, N in BN] + [("tiny", 2, 10000)]
MASKS = ("none", "random", "one", "all_invalid")
WORST = {}


def _tau(dims):
    """the temperature of the gradient check (module docstring): 0.07 unless the narrowest prefix saturates the softmax at it"""
    return TAU if dims[0] >= 64 else 1.0


def _note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio))
    print(f"[ratio] {kernel}: {float(ratio):.4f}")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(B, N, D, seed=7):
    """Gaussian user, negatives and positives, the positive leaning a tenth towards its user (cos about 0.1 at full width, what the
    largest of a few dozen random cosines is at D = 1024, so the rows' scales stay where independent vectors put them).  A positive
    independent of the user makes the one-candidate rows (N = 0) a pure cancellation -- a cosine of 1e-4 out of 2044 terms of size 1 --
    that assert_f32_close would measure against its own magnitude; no trained model has such a positive."""
    g = _gen(seed * 1000 + B + 7 * N + D)
    user = torch.randn(B, D, generator=g)
    return user, torch.randn(B, D, generator=g) + 0.1 * user, torch.randn(B, N, D, generator=g)


def _mask(mode, B, N, seed=11):
    g = _gen(seed + B + N)
    if mode == "none":
        return None
    if mode == "random":
        return torch.rand((B, N), generator=g) > 0.3
    m = torch.zeros((B, N), dtype=torch.bool)
    if mode == "one" and N > 0:
        m[torch.arange(B), torch.randint(0, N, (B,), generator=g)] = True
    return m


def _weights(K):
    """all ones, and (0.5, 0, 2, ...): a zero weight, unequal ones (K = 1: a single non-unit weight)"""
    return [(1.0,) * K, ((0.5, 0.0, 2.0, 1.0, 0.0, 0.25, 3.0, 1.5)[:K] if K > 1 else (0.5,))]


def _dev(t):
    return None if t is None else (t.to(torch.uint8) if t.dtype == torch.bool else t).to(DEV)


@pytest.mark.parametrize("name,B,N", CASES)
def test_mrl_scores_float64(name, B, N):
    """every plane of the scores and inverse norms against float64; ranks = ref64.mrr_rank of the kernel's own scores"""
    dims = DIMS[name]
    user, pos, neg = _inputs(B, N, dims[-1])
    s, inv = hip.mrl_scores(_dev(user), _dev(pos), _dev(neg), dims)
    assert s.shape == inv.shape == (len(dims), B, N + 1)
    s64, s32 = mrl_ref.scores(user, pos, neg, dims), mrl_ref.scores(user, pos, neg, dims, dtype=F32)
    cand = torch.cat([pos[:, None], neg], 1)
    for k, d in enumerate(dims):
        what = f"mrl_scores {name} B{B} N{N} plane {k} (d {d})"
        _note("mrl scores", ref64.assert_f32_close(s[k].cpu(), s64[k], s32[k], what=what))
        i64 = 1.0 / cand[..., :d].double().norm(dim=-1).clamp_min(1e-12)
        i32 = 1.0 / cand[..., :d].norm(dim=-1).clamp_min(1e-12)
        _note("mrl inv_norm", ref64.assert_f32_close(inv[k].cpu(), i64, i32, what=what + " inv_norm"))
    for mode in ("none", "random"):
        m = _mask(mode, B, N)
        got = torch.stack([hip.mrr_rank(s[k], _dev(m)) for k in range(len(dims))]).cpu()
        assert torch.equal(got.to(torch.int64), mrl_ref.ranks(s.cpu(), m)), f"ranks {name} B{B} N{N} {mode}"
    s2, inv2 = hip.mrl_scores(_dev(user), _dev(pos), _dev(neg), dims)
    assert torch.equal(_bits(s), _bits(s2)) and torch.equal(_bits(inv), _bits(inv2)), "two calls, two results"


@pytest.mark.parametrize("name,B,N", CASES)
def test_mrl_infonce_float64(name, B, N):
    """plane_loss, loss and d_user under all-ones weights and under (0.5, 0, 2, ..), every mask kind; need_grad=False: same loss bits"""
    dims = DIMS[name]
    K, D = len(dims), dims[-1]
    gscale = 0.25 if B == 3 else 1.0
    user, pos, neg = _inputs(B, N, D, seed=9)
    u, p_, n_ = _dev(user), _dev(pos), _dev(neg)
    unorm = torch.stack([user[:, :d].double().norm(dim=-1) for d in dims])          # [K, B]
    tau = _tau(dims)
    for mode in (MASKS if N > 0 else ("none",)):
        mask = _mask(mode, B, N)
        pl64, g64 = mrl_ref.plane_terms(user, pos, neg, mask, dims, tau, gscale)
        pl32, g32 = mrl_ref.plane_terms(user, pos, neg, mask, dims, tau, gscale, dtype=F32)
        dead = torch.ones(B, dtype=torch.bool) if N == 0 else (torch.zeros(B, dtype=torch.bool) if mask is None else ~mask.any(1))
        for weights in _weights(K):
            what = f"mrl_infonce {name} B{B} N{N} {mode} tau{tau:g} w{weights}"
            loss, plane, du, s, inv = hip.mrl_infonce(u, p_, n_, _dev(mask), dims, weights, tau, gscale)
            loss_ng, plane_ng, du_ng, _, _ = hip.mrl_infonce(u, p_, n_, _dev(mask), dims, weights, tau, gscale, need_grad=False)
            assert du_ng is None and torch.equal(_bits(loss_ng), _bits(loss)) and torch.equal(_bits(plane_ng), _bits(plane)), \
                f"{what}: need_grad=False changed the loss"
            l64, du64 = mrl_ref.combine(pl64, g64, weights)
            l32, du32 = mrl_ref.combine(pl32, g32, weights)
            for k in range(K):
                _note("mrl plane_loss", ref64.assert_f32_close(plane[k].cpu().reshape(()), pl64[k], pl32[k], scale=abs(float(pl64[k])) + 1.0,
                                                               what=f"{what} plane_loss[{k}]"))
            _note("mrl loss", ref64.assert_f32_close(loss.cpu().reshape(()), l64, l32, scale=abs(float(l64)) + 1.0, what=what + " loss"))
            if (~dead).any():
                _note("mrl d_user", ref64.assert_f32_close(du.cpu()[~dead], du64[~dead], du32[~dead], what=what + " d_user"))
            if dead.any():
                lam = torch.tensor(weights, dtype=F64)[:, None]
                bound = (lam * 2.0 ** -22 * gscale / (B * unorm[:, dead] * tau * tau)).sum(0)
                err = du.cpu().double()[dead].abs().amax(-1)
                assert torch.isfinite(err).all() and (err <= bound).all(), \
                    f"{what}: d_user of a sample without valid negatives: {float((err / bound).max()):.3f} x the bound"
                assert float(du64[dead].abs().max()) < 1e-12
                _note("mrl d_user (no valid negative)", float((err / bound).max()))
        if tau != TAU:                                       # the product's temperature: the losses of the same planes
            pl64, _ = mrl_ref.plane_terms(user, pos, neg, mask, dims, TAU, gscale)
            pl32, _ = mrl_ref.plane_terms(user, pos, neg, mask, dims, TAU, gscale, dtype=F32)
            for weights in _weights(K):
                what = f"mrl_infonce {name} B{B} N{N} {mode} tau{TAU:g} w{weights}"
                loss, plane, _, _, _ = hip.mrl_infonce(u, p_, n_, _dev(mask), dims, weights, TAU, gscale, need_grad=False)
                lam64, lam32 = torch.tensor(weights, dtype=F64), torch.tensor(weights, dtype=F32)
                l64, l32 = (lam64 * pl64).sum(), (lam32 * pl32).sum()
                for k in range(K):
                    _note("mrl plane_loss", ref64.assert_f32_close(plane[k].cpu().reshape(()), pl64[k], pl32[k], scale=abs(float(pl64[k])) + 1.0,
                                                                   what=f"{what} plane_loss[{k}]"))
                _note("mrl loss", ref64.assert_f32_close(loss.cpu().reshape(()), l64, l32, scale=abs(float(l64)) + 1.0, what=what + " loss"))
        if mode == "all_invalid" or N == 0:
            assert float(pl64.abs().max()) < 1e-12


def _sliced(user, pos, neg, mask, d, tau, gscale):
    """the head's own kernels on the contiguous slices [..., :d]"""
    us, ps, ns = user[:, :d].contiguous(), pos[:, :d].contiguous(), neg[..., :d].contiguous()
    s, inv = hip.cosine_scores(us, ps, ns)
    loss, du = hip.infonce_fwd_bwd(us, ps, ns, mask, s, inv, temperature=tau, grad_scale=gscale)
    return s, inv, loss, du


@pytest.mark.parametrize("name,B,N,mode", [(n, 5, 37, "random") for n in DIMS] + [("sweep", 65, 300, "none"), ("eight", 3, 14, "one"),
                                                                                   ("odd", 2, 1, "all_invalid"), ("tiny", 2, 10000, "random"),
                                                                                   ("single", 1, 0, "none")])
def test_mrl_planes_equal_the_sliced_kernels_bit_for_bit(name, B, N, mode):
    dims = DIMS[name]
    K, D = len(dims), dims[-1]
    gscale = 0.5
    user, pos, neg = (_dev(t) for t in _inputs(B, N, D, seed=13))
    mask = _dev(_mask(mode, B, N))
    s, inv = hip.mrl_scores(user, pos, neg, dims)
    loss, plane, du, s2, inv2 = hip.mrl_infonce(user, pos, neg, mask, dims, None, TAU, gscale)
    assert torch.equal(_bits(s), _bits(s2)) and torch.equal(_bits(inv), _bits(inv2)), "ur_mrl_infonce's scores are ur_mrl_scores'"
    for k, d in enumerate(dims):
        sk, ik, lk, duk = _sliced(user, pos, neg, mask, d, TAU, gscale)
        assert torch.equal(_bits(s[k]), _bits(sk)), f"{name}: scores of plane {k} (d {d})"
        assert torch.equal(_bits(inv[k]), _bits(ik)), f"{name}: inverse norms of plane {k} (d {d})"
        assert torch.equal(_bits(plane[k:k + 1]), _bits(lk)), f"{name}: plane_loss[{k}]"
        onehot = tuple(1.0 if q == k else 0.0 for q in range(K))
        l1, p1, du1, _, _ = hip.mrl_infonce(user, pos, neg, mask, dims, onehot, TAU, gscale)
        assert torch.equal(_bits(l1), _bits(lk)), f"{name}: loss under the one-hot weights of plane {k}"
        assert torch.equal(_bits(p1), _bits(plane)), "plane_loss does not depend on the weights"
        assert torch.equal(du1[:, :d], duk), f"{name}: d_user[:, :{d}] under the one-hot weights of plane {k}"
        assert not bool(du1[:, d:].any()), f"{name}: d_user[:, {d}:] under the one-hot weights of plane {k} is not zero"
    if K == 1:                                           # dims = [D], weights = [1]: the existing pair outright
        sk, ik, lk, duk = _sliced(user, pos, neg, mask, D, TAU, gscale)
        assert torch.equal(_bits(loss), _bits(lk)) and torch.equal(_bits(du), _bits(duk)) and torch.equal(_bits(s[0]), _bits(sk))


# ---- determinism and buffers -------------------------------------------------------------------------------------------------------------
GUARD = 64                           # floats on either side of a buffer
CANARY = -1234.5


def _guarded(n):
    """(the whole tensor, the view of n floats in its middle): 256-byte guards filled with a value nothing computes"""
    whole = torch.full((n + 2 * GUARD,), CANARY, dtype=F32, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def _intact(whole, n):
    return bool((whole[:GUARD] == CANARY).all()) and bool((whole[GUARD + n:] == CANARY).all())


def _raw_call(user, pos, neg, mask, dims, weights, bufs, wsb):
    B, D = user.shape
    K = len(dims)
    a = _lib.MrlInfoNCE()
    a.user, a.pos, a.neg, a.neg_mask = user.data_ptr(), pos.data_ptr(), neg.data_ptr(), None if mask is None else mask.data_ptr()
    a.B, a.N, a.D, a.K = B, neg.shape[1], D, K
    a.dims[:K] = dims
    a.weights[:K] = weights
    a.temperature, a.grad_scale = TAU, 1.0
    for name, (_, view) in bufs.items():
        setattr(a, name, view.data_ptr())
    a.workspace_bytes = wsb
    return _lib.load().ur_mrl_infonce(ctypes.byref(a), hip._stream())


@pytest.mark.parametrize("name,B,N", [("odd", 3, 14), ("eight", 5, 37)])
def test_two_calls_same_bits_and_nothing_outside_the_buffers(name, B, N):
    dims = DIMS[name]
    K, D = len(dims), dims[-1]
    weights = _weights(K)[1]
    user, pos, neg = (_dev(t) for t in _inputs(B, N, D, seed=17))
    mask = _dev(_mask("random", B, N))
    lib = _lib.load()
    q = _lib.MrlInfoNCE()
    q.B, q.N, q.D, q.K, q.temperature = B, N, D, K, TAU
    q.dims[:K] = dims
    q.weights[:K] = weights
    assert lib.ur_mrl_infonce(ctypes.byref(q), None) == 0
    need = q.workspace_bytes
    assert need == 4 * (K * ((B + 3) // 4 * 4) + (K * B * (N + 1) + 3) // 4 * 4 + B * 16 * sum(dims))
    sizes = {"scores": K * B * (N + 1), "cand_inv_norm": K * B * (N + 1), "plane_loss": K, "loss": 1, "d_user": B * D, "workspace": need // 4}

    def run(wsb):
        bufs = {k: _guarded(n) for k, n in sizes.items()}
        rc = _raw_call(user, pos, neg, mask, dims, weights, bufs, wsb)
        torch.cuda.synchronize()
        return rc, bufs

    rc, a = run(need)
    assert rc == 0, lib.ur_last_error()
    rc, b = run(need)
    assert rc == 0
    for k, n in sizes.items():
        assert _intact(a[k][0], n), f"{k}: written outside the buffer"
        if k != "workspace":
            assert torch.equal(_bits(a[k][1]), _bits(b[k][1])), f"{k}: two calls, two results"
            assert bool((a[k][1] != CANARY).all()), f"{k}: not every element was written"
    # the wrapper gives those bits too
    loss, plane, du, s, inv = hip.mrl_infonce(user, pos, neg, mask, dims, weights, TAU, 1.0)
    assert torch.equal(_bits(loss), _bits(a["loss"][1])) and torch.equal(_bits(du.flatten()), _bits(a["d_user"][1]))
    assert torch.equal(_bits(s.flatten()), _bits(a["scores"][1])) and torch.equal(_bits(plane), _bits(a["plane_loss"][1]))
    # a workspace one byte short: refused, nothing written anywhere
    rc, c = run(need - 1)
    assert rc < 0 and b"workspace" in lib.ur_last_error()
    for k in sizes:
        assert bool((c[k][0] == CANARY).all()), f"{k}: written by a refused call"
    # ur_mrl_scores: the same guards
    sa = _lib.MrlScores()
    sa.user, sa.pos, sa.neg = user.data_ptr(), pos.data_ptr(), neg.data_ptr()
    sa.B, sa.N, sa.D, sa.K = B, N, D, K
    sa.dims[:K] = dims
    sw, sv = _guarded(sizes["scores"])
    iw, iv = _guarded(sizes["scores"])
    sa.scores, sa.cand_inv_norm = sv.data_ptr(), iv.data_ptr()
    assert lib.ur_mrl_scores(ctypes.byref(sa), hip._stream()) == 0
    torch.cuda.synchronize()
    assert _intact(sw, sizes["scores"]) and _intact(iw, sizes["scores"])
    assert torch.equal(_bits(sv), _bits(a["scores"][1])) and torch.equal(_bits(iv), _bits(a["cand_inv_norm"][1]))
