"""float64 restatement of ur_catalog_softmax (include/unirec_hip_loss.h), taken from the f32 (or bf16, widened exactly) inputs.

    s_bn = (u_b . c_n) * iu_b * ic_n,  iu = 1 / max(|u_b|, 1e-12), ic likewise
    z_bn = s_bn / tau over the rows n that user b keeps: every row except those of exclude[b] other than g_b (negative entries ignored)
    lse_b = log sum_n exp(z_bn);  row_b = -z_b,g + lse_b;  loss = mean_b row_b
    w_bn = (exp(z_bn - lse_b) - [n == g_b]) / tau (0 for a dropped row);  G_b = sum_n w_bn ic_n c_n;  t_b = sum_n w_bn s_bn
    d_user_b = grad_scale / B * iu_b * (G_b - u_b iu_b t_b)

Everything is computed on the CPU in float64; the only f32 numbers are the inputs themselves (tau and grad_scale are rounded to f32
first, as the C ABI passes them)."""
import numpy as np
import torch

F64 = torch.float64


def keep_mask(B, N, gt, exclude):
    """bool [B,N]: the rows user b sums over.  exclude: None, or per-user iterables / an int tensor [B,E] (negative = empty slot)."""
    keep = torch.ones((B, N), dtype=torch.bool)
    if exclude is not None:
        for b in range(B):
            for n in (exclude[b].tolist() if isinstance(exclude[b], torch.Tensor) else exclude[b]):
                n = int(n)
                if 0 <= n < N and n != int(gt[b]):
                    keep[b, n] = False
    return keep


def f32(x):
    return float(np.float32(x))


def catalog_softmax_ref(user, catalog, gt, temperature, exclude=None, grad_scale=1.0):
    """-> dict(loss [], row_loss [B], lse [B], d_user [B,D], scores [B,N], keep [B,N]), all float64 CPU tensors."""
    u = user.detach().cpu().to(F64)
    c = catalog.detach().cpu().to(F64)            # (bf16 -> f64 is exact)
    gt = torch.as_tensor(gt).cpu().to(torch.int64)
    B, N = u.shape[0], c.shape[0]
    tau, gs = f32(temperature), f32(grad_scale)
    iu = 1.0 / u.norm(dim=1).clamp_min(1e-12)
    ic = 1.0 / c.norm(dim=1).clamp_min(1e-12)
    s = (u @ c.T) * iu[:, None] * ic[None, :]
    keep = keep_mask(B, N, gt, exclude)
    z = torch.where(keep, s / tau, torch.full_like(s, -float("inf")))
    lse = torch.logsumexp(z, dim=1)
    zg = z.gather(1, gt[:, None])[:, 0]
    row = lse - zg
    w = torch.exp(z - lse[:, None])
    w[torch.arange(B), gt] -= 1.0
    w = w / tau
    G = (w * ic[None, :]) @ c
    t = (w * torch.where(keep, s, torch.zeros_like(s))).sum(dim=1)
    du = gs / B * iu[:, None] * (G - u * (iu * t)[:, None])
    return {"loss": row.mean(), "row_loss": row, "lse": lse, "d_user": du, "scores": s, "keep": keep}


def autograd_ref(user, catalog, gt, temperature, exclude=None, grad_scale=1.0):
    """The same loss by float64 torch autograd (F.normalize, masked logits, logsumexp): -> (loss, d_user)."""
    u = user.detach().cpu().to(F64).requires_grad_(True)
    c = catalog.detach().cpu().to(F64)
    gt = torch.as_tensor(gt).cpu().to(torch.int64)
    B, N = u.shape[0], c.shape[0]
    s = torch.nn.functional.normalize(u, dim=1, eps=1e-12) @ torch.nn.functional.normalize(c, dim=1, eps=1e-12).T
    z = (s / f32(temperature)).masked_fill(~keep_mask(B, N, gt, exclude), -float("inf"))
    loss = (torch.logsumexp(z, dim=1) - z.gather(1, gt[:, None])[:, 0]).mean()
    (loss * f32(grad_scale)).backward()
    return loss.detach(), u.grad
