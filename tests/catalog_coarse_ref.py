"""The float64 restatement of the two-stage retrieval family (include/unirec_hip_coarse.h), on the host, for the CPU and the GPU tests.

    u~    = user rounded to bf16 (nearest even), widened to float64
    s64   = (u~ . c) / (max(|u~|, 1e-12) * max(|c|, 1e-12))       exact products of bf16 values, float64 sums
    list  = the kept items in the total order (score descending, index ascending), cut to K, padded with (-1, -inf)
    rank  = 1 + #{kept n != g : s_n > s_g}

`kept`: every n not in the user's exclusion row, and the user's own ground truth always (select mode's rule).  The exact scores of the
re-rank are the same expression on the unrounded user.  Nothing here runs on a device or touches the library."""
import numpy as np
import torch

F64 = torch.float64


def round_bf16(x):
    """f32 -> the nearest bf16 (ties to even), as float64"""
    return torch.as_tensor(x).detach().cpu().to(torch.float32).to(torch.bfloat16).to(F64)


def _cos(u, c):
    iu = 1.0 / u.norm(dim=1).clamp_min(1e-12)
    ic = 1.0 / c.norm(dim=1).clamp_min(1e-12)
    return (u @ c.T) * iu[:, None] * ic[None, :]


def coarse_scores(user, catalog):
    """float64 [B,N]: the cosine of the bf16-rounded user with every catalogue row (the catalogue's own stored values)"""
    return _cos(round_bf16(user), torch.as_tensor(catalog).detach().cpu().to(F64))


def exact_scores(user, catalog):
    """float64 [B,N]: the cosine of the f32 user with every catalogue row"""
    return _cos(torch.as_tensor(user).detach().cpu().to(F64), torch.as_tensor(catalog).detach().cpu().to(F64))


def keep_mask(B, N, gt=None, exclude=None):
    """bool [B,N]: exclude = per-user iterables (or a [B,E] tensor) of indices, entries outside [0,N) ignored; gt[b] is always kept"""
    keep = np.ones((B, N), dtype=bool)
    if exclude is not None:
        for b in range(B):
            for n in np.asarray(exclude[b]).reshape(-1):
                n = int(n)
                if 0 <= n < N and (gt is None or n != int(gt[b])):
                    keep[b, n] = False
    return keep


def order(scores_row, index_row):
    """positions of a row's pairs in the total order: score descending, index ascending"""
    return np.lexsort((np.asarray(index_row), -np.asarray(scores_row, dtype=np.float64)))


def select(scores, K, gt=None, exclude=None):
    """(index int32 [B,K], score float64 [B,K], rank int32 [B] or None) of float64 scores [B,N] under the list and rank rules"""
    S = np.asarray(scores, dtype=np.float64)
    B, N = S.shape
    keep = keep_mask(B, N, gt, exclude)
    idx = np.full((B, K), -1, dtype=np.int32)
    val = np.full((B, K), -np.inf, dtype=np.float64)
    rank = None if gt is None else np.zeros((B,), dtype=np.int32)
    for b in range(B):
        cand = np.nonzero(keep[b])[0]
        o = cand[order(S[b, cand], cand)][:K]
        idx[b, :len(o)] = o
        val[b, :len(o)] = S[b, o]
        if gt is not None:
            g = int(gt[b])
            others = cand[cand != g]
            rank[b] = 1 + int((S[b, others] > S[b, g]).sum())
    return idx, val, rank


def rerank(scores, index, k):
    """(index int32 [B,k], score float64 [B,k]): the pairs (b, index[b][j]) under the total order, entries outside [0,N) as empty slots
    at the tail (-1, -inf); scores float64 [B,N]"""
    S = np.asarray(scores, dtype=np.float64)
    index = np.asarray(index)
    B, N = S.shape
    idx = np.full((B, k), -1, dtype=np.int32)
    val = np.full((B, k), -np.inf, dtype=np.float64)
    for b in range(B):
        row = index[b][(index[b] >= 0) & (index[b] < N)]
        o = row[order(S[b, row], row)][:k]
        idx[b, :len(o)] = o
        val[b, :len(o)] = S[b, o]
    return idx, val
