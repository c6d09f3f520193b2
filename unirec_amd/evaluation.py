"""Prompt construction and ranking evaluation next to the joint head.

  * ``construct_input_text``      training/train_item_individual_token_joint.py:579-592 (history prompt with the
                                  ``<|history_item_i_query_j|>`` specials the model overwrites with Q-Former tokens)
  * ``special_token_positions``   :160-171 (where each special sits in ``input_ids``; the product path finds them inside
                                  ``ur_embed_inject_fwd``, this table is the host-visible form for inspection / tests)
  * ``MRREvaluator``              :361-419 (per-user candidate lists: positive first, cosine scores, rank of the positive)
  * ``CatalogEvaluator``          the same metric with pool = ALL items: one shared catalogue [N,D] resident in HBM,
                                  ``ur_catalog_scores`` + ``ur_rank_of_index`` + ``ur_topk``; no host sync per user.
                                  ``retrieve`` is the catalogue-scale form: the scores are streamed in chunks through
                                  ``ur_catalog_scores``' select mode (top-K, rank and a per-user seen-item filter; no [B,N] tensor).
                                  The catalogue may stay bf16 (``dtype=torch.bfloat16``): ``retrieve`` reads it as it is.
  * ``Fp8CatalogEvaluator``       the catalogue at one byte per element (OCP e4m3fn codes and a power-of-two scale per row,
                                  include/unirec_fp8.h): a shortlist pass over the codes and an exact re-rank against the quantised rows.
Tie rule: the positive's rank is 1 + #{strictly greater}; top-K lists the lowest index first.
"""
import numpy as np
import torch

from . import hip

F32 = torch.float32


def construct_input_text(history, item_dict, num_history_items, num_query_tokens_per_item):
    """:579-592 verbatim semantics: numbered titles (truncated to 77 chars + '...') followed by the item's specials;
    empty slots contribute their specials only."""
    history_parts = []
    for i in range(num_history_items):
        query_token_part = "".join(f" <|history_item_{i}_query_{j}|>" for j in range(num_query_tokens_per_item))
        if i < len(history):
            item_id = history[i]
            title = item_dict.get(item_id, {}).get("title", f"Item {item_id}")
            if len(title) > 80:
                title = title[:77] + "..."
            history_parts.append(f"{i + 1}. {title}{query_token_part}")
        else:
            history_parts.append(query_token_part.strip())
    return f"I have bought these items in the past: {', '.join(history_parts)}"


def special_token_positions(input_ids, first_special_id, num_specials):
    """[B, num_specials] int64: position of special id first_special_id + t in each row, -1 when the tokenizer
    truncated it away (:166-171 overwrite only the specials that are present).  Device-side (no per-sample nonzero)."""
    ids = input_ids.to(torch.int64)
    B, S = ids.shape
    rel = ids - int(first_special_id)
    hit = (rel >= 0) & (rel < num_specials)
    pos = torch.full((B, num_specials), -1, dtype=torch.int64, device=ids.device)
    b_idx, s_idx = hit.nonzero(as_tuple=True)
    pos[b_idx, rel[b_idx, s_idx]] = s_idx
    return pos


class MRREvaluator:
    """:361-419.  ``model(input_ids=..., attention_mask=..., history_field_embeddings=..., history_attention_mask=...)``
    -> user embeddings [B,D]; candidates per user: one positive + a ragged list of negatives."""

    def __init__(self, model, tokenizer=None, validation_dataset=None):
        self.model, self.tokenizer, self.validation_dataset = model, tokenizer, validation_dataset

    def _validation_collate_fn(self, batch):
        """:380-395 (negatives stay a list: they are ragged)."""
        st = lambda k: torch.stack([item[k] for item in batch])
        return {"input_ids": st("input_ids"), "attention_mask": st("attention_mask"),
                "history_field_embeddings": st("history_field_embeddings"), "history_attention_mask": st("history_attention_mask"),
                "positive_item_embeddings": st("positive_item_embedding"),
                "negative_item_embeddings": [item["negative_item_embeddings"] for item in batch]}

    @staticmethod
    def ranks_from_embeddings(user_embeddings, positive_item_embeddings, negative_item_embeddings, dims=None):
        """:403-419 on device: ragged negatives are padded and masked; returns int32 ranks [B].
        dims (ascending multiples of 4, the last one D): int32 ranks [K,B] on the first dims[k] components of every embedding, the
        candidates read once (``hip.mrl_scores``)."""
        if dims is not None:
            dims = hip.mrl_dims(dims, "dims", user_embeddings.shape[-1])
        u = user_embeddings.detach().to(F32).contiguous()
        dev = u.device
        p = torch.as_tensor(positive_item_embeddings).to(dev, F32).contiguous()
        negs = [torch.as_tensor(n).to(dev, F32).reshape(-1, u.shape[1]) for n in negative_item_embeddings]
        nmax = max([n.shape[0] for n in negs] + [1])
        neg = torch.zeros((len(negs), nmax, u.shape[1]), dtype=F32, device=dev)
        mask = torch.zeros((len(negs), nmax), dtype=torch.uint8, device=dev)
        for b, n in enumerate(negs):
            neg[b, :n.shape[0]] = n
            mask[b, :n.shape[0]] = 1
        if dims is not None:
            scores, _ = hip.mrl_scores(u, p, neg, dims)
            return torch.stack([hip.mrr_rank(scores[k], mask) for k in range(len(dims))])
        scores, _ = hip.cosine_scores(u, p, neg)
        return hip.mrr_rank(scores, mask)

    def _compute_batch_mrr(self, batch):
        dev = next(self.model.parameters()).device
        user = self.model(input_ids=batch["input_ids"].to(dev), attention_mask=batch["attention_mask"].to(dev),
                          history_field_embeddings=batch["history_field_embeddings"].to(dev),
                          history_attention_mask=batch["history_attention_mask"].to(dev))
        rank = self.ranks_from_embeddings(user, batch["positive_item_embeddings"], batch["negative_item_embeddings"])
        return (1.0 / rank.to(torch.float64)).cpu().tolist()

    def evaluate_mrr(self, batch_size: int = 32) -> float:
        """:367-378."""
        self.model.eval()
        scores = []
        loader = torch.utils.data.DataLoader(self.validation_dataset, batch_size=batch_size, shuffle=False,
                                             collate_fn=self._validation_collate_fn)
        with torch.no_grad():
            for batch in loader:
                scores.extend(self._compute_batch_mrr(batch))
        return float(np.mean(scores))


def pack_exclude(exclude, num_users=None):
    """Per-user exclusion lists -> the sorted int64 [B,E] tensor ``hip.catalog_select`` takes, or None when nothing is excluded.
    ``exclude`` is a ragged list of per-user index iterables, or an int64 [B,E] tensor padded with negative entries.  Rows come out
    ascending and padded with -1 in front (empty slots sort first); duplicates are kept.  Pure: stays on the input's device (CPU
    for lists)."""
    if exclude is None:
        return None
    if isinstance(exclude, torch.Tensor):
        t = exclude.to(torch.int64)
        if t.dim() != 2:
            raise ValueError(f"pack_exclude: a tensor must be [B,E], got {tuple(t.shape)}")
    else:
        rows = [sorted(int(i) for i in r) for r in exclude]
        E = max([len(r) for r in rows] + [0])
        t = torch.full((len(rows), E), -1, dtype=torch.int64)
        for b, r in enumerate(rows):
            if r:
                t[b, E - len(r):] = torch.tensor(r, dtype=torch.int64)
    if num_users is not None and t.shape[0] != num_users:
        raise ValueError(f"pack_exclude: {t.shape[0]} rows for {num_users} users")
    if t.numel() == 0 or not bool((t >= 0).any()):
        return None
    t = torch.where(t < 0, torch.full_like(t, -1), t)
    return torch.sort(t, dim=1).values.contiguous()


def ranking_metrics(rank, ks):
    """Rank-based metrics with ONE relevant item per user, in float64 on rank's device: a [1 + 2 len(ks)] tensor
    (mrr, hit@k for k in ks, ndcg@k for k in ks); hit@k = mean(rank <= k), ndcg@k = mean(1 / log2(1 + rank) if rank <= k else 0).
    Pure (no host read): the caller fetches all of them at once."""
    r = rank.to(torch.float64)
    gain = 1.0 / torch.log2(1.0 + r)
    zero = torch.zeros_like(r)
    out = [(1.0 / r).mean()]
    out += [(r <= k).to(torch.float64).mean() for k in ks]
    out += [torch.where(r <= k, gain, zero).mean() for k in ks]
    return torch.stack(out)


class CatalogEvaluator:
    """MRR / hit@K / top-K of user embeddings against the whole item catalogue (pool = all items)."""

    def __init__(self, catalog, item_ids=None, device="cuda", dtype=F32):
        """dtype=torch.bfloat16 keeps the catalogue in bf16 (f32 input is rounded to nearest even; no f32 copy is kept or made):
        retrieve() then gives what it gives on that catalogue's .float(), bit for bit; evaluate() / scores() need an f32 catalogue."""
        if dtype not in (F32, torch.bfloat16):
            raise ValueError(f"CatalogEvaluator: dtype must be torch.float32 or torch.bfloat16, got {dtype}")
        self.catalog = torch.as_tensor(catalog).to(device, dtype).contiguous()    # [N,D], stays in HBM
        self.item_ids = None if item_ids is None else [str(i) for i in item_ids]
        self._inv = None                                                          # catalogue 1/||c||, computed once
        self._prefix_inv = {}                                                     # prefix width -> 1/||c[:width]|| [N] (retrieve_funnel)

    def truncated(self, dim):
        """A new evaluator over the first `dim` components of every catalogue row, as a contiguous [N, dim] copy of the same dtype
        (dim / D of the bytes retrieve() streams); its norms are computed by its first call.  For a Matryoshka-trained model:
        ``ev.truncated(256).retrieve(user[:, :256], k)``.  dim: a positive multiple of 4, at most D."""
        D = self.catalog.shape[1]
        if isinstance(dim, bool) or not isinstance(dim, int) or dim <= 0 or dim % 4 or dim > D:
            raise ValueError(f"CatalogEvaluator.truncated: dim must be a positive multiple of 4 and at most D = {D}, got {dim!r}")
        return CatalogEvaluator(self.catalog[:, :dim], item_ids=self.item_ids, device=self.catalog.device, dtype=self.catalog.dtype)

    def quantized(self, block_rows=None):
        """An ``Fp8CatalogEvaluator`` over this catalogue's rows, quantised on its device a block of rows at a time: one byte per
        element beside this evaluator's own tensor, which stays as it is."""
        return Fp8CatalogEvaluator(self.catalog, item_ids=self.item_ids, device=self.catalog.device, block_rows=block_rows)

    def scores(self, user_embeddings):
        if self.catalog.dtype != F32:
            raise ValueError("CatalogEvaluator: scores() / evaluate() hold a [B,N] tensor and take an f32 catalogue; use retrieve() on a bf16 one")
        s, self._inv = hip.catalog_scores(user_embeddings.detach().to(self.catalog.device, F32).contiguous(), self.catalog, self._inv)
        return s

    def evaluate(self, user_embeddings, gt_index, k=10):
        """-> dict(rank int32 [B], mrr float, hit_at_k float, topk_index int32 [B,k], topk_score f32 [B,k])."""
        s = self.scores(user_embeddings)
        gt = torch.as_tensor(gt_index).to(s.device, torch.int64)
        rank = hip.rank_of_index(s, gt)
        idx, val = hip.topk(s, k)
        return {"rank": rank, "mrr": float((1.0 / rank.to(torch.float64)).mean().item()),
                "hit_at_k": float((rank <= k).to(torch.float64).mean().item()), "topk_index": idx, "topk_score": val}

    def retrieve(self, user_embeddings, k=10, gt_index=None, exclude=None, ks=None, chunk_rows=None, scorer=None, shortlist=None):
        """Catalogue-scale retrieval: the scores are streamed in chunks and never held as [B,N].
        exclude: items each user has already seen (ragged lists or an int64 [B,E] tensor padded with -1, see pack_exclude); they leave
        the lists and the ranks, except a user's own gt_index.
        -> dict(topk_index int32 [B,k], topk_score f32 [B,k]); with gt_index also rank int32 [B], mrr, and hit_at / ndcg_at:
        dicts keyed by each K of ks (default (k,); any K, the metrics need only the rank).  Same scores, tie rule and rank rule as
        evaluate().  k: an int in [1, 1024]; up to 128 the lists come from ``hip.catalog_select``, longer ones from
        ``hip.catalog_deep_select`` (the same scores, order and rank; a selection kernel built for long lists).
        scorer: None (the library's choice), "vector" or "mfma": which kernel scores the chunks; the results are the same bits.
        shortlist: None (the path above), or an int in [k, 128] for the two-stage path on a bf16 catalogue: ``hip.catalog_coarse_select``
        picks `shortlist` items per user under the coarse bf16-MFMA scores and ``hip.catalog_rerank`` scores those exactly and returns the
        best k.  topk_score then holds the exact scorer's bits for the returned items and the order is the exact one; the list equals the
        exact list wherever the exact k-th and (shortlist + 1)-th scores lie further apart than the coarse error (2^-7 covers it).  rank
        and the metrics come from the COARSE scores and the dict carries rank_is_coarse=True.  `scorer` must stay None."""
        hip.catalog_scorer_id(scorer)
        if shortlist is None and (isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= hip.CATALOG_DEEP_TOPK_MAX):
            raise ValueError(f"retrieve: k must be an int in [1, {hip.CATALOG_DEEP_TOPK_MAX}], got {k!r}")
        if shortlist is not None:
            if scorer is not None:
                raise ValueError(f"retrieve: scorer={scorer!r} chooses between the exact scorers; with shortlist the coarse pass has one kernel, "
                                 "leave scorer=None")
            if self.catalog.dtype != torch.bfloat16:
                raise ValueError("retrieve: shortlist needs a bf16 catalogue (CatalogEvaluator(dtype=torch.bfloat16)), this one is "
                                 f"{self.catalog.dtype}")
            if isinstance(shortlist, bool) or not isinstance(shortlist, int) or isinstance(k, bool) or not isinstance(k, int) or \
                    not 1 <= k <= shortlist <= hip.CATALOG_TOPK_MAX:
                raise ValueError(f"retrieve: shortlist must be an int in [k, {hip.CATALOG_TOPK_MAX}] (k = {k!r}), got {shortlist!r}")
        u = user_embeddings.detach().to(self.catalog.device, F32).contiguous()
        ex = pack_exclude(exclude, u.shape[0])
        if ex is not None:
            ex = ex.to(u.device)
        gt = None if gt_index is None else torch.as_tensor(gt_index).to(u.device, torch.int64)
        if shortlist is not None:
            short, _, rank, self._inv = hip.catalog_coarse_select(u, self.catalog, shortlist, self._inv, gt_index=gt, exclude=ex,
                                                                  chunk_rows=chunk_rows)
            idx, val, _ = hip.catalog_rerank(u, self.catalog, short, k, self._inv)
        elif k <= hip.CATALOG_TOPK_MAX:
            idx, val, rank, self._inv = hip.catalog_select(u, self.catalog, k, self._inv, gt_index=gt, exclude=ex, chunk_rows=chunk_rows,
                                                            scorer=scorer)
        else:
            idx, val, rank, self._inv = hip.catalog_deep_select(u, self.catalog, k, self._inv, gt_index=gt, exclude=ex,
                                                                 chunk_rows=chunk_rows, scorer=scorer)
        out = {"topk_index": idx, "topk_score": val}
        if rank is not None:
            ks = (k,) if ks is None else tuple(int(x) for x in ks)
            m = ranking_metrics(rank, ks).cpu().tolist()                                 # the one host read
            out.update(rank=rank, mrr=m[0], hit_at=dict(zip(ks, m[1:1 + len(ks)])), ndcg_at=dict(zip(ks, m[1 + len(ks):])))
            if shortlist is not None:
                out["rank_is_coarse"] = True
        return out

    def retrieve_two_stage(self, user_embeddings, k=10, shortlist=None, gt_index=None, exclude=None, ks=None, chunk_rows=None):
        """The two-stage path of ``retrieve(k, shortlist=S)`` with shortlists of up to 1024 items, on a bf16 catalogue:
        ``hip.catalog_coarse_deep_select`` picks `shortlist` items per user under the coarse bf16-MFMA scores (the scorer of
        ``hip.catalog_coarse_select``, the selection kernels of ``hip.catalog_deep_select``) and ``hip.catalog_deep_rerank`` scores those
        exactly and returns the best k -- one path for the whole range 1 <= k <= shortlist <= 1024.
        -> the dict of ``retrieve(k, shortlist=S)``: topk_index int32 [B,k], topk_score f32 [B,k] with the exact scorer's bits in the
        exact order; with gt_index also rank / mrr / hit_at / ndcg_at from the COARSE scores and rank_is_coarse=True.  exclude, ks and
        chunk_rows as in retrieve().  For shortlist <= 128 every tensor equals ``retrieve(k, shortlist=shortlist)``'s bit for bit.  The
        list equals the exact ``retrieve(k)`` wherever the exact k-th and (shortlist + 1)-th scores lie further apart than the coarse
        error (2^-7 covers it).
        shortlist=None means min(1024, max(128, 2 k)): a default that leaves the re-rank twice the room it returns, NOT a tuned value --
        choose it from the recall the catalogue needs."""
        if self.catalog.dtype != torch.bfloat16:
            raise ValueError("retrieve: shortlist needs a bf16 catalogue (CatalogEvaluator(dtype=torch.bfloat16)), this one is "
                             f"{self.catalog.dtype}")
        top = hip.CATALOG_DEEP_TOPK_MAX
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= top:
            raise ValueError(f"retrieve_two_stage: k must be an int in [1, {top}], got {k!r}")
        if shortlist is None:
            shortlist = min(top, max(hip.CATALOG_TOPK_MAX, 2 * k))
        if isinstance(shortlist, bool) or not isinstance(shortlist, int) or not k <= shortlist <= top:
            raise ValueError(f"retrieve_two_stage: shortlist must be an int in [k, {top}] (k = {k!r}), got {shortlist!r}")
        u = user_embeddings.detach().to(self.catalog.device, F32).contiguous()
        ex = pack_exclude(exclude, u.shape[0])
        if ex is not None:
            ex = ex.to(u.device)
        gt = None if gt_index is None else torch.as_tensor(gt_index).to(u.device, torch.int64)
        short, _, rank, self._inv = hip.catalog_coarse_deep_select(u, self.catalog, shortlist, self._inv, gt_index=gt, exclude=ex,
                                                                   chunk_rows=chunk_rows)
        idx, val, _ = hip.catalog_deep_rerank(u, self.catalog, short, k, self._inv)
        out = {"topk_index": idx, "topk_score": val}
        if rank is not None:
            ks = (k,) if ks is None else tuple(int(x) for x in ks)
            m = ranking_metrics(rank, ks).cpu().tolist()                                 # the one host read
            out.update(rank=rank, mrr=m[0], hit_at=dict(zip(ks, m[1:1 + len(ks)])), ndcg_at=dict(zip(ks, m[1 + len(ks):])),
                       rank_is_coarse=True)
        return out

    def _prefix_norms(self, dims):
        """{d: the [N] inverse norms of the catalogue's first d components} for d in dims: one ``hip.catalog_prefix_norms`` call for the
        widths not seen before.  The plane of the full width is ``self._inv`` (the same bits), shared with the other paths."""
        D = self.catalog.shape[1]
        missing = tuple(d for d in dims if d not in self._prefix_inv and not (d == D and self._inv is not None))
        if missing:
            planes = hip.catalog_prefix_norms(self.catalog, missing)
            for d, plane in zip(missing, planes):
                if d == D:
                    self._inv = plane
                else:
                    self._prefix_inv[d] = plane
        return {d: self._inv if d == D else self._prefix_inv[d] for d in dims}

    def retrieve_funnel(self, user_embeddings, k=10, dims=None, shortlists=None, gt_index=None, exclude=None, ks=None, chunk_rows=None):
        """Funnel retrieval for a Matryoshka-trained model (``matryoshka_dims``) on a bf16 catalogue: shortlist on the narrow prefix
        dims[0], re-rank the survivors exactly on each wider prefix, the last one dims[-1].  Every stage reads its prefix of the resident
        [N,D] catalogue in place: no truncated copy exists, and one norm plane per prefix is kept.
        Stage 0: ``hip.catalog_funnel_select`` at dims[0] picks shortlists[0] items per user under the coarse bf16-MFMA scores of that
        prefix; it carries gt_index, exclude and chunk_rows.  Stage i >= 1: ``hip.catalog_funnel_rerank`` at dims[i] scores the survivors
        exactly and keeps shortlists[i]; the last stage keeps k.
        dims: 2 to 8 ints, strictly ascending multiples of 8, the last at most D.  shortlists: len(dims) - 1 ints, non-increasing, each in
        [k, 1024]; None means min(1024, max(128, 2 k)) at every stage: a default that leaves each re-rank twice the room the call
        returns, NOT a tuned value -- choose them from the recall each prefix of the model gives.  k: an int in [1, 1024].
        -> the dict of ``retrieve_two_stage``: topk_index int32 [B,k], topk_score f32 [B,k] with the exact scores at dims[-1] in the exact
        order; with gt_index also rank / mrr / hit_at / ndcg_at from the COARSE scores at dims[0], rank_is_coarse=True and
        rank_dim=dims[0].  A prefix of an embedding that was not trained for it is not a shortlist: the recall is the model's."""
        if self.catalog.dtype != torch.bfloat16:
            raise ValueError("retrieve: shortlist needs a bf16 catalogue (CatalogEvaluator(dtype=torch.bfloat16)), this one is "
                             f"{self.catalog.dtype}")
        top, D = hip.CATALOG_DEEP_TOPK_MAX, self.catalog.shape[1]
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= top:
            raise ValueError(f"retrieve_funnel: k must be an int in [1, {top}], got {k!r}")
        if dims is None:
            raise ValueError("retrieve_funnel: dims must be given, the prefix widths of the stages")
        dims = hip.mrl_dims(dims, "retrieve_funnel: dims")
        if len(dims) < 2 or any(d % 8 for d in dims) or dims[-1] > D:
            raise ValueError(f"retrieve_funnel: dims must hold 2 to {hip.MRL_MAX_DIMS} ascending multiples of 8, the last at most D = {D}, "
                             f"got {dims}")
        if shortlists is None:
            shortlists = (min(top, max(hip.CATALOG_TOPK_MAX, 2 * k)),) * (len(dims) - 1)
        try:
            shortlists = tuple(shortlists)
        except TypeError:
            raise ValueError(f"retrieve_funnel: shortlists must be a sequence of {len(dims) - 1} ints, got {shortlists!r}") from None
        if len(shortlists) != len(dims) - 1 or any(isinstance(s, bool) or not isinstance(s, int) for s in shortlists) or \
                any(not k <= s <= top for s in shortlists) or any(b > a for a, b in zip(shortlists, shortlists[1:])):
            raise ValueError(f"retrieve_funnel: shortlists must hold {len(dims) - 1} non-increasing ints in [k, {top}] (k = {k!r}), "
                             f"got {shortlists!r}")
        u = user_embeddings.detach().to(self.catalog.device, F32).contiguous()
        ex = pack_exclude(exclude, u.shape[0])
        if ex is not None:
            ex = ex.to(u.device)
        gt = None if gt_index is None else torch.as_tensor(gt_index).to(u.device, torch.int64)
        inv = self._prefix_norms(dims)
        idx, _, rank, _ = hip.catalog_funnel_select(u, self.catalog, dims[0], shortlists[0], inv[dims[0]], gt_index=gt, exclude=ex,
                                                    chunk_rows=chunk_rows)
        keep = shortlists[1:] + (k,)
        for d, n in zip(dims[1:], keep):
            idx, val, _ = hip.catalog_funnel_rerank(u, self.catalog, idx, d, n, inv[d])
        out = {"topk_index": idx, "topk_score": val}
        if rank is not None:
            ks = (k,) if ks is None else tuple(int(x) for x in ks)
            m = ranking_metrics(rank, ks).cpu().tolist()                                 # the one host read
            out.update(rank=rank, mrr=m[0], hit_at=dict(zip(ks, m[1:1 + len(ks)])), ndcg_at=dict(zip(ks, m[1 + len(ks):])),
                       rank_is_coarse=True, rank_dim=dims[0])
        return out


class Fp8CatalogEvaluator:
    """Two-stage retrieval over a catalogue held at ONE byte per element (include/unirec_fp8.h): ``codes`` uint8 [N,D] (OCP e4m3fn bit
    patterns), ``scale`` f32 [N] (a power of two per row; ``codes.float() * scale[:, None]`` decodes exactly) and ``inv`` f32 [N] (the
    inverse norms of the code rows).  No other tensor of size N x D is held."""

    BLOCK_BYTES = 256 << 20      # full-precision bytes on the device at a time while a host catalogue streams in

    def __init__(self, catalog, item_ids=None, device="cuda", block_rows=None):
        """catalog: an f32 or bf16 tensor [N,D] (anything else is converted to f32), D a multiple of 16 and at most 2048, on the host
        or on a device.  It is quantised by ``hip.catalog_fp8_quantize`` a block of `block_rows` rows at a time (None: blocks of 256 MB);
        a host tensor is copied block by block, so no full-precision device copy is made."""
        cat = torch.as_tensor(catalog)
        if cat.dtype not in (F32, torch.bfloat16):
            cat = cat.to(F32)
        if cat.dim() != 2 or cat.shape[1] == 0 or cat.shape[1] % 16 or cat.shape[1] > 2048:
            raise ValueError(f"Fp8CatalogEvaluator: catalog must be [N,D] with D a positive multiple of 16 and at most 2048, got {tuple(cat.shape)}")
        N, D = cat.shape
        if block_rows is None:
            block_rows = max(1, self.BLOCK_BYTES // (D * cat.element_size()))
        if isinstance(block_rows, bool) or not isinstance(block_rows, int) or block_rows < 1:
            raise ValueError(f"Fp8CatalogEvaluator: block_rows must be a positive int or None, got {block_rows!r}")
        dev = torch.device(device)
        self.item_ids = None if item_ids is None else [str(i) for i in item_ids]
        self.codes = torch.empty((N, D), dtype=hip.FP8_CODES, device=dev)
        self.scale = torch.empty((N,), dtype=F32, device=dev)
        self.inv = torch.empty((N,), dtype=F32, device=dev)
        for r0 in range(0, N, block_rows):
            r1 = min(N, r0 + block_rows)
            block = cat[r0:r1].detach().to(dev).contiguous()
            hip.catalog_fp8_quantize(block, out=(self.codes[r0:r1], self.scale[r0:r1], self.inv[r0:r1]))

    @classmethod
    def from_codes(cls, codes, scale, item_ids=None):
        """An evaluator over codes uint8 (or float8_e4m3fn) [N,D] and scale f32 [N] that exist already, on their device; ``inv`` is
        recomputed from the codes a block of rows at a time (``hip.catalog_prefix_norms`` on the widened block: the row-norm chain, hence
        the bits ``hip.catalog_fp8_quantize`` writes)."""
        if codes.dtype == torch.float8_e4m3fn:
            codes = codes.view(hip.FP8_CODES)
        if codes.dtype != hip.FP8_CODES or codes.dim() != 2 or codes.shape[1] == 0 or codes.shape[1] % 16 or codes.shape[1] > 2048:
            raise ValueError("Fp8CatalogEvaluator.from_codes: codes must be uint8 or float8_e4m3fn [N,D] with D a positive multiple of 16 and at "
                             f"most 2048, got {codes.dtype} {tuple(codes.shape)}")
        if scale.dtype != F32 or scale.shape != (codes.shape[0],):
            raise ValueError(f"Fp8CatalogEvaluator.from_codes: scale must be f32 of shape [{codes.shape[0]}], got {scale.dtype} {tuple(scale.shape)}")
        ev = cls.__new__(cls)
        ev.item_ids = None if item_ids is None else [str(i) for i in item_ids]
        ev.codes = codes.contiguous()
        ev.scale = scale.to(codes.device).contiguous()
        N, D = codes.shape
        ev.inv = torch.empty((N,), dtype=F32, device=codes.device)
        rows = max(1, cls.BLOCK_BYTES // (4 * D))
        for r0 in range(0, N, rows):
            r1 = min(N, r0 + rows)
            values = ev.codes[r0:r1].view(torch.float8_e4m3fn).to(F32)             # a block of f32 code values, freed after its norms
            ev.inv[r0:r1] = hip.catalog_prefix_norms(values, (D,))[0]                # the row-norm chain, the bits of the quantiser's plane
        return ev

    def dequantized(self, index=None):
        """f32 rows: codes.float() * scale[:, None], exact; all N rows, or those of `index` (a 1-D tensor or list of row numbers)."""
        codes, scale = self.codes, self.scale
        if index is not None:
            index = torch.as_tensor(index).to(codes.device, torch.int64)
            codes, scale = codes[index], scale[index]
        return codes.view(torch.float8_e4m3fn).to(F32) * scale[:, None]

    def retrieve_two_stage(self, user_embeddings, k=10, shortlist=None, gt_index=None, exclude=None, ks=None, chunk_rows=None, rerank_with=None):
        """``CatalogEvaluator.retrieve_two_stage`` on the fp8 catalogue: ``hip.catalog_fp8_select`` picks `shortlist` items per user under
        the fp8 scores (users and rows as e4m3 codes, the users quantised by the catalogue's rule; the selection kernels of ``hip.catalog_deep_select``), then
        the shortlist is scored exactly and the best k are returned -- one path for 1 <= k <= shortlist <= 1024.
        rerank_with=None: stage 2 is ``hip.catalog_fp8_rerank``, the exact scores of the QUANTISED catalogue -- the bits
        ``hip.catalog_deep_rerank`` gives on ``dequantized()``.  rerank_with=a ``CatalogEvaluator`` over the same N items: stage 2 is
        that evaluator's ``hip.catalog_deep_rerank``, for a caller that has the full-precision rows resident anyway.
        -> the dict of ``CatalogEvaluator.retrieve_two_stage``: topk_index int32 [B,k], topk_score f32 [B,k] in the exact order of stage
        2; with gt_index also rank / mrr / hit_at / ndcg_at from the COARSE fp8 scores; always rank_is_coarse=True and
        catalog_dtype="fp8_e4m3".  exclude, ks and chunk_rows as in ``CatalogEvaluator.retrieve``.
        shortlist=None means min(1024, max(128, 2 k)): a default that leaves the re-rank twice the room it returns, NOT a tuned value --
        choose it from the recall the catalogue needs."""
        top = hip.CATALOG_DEEP_TOPK_MAX
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= top:
            raise ValueError(f"retrieve_two_stage: k must be an int in [1, {top}], got {k!r}")
        if shortlist is None:
            shortlist = min(top, max(hip.CATALOG_TOPK_MAX, 2 * k))
        if isinstance(shortlist, bool) or not isinstance(shortlist, int) or not k <= shortlist <= top:
            raise ValueError(f"retrieve_two_stage: shortlist must be an int in [k, {top}] (k = {k!r}), got {shortlist!r}")
        if rerank_with is not None and (not isinstance(rerank_with, CatalogEvaluator) or rerank_with.catalog.shape != self.codes.shape):
            got = tuple(rerank_with.catalog.shape) if isinstance(rerank_with, CatalogEvaluator) else type(rerank_with).__name__
            raise ValueError(f"retrieve_two_stage: rerank_with must be a CatalogEvaluator over the same {list(self.codes.shape)} catalogue, got {got}")
        u = user_embeddings.detach().to(self.codes.device, F32).contiguous()
        ex = pack_exclude(exclude, u.shape[0])
        if ex is not None:
            ex = ex.to(u.device)
        gt = None if gt_index is None else torch.as_tensor(gt_index).to(u.device, torch.int64)
        short, _, rank = hip.catalog_fp8_select(u, self.codes, shortlist, self.inv, gt_index=gt, exclude=ex, chunk_rows=chunk_rows)
        if rerank_with is None:
            idx, val = hip.catalog_fp8_rerank(u, self.codes, short, self.inv, k)
        else:
            idx, val, rerank_with._inv = hip.catalog_deep_rerank(u, rerank_with.catalog, short, k, rerank_with._inv)
        out = {"topk_index": idx, "topk_score": val, "rank_is_coarse": True, "catalog_dtype": "fp8_e4m3"}
        if rank is not None:
            ks = (k,) if ks is None else tuple(int(x) for x in ks)
            m = ranking_metrics(rank, ks).cpu().tolist()                                 # the one host read
            out.update(rank=rank, mrr=m[0], hit_at=dict(zip(ks, m[1:1 + len(ks)])), ndcg_at=dict(zip(ks, m[1 + len(ks):])))
        return out
