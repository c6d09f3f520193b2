"""Candidates of the joint step by index into a resident catalogue: the positives and negatives that the reference's collator
assembles on the host as f32 tensors (training/train_item_individual_token_joint.py:295-323, ``positive_item_embeddings`` [B,D] and
``negative_item_embeddings`` [B,P,D]) are rows of the item catalogue, and the catalogue already sits in HBM (``CatalogEvaluator``, f32
or bf16).  ``CatalogCandidates`` turns index tensors into the f32 tensors the unchanged InfoNCE kernels read, with one gather kernel
per tensor (``hip.gather_rows``; a bf16 catalogue is widened exactly in that pass), and can add to the batch's own negatives

  * uniformly sampled negatives, drawn on the device by a counter-based hash of (seed, step, global sample index, slot), and
  * the hardest negatives of this step's own user embeddings, mined with the streaming retrieval kernels (``hip.catalog_select``).

The index / mask assembly (``sample_indices``, ``assemble_candidates``) is pure torch integer arithmetic on [B,P]-sized tensors: no host
read, and it runs on the CPU device."""
import torch

from . import hip
from .evaluation import CatalogEvaluator, pack_exclude

BF16, F32 = torch.bfloat16, torch.float32

_M64 = (1 << 64) - 1
# splitmix64's increment and its two finalizer multipliers, and a fourth odd constant for the step
_C_SEED, _C_STEP, _C_SAMPLE, _C_SLOT = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def _i64(x):
    """The int64 that holds the low 64 bits of the Python integer x (torch int64 arithmetic wraps modulo 2^64)."""
    x &= _M64
    return x - (1 << 64) if x >> 63 else x


def _lsr(z, k):
    """Logical right shift of int64 z by k bits (torch's >> on int64 is arithmetic)."""
    return (z >> k) & ((1 << (64 - k)) - 1)


def sample_indices(seed, step, first_sample, B, num, N, device="cpu"):
    """int64 [B, num] uniform indices in [0, N), with replacement: a pure function of (seed, step, first_sample + b, slot, N).
    All arithmetic is on unsigned 64-bit integers modulo 2^64; >> is the logical shift:

        key = seed * 0x9E3779B97F4A7C15 + step * 0xD1B54A32D192ED03
        z   = key + (first_sample + b) * 0xBF58476D1CE4E5B9 + (slot + 1) * 0x94D049BB133111EB
        z   = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
        z   = (z ^ (z >> 27)) * 0x94D049BB133111EB
        z   = z ^ (z >> 31)                                  (the splitmix64 finalizer)
        index[b][slot] = ((z >> 33) * N) >> 31               (the top 31 bits scaled to [0, N); 1 <= N <= 2^31 - 1)

    Nothing depends on B or num, so a shard of the batch draws what the whole batch draws for the same users.  An index is at most
    N / 2^31 more likely than another (the multiply-shift map of 2^31 values onto N)."""
    if not 1 <= int(N) <= 2 ** 31 - 1:
        raise ValueError(f"sample_indices: N must be in [1, 2^31 - 1], got {N}")
    key = int(seed) * _C_SEED + int(step) * _C_STEP
    b = torch.arange(int(first_sample), int(first_sample) + int(B), dtype=torch.int64, device=device)
    s = torch.arange(1, int(num) + 1, dtype=torch.int64, device=device)
    z = (b * _i64(_C_SAMPLE) + _i64(key))[:, None] + (s * _i64(_C_SLOT))[None, :]
    z = (z ^ _lsr(z, 30)) * _i64(_C_SAMPLE)
    z = (z ^ _lsr(z, 27)) * _i64(_C_SLOT)
    z = z ^ _lsr(z, 31)
    return (_lsr(z, 33) * int(N)) >> 31


def _in_rows(values, table):
    """bool [B,R]: values[b][r] occurs in table[b] (int64 [B,T]); [B,R]- and [B,T]-sized work only (a sort and a binary search)."""
    if table is None or table.shape[1] == 0:
        return torch.zeros(values.shape, dtype=torch.bool, device=values.device)
    t = torch.sort(table, dim=1).values.contiguous()
    at = torch.searchsorted(t, values.contiguous()).clamp_(max=t.shape[1] - 1)
    return t.gather(1, at) == values


def assemble_candidates(positive_index, explicit_index=None, explicit_mask=None, random_index=None, mined_index=None, exclude=None):
    """The negatives of one step as (index int64 [B,P], mask uint8 [B,P]), columns in the order explicit, random, mined:
      an explicit column is valid iff its index is >= 0 and explicit_mask (if given) is nonzero there;
      a random column is valid iff its index is not positive_index[b], not in exclude[b] and not in mined_index[b];
      a mined column is valid iff its index is >= 0.
    Invalid columns carry index -1 (``gather_rows`` writes a zero row) and mask 0.  exclude: int64 [B,E], negative entries are empty
    slots (``pack_exclude``'s output, or any padded tensor).  Pure: torch ops on the inputs' device, no host read."""
    pos = positive_index.to(torch.int64)
    parts, valid = [], []
    if explicit_index is not None and explicit_index.shape[1]:
        e = explicit_index.to(torch.int64)
        ok = e >= 0
        if explicit_mask is not None:
            ok = ok & (explicit_mask.to(e.device) != 0)
        parts.append(e); valid.append(ok)
    if random_index is not None and random_index.shape[1]:
        r = random_index.to(torch.int64)
        ok = (r != pos[:, None]) & ~_in_rows(r, exclude) & ~_in_rows(r, mined_index)
        parts.append(r); valid.append(ok)
    if mined_index is not None and mined_index.shape[1]:
        m = mined_index.to(torch.int64)
        parts.append(m); valid.append(m >= 0)
    if not parts:
        raise ValueError("assemble_candidates: no negative column (no explicit index, num_random = 0 and num_hard = 0)")
    index, ok = torch.cat(parts, dim=1), torch.cat(valid, dim=1)
    return torch.where(ok, index, torch.full_like(index, -1)), ok.to(torch.uint8)


class CatalogCandidates:
    """Positives and negatives of a joint training step as indices into a resident catalogue (``JointTrainer(negatives=...)``)."""

    def __init__(self, catalog, num_random=0, num_hard=0, hard_skip=0, seed=0, scorer=None, coarse=False):
        """catalog: a CatalogEvaluator, or an [N,D] f32 / bf16 tensor (wrapped in one where it lies, so the catalogue norms that mining
        needs are computed once).  num_random uniformly sampled negatives per user (``sample``), num_hard mined ones (``mine``) after the
        hard_skip best-scoring items; hard_skip + num_hard <= hip.CATALOG_TOPK_MAX.  scorer: as for CatalogEvaluator.retrieve.
        coarse=True (a bf16 catalogue, scorer=None): ``mine`` runs ``hip.catalog_coarse_select`` -- the bf16-MFMA scores of the users
        rounded to bf16 -- with no re-rank: the mined rows are scored exactly by the InfoNCE kernels anyway, so the coarse scores only
        decide which near-boundary items are mined."""
        hip.catalog_scorer_id(scorer)
        if not isinstance(coarse, bool):
            raise ValueError(f"CatalogCandidates: coarse must be True or False, got {coarse!r}")
        if coarse and scorer is not None:
            raise ValueError(f"CatalogCandidates: coarse=True has one scoring kernel; scorer must be None, got {scorer!r}")
        self.coarse = coarse
        self.num_random, self.num_hard, self.hard_skip, self.seed, self.scorer = int(num_random), int(num_hard), int(hard_skip), int(seed), scorer
        if self.num_random < 0 or self.num_hard < 0 or self.hard_skip < 0:
            raise ValueError("CatalogCandidates: num_random, num_hard and hard_skip must be >= 0")
        if self.hard_skip + self.num_hard > hip.CATALOG_TOPK_MAX:
            raise ValueError(f"CatalogCandidates: hard_skip + num_hard = {self.hard_skip + self.num_hard} exceeds the retrieval list "
                             f"length hip.CATALOG_TOPK_MAX = {hip.CATALOG_TOPK_MAX}")
        if not isinstance(catalog, CatalogEvaluator):
            catalog = torch.as_tensor(catalog)
            if catalog.dim() != 2 or catalog.dtype not in (F32, BF16):
                raise ValueError("CatalogCandidates: catalog must be a CatalogEvaluator or an [N, D] f32 / bf16 tensor")
            catalog = CatalogEvaluator(catalog, device=catalog.device, dtype=catalog.dtype)
        if coarse and catalog.catalog.dtype != BF16:
            raise ValueError(f"CatalogCandidates: coarse=True needs a bf16 catalogue (CatalogEvaluator(dtype=torch.bfloat16)), got {catalog.catalog.dtype}")
        self.evaluator = catalog
        self.chunk_rows = None          # catalogue rows scored per chunk when mining (a multiple of 1024); None = the library's choice
        self.last_index = self.last_mask = None

    @property
    def catalog(self):
        return self.evaluator.catalog

    def gather(self, index):
        """f32 index.shape + [D] rows of the catalogue, zero rows for indices outside [0, N): one gather kernel for either catalogue
        dtype (bf16 rows are widened exactly as they are written; no f32 copy of the catalogue, no second pass)."""
        return hip.gather_rows(self.catalog, index, out_dtype=F32)

    def sample(self, B, step=0, first_sample=0):
        """int64 [B, num_random] on the catalogue's device: ``sample_indices`` (the hash is documented there) keyed on this object's seed,
        the step and the global sample index first_sample + b.  With replacement; duplicates are kept."""
        return sample_indices(self.seed, step, first_sample, B, self.num_random, self.catalog.shape[0], self.catalog.device)

    def _mine(self, user, gt_index, ex):
        ev, K = self.evaluator, self.hard_skip + self.num_hard
        with torch.no_grad():
            u = user.detach().to(ev.catalog.device, F32).contiguous()
            gt = torch.as_tensor(gt_index).to(u.device, torch.int64)
            if self.coarse:
                idx, _, _, ev._inv = hip.catalog_coarse_select(u, ev.catalog, K, ev._inv, gt_index=gt, exclude=ex, chunk_rows=self.chunk_rows)
            else:
                idx, _, _, ev._inv = hip.catalog_select(u, ev.catalog, K, ev._inv, gt_index=gt, exclude=ex, chunk_rows=self.chunk_rows, scorer=self.scorer)
            idx = idx[:, self.hard_skip:].to(torch.int64)
            return torch.where(idx == gt[:, None], torch.full_like(idx, -1), idx)

    def mine(self, user, gt_index, exclude=None):
        """int64 [B, num_hard]: the items ranked hard_skip + 1 .. hard_skip + num_hard for each user among the items not in exclude[b]
        (one streaming hip.catalog_select call on user.detach(), nothing of size B x N), with the user's own gt_index, which retrieval
        never excludes, replaced by -1; a list shorter than that ends in -1."""
        ex = pack_exclude(exclude, user.shape[0])
        return self._mine(user, gt_index, None if ex is None else ex.to(self.catalog.device))

    def candidates(self, user, positive_index, negative_index=None, negative_masks=None, exclude=None, step=0, first_sample=0):
        """-> (pos f32 [B,D], neg f32 [B,P,D], mask uint8 [B,P], index int64 [B,P]); P = explicit + num_random + num_hard columns in
        that order, valid by ``assemble_candidates``' rule; invalid columns are zero rows with mask 0.  negative_index int64 [B,P_e]
        padded with -1; exclude: the items each user has seen (ragged lists or [B,E] padded with -1), kept out of the mined and the
        random negatives.  positive_index outside [0, N) is the caller's error."""
        dev = self.catalog.device
        B = user.shape[0]
        positive_index = torch.as_tensor(positive_index).to(dev, torch.int64)
        ex = pack_exclude(exclude, B)
        ex = None if ex is None else ex.to(dev)
        mined = self._mine(user, positive_index, ex) if self.num_hard else None
        rand = self.sample(B, step, first_sample) if self.num_random else None
        if negative_index is not None:
            negative_index = torch.as_tensor(negative_index).to(dev)
        index, mask = assemble_candidates(positive_index, negative_index, negative_masks, rand, mined, ex)
        self.last_index, self.last_mask = index, mask
        return self.gather(positive_index), self.gather(index), mask, index
