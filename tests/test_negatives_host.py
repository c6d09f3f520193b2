"""CPU: candidates by index -- the argument checks of ur_gather_rows' bf16 -> f32 pair through the raw library (fake non-null
pointers: every call here returns before any launch), the counter-based sampler against a numpy restatement of its documented hash,
the mask rule of assemble_candidates on hand-made index tensors, and the construction / wiring errors."""
import numpy as np
import pytest
import torch

from unirec_amd import _lib, hip
from unirec_amd.negatives import CatalogCandidates, assemble_candidates, sample_indices

FAKE = 256          # non-null, 16-byte aligned, never dereferenced on the host
U8, BF16, F32 = 0, 1, 2


def _gather(lib, src_kind, out_kind, row_elems=16, n_out=4, n_src=10):
    return lib.ur_gather_rows(FAKE, src_kind, FAKE, out_kind, FAKE, row_elems, n_out, n_src, None)


def test_widening_pair_is_legal_and_checked():
    lib = _lib.load()
    assert _gather(lib, BF16, F32, n_out=0) == 0, lib.ur_last_error()
    assert _gather(lib, BF16, F32, row_elems=12) < 0
    assert b"ur_gather_rows" in lib.ur_last_error()
    assert lib.ur_gather_rows(FAKE + 8, BF16, FAKE, F32, FAKE, 16, 4, 10, None) < 0        # src not 16-byte aligned
    assert b"ur_gather_rows" in lib.ur_last_error()
    assert lib.ur_gather_rows(FAKE, BF16, FAKE + 8, F32, FAKE, 16, 4, 10, None) < 0        # out not 16-byte aligned
    assert lib.ur_gather_rows(FAKE, BF16, None, F32, FAKE, 16, 4, 10, None) < 0
    assert _lib.ABI_VERSION >= 17 and lib.ur_version() == _lib.ABI_VERSION      # (the widening pair arrived with ABI 17)


@pytest.mark.parametrize("src_kind,out_kind", [(U8, F32), (F32, U8), (BF16, U8), (U8, BF16), (3, F32), (BF16, 3)])
@pytest.mark.parametrize("n_out", [0, 4])
def test_other_mixed_pairs_are_still_refused(src_kind, out_kind, n_out):
    lib = _lib.load()
    assert _gather(lib, src_kind, out_kind, n_out=n_out) < 0
    assert b"ur_gather_rows" in lib.ur_last_error()


def test_pairs_of_before_pass_the_empty_call():
    lib = _lib.load()
    for src_kind, out_kind in ((U8, U8), (BF16, BF16), (F32, F32), (F32, BF16)):
        assert _gather(lib, src_kind, out_kind, n_out=0) == 0


# ---- sample(): an independent restatement of the documented hash, in numpy uint64 arithmetic (which wraps modulo 2^64)
def _np_sample(seed, step, first_sample, B, num, N):
    u = np.uint64
    key = u((seed * 0x9E3779B97F4A7C15 + step * 0xD1B54A32D192ED03) % 2 ** 64)
    out = np.empty((B, num), dtype=np.int64)
    with np.errstate(over="ignore"):
        for b in range(B):
            for slot in range(num):
                z = key + u(first_sample + b) * u(0xBF58476D1CE4E5B9) + u(slot + 1) * u(0x94D049BB133111EB)
                z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
                z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
                z = z ^ (z >> u(31))
                out[b, slot] = int(((z >> u(33)) * u(N)) >> u(31))
    return out


@pytest.mark.parametrize("seed,step", [(0, 0), (1234567, 98765)])
def test_sample_equals_the_documented_hash(seed, step):
    N = 1_000_003
    got = sample_indices(seed, step, 3, 6, 5, N)
    assert got.dtype == torch.int64 and got.shape == (6, 5)
    assert np.array_equal(got.numpy(), _np_sample(seed, step, 3, 6, 5, N))
    assert int(got.min()) >= 0 and int(got.max()) < N
    assert torch.equal(sample_indices(seed, step, 2, 4, 5, 1), torch.zeros(4, 5, dtype=torch.int64)), "N = 1 leaves one index"
    # the method is the free function on the object's (seed, N, num_random, device)
    cat = torch.zeros(97, 8)
    cc = CatalogCandidates(cat, num_random=7, seed=seed)
    s = cc.sample(5, step, 11)
    assert s.device == cat.device and torch.equal(s, sample_indices(seed, step, 11, 5, 7, 97))
    assert np.array_equal(s.numpy(), _np_sample(seed, step, 11, 5, 7, 97))
    # the largest catalogue the retrieval kernels take
    big = sample_indices(seed, step, 0, 4, 64, 2 ** 31 - 1)
    assert np.array_equal(big.numpy(), _np_sample(seed, step, 0, 4, 64, 2 ** 31 - 1)) and int(big.min()) >= 0 and int(big.max()) < 2 ** 31 - 1


def test_sample_split_invariance_and_keys():
    cc = CatalogCandidates(torch.zeros(5000, 8), num_random=12, seed=7)
    whole = cc.sample(8, 3, 0)
    assert torch.equal(whole[4:], cc.sample(4, 3, 4))
    assert torch.equal(whole[:4], cc.sample(4, 3, 0))
    assert not torch.equal(whole, cc.sample(8, 4, 0)), "another step draws again"
    assert not torch.equal(whole, CatalogCandidates(torch.zeros(5000, 8), num_random=12, seed=8).sample(8, 3, 0)), "another seed draws again"
    assert torch.equal(whole, CatalogCandidates(torch.zeros(5000, 8), num_random=12, seed=7).sample(8, 3, 0)), "pure"
    # fewer slots are a prefix: a slot's draw does not depend on num_random
    assert torch.equal(whole[:, :5], CatalogCandidates(torch.zeros(5000, 8), num_random=5, seed=7).sample(8, 3, 0))


def test_sample_spread():
    """65 536 draws over N = 16: expectation 4096 per bin, binomial sigma = sqrt(65536 * 1/16 * 15/16) = 61.97; the bound is 6 sigma."""
    s = sample_indices(5, 17, 0, 256, 256, 16)
    counts = torch.bincount(s.flatten(), minlength=16)
    assert counts.numel() == 16 and int(counts.sum()) == 65536
    dev = (counts - 4096).abs()
    print("bin counts", counts.tolist())
    assert int(dev.max()) <= 372, counts.tolist()


# ---- the mask rule
def test_mask_rule_on_hand_made_indices():
    pos = torch.tensor([10, 20, 30])
    explicit = torch.tensor([[1, 2, -1], [3, -1, -1], [4, 5, 6]])
    batch_mask = torch.tensor([[1, 0, 1], [1, 1, 1], [1, 1, 0]])
    #                     b0: the positive, free, seen (41), mined (50)   b1: all free (a duplicate kept)   b2: seen, mined, free, positive
    rand = torch.tensor([[10, 11, 41, 50], [7, 7, 8, 9], [43, 61, 12, 30]])
    mined = torch.tensor([[50, 51], [52, -1], [-1, 61]])
    exclude = torch.tensor([[-1, 41, 40], [-1, -1, -1], [43, 42, -1]])          # unsorted and padded: any padded tensor is taken
    index, mask = assemble_candidates(pos, explicit, batch_mask, rand, mined, exclude)
    want_mask = torch.tensor([[1, 0, 0,  0, 1, 0, 0,  1, 1],
                              [1, 0, 0,  1, 1, 1, 1,  1, 0],
                              [1, 1, 0,  0, 0, 1, 0,  0, 1]], dtype=torch.uint8)
    want_index = torch.tensor([[1, -1, -1,  -1, 11, -1, -1,  50, 51],
                               [3, -1, -1,  7, 7, 8, 9,  52, -1],
                               [4, 5, -1,  -1, -1, 12, -1,  -1, 61]])
    assert mask.dtype == torch.uint8 and index.dtype == torch.int64
    assert torch.equal(mask, want_mask), mask
    assert torch.equal(index, want_index), index
    # without the optional parts: no batch mask, no exclusion, no mined list
    index, mask = assemble_candidates(pos, explicit, None, rand, None, None)
    assert torch.equal(mask, torch.tensor([[1, 1, 0,  0, 1, 1, 1], [1, 0, 0,  1, 1, 1, 1], [1, 1, 1,  1, 1, 1, 0]], dtype=torch.uint8))
    assert torch.equal(index[mask.bool()], torch.cat([explicit, rand], 1)[mask.bool()]) and bool((index[~mask.bool()] == -1).all())
    # explicit columns alone, and random columns alone
    index, mask = assemble_candidates(pos, explicit)
    assert torch.equal(index, explicit) and torch.equal(mask, (explicit >= 0).to(torch.uint8))
    index, mask = assemble_candidates(pos, None, None, rand)
    assert torch.equal(mask, (rand != pos[:, None]).to(torch.uint8))
    with pytest.raises(ValueError):
        assemble_candidates(pos)


def test_mask_rule_against_a_loop():
    g = torch.Generator().manual_seed(11)
    B, N = 6, 40
    pos = torch.randint(0, N, (B,), generator=g)
    explicit = torch.randint(-1, N, (B, 5), generator=g)
    bmask = torch.randint(0, 2, (B, 5), generator=g)
    rand = torch.randint(0, N, (B, 30), generator=g)
    mined = torch.randint(-1, N, (B, 4), generator=g)
    exclude = torch.randint(-1, N, (B, 9), generator=g)
    index, mask = assemble_candidates(pos, explicit, bmask, rand, mined, exclude)
    for b in range(B):
        seen, hard = set(exclude[b].tolist()) - {-1}, set(mined[b].tolist()) - {-1}
        want = [int(e >= 0 and m) for e, m in zip(explicit[b].tolist(), bmask[b].tolist())]
        want += [int(r != int(pos[b]) and r not in seen and r not in hard) for r in rand[b].tolist()]
        want += [int(m >= 0) for m in mined[b].tolist()]
        full = explicit[b].tolist() + rand[b].tolist() + mined[b].tolist()
        assert mask[b].tolist() == want, b
        assert index[b].tolist() == [i if w else -1 for i, w in zip(full, want)], b


# ---- construction and wiring
def test_construction_errors(monkeypatch):
    cat = torch.zeros(10, 8)
    with pytest.raises(ValueError) as e:
        CatalogCandidates(cat, num_hard=100, hard_skip=29)
    assert "129" in str(e.value)
    CatalogCandidates(cat, num_hard=100, hard_skip=28)
    CatalogCandidates(cat, num_hard=hip.CATALOG_TOPK_MAX)
    with pytest.raises(ValueError):
        CatalogCandidates(cat, num_random=-1)
    with pytest.raises(ValueError):
        CatalogCandidates(cat.to(torch.float16))
    with pytest.raises(ValueError):
        CatalogCandidates(torch.zeros(10))

    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    for bad in ("MFMA", "tensor", 2):
        with pytest.raises(ValueError):
            CatalogCandidates(cat, scorer=bad)
    for good in (None, "vector", "mfma"):
        assert CatalogCandidates(cat, scorer=good).scorer == good


def test_a_tensor_is_wrapped_and_an_evaluator_is_kept():
    from unirec_amd.evaluation import CatalogEvaluator
    cat = torch.randn(10, 8, generator=torch.Generator().manual_seed(0))
    cc = CatalogCandidates(cat.to(torch.bfloat16))
    assert isinstance(cc.evaluator, CatalogEvaluator) and cc.catalog.dtype == torch.bfloat16 and cc.catalog.device == cat.device
    assert torch.equal(cc.catalog, cat.to(torch.bfloat16))
    ev = CatalogEvaluator(cat, device="cpu")
    assert CatalogCandidates(ev).evaluator is ev


def test_index_batch_without_negatives_names_the_argument():
    from unirec_amd.joint import MultiModalTrainer

    def model(**kw):
        raise AssertionError("the forward ran")
    with pytest.raises(ValueError) as e:
        MultiModalTrainer().compute_loss(model, {"positive_item_index": torch.tensor([1, 2])})
    assert "negatives" in str(e.value)
