#!/usr/bin/env python3
"""Generate tests/golden/pool_tiny.npz: the pooled vectors of the two mask-aware pooling rules on the installed
``transformers.Qwen3Model`` at the _TINYQ shape, one left-padded and one right-padded batch (tests/pool_ref.POOL_CASES).

Follows make_golden.py (its shim, weights from the oracle.weights generator pushed in through load_state_dict; nothing of the reference
is written anywhere).  "last" is the reference's OWN ``last_token_pool``, imported from its training module here; a masked mean does
not exist in the reference, so that rule is written below and is pinned by the oracle alone (README, parity section).  Stored per
padding side and rule: the pooled vectors and the gradient of loss = sum(pooled * r) with respect to inputs_embeds, r seeded.
Inputs are regenerated from seeds (tests/pool_ref.pool_case_inputs): the file holds outputs only.

The attention implementation is sdpa; the two HF paths differ only in the rows of fully masked queries (left padding), which neither
rule reads and which no valid query attends to.

Usage:  python tests/golden/make_golden_pool.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (installs the shim and imports the reference's training module as mg.rj)
from tests import pool_ref  # noqa: E402
from tests.golden import cases  # noqa: E402


def masked_mean_pool(last_hidden_states, attention_mask):
    m = attention_mask.to(last_hidden_states.dtype)[..., None]
    return (last_hidden_states * m).sum(dim=1) / m.sum(dim=1)


def main():
    res = {}
    for side, case in pool_ref.POOL_CASES.items():
        x, am, r = pool_ref.pool_case_inputs(side)
        base = mg.build_hf_qwen3(cases.qwen_cfg(case), case["seed"] + 1, "sdpa")
        amt, rt = torch.from_numpy(am), torch.from_numpy(r)
        for mode, fn in (("last", mg.rj.last_token_pool), ("masked_mean", masked_mean_pool)):
            xt = torch.from_numpy(x).requires_grad_(True)
            h = base(inputs_embeds=xt, attention_mask=amt).last_hidden_state
            pooled = fn(h, amt)
            (pooled * rt).sum().backward()
            res[f"{side}/{mode}/pooled"] = pooled.detach().numpy()
            res[f"{side}/{mode}/grad_inputs_embeds"] = xt.grad.numpy().copy()
    path = os.path.join(HERE, "pool_tiny.npz")
    np.savez_compressed(path, **res)
    nan = [k for k, v in res.items() if not np.isfinite(v).all()]
    print(f"pool_tiny: {len(res)} arrays, {os.path.getsize(path) / 1024:.1f} KiB, non-finite: {nan}")


if __name__ == "__main__":
    main()
