#!/usr/bin/env python3
"""Generate tests/golden/mrl_tiny.npz: the Matryoshka InfoNCE loss as the reference's OWN ``InfoNCELoss`` gives it term by term.

The reference has no Matryoshka loss; it pins every term of one: plane k is its ``InfoNCELoss`` (imported from its training module
through make_golden.py's shim, as ``mg.rj``) applied to ``u[:, :d_k], p[:, :d_k], n[..., :d_k]``.  This script calls it on those
slices for the two cases and the dims of tests/mrl_ref.py, sums the planes under each of the two weight vectors and takes ``d user``
from autograd.  Stored per case: the per-plane losses, and per weight vector the weighted total and the gradient.  Inputs are
regenerated from seeds (tests/mrl_ref.mrl_case_inputs): the file holds outputs only, and nothing of the reference is written anywhere.

Usage:  python tests/golden/make_golden_mrl.py
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
from tests import mrl_ref  # noqa: E402


def main():
    res = {}
    loss_fn = mg.rj.InfoNCELoss(temperature=mrl_ref.MRL_TAU)
    for name in mrl_ref.MRL_CASES:
        user, pos, neg, mask = mrl_ref.mrl_case_inputs(name)
        for wname, weights in mrl_ref.MRL_WEIGHTS.items():
            u = user.clone().requires_grad_(True)
            planes = [loss_fn(u[:, :d], pos[:, :d], neg[..., :d], mask) for d in mrl_ref.MRL_DIMS]
            total = sum(lam * l for lam, l in zip(weights, planes))
            total.backward()
            res[f"{name}/plane_loss"] = np.array([float(l.detach()) for l in planes], dtype=np.float32)
            res[f"{name}/{wname}/loss"] = total.detach().numpy()
            res[f"{name}/{wname}/d_user"] = u.grad.numpy().copy()
    assert sorted(res) == mrl_ref.fixture_keys()
    path = os.path.join(HERE, "mrl_tiny.npz")
    np.savez_compressed(path, **res)
    nan = [k for k, v in res.items() if not np.isfinite(v).all()]
    print(f"mrl_tiny: {len(res)} arrays, {os.path.getsize(path) / 1024:.1f} KiB, non-finite: {nan}")


if __name__ == "__main__":
    main()
