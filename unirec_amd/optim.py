"""Fused AdamW over flat parameter packs (one HIP kernel launch per contiguous run of live tensors; one per pack when
every tensor received a gradient).

Semantics = torch.optim.AdamW (decoupled weight decay), the optimizer of all three reference loops
(training/item_qformer_training.py:108, training/user_qformer_training.py:196, HF Trainer default at
train_item_individual_token_joint.py:755-773), including what it does with parameters a backward did not reach:
``grad is None`` => the parameter is skipped entirely -- no weight decay, no moment update, its own step count does not
advance (the item Q-Former's heads and ``UserQFormer.prediction_head`` in the joint step).  Which tensors are live is
what the backward published since the last ``zero_grad()`` (packing.ParamPack.live).  Gradients are OVERWRITTEN, not
accumulated, by every backward: call ``zero_grad()`` once per step as the reference loops do, so a tensor touched in one
step and untouched in the next is not re-stepped with a stale gradient.  ``grad_scale`` folds the 1/world_size of a
summed all-reduce into the update.  ``state_dict`` / ``load_state_dict`` carry the moments and step counts (resume).

``max_grad_norm`` (off by default) adds what HF Trainer does with ``TrainingArguments.max_grad_norm`` after the backward:
``torch.nn.utils.clip_grad_norm_`` over every tensor the step updates (all packs together: one global L2 norm), here as one
deterministic norm launch that writes the norm and the clip coefficient to device memory, read by the AdamW launches on the same
stream -- no host sync.  ``no_decay`` names take ``weight_decay = 0`` (HF's bias / LayerNorm rule).  ``get_scheduler`` is
``transformers.get_scheduler``'s arithmetic on the host: the learning rate is a kernel argument.
"""
import math

import torch

from . import hip


class FusedAdamW:
    def __init__(self, packs, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=None, no_decay=()):
        self.packs = [p for p in packs if p is not None]
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"FusedAdamW: max_grad_norm must be > 0 or None (off), got {max_grad_norm}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.no_decay = frozenset(no_decay)          # pack tensor names stepped with weight_decay = 0 (in every pack)
        self.step_count = 0
        self.state = [(torch.zeros_like(p.master), torch.zeros_like(p.master)) for p in self.packs]
        self.steps = [{n: 0 for n in p.names} for p in self.packs]          # per-tensor step counts (bias correction)
        self._norm = self._coef = None               # 0-d device scalars of the clipped step (allocated once)

    @property
    def last_grad_norm(self):
        """Global gradient norm of the latest clipped step as a 0-d f32 DEVICE tensor (reading it is the caller's host sync);
        None before the first clipped step or with clipping off."""
        return self._norm

    def zero_grad(self, set_to_none=True):
        for p in self.packs:
            p.clear_grads(set_to_none)

    def _drop_stale(self):
        # torch.optim.AdamW's rule whoever reset the gradients: a tensor whose .grad is None now (model.zero_grad(), HF Trainer, a
        # torch optimizer's zero_grad -- none of which clears pack.live) is not stepped
        for pack in self.packs:
            stale = [n for n in pack.live if pack.params[n].grad is None]
            for n in stale:
                pack.live.discard(n)

    def grad_spans(self):
        """(pack index, lo, hi) of every merged contiguous span of the tensors step() will update (stale ones dropped first): the
        gradient elements of the global norm -- HF's one norm over model.parameters() with grad is not None."""
        self._drop_stale()
        return [(k, lo, hi) for k, p in enumerate(self.packs) for lo, hi in p.live_spans()]

    def step(self, grad_scale=1.0, lr=None):
        """One AdamW step of every live tensor at `lr` (default self.lr).  With max_grad_norm set, the norm of the gradient times
        grad_scale (the averaged gradient of a summed all-reduce) and the clip coefficient are computed first on the current stream."""
        self.step_count += 1
        lr = self.lr if lr is None else lr
        coef = None
        if self.max_grad_norm is not None:
            spans = self.grad_spans()
            if self._norm is None:
                dev = self.packs[0].grad.device
                self._norm = torch.zeros((), dtype=torch.float32, device=dev)
                self._coef = torch.ones((), dtype=torch.float32, device=dev)
            hip.grad_norm_clip([self.packs[k].grad[lo:hi] for k, lo, hi in spans], grad_scale, self.max_grad_norm, self._norm, self._coef)
            coef = self._coef
        else:
            self._drop_stale()
        nd = self.no_decay
        for pack, (m, v), steps in zip(self.packs, self.state, self.steps):
            if not pack.live:
                continue
            for n in pack.live:
                steps[n] += 1
            # runs split where the step count (bias correction) or the decay changes; with no_decay empty these are the step-count runs
            for lo, hi, (t, decays) in pack.live_ranges(key=lambda n: (steps[n], n not in nd)):
                hip.adamw_step(pack.master[lo:hi], pack.grad[lo:hi], m[lo:hi], v[lo:hi], lr, self.betas[0], self.betas[1],
                               self.eps, self.weight_decay if decays else 0.0, t, grad_scale, coef=coef)
            pack.mark_dirty()

    # ---- resume -----------------------------------------------------------------------------------------------------
    def state_dict(self):
        return {"step_count": self.step_count, "lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay,
                "max_grad_norm": self.max_grad_norm, "no_decay": sorted(self.no_decay),
                "packs": [{"names": list(p.names), "offsets": dict(p.offsets), "steps": dict(s), "exp_avg": m.detach().clone(),
                           "exp_avg_sq": v.detach().clone()} for p, (m, v), s in zip(self.packs, self.state, self.steps)]}

    def load_state_dict(self, sd):
        if len(sd["packs"]) != len(self.packs):
            raise ValueError(f"optimizer state holds {len(sd['packs'])} packs, this optimizer {len(self.packs)}")
        for p, (m, v), s, rec in zip(self.packs, self.state, self.steps, sd["packs"]):
            if list(rec["names"]) == list(p.names) and dict(rec["offsets"]) == dict(p.offsets):
                m.copy_(rec["exp_avg"].to(m.device))
                v.copy_(rec["exp_avg_sq"].to(v.device))
            elif set(rec["names"]) == set(p.names):
                # same tensors, another order (a pack layout change between versions, e.g. the hoisted cross-attention K|V weights):
                # the moments move tensor by tensor, recorded offsets -> current offsets
                rm, rv, roff = rec["exp_avg"].to(m.device), rec["exp_avg_sq"].to(v.device), dict(rec["offsets"])
                # every recorded tensor's extent = the gap to the next recorded offset (or the buffer's end) must be the 8-padded size
                # of the CURRENT tensor: the same names at another shape (a different LoRA rank, hidden size) would otherwise load
                # moments that overlap the neighbours
                order = sorted(roff.values()) + [rm.numel()]
                extent = {o: order[k + 1] - o for k, o in enumerate(order[:-1])}
                for n in p.names:
                    num = p.params[n].numel()
                    if extent[roff[n]] != (num + 7) // 8 * 8:
                        raise ValueError(f"optimizer state: {n} was recorded with {extent[roff[n]]} (padded) elements, the pack holds {num}")
                for n in p.names:
                    lo, num = p.offsets[n], p.params[n].numel()
                    m[lo:lo + num].copy_(rm[roff[n]:roff[n] + num])
                    v[lo:lo + num].copy_(rv[roff[n]:roff[n] + num])
            else:
                raise ValueError("optimizer state does not match the parameter pack (different tensor names)")
            s.update(rec["steps"])
        self.step_count = int(sd["step_count"])
        self.lr, self.betas, self.eps, self.weight_decay = sd["lr"], tuple(sd["betas"]), sd["eps"], sd["weight_decay"]
        # (a state saved before clipping existed has neither key: the optimizer keeps what it was built with)
        if "max_grad_norm" in sd:
            self.max_grad_norm = None if sd["max_grad_norm"] is None else float(sd["max_grad_norm"])
        if "no_decay" in sd:
            self.no_decay = frozenset(sd["no_decay"])


# ---- learning-rate schedules (transformers.get_scheduler's lambdas, the same float arithmetic) ---------------------------------------
def _warm(step, warmup):
    return float(step) / float(max(1, warmup))


def _linear(step, warmup, total):
    if step < warmup:
        return _warm(step, warmup)
    return max(0.0, float(total - step) / float(max(1, total - warmup)))


def _cosine(step, warmup, total, num_cycles=0.5):
    if step < warmup:
        return _warm(step, warmup)
    progress = float(step - warmup) / float(max(1, total - warmup))
    factor = 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * progress))
    return max(0, factor)


def _constant_with_warmup(step, warmup):
    if step < warmup:
        return float(step) / float(max(1.0, warmup))
    return 1.0


_SCHEDULES = {
    "linear": lambda s, w, t: _linear(s, w, t),
    "cosine": lambda s, w, t: _cosine(s, w, t),
    "constant": lambda s, w, t: 1.0,
    "constant_with_warmup": lambda s, w, t: _constant_with_warmup(s, w),
}


class LRSchedule:
    """torch LambdaLR over a FusedAdamW: lr = base_lr * factor(last_epoch); construction applies factor(0) (HF's first update runs at
    lr * 0 / warmup = 0), every step() advances one and sets opt.lr.  Host arithmetic only."""

    def __init__(self, opt, name, num_warmup_steps=0, num_training_steps=None):
        self.opt, self.name = opt, name
        self.num_warmup_steps, self.num_training_steps = int(num_warmup_steps or 0), num_training_steps
        self.base_lr = float(opt.lr)
        self.last_epoch = 0
        self._fn = _SCHEDULES[name]
        self._apply()

    def _apply(self):
        self.opt.lr = self.base_lr * self._fn(self.last_epoch, self.num_warmup_steps, self.num_training_steps)
        self._last_lr = [self.opt.lr]

    def step(self):
        self.last_epoch += 1
        self._apply()

    def get_last_lr(self):
        return list(self._last_lr)

    def state_dict(self):
        return {"name": self.name, "num_warmup_steps": self.num_warmup_steps, "num_training_steps": self.num_training_steps,
                "base_lr": self.base_lr, "last_epoch": self.last_epoch}

    def load_state_dict(self, sd):
        if sd["name"] != self.name:
            raise ValueError(f"schedule state is {sd['name']!r}, this schedule {self.name!r}")
        self.num_warmup_steps, self.num_training_steps = sd["num_warmup_steps"], sd["num_training_steps"]
        self.base_lr, self.last_epoch = sd["base_lr"], sd["last_epoch"]
        self._apply()


def get_scheduler(name, opt, num_warmup_steps=None, num_training_steps=None):
    """transformers.get_scheduler for the schedules the joint step uses: 'linear' (the reference's), 'cosine', 'constant',
    'constant_with_warmup'.  The value at every step equals HF's."""
    name = getattr(name, "value", name)          # transformers.SchedulerType
    if name not in _SCHEDULES:
        raise ValueError(f"get_scheduler: unsupported schedule {name!r} (supported: {sorted(_SCHEDULES)})")
    if name != "constant" and num_warmup_steps is None:
        raise ValueError(f"{name} requires `num_warmup_steps`, please provide that argument.")
    if name in ("linear", "cosine") and num_training_steps is None:
        raise ValueError(f"{name} requires `num_training_steps`, please provide that argument.")
    return LRSchedule(opt, name, num_warmup_steps or 0, num_training_steps)
