"""GPU: fused global gradient-norm clipping (ur_grad_norm_clip + ur_adamw_step_dev), FusedAdamW(max_grad_norm=...) with the
HF schedules, and JointTrainer -- against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW + transformers.get_scheduler."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _norm(ranges, grad_scale=1.0, max_norm=1.0):
    from unirec_amd import hip
    n, c = torch.empty((), device=DEV), torch.empty((), device=DEV)
    hip.grad_norm_clip(ranges, grad_scale, max_norm, n, c)
    return n, c


def _ref_norm(ranges, grad_scale=1.0):
    return float(torch.linalg.vector_norm(torch.cat([r.double() for r in ranges]))) * grad_scale


def test_norm_matches_float64_and_is_deterministic():
    g = torch.Generator(device=DEV).manual_seed(1)
    sizes = [1, 7, 8, 4097, 2 ** 20 + 3]
    ranges = [torch.randn(n, device=DEV, generator=g) for n in sizes]
    for rs in [ranges[i:i + 1] for i in range(len(sizes))] + [ranges]:
        n1, c1 = _norm(rs, 0.5, 3.0)
        n2, c2 = _norm(rs, 0.5, 3.0)
        ref = _ref_norm(rs, 0.5)
        assert abs(float(n1) - ref) <= 1e-5 * ref, (len(rs), float(n1), ref)
        assert torch.equal(n1, n2) and torch.equal(c1, c2)
        coef = 3.0 / (float(n1) + 1e-6)
        assert float(c1) == pytest.approx(min(coef, 1.0), rel=1e-6)
    # many ranges (above the UR_NORM_MAX_RANGES = 64 per launch): slices of one buffer at 8-element offsets, some empty
    buf = torch.randn(8_000_000, device=DEV, generator=g)
    gen = torch.Generator().manual_seed(2)
    rs, off = [], 0
    for k in range(150):
        n = 0 if k % 37 == 5 else int(torch.randint(1, 40000, (1,), generator=gen))
        rs.append(buf[off:off + n])
        off = (off + n + 7) // 8 * 8 + 8 * int(torch.randint(0, 3, (1,), generator=gen))
    n1, _ = _norm(rs)
    n2, _ = _norm(rs)
    ref = _ref_norm(rs)
    assert abs(float(n1) - ref) <= 1e-5 * ref and torch.equal(n1, n2)
    # one pack at the C4 size (item Q-Former + LoRA live gradients: ~190 M f32)
    big = torch.randn(190_000_003, device=DEV, generator=g) * 1e-3
    n1, c1 = _norm([big], 1.0, 1.0)
    n2, c2 = _norm([big], 1.0, 1.0)
    ref = _ref_norm([big])
    assert abs(float(n1) - ref) <= 1e-5 * ref and torch.equal(n1, n2) and torch.equal(c1, c2)
    del big


def _packs(seed):
    from unirec_amd.packing import ParamPack
    g = torch.Generator().manual_seed(seed)
    specs = [[("w1", (64, 48)), ("b1", (64,)), ("w2", (33, 7)), ("ln", (48,))], [("a", (1000,)), ("b", (16, 17)), ("c", (40, 40))]]
    packs = [ParamPack([(n, torch.nn.Parameter(torch.randn(*s, generator=g))) for n, s in spec], DEV) for spec in specs]
    return packs


def _grads(packs, step, scale):
    g = torch.Generator().manual_seed(100 + step)
    return [{n: (torch.randn(p.shapes[n], generator=g) * scale).to(DEV) for n in p.names} for p in packs]


def test_clipped_training_matches_torch():
    from transformers import get_scheduler as hf_sched
    from unirec_amd.optim import FusedAdamW, get_scheduler
    packs = _packs(3)
    ref = [{n: torch.nn.Parameter(p.params[n].detach().clone()) for n in p.names} for p in packs]
    allref = [t for r in ref for t in r.values()]
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    opt = FusedAdamW(packs, max_grad_norm=1.0, **kw)
    sched = get_scheduler("linear", opt, num_warmup_steps=2, num_training_steps=5)
    topt = torch.optim.AdamW(allref, foreach=False, **kw)
    tsched = hf_sched("linear", topt, num_warmup_steps=2, num_training_steps=5)
    plan = [({"w1", "b1", "ln"}, {"a", "c"}), ({"w1", "b1", "w2", "ln"}, {"a", "b", "c"}), ({"w2"}, {"b"}),
            ({"w1", "b1", "ln"}, {"a", "b", "c"}), ({"w1", "w2"}, {"a"})]
    for step, live in enumerate(plan):
        grads = _grads(packs, step, 0.3 if step != 2 else 1e-3)         # step 2: the norm stays under max_grad_norm
        opt.zero_grad()
        for t in allref:
            t.grad = None
        for p, r, gs, lv in zip(packs, ref, grads, live):
            for n in lv:
                p.g32(n).copy_(gs[n])
                r[n].grad = gs[n] * 0.5                                     # the averaged gradient of a 2-rank sum
            p.publish_grads(sorted(lv))
        opt.step(grad_scale=0.5)
        sched.step()
        tn = torch.nn.utils.clip_grad_norm_([t for t in allref if t.grad is not None], 1.0)
        topt.step()
        tsched.step()
        assert float(opt.last_grad_norm) == pytest.approx(float(tn), rel=1e-5), step
        assert (float(tn) > 1.0) == (step != 2)
        for k, (p, r) in enumerate(zip(packs, ref)):
            m, v = opt.state[k]
            for n in p.names:
                torch.testing.assert_close(p.w32(n), r[n].detach(), rtol=1e-6, atol=1e-7, msg=f"step {step}: {n}")
                st = topt.state.get(r[n])
                if st:
                    lo, hi = p.offsets[n], p.offsets[n] + r[n].numel()
                    torch.testing.assert_close(m[lo:hi], st["exp_avg"].flatten(), rtol=1e-6, atol=1e-7, msg=f"step {step}: m {n}")
                    torch.testing.assert_close(v[lo:hi], st["exp_avg_sq"].flatten(), rtol=1e-6, atol=1e-7, msg=f"step {step}: v {n}")


def _same_step(max_grad_norm):
    from unirec_amd.optim import FusedAdamW
    packs = _packs(4)
    opt = FusedAdamW(packs, lr=1e-3, weight_decay=0.01, max_grad_norm=max_grad_norm)
    for step in range(2):
        grads = _grads(packs, step, 1e-3)
        opt.zero_grad()
        for p, gs in zip(packs, grads):
            for n in p.names:
                p.g32(n).copy_(gs[n])
            p.publish_grads(p.names[:-1] if step == 0 else None)
        opt.step(grad_scale=0.5)
    return packs, opt


def test_unclipped_paths_stay_bit_identical():
    from unirec_amd import hip
    from unirec_amd.optim import FusedAdamW
    a, oa = _same_step(1e6)         # the clamp does not bite: coef == 1.0f exactly
    b, ob = _same_step(None)
    assert float(oa._coef) == 1.0 and ob.last_grad_norm is None
    for pa, pb, sa, sb in zip(a, b, oa.state, ob.state):
        assert torch.equal(pa.master, pb.master) and torch.equal(sa[0], sb[0]) and torch.equal(sa[1], sb[1])
    # max_grad_norm=None: the launches of direct hip.adamw_step calls over the same runs
    packs = _packs(5)
    twin = [(p.master.clone(), torch.zeros_like(p.master), torch.zeros_like(p.master)) for p in packs]
    opt = FusedAdamW(packs, lr=1e-3, weight_decay=0.01)
    grads = _grads(packs, 0, 1.0)
    for p, gs in zip(packs, grads):
        for n in p.names:
            p.g32(n).copy_(gs[n])
        p.publish_grads()
    opt.step(grad_scale=0.25)
    for p, (w, m, v), (om, ov) in zip(packs, twin, opt.state):
        hip.adamw_step(w, p.grad, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0.25)
        assert torch.equal(w, p.master) and torch.equal(m, om) and torch.equal(v, ov)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nonfinite_gradient_behaves_as_torch(bad):
    from unirec_amd.optim import FusedAdamW
    packs = _packs(6)
    ref = [{n: torch.nn.Parameter(p.params[n].detach().clone()) for n in p.names} for p in packs]
    allref = [t for r in ref for t in r.values()]
    opt = FusedAdamW(packs, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    topt = torch.optim.AdamW(allref, lr=1e-3, weight_decay=0.01, foreach=False)
    grads = _grads(packs, 0, 0.3)
    grads[1]["b"][3, 5] = bad
    for p, r, gs in zip(packs, ref, grads):
        for n in p.names:
            p.g32(n).copy_(gs[n])
            r[n].grad = gs[n].clone()
        p.publish_grads()
    opt.step()
    tn = torch.nn.utils.clip_grad_norm_(allref, 1.0)
    topt.step()
    assert (torch.isnan(opt.last_grad_norm) and torch.isnan(tn)) or float(opt.last_grad_norm) == float(tn) == float("inf")
    for p, r in zip(packs, ref):
        for n in p.names:
            mine, theirs = p.w32(n), r[n].detach()
            assert torch.equal(torch.isnan(mine), torch.isnan(theirs)), n
            torch.testing.assert_close(mine, theirs, rtol=1e-6, atol=1e-7, equal_nan=True)


def test_clipped_step_does_not_sync_the_host():
    from unirec_amd.optim import FusedAdamW
    packs = _packs(7)
    opt = FusedAdamW(packs, lr=1e-3, max_grad_norm=1.0)
    for step in range(2):
        grads = _grads(packs, step, 0.3)
        opt.zero_grad()
        for p, gs in zip(packs, grads):
            for n in p.names:
                p.g32(n).copy_(gs[n])
            p.publish_grads()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            opt.step(grad_scale=0.5, lr=2e-4)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    assert opt.last_grad_norm.is_cuda and opt.last_grad_norm.dim() == 0


def _joint(case_name="joint_left", B=None):
    from tests.golden import cases
    from tests.test_gpu_joint import _build_joint
    case = dict(cases.ALL[case_name], drop_one_special=False, **({} if B is None else {"B": B}))
    m, qf = _build_joint(case, use_lora=True, lora_seed=case["seed"] + 2)
    return case, m


def _inputs(case, lo=None, hi=None):
    import numpy as np
    from tests.golden import cases
    ids, am, hfe, ham, pos, neg, nmask = cases.joint_inputs(case)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(DEV)
    return {"input_ids": t(ids), "attention_mask": t(am), "history_field_embeddings": t(hfe), "history_attention_mask": t(ham),
            "positive_item_embeddings": t(pos), "negative_item_embeddings": t(neg), "negative_masks": t(nmask)}


def test_joint_trainer_matches_a_hand_composed_step(tmp_path):
    from transformers import Trainer, TrainingArguments
    from transformers import get_scheduler as hf_sched
    from unirec_amd.joint import JointTrainer, MultiModalTrainer
    args = TrainingArguments(output_dir=str(tmp_path), learning_rate=1e-4, warmup_steps=1, max_steps=3, max_grad_norm=1.0,
                             weight_decay=0.01, logging_steps=1, report_to=[])
    case, ma = _joint()
    _, mb = _joint()
    batch = _inputs(case)
    tr = JointTrainer(ma, args)
    # hand-composed on the second copy: compute_loss -> backward -> torch clip / AdamW (HF's decay groups) / schedule
    decay = set(Trainer.get_decay_parameter_names(None, mb))
    packs = [mb.qformer_model._ensure_pack(batch["input_ids"].device), mb.base_model._ensure_pack(batch["input_ids"].device)]
    ids = {id(p.params[n]) for p in packs for n in p.names}
    named = [(n, p) for n, p in mb.named_parameters() if id(p) in ids]
    groups = [{"params": [p for n, p in named if n in decay], "weight_decay": 0.01},
              {"params": [p for n, p in named if n not in decay], "weight_decay": 0.0}]
    topt = torch.optim.AdamW(groups, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    tsched = hf_sched("linear", topt, num_warmup_steps=1, num_training_steps=3)
    loss_fn = MultiModalTrainer()
    norms, lrs = [], []
    for step in range(3):
        la = tr.training_step(batch)
        for p in packs:
            p.clear_grads()
        lb = loss_fn.compute_loss(mb, batch)
        lb.backward()
        lrs.append(topt.param_groups[0]["lr"])
        norms.append(float(torch.nn.utils.clip_grad_norm_([p for _, p in named if p.grad is not None], 1.0)))
        topt.step()
        tsched.step()
        for p in packs:
            p.mark_dirty()
        assert float(la) == pytest.approx(float(lb.detach()), rel=1e-5, abs=1e-6), step
        for pa, pb in zip(tr.packs, packs):
            torch.testing.assert_close(pa.master, pb.master, rtol=1e-6, atol=1e-7, msg=f"step {step}")
        # the next step starts from the SAME weights on both sides: torch's AdamW rounds some f32 masters one ulp away from the
        # kernel's, which can flip their bf16 operand, and the forward would compound that into the next step's comparison
        with torch.no_grad():
            for pa, pb in zip(tr.packs, packs):
                pb.master.copy_(pa.master)
                pb.mark_dirty()
    assert norms[0] > 1.0, "the clip must bite for this test to mean anything"
    hist = tr.state.log_history
    assert [h["step"] for h in hist] == [1, 2, 3]
    assert [h["learning_rate"] for h in hist] == lrs
    for h, n in zip(hist, norms):
        assert h["grad_norm"] == pytest.approx(n, rel=1e-5)
    # moments of the last step
    for pa, pb, (m, v) in zip(tr.packs, packs, tr.optimizer.state):
        for n in pa.names:
            st = topt.state.get(pb.params[n])
            if st:
                lo, hi = pa.offsets[n], pa.offsets[n] + pa.params[n].numel()
                torch.testing.assert_close(m[lo:hi], st["exp_avg"].flatten(), rtol=1e-6, atol=1e-7, msg=n)
                torch.testing.assert_close(v[lo:hi], st["exp_avg_sq"].flatten(), rtol=1e-6, atol=1e-7, msg=n)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(outdir, world, Bg):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   UNIREC_DP_BACKEND="gloo", OMP_NUM_THREADS="2", GLOO_SOCKET_IFNAME="lo")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "clip_dp_worker.py"), str(outdir), str(Bg)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0])
    except subprocess.TimeoutExpired:
        for p in procs:
            if p.poll() is None:
                p.kill()
        tails = [p.communicate()[0][-2000:] for p in procs]
        raise AssertionError(f"a rank did not finish within 240 s (world {world}):\n" + "\n-----\n".join(tails))
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [torch.load(os.path.join(outdir, f"rank{r}.pt")) for r in range(world)]


def test_clipped_joint_step_under_two_ranks(tmp_path):
    """One clipped JointTrainer step on two gloo ranks sharing cuda:0: both ranks end bit-identical (parameters and grad_norm), and
    the step equals the single-process step over the concatenated batch (the norm of the AVERAGED gradient, the same coefficient)."""
    d2 = tmp_path / "w2"; d2.mkdir()
    r0, r1 = _launch(d2, 2, 4)
    assert r0["world"] == 2 and r0["n"] == 2 and r1["n"] == 2
    assert r0["grad_norm"] == r1["grad_norm"] and r0["grad_norm"] > r0["max_grad_norm"]
    for k in ("qformer", "lora"):
        assert torch.equal(r0["master"][k], r1["master"][k]) and torch.equal(r0["exp_avg"][k], r1["exp_avg"][k])
    d1 = tmp_path / "w1"; d1.mkdir()
    (s0,) = _launch(d1, 1, 4)
    assert s0["world"] == 1
    assert abs(r0["grad_norm"] - s0["grad_norm"]) <= 3e-2 * s0["grad_norm"], (r0["grad_norm"], s0["grad_norm"])
    for k in ("qformer", "lora"):
        m2, m1 = r0["exp_avg"][k], s0["exp_avg"][k]          # (1 - beta1) * coef * averaged gradient
        rel = float((m2 - m1).norm() / m1.norm())
        print(k, "2-rank vs 1-rank clipped first moment rel err", rel)
        assert float(m1.norm()) > 0 and rel <= 3e-2, (k, rel)
