"""GPU: the optimizer step, the casts, the bf16 add and the transposes of csrc/elementwise.hip, ELEMENT BY ELEMENT against float64 or bit
for bit (tests/ref64.py, checked on the CPU in tests/test_ref64.py; inputs from tests/ew_cases.py), at sizes that enter the grid-stride
loops the product always runs: ew_grid caps a launch at 2048 workgroups of 256 threads, so AdamW (4 elements per thread) strides from
2,097,152 elements on and the casts / the add (8 per thread) from 4,194,304.

Criteria (docs/lab_notes.md, "Element-wise float64 tests: AdamW, casts, field projection and split-K"):
  ur_adamw_step / _dev   param, exp_avg and exp_avg_sq each by ref64.assert_f32_close in rows of 64: |got - ref64| <= 8 e32 + 2^-20 row max
                         |ref64|, e32 = the same formula in float32 torch.  Gradients of one power of ten per row, 1e-12 .. 1e3, with exact
                         zeros (v = 0: the denominator is eps); |p| <= 0.1 against steps of lr = 0.05 .. 0.1.
                         *coef == 1.0f is ur_adamw_step bit for bit; *coef == 0 leaves the moments decayed only (exactly b m).
  norm -> coef -> step   ur_grad_norm_clip and ur_adamw_step_dev on one stream against the float64 norm, coefficient and step
  ur_cast_f32_to_bf16    torch's CPU conversion bit for bit (NaN = NaN) over all 65,536 upper halves x 6 low halves
  ur_cast_bf16_to_f32    all 65,536 patterns, bit for bit
  ur_add_bf16            bf16(float32(a) + float32(b)) bit for bit, and within 1 bf16 ulp of the float64 sum
  transposes             bit for bit
Every output buffer is pre-filled with a sentinel and carries guard elements behind its end that must keep their bits.  Every test prints its
worst error / bound ("[ratio] kernel: x")."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ew_cases, ref64  # noqa: E402
from unirec_amd import _lib, hip  # noqa: E402
from unirec_amd._lib import UniRecHipError  # noqa: E402

# entry point -> the primitive-level tests of this module that hold it against a reference (tests/test_abi_test_coverage.py)
COVERS = {
    "ur_adamw_step": ["test_adamw_step_every_element", "test_adamw_refuses_bad_arguments_without_a_launch"],
    "ur_adamw_step_dev": ["test_adamw_step_dev_coefficients", "test_norm_clip_then_step_on_one_stream", "test_adamw_refuses_bad_arguments_without_a_launch"],
    "ur_grad_norm_clip": ["test_norm_clip_then_step_on_one_stream"],
    "ur_cast_f32_to_bf16": ["test_cast_f32_to_bf16_every_upper_half", "test_cast_lengths_and_the_grid_stride_loop"],
    "ur_cast_bf16_to_f32": ["test_cast_bf16_to_f32_every_pattern", "test_cast_lengths_and_the_grid_stride_loop"],
    "ur_add_bf16": ["test_add_bf16_past_the_grid_cap"],
    "ur_transpose_bf16": ["test_transposes_move_every_bit"],
    "ur_transpose_bf16_batched": ["test_transposes_move_every_bit"],
}

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GUARD = 64                           # elements behind every output that must keep their bits
SENT32 = 0x4B4B4B4B                  # 13323083.0f: nothing here computes it
SENT16 = 0x4B4B
H = ew_cases.ADAMW_HYPER
GS = ew_cases.ADAMW_GRAD_SCALE
WORST = {}


def _note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio))
    print(f"[ratio] {kernel}: {float(ratio):.4f}")


def _guarded(t):
    """device copy of the flat tensor t in front of GUARD sentinel elements: (the view of t's length, the whole buffer)"""
    n = t.numel()
    if t.element_size() == 4:
        base = torch.full((n + GUARD,), SENT32, dtype=torch.int32, device=DEV).view(t.dtype)
    else:
        base = torch.full((n + GUARD,), SENT16, dtype=torch.int16, device=DEV).view(t.dtype)
    base[:n] = t.to(DEV)
    return base[:n], base


def _guard_intact(base, n, what):
    ints = base.view(torch.int32 if base.element_size() == 4 else torch.int16)
    assert (ints[n:] == (SENT32 if base.element_size() == 4 else SENT16)).all(), f"{what}: elements behind the end were written"


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _step(n, step, wd, seed, lr, coef=None):
    """one launch on guarded device copies of ew_cases.adamw_inputs; returns (inputs on the CPU, (p, m, v) after the step on the CPU)"""
    cpu = ew_cases.adamw_inputs(n, step, seed)
    (p, pb), (g, gb), (m, mb), (v, vb) = (_guarded(t) for t in cpu)
    hip.adamw_step(p, g, m, v, lr, H["b1"], H["b2"], H["eps"], wd, step, grad_scale=GS, coef=coef)
    torch.cuda.synchronize()
    for b, name in ((pb, "param"), (gb, "grad"), (mb, "exp_avg"), (vb, "exp_avg_sq")):
        _guard_intact(b, n, f"n {n}: {name}")
    assert torch.equal(_bits(g).cpu(), _bits(cpu[1])), "the gradient was modified"
    return cpu, (p.cpu(), m.cpu(), v.cpu())


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("step", ew_cases.ADAMW_STEPS)
def test_adamw_step_every_element(step, wd):
    """the tail alone, one vector, vector + tail, a prime, and 2,097,152 + 3 * 1024 + 3: the grid-stride loop with a ragged end"""
    lr = 0.05 if step % 2 else 0.1
    for n in ew_cases.ADAMW_SIZES:
        cpu, got = _step(n, step, wd, n + step, lr)
        p, g, m, v = cpu
        assert (g == 0).any() or n < 8
        upd = (got[0].double() - p.double() * (1 - lr * wd)).abs()
        assert n < 8 or float(upd.max()) >= 0.9 * lr                       # the step is at least as large as the parameters
        _note("adamw_kernel", ref64.assert_adamw_close(got, p, g, m, v, lr, H["b1"], H["b2"], H["eps"], wd, step, GS, what=f"n {n} step {step} wd {wd}"))


def test_adamw_step_dev_coefficients():
    """*coef == 1.0f: ur_adamw_step's bits; 0.37: the float64 reference; 0 (an infinite norm): the moments are decayed only"""
    step, wd, lr = 10, 0.1, 0.05
    for n in (7, 1021, ew_cases.ADAMW_SIZES[-1]):
        cpu, plain = _step(n, step, wd, n, lr)
        p, g, m, v = cpu
        one = torch.ones((), device=DEV)
        _, dev1 = _step(n, step, wd, n, lr, coef=one)
        for a, b, name in zip(plain, dev1, ("param", "exp_avg", "exp_avg_sq")):
            assert torch.equal(_bits(a), _bits(b)), f"n {n}: {name} differs between ur_adamw_step and ur_adamw_step_dev(*coef = 1)"
        c = torch.full((), 0.37, device=DEV)
        _, got = _step(n, step, wd, n, lr, coef=c)
        _note("adamw_kernel<dev>", ref64.assert_adamw_close(got, p, g, m, v, lr, H["b1"], H["b2"], H["eps"], wd, step, GS, coef=0.37, what=f"n {n} coef 0.37"))
        _, got0 = _step(n, step, wd, n, lr, coef=torch.zeros((), device=DEV))
        _note("adamw_kernel<dev>", ref64.assert_adamw_close(got0, p, g, m, v, lr, H["b1"], H["b2"], H["eps"], wd, step, GS, coef=0.0, what=f"n {n} coef 0"))
        b1, b2 = torch.tensor(H["b1"], dtype=F32), torch.tensor(H["b2"], dtype=F32)
        assert torch.equal(got0[1], b1 * m) and torch.equal(got0[2], b2 * v), f"n {n}: a zero coefficient must leave the moments decayed only"


def test_adamw_refuses_bad_arguments_without_a_launch():
    n = 1021
    cpu = ew_cases.adamw_inputs(n, 2, 1)
    bufs = [_guarded(t) for t in cpu]
    before = [b.clone() for _, b in bufs]
    (p, _), (g, _), (m, _), (v, _) = bufs
    coef = torch.ones((), device=DEV)
    args = (0.05, H["b1"], H["b2"], H["eps"], 0.1)
    for c in (None, coef):
        with pytest.raises(UniRecHipError, match="step >= 1"):
            hip.adamw_step(p, g, m, v, *args, 0, grad_scale=GS, coef=c)
        with pytest.raises(UniRecHipError, match="misaligned"):
            hip.adamw_step(p[1:], g[1:], m[1:], v[1:], *args, 2, grad_scale=GS, coef=c)
        with pytest.raises(UniRecHipError, match="misaligned"):
            hip.adamw_step(p[:-1], g[:-1], m[1:], v[:-1], *args, 2, grad_scale=GS, coef=c)
    lib = _lib.load()
    rc = lib.ur_adamw_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, *args, 2, GS, 0, hip._stream())
    assert rc < 0 and b"coef" in lib.ur_last_error()
    rc = lib.ur_adamw_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, *args, 2, GS, coef.data_ptr() + 2, hip._stream())
    assert rc < 0 and b"coef" in lib.ur_last_error()
    torch.cuda.synchronize()
    for (_, b), b0 in zip(bufs, before):
        assert torch.equal(_bits(b), _bits(b0)), "a refused call wrote"


def test_norm_clip_then_step_on_one_stream():
    """ur_grad_norm_clip over two ranges (one longer than UR_NORM_BLOCK_ELEMS with a ragged last piece), then ur_adamw_step_dev on each with
    the coefficient still on the device: float64 norm -> coefficient -> step.  The float32 yardstick forms its own norm and coefficient."""
    step, wd, lr, scale = 2, 0.1, 0.05, 0.5
    sizes = (2 * _lib.NORM_BLOCK_ELEMS + 1000 + 3, 1021)
    cpus = [ew_cases.adamw_inputs(n, step, 40 + i) for i, n in enumerate(sizes)]
    g64 = torch.cat([c[1].double() for c in cpus])
    norm64 = float(g64.pow(2).sum().sqrt()) * scale
    max_norm = 0.25 * norm64                                               # clips: coef about 0.25
    f = lambda x: torch.tensor(x, dtype=F32)      # noqa: E731
    norm32 = torch.cat([c[1] for c in cpus]).pow(2).sum().sqrt() * f(scale)
    coef32 = float(torch.clamp(f(max_norm) / (norm32 + f(1e-6)), max=1.0))
    norm64 = float(g64.pow(2).sum().sqrt()) * float(f(scale))
    coef64 = min(float(f(max_norm)) / (norm64 + float(f(1e-6))), 1.0)
    dev = [[_guarded(t) for t in c] for c in cpus]
    out_norm, out_coef = torch.zeros((), device=DEV), torch.zeros((), device=DEV)
    hip.grad_norm_clip([d[1][0] for d in dev], scale, max_norm, out_norm, out_coef)
    for d in dev:
        hip.adamw_step(d[0][0], d[1][0], d[2][0], d[3][0], lr, H["b1"], H["b2"], H["eps"], wd, step, grad_scale=scale, coef=out_coef)
    torch.cuda.synchronize()
    _note("norm_finish_kernel (norm)", ref64.assert_f32_close(out_norm, torch.tensor(norm64, dtype=F64), norm32, scale=abs(norm64), what="norm"))
    _note("norm_finish_kernel (coef)", ref64.assert_f32_close(out_coef, torch.tensor(coef64, dtype=F64), torch.tensor(coef32), scale=abs(coef64), what="coef"))
    assert 0.2 < coef64 < 0.3
    for i, (c, d) in enumerate(zip(cpus, dev)):
        n = sizes[i]
        for (_, b), name in zip(d, ("param", "grad", "exp_avg", "exp_avg_sq")):
            _guard_intact(b, n, f"range {i}: {name}")
        got = (d[0][0].cpu(), d[2][0].cpu(), d[3][0].cpu())
        _note("norm -> coef -> adamw_kernel<dev>", ref64.assert_adamw_close(got, *c, lr, H["b1"], H["b2"], H["eps"], wd, step, scale, coef=coef64, coef32=coef32,
                                                                           what=f"range {i}"))


# ---- casts ---------------------------------------------------------------------------------------------------------------------
def _cast_down(x_cpu):
    n = x_cpu.numel()
    src = x_cpu.to(DEV)
    dst, base = _guarded(torch.zeros(n, dtype=BF16))
    _bits(base)[:n] = SENT16
    hip.cast_f32_to_bf16(src, dst)
    torch.cuda.synchronize()
    _guard_intact(base, n, f"cast_f2b n {n}")
    return dst.cpu()


def _cast_up(b_cpu):
    n = b_cpu.numel()
    src = b_cpu.to(DEV)
    dst, base = _guarded(torch.zeros(n, dtype=F32))
    _bits(base)[:n] = SENT32
    hip.cast_bf16_to_f32(src, dst)
    torch.cuda.synchronize()
    _guard_intact(base, n, f"cast_b2f n {n}")
    return dst.cpu()


def test_cast_f32_to_bf16_every_upper_half():
    """ties to even, the carry into the exponent, overflow to infinity, subnormals, both zeros, infinities and NaN: 6 x 65,536 words"""
    x = ew_cases.cast_patterns()
    _note("cast_f2b_kernel", ref64.assert_bf16_bits(_cast_down(x), ref64.cast_f32_to_bf16(x), "every upper half"))
    # the same words through the tail loop (n % 8 elements, one element at a time: f2bf, not pack_bf2)
    tail = x[torch.arange(0, x.numel(), 8 * 31)][:7 * 120].reshape(-1, 7)
    for row in tail[:24]:
        ref64.assert_bf16_bits(_cast_down(row.contiguous()), ref64.cast_f32_to_bf16(row), "tail loop")


def test_cast_bf16_to_f32_every_pattern():
    b = ew_cases.bf16_patterns()
    want = b.view(torch.int16).to(torch.int32) << 16
    assert torch.equal(_bits(_cast_up(b)), want)
    for k in (1, 7):                                                       # the tail loop
        assert torch.equal(_bits(_cast_up(b[0x7F7A:0x7F7A + k].contiguous())), want[0x7F7A:0x7F7A + k])
    _note("cast_b2f_kernel", 0.0)


def test_cast_lengths_and_the_grid_stride_loop():
    """1, 7, 8, 9 and 4,194,304 + 2 * 2048 + 5 elements: the last enters the grid-stride loop and ends in the tail loop"""
    words = ew_cases.cast_patterns()
    for n in ew_cases.CAST_SIZES:
        idx = (torch.arange(n) * 37) % words.numel()                       # 37 is coprime to 6 * 65536: every word, in a scattered order
        x = words[idx].contiguous()
        down = _cast_down(x)
        ref64.assert_bf16_bits(down, ref64.cast_f32_to_bf16(x), f"f32 -> bf16, n {n}")
        up = _cast_up(down)
        assert torch.equal(_bits(up), _bits(down).to(torch.int32) << 16), f"bf16 -> f32, n {n}"


def test_add_bf16_past_the_grid_cap():
    n = ew_cases.ADD_SIZE
    a, b = ew_cases.add_operands(n, 5)
    out, base = _guarded(torch.zeros(n, dtype=BF16))
    _bits(base)[:n] = SENT16
    hip.add_bf16(a.to(DEV), b.to(DEV), out)
    torch.cuda.synchronize()
    _guard_intact(base, n, "add_bf16")
    want, s64 = ref64.add_bf16(a, b)
    got = out.cpu()
    ref64.assert_bf16_bits(got, want, "bf16(float32(a) + float32(b))")
    _note("add_kernel", ref64.assert_within_ulps(got, s64, 1, 0.0, "against the float64 sum"))
    small = hip.add_bf16(a[:8].to(DEV), b[:8].to(DEV))
    ref64.assert_bf16_bits(small.cpu(), want[:8], "one vector")
    with pytest.raises(UniRecHipError, match="multiple of 8"):
        hip.add_bf16(a[:7].to(DEV), b[:7].to(DEV))


# ---- transposes ------------------------------------------------------------------------------------------------------------------
TRANSPOSE_SHAPES = [(1, 1), (1, 5), (33, 70), (32, 32), (16, 1024), (100, 31), (2048, 16)]


def test_transposes_move_every_bit():
    """every bf16 pattern (NaNs included: bits are compared), tiles with ragged edges in both directions; one launch per matrix and all in one"""
    pats = ew_cases.bf16_patterns()
    srcs = []
    for i, (r, c) in enumerate(TRANSPOSE_SHAPES):
        idx = (torch.arange(r * c) * 37 + 1000 * i) % 65536
        srcs.append(pats[idx].reshape(r, c).contiguous().to(DEV))
    for s in srcs:
        r, c = s.shape
        dst, base = _guarded(torch.zeros(r * c, dtype=BF16))
        _bits(base)[:r * c] = SENT16
        hip.transpose_bf16(s, dst.view(c, r))
        torch.cuda.synchronize()
        _guard_intact(base, r * c, f"transpose {r} x {c}")
        assert torch.equal(_bits(dst.view(c, r)), _bits(s).t().contiguous()), f"transpose {r} x {c}"
    bt = hip.BatchedTranspose(srcs)
    for s, o in zip(srcs, bt.run()):
        assert tuple(o.shape) == (s.shape[1], s.shape[0]) and torch.equal(_bits(o), _bits(s).t().contiguous()), f"batched transpose {tuple(s.shape)}"
    _note("transpose_kernel", 0.0)
