"""Float64 reference of the LoRA merge (ur_lora_merge, include/unirec_hip_adapter.h) and the bound its outputs are held to.

    ref[o,i] = W[o,i] + scale * sum_k B[o,k] A[k,i]            S[o,i] = sum_k |B[o,k] A[k,i]|

The kernel's arithmetic is one fmaf per k in ascending order (r roundings, each at most 2^-24 of a partial sum that |.| bounds by S)
and one final fmaf(scale, acc, W) (one rounding, 2^-24 of the result); the bf16 output adds one round-to-nearest-even:

    f32 output:   |got - ref| <= 2^-24 |ref| + r 2^-24 |scale| S
    bf16 output:  the f32 bound plus half a bf16 ulp of |ref|

Derived from the number formats, not measured.  (The bf16 rounding acts on the f32 value, not on ref: where the two sit in different
binades the half ulp is that of the f32 value, at most 2^-9 of the f32 error more -- far inside the slack between the worst-case chain
bound and what r roundings of mixed sign give.)"""
import torch

F64 = torch.float64
U32 = 2.0 ** -24


def merge_terms(W, A, B):
    """(B A, S) in float64: shared by both signs of the scale"""
    A64, B64 = A.to(F64), B.to(F64)
    return B64 @ A64, B64.abs() @ A64.abs()


def lora_merge_ref(W, A, B, scale, terms=None):
    """(ref, f32 bound, bf16 bound), float64 [out, in]"""
    BA, S = merge_terms(W, A, B) if terms is None else terms
    ref = W.to(F64) + float(scale) * BA
    b32 = U32 * ref.abs() + A.shape[0] * U32 * abs(float(scale)) * S
    return ref, b32, b32 + bf16_half_ulp(ref)


def bf16_half_ulp(x):
    """half the spacing of bf16 (8 significand bits, f32's exponent range) at |x|; 0 at 0"""
    _, e = torch.frexp(x.abs().to(F64))                    # |x| = m 2^e, m in [0.5, 1): the binade's ulp is 2^(e - 8)
    half = torch.ldexp(torch.ones_like(x, dtype=F64), e.clamp_min(-125) - 9)
    return torch.where(x == 0, torch.zeros_like(half), half)


def merge_inputs(out_rows, in_cols, r, seed):
    """W, A, B f32: signed magnitudes 2^-20 .. 2^8 (log-uniform), a tenth of the entries zero, row 1 of A and column 2 of B all zero"""
    g = torch.Generator().manual_seed(seed)

    def draw(*shape):
        mag = torch.exp2(torch.rand(shape, generator=g, dtype=F64) * 28.0 - 20.0)
        sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).to(F64)
        keep = (torch.rand(shape, generator=g) >= 0.1).to(F64)
        return (mag * sign * keep).to(torch.float32)
    W, A, B = draw(out_rows, in_cols), draw(r, in_cols), draw(out_rows, r)
    A[1, :] = 0.0
    B[:, 2] = 0.0
    return W, A, B
