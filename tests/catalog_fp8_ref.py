"""The rule of include/unirec_fp8.h restated on the host, in numpy and torch on the CPU, for the CPU and the GPU tests.

    a      = max_d |x_nd|                                   (bf16 widened exactly)
    e      = 0 if a == 0 or a is not finite; else with a = m 2^x, m in [0.5, 1): 9 - x if m <= 0.875 else 8 - x; clamped to [-64, 64]
    scale  = 2^-e
    code   = torch.tensor(x * 2^e, dtype=float32).to(torch.float8_e4m3fn)           (nearest even, subnormals, signed zero)
    inv    = 1 / max(|codes.float()|, 1e-12) in the f32 chain of the row-norm kernel (lane l of 64: x^2 + y^2 + z^2 + w^2 of its pieces at
             d = 4 l + 256 i, ascending i; the xor-shuffle sum 32, 16, .. 1; sqrt; max; one division)
    s64    = float64(q . c) * float64(iu8) * float64(inv)      the fp8 shortlist score, with the planes above
    bound  = ((D + 2) 2^-23 sum_d |q_d c_d|) iu8 inv + 2^-22 |s64|

The decode table is written from the format (1 sign, 4 exponent bits of bias 7, 3 mantissa bits, subnormals m 2^-9, 0x7f / 0xff NaN), not
from torch; tests/test_catalog_fp8_host.py holds it to torch's view.  Nothing here runs on a device or touches the library."""
import numpy as np
import torch

F32 = np.float32


def decode_table():
    """float32 [256]: the value of every e4m3fn code"""
    t = np.zeros(256, dtype=np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        v = m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7)
        if (c & 0x7f) == 0x7f:
            v = np.nan
        t[c] = -v if c & 0x80 else v
    return t.astype(F32)


DECODE = decode_table()


def decode(codes):
    """uint8 [...] -> float32 [...]"""
    return DECODE[np.asarray(codes, dtype=np.uint8)]


def row_exponent(a):
    """int32 [...]: e of the rule for the row maxima a (float32, non-negative)"""
    a = np.asarray(a, dtype=F32)
    m, x = np.frexp(a.astype(np.float64))                      # exact: a float32 is a float64
    e = np.where(m <= 0.875, 9 - x, 8 - x)
    e = np.clip(e, -64, 64)
    return np.where((a == 0) | ~np.isfinite(a), 0, e).astype(np.int32)


def row_exponent_by_search(a):
    """the largest e in [-64, 64] with a * 2^e <= 448, by trying them all in float64 (exact); for a finite a > 0"""
    a = float(a)
    best = -64
    for e in range(-64, 65):
        if a * 2.0 ** e <= 448.0:
            best = e
    return best


def encode(v):
    """float32 [...] -> uint8 [...]: torch's CPU conversion to float8_e4m3fn, as bit patterns"""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=F32)))
    return t.to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def row_inv_norm(values):
    """float32 [N]: the row-norm kernel's chain on float32 rows [N, D] (D a multiple of 4), every operation rounded to float32"""
    v = np.asarray(values, dtype=F32)
    N, D = v.shape
    pad = (-D) % 256
    sq = np.pad(v, ((0, 0), (0, pad))).reshape(N, -1, 64, 4)   # [row, i, lane, element]: zero pieces add nothing
    sq = sq * sq
    s = np.zeros((N, 64), dtype=F32)
    for i in range(sq.shape[1]):
        s = s + (((sq[:, i, :, 0] + sq[:, i, :, 1]) + sq[:, i, :, 2]) + sq[:, i, :, 3])
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    assert s.dtype == F32
    return (F32(1.0) / np.maximum(np.sqrt(s[:, 0]), F32(1e-12))).astype(F32)


def quantize(x):
    """x: torch [N, D] float32 or bfloat16 (CPU) -> (codes uint8 [N, D], scale float32 [N], inv float32 [N]) as numpy arrays"""
    xf = torch.as_tensor(x).detach().cpu().to(torch.float32).numpy()
    a = np.abs(xf).max(axis=1) if xf.shape[1] else np.zeros(xf.shape[0], dtype=F32)
    e = row_exponent(a)
    up = np.ldexp(F32(1.0), e).astype(F32)
    codes = encode(xf * up[:, None])                           # a float32 product, as the rule says
    scale = np.ldexp(F32(1.0), -e).astype(F32)
    return codes, scale, row_inv_norm(decode(codes))


def dequantize(codes, scale):
    """float32 [N, D]: codes.float() * scale[:, None], exact"""
    return decode(codes) * np.asarray(scale, dtype=F32)[:, None]


def scores64(q, iu8, c, inv):
    """(s64 float64 [B, N], bound float64 [B, N]) for user codes q [B, D] with iu8 [B] and catalogue codes c [N, D] with inv [N]"""
    qv, cv = decode(q).astype(np.float64), decode(c).astype(np.float64)
    D = qv.shape[1]
    w = np.asarray(iu8, dtype=np.float64)[:, None] * np.asarray(inv, dtype=np.float64)[None, :]
    s = (qv @ cv.T) * w
    bound = (D + 2) * 2.0 ** -23 * (np.abs(qv) @ np.abs(cv).T) * w + 2.0 ** -22 * np.abs(s)
    return s, bound


def exact_scores64(user, c):
    """float64 [B, N]: the cosine of the f32 user with the code values of every row (what the fp8 re-rank scores)"""
    u = np.asarray(torch.as_tensor(user).detach().cpu().to(torch.float64).numpy())
    cv = decode(c).astype(np.float64)
    iu = 1.0 / np.maximum(np.sqrt((u * u).sum(1)), 1e-12)
    ic = 1.0 / np.maximum(np.sqrt((cv * cv).sum(1)), 1e-12)
    return (u @ cv.T) * iu[:, None] * ic[None, :]
