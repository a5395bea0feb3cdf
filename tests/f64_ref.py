"""Exact float64 helpers shared by the float64-reference kernel tests (test_gpu_conv3.py, test_gpu_linear.py): roundings of a float64
value to the engine's storage formats, in one rounding each, and the decoders of the formats that torch has no dtype for."""
import torch


def pow2(k: torch.Tensor) -> torch.Tensor:
    """2^k as float64, exactly (built from the exponent bits; torch.ldexp goes through a float32 pow on the device)."""
    return ((k.to(torch.int64) + 1023) << 52).view(torch.float64)


def rne_bf16(r: torch.Tensor) -> torch.Tensor:
    """float64 -> the float64 value of its bf16 rounding to nearest even (8 significant bits), in one rounding."""
    m, e = torch.frexp(r)
    return torch.round(m * 256.0) * pow2(e - 8)


def bf16q(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).float()


def rne_e4m3(r: torch.Tensor) -> torch.Tensor:
    """float64 -> the float64 value of its OCP e4m3 rounding (common.h f2e4m3, v_cvt_pk_fp8_f32): round to nearest even with 4
    significant bits, multiples of 2^-9 below the smallest normal 2^-6, saturated at +-448."""
    a = r.clamp(-448.0, 448.0)
    m, e = torch.frexp(a)                                  # a = m 2^e, 0.5 <= |m| < 1
    q = torch.where(a.abs() < 2.0 ** -6, torch.round(a * 512.0) / 512.0, torch.round(m * 16.0) * pow2(e - 4))
    return q.clamp(-448.0, 448.0)


def e4m3_value(b: torch.Tensor) -> torch.Tensor:
    """raw e4m3 bytes (uint8) -> float64 (common.h e4m32f; 0x7f / 0xff are NaN)."""
    b = b.to(torch.int64)
    e, m = (b >> 3) & 15, b & 7
    a = torch.where(e == 0, m.double() / 512.0, (8 + m).double() * pow2(e - 10))
    a = torch.where((b & 0x7f) == 0x7f, torch.full_like(a, float("nan")), a)
    return torch.where((b & 0x80) != 0, -a, a)


def bx3_value(u: torch.Tensor) -> torch.Tensor:
    """A matrix in the bf16x3 unit format (rows of 32-byte units of 8 elements, [8 x bf16 hi | 8 x bf16 lo], common.h), given as its
    raw 4-byte words [..., n] (n a multiple of 8) -> float64 hi + lo, [..., n]."""
    h = u.contiguous().view(torch.int16).view(*u.shape[:-1], u.shape[-1] // 8, 2, 8)
    hi = (h[..., 0, :].to(torch.int32) << 16).view(torch.float32).double()
    lo = (h[..., 1, :].to(torch.int32) << 16).view(torch.float32).double()
    return (hi + lo).reshape(*u.shape)
