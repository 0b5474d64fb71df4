"""MX (OCP microscaling v1.0) block-scaled rows in plain torch.

The public helper for the packed row format of ``DDStore.add_mx`` (docs/API.md,
"MX storage") and the host backend of those calls. 32 consecutive values share
one power-of-two scale byte (E8M0); the elements are e4m3 / e5m2 bytes or e2m1
nibbles. A packed row is::

    [nblk * 32 element codes][nblk scale bytes][zero pad to a multiple of 16 B]

Not a hot path: the GPU store quantizes and dequantizes in its own kernels.
"""
import os

import torch

ELEMS = ("e4m3", "e5m2", "e2m1")
BLOCK = 32
# elem -> (emax, largest finite value, torch dtype of a code byte)
_FMT = {
    "e4m3": (8, 448.0, torch.float8_e4m3fn),
    "e5m2": (15, 57344.0, torch.float8_e5m2),
    "e2m1": (2, 6.0, None),
}
_E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float32)

# ``update_mx`` of a host array on a GPU store stages it in pieces of at most
# this many source bytes, so the device never holds more of the source than
# one piece (DDSTORE_MX_STAGE_BYTES; default 64 MiB).
STAGE_BYTES = int(os.environ.get("DDSTORE_MX_STAGE_BYTES", str(64 << 20)))


def _ldexp(x: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """x * 2^e in float64 (exact for every use here)."""
    return x * torch.pow(torch.tensor(2.0, dtype=torch.float64), e.to(torch.float64))


def _check(elem: str) -> None:
    if elem not in _FMT:
        raise ValueError(f"ddstore mx: unknown element kind '{elem}' (one of {ELEMS})")


def row_bytes(disp: int, elem: str) -> int:
    """Bytes of one packed row of logical width ``disp``."""
    _check(elem)
    nblk = -(-int(disp) // BLOCK)
    payload = nblk * (16 if elem == "e2m1" else 32)
    return (payload + nblk + 15) // 16 * 16


def quantize(t: torch.Tensor, elem: str = "e4m3") -> torch.Tensor:
    """``(n, disp)`` f32/f16/bf16 -> ``(n, row_bytes)`` uint8 packed rows."""
    _check(elem)
    t = torch.as_tensor(t)
    if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"ddstore mx: quantize takes f32/f16/bf16, got {t.dtype}")
    if t.dim() != 2:
        raise ValueError("ddstore mx: quantize takes an (n, disp) array")
    emax, vmax, fdt = _FMT[elem]
    n, disp = t.shape
    nblk = -(-disp // BLOCK)
    x = torch.zeros((n, nblk * BLOCK), dtype=torch.float64)
    x[:, :disp] = t.detach().cpu().to(torch.float64)   # exact
    x = x.view(n, nblk, BLOCK)
    bad = ~torch.isfinite(x).all(-1)
    amax = x.abs().amax(-1)
    zero = amax == 0
    # frexp: amax = m * 2^e with m in [0.5, 1), so floor(log2(amax)) = e - 1
    e = torch.frexp(torch.where(bad | zero, torch.ones_like(amax), amax))[1]
    X = (e.to(torch.int64) - 1 - emax).clamp(-127, 127)
    sb = torch.where(bad, 255, torch.where(zero, 0, X + 127))
    X = sb - 127                                        # zero block: 2^-127
    scaled = _ldexp(x, (-X).unsqueeze(-1))              # exact in float64
    scaled = torch.where(bad.unsqueeze(-1), torch.zeros_like(scaled), scaled)
    scaled = scaled.clamp(-vmax, vmax)                  # saturate, keeps -0.0
    if fdt is not None:
        codes = scaled.to(torch.float32).to(fdt).view(torch.uint8)
    else:
        a = scaled.abs()
        mag = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75)
               + (a > 2.5) + (a >= 3.5) + (a > 5.0))    # ties to the even code
        c = mag | (torch.signbit(scaled).to(torch.uint8) << 3)
        c = c.view(n, nblk, BLOCK // 2, 2)
        codes = c[..., 0] | (c[..., 1] << 4)            # even column low
    out = torch.zeros((n, row_bytes(disp, elem)), dtype=torch.uint8)
    pay = codes.reshape(n, -1)
    out[:, :pay.shape[1]] = pay
    out[:, pay.shape[1]:pay.shape[1] + nblk] = sb.to(torch.uint8)
    return out


def dequantize(packed: torch.Tensor, disp: int, elem: str = "e4m3") -> torch.Tensor:
    """``(n, row_bytes)`` uint8 packed rows -> ``(n, disp)`` float32."""
    _check(elem)
    packed = torch.as_tensor(packed).cpu()
    if packed.dtype != torch.uint8 or packed.dim() != 2 \
            or packed.shape[1] != row_bytes(disp, elem):
        raise ValueError("ddstore mx: dequantize takes (n, row_bytes) uint8 rows")
    n = packed.shape[0]
    nblk = -(-disp // BLOCK)
    fdt = _FMT[elem][2]
    npay = nblk * (16 if fdt is None else 32)
    pay = packed[:, :npay].contiguous()
    if fdt is not None:
        val = pay.view(fdt).to(torch.float32)
    else:
        nib = torch.stack([pay & 15, pay >> 4], dim=-1).reshape(n, -1).to(torch.int64)
        val = _E2M1[nib & 7] * (1.0 - 2.0 * (nib >> 3).to(torch.float32))
    sb = packed[:, npay:npay + nblk].to(torch.int64)
    out = _ldexp(val.to(torch.float64).view(n, nblk, BLOCK), (sb - 127).unsqueeze(-1))
    out = torch.where((sb == 255).unsqueeze(-1), torch.full_like(out, float("nan")), out)
    return out.view(n, -1)[:, :disp].to(torch.float32).contiguous()
