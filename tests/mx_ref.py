"""Float64 NumPy model of the MX quantization and decode rules (docs/API.md,
"MX storage") and the input set of the MX tests. Independent of
``ddstore_amd/mx.py``: powers of two and round-to-nearest-even are exact in
float64, so every comparison against it is bit for bit."""
import functools

import numpy as np

ELEMS = ("e4m3", "e5m2", "e2m1")
# exponent bits, mantissa bits, bias, largest finite value, emax
FMT = {"e4m3": (4, 3, 7, 448.0, 8), "e5m2": (5, 2, 15, 57344.0, 15),
       "e2m1": (2, 1, 1, 6.0, 2)}


def row_bytes(disp, elem):
    nblk = -(-disp // 32)
    return (nblk * (16 if elem == "e2m1" else 32) + nblk + 15) // 16 * 16


def _encode(x, elem):
    """Finite float64 -> element codes: nearest even, subnormals, saturating."""
    eb, mb, bias, vmax, _ = FMT[elem]
    a = np.minimum(np.abs(x), vmax)
    # binade of a; zero and the subnormals share the first one
    E = np.where(a == 0, 1 - bias, np.maximum(np.frexp(a)[1] - 1, 1 - bias))
    r = np.rint(a / np.ldexp(1.0, E - mb))            # exact division, ties to even
    mag = ((E + bias - 1) * (1 << mb) + r).astype(np.uint8)   # a carry moves up a binade
    return mag | (np.signbit(x).astype(np.uint8) << (eb + mb))


def quantize(x, elem):
    """(n, disp) float array -> (n, row_bytes) uint8 packed rows."""
    n, disp = x.shape
    nblk = -(-disp // 32)
    v = np.zeros((n, nblk * 32))
    v[:, :disp] = x.astype(np.float64)
    v = v.reshape(n, nblk, 32)
    bad = ~np.isfinite(v).all(-1)
    amax = np.where(bad, 1.0, np.abs(np.nan_to_num(v)).max(-1))
    X = np.clip(np.frexp(np.where(amax == 0, 1.0, amax))[1] - 1 - FMT[elem][4], -127, 127)
    sb = np.where(bad, 255, np.where(amax == 0, 0, X + 127))
    scaled = np.where(bad[..., None], 0.0, np.ldexp(np.nan_to_num(v), 127 - sb[..., None]))
    codes = _encode(scaled, elem).reshape(n, -1)
    if elem == "e2m1":
        codes = codes[:, 0::2] | (codes[:, 1::2] << 4)
    out = np.zeros((n, row_bytes(disp, elem)), np.uint8)
    out[:, :codes.shape[1]] = codes
    out[:, codes.shape[1]:codes.shape[1] + nblk] = sb
    return out


def decode(packed, disp, elem):
    """(n, row_bytes) uint8 -> (n, disp) float32 (exact by the contract)."""
    eb, mb, bias, _, _ = FMT[elem]
    n = packed.shape[0]
    nblk = -(-disp // 32)
    npay = nblk * (16 if elem == "e2m1" else 32)
    c = packed[:, :npay]
    if elem == "e2m1":
        c = np.stack([c & 15, c >> 4], -1).reshape(n, -1)
    c = c.astype(np.int64)
    f, m = (c >> mb) & ((1 << eb) - 1), c & ((1 << mb) - 1)
    v = np.where(f == 0, np.ldexp(m.astype(np.float64), 1 - bias - mb),
                 np.ldexp((m + (1 << mb)).astype(np.float64), f - bias - mb))
    v = np.where((c >> (eb + mb)) & 1, -v, v).reshape(n, nblk, 32)
    sb = packed[:, npay:npay + nblk].astype(np.int64)[..., None]
    v = np.where(sb == 255, np.nan, np.ldexp(v, sb - 127))
    return v.reshape(n, -1)[:, :disp].astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(n, disp):
    """(n, disp) float32, row-major blocks of 32 cycling through: amax a power
    of two; amax just below one (1.99, 509/256: saturating); element
    midpoints; element subnormals; all zero with -0.0; f32 subnormals; 3e38;
    one NaN; one inf; magnitudes 2^20 apart; random. Built once per shape."""
    rng = np.random.default_rng(1234)
    nblk = -(-disp // 32)
    x = np.zeros((n, nblk * 32), np.float32)
    blocks = x.reshape(-1, 32)
    grid = np.concatenate([np.arange(0, 64) / 64.0, np.arange(64, 1024, 8) / 64.0])
    for i in range(blocks.shape[0]):
        u = rng.uniform(-1, 1, 32)
        k = i % 11
        scale = np.float64(2.0) ** rng.integers(-30, 30)
        if k == 0:
            b = u * 0.9; b[3] = -1.0
        elif k == 1:
            b = u; b[5] = 1.99; b[6] = 509 / 256; b[7] = -1.75
        elif k == 2:    # every quarter step up to 1, then eighths: ties of all kinds
            b = rng.choice(grid, 32) * rng.choice([-1, 1], 32); b[0] = 8.0
        elif k == 3:    # far below amax: element subnormals and round-to-zero
            b = u * 2.0 ** rng.integers(-12, -2, 32); b[1] = 1.5
        elif k == 4:
            b = np.zeros(32); b[2] = -0.0; b[9] = -0.0; scale = 1.0
        elif k == 5:
            b = u * 1e-40; b[4] = 1e-45; scale = 1.0
        elif k == 6:
            b = u * 1e30; b[8] = 3e38; scale = 1.0
        elif k == 7:
            b = u; b[11] = np.nan
        elif k == 8:
            b = u; b[12] = -np.inf
        elif k == 9:
            b = u * np.where(np.arange(32) % 2, 1.0, 2.0 ** -20)
        else:
            b = u * 2.0 ** rng.integers(-6, 6, 32)
        with np.errstate(over="ignore"):
            blocks[i] = (b * scale).astype(np.float32)
    out = np.ascontiguousarray(x[:, :disp])
    out.setflags(write=False)
    return out
