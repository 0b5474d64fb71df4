"""Exact model of the store's dtype cast, and the input tables it is run over.

The contract (docs/API.md, "Cast semantics"): a fetch with a different output
dtype returns what the host backend returns, torch's CPU ``Tensor.to(dtype)``.
This file derives the same numbers a second time, from the number formats
alone: NumPy integer arithmetic on bit patterns, plus float64 arithmetic in
the affine model. It calls no f16/bf16/fp8 conversion of NumPy, torch or
ml_dtypes and no ``Tensor.to``; ``tests/test_cast_ref_cpu.py`` proves it equal
to torch's CPU cast pair by pair.

Values travel as bit patterns: uint8 for u8 and the fp8s, uint16 for f16 and
bf16, uint32 / uint64 for f32 / f64, int32 / int64 for the integers.

The rules:
  * every float target rounds to nearest, ties to even, keeps subnormals and
    the sign of zero; overflow gives inf (NaN for e4m3fn, which has no inf and
    turns inf into NaN too);
  * a float target narrower than f32 is reached THROUGH f32, so an input that
    f32 does not hold exactly (f64, i64, i32) is rounded twice;
  * int -> f32 / f64 is one rounding of the exact integer;
  * int -> narrower int keeps the low bits;
  * float -> int truncates toward zero and is defined only for a finite input
    whose truncated value the target holds -- the only undefined class;
  * affine is fma(x_f32, scale, shift) rounded ONCE to f32, then cast.
"""
import fractions

import numpy as np

KINDS = ("u8", "i32", "i64", "f32", "f64", "f16", "bf16", "e4m3", "e5m2")
INT_KINDS = ("u8", "i32", "i64")
FLOAT_KINDS = ("f32", "f64", "f16", "bf16", "e4m3", "e5m2")

# float formats: (exponent bits, mantissa bits, has inf / IEEE NaNs)
FMT = {
    "f16": (5, 10, True),
    "bf16": (8, 7, True),
    "e5m2": (5, 2, True),
    "e4m3": (4, 3, False),   # OCP e4m3fn: no inf, NaN is S.1111.111 only
    "f32": (8, 23, True),
    "f64": (11, 52, True),
}
# integer ranges
IRANGE = {"u8": (0, 255), "i32": (-2**31, 2**31 - 1), "i64": (-2**63, 2**63 - 1)}
# storage dtype of a kind's bit patterns
BITS = {"u8": np.uint8, "i32": np.int32, "i64": np.int64, "f32": np.uint32,
        "f64": np.uint64, "f16": np.uint16, "bf16": np.uint16,
        "e4m3": np.uint8, "e5m2": np.uint8}

_U = np.uint64


def _bitlen(m):
    """Bit length of every uint64 in m."""
    x = m.astype(_U)
    bl = np.zeros(x.shape, np.int64)
    for k in (32, 16, 8, 4, 2, 1):
        big = (x >> _U(k)) != 0
        bl += np.where(big, k, 0)
        x = np.where(big, x >> _U(k), x)
    return bl + (x != 0)


def _shl(m, s):
    return m << s.astype(_U)


def _shr(m, s):
    return m >> s.astype(_U)


def decode(bits, kind):
    """Bit patterns -> (sign, M, e, isnan, isinf): the value is
    (-1)^sign * M * 2^e with M a uint64, for every pattern that is a number."""
    if kind in INT_KINDS:
        v = np.asarray(bits).astype(np.int64)
        sign = v < 0
        mag = v.astype(_U)
        mag = np.where(sign, (~mag) + _U(1), mag)   # |v|, 2^63 included
        z = np.zeros(v.shape, bool)
        return sign, mag, np.zeros(v.shape, np.int64), z, z.copy()
    eb, mb, ieee = FMT[kind]
    b = np.asarray(bits).astype(_U)
    bias = (1 << (eb - 1)) - 1
    sign = ((b >> _U(eb + mb)) & _U(1)) != 0
    ef = ((b >> _U(mb)) & _U((1 << eb) - 1)).astype(np.int64)
    mant = b & _U((1 << mb) - 1)
    emax = (1 << eb) - 1
    if ieee:
        isnan = (ef == emax) & (mant != 0)
        isinf = (ef == emax) & (mant == 0)
    else:
        isnan = (ef == emax) & (mant == _U((1 << mb) - 1))
        isinf = np.zeros(b.shape, bool)
    M = np.where(ef == 0, mant, mant | _U(1 << mb))
    e = np.where(ef == 0, 1, ef) - bias - mb
    special = isnan | isinf
    M = np.where(special, _U(0), M)
    return sign, M, e.astype(np.int64), isnan, isinf


def round_to_format(sign, M, e, isnan, isinf, kind):
    """(-1)^sign * M * 2^e rounded once, to nearest even, to float format
    `kind`; returns its bit patterns (uint64). Serves every float format."""
    eb, mb, ieee = FMT[kind]
    bias = (1 << (eb - 1)) - 1
    emin = 1 - bias
    top = (1 << eb) - 1                       # all-ones exponent field
    inf_bits = _U(top << mb)
    if ieee:
        over_bits = inf_bits                  # overflow and inf -> inf
        nan_bits = inf_bits | _U(1 << (mb - 1))
    else:
        over_bits = _U((top << mb) | ((1 << mb) - 1))   # -> NaN
        nan_bits = over_bits
    bl = _bitlen(M)
    E = bl - 1 + e                            # value in [2^E, 2^(E+1))
    # anything this large overflows whatever its mantissa; clipping keeps the
    # shifts below in range
    huge = E > (top - bias + 1)
    E = np.minimum(E, top - bias + 1)
    Ec = np.maximum(E, emin)
    q = Ec - mb                               # result is a multiple of 2^q
    s = q - np.where(huge, q, e)              # right shift that gets there
    R = np.zeros(M.shape, _U)
    left = s <= 0
    R = np.where(left, _shl(M, np.where(left, -s, 0)), R)
    mid = (s > 0) & (s < 64)
    sc = np.where(mid, s, 1)
    Rm = _shr(M, sc)
    rem = M & (_shl(np.ones(M.shape, _U), sc) - _U(1))
    half = _shl(np.ones(M.shape, _U), sc - 1)
    up = (rem > half) | ((rem == half) & ((Rm & _U(1)) != 0))
    R = np.where(mid, Rm + up.astype(_U), R)
    # s == 64: everything is remainder, half is 2^63; a tie goes to even, 0
    R = np.where(s == 64, (M > _U(1 << 63)).astype(_U), R)
    # s > 64: below half a quantum, 0
    out = ((Ec + bias - 1).astype(_U) << _U(mb)) + R
    out = np.where(M == 0, _U(0), out)
    limit = inf_bits if ieee else over_bits
    out = np.where(huge | (out >= limit), over_bits, out)
    out = np.where(isinf, over_bits, out)
    out = np.where(isnan, nan_bits, out)
    return out | (sign.astype(_U) << _U(eb + mb))


def is_nan_bits(bits, kind):
    if kind in INT_KINDS:
        return np.zeros(np.asarray(bits).shape, bool)
    return decode(bits, kind)[3]


def to_f64(bits, kind):
    """The exact value of every pattern as float64 (i64 beyond 2^53 rounds);
    for the mask conditions and the affine model."""
    if kind in INT_KINDS:
        return np.asarray(bits).astype(np.float64)
    sign, M, e, isnan, isinf = decode(bits, kind)
    v = np.ldexp(M.astype(np.float64), e.astype(np.int64))
    v = np.where(isinf, np.inf, v)
    v = np.where(isnan, np.nan, v)
    return np.where(sign, -v, v)


def _float_to_int(bits, in_kind, out_kind):
    sign, M, e, isnan, isinf = decode(bits, in_kind)
    lo, hi = IRANGE[out_kind]
    bl = _bitlen(M)
    fits = (M == 0) | (bl + e <= 64)          # magnitude fits a uint64
    neg = e < 0
    t = np.where(neg, _shr(M, np.minimum(np.where(neg, -e, 0), 63)),
                 _shl(M, np.where(fits & ~neg, e, 0)))
    t = np.where(fits, t, _U(0))
    bound = np.where(sign, _U(-lo), _U(hi))
    defined = ~isnan & ~isinf & fits & (t <= bound)
    two = np.where(sign, (~t) + _U(1), t)     # two's complement, low bits kept
    two = np.where(defined, two, _U(0))
    return two.astype(BITS[out_kind]), defined


def model_cast(values, in_kind, out_kind):
    """Bit patterns of `values` (kind in_kind) cast to out_kind, and the mask
    of positions where the contract defines the result."""
    bits = np.ascontiguousarray(values, dtype=BITS[in_kind])
    all_true = np.ones(bits.shape, bool)
    if in_kind == out_kind:
        return bits.copy(), all_true
    if out_kind in INT_KINDS:
        if in_kind in INT_KINDS:              # low bits
            return bits.astype(np.int64).astype(BITS[out_kind]), all_true
        return _float_to_int(bits, in_kind, out_kind)
    d = decode(bits, in_kind)
    if FMT[out_kind][1] < 23:                 # narrower than f32: through f32
        d = decode(round_to_format(*d, "f32").astype(np.uint32), "f32")
    return round_to_format(*d, out_kind).astype(BITS[out_kind]), all_true


def _f32_values(values, in_kind):
    """The input cast to f32 by the rules above, as float64 (exact)."""
    b, _ = model_cast(values, in_kind, "f32")
    with np.errstate(invalid="ignore"):       # signalling NaNs
        return b.view(np.float32).astype(np.float64)


def fma_f32(x, scale, shift):
    """fma(x, scale, shift) rounded once to f32; x holds f32 values as
    float64, scale and shift are f32-representable. The product of two f32 is
    exact in float64; TwoSum gives the exact error of the sum, which turns
    the float64 sum into round-to-odd, and that survives the final rounding
    to f32 unchanged (53 >= 24 + 2 bits)."""
    with np.errstate(all="ignore"):
        p = x * np.float64(scale)
        t = np.float64(shift)
        s = p + t
        bb = s - p
        err = (p - (s - bb)) + (t - bb)
        sb = s.view(np.uint64) if s.flags.c_contiguous else s.copy().view(np.uint64)
        even = (sb & _U(1)) == 0
        fix = np.isfinite(s) & (err != 0) & even
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def fma_f32_exact(x, scale, shift):
    """One element of fma_f32 in exact rational arithmetic (the check of the
    vector form): round-to-odd float64 of the exact sum, then to f32."""
    if not np.isfinite(x):
        return np.float32(np.float64(x) * scale + shift)
    exact = (fractions.Fraction(float(x)) * fractions.Fraction(float(scale))
             + fractions.Fraction(float(shift)))
    d = float(exact)                          # correctly rounded float64
    got = fractions.Fraction(d)
    if got != exact and (np.float64(d).view(np.uint64) & _U(1)) == 0:
        d = float(np.nextafter(np.float64(d), np.inf if exact > got else -np.inf))
    return np.float32(d)


def model_affine(values, in_kind, out_kind, scale, shift):
    """cast(fma(x_f32, scale, shift)): the fused, single-rounding form the
    kernels compute. scale and shift are rounded to f32 first, as the kernel
    arguments are."""
    sc, sh = np.float32(scale), np.float32(shift)
    y = fma_f32(_f32_values(values, in_kind), sc, sh)
    return model_cast(y.view(np.uint32), "f32", out_kind)


def model_affine_unfused(values, in_kind, out_kind, scale, shift):
    """The host backend's form: the product rounded to f32, then the sum
    rounded to f32. Used only to check the host path and to prove that a
    table separates the two forms."""
    sc, sh = np.float64(np.float32(scale)), np.float64(np.float32(shift))
    x = _f32_values(values, in_kind)
    with np.errstate(all="ignore"):
        # float64 holds the product of two f32 and the sum of two f32 values
        # closely enough that rounding it to f32 is the single f32 rounding
        # (2 * 24 + 2 <= 53)
        p = (x * sc).astype(np.float32).astype(np.float64)
        y = (p + sh).astype(np.float32)
    return model_cast(y.view(np.uint32), "f32", out_kind)


def mismatches(got_bits, exp_bits, defined, out_kind):
    """Indices where got differs from the model: bit for bit where defined,
    a NaN only has to be a NaN."""
    got = np.asarray(got_bits).reshape(-1)
    exp = np.asarray(exp_bits).reshape(-1)
    ok = got == exp
    if out_kind in FLOAT_KINDS:
        ok |= is_nan_bits(got, out_kind) & is_nan_bits(exp, out_kind)
    return np.nonzero(~ok & np.asarray(defined).reshape(-1))[0]


# --------------------------------------------------------------------------
# The tables: built from the formats, nothing random.
# --------------------------------------------------------------------------
def _as_if_finite(mag, kind):
    """Value of magnitude pattern `mag` read as a finite number even where the
    format says inf/NaN: the would-be next value above the largest finite."""
    eb, mb, _ = FMT[kind]
    bias = (1 << (eb - 1)) - 1
    mag = np.asarray(mag, dtype=np.int64)
    ef, mant = mag >> mb, mag & ((1 << mb) - 1)
    M = np.where(ef == 0, mant, mant | (1 << mb)).astype(np.float64)
    return np.ldexp(M, np.where(ef == 0, 1, ef) - bias - mb)


def _max_finite_mag(kind):
    eb, mb, ieee = FMT[kind]
    top = (1 << eb) - 1
    return (top << mb) - 1 if ieee else (top << mb) | ((1 << mb) - 2)


def midpoints_f64(kind):
    """The exact midpoint of every pair of adjacent values of float format
    `kind`, from (0, smallest subnormal) to (largest finite, the would-be next
    value), as positive float64 (all exact)."""
    m = np.arange(0, _max_finite_mag(kind) + 1)
    return (_as_if_finite(m, kind) + _as_if_finite(m + 1, kind)) / 2


def _both_signs(bits, signbit):
    bits = np.asarray(bits)
    return np.concatenate([bits, bits | bits.dtype.type(signbit)])


def _with_neighbours(bits, steps=(1,)):
    out = [bits]
    for d in steps:
        out += [bits - bits.dtype.type(d), bits + bits.dtype.type(d)]
    return np.concatenate(out)


def _f32_bits(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).view(np.uint32)


def _f64_bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


F32_SPECIALS = np.array([
    0x00000000, 0x7F800000,                  # 0, inf
    0x7FC00000, 0x7F800001, 0x7FC00001,      # quiet and signalling NaNs
    0x00000001, 0x007FFFFF,                  # smallest, largest subnormal
    0x00800000, 0x7F7FFFFF,                  # smallest, largest normal
    0x3F800000, 0x42F6E979, 0x3EAAAAAB,      # 1, 123.456, 1/3
], dtype=np.uint32)


def f32_mid_table(kind):
    """Every midpoint of target format `kind` and its two f32 neighbours,
    both signs."""
    mid = _f32_bits(midpoints_f64(kind))
    return _both_signs(_with_neighbours(mid), 0x80000000)


def _f32_int_probes():
    v = []
    for k in (0, 1, 255, 256):
        below = np.nextafter(np.float32(k + 1), np.float32(0))
        v += [np.float32(k), np.float32(k + 0.5), below]
    b = np.array(v, dtype=np.float32).view(np.uint32)
    lim = _with_neighbours(_f32_bits([2.0**31, 2.0**63, 2.0**32, 2.0**24]))
    return _both_signs(np.concatenate([b, lim]), 0x80000000)


def _f32_base():
    return np.concatenate([_both_signs(F32_SPECIALS, 0x80000000), _f32_int_probes(),
                           f32_mid_table("e4m3"), f32_mid_table("e5m2")])


def f32_table(out_kind):
    t = _f32_base()
    if out_kind in ("f16", "bf16"):
        t = np.concatenate([t, f32_mid_table(out_kind)])
    return t


F64_SPECIALS = np.array([
    0x0000000000000000, 0x7FF0000000000000,
    0x7FF8000000000000, 0x7FF0000000000001,
    0x0000000000000001, 0x000FFFFFFFFFFFFF,
    0x0010000000000000, 0x7FEFFFFFFFFFFFFF,
    0x3FF0000000000000, 0x3FD5555555555555,
], dtype=np.uint64)


def _f64_narrow_probes(kind):
    """Midpoints of `kind` +- one f64 ulp, and the double-rounding probes:
    a midpoint +- a quarter of an f32 ulp (2^27 f64 ulps), which rounding
    through f32 first turns into the tie itself."""
    mid = _f64_bits(midpoints_f64(kind))
    return _both_signs(_with_neighbours(mid, (1, 1 << 27))[mid.size:], 1 << 63)


def _f64_f32mid_probes():
    """Midpoints of adjacent f32 values +- one f64 ulp: every exponent, a few
    mantissas, the one above FLT_MAX and the one below the smallest
    subnormal."""
    ex = np.arange(0, 255, dtype=np.int64)
    mags = np.concatenate([(ex << 23) | m for m in (0, 1, 0x2AAAAA, 0x7FFFFE, 0x7FFFFF)])
    mid = (_as_if_finite(mags, "f32") + _as_if_finite(mags + 1, "f32")) / 2
    return _both_signs(_with_neighbours(_f64_bits(mid)), 1 << 63)


def _f64_int_probes():
    ks = [1.0, 255.0, 256.0, 2.0**24, 2.0**31 - 1, 2.0**31, 2.0**31 + 1, 2.0**32,
          2.0**53, 2.0**63, 2.0**64, 0.5, 255.5, 2.0**31 - 0.5, 2.0**31 + 0.5]
    return _both_signs(_with_neighbours(_f64_bits(ks)), 1 << 63)


def _widen(f32_bits):
    with np.errstate(invalid="ignore"):       # signalling NaNs
        return _f64_bits(f32_bits.view(np.float32).astype(np.float64))


def _f64_base():
    # widening canonicalises NaN payloads; F64_SPECIALS carries the NaNs
    return np.concatenate([
        _both_signs(F64_SPECIALS, 1 << 63), _widen(_f32_base()),
        _f64_f32mid_probes(), _f64_int_probes(),
        _f64_narrow_probes("e4m3"), _f64_narrow_probes("e5m2")])


def f64_table(out_kind):
    t = _f64_base()
    if out_kind in ("f16", "bf16"):
        t = np.concatenate([t, _widen(f32_mid_table(out_kind)),
                            _f64_narrow_probes(out_kind)])
    return t


def int_table(kind):
    lo, hi = IRANGE[kind]
    nb = 31 if kind == "i32" else 63
    v = set(range(-520, 521))                 # every fp8 value and tie, the
    #                                           bf16 ties below 2^9, 255..257
    v |= set(range(2040, 2056)) | set(range(65500, 65540))   # f16 ties, overflow
    v |= {lo, lo + 1, hi, hi - 1, 2**31 - 1, 2**31, 2**31 + 1}
    for k in range(nb + 1):
        v |= {2**k - 1, 2**k, 2**k + 1}
        # ties of a p-bit significand, even and odd below, and their neighbours
        for p in (3, 4, 8, 11, 24, 53):
            if k >= p:
                for odd in (1, 3):
                    t = 2**k + odd * 2**(k - p)
                    v |= {t - 1, t, t + 1}
    v |= {-x for x in v}
    v = sorted(x for x in v if lo <= x <= hi)
    return np.array(v, dtype=BITS[kind])


_TABLES = {}


def table(in_kind, out_kind):
    """The input table of one (in, out) pair, as bit patterns. Exhaustive for
    the 8- and 16-bit kinds; f32 and f64 tables depend on the target."""
    key = (in_kind, out_kind if in_kind in ("f32", "f64") and
           out_kind in ("f16", "bf16") else None)
    if key not in _TABLES:
        if in_kind in ("u8", "e4m3", "e5m2"):
            t = np.arange(256, dtype=np.uint8)
        elif in_kind in ("f16", "bf16"):
            t = np.arange(65536, dtype=np.uint32).astype(np.uint16)
        elif in_kind == "f32":
            t = f32_table(out_kind)
        elif in_kind == "f64":
            t = f64_table(out_kind)
        else:
            t = int_table(in_kind)
        t.setflags(write=False)
        _TABLES[key] = t
    return _TABLES[key]


def pairs():
    return [(i, o) for i in KINDS for o in KINDS]


# affine: inputs, outputs and the two (scale, shift) pairs. The first has two
# significant bits in each, so for an input of at most 22 significant bits
# (u8, f16, bf16, fp8) the product is exact and no form of the arithmetic can
# differ; the second has full 24-bit significands (the f32 nearest 1/255 and
# -0.4914).
AFFINE_IN = ("u8", "f16", "bf16", "e4m3", "f32", "i64")
AFFINE_OUT = ("f32", "f16", "bf16")
AFFINE_EXACT = (0.0234375, -1.5)
AFFINE_FULL = (float(np.float32(1 / 255)), float(np.float32(-0.4914)))


def affine_table(in_kind):
    # for f32 the base table and the f16 midpoints: values of every exponent
    return table(in_kind, "f16" if in_kind == "f32" else "f32")


# --------------------------------------------------------------------------
# torch glue for the tests (views only, no conversion)
# --------------------------------------------------------------------------
def torch_dtype(kind):
    import torch

    return {"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64,
            "f32": torch.float32, "f64": torch.float64, "f16": torch.float16,
            "bf16": torch.bfloat16, "e4m3": torch.float8_e4m3fn,
            "e5m2": torch.float8_e5m2}[kind]


_SIGNED = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}


def to_torch(bits, kind):
    """Bit patterns -> a torch tensor of the kind's dtype (a view)."""
    import torch

    a = np.ascontiguousarray(bits, dtype=BITS[kind])
    if kind == "u8":
        return torch.from_numpy(a.copy())
    t = torch.from_numpy(a.view(_SIGNED[a.itemsize]).copy())
    return t.view(torch_dtype(kind))


def from_torch(t, kind):
    """A torch tensor -> its bit patterns."""
    import torch

    t = t.detach().cpu().contiguous()
    iv = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
    return t.view(iv[t.element_size()]).numpy().view(BITS[kind])


def as_rows(bits, width):
    """The table laid out as rows of `width`, padded with zeros."""
    n = -(-bits.size // width)
    a = np.zeros(n * width, dtype=bits.dtype)
    a[:bits.size] = bits
    return a.reshape(n, width)
