"""Inputs shared by the row-conversion tests (test_convert_rows_cpu.py, test_gpu_convert_rows.py): the boundary
set of the e4m3 quantiser per exponent, random f32 bit patterns and the tie patterns of the bf16 rounding.  The
expected values never come from here: they are ia.quantize_fp8_e4m3 / ia.f32_to_bf16_bits, the definitions."""
import functools

import numpy as np

import islands_amd as ia

EXPONENTS = (-32, -9, 0, 5, 32)
F32_MAX = np.finfo(np.float32).max
F32_DENORM_MIN = np.float32(2.0 ** -149)


def e4m3_values() -> np.ndarray:
    """the 127 finite non-negative e4m3 values, ascending (codes 0x00 .. 0x7E), float64"""
    return ia.fp8_e4m3_to_f32(np.arange(0x7F, dtype=np.uint8)).astype(np.float64)


def neighbours(x: np.ndarray) -> np.ndarray:
    """x (float32) with the float32 just below and just above each element"""
    x = x.astype(np.float32)
    return np.concatenate([np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))])


@functools.lru_cache(maxsize=None)
def boundary_set(e: int) -> np.ndarray:
    """float32 values at which narrow_fp8(., e) can go wrong, both signs of each: every finite non-negative e4m3
    value times 2^e; the midpoint of every adjacent pair (exact in float32) and its two float32 neighbours;
    448 * 2^e and 464 * 2^e (the last tie: above it the unclamped rounding would reach the NaN code) with their
    neighbours; 2^-10 * 2^e, which ties to zero; 0, the largest float, infinity and the smallest denormal."""
    v = e4m3_values()
    s = 2.0 ** e
    mid = (v[:-1] + v[1:]) / 2 * s
    mid32 = mid.astype(np.float32)
    assert (mid32.astype(np.float64) == mid).all()  # exact in float32
    vals = (v * s).astype(np.float32)
    assert (vals.astype(np.float64) == v * s).all()
    tops = np.array([448.0 * s, 464.0 * s], dtype=np.float32)
    pos = np.concatenate([vals, neighbours(mid32), neighbours(tops), np.array([2.0 ** -10 * s], dtype=np.float32),
                          np.array([0.0, F32_MAX, np.inf, F32_DENORM_MIN], dtype=np.float32)])
    out = np.concatenate([pos, -pos]).astype(np.float32)
    assert not np.isnan(out).any()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def random_patterns(count: int = 1 << 20, seed: int = 5) -> np.ndarray:
    """uniformly random u32 bit patterns: every exponent field, denormals, infinities and NaNs among them"""
    b = np.random.default_rng(seed).integers(0, 1 << 32, size=count, dtype=np.uint64).astype(np.uint32)
    b.setflags(write=False)
    return b


def is_nan_bits(b: np.ndarray) -> np.ndarray:
    return (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


@functools.lru_cache(maxsize=None)
def bf16_tie_patterns() -> np.ndarray:
    """every u32 pattern whose low half is 0x7FFF, 0x8000 or 0x8001: just below, at and just above every tie of
    the bf16 rounding, for both parities of the kept half, the finite values that round to infinity and the NaNs
    whose payload lies in the low half alone"""
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    b = np.concatenate([hi | np.uint32(low) for low in (0x7FFF, 0x8000, 0x8001)])
    b.setflags(write=False)
    return b


def auto_scale_exp(top: float) -> int:
    """the definition's loop: the smallest e in [-32, 32] with top <= 448 * 2^e (float64: both sides exact)"""
    e = -32
    while e < 32 and top > 448.0 * 2.0 ** e:
        e += 1
    return e
