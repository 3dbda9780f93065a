"""Numpy model of the rule that decides whether a FLOAT64 column is kept once more as float32
(table.cc narrow_float_column / k_narrow_f32): every value x must satisfy
  - the bits of (double)(float) x equal the bits of x, and
  - (float) x is a zero or a normal number, an infinity or a NaN -- never a denormal --
    tested on the bits.
The tests pick their inputs with it; it is pinned in test_narrow_float_cpu.py."""
import numpy as np


def exact_f32_mask(x):
    """per value of the float64 array `x`: does it qualify?"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        f = x.astype(np.float32)
        back = f.astype(np.float64)
    same = back.view(np.uint64) == x.view(np.uint64)
    fb = f.view(np.uint32)
    normal_or_zero = ((fb & np.uint32(0x7f800000)) != 0) | ((fb & np.uint32(0x7fffffff)) == 0)
    return same & normal_or_zero


def column_qualifies(x):
    return bool(exact_f32_mask(x).all())


def f64(bits):
    """the double with these 64 bits"""
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN_NORMAL = float(np.finfo(np.float32).tiny)
QUIET_NAN = f64(0x7ff8000000000000)

# values a float32 copy holds exactly ...
QUALIFYING = {
    "+0": 0.0,
    "-0": -0.0,
    "+inf": float("inf"),
    "-inf": float("-inf"),
    "quiet NaN": QUIET_NAN,
    "FLT_MAX": FLT_MAX,
    "smallest normal": FLT_MIN_NORMAL,
    "1 + 2^-23": 1.0 + 2.0 ** -23,
    "-16777216": -16777216.0,
}
# ... and values it does not
DISQUALIFYING = {
    "1 + 2^-24": 1.0 + 2.0 ** -24,
    "16777217": 16777217.0,
    "0.1": 0.1,
    "2^-149": 2.0 ** -149,
    "FLT_MAX (1 + 2^-30)": FLT_MAX * (1.0 + 2.0 ** -30),
    "NaN, bit 0 set": f64(0x7ff8000000000001),
    "signalling NaN": f64(0x7ff4000000000000),
}
