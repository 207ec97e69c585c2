"""numpy reference of the e4m3 K/V cache's rounding (kv_f8, csrc/llama_kernels.h): OCP e4m3fn has 1 sign, 4 exponent (bias 7) and 3 mantissa bits, no
inf; its largest finite number is 448, numbers below 2^-6 are subnormal (steps of 2^-9), and what lies below half the smallest step, 2^-10, rounds to zero.

e4m3_round(x) is what the cache's writers store and its readers widen: clamp to +-448 (the kernels do it in plain arithmetic before the conversion), then
round to nearest-even at 3 mantissa bits with the exponent floored at -6.  The sign of a zero is kept.  Shared by the CPU test, which holds it against
torch.float8_e4m3fn, and the GPU tests, which therefore do not depend on torch's fp8 support."""
import numpy as np

E4M3_MAX = 448.0


def e4m3_round(x):
    x = np.asarray(x, dtype=np.float32)
    a = np.abs(np.clip(x, -E4M3_MAX, E4M3_MAX)).astype(np.float64)
    _, ex = np.frexp(a)                                   # a = m * 2^ex, m in [0.5, 1): the leading bit is 2^(ex - 1)
    quantum = np.ldexp(1.0, np.maximum(ex - 1, -6) - 3)    # three mantissa bits below the leading one; subnormals share the quantum 2^-9
    r = np.rint(a / quantum) * quantum                     # exact quotients, ties to even
    return np.copysign(r, x).astype(np.float32)


def e4m3_finite_codes():
    """the 254 finite e4m3fn numbers as float32 (0x7f and 0xff are NaN), in code order"""
    out = []
    for code in range(256):
        e, m = (code >> 3) & 15, code & 7
        if e == 15 and m == 7:
            continue
        mag = (8 + m) * 2.0 ** (e - 10) if e else m * 2.0 ** -9
        out.append(-mag if code & 128 else mag)
    return np.array(out, dtype=np.float32)
