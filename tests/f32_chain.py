"""The arithmetic of sample_dtype="f32mma" (include/gpet_hip.h, gpet_batch_set_sample_arith) evaluated exactly in numpy: a
vectorised float32 fmaf and the k-ordered chain of it.  The oracle has no such mode; the tests of the mode
(tests/test_gpu_sample_f32mma.py, tests/test_gpu_trace_f32mma.py) take their expected values from here, and
tests/test_f32_chain.py checks this file against the C library's fmaf.

fmaf(a, b, c) is a * b + c rounded ONCE to float32.  float32(float64(a) * float64(b) + float64(c)) rounds twice -- the sum to
float64, then to float32 -- and is wrong where the float64 sum lands exactly halfway between two floats although the true sum
does not.  Here: the product of two floats is exact in float64 (48 bits); the float64 sum s and its TwoSum error e give the true
sum s + e; a rounding boundary of float32 (a halfway point, itself a float64) cannot lie strictly between the true sum and s,
since s is the float64 nearest the true sum; so float32(s) is right unless s IS a halfway point and e != 0, and then the true
sum lies on e's side of it."""
import numpy as np


def fmaf(a, b, c):
    """a * b + c with one rounding, elementwise on float32 arrays (broadcasting); finite results below the overflow threshold."""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)  # exact
    c64 = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)  # TwoSum: p + c64 == s + e exactly
    f = s.astype(np.float32)  # round to nearest even
    d = s - f.astype(np.float64)  # exact
    # the float on the other side of s, and whether s is exactly halfway between the two
    other = np.nextafter(f, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    tie = (d != 0) & (e != 0) & (s == 0.5 * (f.astype(np.float64) + other.astype(np.float64)))
    lo, hi = np.minimum(f, other), np.maximum(f, other)
    return np.where(tie, np.where(e > 0, hi, lo), f).astype(np.float32)


def chain(Z, A, order=None):
    """acc[s][j] = fmaf(Z[s][k], A[k][j], acc[s][j]) over k in `order` (default: ascending) from +0: float32 [S][L].
    Z [S][r] and A [r][L] are narrowed to float32 first (round to nearest even)."""
    Z = np.asarray(Z).astype(np.float32)
    A = np.asarray(A).astype(np.float32)
    acc = np.zeros((Z.shape[0], A.shape[1]), dtype=np.float32)
    for k in (range(Z.shape[1]) if order is None else order):
        acc = fmaf(Z[:, k, None], A[None, k, :], acc)
    return acc
