"""The argument set the exp() restatements are pinned on (tests/test_exp_host.py, tests/test_gpu_exp.py), built once per process and left
unchanged: about 2 * 10^6 doubles, deterministic.
  specials    +-0, +-2^-55, +-2^-54 (the `1 + x` shortcut ends between them), the largest negative subnormal, +-1e300, +-inf, NaN
  thresholds  512 and -512 (where the careful scaling starts), -708.396... (first subnormal result), -745.133... (underflow to 0),
              709.782... (overflow), each with both neighbours
  table steps -j ln2/128 and the half-way points -(j + 1/2) ln2/128 with both neighbours, j = 0 .. 138 239 (down to -748): the table index
              and the rounding of `InvLn2N*x + Shift` change there — the one place the FMA build's fused product shows
  KDE stream  -(z*z/2), z = (g * 0.0025 - d) / h for g = 0 .. 400, h in {0.01, 0.015} and 1 250 seeded d in [0, 1): what cluster_kernel asks
  positive    10^5 seeded arguments in [512, 709.78): the branch that scales by 2^1009
`libm_exp` is glibc's exp() itself through ctypes (numpy's exp is its own SIMD loop, not libm's)."""
import ctypes as C
import ctypes.util
import numpy as np

LN2_128 = float.fromhex("0x1.62e42fefa39efp-1") / 128


def _build():
    inf = np.inf
    specials = np.array([0.0, -0.0, 2.0 ** -55, -2.0 ** -55, 2.0 ** -54, -2.0 ** -54, -4.9e-324, 1e300, -1e300, inf, -inf, np.nan])
    thr = np.array([512.0, -512.0, -708.3964185322641, -745.1332191019411, 709.782712893384])
    thresholds = np.concatenate([np.nextafter(thr, -inf), thr, np.nextafter(thr, inf)])
    j = np.arange(138240, dtype=np.float64)
    steps = []
    for base in (-j * LN2_128, -(j + 0.5) * LN2_128):
        steps += [np.nextafter(base, -inf), base, np.nextafter(base, inf)]
    rng = np.random.default_rng(20240607)
    d = rng.random(1250)
    g = np.arange(401, dtype=np.float64) * 0.0025
    kde = []
    for h in (0.01, 0.015):
        z = (g[:, None] - d[None, :]) / h
        kde.append((-(z * z / 2)).ravel())
    positive = 512.0 + rng.random(100000) * (709.78 - 512.0)
    parts = {"specials": specials, "thresholds": thresholds, "steps": np.concatenate(steps), "kde": np.concatenate(kde), "positive": positive}
    x = np.ascontiguousarray(np.concatenate(list(parts.values())))
    x.setflags(write=False)
    return x, {k: v.size for k, v in parts.items()}


ARGS, PARTS = _build()


def libm_exp(x):
    """glibc's exp() on every element, one call each"""
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    f = libm.exp
    f.restype = C.c_double
    f.argtypes = [C.c_double]
    return np.array([f(v) for v in x.tolist()], dtype=np.float64)


def mismatches(a, b):
    """indices where two float64 arrays differ as bit patterns, NaN == NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b)))
