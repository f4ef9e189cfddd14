"""The cases and bars of the LPIPS tests (tests/test_gpu_lpips.py, tests/test_lpips_host.py).

A case is (P, H, W) with seeded images in [-1, 1] and the seeded stand-in weights of lzzx_nerf_amd.synthetic.lpips_alex_state(0).  The
kernels are held to the float64 evaluation of tests/lpips_checker.py within BARS: BAR_FACTOR times the largest deviation of the checker's
own float32 evaluation from its float64 one over these cases (MEASURED), relative for the per-patch value, relative to the case's largest
|gradient| in float64 for the gradient.  Why 8: ours and torch's are both f32 sums of up to 3456 terms in different orders, a sequential
k-ordered MFMA chain with split-K loses a few times more than a blocked library sum, and the rest is headroom; a wrong tap, pad, stride,
weight index or pool window shows at 1e-3 and above.

    python tests/lpips_cases.py --measure      prints MEASURED for this file (CPU only)
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name: (P, H, W) and why this shape
CASES = {
    "min31": (1, 31, 31),        # the minimum; taps 7, 3, 1, 1, 1
    "pad32": (1, 32, 32),        # the padded minimum
    "odd35x47": (2, 35, 47),     # odd and non-square; taps 8x11, 3x5, 1x2; two patches
    "sq64": (3, 64, 64),         # taps 15, 7, 3
    "r96x80": (1, 96, 80),       # taps 23x19, 11x9, 5x4
    "p5": (5, 33, 40),           # a patch count that is not a multiple of any tile; taps 7x9, 3x4, 1x1
}
WEIGHT_SEED = 0
BAR_FACTOR = 8.0

# the largest deviation of the checker's float32 evaluation from its float64 evaluation over CASES, by `--measure`
MEASURED = {
    "value_rel": 3.695e-07,
    "grad_rel": 2.458e-06,
}
BARS = {k: BAR_FACTOR * v for k, v in MEASURED.items()}


@functools.lru_cache(maxsize=None)
def state(seed=WEIGHT_SEED):
    from lzzx_nerf_amd.synthetic import lpips_alex_state
    return lpips_alex_state(seed)


def images(name):
    """(pred, target) [P,3,H,W] f32 in [-1, 1]: a smooth seeded target plus noise, and pred a perturbation of it, clipped"""
    P, H, W = CASES[name]
    rng = np.random.default_rng(1000 + sorted(CASES).index(name))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    target = np.empty((P, 3, H, W))
    for p in range(P):
        for c in range(3):
            fy, fx, ph = rng.uniform(0.05, 0.6), rng.uniform(0.05, 0.6), rng.uniform(0, 6.28)
            target[p, c] = 0.6 * np.sin(fy * y + fx * x + ph) + 0.3 * rng.uniform(-1, 1, (H, W))
    pred = np.clip(target + 0.25 * rng.standard_normal(target.shape), -1, 1)
    return pred.astype(np.float32), np.clip(target, -1, 1).astype(np.float32)


def upstream(name):
    """the gradient arriving at the [P] values: not all ones, so that a patch's gradient is scaled by its own element"""
    P = CASES[name][0]
    return (1.0 + 0.25 * np.arange(P)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(name, dtype_name="float64"):
    """(value [P], gradient [P,3,H,W]) of the checker in float64 (or float32); computed once per process and shared"""
    import torch

    import lpips_checker as K
    pred, target = images(name)
    v, g = K.value_and_grad(state(), pred, target, getattr(torch, dtype_name), upstream(name))
    v.setflags(write=False)
    g.setflags(write=False)
    return v, g


def deviations(value, grad, name):
    """(largest relative deviation of the values, largest gradient deviation over the case's largest |gradient|) from the float64 checker"""
    v64, g64 = reference(name)
    dv = float(np.max(np.abs(np.asarray(value, np.float64) - v64) / np.abs(v64)))
    dg = float(np.max(np.abs(np.asarray(grad, np.float64) - g64)) / np.max(np.abs(g64)))
    return dv, dg


def measure():
    out = {"value_rel": 0.0, "grad_rel": 0.0}
    for name in CASES:
        v32, g32 = reference(name, "float32")
        dv, dg = deviations(v32, g32, name)
        print("%-10s %-14s value %.3e  gradient %.3e" % (name, CASES[name], dv, dg))
        out["value_rel"], out["grad_rel"] = max(out["value_rel"], dv), max(out["grad_rel"], dg)
    print("MEASURED = {")
    for k, v in out.items():
        print('    "%s": %.3e,' % (k, v))
    print("}")
    return out


if __name__ == "__main__":
    if "--measure" in sys.argv:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        measure()
    else:
        print(__doc__)
