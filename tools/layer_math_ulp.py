"""Worst error of the device math functions the layer kernels call, from the arrays ``tools/layer_math_probe.hip``
wrote, against float64 — in units of ``2^-23 |f(x)|`` — and the budget T each gives (next power of two at or above
twice the worst; ``tests/test_layer_oracles.py`` ``T``, ``docs/LAYER_TEST_BOUNDS.md``).

    python tools/layer_math_ulp.py <dir with probe_*.bin>
"""
import math
import sys

import numpy as np
import torch

U = 2.0 ** -23
FMAX = 3.4028234663852886e38
REFS = {
    "erff": torch.erf, "tanhf": torch.tanh, "expf": torch.exp, "logf": torch.log, "log1pf": torch.log1p,
    "pow09": lambda t: torch.tensor(float(np.float32(0.9)), dtype=torch.float64) ** t,
    "pow0999": lambda t: torch.tensor(float(np.float32(0.999)), dtype=torch.float64) ** t,
    "rsqrtf": torch.rsqrt, "sqrtf": torch.sqrt,
    "fastexp": torch.exp,  # __expf: reported in units of (2 + |x|) 2^-23 |f|
}


def main(d):
    for name, f in REFS.items():
        a = torch.from_numpy(np.fromfile(f"{d}/probe_{name}.bin", dtype=np.float32).astype(np.float64))
        x, y = a[:a.numel() // 2], a[a.numel() // 2:]
        r = f(x)
        normal = torch.isfinite(r) & (r.abs() >= 2.0 ** -126) & (r.abs() <= FMAX)  # fp32's normal range
        ulp = (y - r).abs() / (U * r.abs())
        if name == "fastexp":
            ulp = ulp / (2 + x.abs())
        ulp = torch.where(normal, ulp, torch.zeros_like(ulp))
        i = int(ulp.argmax())
        small = torch.isfinite(r) & (r.abs() < 2.0 ** -126)  # below the smallest normal: absolute error only
        flush = float((y - r).abs()[small].max()) if bool(small.any()) else 0.0
        big = ~torch.isfinite(r) | (r.abs() > FMAX)
        r = torch.where(r.abs() > FMAX, torch.sign(r) * float("inf"), r)
        bad = int((big & ~((torch.isnan(r) & torch.isnan(y)) | (r == y))).sum())
        w = float(ulp[i])
        print(f"{name:8s} worst {w:.3f} at x = {float(x[i]):.6g}   T = {2 ** max(0, math.ceil(math.log2(2 * w)))}"
              f"   sub-normal results: worst |err| {flush:.3g}   non-finite mismatches {bad}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ".")
