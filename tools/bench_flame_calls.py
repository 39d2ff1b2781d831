#!/usr/bin/env python3
"""Single calls of FLAME's device ops, event-timed: ``REPEATS`` x ``CALLS`` calls each at P = 47693 (the
TransformerModel's parameter count) and n = 8 / 32 / 64, microseconds per call, one JSON line per (n, op, repeat).
``agg.cclip`` (L = 3, with a centre), which has the rule's four-launch structure (the anchored Gram pass, a one-wave
kernel, a row pass), and ``agg.signguard`` run beside it.

    python tools/bench_flame_calls.py --out profiles/bench_flame_calls.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, REPEATS, CALLS = 47693, 5, 100


def timed(fn):
    import torch

    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / CALLS)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import torch

    from attackfl_amd import agg, ops

    dev = torch.device("cuda", 0)
    with open(args.out, "a") as fh:
        for n in (8, 32, 64):
            gen = torch.Generator().manual_seed(n)
            g = (0.3 * torch.randn(P, generator=gen)).to(dev)
            U = g[None] + (0.01 * torch.randn(n, P, generator=gen)).to(dev)
            sizes = torch.tensor([300.0 + 37.0 * ((5 * i) % 7) for i in range(n)])
            a0 = (sizes.double() / sizes.double().sum()).to(dev)
            G = ops.gram_anchored(U, g)
            keep, c, info = ops.flame_select(G, a0, 0.001)
            zero = torch.zeros(1, dtype=torch.float64, device=dev)
            ops_ = {
                "gram_anchored": lambda: ops.gram_anchored(U, g),
                "flame_select": lambda: ops.flame_select(G, a0, 0.001),
                "flame_rows": lambda: ops.flame_rows(U, c, g, info[1:2], 77),
                "flame_rows sigma 0": lambda: ops.flame_rows(U, c, g, zero, 77),
                "anchored_rows": lambda: ops.anchored_rows(U, c, g),
                "agg.flame": lambda: agg.flame(U, sizes, centre=g, seed=77),
                "agg.flame noise 0": lambda: agg.flame(U, sizes, centre=g, seed=77, flame_noise=0.0),
                "agg.cclip": lambda: agg.cclip(U, sizes, centre=g),
                "agg.signguard": lambda: agg.signguard(U, sizes, centre=g, seed=77),
            }
            for name, fn in ops_.items():
                us = timed(fn)
                for r, v in enumerate(us):
                    fh.write(json.dumps({"n": n, "P": P, "op": name, "repeat": r, "us_per_call": round(v, 2),
                                         "kept": int(keep.sum())}) + "\n")
                print(f"n={n} {name}: {sum(us) / len(us):.1f} us (min {min(us):.1f}, max {max(us):.1f})", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
