#!/usr/bin/env python
"""Pre-aggregation timings on the device (profiles/bench_preagg.md).

``calls``: device events over 200 calls, three repeats in one session, P = 47693 (TransformerModel):
``ops.mix_rows`` (``k_mix_rows``) against the loop of R ``ops.weighted_rows`` calls it replaces, at (n, R) = (8, 8),
(32, 32), (64, 64), (64, 32); ``ops.nnm_weights`` (``k_nnm_weights``), the distance pass, ``agg.nnm`` and
``agg.bucketing`` (s = 2) as a whole at n = 8 / 32 / 64.

``rounds``: 30 timed rounds (2 more first) of the headline shape (8 clients, ``multi_krum``, ``7:Min-Max:2``, the
workload of bench.py) with ``engine.pre-agg`` none / nnm alternately, three times each in one process after one
untimed run; per-round times are ``t_round`` of the engine's metrics JSONL.

    python tools/bench_preagg.py calls --out profiles/bench_preagg_calls.jsonl
    python tools/bench_preagg.py rounds --out profiles/bench_preagg_rounds.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

P = 47693


def timed(fn, calls=200, warm=20):
    """Microseconds per call between two device events."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls


def rows(n, g, dev):
    return (0.3 * torch.randn(1, P, generator=g) + 0.01 * torch.randn(n, P, generator=g)).to(dev)


def calls():
    from attackfl_amd import agg, ops

    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    for rep in range(3):
        for n, R in ((8, 8), (32, 32), (64, 64), (64, 32)):
            U = rows(n, g, dev)
            W = torch.rand(R, n, generator=g, dtype=torch.float64).to(dev)
            ws = [W[r].contiguous() for r in range(R)]
            t_mix = timed(lambda: ops.mix_rows(W, U))
            t_loop = timed(lambda: [ops.weighted_rows(U, w) for w in ws], calls=50, warm=5)
            yield {"what": "mix_rows", "rep": rep, "n": n, "R": R, "P": P, "mix_us": round(t_mix, 2),
                   "loop_us": round(t_loop, 2), "ratio": round(t_loop / t_mix, 2)}
        for n in (8, 32, 64):
            U = rows(n, g, dev)
            f = max(0, (n - 3) // 4)
            D = ops.pairwise_sqdist(U)
            yield {"what": "nnm", "rep": rep, "n": n, "f": f, "P": P,
                   "nnm_weights_us": round(timed(lambda: ops.nnm_weights(D, f)), 2),
                   "pairwise_sqdist_us": round(timed(lambda: ops.pairwise_sqdist(U)), 2),
                   "agg_nnm_us": round(timed(lambda: agg.nnm(U, None, f)), 2),
                   "agg_bucketing2_us": round(timed(lambda: agg.bucketing(U, None, 2, 5)), 2)}


def run_rounds(pre):
    from attackfl_amd.config import from_dict
    from attackfl_amd.fl.engine import FLEngine, build_client_table
    from launch import parse_attackers

    tmp = tempfile.mkdtemp(prefix="afl_preagg_")
    cfg = from_dict({
        "server": {"num-round": 32, "clients": 8, "mode": "multi_krum", "model": "TransformerModel", "data-name": "ICU"},
        "data": {"synthetic": True},
        "engine": {"checkpoint-dir": tmp, "trainer": "auto", "seed": 1, "metrics": tmp + "/m.jsonl", "pre-agg": pre},
        "log_path": tmp})
    eng = FLEngine(cfg, device="cuda", table=build_client_table(cfg, 1, parse_attackers("7:Min-Max:2")), verbose=False)
    eng.run()
    eng.close()
    recs = [json.loads(line) for line in open(tmp + "/m.jsonl")]
    t = [r["t_round"] for r in recs[2:] if r["ok"]]
    return {"pre_agg": pre, "rounds": len(t), "mean_ms": round(1e3 * statistics.mean(t), 4),
            "median_ms": round(1e3 * statistics.median(t), 4), "auc": round(recs[-1]["metric"], 4),
            "early": sum(1 for r in recs if r.get("path") == "early-launch")}


def rounds():
    from attackfl_amd.utils.log import set_quiet

    set_quiet(True)
    run_rounds("none")  # (untimed: module load, allocator, code objects)
    for rep in range(3):
        for pre in ("none", "nnm"):
            yield {**run_rounds(pre), "rep": rep}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["calls", "rounds"])
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_preagg: no GPU (timings are taken on the device only)", file=sys.stderr)
        return 1
    with open(args.out, "w") as fh:
        for rec in (calls() if args.what == "calls" else rounds()):
            fh.write(json.dumps(rec) + "\n")
            fh.flush()
            print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
