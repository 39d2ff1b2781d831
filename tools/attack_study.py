#!/usr/bin/env python3
"""Post-attack quality study (BASELINE north star: "post-attack test-accuracy"): per-round test
ROC-AUC of TransformerModel/ICU under every reference attack (src/Utils.py:52-214) against FedAvg and the
robust aggregators (server.py:286-494), with 3 attackers of 8 clients from round 2.

Every cell runs with fixed seeds on the GPU (fused bf16 trainer, native aggregation / attack kernels) or on
the CPU (``trainer: oracle`` — the fp32 twin of the fused trainer with the same dropout masks — and the
PyTorch composites), so the two devices follow the same trajectories up to bf16 rounding and their final
AUCs can be compared cell by cell.  One JSON line per cell:

    {"device", "mode", "attack", "rounds", "auc": [per round], "final_auc", "attack_gamma": [...], "seconds"}

    python tools/attack_study.py --device cuda --out study_gpu.jsonl [--cells fedavg:LIE,median:Min-Max]
    python tools/attack_study.py --device cpu --out study_cpu.jsonl --jobs 4
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ["fedavg", "median", "trimmed_mean", "krum", "hyper", "multi_krum", "bulyan"]
# the AGR-tailored attacks (docs/PARITY.md) take [m, f]: [3, 3] for the 3-of-8 setting, f lowered by ``agr_args`` to
# what the attacker's sample admits
ATTACKS = {"none": None, "LIE": [0.74], "Min-Max": [], "Min-Sum": [], "Opt-Fang": [], "Random": [0.5],
           "AGR-Krum": [3, 3], "AGR-MKrum": [3, 3], "AGR-Bulyan": [3, 3]}


def agr_args(attack: str, K: int, m: int, f: int):
    """[m, f] with f the largest value <= the wanted one that the modelled system of K genuine rows + m copies admits
    (K + m >= 2 f + 3, AGR-Bulyan 4 f + 3; at least 1).  5 genuine clients and 3 attackers: f = 2 (Krum, Multi-Krum)
    and f = 1 (Bulyan, also the server's f = auto at 8 clients) when every genuine model is sampled.  Where not even
    f = 1 fits, the attack itself submits the attacker's own model (gamma 0)."""
    per = 4 if attack == "AGR-Bulyan" else 2
    return [m, max(1, min(f, (K + m - 3) // per))]

def cells(spec: str):
    if spec:
        return [tuple(c.split(":", 1)) for c in spec.split(",")]
    return [(m, a) for m in MODES for a in ATTACKS]


def run_cell(mode: str, attack: str, device: str, rounds: int, threads: int = 0, genuine_rate: float = 0.5,
             distance: str = "spectral", seed: int = 7, tau: float = None, attackers: int = 3,
             engine_set: dict = None) -> dict:
    import torch

    if threads:
        torch.set_num_threads(threads)
    from attackfl_amd.config import AttackSpec, from_dict
    from attackfl_amd.fl.engine import FLEngine, build_client_table
    from attackfl_amd.utils.log import set_quiet

    set_quiet(True)
    tmp = tempfile.mkdtemp(prefix="afl_study_")
    d = {
        "server": {"num-round": rounds, "clients": 8, "mode": mode, "model": "TransformerModel", "data-name": "ICU",
                   "genuine-rate": genuine_rate, "random-seed": seed - 6, "data-distribution": {"num-data-range": [800, 1200]}},
        "learning": {"epoch": 2, "batch-size": 128, "learning-rate": 0.004},
        "data": {"synthetic": True, "train-size": 20000, "test-size": 3000},
        "engine": {"checkpoint-dir": tmp, "trainer": "auto" if device.startswith("cuda") else "oracle", "seed": seed,
                   "max-retries": 5, "distance": distance, **(engine_set or {})},
        "log_path": tmp,
    }
    cfg = from_dict(d)
    who = range(8 - attackers, 8)
    args = ATTACKS[attack]
    if attack.startswith("AGR-"):  # (K: the attacker's sample of the 8 - attackers genuine models, engine rule)
        args = agr_args(attack, max(int(genuine_rate * (8 - attackers)), 1), attackers, int(args[1]))
    atk = {} if args is None else {c: AttackSpec(attack, 2, args, tau=tau) for c in who}
    eng = FLEngine(cfg, device=device, table=build_client_table(cfg, 1, atk), verbose=False)
    t0 = time.time()
    stalled = False
    try:
        eng.run()
    except RuntimeError:  # max-retries consecutive failed rounds: the attack stopped training progress
        stalled = True
    hist = eng.history
    eng.close()
    ok = [r for r in hist if r["ok"]]
    return {"device": "gpu" if device.startswith("cuda") else "cpu", "mode": mode, "attack": attack,
            "genuine_rate": genuine_rate, "distance": distance, "seed": seed,
            "tau": next((a.tau for a in atk.values()), 1.0 if tau is None else tau),
            "attackers": len(atk), "attack_args": args, "engine_set": engine_set or {}, "rounds": len(ok),
            "failed_rounds": len(hist) - len(ok), "stalled": stalled,
            "auc": [round(r["metric"], 5) for r in ok], "final_auc": round(ok[-1]["metric"], 5) if ok else None,
            "attack_gamma": [round(r["attack"]["gamma"], 4) for r in ok if "attack" in r and "gamma" in r["attack"]],
            # last ACCEPTED γ per attacking round (0: every tried γ was rejected)
            "gamma_succ": [round(r["attack"]["gamma_succ"], 4) for r in ok if "gamma_succ" in r.get("attack", {})],
            # every tried γ of the last attacking round (the reference prints each, src/Utils.py:119)
            "gammas_last": next((r["attack"]["gammas"] for r in reversed(hist) if "gammas" in r.get("attack", {})), None),
            # foolsgold: every client's weight, averaged over the successful rounds that had a history, and the last one
            **({"alpha_mean": [round(sum(r["alpha"][i] for r in ok[1:]) / max(1, len(ok) - 1), 4) for i in range(8)],
                "alpha_last": [round(a, 4) for a in ok[-1]["alpha"]]} if ok and "alpha" in ok[-1] else {}),
            # the filtering rules (signguard: kept; dnc, multi_krum, bulyan: selected): per successful round the
            # attackers the rule kept, and how many rows it kept in all
            **({"attackers_kept": [[c for c in who if c in r[k]] for r in ok for k in ("kept", "selected") if k in r],
                "rows_kept": [len(r[k]) for r in ok for k in ("kept", "selected") if k in r]}
               if ok and any(k in ok[-1] and isinstance(ok[-1][k], list) for k in ("kept", "selected")) else {}),
            "seconds": round(time.time() - t0, 2)}


def _worker(args):
    mode, attack, device, rounds, threads, gr, dist, seed, tau, na, es = args
    return run_cell(mode, attack, device, rounds, threads, gr, dist, seed, tau, na, es)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--cells", default="", help="mode:attack,... (default: every mode x attack)")
    ap.add_argument("--jobs", type=int, default=1, help="parallel CPU processes")
    ap.add_argument("--genuine-rate", type=float, default=0.5, help="server.genuine-rate (reference default 0.5)")
    ap.add_argument("--distance", default="spectral", choices=["spectral", "flat"])
    ap.add_argument("--tau", type=float, default=None,
                    help="bisection stop gap (default: the attack's own, 1.0 as the reference, 0.02 for the AGR modes)")
    ap.add_argument("--attackers", type=int, default=3, help="attacking clients (the last N of 8)")
    ap.add_argument("--seeds", default="7", help="comma-separated run seeds (engine seed; server random-seed = seed - 6)")
    ap.add_argument("--engine-set", default="", help="engine keys for every cell, key=value,... (e.g. cclip-iters=1)")
    args = ap.parse_args()
    import yaml

    engine_set = {k: yaml.safe_load(v) for k, v in (kv.split("=", 1) for kv in args.engine_set.split(",") if kv)}
    seeds = [int(x) for x in args.seeds.split(",")]
    todo = [(m, a, sd) for m, a in cells(args.cells) for sd in seeds]
    with open(args.out, "a") as fh:
        if args.jobs > 1 and not args.device.startswith("cuda"):
            import multiprocessing as mp

            threads = max(1, (os.cpu_count() or 8) // args.jobs)
            with mp.get_context("spawn").Pool(args.jobs) as pool:
                for res in pool.imap_unordered(_worker, [(m, a, args.device, args.rounds, threads, args.genuine_rate,
                                                                   args.distance, sd, args.tau, args.attackers, engine_set)
                                                                  for m, a, sd in todo]):
                    fh.write(json.dumps(res) + "\n")
                    fh.flush()
                    print(res["mode"], res["attack"], res["final_auc"], res["seconds"], flush=True)
        else:
            for m, a, sd in todo:
                res = run_cell(m, a, args.device, args.rounds, 0, args.genuine_rate, args.distance, sd, args.tau,
                               args.attackers, engine_set)
                fh.write(json.dumps(res) + "\n")
                fh.flush()
                print(res["mode"], res["attack"], res["final_auc"], res["seconds"], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
