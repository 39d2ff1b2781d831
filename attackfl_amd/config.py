"""Typed ``config.yaml`` schema.

Same keys and defaults as the reference ``config.yaml:1-38`` (read at ``server.py:55-89``,
``client.py:42-48``).  Every reference key is accepted unchanged; the ``rabbit:`` section is
parsed and ignored (there is no broker: transport is RCCL / gloo, see ``parallel/comm.py``).

Extensions (all optional, defaults keep reference behaviour):

``comm:``
  backend: auto | nccl | gloo | loopback
  clients-per-rank: int (packed launcher; 0 = clients / world)
  one-shot-allgather: auto | true | false  (IPC xGMI all-gather of the update blocks on one node:
                            stream-ordered, no host staging; auto = on for GPU ranks of one host, verified
                            collectively at setup with a fallback to the process group's all-gather)
  fedavg-allreduce: auto | true | false  (fedavg without attackers/detection: one all_reduce of
                            [sum s_i w_i | sum s_i] instead of the update all-gather; auto = world > 1
                            without the IPC path)
  timeout-s: collective timeout (failure detection)
  attackers: {client_index: {mode, round, args, gamma, tau}}  (launcher-side attack assignment; mode: the
                            reference's Random | LIE | Min-Max | Min-Sum | Opt-Fang plus the AGR-tailored AGR-Krum |
                            AGR-MKrum | AGR-Bulyan with args [m, f, dev], docs/PARITY.md; gamma / tau: the bisection's
                            start and stop gap, default 50 / 1, for the AGR modes 10 / 0.02)
``data:``
  synthetic: auto | true | false   (auto = use the reference pickles when present)
  train-size / test-size / seed / har-train-size / har-test-size
``server:``
  mode: the reference's modes plus multi_krum | bulyan | geomed | dnc | cclip | foolsgold | signguard | flame
        (Multi-Krum, Bulyan, the geometric median / RFA, Divide-and-Conquer and centred clipping: defences that assume f >= 1
        Byzantine clients; ``krum`` keeps the reference's f = 0, A-11; FoolsGold: the one rule with memory across rounds,
        a per-client history of updates whose cosines weigh colluders down; SignGuard: a norm filter about the median
        norm and a clustering of the updates' sign statistics; FLAME: the majority cluster of the updates' cosine
        distances, clipping to the median norm and Gaussian noise; definitions in docs/PARITY.md)
``engine:``
  trainer: auto | fused | graph | eager | oracle  (fused = HIP persistent TransformerModel / RNNModel
                                    kernels; graph = HIP-graph-replayed layer programs for CNN/RNN/HAR models;
                                    oracle = CPU fp32 twin of the fused TransformerModel trainer, same masks)
  distance: spectral | flat         (attack distance; spectral = reference ``torch.linalg.norm(ord=2)``)
  seed: int                         (torch / client RNG seed; the reference seeds only ``random``)
  metrics: path of the JSONL metrics file ('' disables)
  checkpoint-dir: where ``*.pth`` files go (reference: CWD)
  async-checkpoint: bool            (default True: the leader writes ``*.pth`` from a background thread)
  compat-hyper-resume: bool         (True = reproduce reference A-5: a loaded hyper checkpoint is discarded)
  compat-fltrust: bool              (True = reproduce reference A-10: FLTrust subtracts the global model twice)
  max-retries: int                  (consecutive failed rounds before the run aborts)
  trace: bool                       (roctx ranges around every round phase; also ATTACKFL_TRACE=1)
  phase-sync: bool                  (synchronise after the aggregate so per-phase times are device times)
  speculative: bool                 (default True: on GPU ranks, enqueue the next round's training
                                    before this round's validation / checkpoint, which overlap it)
  compat-har-train: bool            (True = reference train_HAR semantics: no size-1 batch skip, no NaN
                                    abort, client.py:114-131)
  compat-fedavg-alias: bool         (True = reproduce reference A-13: FedAvg writes the aggregate into the
                                    first client's stored update, which attackers may receive as "genuine")
  fault-inject: [{client, round}]   (NaN-poison a client's model before that training round)
  gmm-rank: int                     (gmm mode's PCA rank, default 1; 0 = max(1, min(4, n // 2 - 1)), the
                                    round-5 rule: profiles/gmm_rank_study_r6.md)
  byz-f: auto | int >= 0            (multi_krum / bulyan / dnc: the assumed number f of Byzantine clients; auto =
                                    max(0, (n - 3) // 4), the largest f Bulyan admits; an explicit f >= 1 needs
                                    n >= 2 f + 3 (multi_krum, dnc) or n >= 4 f + 3 (bulyan) or the round raises;
                                    dnc drops min(ceil(dnc-c f), n - 1) rows per iteration)
  geomed-iters: int >= 1            (geomed: at most that many smoothed-Weiszfeld iterations, default 100; fewer
                                    once the objective moves by <= 1e-9 of itself)
  geomed-nu: float > 0              (geomed: the smoothing floor of the distances, default 1e-6, the RFA value)
  dnc-iters: int >= 1               (dnc: independent column sub-samples whose keep masks are intersected, default 1)
  dnc-sub-dim: int >= 1             (dnc: columns per sub-sample, default 10000; >= P uses every column)
  dnc-c: float > 0                  (dnc: the filtering fraction, ceil(c f) rows dropped per iteration, default 1.0)
  cclip-iters: int >= 1             (cclip: clipping iterations, all of them run, default 3; 1 = norm bounding)
  cclip-tau: auto | float > 0       (cclip: the clipping radius; auto, the default = the lower median of the rows'
                                    distances to the round's starting model, found on the device every round)
  foolsgold-kappa: float > 0        (foolsgold: the logit's confidence scale, default 1.0)
  signguard-frac: float > 0         (signguard: the fraction of the columns whose signs are counted, one contiguous
                                    window placed by the round's seed, default 0.1; >= 1 = every column)
  signguard-lo: float > 0           (signguard: a row passes the norm filter from lo times the median norm, default 0.1)
  signguard-hi: float > 0           (signguard: ... up to hi times the median norm, default 3.0; lo <= hi)
  flame-noise: float >= 0           (flame: the noise level lambda, sigma = lambda times the median norm of the round's
                                    updates, default 0.001, the paper's value for its main tasks; 0 = no noise)
  pre-agg: none | nnm | bucketing   (pre-aggregation in front of the rule of ``server.mode``, docs/PARITY.md; default
                                    none.  nnm: every row becomes the mean of its n - f nearest rows, itself included
                                    (f from byz-f, needs n >= 2 f + 3 when explicit); bucketing: the rows are shuffled
                                    with the round's seed and averaged in buckets of bucket-size, and the rule, its
                                    byz-f ``auto`` and its admissibility checks then see the ceil(n / bucket-size)
                                    bucket means.  Refused for fedavg, hyper, FLTrust, gmm and foolsgold, whose
                                    history is keyed by client: mixed rows have no identity)
  bucket-size: int >= 1             (bucketing: rows per bucket, default 2; 1 leaves the rows as they are)
  save-state: bool                  (write {model}.state.pt + {model}.clients.r{rank}.pt every round)
  resume: bool                      (continue from those files: counters, RNGs, optimizer moments)
"""
from __future__ import annotations

import copy
import os
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

import yaml

SERVER_MODES = ("fedavg", "hyper", "FLTrust", "trimmed_mean", "shieldfl", "gmm", "krum", "median", "scionfl",
                "fltracer", "byzantine", "multi_krum", "bulyan", "geomed", "dnc", "cclip", "foolsgold", "signguard",
                "flame")
ATTACK_MODES = ("Random", "Min-Max", "Min-Sum", "Opt-Fang", "LIE", "AGR-Krum", "AGR-MKrum", "AGR-Bulyan")
# the AGR-tailored attacks (beyond the reference; docs/PARITY.md) and the rule each one models
AGR_ATTACK_TARGETS = {"AGR-Krum": "krum", "AGR-MKrum": "mkrum", "AGR-Bulyan": "bulyan"}


def agr_attack_args(mode: str, args) -> tuple:
    """``attack_args = [m, f, dev]`` of an AGR-tailored attack, all optional -> (m, f, dev) as ints: m >= 1 identical
    malicious copies the attacker assumes (default 1), f the Byzantine count it assumes the rule runs with (default m;
    f = 0, this project's ``server.mode: krum`` (A-11), only for AGR-Krum), dev 0 = unbiased std, 1 = sign(mean),
    2 = mean / ||mean||_2.  A non-integer or out-of-range value raises ValueError."""
    vals = [float(a) for a in (args or [])]
    if len(vals) > 3:
        raise ValueError(f"{mode} takes at most 3 attack args [m, f, dev] (got {vals})")
    for name, v in zip(("m", "f", "dev"), vals):
        if v != v or v != int(v):
            raise ValueError(f"{mode}: attack arg {name} must be an integer (got {v})")
    m = int(vals[0]) if len(vals) > 0 else 1
    f = int(vals[1]) if len(vals) > 1 else m
    dev = int(vals[2]) if len(vals) > 2 else 0
    fmin = 0 if mode == "AGR-Krum" else 1
    if m < 1 or f < fmin or dev not in (0, 1, 2):
        raise ValueError(f"{mode}: attack args [m, f, dev] need m >= 1, f >= {fmin} and dev in 0 / 1 / 2 "
                         f"(got m = {m}, f = {f}, dev = {dev})")
    return m, f, dev
MODEL_NAMES = ("CNNModel", "RNNModel", "TransformerModel", "TransformerClassifier")
DATA_NAMES = ("ICU", "HAR", "CIFAR10")

REFERENCE_DEFAULTS: Dict[str, Any] = {
    "name": "Federated Learning poisoning attack testbed",
    "server": {
        "num-round": 30,
        "clients": 3,
        "mode": "hyper",
        "hyper-detection": {"enable": False, "cosine-search": 10, "n_components": 3, "eps": 0.007,
                            "min_samples": 3},
        "model": "TransformerModel",
        "data-name": "ICU",
        "parameters": {"load": False},
        "validation": True,
        "data-distribution": {"num-data-range": [12000, 15000]},
        "genuine-rate": 0.5,
        "random-seed": 1,
    },
    "rabbit": {"address": "192.0.0.1", "username": "admin", "password": "admin"},
    "log_path": ".",
    "learning": {"epoch": 5, "learning-rate": 0.004, "hyper-lr": 0.001, "momentum": 0.5, "batch-size": 128,
                 "clip-grad-norm": 1.0},
}


@dataclass(frozen=True)
class RuleKnob:
    """One engine knob of a server rule: the ``engine:`` key, the keyword the rule receives, what it holds (``kind``
    "int" >= ``lo``, unchecked when ``lo`` is None, "number" > 0, or "number0" >= 0 and finite; ``auto``: or the string
    "auto") and the default.
    Stated once, in RULE_KNOBS: the engine defaults, ``validate``, ``FLEngine._rule_args`` and the rules (``agg``)
    read it."""
    key: str
    kw: str
    kind: str
    default: Any
    lo: Optional[int] = None
    auto: bool = False

    def check(self, v, where: str = "", coerce: bool = False):
        """-> ``v`` when admissible, else ValueError.  A bool never is; a string only as a "number" (YAML 1.1 reads
        "1e-6", without a dot, as a string); NaN is neither > 0 nor >= 0.  ``coerce`` (the engine's keywords, a rule's
        own arguments): None counts as "auto", any other value goes through ``int`` / ``float`` first."""
        if self.auto and ((isinstance(v, str) and v == "auto") or (coerce and v is None)):
            return "auto"
        if coerce:
            v = int(v) if self.kind == "int" else float(v)
        if self.kind == "int" and self.lo is None:
            return v
        try:
            ok = not isinstance(v, bool) and ((isinstance(v, int) and v >= self.lo) if self.kind == "int"
                                              else float(v) > 0 if self.kind == "number"
                                              else 0 <= float(v) < float("inf"))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            what = (f"an integer >= {self.lo}" if self.kind == "int" else "a number > 0" if self.kind == "number"
                    else "a finite number >= 0")
            what = "'auto' or " + what if self.auto else what
            raise ValueError(f"{where}{self.key} must be {what} (got {v!r})")
        return v


RULE_KNOBS = (  # engine key, rule keyword, kind, default, lo, auto  (what each one means: the module docstring)
    RuleKnob("gmm-rank", "gmm_rank", "int", 1),
    RuleKnob("byz-f", "byz_f", "int", "auto", 0, True),
    RuleKnob("geomed-iters", "geomed_iters", "int", 100, 1),
    RuleKnob("geomed-nu", "geomed_nu", "number", 1e-6),
    RuleKnob("dnc-iters", "dnc_iters", "int", 1, 1),
    RuleKnob("dnc-sub-dim", "dnc_sub_dim", "int", 10000, 1),
    RuleKnob("dnc-c", "dnc_c", "number", 1.0),
    RuleKnob("cclip-iters", "cclip_iters", "int", 3, 1),
    RuleKnob("cclip-tau", "cclip_tau", "number", "auto", None, True),
)
KNOB = {k.kw: k for k in RULE_KNOBS}

# pre-aggregation in front of a robust rule (``engine.pre-agg``; docs/PARITY.md): not rule knobs, the rules never see them
PRE_AGG_KINDS = ("none", "nnm", "bucketing")
# FedAvg has its own fused and all-reduce paths, the hypernetwork and FLTrust train, gmm reads per-row attacker flags,
# foolsgold keeps a history per client id (a mixed row belongs to no client)
PRE_AGG_REFUSED_MODES = ("fedavg", "hyper", "FLTrust", "gmm", "foolsgold")
BUCKET_SIZE = RuleKnob("bucket-size", "bucket_size", "int", 2, 1)
# foolsgold is stateful and lives outside agg.AGGREGATORS: its knob is not a keyword every rule receives either
FOOLSGOLD_KAPPA = RuleKnob("foolsgold-kappa", "foolsgold_kappa", "number", 1.0)
# signguard's knobs reach its rule through its own server mode (fl/server_modes.py SignGuardMode), not through the
# keywords every rule receives
SIGNGUARD_FRAC = RuleKnob("signguard-frac", "signguard_frac", "number", 0.1)
SIGNGUARD_LO = RuleKnob("signguard-lo", "signguard_lo", "number", 0.1)
SIGNGUARD_HI = RuleKnob("signguard-hi", "signguard_hi", "number", 3.0)
SIGNGUARD_KNOBS = (SIGNGUARD_FRAC, SIGNGUARD_LO, SIGNGUARD_HI)
# flame's knob, likewise through its own server mode (FlameMode): the noise level lambda, 0 = no noise
FLAME_NOISE = RuleKnob("flame-noise", "flame_noise", "number0", 0.001)

EXTENSION_DEFAULTS: Dict[str, Any] = {
    "comm": {"backend": "auto", "address": "", "port": 29517, "clients-per-rank": 0, "one-shot-allgather": "auto",
             "fedavg-allreduce": "auto", "timeout-s": 600, "attackers": {}},
    "data": {"synthetic": "auto", "train-size": 60000, "test-size": 10000, "seed": 1234,
             "har-train-size": 2048, "har-test-size": 512, "root": "."},
    "engine": {"trainer": "auto", "distance": "spectral", "seed": 0, "metrics": "", "checkpoint-dir": ".",
               "async-checkpoint": True, "compat-hyper-resume": False, "compat-fltrust": False, "max-retries": 50, "trace": False,
               "phase-sync": False, "fault-inject": [], "save-state": False, "resume": False,
               "speculative": True, "compat-har-train": False, "compat-fedavg-alias": False,
               **{k.key: k.default for k in RULE_KNOBS}, "pre-agg": "none", BUCKET_SIZE.key: BUCKET_SIZE.default,
               FOOLSGOLD_KAPPA.key: FOOLSGOLD_KAPPA.default, **{k.key: k.default for k in SIGNGUARD_KNOBS},
               FLAME_NOISE.key: FLAME_NOISE.default},
}


def _deep_merge(base: Dict[str, Any], over: Dict[str, Any]) -> Dict[str, Any]:
    out = copy.deepcopy(base)
    for k, v in (over or {}).items():
        if isinstance(v, dict) and isinstance(out.get(k), dict):
            out[k] = _deep_merge(out[k], v)
        else:
            out[k] = copy.deepcopy(v)
    return out


@dataclass
class AttackSpec:
    """One attacker's schedule.  ``gamma`` / ``tau`` are the Min-Max / Min-Sum / Opt-Fang bisection's start
    value and stop gap; the reference hard-codes them to 50 and 1 (``src/Utils.py:101,134,167``), which
    stay the defaults.  With those the tried γs are 50, 25, ..., 1.5625 and a candidate can only be
    accepted at γ ≥ 1.5625 (profiles/attack_study/README.md shows why that rarely passes the distance check).
    Left unset (None) they resolve to those 50 / 1 for the reference's five modes and to 10 / 0.02 for the AGR-tailored
    modes (10 is the start value of the NDSS 2021 paper's published code; 9 iterations, γ resolved to 0.04): a
    candidate that a Krum-type rule still selects sits at γ of about 1, below anything 50 / 1 can accept.  The AGR
    modes' ``args`` are ``[m, f, dev]`` (``agr_attack_args``), checked here, not at round ``round``."""
    mode: str
    round: int
    args: List[float] = field(default_factory=list)
    gamma: Optional[float] = None
    tau: Optional[float] = None

    def __post_init__(self):
        if self.mode not in ATTACK_MODES:
            raise ValueError(f"Attack mode '{self.mode}' is not valid (choose from {ATTACK_MODES}).")
        self.round = int(self.round)
        self.args = [float(a) for a in (self.args or [])]
        agr = self.mode in AGR_ATTACK_TARGETS
        if agr:
            agr_attack_args(self.mode, self.args)
        self.gamma = float((10.0 if agr else 50.0) if self.gamma is None else self.gamma)
        self.tau = float((0.02 if agr else 1.0) if self.tau is None else self.tau)
        if not (self.gamma > 0 and self.tau > 0):
            raise ValueError(f"bisection gamma / tau must be positive (got {self.gamma}, {self.tau})")

    def to_dict(self) -> Dict[str, Any]:
        return {"mode": self.mode, "round": self.round, "args": self.args, "gamma": self.gamma, "tau": self.tau}

    @classmethod
    def from_dict(cls, v: Dict[str, Any]) -> "AttackSpec":
        return cls(v["mode"], v.get("round", 1), v.get("args", []), v.get("gamma"), v.get("tau"))


@dataclass
class Config:
    raw: Dict[str, Any]

    # ---- server ----
    @property
    def num_round(self) -> int:
        return int(self.raw["server"]["num-round"])

    @property
    def clients(self) -> int:
        return int(self.raw["server"]["clients"])

    @property
    def mode(self) -> str:
        return str(self.raw["server"]["mode"])

    @property
    def model(self) -> str:
        return str(self.raw["server"]["model"])

    @property
    def data_name(self) -> str:
        return str(self.raw["server"]["data-name"])

    @property
    def load_parameters(self) -> bool:
        return bool(self.raw["server"]["parameters"]["load"])

    @property
    def validation(self) -> bool:
        return bool(self.raw["server"]["validation"])

    @property
    def data_range(self) -> List[int]:
        r = self.raw["server"]["data-distribution"]["num-data-range"]
        return [int(r[0]), int(r[1])]

    @property
    def genuine_rate(self) -> float:
        return float(self.raw["server"]["genuine-rate"])

    @property
    def random_seed(self):
        return self.raw["server"]["random-seed"]

    @property
    def hyper_detection(self) -> Dict[str, Any]:
        return self.raw["server"]["hyper-detection"]

    # ---- learning ----
    @property
    def epoch(self) -> int:
        return int(self.raw["learning"]["epoch"])

    @property
    def batch_size(self) -> int:
        return int(self.raw["learning"]["batch-size"])

    @property
    def lr(self) -> float:
        return float(self.raw["learning"]["learning-rate"])

    @property
    def hyper_lr(self) -> float:
        return float(self.raw["learning"]["hyper-lr"])

    @property
    def momentum(self) -> float:
        return float(self.raw["learning"]["momentum"])

    @property
    def clip_grad_norm(self) -> float:
        return float(self.raw["learning"].get("clip-grad-norm", 0.0))

    @property
    def log_path(self) -> str:
        return str(self.raw["log_path"])

    # ---- extensions ----
    @property
    def comm(self) -> Dict[str, Any]:
        return self.raw["comm"]

    @property
    def data(self) -> Dict[str, Any]:
        return self.raw["data"]

    @property
    def engine(self) -> Dict[str, Any]:
        return self.raw["engine"]

    def attackers(self) -> Dict[int, AttackSpec]:
        out: Dict[int, AttackSpec] = {}
        for k, v in (self.raw["comm"].get("attackers") or {}).items():
            out[int(k)] = AttackSpec.from_dict(v)
        return out

    def validate(self) -> "Config":
        if self.mode not in SERVER_MODES:
            raise ValueError(f"Server mode '{self.mode}' is not valid.")
        if self.model not in MODEL_NAMES:
            raise ValueError(f"Model name '{self.model}' is not valid.")
        if self.data_name not in DATA_NAMES:
            raise ValueError(f"Data name '{self.data_name}' is not valid.")
        lo, hi = self.data_range
        if lo > hi or lo < 0:
            raise ValueError(f"num-data-range {self.data_range} is invalid")
        if self.clients < 1:
            raise ValueError("server.clients must be >= 1")
        if self.engine["distance"] not in ("spectral", "flat"):
            raise ValueError("engine.distance must be 'spectral' or 'flat'")
        for k in RULE_KNOBS:
            k.check(self.engine.get(k.key, k.default), "engine.")
        pre = self.engine.get("pre-agg", "none")
        if not isinstance(pre, str) or pre not in PRE_AGG_KINDS:
            raise ValueError(f"engine.pre-agg must be one of {PRE_AGG_KINDS} (got {pre!r})")
        BUCKET_SIZE.check(self.engine.get(BUCKET_SIZE.key, BUCKET_SIZE.default), "engine.")
        FOOLSGOLD_KAPPA.check(self.engine.get(FOOLSGOLD_KAPPA.key, FOOLSGOLD_KAPPA.default), "engine.")
        sg = [k.check(self.engine.get(k.key, k.default), "engine.") for k in SIGNGUARD_KNOBS]
        if float(sg[1]) > float(sg[2]):
            raise ValueError(f"engine.signguard-lo must be <= engine.signguard-hi (got {sg[1]!r}, {sg[2]!r})")
        FLAME_NOISE.check(self.engine.get(FLAME_NOISE.key, FLAME_NOISE.default), "engine.")
        if pre != "none" and self.mode in PRE_AGG_REFUSED_MODES:
            raise ValueError(f"engine.pre-agg: {pre} does not apply to server.mode '{self.mode}' (it goes in front of "
                             f"a robust rule; not {', '.join(PRE_AGG_REFUSED_MODES)})")
        return self

    def to_dict(self) -> Dict[str, Any]:
        return copy.deepcopy(self.raw)


def from_dict(d: Optional[Dict[str, Any]] = None) -> Config:
    raw = _deep_merge(REFERENCE_DEFAULTS, {})
    raw = _deep_merge(raw, EXTENSION_DEFAULTS)
    raw = _deep_merge(raw, d or {})
    return Config(raw).validate()


def load_config(path: str = "config.yaml", overrides: Optional[Dict[str, Any]] = None) -> Config:
    """Load ``config.yaml`` (reference schema + optional extensions)."""
    d: Dict[str, Any] = {}
    if path and os.path.exists(path):
        with open(path, "r") as fh:
            d = yaml.safe_load(fh) or {}
    elif path and path != "config.yaml":
        raise FileNotFoundError(path)
    if overrides:
        d = _deep_merge(d, overrides)
    return from_dict(d)
