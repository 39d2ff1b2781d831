"""SPMD federated-learning round engine.

Replaces the reference's broker-driven state machines — server ``on_request`` /
``process_consumer`` / ``notify_clients`` (``server.py:205-624``) and client
``RpcClient.response_message`` (``src/RpcClient.py:64-172``) — with one synchronous loop that
every rank runs:

  START  (replicated decisions: per-client parameters, attackers' genuine-model sample)
  LOCAL  (this rank's clients: fused training kernel for all genuine clients at once, attacks)
  GATHER (one all-gather of fixed-layout ``[slots, W]`` blocks  == the UPDATE messages)
  SERVER (replicated aggregation/defense/hypernetwork update — deterministic kernels)
  CHECK  (replicated validation and hyper-detection decision; the leader logs and checkpoints)
  NEXT   (retry the same round on failure, exactly like the reference's ``round`` counter)

Server state is replicated on every rank instead of living in one process, and every decision that
ends a round (validation, detection) is computed by deterministic kernels on identical inputs on
every rank, so the only traffic per round is the update all-gather (or, for plain FedAvg over
RCCL, one all-reduce): no control broadcast, and the next round's training can be enqueued before
this round's validation at any world size (speculative launch, ``run_round``).
"""
from __future__ import annotations

import atexit
import contextlib
import os
import random
import time
import uuid
import weakref
import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import ops
from ..agg import AGGREGATORS
from ..agg import host_info as agg_host_info
from ..attacks import DistanceEngine, host_info, run_attack
from ..config import RULE_KNOBS, AttackSpec, Config
from ..data import DeviceTable, resolve_dataset
from ..detect import HyperDetector
from ..eval import Validation
from ..models import ParamLayout, build_model
from ..ops import onchip
from ..parallel.comm import Comm, LoopbackComm
from ..utils import trace
from ..utils.ckpt import CheckpointWriter
from ..utils.log import Logger, MetricsWriter, NullLogger, print_with_color
from .hyper_server import HyperServer
from .server_modes import MODES, ServerMode
from .trainers import Pending, Plan, make_plan, make_trainer

# every rule of AGGREGATORS runs on the device without a host read (gmm, signguard and flame up to 64 rows; gmm's
# success is a device bool): with one of them the aggregate and the next round's launch are enqueued before the host
# waits for the training, as for FedAvg, FLTrust and the native hypernetwork update (ServerMode.early_ok, FLEngine._early_launch)
EARLY_AGGREGATORS = tuple(m for m in AGGREGATORS if m != "fedavg")

META = 5  # valid, result, size, is_attacker, decision word; then the client's per-epoch losses (E columns)
DECISION = 4  # column of the sender's decision word (``FLEngine._decision_word``)


class Staging:
    """Per-round host metadata -> device in ONE copy: the arrays are packed (8-byte aligned) into a
    reused pinned buffer, copied with one non-blocking H2D copy into a reused device buffer, and returned
    as typed device views — built once per layout (the same shapes every round), because the ~18 tensor
    view ops per round cost more host time than the copy.  Two buffers alternate, so the next round's
    metadata can be staged (``FLEngine._prepare_local``) while kernels of the current round that read the
    previous views are still queued; a buffer's copy is stream-ordered after the kernels of the round
    before that read it.  On a CPU device the arrays are simply wrapped."""

    SLOTS = 2

    def __init__(self, device: torch.device):
        self.device = torch.device(device)
        self._slots = [{"host": None, "dev": None, "done": None, "views": {}} for _ in range(self.SLOTS)]
        self._next = 0

    def upload(self, arrays: Sequence[np.ndarray]) -> List[torch.Tensor]:
        if self.device.type != "cuda":
            return [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]
        sl = self._slots[self._next]
        self._next = (self._next + 1) % self.SLOTS
        offs, n = [], 0
        for a in arrays:
            offs.append(n)
            n += (a.nbytes + 7) // 8 * 8
        n = max(n, 8)
        if sl["host"] is None or sl["host"].numel() < n:
            sl["host"] = torch.empty(max(n, 4096), dtype=torch.uint8, pin_memory=True)
            sl["dev"] = torch.empty(sl["host"].numel(), dtype=torch.uint8, device=self.device)
            sl["views"].clear()
        elif sl["done"] is not None:
            sl["done"].synchronize()  # this buffer's last copy finished long ago; never overwrite one in flight
        hb = sl["host"].numpy()
        for a, o in zip(arrays, offs):
            hb[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        sl["dev"][:n].copy_(sl["host"][:n], non_blocking=True)
        if sl["done"] is None:
            sl["done"] = torch.cuda.Event()
        sl["done"].record(torch.cuda.current_stream(self.device))
        key = tuple((a.shape, a.dtype.str) for a in arrays)
        out = sl["views"].get(key)
        if out is None:
            out = []
            for a, o in zip(arrays, offs):
                t = sl["dev"][o:o + a.nbytes].view(_TORCH_DT[a.dtype.str[1:]])
                out.append(t.reshape(a.shape))
            sl["views"][key] = out
        return out


def _no_dev_seed(s: int) -> int:
    return 0


_TORCH_DT = {"f4": torch.float32, "i4": torch.int32, "i8": torch.int64, "f8": torch.float64}


@dataclass
class ClientInfo:
    index: int
    uuid: str
    owner: int
    attack: Optional[AttackSpec] = None


@dataclass
class LocalClient:
    info: ClientInfo
    rng: random.Random
    seed: int
    training_round: int = 0
    genuine: Optional[torch.Tensor] = None     # last received genuine models [K, P]


def build_client_table(cfg: Config, world: int, attackers: Optional[Dict[int, AttackSpec]] = None,
                       clients_per_rank: int = 0) -> List[ClientInfo]:
    """Packed placement: client c lives on rank c // ceil(N / world) (contiguous blocks)."""
    n = cfg.clients
    cpr = clients_per_rank or -(-n // world)
    atk = attackers if attackers is not None else cfg.attackers()
    seed = int(cfg.engine.get("seed", 0))
    table = []
    for c in range(n):
        owner = min(c // cpr, world - 1)
        uid = str(uuid.UUID(int=(seed * 1000003 + c + 1) & ((1 << 128) - 1), version=4))
        table.append(ClientInfo(c, uid, owner, atk.get(c)))
    return table


@dataclass(slots=True)
class Prepared:
    """Host half of a launch (``FLEngine._prepare_local``).  The fields from ``dec`` on are staged for those attack
    decisions by ``FLEngine._stage``, and staged again if an attacker's first attack round flips them."""
    tq: float                                # host clock when the preparation began
    meta: np.ndarray                         # [slots, META + E] host mirror of the block's meta columns and losses
    clients: List[tuple]                     # (local row, client, LocalClient, num_data) of every started client
    js: List[int]                            # their local rows
    faults: List[int]                        # local rows poisoned with NaN before this training (fault injection)
    selected: tuple                          # the selection it was prepared for
    dec: tuple = ()                          # per started client: attacks instead of training
    train_rows: Optional[List[int]] = None   # local rows in the training launch (attackers ride along with 0 rows)
    train_seeds: Optional[List[int]] = None  # their dropout seeds
    meta_d: Optional[torch.Tensor] = None    # meta[:, :META] on the device
    js_d: Optional[torch.Tensor] = None      # js on the device
    rows_d: Optional[torch.Tensor] = None    # train_rows on the device
    tseed_d: Optional[torch.Tensor] = None   # train_seeds on the device, in the trainer's int32 form
    plan: Optional[Plan] = None              # the training rows' sampling plan (None: nobody trains)
    fedavg_w: Optional[torch.Tensor] = None  # one rank, every selected row stored: FedAvg weights on the device
    sizes_h: Optional[torch.Tensor] = None   # one rank: the selected clients' sizes (fp64, host)
    tq1: float = 0.0                         # host clock at the start of the staging, and after its upload
    tq2: float = 0.0
    staged_ev: Optional["torch.cuda.Event"] = None  # staged on the staging stream: the launch waits for this


@dataclass(slots=True)
class Launch:
    """Device half of a launch (``FLEngine._enqueue_local``) and, once ``_finish_local`` ran, its outcome: the
    meta mirror ``prep.meta`` completed with the ok flags and losses, the filled ``block``, ``lw_times``."""
    prep: Prepared
    block: Optional[torch.Tensor]            # this rank's update block [slots, W]; None: plain rows
    plain: bool                              # one rank, all trained in place: local_params ARE the update rows
    in_place: bool                           # every local client is in the launch: local_params trained in place
    params: Optional[torch.Tensor]           # the rows handed to the trainer (None: nobody trains)
    pending: Optional[Pending]               # the training launch (None: nobody trains)
    attack_jobs: List[tuple]                 # (local row, client, LocalClient, AttackSpec) of this round's attacks
    ready: Optional["torch.cuda.Event"]      # the attackers' inputs are complete (before the training launch)
    t_enqueue: float                         # host time from the enqueue's start to the training launch
    t_launch: float                          # host time of the training launch itself
    atk_out: Optional[List[tuple]] = None    # (local row, ok, malicious update); None until _finish_attacks ran
    tw: float = 0.0                          # host clock before and after the attacks
    tp2: float = 0.0
    lw_times: Optional[Dict[str, float]] = None  # the round record's t_lw_* entries


@dataclass
class EarlyLaunch:
    """An early launch (``FLEngine._early_launch``): what its server step reported and what undoing it needs."""
    g_old: Optional[torch.Tensor]            # the global model before the step
    mode_mark: object                        # the server mode's ``mark()`` before the step, for its ``undo``
    snap: tuple                              # (per local client (rng state, training round, genuine), server rng state)
    prep: Optional[Prepared]                 # the next launch's host half, staged ahead
    info: dict = field(default_factory=dict)  # the server step's info
    rule_ok: Optional[tuple] = None          # gmm: (pinned bool, event) of the filter's success
    keep: Optional[List[int]] = None         # with attackers: the genuine rows stored, and the pool made of them
    pool: Optional[torch.Tensor] = None
    agg_done: Optional["torch.cuda.Event"] = None


_LIVE: "weakref.WeakSet[FLEngine]" = weakref.WeakSet()


@atexit.register
def _close_live_engines():
    """Interpreter exit: close every engine its script did not close (a pending speculative launch and the
    checkpoint writer thread would otherwise still run while the runtime tears down: abort at exit)."""
    for eng in list(_LIVE):
        try:
            eng.close()
        except Exception:  # noqa: BLE001 (best effort at exit)
            pass


class FLEngine:
    def __init__(self, cfg: Config, comm: Optional[Comm] = None, table: Optional[List[ClientInfo]] = None,
                 device=None, leader: Optional[bool] = None, verbose: bool = True, train_dataset=None,
                 test_dataset=None):
        _LIVE.add(self)
        self._closed = False  # (before anything below can raise: the exit hook closes half-built engines too)
        self.cfg = cfg
        self.comm = comm or LoopbackComm(device or "cpu")
        self.device = torch.device(device) if device is not None else self.comm.device
        self.rank = self.comm.rank
        self.world = self.comm.world
        self.leader = (self.rank == 0) if leader is None else leader
        self.verbose = verbose and self.leader
        self.table = table if table is not None else build_client_table(cfg, self.world)
        self.n_clients = len(self.table)
        self.mode = cfg.mode
        self.model_name = cfg.model
        self.data_name = cfg.data_name
        self.seed = int(cfg.engine.get("seed", 0))
        self.ckpt_dir = cfg.engine.get("checkpoint-dir", ".")
        self.ckpt_writer = CheckpointWriter(bool(cfg.engine.get("async-checkpoint", True)))
        # synchronise after the aggregate so t_aggregate / t_validate are device times (diagnostics only)
        self.phase_sync = bool(cfg.engine.get("phase-sync", False))
        self._saved_params: Optional[torch.Tensor] = None
        self.max_retries = int(cfg.engine.get("max-retries", 50))
        self.layout = ParamLayout.for_model(self.model_name)
        self.P = self.layout.P
        self.E = cfg.epoch
        # update block row: [P update | META | E epoch losses], padded to 16 bytes (aligned IPC pushes)
        self.W = (self.P + META + self.E + 3) // 4 * 4
        self.dist = DistanceEngine(self.layout, cfg.engine.get("distance", "spectral"))

        # ---- logging (leader only, like the reference's single server process) ----
        if self.leader:
            os.makedirs(cfg.log_path, exist_ok=True)
            self.logger = Logger(os.path.join(cfg.log_path, "app.log"))
            self.metrics = MetricsWriter(cfg.engine.get("metrics") or None)
        else:
            self.logger = NullLogger()
            self.metrics = MetricsWriter(None)

        # ---- data (train set shared by all clients, resident on this rank's device) ----
        self.local = [LocalClient(ci, random.Random(self.seed * 7919 + ci.index), self.seed * 104729 + ci.index)
                      for ci in self.table if ci.owner == self.rank]
        mode_cls = MODES[self.mode]  # (the one place that maps the mode's name to its ServerMode)
        need_train = len(self.local) > 0 or mode_cls.needs_train_table
        self.train_table = None
        if need_train:
            ds = train_dataset if train_dataset is not None else resolve_dataset(self.data_name, "train", cfg.data,
                                                                                 verbose=self.verbose)
            self.train_table = DeviceTable(ds, self.device)
        self.trainer = make_trainer(cfg.engine.get("trainer", "auto"), self.model_name, self.data_name,
                                    self.train_table, self.device) if self.train_table is not None else None
        if self.trainer is not None and hasattr(self.trainer, "compat_har"):
            self.trainer.compat_har = bool(cfg.engine.get("compat-har-train", False))
        # validation runs on EVERY rank: its kernels are deterministic and the global model is bit-identical
        # on all ranks, so each rank reaches the leader's decision without a control broadcast
        self.validation = None
        if cfg.validation:
            self.validation = Validation(self.model_name, self.data_name, self.logger, self.device, cfg.data,
                                         dataset=test_dataset, verbose=self.verbose)
        self.slots = max(sum(1 for ci in self.table if ci.owner == r) for r in range(self.world))
        # persistent per-client models (the reference's ``RpcClient.model``), own random init (A-16)
        self.local_params = torch.zeros(max(1, len(self.local)), self.P, dtype=torch.float32, device=self.device)
        for j, lc in enumerate(self.local):
            m = build_model(self.model_name, seed=lc.seed)
            self.local_params[j].copy_(self.layout.flatten(m.state_dict(), device=self.device))

        # ---- server state (replicated) ----
        self.server_rng = random.Random(cfg.random_seed) if cfg.random_seed else random.Random()
        self.global_params: Optional[torch.Tensor] = None
        self.selected: List[int] = []
        self._selection_done = False
        self.genuine_pool: Optional[torch.Tensor] = None
        self.hyper: Optional[HyperServer] = None      # (both set by HyperMode)
        self.detector: Optional[HyperDetector] = None
        self.torch_gen = torch.Generator(device=self.device if self.device.type == "cuda" else "cpu")
        self.torch_gen.manual_seed(self.seed * 31337 + self.rank)
        self.server: ServerMode = mode_cls(self)  # the mode's work and its state (fl/server_modes.py)
        self.round_no = 1
        self.rounds_left = cfg.num_round
        self.history: List[dict] = []
        if cfg.engine.get("trace", False):
            trace.enable(True)
        # fault injection: [{client: i, round: r}] -> client i's model is NaN-poisoned before
        # its local training of training-round r, which fails that client and retries the FL round
        self.faults = {(int(f["client"]), int(f["round"])) for f in (cfg.engine.get("fault-inject") or [])}
        # FedAvg fast path: with no attacker and no detection, the server needs only
        # sum_i s_i w_i and sum_i s_i -> ONE all_reduce of [P + 5] (+ #failed, #reported, the decision word and its
        # square) instead of the [N, P] all-gather
        # auto = world > 1 without the IPC one-shot gather (which moves whole blocks in one stream-ordered hop
        # and keeps FedAvg on the same deterministic kernel as a single rank)
        fa = str(cfg.comm.get("fedavg-allreduce", "auto")).lower()
        eligible = (self.mode == "fedavg" and all(ci.attack is None for ci in self.table)
                    and not cfg.hyper_detection.get("enable", False))
        self.fast_fedavg = eligible and (fa == "true" or (fa == "auto" and self.world > 1
                                                          and not getattr(self.comm, "one_shot", False)))
        # speculative next-round launch (run_round): replicated-state modes whose retry of a failed round
        # relaunches exactly the same client work (no detection, START from the in-memory global model /
        # hypernetwork; attackers draw from the pool set before the launch), no resume sidecars.  Any world
        # size: validation is replicated, so no rank waits for another's decision before the next launch.
        self._spec: Optional[Launch] = None  # the next round's launch, enqueued ahead (speculative / early)
        self._next_prep: Optional[Prepared] = None  # the next launch's host half, staged while this training runs
        self._start_ready = None  # event: the latest launch's START models are generated (the validation stream waits)
        self._attack_info = None  # the round in progress: the last attack's info
        self._sel_cache = None
        self._rows_idx: dict = {}  # _take_rows: index lists already on the device
        self._staging = Staging(self.device)
        # created on first use: GPU streams, the meta read's pinned buffer
        self._val_stream = self._side = self._stage_stream = self._meta_pinned = None
        self._has_attackers = any(ci.attack is not None for ci in self.table)
        self._speculative = (bool(cfg.engine.get("speculative", True)) and self.device.type == "cuda"
                             and not cfg.hyper_detection.get("enable", False) and not cfg.load_parameters
                             and not cfg.engine.get("save-state", False) and not self.phase_sync
                             and self.trainer is not None)
        if cfg.engine.get("resume", False):
            self.load_state()
        self.logger.log_info("### Application start ###\n")

    # ------------------------------------------------------------------------------------------
    # server init / checkpoint
    # ------------------------------------------------------------------------------------------
    def _pth(self, hyper: bool = False) -> str:
        if hyper:
            return os.path.join(self.ckpt_dir, f"{self.model_name}_hyper_{self.cfg.clients}.pth")
        return os.path.join(self.ckpt_dir, f"{self.model_name}.pth")

    def save_checkpoint(self):
        """Reference ``server.py:551-553`` (same files and keys).  Every rank remembers the saved
        global model (what ``{model}.pth`` now holds) so ``load: True`` rounds need no file read;
        the leader writes the mode's file in the background (``ServerMode.checkpoint``, ``utils/ckpt.py``)."""
        if self.global_params is not None:  # (the hypernetwork's rounds have none)
            self._saved_params = self.global_params.detach().clone()
        if not self.leader:
            return
        os.makedirs(self.ckpt_dir, exist_ok=True)
        self.server.checkpoint()

    # ---- resumable run state (new: the reference persists only the model) ----
    def _state_paths(self):
        base = os.path.join(self.ckpt_dir, self.model_name)
        return base + ".state.pt", f"{base}.clients.r{self.rank}.pt"

    def save_state(self) -> None:
        """Replicated server state (leader) + this rank's client state, loadable with
        ``torch.load(weights_only=True)``: round counters, RNG states, hypernetwork Adam moments,
        the genuine pool attackers sample from, and every local client's model and RNG."""
        os.makedirs(self.ckpt_dir, exist_ok=True)
        srv_path, cli_path = self._state_paths()
        if self.leader:
            v, st, gauss = self.server_rng.getstate()
            srv = {"round_no": self.round_no, "rounds_left": self.rounds_left, "rng_version": v,
                   "rng_state": list(st), "rng_gauss": gauss, "selected": list(self.selected),
                   "global": self.global_params.detach().cpu() if self.global_params is not None else None,
                   "genuine_pool": self.genuine_pool.detach().cpu() if self.genuine_pool is not None else None,
                   **self.server.state()}
            torch.save(srv, srv_path + ".tmp")
            os.replace(srv_path + ".tmp", srv_path)
        cli = {"params": self.local_params.detach().cpu(), "index": [lc.info.index for lc in self.local],
               "training_round": [lc.training_round for lc in self.local],
               "rng": [[lc.rng.getstate()[0], list(lc.rng.getstate()[1]), lc.rng.getstate()[2]] for lc in self.local]}
        torch.save(cli, cli_path + ".tmp")
        os.replace(cli_path + ".tmp", cli_path)

    def load_state(self) -> bool:
        srv_path, cli_path = self._state_paths()
        if not os.path.exists(srv_path):
            return False
        srv = torch.load(srv_path, weights_only=True, map_location="cpu")
        self.round_no = int(srv["round_no"])
        self.rounds_left = int(srv["rounds_left"])
        self.server_rng.setstate((srv["rng_version"], tuple(srv["rng_state"]), srv["rng_gauss"]))
        if srv.get("selected"):
            self.selected = list(srv["selected"])
            self._selection_done = True
        if srv.get("global") is not None:
            self.global_params = srv["global"].to(self.device)
        if srv.get("genuine_pool") is not None:
            self.genuine_pool = srv["genuine_pool"].to(self.device)
        self.server.load(srv)
        if os.path.exists(cli_path):
            cli = torch.load(cli_path, weights_only=True, map_location="cpu")
            self.local_params.copy_(cli["params"].to(self.device))
            for lc, tr, rs in zip(self.local, cli["training_round"], cli["rng"]):
                lc.training_round = int(tr)
                lc.rng.setstate((rs[0], tuple(rs[1]), rs[2]))
        print_with_color(f"Resumed run state from {srv_path} at round {self.round_no}", "yellow")
        return True

    # ------------------------------------------------------------------------------------------
    # START
    # ------------------------------------------------------------------------------------------
    def client_selection(self):
        self._selection_done = True
        self.selected = list(range(self.n_clients))
        self.logger.log_info(f"Active with {len(self.selected)} client: {self.selected}")

    def _start_params(self) -> Optional[torch.Tensor]:
        """The model every client starts the round from, where the mode has one (``ServerMode.start``)."""
        if self.cfg.load_parameters:
            if self._saved_params is not None:  # == the file this run last wrote
                return self._saved_params
            self.ckpt_writer.flush()
            p = self._pth(False)
            if os.path.exists(p):
                return self.layout.flatten(torch.load(p, weights_only=True, map_location="cpu"), device=self.device)
            return None
        return self.global_params

    def _genuine_for_attackers(self) -> Dict[int, Optional[torch.Tensor]]:
        """Replicated: every rank draws the same sample for every attacker (server RNG in sync)."""
        out: Dict[int, Optional[torch.Tensor]] = {}
        pool = self.genuine_pool
        for i in self.selected:
            ci = self.table[i]
            if ci.attack is None:
                continue
            if pool is not None and pool.shape[0] > 0:
                G = pool.shape[0]
                k = max(int(self.cfg.genuine_rate * G), 1)
                idx = self.server_rng.sample(range(G), k)
                out[i] = self._take_rows(pool, idx) if ci.owner == self.rank else None
            else:
                out[i] = None
        return out

    def _take_rows(self, pool: torch.Tensor, idx: List[int]) -> torch.Tensor:
        """``pool[idx]`` with the index list on the device through a small cache and a pinned, non-blocking
        upload: indexing a device tensor with a Python list (or a pageable ``.to``) makes a pageable host ->
        device copy, which synchronises the stream — the host would wait for the training launch already
        enqueued, the early launch's whole point (a random genuine sample misses the cache most rounds)."""
        if pool.device.type != "cuda":
            return pool[idx]
        from ..ops.layers import upload

        key = tuple(idx)
        cache = self._rows_idx
        ix = cache.get(key)
        if ix is None:
            if len(cache) > 1024:
                cache.clear()
            ix = cache[key] = upload(torch.tensor(idx, dtype=torch.long), pool.device)
        return pool.index_select(0, ix)

    # ------------------------------------------------------------------------------------------
    # LOCAL
    # ------------------------------------------------------------------------------------------
    @property
    def _dev_seed(self):
        ds = getattr(self.trainer, "device_seed", None)
        return ds if (ds is not None and self.device.type == "cuda") else _no_dev_seed

    def _side_stream(self):
        if self.device.type != "cuda":
            return None
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        return self._side

    def _launch_local(self, genuine: Dict[int, Optional[torch.Tensor]]) -> Launch:
        """Prepare this rank's clients for the round and enqueue the genuine clients' training (async).
        Uses the preparation staged ahead by ``run_round`` when there is one."""
        prep, self._next_prep = self._next_prep, None
        if prep is None or prep.selected != tuple(self.selected):
            prep = self._prepare_local()
        return self._enqueue_local(prep, genuine)

    def _prepare_local(self) -> Prepared:
        """Host half of a launch — client counters, the data draws, fault injection, the plan — none of which
        depends on the previous round's outcome, so ``run_round`` stages the NEXT launch's half before it
        waits for the current training (the draws are the same whenever they happen: one per launch, in
        launch order).  Uploads and the plan kernel are enqueued here; which clients attack is re-checked at
        enqueue time (an attacker's first attack round waits for its genuine sample)."""
        tq = time.perf_counter()
        cfg = self.cfg
        meta = np.zeros((self.slots, META + self.E), dtype=np.float32)  # host-built, uploaded once (+ losses)
        lo, hi = cfg.data_range
        clients, faults = [], []
        for j, lc in enumerate(self.local):
            i = lc.info.index
            if i not in self.selected:
                continue
            lc.training_round += 1
            if (i, lc.training_round) in self.faults:
                faults.append(j)
                print_with_color(f"[fault-inject] client {i} poisoned with NaN (training round {lc.training_round})",
                                 "red")
            num_data = lc.rng.randrange(lo, hi + 1)
            meta[j, 0] = 1.0
            meta[j, 2] = float(num_data)
            meta[j, 3] = 1.0 if lc.info.attack is not None else 0.0
            clients.append((j, i, lc, num_data))
        prep = Prepared(tq, meta, clients, [j for j, _, _, _ in clients], faults, tuple(self.selected))
        self._stage(prep, self._attack_decisions(prep))
        return prep

    def _prepare_staged(self) -> Prepared:
        """``_prepare_local`` with its device half (the upload and the plan kernel) on a staging stream: those
        depend on nothing the running training writes, and on the compute stream they sat behind it, in the gap
        between two training kernels.  The launch waits for the staging event (``_enqueue_local``)."""
        dev = self.device
        if dev.type != "cuda":
            return self._prepare_local()
        if self._stage_stream is None:
            self._stage_stream = torch.cuda.Stream(device=dev)
        main = torch.cuda.current_stream(dev)
        with torch.cuda.stream(self._stage_stream):
            prep = self._prepare_local()
            prep.staged_ev = torch.cuda.Event()
            prep.staged_ev.record(self._stage_stream)
        if prep.plan is not None and prep.plan.order.is_cuda:
            prep.plan.order.record_stream(main)  # (allocated on the staging stream, read by the launch on main)
        return prep

    @staticmethod
    def _attack_decisions(prep: Prepared) -> tuple:
        return tuple(lc.info.attack is not None and lc.training_round >= lc.info.attack.round
                     and lc.genuine is not None and lc.genuine.shape[0] > 0 for _, _, lc, _ in prep.clients)

    def _stage(self, prep: Prepared, decisions: tuple) -> None:
        """Training rows / sizes / seeds for the given attack decisions, their ONE upload and the plan."""
        cfg, dev = self.cfg, self.device
        prep.dec, prep.tq1 = decisions, time.perf_counter()
        train_rows, train_nd, train_seeds, attack_rows = [], [], [], []
        for (j, i, lc, num_data), atk in zip(prep.clients, decisions):
            if atk:
                attack_rows.append((j, lc))
            else:
                train_rows.append(j)
                train_nd.append(num_data)
                train_seeds.append(lc.seed * 7 + lc.training_round)
        if train_rows and attack_rows:
            # the attackers ride along with ZERO rows (nd = 0: the trainer leaves their models untouched), so the
            # launch covers every local client in place — no gather / scatter of the trained rows — and their
            # attack results are written into their local_params rows once the launch is done (_finish_local)
            for j, lc in attack_rows:
                train_rows.append(j)
                train_nd.append(0)
                train_seeds.append(lc.seed * 7 + lc.training_round)
            order = sorted(range(len(train_rows)), key=lambda k: train_rows[k])
            train_rows = [train_rows[k] for k in order]
            train_nd = [train_nd[k] for k in order]
            train_seeds = [train_seeds[k] for k in order]
        # FedAvg weights of the selected rows (single rank, every row stored): staged with the rest, so the
        # aggregate needs no host -> device copy after the training (== ops.fedavg's s / s.sum(), exact sums)
        sel_nd = np.asarray([prep.meta[r, 2] for r in self._local_rows()], np.float64) if self.world == 1 else None
        fw = sel_nd / sel_nd.sum() if sel_nd is not None and sel_nd.size and sel_nd.sum() > 0 else np.zeros(1)
        # every per-round host value the device needs goes up in ONE asynchronous copy (a pageable
        # torch.tensor(..., device=) per item was a blocking copy each: ~1.5 ms of host time per round)
        plan_seeds = [sd * 1000003 + 17 for sd in train_seeds]
        prep.meta_d, prep.js_d, prep.rows_d, pseed_d, nd_d, prep.tseed_d, fw_d = self._staging.upload([
            prep.meta[:, :META], np.asarray(prep.js, np.int64), np.asarray(train_rows, np.int64),
            np.asarray([(s & 0xFFFFFFFFFFFFFFFF) - (1 << 64) if (s & 0xFFFFFFFFFFFFFFFF) >= (1 << 63)
                        else (s & 0xFFFFFFFFFFFFFFFF) for s in plan_seeds], np.int64),
            np.asarray(train_nd, np.int32),
            np.asarray([self._dev_seed(s) for s in train_seeds], np.int32), fw])
        prep.tq2 = time.perf_counter()
        prep.plan = None
        if train_rows:
            prep.plan = make_plan(self.train_table.n, train_nd, cfg.epoch, plan_seeds, dev,
                                  staged=(pseed_d, nd_d) if dev.type == "cuda" else None)
        prep.train_rows, prep.train_seeds = train_rows, train_seeds
        prep.fedavg_w = fw_d if sel_nd is not None and fw.size == len(self.selected) else None
        prep.sizes_h = torch.from_numpy(sel_nd) if sel_nd is not None else None

    def _enqueue_local(self, prep: Prepared, genuine: Dict[int, Optional[torch.Tensor]]) -> Launch:
        """Device half of a launch: START parameters, the update block, the training launch."""
        cfg, dev = self.cfg, self.device
        tq = time.perf_counter()
        if prep.staged_ev is not None:  # uploads / plan staged on the staging stream (_prepare_staged)
            torch.cuda.current_stream(dev).wait_event(prep.staged_ev)
        for j, i, lc, _ in prep.clients:
            g = genuine.get(i)
            if lc.info.attack is not None and g is not None and g.shape[0] > 0:
                lc.genuine = g
        dec = self._attack_decisions(prep)
        if dec != prep.dec:
            self._stage(prep, dec)  # (an attacker's first attack round)
        attack_jobs = [(j, i, lc, lc.info.attack) for (j, i, lc, _), a in zip(prep.clients, dec) if a]
        train_rows, js, n_local = prep.train_rows, prep.js, len(self.local)
        # the common case (every local client trains) trains local_params in place: no gather / scatter
        in_place = train_rows == list(range(n_local))
        # single rank, every local client in the launch (attackers with zero rows), trained in place: the round
        # reads the update matrix straight from local_params and the meta columns from the host mirror, so
        # no update block is built at all
        plain = (bool(train_rows) and in_place and self.world == 1 and not self.fast_fedavg
                 and self._local_rows() == list(range(n_local)))
        block = None if plain else torch.zeros(self.slots, self.W, dtype=torch.float32, device=dev)
        # START parameters of every started client (one batched generate / broadcast copy)
        if prep.clients:
            start = self.server.start([i for _, i, _, _ in prep.clients])
            if start is not None:
                if js == list(range(len(js))):
                    self.local_params[:len(js)].copy_(start)
                else:
                    self.local_params.index_copy_(0, prep.js_d, start.contiguous())
        if self._speculative and dev.type == "cuda":
            # START is generated (hyper: the memoised generate_many validation reuses): a speculative
            # round's validation stream waits for this point, not for the training launched below
            self._start_ready = torch.cuda.Event()
            self._start_ready.record(torch.cuda.current_stream(dev))
        for j in prep.faults:
            self.local_params[j, 0] = float("nan")
        if block is not None:
            block[:, self.P:self.P + META] = prep.meta_d
        tp0 = time.perf_counter()
        params = pending = ready = None
        if attack_jobs and dev.type == "cuda":
            # the attackers' inputs are ready now; the side stream must not also wait for the training launch
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(dev))
        if train_rows:
            params = self.local_params if in_place else self.local_params.index_select(0, prep.rows_d).contiguous()
            pending = self.trainer.launch(params, prep.plan, cfg.lr, cfg.batch_size, prep.train_seeds,
                                          seeds_dev=prep.tseed_d if self._dev_seed is not _no_dev_seed else None)
        self.ckpt_writer.kick()  # last round's deferred checkpoint copy overlaps this round's training
        return Launch(prep, block, plain, in_place, params, pending, attack_jobs, ready, t_enqueue=tp0 - tq,
                      t_launch=time.perf_counter() - tp0)

    def _finish_attacks(self, launch: Launch) -> None:
        """Attackers' math on a side stream; their results replace their local_params rows (stream-ordered
        after the training launch, which read / wrote back their untouched models: no host wait)."""
        attack_jobs, ready, dev = launch.attack_jobs, launch.ready, self.device
        launch.tw = time.perf_counter()  # a speculative launch (run_round) may have been enqueued long before
        atk_out = []  # (row, ok, malicious update)
        if attack_jobs:
            # the attackers do not train: their math runs on a side stream while the genuine clients'
            # training launch occupies its own CUs (the reference runs every client concurrently too)
            side = self._side_stream()
            if side is not None:
                side.wait_event(ready)
            with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
                for j, i, lc, atk in attack_jobs:
                    res = run_attack(atk.mode, atk.args, self.local_params[j], lc.genuine, self.dist,
                                     seed=lc.seed * 1009 + lc.training_round, gamma=atk.gamma, tau=atk.tau)
                    atk_out.append((j, res.ok and res.params is not None, res.params))
                    self._attack_info = res.info
                    if self.verbose:  # (reads the attack's device scalars back: verbose runs only)
                        hi = host_info(res.info)
                        for g in hi.get("gammas", []):  # the reference's per-iteration print (src/Utils.py:119)
                            print(f"Gamma is {g}")
                        print_with_color(f"[===] Client {i} attacks with {atk.mode} "
                                         f"{ {k: v for k, v in hi.items() if not isinstance(v, list)} }", "red")
            if side is not None:
                torch.cuda.current_stream(dev).wait_stream(side)
        if launch.pending is not None and launch.in_place:
            for j, ok, mal in atk_out:
                if ok:
                    self.local_params[j].copy_(mal)
        launch.atk_out, launch.tp2 = atk_out, time.perf_counter()

    def _finish_local(self, launch: Launch) -> None:
        """Attackers' math (``_finish_attacks``, unless done already), then wait for the training launch, complete
        the host meta mirror and fill the update block (none at world 1 with plain rows)."""
        if launch.atk_out is None:
            self._finish_attacks(launch)
        prep, block, pending, in_place = launch.prep, launch.block, launch.pending, launch.in_place
        hm = prep.meta  # host mirror of the block's meta columns (ok filled in below): no device read needed
        P, E = self.P, self.E
        if pending is not None:
            ok_dev, loss_dev = pending.ok_device(), pending.losses_device()
            # world > 1: the ok flags and losses travel in the block and the host learns every rank's meta from
            # ONE read after the gather, so it does not wait for its own training here (one host round trip less)
            if self.world == 1 or ok_dev is None or loss_dev is None:
                oks, losses = pending.result()
                for k, (j, o) in enumerate(zip(prep.train_rows, oks)):
                    hm[j, 1] = 1.0 if o else 0.0
                    hm[j, META:META + E] = np.asarray(losses[k], dtype=np.float32)[:E]
        tp3 = time.perf_counter()
        if pending is not None and block is not None:
            if in_place:  # the leading rows, as slice copies
                rows, src = slice(0, len(self.local)), self.local_params[:len(self.local)]
            else:  # a subset trained on gathered rows: back into the clients' models first
                rows, src = prep.rows_d, launch.params
                self.local_params.index_copy_(0, rows, src)
            block[rows, :P] = src
            block[rows, P + 1] = ((ok_dev > 0).float() if ok_dev is not None
                                  else torch.tensor([1.0 if o else 0.0 for o in oks], device=self.device))
            block[rows, P + META:P + META + E] = (loss_dev if loss_dev is not None
                                                  else losses.to(self.device)).float()
        # A-15: an attacker still reports its num_data, ok = the attack's result.  Its update is already in its
        # local_params row when it rode along in place (_finish_attacks); otherwise nothing was launched for it
        for j, ok, mal in launch.atk_out:
            hm[j, 1] = 1.0 if ok else 0.0
            if block is not None:
                if ok and not in_place:
                    block[j, :P] = mal
                block[j, P + 1] = 1.0 if ok else 0.0
        if block is not None:
            # every rank stamps its view of the replicated server state into its rows; the gather's reader checks
            # that all ranks agree (_check_decisions), so a rank whose validation / detection diverged fails loudly
            block[:, P + DECISION] = float(self._decision_word())
        launch.lw_times = {"t_lw_prep": (prep.tq2 - prep.tq) + launch.t_enqueue, "t_lw_prep_host": prep.tq1 - prep.tq,
                           "t_lw_prep_upload": prep.tq2 - prep.tq1, "t_lw_launch": launch.t_launch,
                           "t_lw_attack": launch.tp2 - launch.tw, "t_lw_wait": tp3 - launch.tp2,
                           "t_lw_post": time.perf_counter() - tp3}

    def _local_rows(self) -> List[int]:
        """Block rows of the selected clients (cached per selection)."""
        key = tuple(self.selected)
        if self._sel_cache is None or self._sel_cache[0] != key:
            rows = [self.table[i].owner * self.slots + self._slot_of(i) for i in self.selected]
            idx = torch.tensor(rows, device=self.device, dtype=torch.long)
            self._sel_cache = (key, rows, idx)
        return self._sel_cache[1]

    # ------------------------------------------------------------------------------------------
    # SERVER
    # ------------------------------------------------------------------------------------------
    def _rule_args(self) -> dict:
        """The keywords every rule receives (each reads its own): every knob of ``config.RULE_KNOBS`` under its keyword,
        the round's seed (scionfl; dnc keys its column sub-samples with it) and cclip's ``centre`` (the global model the
        round started from: in the early launch the launch's START; None before there is one)."""
        e = self.cfg.engine
        return {**{k.kw: k.check(e.get(k.key, k.default), coerce=True) for k in RULE_KNOBS},
                "seed": self.seed * 13 + self.round_no, "centre": self.global_params}

    def _server_step(self, U: torch.Tensor, sizes: torch.Tensor, attackers: torch.Tensor,
                     ok_all: Optional[torch.Tensor], w: Optional[torch.Tensor] = None, gen_key=None):
        """The server mode's step (``ServerMode.step``) on the update rows ``U``: the single entry of both paths.
        ``ok_all`` None: the host knows that every client succeeded (the serial path, ``_aggregate``).  A 0-d device
        bool, "every client succeeded" as the device knows it (``_early_launch``): nothing is read back, the new
        global model is ``where(ok_all [& the rule's success], new, old)`` and the hypernetwork update gets it as
        ``enable``; FedAvg also takes the clients' int32 success flags themselves and reduces them inside its own
        pass.  ``w``: FedAvg weights already on the device (each caller keeps its own source); ``gen_key``: the clients
        whose next START models the hypernetwork update generates.  Returns (info, the rule's own success: None =
        always, or a 0-d tensor — gmm).  ``engine.pre-agg`` (nnm, bucketing: ``agg.pre_aggregate``) goes in front of a
        rule of AGGREGATORS on either path.  What a failed early round rolls back stays on the mode (``mark``,
        ``undo``), the global model on ``self`` (``_early_launch_failed``)."""
        return self.server.step(U, sizes, attackers, ok_all, w=w, gen_key=gen_key)

    def _aggregate(self, U: torch.Tensor, sizes: torch.Tensor, attackers: torch.Tensor, round_ok: bool,
                   w: Optional[torch.Tensor]) -> dict:
        """The serial path: the host has read the round's meta.  ``w``: the FedAvg weights staged with the launch
        (one rank, every row stored; the several-rank serial path weighs by the host sizes)."""
        if not round_ok:
            return {}
        if w is not None and not (U.is_cuda and U.shape[0] == w.shape[0]):
            w = None
        return self._server_step(U, sizes, attackers, None, w=w)[0]

    # ------------------------------------------------------------------------------------------
    # one round
    # ------------------------------------------------------------------------------------------
    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def run_round(self, last: bool = False) -> dict:
        """One FL round.  ``last``: the caller will not run another round, so no speculative launch."""
        if not self._selection_done:
            self.client_selection()
        t0 = time.perf_counter()
        if self.verbose:
            print_with_color(f"Start training round {self.round_no}", "yellow")
        self._attack_info = None
        self.server.begin_round()
        with trace.range("fl/local"):
            launch, self._spec = self._spec, None
            if launch is None:
                launch = self._launch_local(self._genuine_for_attackers())
            if self._speculative and self.rounds_left > 1 and not last and self._next_prep is None:
                # the next launch's host half (draws, uploads, plan) while this round's training runs: after
                # it, only the aggregate, START and the launch itself separate two training kernels
                self._next_prep = self._prepare_staged()
            esl = self._early_launch(launch, last)
            self._finish_local(launch)
            if self.phase_sync:  # stream-ordered otherwise: the timing-only sync is skipped
                self._sync()
        t1 = time.perf_counter()
        U = snapshot = None
        stored = len(self.selected)
        if esl is not None:
            # one rank: the aggregate and the next launch went in before the wait (_early_launch)
            meta = torch.from_numpy(launch.prep.meta[self._local_rows()])
            round_ok, info = self._early_outcome(esl, meta.numpy()[:, 1] > 0.5)
            t2 = t3 = time.perf_counter()
        elif self.fast_fedavg:
            round_ok, meta = self._fedavg_allreduce(launch.block, launch.prep.meta)
            info = {"path": "fedavg-allreduce"}
            t2 = t3 = time.perf_counter()
        else:
            U, meta, esl = self._gather(launch, last)
            t2 = time.perf_counter()
            mn = meta.numpy()  # (numpy: a handful of tiny host ops, cheaper than torch CPU tensors)
            results = mn[:, 1] > 0.5
            sizes = torch.from_numpy(mn[:, 2].copy())
            attackers = torch.from_numpy(mn[:, 3] > 0.5)
            round_ok = bool(results.all())
            # stored updates (arrival in client order; the reference stops storing after a failure)
            if not round_ok:
                stored = int(np.nonzero(~results)[0][0])
            snapshot = self.hyper.snapshot() if self.detector is not None else None  # (detection may roll back)
            if esl is not None:  # (several ranks: the aggregate and the next launch are in already)
                round_ok, info = self._early_outcome(esl, results)
            else:
                with trace.range("fl/aggregate"):
                    info = self._aggregate(U, sizes, attackers, round_ok, launch.prep.fedavg_w)
                    if self.phase_sync:  # per-phase timings only; otherwise validation queues behind it
                        self._sync()
            if info.get("agg_failed"):
                round_ok = False
            t3 = time.perf_counter()
        # ---- genuine pool for the next START (non-attacker rows stored this round; only attackers read it) ----
        if self._has_attackers and U is not None and esl is None:
            keep = self._store_genuine(U, stored)
            if (keep and keep[0] == 0 and round_ok and self.server.aliases_first_stored
                    and self.global_params is not None):
                # A-13: the reference averages INTO the first stored update's dict, which is also the first
                # genuine model in the pool (server.py:263-268,763): attackers may receive the aggregate
                self.genuine_pool[0] = self.global_params
        # Speculative next launch: the next round's local training is enqueued right behind the aggregate,
        # BEFORE this round's validation / checkpoint, which then run on a side stream next to it (the
        # trainer occupies a few CUs).  Valid whatever validation decides: a failed round is retried from the
        # same global model with the same client counters, i.e. exactly this launch.  Every rank decides
        # the same (replicated validation), so the ranks' launches and gathers stay in lockstep.
        vstream = agg_done = None
        if esl is not None and self._spec is not None:
            agg_done = esl.agg_done
        elif self._speculative and round_ok and self.rounds_left > 1 and not last:
            # (no global model, as in hyper mode: nothing; test() falls back to the ordinary path if it changes later)
            self._prefetch_validation(self.global_params)
            agg_done = torch.cuda.Event()
            agg_done.record(torch.cuda.current_stream(self.device))
            self._spec = self._launch_local(self._genuine_for_attackers())
        if agg_done is not None:
            if self._val_stream is None:
                self._val_stream = torch.cuda.Stream(device=self.device)
            vstream = self._val_stream
            vstream.wait_event(agg_done)
            vstream.wait_event(self._start_ready)
        with (torch.cuda.stream(vstream) if vstream is not None else contextlib.nullcontext()):
            rec = self._finish_round(snapshot, info, round_ok, launch.lw_times, meta, t0, t1, t2, t3)
        if vstream is not None:
            self.ckpt_writer.kick()  # the next launch is already in: copy + write while it trains
        return rec

    def _gather(self, launch: Launch, last: bool):
        """The general path's exchange: (update rows ``U`` of the selected clients, their host meta, the early
        launch enqueued on the gathered rows or None)."""
        trace.push("fl/gather")
        P, block = self.P, launch.block
        rows = self._local_rows()
        idx = self._sel_cache[2]
        esl = None
        if self.world == 1:  # every row is local: the host already knows the meta columns
            meta = torch.from_numpy(launch.prep.meta[rows])
            if launch.plain:
                U = self.local_params[:len(rows)]  # the trained models ARE the update rows: no block at all
            else:
                U = self.comm.all_gather_rows(block).index_select(0, idx)[:, :P].contiguous()
        else:
            allb = self.comm.all_gather_rows(block)                    # [world*slots, W]
            sel = allb.index_select(0, idx)
            U = sel[:, :P].contiguous()
            # the round's ONE host read: every client's [valid, result, size, attacker, decision | losses]; it
            # is queued BEFORE the early launch and waited for through its own event, so the host waits for
            # the gather (the slowest rank's clients), not for the next round's training queued behind it
            # (+ one row per rank — its first slot — so every rank's decision word is checked, also a rank
            # none of whose clients is selected or valid this round)
            nsel = sel.shape[0]
            per_rank = allb[0::block.shape[0], P:P + META + self.E] if block.shape[0] else allb[:0, P:P + META + self.E]
            mread = self._meta_read(torch.cat([sel[:, P:P + META + self.E], per_rank], 0))
            # FedAvg / hyper: the aggregate and the next launch go in on the device before the host read
            esl = self._early_launch(launch, last, U=U, sel=sel)
            mall = mread()
            meta, rank_rows = mall[:nsel], mall[nsel:]
            self.comm.check()
            self._check_decisions(meta.numpy(), rank_rows.numpy()[:, DECISION])
            if launch.pending is not None:
                launch.pending.result()  # the training has finished by now: surfaces hand-off timeouts
        if self.phase_sync:
            self._sync()
        trace.pop()
        return U, meta, esl

    def _meta_read(self, cols: torch.Tensor):
        """Start the device -> host copy of the gathered meta columns; returns a callable that waits for THAT
        copy only (an event recorded right after it) and yields the fp64 host matrix."""
        if cols.device.type != "cuda":
            m = cols.double().cpu()
            return lambda: m
        buf = self._meta_pinned
        if buf is None or buf.shape != cols.shape:
            buf = self._meta_pinned = torch.empty(cols.shape, dtype=torch.float32, pin_memory=True)
        buf.copy_(cols, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))

        def wait():
            ev.synchronize()
            return buf.double()  # (a copy: the pinned buffer is reused next round)
        return wait

    def _decision_word(self) -> int:
        """23-bit digest (exact in fp32) of the replicated server state every rank must agree on: the round
        counters (which encode every past round_ok) and the selected set (which encodes every removal)."""
        key = f"{self.round_no}|{self.rounds_left}|{','.join(map(str, self.selected))}".encode()
        return zlib.crc32(key) & 0x7FFFFF

    def _check_decisions(self, mn: np.ndarray, rank_words: np.ndarray = None) -> None:
        """Raise if the ranks' decision words differ: a rank's validation or detection decided otherwise (e.g.
        a mixed CPU / GPU gloo world whose kernels are not bit-identical), and continuing would desynchronise
        the collectives or silently diverge the replicated models.  ``rank_words``: one word per rank (its
        first slot row), so a rank without a selected, valid client is checked too (as the all-reduce path)."""
        valid = mn[:, 0] > 0.5
        words = mn[valid, DECISION]
        if rank_words is not None:
            words = np.concatenate([words, np.asarray(rank_words, dtype=words.dtype)])
        if words.size and not np.all(words == words[0]):
            raise RuntimeError(f"ranks disagree on the replicated server state (round {self.round_no}): decision "
                               f"words {sorted(set(int(w) for w in words))}; validation / detection must be "
                               "bit-identical on every rank (do not mix devices in one world)")

    def _fills_gpu(self) -> bool:
        """The training launch occupies every CU (the on-chip CNN trainer: 32 workgroups per client), so nothing
        queued beside it on another stream starts before it ends."""
        if self.device.type != "cuda" or getattr(self.trainer, "kind", "") != "graph" or self.model_name != "CNNModel":
            return False
        return len(self.local) * int(ops.native().cnn2_wgs_per_client()) >= onchip.cu_share(self.device)

    def _prefetch_validation(self, g: Optional[torch.Tensor]) -> None:
        """Ahead of a speculative launch that fills the GPU: this round's validation forward + AUC go in FIRST
        (stream order), so the host has its metric while the next training runs (Validation.prefetch)."""
        if g is not None and self.validation is not None and self._fills_gpu():
            self.validation.prefetch(g)

    def _early_ok(self, last: bool) -> bool:
        """Whether this round launches early (``_early_launch``).  The mode's half is ``ServerMode.early_ok``: FedAvg,
        the hypernetwork's native update, FLTrust, foolsgold (the device decides whether its history advances) and
        every rule of AGGREGATORS — all device work without a host read (gmm up to 64 rows)."""
        return self._speculative and self.rounds_left > 1 and not last and self.server.early_ok()

    def _store_genuine(self, U: torch.Tensor, stored: int) -> List[int]:
        """The genuine pool of the next START: the non-attacker rows among the first ``stored`` of ``U`` (a new
        tensor, taken before the next START overwrites the rows).  Returns their row numbers."""
        keep = [k for k, i in enumerate(self.selected[:stored]) if self.table[i].attack is None]
        self.genuine_pool = self._take_rows(U, keep) if keep else None
        return keep

    def _early_launch(self, launch: Launch, last: bool, U: Optional[torch.Tensor] = None,
                      sel: Optional[torch.Tensor] = None) -> Optional["EarlyLaunch"]:
        """This round's server step and the NEXT round's launch, enqueued before the host waits for this round's
        training (one rank, plain rows) or reads the gathered meta (several ranks), so no host work separates two
        training kernels.  The step keeps the old global model on the device when a client failed (the host
        learns that after the wait), which makes the launch exactly this round's retry (same START, the next client
        draws); with attackers a failure discards it and restores the host state it consumed, because their
        genuine sample then comes from the stored prefix.  Returns None where the ordinary path runs."""
        if not self._early_ok(last):
            return None
        if sel is None:  # one rank, plain rows: before the host waits for the training
            prep = launch.prep
            if not (self.world == 1 and launch.plain and prep.fedavg_w is not None):
                return None
            self._finish_attacks(launch)
            if not all(ok for _, ok, _ in launch.atk_out):
                return None
            n = len(self.selected)
            U = self.local_params[:n]
            ok_all = launch.pending.ok_device()[:n]
            if not (self.server.takes_ok_flags and ok_all.dtype == torch.int32):  # (FedAvg: reduced in the aggregate)
                ok_all = (ok_all > 0).all()
            w, sizes = prep.fedavg_w, prep.sizes_h
            attackers = torch.from_numpy(prep.meta[self._local_rows(), 3] > 0.5)
        else:  # several ranks: called on the gathered rows (device), before the host reads their meta
            P = self.P
            ok_all = ((sel[:, P] > 0.5) & (sel[:, P + 1] > 0.5)).all()
            sizes = sel[:, P + 2].double()
            w = sizes / sizes.sum()
            attackers = sel[:, P + 3] > 0.5
        # (the snapshot already includes the staged host half's draws; its clients' START models come out of the
        # hypernetwork update's last launches)
        esl = EarlyLaunch(g_old=self.global_params, mode_mark=self.server.mark(),
                          snap=([(lc.rng.getstate(), lc.training_round, lc.genuine) for lc in self.local],
                                self.server_rng.getstate()),
                          prep=self._next_prep)
        gen_key = [i for _, i, _, _ in esl.prep.clients] if esl.prep is not None and esl.prep.clients else None
        esl.info, rule_ok = self._server_step(U, sizes, attackers, ok_all, w=w, gen_key=gen_key)
        if rule_ok is not None:
            # gmm's success (some row kept): the host reads it after its wait from a pinned copy queued BEFORE the
            # next launch, so it waits for the filter and not for the training behind it (_early_outcome)
            okh = torch.empty(1, dtype=torch.bool, pin_memory=True)
            okh.copy_(rule_ok.reshape(1), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            esl.rule_ok = (okh, ev)
        if self._has_attackers:  # the pool of a fully stored round
            esl.keep = self._store_genuine(U, len(self.selected))
            esl.pool = self.genuine_pool
        self._prefetch_validation(self.global_params)  # (no global model, as in hyper mode: nothing)
        esl.agg_done = torch.cuda.Event()
        esl.agg_done.record(torch.cuda.current_stream(self.device))
        self._spec = self._launch_local(self._genuine_for_attackers())
        return esl

    def _early_outcome(self, esl: "EarlyLaunch", results: np.ndarray):
        """After the host's wait: (round ok, info) of a round whose server step went in early; a failed one is
        undone (``_early_launch_failed``)."""
        round_ok = bool(results.all())
        info = {**esl.info, "path": "early-launch"} if round_ok else {}
        if round_ok and esl.rule_ok is not None:
            okh, ev = esl.rule_ok
            ev.synchronize()
            if not bool(okh[0]):
                round_ok, info = False, {**esl.info, "agg_failed": True}
        if not round_ok:
            self._early_launch_failed(esl, results)
        return round_ok, info

    def _early_launch_failed(self, esl: "EarlyLaunch", results: np.ndarray) -> None:
        self.global_params = esl.g_old  # (the device selected the same values: the launch's START)
        self.server.undo(esl.mode_mark)
        if esl.keep is None:
            return  # no attackers: the launch in flight is this round's retry
        # attackers sample the stored prefix's genuine rows: discard the launch, restore what it consumed
        # (every row is stored when only the aggregate failed: gmm kept no row)
        stored = int(np.nonzero(~results)[0][0]) if not results.all() else len(results)
        m = sum(k < stored for k in esl.keep)  # (keep ascends: the pool's first m rows)
        states, srng = esl.snap
        for lc, (rs, tr, gen) in zip(self.local, states):
            lc.rng.setstate(rs)
            lc.training_round = tr
            lc.genuine = gen
        self.server_rng.setstate(srng)
        self._spec = None
        self._next_prep = esl.prep  # the launch's host half is reused as it was (same draws)
        self.genuine_pool = esl.pool[:m] if m else None

    def _client_losses(self, meta: Optional[torch.Tensor]) -> Optional[List[Optional[List[float]]]]:
        """Per-epoch training loss of every selected client (None for attackers and failed clients), from
        the round's meta rows (host mirror on one rank, the gathered block's loss columns otherwise)."""
        if meta is None or meta.shape[1] < META + self.E:
            return None
        return [None if (meta[r, 3] > 0.5 or meta[r, 1] < 0.5)
                else [round(float(x), 6) for x in meta[r, META:META + self.E]] for r in range(len(self.selected))]

    def _finish_round(self, snapshot, info, round_ok, lw_times: Dict[str, float], meta: Optional[torch.Tensor],
                      t0, t1, t2, t3) -> dict:
        trace.push("fl/validate")
        # ---- replicated detection + validation: every rank computes the same decision ----
        removed: List[int] = []
        metric = float("nan")
        # the reference validates len(all_model_parameters) generated models: the clients that reported this
        # round, counted before any removal (server.py:541)
        n_val = len(self.selected)
        if self.detector is not None:
            embs = {i: self.hyper.embedding(i).cpu().numpy()[None, :] for i in self.selected}
            removed = self.detector.step(self.round_no, self.selected, embs)
        if removed:
            # removal and rollback come BEFORE validation, so the logged metric and the round's success are
            # those of the rolled-back hypernetwork (server.py:532-543)
            for r in removed:
                if self.verbose:
                    print_with_color(f"Removing anomaly {r}, rolling back", "yellow")
                if r in self.selected:
                    self.selected.remove(r)
            self.hyper.restore(snapshot)
        if self.validation is not None and round_ok:
            round_ok, metric = self.server.validate(n_val)
        trace.pop()
        t4 = time.perf_counter()
        if round_ok:
            with trace.range("fl/checkpoint"):
                self.save_checkpoint()
                self.rounds_left -= 1
                if self.cfg.engine.get("save-state", False):
                    self.round_no += 1
                    self.save_state()
                    self.round_no -= 1
        elif self.verbose:
            print_with_color("Training failed!", "yellow")
        t5 = time.perf_counter()
        rec = {"round": self.round_no, "ok": round_ok, "metric": metric, **lw_times,
               "t_local": t1 - t0, "t_gather": t2 - t1,
               "t_aggregate": t3 - t2, "t_validate": t4 - t3, "t_checkpoint": t5 - t4, "t_round": t5 - t0,
               "n_selected": len(self.selected), "removed": removed}
        if self._attack_info:
            # every tried γ and its accept decision, not just the last one (the reference prints each γ)
            rec["attack"] = {k: v for k, v in host_info(self._attack_info).items() if isinstance(v, (int, float, list))}
        # (device-resident outputs of the mode and the aggregator: read now, after validation)
        info = agg_host_info(self.server.end_round(info))
        rec.update({k: v for k, v in info.items() if isinstance(v, (int, float, list, str)) or k == "pre_agg"})
        losses = self._client_losses(meta)
        if losses is not None:
            rec["client_loss"] = losses
            if self.verbose:
                self._print_losses(losses, meta)
        self.metrics.write(rec)
        self.history.append(rec)
        if round_ok:
            self.round_no += 1
        return rec

    def _print_losses(self, losses, meta: torch.Tensor) -> None:
        """Reference client prints (``client.py:109`` ICU: ``Loss {mean}`` per epoch; ``client.py:130`` HAR:
        ``Epoch {e}, Loss: {sum:.4f}``), one block per client, from the server's view of the round."""
        for i, ls in zip(self.selected, losses):
            if ls is None:
                continue
            if self.data_name == "HAR":
                nb = max(1, -(-int(meta[self.selected.index(i), 2]) // self.cfg.batch_size))
                for e, l in enumerate(ls):
                    print(f"[client {i}] Epoch {e + 1}, Loss: {l * nb:.4f}")
            else:
                for l in ls:
                    print_with_color(f"[client {i}] Loss {l} ", "yellow")

    def _fedavg_allreduce(self, block: torch.Tensor, meta_host: np.ndarray):
        """FedAvg over one all_reduce: [sum s_i w_i | sum s_i | #failed | #reported] (fp64).  Returns
        (round ok, host meta of the selected rows — one rank only); sets ``global_params`` on success."""
        P = self.P
        present = block[:, P] > 0.5
        size = torch.where(present, block[:, P + 2], torch.zeros_like(block[:, P + 2])).double()
        red = torch.zeros(P + 5, dtype=torch.float64, device=block.device)
        red[:P] = (size[:, None] * block[:, :P].double()).sum(0)
        red[P] = size.sum()
        red[P + 1] = (present & (block[:, P + 1] < 0.5)).double().sum()
        red[P + 2] = present.double().sum()
        # decision words: all equal iff n * sum(w^2) == (sum w)^2 (exact in fp64 for 23-bit words)
        word = float(self._decision_word())
        red[P + 3] = word
        red[P + 4] = word * word
        with trace.range("fl/allreduce"):
            if self.world > 1:
                self.comm.all_reduce_(red)
            if self.phase_sync:
                self._sync()
        fl = red[P + 1:P + 5].cpu()  # one device -> host read for the counters (waits for the reduce)
        if float(fl[2]) ** 2 != self.world * float(fl[3]):
            raise RuntimeError(f"ranks disagree on the replicated server state (round {self.round_no}); "
                               "validation / detection must be bit-identical on every rank")
        round_ok = int(fl[0]) == 0 and int(fl[1]) == len(self.selected)
        if round_ok:
            self.global_params = (red[:P] / red[P]).to(torch.float32)
        # per-client meta (losses for the JSONL): only a single rank knows every row without another read
        meta = torch.from_numpy(meta_host[self._local_rows()]) if self.world == 1 else None
        return round_ok, meta

    def _slot_of(self, i: int) -> int:
        owner = self.table[i].owner
        return sum(1 for c in self.table[:i] if c.owner == owner)

    def run(self, max_rounds: Optional[int] = None) -> List[dict]:
        if not self.selected:
            self.client_selection()
        fails = 0
        done = 0
        while self.rounds_left > 0:
            # the caller's last round launches nothing speculatively (no un-aggregated extra training)
            rec = self.run_round(last=max_rounds is not None and done + 1 >= max_rounds)
            done += 1
            fails = 0 if rec["ok"] else fails + 1
            if self.max_retries and fails > self.max_retries:
                raise RuntimeError(f"round {self.round_no} failed {fails} times in a row")
            if max_rounds is not None and done >= max_rounds:
                break
        if self.verbose and self.rounds_left <= 0:
            print_with_color("Training finished, stopping clients.", "green")
        self.ckpt_writer.flush()
        return self.history

    def close(self):
        if self._closed:
            return
        self._closed = True
        if self._spec is not None:
            # a speculative launch nobody consumed (bench.py drives run_round itself): wait for the GPU work,
            # skip the block / meta bookkeeping.  Client state (local_params, training_round, client RNGs) is
            # then one round ahead of history / round_no.
            launch, self._spec = self._spec, None
            if launch.pending is not None:
                launch.pending.result()
            self._sync()
        self.ckpt_writer.close()
        self.metrics.close()
        if hasattr(self.logger, "close"):
            self.logger.close()
