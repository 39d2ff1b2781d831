"""The server's mode as one object: what ``server.mode`` means to a round, and the state a mode carries, live here and
nowhere in ``engine.py``.  ``FLEngine.server`` is one ``ServerMode``; the engine calls the members below at fixed points
of a round and never asks which mode it runs (``fast_fedavg``, a communication decision, is its one exception).

A mode keeps on ``self`` whatever a failed early round must roll back (``FLEngine._early_launch``): ``mark()`` is taken
before the step, and ``undo(mark)`` gets that very object if the host then learns that the round failed.  The global
model is the engine's: ``step`` assigns ``eng.global_params``, the engine restores it.
"""
from __future__ import annotations

import os
from typing import List, Optional

import torch

from .. import ops
from ..agg import AGGREGATORS, AggResult, pre_aggregate
from ..agg import foolsgold as agg_foolsgold
from ..config import FLAME_NOISE, FOOLSGOLD_KAPPA, SIGNGUARD_KNOBS
from ..data import DeviceTable, resolve_dataset
from ..detect import HyperDetector
from ..models import build_model
from ..utils.log import print_with_color
from .hyper_server import HyperServer
from .trainers import Plan, make_trainer


class ServerMode:
    needs_train_table = False    # the engine loads the train set even on a rank without clients
    takes_ok_flags = False       # one rank's early step gets the clients' int32 success flags, not their reduction
    aliases_first_stored = False  # A-13: the aggregate is also the genuine pool's first model

    def __init__(self, eng):
        self.eng = eng

    def early_ok(self) -> bool:
        """The step is device work without a host read and retries from ``eng.global_params``: it may go in before
        the host knows the round's outcome."""
        eng = self.eng
        return (not eng.fast_fedavg and eng.global_params is not None
                and not eng.cfg.engine.get("compat-fedavg-alias", False))

    def step(self, U: torch.Tensor, sizes: torch.Tensor, attackers: torch.Tensor, ok_all: Optional[torch.Tensor],
             w: Optional[torch.Tensor] = None, gen_key=None):
        """The contract of ``FLEngine._server_step``."""
        raise NotImplementedError

    def mark(self):
        """Before an early step: whatever ``undo`` needs to take the step back on ``self`` (the default: nothing)."""

    def undo(self, mark) -> None:
        """The early round failed on the device, which kept its old values: the host side of ``self`` goes back too."""

    def begin_round(self) -> None:
        """A round (or its retry) begins."""

    def end_round(self, info: dict) -> dict:
        """At the round's end, where the host has synchronised: ``info`` completed with what the mode reports."""
        return info

    def state(self) -> dict:
        """The mode's keys of the server's state file (``FLEngine.save_state``)."""
        return {}

    def load(self, srv: dict) -> None:
        """Take the mode's keys out of a loaded state file, where it has them."""

    def start(self, ids: List[int]) -> Optional[torch.Tensor]:
        """START models of the clients ``ids`` as rows (None: they keep their own models)."""
        p = self.eng._start_params()
        return None if p is None else p[None, :].expand(len(ids), -1)

    def checkpoint(self) -> None:
        """The leader's ``{model}.pth``."""
        eng = self.eng
        if eng.global_params is not None:
            layout = eng.layout
            # deferred: an immediate copy let the writer thread's torch.save (GIL-bound, ~0.5 ms) run
            # in the gap between two rounds' training launches and stall the next round's preparation;
            # kicked after the next launch it runs while the GPU trains.  global_params is replaced, never
            # updated in place, so the submitted tensor stays valid until the copy.
            eng.ckpt_writer.submit("global", eng.global_params, lambda f: layout.unflatten(f, clone=False),
                                   eng._pth(False), defer=True)

    def validate(self, n_val: int):
        """-> (round ok, metric) of the server-side validation (the engine has one)."""
        g = self.eng.global_params
        return (False, float("nan")) if g is None else self.eng.validation.test(g)


class RuleMode(ServerMode):
    """Every stateless rule of ``AGGREGATORS``, FedAvg included."""

    def __init__(self, eng):
        super().__init__(eng)
        self.name = eng.mode
        self.takes_ok_flags = self.name == "fedavg"  # (FedAvg reduces them inside its own pass)
        self.aliases_first_stored = self.name == "fedavg" and bool(eng.cfg.engine.get("compat-fedavg-alias", False))

    def early_ok(self) -> bool:
        # (gmm runs on the device without a host read up to 64 rows; its success is a device bool)
        return super().early_ok() and not (self.name == "gmm" and len(self.eng.selected) > 64)

    def _args(self) -> dict:
        """The keywords the rule is called with."""
        return self.eng._rule_args()

    def step(self, U, sizes, attackers, ok_all, w=None, gen_key=None):
        eng = self.eng
        g_old = eng.global_params
        if self.name == "fedavg" and w is not None:
            # the weights were staged with the launch (sizes known then): no host -> device copy here
            if ok_all is None:
                eng.global_params = ops.weighted_rows(U, w)
            elif ok_all.dim():
                eng.global_params = ops.weighted_rows(U, w, ok_all, g_old)  # (the success check fused into the pass)
            else:
                eng.global_params = torch.where(ok_all, ops.weighted_rows(U, w), g_old)
            return {"n": int(U.shape[0])}, None
        args, pre = self._args(), None
        if eng.cfg.engine.get("pre-agg", "none") != "none":
            # (device work without a host read, like the rules: the rule then sees the mixed rows and their sizes)
            U, sizes, pre = pre_aggregate(eng.cfg.engine["pre-agg"], U, sizes, byz_f=args["byz_f"], seed=args["seed"],
                                          bucket_size=eng.cfg.engine.get("bucket-size", 2))
        res: AggResult = AGGREGATORS[self.name](U, sizes, attackers=attackers, **args)
        info = {k: v for k, v in res.info.items() if k != "scores"}
        if pre is not None:
            info["pre_agg"] = pre
        if ok_all is None:
            if not bool(res.ok):  # (gmm on the device: a 0-d tensor, the serial path's one synchronising read)
                info["agg_failed"] = True
            elif res.params is not None:
                g = res.params.to(torch.float32)
                if g.untyped_storage().data_ptr() == U.untyped_storage().data_ptr():
                    g = g.clone()  # a selected row (e.g. Krum) of U, which may be the live client models
                eng.global_params = g
            return info, None
        rule_ok = None if res.ok is True else torch.as_tensor(res.ok, device=U.device)
        if res.params is not None:  # (a new tensor: never a row of U)
            eng.global_params = torch.where(ok_all if rule_ok is None else ok_all & rule_ok,
                                            res.params.to(torch.float32), g_old)
        return info, rule_ok


class SignGuardMode(RuleMode):
    """SignGuard: a stateless rule of ``AGGREGATORS`` whose three knobs are its own, not keywords of every rule."""

    def early_ok(self) -> bool:
        # (beyond the kernel's 64 rows the rule is its host mirror, which reads the statistics back)
        return super().early_ok() and len(self.eng.selected) <= 64

    def _args(self) -> dict:
        e = self.eng.cfg.engine
        return {**super()._args(), **{k.kw: k.check(e.get(k.key, k.default), coerce=True) for k in SIGNGUARD_KNOBS}}


class FlameMode(RuleMode):
    """FLAME: a stateless rule of ``AGGREGATORS`` with a knob of its own (the noise level)."""

    def early_ok(self) -> bool:
        # (beyond the kernel's 64 rows the rule is its host mirror, which reads the Gram back)
        return super().early_ok() and len(self.eng.selected) <= 64

    def _args(self) -> dict:
        e = self.eng.cfg.engine
        return {**super()._args(), FLAME_NOISE.kw: FLAME_NOISE.check(e.get(FLAME_NOISE.key, FLAME_NOISE.default),
                                                                     coerce=True)}


class FLTrustMode(ServerMode):
    """FLTrust: the server model, the round's trust scores, the server model's training in flight and the root set."""
    needs_train_table = True

    def __init__(self, eng):
        super().__init__(eng)
        m = build_model(eng.model_name, seed=eng.seed + 77)
        self.model: torch.Tensor = eng.layout.flatten(m.state_dict(), device=eng.device)
        self.trust: Optional[torch.Tensor] = None  # of the round in progress
        self._pending = None  # the server model's training, checked at the round's end
        self._root = None  # created on first use

    def step(self, U, sizes, attackers, ok_all, w=None, gen_key=None):
        eng = self.eng
        g_old = eng.global_params
        new = self.fltrust(U)
        eng.global_params = new if ok_all is None else torch.where(ok_all, new, g_old)
        return {}, None

    def mark(self):
        return self.model

    def undo(self, mark) -> None:
        """No server-model step and no trust scores for a failed round.  Its training ran all the same, right behind
        the clients' training the host has waited for: a hand-off timeout in it raises here, on the failed path only."""
        self._check_pending()
        self.model, self.trust = mark, None

    def begin_round(self) -> None:
        self.trust = None

    def end_round(self, info: dict) -> dict:
        self._check_pending()  # (the root training: finished by now; raises on a hand-off timeout)
        if self.trust is not None:
            info["trust"] = [round(float(x), 6) for x in self.trust.tolist()]
        return info

    def _check_pending(self) -> None:
        pending, self._pending = self._pending, None
        if pending is not None:
            pending.result()

    def _setup(self):
        """Root set (first 200 test rows, ``server.py:290-293``), its device table and the server model's
        trainer: built once and reused every round."""
        if self._root is None:
            from ..data import ICUData

            eng = self.eng
            root = resolve_dataset(eng.data_name, "test", eng.cfg.data, verbose=False)
            if isinstance(root, ICUData):
                root = ICUData(vitals=root.vitals[:200], labs=root.labs[:200], labels=root.labels[:200])
            table = DeviceTable(root, eng.device)
            trainer = make_trainer(eng.cfg.engine.get("trainer", "auto"), eng.model_name, eng.data_name, table,
                                   eng.device)
            nd = min(200, table.n)
            # DataLoader(batch_size=100, shuffle=False): the same in-order visit every epoch
            order = torch.arange(nd, dtype=torch.int32, device=eng.device)[None, None, :].expand(
                1, eng.cfg.epoch, nd).contiguous()
            plan = Plan(order, torch.tensor([nd], dtype=torch.int32), eng.cfg.epoch,
                        nd_dev=torch.tensor([nd], dtype=torch.int32, device=eng.device))
            self._root = (table, trainer, plan)
        return self._root

    def fltrust(self, U: torch.Tensor) -> torch.Tensor:
        """FLTrust with a server model trained on the first 200 test rows (``server.py:682-743``).
        Everything stays on the device: the server model's training is enqueued (its result is ignored,
        like the reference's ``train_on_device`` return value), and the trust scores, norms and the
        trust-weighted sum are device tensors; ``trust`` reaches the JSONL lazily after validation."""
        eng = self.eng
        compat = bool(eng.cfg.engine.get("compat-fltrust", False))
        g0 = eng.global_params if eng.global_params is not None else self.model.clone()
        _, trainer, plan = self._setup()
        params = g0.clone()[None]
        # kept and read at the round's host synchronisation (end_round): a NaN result is ignored like the
        # reference's train_on_device return value, a cross-workgroup timeout still raises
        seed = eng.seed + eng.round_no
        ds = getattr(trainer, "device_seed", None)
        seeds_dev = None
        if ds is not None and eng.device.type == "cuda":
            # a pinned, non-blocking upload: the trainer's own upload of a host list is a pageable copy, which
            # waits for the clients' training (the early launch enqueues this before that ends)
            from ..ops.layers import upload
            seeds_dev = upload(torch.tensor([ds(seed)], dtype=torch.int32), eng.device)
        self._pending = trainer.launch(params, plan, eng.cfg.lr, 100, [seed], seeds_dev=seeds_dev)
        server_new = params[0]
        g0_delta = server_new - g0
        if compat and eng.global_params is None:
            g0_delta = torch.zeros_like(g0)  # round-1 alias: state_dict() views were trained in place
        deltas = U - g0[None, :]
        if compat:
            deltas = deltas - g0[None, :]   # A-10: the stored delta is reduced by g_0 a second time
        norm_g0 = torch.linalg.vector_norm(g0_delta.double())
        norms = ops.row_norms(deltas).double()
        cos = ops.cosine_to(deltas, g0_delta, eps=1e-8).double()
        trust = torch.clamp(cos, min=0.0)
        scale = (norm_g0 / (norms + 1e-6)) * trust
        w = scale / (trust.sum() + 1e-6)
        agg = ops.weighted_rows(deltas, w)
        self.model = server_new
        self.trust = trust
        return g0 + agg


class FoolsGoldMode(ServerMode):
    """FoolsGold (replicated, every rank its own identical copy): the clients' update histories [n_clients, P] in two
    ping-pong buffers (a step reads one and writes the other, so undoing it is switching back), which one is in use,
    and ``rounds``, the successful rounds accumulated (a 0-d int64 tensor: the device counts in the early launch)."""

    def __init__(self, eng):
        super().__init__(eng)
        self._bufs = [torch.zeros(eng.n_clients, eng.P, dtype=torch.float32, device=eng.device) for _ in range(2)]
        self._cur = 0
        self.rounds = torch.zeros((), dtype=torch.int64, device=eng.device)
        self._ids = None  # (selection, its client ids on the device)

    @property
    def history(self) -> torch.Tensor:
        """The clients' update histories [n_clients, P], row = client id."""
        return self._bufs[self._cur]

    def step(self, U, sizes, attackers, ok_all, w=None, gen_key=None):
        eng = self.eng
        g_old = eng.global_params
        new, info = self.foolsgold(U, sizes, ok_all)
        eng.global_params = new if ok_all is None else torch.where(ok_all, new, g_old)
        return info, None

    def mark(self):
        return self._cur, self.rounds

    def undo(self, mark) -> None:
        self._cur, self.rounds = mark  # the device kept the old history's bits: back to the buffer that holds them

    def state(self) -> dict:
        return {"fg_history": self.history.detach().cpu(), "fg_rounds": int(self.rounds)}

    def load(self, srv: dict) -> None:
        if "fg_history" in srv:
            dev = self.eng.device
            self.history.copy_(srv["fg_history"].to(dev))
            self.rounds = torch.as_tensor(int(srv["fg_rounds"]), dtype=torch.int64).to(dev)

    def foolsgold(self, U: torch.Tensor, sizes: torch.Tensor, ok_all: Optional[torch.Tensor]):
        """FoolsGold (``agg.foolsgold``) on the selected clients' rows about the model the round started from, with the
        mode's history: read from the buffer in use, written to the other one, which then becomes the one in use.
        ``ok_all`` goes in as ``enable``, so a round that failed on the device leaves the history's bits (and the count
        of rounds) as they were.  A selection that is a strict subset of the clients is gathered from and scattered to
        its rows of the history by client id, the other rows copied.  Before there is a global model (round 1) the
        result is FedAvg and nothing is accumulated.  -> (the new global model, info)."""
        eng = self.eng
        H, nxt = self._bufs[self._cur], self._bufs[1 - self._cur]
        kappa = eng.cfg.engine.get(FOOLSGOLD_KAPPA.key, FOOLSGOLD_KAPPA.default)
        enable = None if ok_all is None else ok_all.all().to(torch.int32).reshape(1)
        full = list(eng.selected) == list(range(eng.n_clients))
        ids = None
        if not full:
            key = tuple(eng.selected)
            if self._ids is None or self._ids[0] != key:
                ix = torch.tensor(eng.selected, dtype=torch.long)
                if eng.device.type == "cuda":  # (pinned and non-blocking: no wait for the stream)
                    from ..ops.layers import upload
                    ix = upload(ix, eng.device)
                self._ids = (key, ix)
            ids = self._ids[1]
        res = agg_foolsgold(U, sizes, centre=eng.global_params, history=H if full else H.index_select(0, ids),
                            kappa=kappa, enable=enable, rounds=self.rounds, out=nxt if full else None)
        info = {k: v for k, v in res.info.items() if k != "history"}
        if eng.global_params is not None:  # (no centre: the history is untouched)
            if not full:
                nxt.copy_(H)
                nxt.index_copy_(0, ids, res.info["history"])
            self._cur = 1 - self._cur
            self.rounds = res.info["rounds"]
        return res.params, info


class HyperMode(ServerMode):
    """The pFedHN hypernetwork (``HyperServer``) and its detector; the engine keeps both as ``eng.hyper`` and
    ``eng.detector`` too, for its detection phase and for callers outside (the benchmark reads ``eng.hyper``)."""

    def __init__(self, eng):
        super().__init__(eng)
        cfg = eng.cfg
        net = build_model(eng.model_name, seed=eng.seed + 99)
        target_sd = net.state_dict()
        hyper_ckpt = None
        if cfg.load_parameters:
            if os.path.exists(eng._pth(True)):
                hyper_ckpt = torch.load(eng._pth(True), weights_only=True, map_location="cpu")
            elif os.path.exists(eng._pth(False)):
                net.load_state_dict(torch.load(eng._pth(False), weights_only=True, map_location="cpu"))
                target_sd = net.state_dict()
        self.hyper = eng.hyper = HyperServer(target_sd, cfg.clients, cfg.hyper_lr, cfg.clip_grad_norm, eng.device,
                                             seed=eng.seed)
        if hyper_ckpt is not None:
            if cfg.engine.get("compat-hyper-resume", False):
                print_with_color("[compat A-5] hyper checkpoint loaded then discarded", "yellow")
            else:
                self.hyper.hnet.load_state_dict(hyper_ckpt)
                print_with_color(f"Load state dict from hyper model: {eng._pth(True)}", "yellow")
        hd = cfg.hyper_detection
        if hd.get("enable", False):
            # replicated like validation (the embeddings are bit-identical on every rank; PCA / DBSCAN are
            # deterministic host code); only the leader writes all_embeddings.npy and prints
            eng.detector = HyperDetector(cfg.clients, int(hd.get("n_components", 3)), float(hd.get("eps", 0.007)),
                                         int(hd.get("min_samples", 3)),
                                         save_path=os.path.join(eng.ckpt_dir, "all_embeddings.npy")
                                         if eng.leader else "", verbose=eng.leader)
        self._tail = None  # the checkpoint's constant tail, created on first use
        self._stepped = False  # this round's update ran: its info is read at the round's end

    def early_ok(self) -> bool:
        return self.eng.device.type == "cuda" and self.hyper._native_ok()

    def step(self, U, sizes, attackers, ok_all, w=None, gen_key=None):
        eng = self.eng
        eng.ckpt_writer.fence()  # the previous round's checkpoint copy of the arena, updated in place below
        # (a device ok_all: the update runs, or leaves the hypernetwork untouched, as the device decides)
        kw = {} if ok_all is None else {"enable": ok_all.to(torch.int32).reshape(1), "gen_key": gen_key}
        self.hyper.train(eng.selected, {i: U[k] for k, i in enumerate(eng.selected)}, **kw)
        self._stepped = True
        return {}, None

    def mark(self):
        return self.hyper.step

    def undo(self, mark) -> None:
        self.hyper.step = mark  # the device skipped the hypernetwork update: its step count too
        self.hyper.drop_info()
        self._stepped = False

    def begin_round(self) -> None:
        self._stepped = False

    def end_round(self, info: dict) -> dict:
        if self._stepped:
            info.update(self.hyper.last_info)  # read after validation: no sync between the update and it
        return info

    def state(self) -> dict:
        h = self.hyper
        return {"hyper_arena": h.hnet.arena.detach().cpu(), "hyper_m": h.m.cpu(), "hyper_v": h.v.cpu(),
                "hyper_step": h.step}

    def load(self, srv: dict) -> None:
        if "hyper_m" in srv:
            self.hyper.load_arena(srv["hyper_arena"])
            self.hyper.m.copy_(srv["hyper_m"])
            self.hyper.v.copy_(srv["hyper_v"])
            self.hyper.step = int(srv["hyper_step"])

    def start(self, ids: List[int]) -> torch.Tensor:
        return self.hyper.generate_many(ids)  # (one batched generate)

    def checkpoint(self) -> None:
        """The leader's ``{model}_hyper_{clients}.pth``."""
        hnet = self.hyper.hnet
        # deferred: the arena's copy is issued after the next training launch (utils/ckpt.py)
        if self._tail is None:
            self._tail = hnet.target_tail()
        self.eng.ckpt_writer.submit("hyper", hnet.arena, lambda a: hnet.state_dict_of(a, clone=False),
                                    self.eng._pth(True), defer=True, tail=self._tail)

    def validate(self, n_val: int):
        return self.eng.validation.test_hyper(self.hyper, n_val)


MODES = {**{name: RuleMode for name in AGGREGATORS}, "hyper": HyperMode, "FLTrust": FLTrustMode,
         "foolsgold": FoolsGoldMode, "signguard": SignGuardMode, "flame": FlameMode}
