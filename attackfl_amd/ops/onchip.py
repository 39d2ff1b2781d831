"""Host side of a persistent training launch (tf2 / rnn2 / cnn2): the launch policy, stated once, and the plumbing
every such launch shares.  The policy:
* every workgroup of a client must be co-resident (they spin on each other's hand-off words), one per CU;
* a process may count only on its share of the CUs (``cu_share``): other processes on the GPU run their own;
* more clients than one launch holds (``capacity``) run as back-to-back launches of clients that fit
  (``client_chunks`` / ``chunked``), bit-identical to the one-launch run.

``Trainer`` describes one fused trainer to ``fl.trainers.FusedTrainer``; the instances live with their models
(``ops.transformer.TRAINER``, ``ops.rnn.TRAINER``).  This module imports neither and needs no GPU to import.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Tuple

import numpy as np
import torch

from ..parallel.launcher import gpu_sharers


def device_cus(dev) -> int:
    """CUs of the whole device (the module's one device query)."""
    return torch.cuda.get_device_properties(dev).multi_processor_count


def cu_share(dev) -> int:
    """This process's share of the device's CUs: processes sharing the GPU run their own persistent launches on
    the same CUs, so a launch may count on only its share of them."""
    return device_cus(dev) // gpu_sharers()


def capacity(dev, wgs_per_client: int) -> int:
    """Clients per persistent launch of ``wgs_per_client`` co-resident workgroups each (rnn2 3, tf2 4, cnn2 32) on
    this process's share of the CUs, at least 1; ``AFL_MAX_CLIENTS_PER_LAUNCH`` caps it (tests).  More clients run
    in back-to-back launches."""
    cap = max(1, cu_share(dev) // wgs_per_client)
    lim = int(os.environ.get("AFL_MAX_CLIENTS_PER_LAUNCH", "0") or 0)
    return min(cap, lim) if lim > 0 else cap


def client_chunks(C: int, cap: int) -> List[Tuple[int, int]]:
    """[a, b) client ranges of at most ``cap`` clients, as few launches as possible, balanced."""
    if C <= 0:
        return []
    n = -(-C // max(1, cap))
    size = -(-C // n)
    return [(a, min(C, a + size)) for a in range(0, C, size)]


def chunked(launch, C: int, cap: int, params, order, nd_t, seeds_t):
    """Run ``launch(params, order, nd, seeds, first) -> (ok, losses)`` over client chunks of at most ``cap``
    clients, back to back on the current stream (``first``: the chunk that takes the diagnostic stamps, if any);
    the per-chunk device results are concatenated (no host sync)."""
    parts = client_chunks(C, cap)
    if len(parts) <= 1:
        return launch(params, order, nd_t, seeds_t, True)
    oks, losses = [], []
    for i, (a, b) in enumerate(parts):
        ok, ls = launch(params[a:b], order[a:b], nd_t[a:b], seeds_t[a:b], i == 0)
        oks.append(ok)
        losses.append(ls)
    return torch.cat(oks), torch.cat(losses)


def on_device(t, dev) -> bool:
    """``t`` is already an int32 tensor on ``dev`` (the engine stages a round's metadata there)."""
    return torch.is_tensor(t) and t.device == dev and t.dtype == torch.int32


def dev_i32(nd, dev) -> torch.Tensor:
    """``nd`` as a device int32 tensor (passed through when the engine already staged it there)."""
    if on_device(nd, dev):
        return nd
    return torch.as_tensor(list(nd) if not torch.is_tensor(nd) else nd.tolist(), dtype=torch.int32, device=dev)


_KT_CACHE: Dict[tuple, torch.Tensor] = {}


def adam_step_table(lr: float, steps: int, dev) -> torch.Tensor:
    """[n >= steps, 2] fp32 device table of torch.optim.Adam's per-step scalars, computed in double like
    torch does on the host: (lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)) for t = 1..n.  Cached per (lr,
    device) and grown in powers of two, so a round never uploads it again."""
    key = (lr, str(dev))
    t = _KT_CACHE.get(key)
    if t is None or t.shape[0] < steps:
        n = 1 << max(10, (max(steps, 1) - 1).bit_length())
        tt = np.arange(1, n + 1, dtype=np.float64)
        tab = np.stack([lr / (1.0 - 0.9 ** tt), 1.0 / np.sqrt(1.0 - 0.999 ** tt)], axis=1).astype(np.float32)
        t = _KT_CACHE[key] = torch.from_numpy(tab).to(dev)
    return t


def finish(ok: torch.Tensor, losses: torch.Tensor, what: str = "fused trainer") -> Tuple[torch.Tensor, torch.Tensor]:
    """Synchronise on an enqueued launch -> host (ok, losses); a negative ok means a cross-workgroup hand-off
    timed out."""
    ok = ok.cpu()
    if bool((ok < 0).any()):
        raise RuntimeError(f"{what}: a cross-workgroup hand-off timed out (workgroups not co-resident?)")
    return ok, losses.cpu()


@dataclass(frozen=True)
class Trainer:
    """One fused whole-round trainer, as ``FusedTrainer`` sees it."""

    model: str
    nparam: int
    wgs: Callable[[], int]              # workgroups per client of the on-chip launch (asked when first needed)
    device_seed: Callable[[int], int]   # the int32 the kernel receives for a client seed
    launch: Callable                    # (params, rows, order, nd, epochs, batch, lr, seeds) -> device (ok, losses)
    what: str                           # error label of ``finish``

    def capacity(self, dev) -> int:
        return capacity(dev, self.wgs())


def enqueue(t: Trainer, train, params, rows, order, nd, seeds, stamps, lr: float, steps, chunk: bool):
    """Stage a round's metadata and enqueue ``train(params, rows, order, nd, seeds, kt, stamps)`` on the current
    stream, over chunks of ``t.capacity`` clients when ``chunk`` (a stamped run stamps its first chunk only) ->
    DEVICE (ok [C] int32, losses [C, E]), no host sync.  ``steps``: optimizer steps per client of an on-chip
    launch, which takes the Adam step table ``kt``; None for the global-workspace kernels."""
    dev = params.device
    nd_t = dev_i32(nd, dev)
    seeds_t = seeds if on_device(seeds, dev) else \
        torch.tensor([t.device_seed(s) for s in seeds], dtype=torch.int32, device=dev)
    kt = adam_step_table(float(lr), steps, dev) if steps is not None else None
    rows_c, order_c = rows.contiguous(), order.contiguous()

    def launch(p, o, n, s, first=True):
        return train(p, rows_c, o, n, s, kt, stamps if first else None)
    if not chunk:
        return launch(params, order_c, nd_t, seeds_t)
    return chunked(launch, params.shape[0], t.capacity(dev), params, order_c, nd_t, seeds_t)
