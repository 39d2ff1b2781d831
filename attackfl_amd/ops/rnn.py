"""Fused RNNModel/ICU local training and evaluation (``csrc/kernels/rnn2.hip``, on-chip, split 4; ``rnn.hip``,
the global-workspace kernel, as split 3): one launch trains all of a rank's clients for all their local epochs,
three co-resident workgroups per client (head | vitals | labs).  The launch policy (co-residency, chunking) is
``ops/onchip.py``.

Dropout masks follow the layer-program convention (``fl/programs.py``), so the composite ``RNNProgram`` on CPU is
the exact-semantics oracle of this kernel (tests/test_gpu_rnn.py).
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from . import native, onchip
from .masks import M32

NPARAM = 97665


def device_seed(s: int) -> int:
    """The int32 the kernel receives for client seed ``s`` (low 32 bits, two's complement)."""
    s = int(s) & M32
    return s - 2 ** 32 if s >= 2 ** 31 else s


def train_clients_async(params: torch.Tensor, rows: torch.Tensor, order: torch.Tensor, nd, epochs: int, batch: int,
                        lr: float, seeds: Sequence[int], opt_mode: int = 0, split: int = 4,
                        stamps: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Enqueue the training launch on the current stream and return (ok [C] int32, losses [C, E]) as
    DEVICE tensors without synchronising (see ``onchip.finish``); arguments as ``train_clients``."""
    def train(p, r, o, n, s, kt, st):
        return native().rnn_train(p, r, o, n, s, int(epochs), int(batch), float(lr), int(opt_mode), int(split), kt, st)
    steps = int(epochs) * -(-int(order.shape[2]) // int(batch)) if split == 4 else None
    return onchip.enqueue(TRAINER, train, params, rows, order, nd, seeds, stamps, lr, steps, chunk=True)


def train_clients(params: torch.Tensor, rows: torch.Tensor, order: torch.Tensor, nd, epochs: int, batch: int,
                  lr: float, seeds: Sequence[int], opt_mode: int = 0, split: int = 4,
                  stamps: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Train ``params [C, 97665]`` in place.  Returns (ok [C] int32, losses [C, E]) on the host.

    ``split``: 4 = the on-chip trainer (``rnn2.hip``: weights, optimizer state and activations in registers / LDS
    for the whole round); 3 = the global-workspace kernel (``rnn.hip``).  Both run three workgroups per client.
    ``stamps``: optional device int64 [64] per-phase timers of workgroup ``stamps[63]`` of the first launch
    (split 4 only; tools/phase_profile.py)."""
    return onchip.finish(*train_clients_async(params, rows, order, nd, epochs, batch, lr, seeds, opt_mode, split,
                                              stamps), what=TRAINER.what)


TRAINER = onchip.Trainer(model="RNNModel", nparam=NPARAM, wgs=lambda: 3, device_seed=device_seed,
                         launch=train_clients_async, what="fused RNN trainer")


def eval_many(params: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """Sigmoid outputs of C RNNModels (``params [C, 97665]``, eval mode) over ``rows [n, 24]`` -> ``[C, n]``:
    one launch (``rnn2.hip`` ``k_rnn2_eval``)."""
    p = params if params.dim() == 2 else params[None]
    return native().rnn_eval_many(p.contiguous(), rows.contiguous())
