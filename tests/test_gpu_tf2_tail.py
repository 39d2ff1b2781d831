"""The on-chip TransformerModel trainer's per-step tail (tf2.hip br_update): the owner-computed vector Adam (every
bias / LayerNorm entry updated by the thread whose registers hold its gradient sum, with no barrier between the
weight-gradient units and the update), on full and sparse row tiles, and the abort path through the progress
counters."""
import functools
import time

import pytest
import torch

import test_gpu_transformer as G
from attackfl_amd.models import ParamLayout
from attackfl_amd.ops import transformer as T

pytestmark = pytest.mark.gpu

LAY = ParamLayout.for_model("TransformerModel")


def _is_vector_slot(name):
    """Bias and LayerNorm slots: the entries the vector Adam owns (and the head's)."""
    return name.endswith("bias") or "norm" in name or "_bn." in name


@pytest.mark.parametrize("split", [3, 4])
def test_zero_update_round_trip(gpu, split):
    """One step at lr = 0 through init, a full step and fini: every parameter comes back to the slot it left."""
    rows, params, plan = G._setup(2, [128, 128])
    dev = params.clone().to(gpu)
    ok, _ = T.train_clients(dev, rows.to(gpu), plan.order.to(gpu), plan.nd, 1, 128, 0.0, [11, 12], opt_mode=1,
                            split=split)
    assert ok.tolist() == [1, 1]
    assert torch.equal(dev.cpu(), params)


SPARSE_ND = [128, 100, 17]


@functools.lru_cache(maxsize=None)
def _sparse_case():
    rows, params, plan = G._setup(3, SPARSE_ND)
    ref = params.clone()
    T.reference_train(ref, rows, plan.order, plan.nd, 1, 128, 1.0, [11, 12, 13], opt_mode=1, max_steps=1)
    return rows, params, plan, params - ref


@pytest.mark.parametrize("split", [3, 4])
def test_sparse_row_tiles(gpu, split):
    """One SGD step on batches of 128, 100 and 17 rows (at 17 one wave is full, one has a single row, six have none:
    whole K-slices of the weight-gradient GEMMs are zeros): every slot's raw gradient matches the oracle with the
    bound of test_sgd_step_gradients_match, and in the bias / LayerNorm slots the largest oracle element is the
    largest device element too (a permuted entry -> thread map moves it)."""
    rows, params, plan, g_ref = _sparse_case()
    dev = params.clone().to(gpu)
    ok, _ = T.train_clients(dev, rows.to(gpu), plan.order.to(gpu), plan.nd, 1, 128, 1.0, [11, 12, 13], opt_mode=1,
                            split=split)
    assert ok.tolist() == [1, 1, 1]
    g_dev = params - dev.cpu()
    for s in LAY.slots:
        a = g_dev[:, s.offset:s.offset + s.numel]
        b = g_ref[:, s.offset:s.offset + s.numel]
        scale = b.abs().max().item() + 1e-6
        err = (a - b).abs().max().item() / scale
        print(s.name, "err", err, "scale", scale)
        assert err < 0.08, (s.name, err, scale)
    for s in LAY.slots:
        if not _is_vector_slot(s.name):
            continue
        a = g_dev[:, s.offset:s.offset + s.numel].abs()
        b = g_ref[:, s.offset:s.offset + s.numel].abs()
        for c in range(len(SPARSE_ND)):
            assert int(a[c].argmax()) == int(b[c].argmax()), (s.name, c, int(a[c].argmax()), int(b[c].argmax()))


def test_two_adam_steps(gpu):
    """256 and 129 rows at batch 128: client 0 takes two Adam steps, client 1 one (its size-1 batch is skipped).
    Close to the oracle (bound and form of test_size_one_batch_skipped), and bit-equal from run to run: the
    accumulators their owners zero leave nothing behind from step to step or launch to launch."""
    rows, params, plan = G._setup(2, [256, 129])
    ref = params.clone()
    T.reference_train(ref, rows, plan.order, plan.nd, 1, 128, 0.004, [9, 10])
    outs = []
    for _ in range(3):
        dev = params.clone().to(gpu)
        ok, _ = T.train_clients(dev, rows.to(gpu), plan.order.to(gpu), plan.nd, 1, 128, 0.004, [9, 10])
        assert ok.tolist() == [1, 1]
        outs.append(dev.cpu())
    d = (outs[0] - ref).abs().max().item()
    print("max |dev - ref|", d)
    assert d < 0.02
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_failed_client_returns_promptly(gpu):
    """A NaN parameter in client 1: its round fails (ok 0), client 0 trains, and the launch ends at once — every
    wave leaves the step through the abort check behind the progress counters instead of spinning on one of them
    to the poll bound (2^24 polls of at least 64 cycles each: over 0.4 s at 2.4 GHz, against well under a
    millisecond for the three steps; a timed-out hand-off would also surface as ok = -1)."""
    rows, params, plan = G._setup(2, [300, 300])
    params[1, 5] = float("nan")
    rd, od = rows.to(gpu), plan.order.to(gpu)
    T.train_clients(params.clone().to(gpu), rd, od, plan.nd, 1, 128, 0.004, [1, 2])  # (module load, allocations)
    dev = params.clone().to(gpu)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ok, _ = T.train_clients(dev, rd, od, plan.nd, 1, 128, 0.004, [1, 2])
    dt = time.perf_counter() - t0
    print("failed-client launch", dt, "s")
    assert ok.tolist() == [1, 0]
    assert torch.isfinite(dev[0]).all()
    assert dt < 0.25, dt
