"""The on-chip TransformerModel trainer with its head split over two workgroups (tf2.hip: head half H0 serves batch
rows 0-63, H1 rows 64-127, each rebuilds the other's rows from an export and runs the full update): the optimiser
sees the same data flow as with one head workgroup, so small rounds are pinned bit for bit to the build before the
split; the gradients are checked against the oracle at batch sizes around the half boundary; a NaN seen by one half
only fails the client at once in every workgroup; and one client more than a launch holds runs in two launches."""
import functools
import hashlib
import json
import os
import time

import pytest
import torch

import test_gpu_transformer as G
from attackfl_amd.fl.trainers import make_plan
from attackfl_amd.models import ParamLayout
from attackfl_amd.ops import onchip
from attackfl_amd.ops import transformer as T

pytestmark = pytest.mark.gpu

LAY = ParamLayout.for_model("TransformerModel")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tf2_twin_bits.json")

# (a) 640 rows: 10 steps, both export-slot parities five times; 65: H1 holds exactly one row; 191: H1 is empty on the
#     second batch (63 rows); 63: H1 is always empty and H0's last tile has 15 rows.  (b) batch 96: H1 holds 32 rows,
#     then (200 rows) a batch of 8; the 97-row client skips its size-1 batch.
CASES = {
    "a": {"nd": [640, 65, 191, 63], "epochs": 2, "batch": 128, "lr": 0.004, "seeds": [21, 22, 23, 24]},
    "b": {"nd": [200, 97], "epochs": 2, "batch": 96, "lr": 0.004, "seeds": [31, 32]},
}


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_case(c, gpu):
    """Trains the case's clients (Adam) and returns the hashes of the parameters, ok and the epoch losses."""
    rows, params, _ = G._setup(len(c["nd"]), c["nd"])
    plan = make_plan(rows.shape[0], c["nd"], c["epochs"], torch.Generator().manual_seed(7), "cpu")
    dev = params.clone().to(gpu)
    ok, losses = T.train_clients(dev, rows.to(gpu), plan.order.to(gpu), plan.nd, c["epochs"], c["batch"], c["lr"],
                                 c["seeds"])
    assert ok.tolist() == [1] * len(c["nd"])
    return {"params": _sha(dev), "ok": _sha(ok), "losses": _sha(losses)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_match_parent_build(gpu, name):
    """Parameters, ok and losses hash to what the one-head build returned (tests/golden/tf2_twin_bits.json, recorded
    on MI355X at the commit before)."""
    with open(GOLDEN) as fh:
        gold = json.load(fh)[name]
    assert gold["case"] == CASES[name]
    got = run_case(CASES[name], gpu)
    print(got)
    assert got == gold["sha256"]


HALF_BATCHES = [2, 63, 64, 65, 127]


@functools.lru_cache(maxsize=None)
def _half_case(bs):
    rows, params, plan = G._setup(2, [bs, bs])
    ref = params.clone()
    T.reference_train(ref, rows, plan.order, plan.nd, 1, bs, 1.0, [11, 12], opt_mode=1, max_steps=1)
    return rows, params, plan, params - ref


@pytest.mark.parametrize("bs", HALF_BATCHES)
def test_half_boundary_gradients(gpu, bs):
    """One raw-SGD step of `bs` rows (H1 empty, one row short of full, exactly full H0, one row in H1, one row short
    of a full batch): every slot's gradient within the bound of test_sparse_row_tiles of the oracle, three runs
    bit-equal, and each client alone bit-equal to the packed launch."""
    rows, params, plan, g_ref = _half_case(bs)
    rd, od = rows.to(gpu), plan.order.to(gpu)
    outs = []
    for _ in range(3):
        dev = params.clone().to(gpu)
        ok, _ = T.train_clients(dev, rd, od, plan.nd, 1, bs, 1.0, [11, 12], opt_mode=1)
        assert ok.tolist() == [1, 1]
        outs.append(dev.cpu())
    g_dev = params - outs[0]
    for s in LAY.slots:
        a = g_dev[:, s.offset:s.offset + s.numel]
        b = g_ref[:, s.offset:s.offset + s.numel]
        scale = b.abs().max().item() + 1e-6
        err = (a - b).abs().max().item() / scale
        print(s.name, "err", err, "scale", scale)
        assert err < 0.08, (s.name, err, scale)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    for c in range(2):
        dev = params[c:c + 1].clone().to(gpu)
        ok, _ = T.train_clients(dev, rd, od[c:c + 1], plan.nd[c:c + 1], 1, bs, 1.0, [11 + c], opt_mode=1)
        assert ok.tolist() == [1]
        assert torch.equal(dev.cpu()[0], outs[0][c]), c


@pytest.mark.parametrize("pos", [100, 20])
def test_nan_in_one_half(gpu, pos):
    """A NaN input feature in the row at batch position `pos` of client 1's first batch (>= 64: only head half H1
    sees it; < 64: only H0): the client's round fails before any update, client 0 trains, and the launch ends at once
    (the bound of test_failed_client_returns_promptly)."""
    rows, params, plan = G._setup(2, [300, 300])
    bad = rows[int(plan.order[1, 0, pos])].clone()
    bad[0] = float("nan")
    rows = torch.cat([rows, bad[None]], 0)
    order = plan.order.clone()
    order[1, 0, pos] = rows.shape[0] - 1
    rd, od = rows.to(gpu), order.to(gpu)
    T.train_clients(params.clone().to(gpu), rd, plan.order.to(gpu), plan.nd, 1, 128, 0.004, [1, 2])  # (module load)
    dev = params.clone().to(gpu)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ok, _ = T.train_clients(dev, rd, od, plan.nd, 1, 128, 0.004, [1, 2])
    dt = time.perf_counter() - t0
    print("failed-client launch", dt, "s")
    assert ok.tolist() == [1, 0]
    out = dev.cpu()
    assert torch.equal(out[1], params[1])  # (the failing step is the first: the pre-step values are the initial ones)
    assert torch.isfinite(out).all() and not torch.equal(out[0], params[0])
    assert dt < 0.25, dt


def test_one_client_more_than_a_launch_holds(gpu):
    """onchip.capacity(gpu, 4) + 1 clients of 4 rows, 1 epoch: two launches, every client trains, and the result is
    bit-equal to the same clients launched as the two chunks explicitly."""
    cap = onchip.capacity(gpu, 4)
    C = cap + 1
    parts = onchip.client_chunks(C, cap)
    assert len(parts) == 2
    rows, base, _ = G._setup(1, [4])
    params = base.repeat(C, 1) * (1.0 + 1e-3 * torch.arange(C, dtype=torch.float32)[:, None])
    plan = make_plan(rows.shape[0], [4] * C, 1, torch.Generator().manual_seed(7), "cpu")
    seeds = list(range(40, 40 + C))
    rd, od = rows.to(gpu), plan.order.to(gpu)
    dev = params.clone().to(gpu)
    ok, losses = T.train_clients(dev, rd, od, plan.nd, 1, 128, 0.004, seeds)
    assert ok.tolist() == [1] * C
    assert not torch.equal(dev.cpu(), params)
    for a, b in parts:
        part = params[a:b].clone().to(gpu)
        ok_p, losses_p = T.train_clients(part, rd, od[a:b], plan.nd[a:b], 1, 128, 0.004, seeds[a:b])
        assert ok_p.tolist() == [1] * (b - a)
        assert torch.equal(part, dev[a:b]) and torch.equal(losses_p, losses[a:b])
