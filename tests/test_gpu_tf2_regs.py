"""The on-chip TransformerModel trainer after its move to one register class (tf2.hip): the optimiser sees the same
data flow as before, so a small round is pinned bit for bit to the build before the move, and the row loads, whose
address arithmetic is rebuilt in the hand-off window, fetch the rows the order table names for every client."""
import functools
import hashlib
import json
import os

import pytest
import torch

import test_gpu_transformer as G
from attackfl_amd.fl.trainers import make_plan
from attackfl_amd.models import ParamLayout
from attackfl_amd.ops import transformer as T

pytestmark = pytest.mark.gpu

LAY = ParamLayout.for_model("TransformerModel")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tf2_bits.json")


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def test_bits_match_parent_build(gpu):
    """3 clients of 130, 100 and 17 rows, 2 epochs at batch 128 (a full batch, then a 2-row batch and an epoch boundary;
    17 rows leave six waves without rows), Adam: parameters, ok and losses hash to what the two-class build returned
    (tests/golden/tf2_bits.json, recorded on MI355X at the commit before)."""
    with open(GOLDEN) as fh:
        gold = json.load(fh)
    c = gold["case"]
    rows, params, _ = G._setup(c["clients"], c["nd"])
    plan = make_plan(rows.shape[0], c["nd"], c["epochs"], torch.Generator().manual_seed(7), "cpu")
    dev = params.clone().to(gpu)
    ok, losses = T.train_clients(dev, rows.to(gpu), plan.order.to(gpu), plan.nd, c["epochs"], c["batch"], c["lr"],
                                 c["seeds"])
    assert ok.tolist() == [1, 1, 1]
    assert str(ok.dtype) == "torch." + gold["dtypes"]["ok"] and str(losses.dtype) == "torch." + gold["dtypes"]["losses"]
    got = {"params": _sha(dev), "ok": _sha(ok), "losses": _sha(losses)}
    print(got)
    assert got == gold["sha256"]


ROW_ND = [128, 100, 17]


@functools.lru_cache(maxsize=None)
def _row_case():
    """The row table (2000 rows) is larger than any client uses; the last client's order names the table's last rows."""
    rows, params, plan = G._setup(3, ROW_ND)
    order = plan.order.clone()
    n = ROW_ND[2]
    order[2, 0, :n] = torch.arange(rows.shape[0] - n, rows.shape[0], dtype=order.dtype).flip(0)
    ref = params.clone()
    T.reference_train(ref, rows, order, plan.nd, 1, 128, 1.0, [11, 12, 13], opt_mode=1, max_steps=1)
    return rows, params, order, plan.nd, params - ref


def test_row_addressing(gpu):
    """One raw-SGD step: every slot's gradient within the bound of test_sparse_row_tiles of the oracle that reads the
    same order table (clients 1 and 2 exercise the cid > 0 offsets; a wrong row moves the input-side gradients far
    past the bound), and two runs bit-equal."""
    rows, params, order, nd, g_ref = _row_case()
    outs = []
    for _ in range(2):
        dev = params.clone().to(gpu)
        ok, _ = T.train_clients(dev, rows.to(gpu), order.to(gpu), nd, 1, 128, 1.0, [11, 12, 13], opt_mode=1)
        assert ok.tolist() == [1, 1, 1]
        outs.append(dev.cpu())
    g_dev = params - outs[0]
    for s in LAY.slots:
        a = g_dev[:, s.offset:s.offset + s.numel]
        b = g_ref[:, s.offset:s.offset + s.numel]
        scale = b.abs().max().item() + 1e-6
        err = (a - b).abs().max().item() / scale
        print(s.name, "err", err, "scale", scale)
        assert err < 0.08, (s.name, err, scale)
    assert torch.equal(outs[0], outs[1])
