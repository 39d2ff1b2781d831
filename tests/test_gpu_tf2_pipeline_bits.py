"""The on-chip TransformerModel trainer (tf2.hip) after the step chain's latency work — weight fragments loaded ahead
of their MFMAs, the vector Adam run inside the units' staged Adam — against the build before it: small rounds hash to
what the parent commit's library returned (tests/golden/tf2_pipeline_bits.json names that commit), and the bias /
LayerNorm tensors — the vector entries whose Adam moved — are compared tensor by tensor.

Cases (batch 128): 293 rows = 3 steps per epoch with a last batch of 37 rows (head half H1 without a valid row), two
epochs = six Adam steps (an Adam contraction slip shows from the second step on); 200 rows = a second batch of 72
rows, which spans both head halves; the SGD mode through the same update code; a NaN label in step 2, after which
the client has failed and holds the parameters of step 1.

    python tests/test_gpu_tf2_pipeline_bits.py OUT.json COMMIT     records the goldens with the library that is
                                                                    loaded (COMMIT: the commit it was built from)
"""
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (for the recording run below)

import test_gpu_transformer as G
from attackfl_amd.fl.trainers import make_plan
from attackfl_amd.models import ParamLayout
from attackfl_amd.ops import transformer as T

pytestmark = pytest.mark.gpu

LAY = ParamLayout.for_model("TransformerModel")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tf2_pipeline_bits.json")

# opt_mode 0 = Adam, 1 = the kernel's SGD mode; nan_step: the (1-based) step of epoch 0 whose batch gets a NaN label
CASES = {
    "293x1": {"nd": [293], "epochs": 2, "batch": 128, "lr": 0.004, "seeds": [41], "opt_mode": 0, "nan_step": 0},
    "293x3": {"nd": [293] * 3, "epochs": 2, "batch": 128, "lr": 0.004, "seeds": [41, 42, 43], "opt_mode": 0,
              "nan_step": 0},
    "200x1": {"nd": [200], "epochs": 2, "batch": 128, "lr": 0.004, "seeds": [51], "opt_mode": 0, "nan_step": 0},
    "200x3": {"nd": [200] * 3, "epochs": 2, "batch": 128, "lr": 0.004, "seeds": [51, 52, 53], "opt_mode": 0,
              "nan_step": 0},
    "293x1-sgd": {"nd": [293], "epochs": 2, "batch": 128, "lr": 0.004, "seeds": [41], "opt_mode": 1, "nan_step": 0},
    "293x1-nan": {"nd": [293], "epochs": 2, "batch": 128, "lr": 0.004, "seeds": [41], "opt_mode": 0, "nan_step": 2},
}


def vector_slots():
    """The bias and LayerNorm tensors of both branches and the head: the trainer's vector entries."""
    return [s for s in LAY.slots if s.name.endswith(".bias") or s.name.endswith("norm.weight")
            or s.name.endswith("_bn.weight") or s.name.endswith("in_proj_bias")]


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def _inputs(nclients, nd0, epochs):
    rows, params, _ = G._setup(nclients, [nd0] * nclients)
    plan = make_plan(rows.shape[0], [nd0] * nclients, epochs, torch.Generator().manual_seed(7), "cpu")
    return rows, params, plan


def run_case(c, gpu):
    """Trains the case's clients; returns (hashes of params / ok / losses, {vector tensor: hash}, ok as a list)."""
    rows, params, plan = _inputs(len(c["nd"]), c["nd"][0], c["epochs"])
    order = plan.order
    if c["nan_step"]:
        pos = (c["nan_step"] - 1) * c["batch"] + 5  # a row of that step's batch, epoch 0, client 0
        bad = rows[int(order[0, 0, pos])].clone()
        bad[-1] = float("nan")
        rows = torch.cat([rows, bad[None]], 0)
        order = order.clone()
        order[0, 0, pos] = rows.shape[0] - 1
    dev = params.clone().to(gpu)
    ok, losses = T.train_clients(dev, rows.to(gpu), order.to(gpu), plan.nd, c["epochs"], c["batch"], c["lr"],
                                 c["seeds"], opt_mode=c["opt_mode"])
    out = dev.cpu()
    vec = {s.name: _sha(out[:, s.offset:s.offset + s.numel]) for s in vector_slots()}
    return {"params": _sha(out), "ok": _sha(ok), "losses": _sha(losses)}, vec, ok.tolist(), out, params


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_match_parent_build(gpu, name):
    """Parameters, per-epoch losses and ok hash to what the parent commit's library returned, and so does every
    bias / LayerNorm tensor on its own (the message names the first that differs)."""
    with open(GOLDEN) as fh:
        gold = json.load(fh)["cases"][name]
    c = CASES[name]
    assert gold["case"] == c
    sha, vec, ok, out, params = run_case(c, gpu)
    print(name, "ok", ok, sha)
    assert ok == ([0] if c["nan_step"] else [1] * len(c["nd"]))
    if c["nan_step"]:  # failed in step 2: the update of step 1 was applied, nothing after it
        assert torch.isfinite(out).all() and not torch.equal(out, params)
    assert sorted(vec) == sorted(gold["vector"]) and len(vec) == 25
    diff = [s.name for s in vector_slots() if vec[s.name] != gold["vector"][s.name]]
    print(name, "vector tensors that differ:", diff)
    assert not diff, f"first differing bias / LayerNorm tensor: {diff[0]} ({len(diff)} of {len(vec)} differ)"
    assert sha == gold["sha256"]


if __name__ == "__main__":
    gpu = torch.device("cuda", 0)
    cases = {}
    for name in sorted(CASES):
        sha, vec, ok, _, _ = run_case(CASES[name], gpu)
        cases[name] = {"case": CASES[name], "ok": ok, "sha256": sha, "vector": vec}
    with open(sys.argv[1], "w") as fh:
        json.dump({"recorded_with": sys.argv[2],
                   "dtypes": {"params": "float32", "ok": "int32", "losses": "float32"}, "cases": cases}, fh, indent=1)
    print("wrote", sys.argv[1])
