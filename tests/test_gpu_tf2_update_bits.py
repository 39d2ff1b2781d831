"""The on-chip TransformerModel trainer (tf2.hip) after its update tail was regrouped — the leaders' ffn.3 / ffn.0 Adam,
images and stores before counter A, right behind the abort decision they now take after counter C; the dense tile and
the vector entries in a pass of their own after counter B — against the build before it: small rounds hash to what
the parent commit's library returned
(tests/golden/tf2_update_bits.json names that commit), and the weight tensors whose Adam moved are compared tensor by
tensor: dense, ffn.0, ffn.3, out_proj and the v rows of in_proj, both branches.

Cases (batch 128, 2 epochs, lr 0.004): 293 rows = 3 steps per epoch with a last batch of 37 rows, one client and three;
130 rows = a last batch of 2 rows; 128 rows = exactly one full batch per epoch; the SGD mode through the same update
code.  Abort placement: a NaN label in step 1 must leave every parameter as it was (the ffn update now precedes
counter A: it must still follow the abort decision); a NaN label in step 2 of client 1 of 3 leaves that client with
its step-1 parameters and the other two clients untouched by it.

    python tests/test_gpu_tf2_update_bits.py OUT.json COMMIT     records the goldens with the library that is
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
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tf2_update_bits.json")

# opt_mode 0 = Adam, 1 = the kernel's SGD mode; nan: (client, 1-based step of epoch 0) whose batch gets a NaN label
BASE = {"epochs": 2, "batch": 128, "lr": 0.004, "opt_mode": 0, "nan": None}
CASES = {
    "293x1": dict(BASE, nd=[293], seeds=[41]),
    "293x3": dict(BASE, nd=[293] * 3, seeds=[41, 42, 43]),
    "130x1": dict(BASE, nd=[130], seeds=[61]),
    "128x1": dict(BASE, nd=[128], seeds=[71]),
    "293x1-sgd": dict(BASE, nd=[293], seeds=[41], opt_mode=1),
    # not compared as a whole: client 1's parameters after its only applied step are the golden
    "293x3-nan": dict(BASE, nd=[293] * 3, seeds=[41, 42, 43], nan=[1, 2]),
}
BITS = ["128x1", "130x1", "293x1", "293x1-sgd", "293x3"]
NAN_STEP1 = dict(BASE, nd=[293], seeds=[41], nan=[0, 1])


def weight_views():
    """(name, offset, numel) of the weight tensors whose Adam the update tail runs, both branches."""
    by = {s.name: s for s in LAY.slots}
    out = []
    for b in ("vitals", "labs"):
        for n in ("dense.weight", "transformer.ffn.0.weight", "transformer.ffn.3.weight",
                  "transformer.attention.out_proj.weight"):
            s = by[f"{b}_{n}"]
            out.append((s.name, s.offset, s.numel))
        s = by[f"{b}_transformer.attention.in_proj_weight"]  # [192, 64]: the v rows are 128 .. 191
        out.append((s.name + "[v]", s.offset + 128 * 64, 64 * 64))
    return out


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def _inputs(nclients, nd0, epochs):
    rows, params, _ = G._setup(nclients, [nd0] * nclients)
    plan = make_plan(rows.shape[0], [nd0] * nclients, epochs, torch.Generator().manual_seed(7), "cpu")
    return rows, params, plan


def run_case(c, gpu):
    """Trains the case's clients; returns the hashes (whole / per weight tensor / per client), ok, the trained and
    the initial parameters."""
    rows, params, plan = _inputs(len(c["nd"]), c["nd"][0], c["epochs"])
    order = plan.order
    if c["nan"]:
        cl, step = c["nan"]
        pos = (step - 1) * c["batch"] + 5  # a row of that step's batch, epoch 0
        bad = rows[int(order[cl, 0, pos])].clone()
        bad[-1] = float("nan")
        rows = torch.cat([rows, bad[None]], 0)
        order = order.clone()
        order[cl, 0, pos] = rows.shape[0] - 1
    dev = params.clone().to(gpu)
    ok, losses = T.train_clients(dev, rows.to(gpu), order.to(gpu), plan.nd, c["epochs"], c["batch"], c["lr"],
                                 c["seeds"], opt_mode=c["opt_mode"])
    out = dev.cpu()
    return {"sha256": {"params": _sha(out), "ok": _sha(ok), "losses": _sha(losses)},
            "weights": {n: _sha(out[:, o:o + k]) for n, o, k in weight_views()},
            "clients": [_sha(out[i]) for i in range(out.shape[0])],
            "ok": ok.tolist(), "out": out, "params": params}


_RUNS = {}


def _run(name, gpu):
    """One training run per case and session (the clean three-client run serves two tests)."""
    if name not in _RUNS:
        _RUNS[name] = run_case(CASES[name], gpu)
    return _RUNS[name]


@functools.lru_cache(maxsize=None)
def _gold():
    with open(GOLDEN) as fh:
        return json.load(fh)["cases"]


@pytest.mark.parametrize("name", BITS)
def test_bits_match_parent_build(gpu, name):
    """Parameters, per-epoch losses and ok hash to what the parent commit's library returned, and so does every weight
    tensor of the update tail on its own (the message names the first that differs)."""
    gold = _gold()[name]
    assert gold["case"] == CASES[name]
    r = _run(name, gpu)
    print(name, "ok", r["ok"], r["sha256"])
    assert r["ok"] == [1] * len(CASES[name]["nd"])
    assert sorted(r["weights"]) == sorted(gold["weights"]) and len(r["weights"]) == 10
    diff = [n for n, _, _ in weight_views() if r["weights"][n] != gold["weights"][n]]
    print(name, "weight tensors that differ:", diff)
    assert not diff, f"first differing weight tensor: {diff[0]} ({len(diff)} of {len(r['weights'])} differ)"
    assert r["sha256"] == gold["sha256"]


def test_nan_in_step_1_updates_nothing(gpu):
    """A NaN label in the first step: the client fails and every parameter keeps its initial bits — no update of the
    step, the ffn tiles' early one included, is applied before the abort decision."""
    r = run_case(NAN_STEP1, gpu)
    print("nan step 1: ok", r["ok"])
    assert r["ok"] == [0]
    same = r["out"].view(torch.int32) == r["params"].view(torch.int32)
    moved = [n for n, o, k in weight_views() if not bool(same[:, o:o + k].all())]
    print("nan step 1: weight tensors that moved:", moved, "elements that moved:", int((~same).sum()))
    assert not moved, f"first weight tensor updated in an aborted step: {moved[0]}"
    assert bool(same.all())


def test_nan_in_step_2_of_one_client(gpu):
    """A NaN label in step 2 of client 1 of 3: clients 0 and 2 end where the clean three-client run ends, client 1 holds
    the parameters of its step 1 (what the parent commit's library left there)."""
    gold = _gold()
    assert gold["293x3-nan"]["case"] == CASES["293x3-nan"]
    r = run_case(CASES["293x3-nan"], gpu)
    print("nan step 2 of client 1: ok", r["ok"])
    assert r["ok"] == [1, 0, 1]
    assert r["clients"][0] == gold["293x3"]["clients"][0], "client 0 differs from the clean run"
    assert r["clients"][2] == gold["293x3"]["clients"][2], "client 2 differs from the clean run"
    assert torch.isfinite(r["out"][1]).all() and not torch.equal(r["out"][1], r["params"][1])
    if r["clients"][1] != gold["293x3-nan"]["clients"][1]:
        diff = [n for n, _, _ in weight_views() if r["weights"][n] != gold["293x3-nan"]["weights"][n]]
        pytest.fail(f"client 1 does not hold the parent's step-1 parameters; weight tensors that differ: {diff}")


if __name__ == "__main__":
    gpu = torch.device("cuda", 0)
    cases = {}
    for name in sorted(CASES):
        r = run_case(CASES[name], gpu)
        cases[name] = {"case": CASES[name], "ok": r["ok"], "sha256": r["sha256"], "weights": r["weights"],
                       "clients": r["clients"]}
    with open(sys.argv[1], "w") as fh:
        json.dump({"recorded_with": sys.argv[2],
                   "dtypes": {"params": "float32", "ok": "int32", "losses": "float32"}, "cases": cases}, fh, indent=1)
    print("wrote", sys.argv[1])
