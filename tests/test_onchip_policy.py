"""The persistent trainers' launch policy (attackfl_amd/ops/onchip.py), on the CPU: the co-residency budget with a
substituted CU count, the chunking of a launch, the trainer descriptions and the import structure."""
import ast
import os
import subprocess
import sys

import pytest
import torch

from attackfl_amd.ops import onchip
from attackfl_amd.parallel import launcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def mi355x(monkeypatch):
    """One MI355X: 256 CUs, whatever device is asked for; no launch cap, sharers set by the test."""
    monkeypatch.setattr(onchip, "device_cus", lambda dev: 256)
    monkeypatch.delenv("AFL_MAX_CLIENTS_PER_LAUNCH", raising=False)
    monkeypatch.setattr(launcher, "_SHARERS", None)
    return lambda n: monkeypatch.setattr(launcher, "_SHARERS", n)


# max(1, (256 // sharers) // wgs)
CAPACITY = {(1, 3): 85, (1, 4): 64, (1, 32): 8, (8, 3): 10, (8, 4): 8, (8, 32): 1}


@pytest.mark.parametrize("sharers,wgs", sorted(CAPACITY))
def test_capacity_on_256_cus(mi355x, monkeypatch, sharers, wgs):
    mi355x(sharers)
    want = CAPACITY[(sharers, wgs)]
    assert onchip.cu_share("cuda:0") == 256 // sharers
    assert onchip.capacity("cuda:0", wgs) == want
    monkeypatch.setenv("AFL_MAX_CLIENTS_PER_LAUNCH", "2")
    assert onchip.capacity("cuda:0", wgs) == min(want, 2)
    assert onchip.capacity("cuda:0", wgs_per_client=wgs) == min(want, 2)


def test_capacity_is_at_least_one_and_needs_the_workgroup_count(mi355x):
    mi355x(128)  # a share of 2 CUs, fewer than any trainer's workgroups per client
    assert onchip.cu_share("cuda:0") == 2
    for wgs in (3, 4, 32):
        assert onchip.capacity("cuda:0", wgs) == 1
    with pytest.raises(TypeError):
        onchip.capacity("cuda:0")


def _record(calls):
    def launch(params, order, nd, seeds, first):
        calls.append((params, order, nd, seeds, first))
        return params[:, 0].to(torch.int32), params[:, 1:3]
    return launch


def test_chunked_slices_in_client_order():
    C = 17
    params = torch.arange(C * 3, dtype=torch.float32).reshape(C, 3)
    order = torch.arange(C * 2).reshape(C, 1, 2)
    nd, seeds = torch.arange(C), torch.arange(C) + 100
    calls = []
    ok, losses = onchip.chunked(_record(calls), C, 8, params, order, nd, seeds)
    bounds = [(0, 6), (6, 12), (12, 17)]
    assert onchip.client_chunks(C, 8) == bounds
    assert len(calls) == 3
    for (a, b), (p, o, n, s, first) in zip(bounds, calls):
        assert torch.equal(p, params[a:b]) and torch.equal(o, order[a:b])
        assert torch.equal(n, nd[a:b]) and torch.equal(s, seeds[a:b])
        assert first is (a == 0)
    assert torch.equal(ok, params[:, 0].to(torch.int32))
    assert torch.equal(losses, params[:, 1:3])


@pytest.mark.parametrize("C", [1, 7, 8])
def test_chunked_one_launch_gets_the_unsliced_tensors(C):
    params = torch.arange(C * 3, dtype=torch.float32).reshape(C, 3)
    order, nd, seeds = torch.zeros(C, 1, 2), torch.arange(C), torch.arange(C)
    calls = []
    ok, losses = onchip.chunked(_record(calls), C, 8, params, order, nd, seeds)
    assert len(calls) == 1
    p, o, n, s, first = calls[0]
    assert p is params and o is order and n is nd and s is seeds and first is True
    assert torch.equal(ok, params[:, 0].to(torch.int32)) and torch.equal(losses, params[:, 1:3])


def test_onchip_imports_without_the_model_modules():
    code = ("import sys; import attackfl_amd.ops.onchip; "
            "bad = [m for m in ('attackfl_amd.ops.transformer', 'attackfl_amd.ops.rnn') if m in sys.modules]; "
            "assert not bad, bad")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr


def _imported(path):
    """Modules a file imports anywhere, function bodies included, as (level, module, names)."""
    tree = ast.parse(open(path).read())
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            out.append((node.level, node.module or "", [a.name for a in node.names]))
        elif isinstance(node, ast.Import):
            out += [(0, a.name, []) for a in node.names]
    return out


@pytest.mark.parametrize("mod,other", [("transformer", "rnn"), ("rnn", "transformer"), ("onchip", "rnn"),
                                       ("onchip", "transformer")])
def test_model_modules_do_not_import_each_other(mod, other):
    for level, module, names in _imported(os.path.join(ROOT, "attackfl_amd", "ops", mod + ".py")):
        assert module.split(".")[-1] != other, (mod, module)
        if module in ("", "ops", "attackfl_amd.ops"):
            assert other not in names, (mod, names)


SEEDS = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 63 + 5]


def test_trainer_descriptions():
    from attackfl_amd.ops import rnn, transformer

    tf, rn = transformer.TRAINER, rnn.TRAINER
    assert (tf.model, tf.nparam, tf.what) == ("TransformerModel", 47693, "fused trainer")
    assert (rn.model, rn.nparam, rn.what) == ("RNNModel", 97665, "fused RNN trainer")
    assert rn.wgs() == 3
    # the kernels' int32 seed forms: the low 31 bits (TransformerModel), the low 32 bits as two's complement (RNNModel)
    assert [tf.device_seed(s) for s in SEEDS] == [0, 1, 2 ** 31 - 1, 0, 2 ** 31 - 1, 5]
    assert [rn.device_seed(s) for s in SEEDS] == [0, 1, 2 ** 31 - 1, -2 ** 31, -1, 5]
    assert [tf.device_seed(s) for s in SEEDS] == [transformer.device_seed(s) for s in SEEDS]
    assert [rn.device_seed(s) for s in SEEDS] == [rnn.device_seed(s) for s in SEEDS]
    assert tf.launch is transformer.train_clients_async and rn.launch is rnn.train_clients_async
    with pytest.raises(Exception):  # frozen
        tf.nparam = 1
