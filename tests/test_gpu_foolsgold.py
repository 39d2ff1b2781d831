"""FoolsGold on the device: ``k_hist_gram`` (the history step and its Gram in one sweep) against the torch expression, the
anchored Gram pass and the fp64 product; ``k_foolsgold_weights`` against the composite on the device's own Gram;
``agg.foolsgold`` (four launches) against the fp64 parameter-space loop of tests/test_foolsgold.py; bit reproducibility;
refused arguments; the engine (the early launch against the serial schedule, with and without a failed round).

Bounds.  History: bit equality with ``H + (U - g[None])``, two fp32 roundings that any IEEE device makes alike.  Gram:
bit equality with ``ops.gram_anchored(H_new, zeros)`` (same tile walk, MFMA order and reduction), and 1e-9 max |G|
against the fp64 product, the bound tests/test_gpu_cclip.py holds the anchored pass to.  Weights: 1e-9 absolute on
alpha and c in [0, 1] against the composite on the same Gram: the map from cosines to alpha is continuous with slope
<= 4.3 kappa where it is not clipped, and fp64 leaves orders of margin."""
import os

import pytest
import torch

import test_foolsgold as R
from attackfl_amd import agg, ops
from attackfl_amd.config import from_dict
from attackfl_amd.fl.engine import FLEngine, build_client_table
from attackfl_amd.ops import composite as C
from launch import parse_attackers

pytestmark = pytest.mark.gpu

HIST_SHAPES = [(n, P) for n in (1, 2, 3, 8, 17, 33, 64) for P in (1, 63, 1025, 4099)] + [(8, 47693)]
WEIGHT_NS = [1, 2, 3, 8, 33, 64]


def make_hist(n, P):
    """An old history of about two rounds' updates, this round's rows and the model the round started from."""
    gen = torch.Generator().manual_seed(100 * n + P % 97)
    g = 0.3 * torch.randn(P, generator=gen)
    H = 0.014 * torch.randn(n, P, generator=gen)
    U = g[None] + 0.01 * torch.randn(n, P, generator=gen)
    return U, g, H


def bits(t):
    return t.detach().cpu().view(torch.int32)


# ---------------------------------------------------------------------------------- k_hist_gram
@pytest.mark.parametrize("n,P", HIST_SHAPES)
def test_hist_gram_bits_and_accuracy(gpu, n, P):
    U, g, H = make_hist(n, P)
    want = H + (U - g[None])
    Ud, gd, Hd = U.to(gpu), g.to(gpu), H.to(gpu)
    Hn, G = ops.hist_gram(Ud, gd, Hd, None)
    assert Hn.is_cuda and Hn.dtype == torch.float32 and Hn.data_ptr() != Hd.data_ptr()
    assert torch.equal(bits(Hn), bits(want))
    assert torch.equal(Hd.cpu(), H) and torch.equal(Ud.cpu(), U)  # (the inputs are read only)
    assert G.shape == (n, n) and G.dtype == torch.float64
    assert torch.equal(G, ops.gram_anchored(Hn, torch.zeros(P, device=gpu)))
    ref = want.double() @ want.double().t()
    err = (G.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)
    print(f"hist_gram n={n} P={P}: Gram error {err:.3e} max |G|")
    assert err <= 1e-9
    # enable = 1 from the device is the same pass; a second buffer of the caller's receives the history
    out = torch.full_like(Hd, float("nan"))
    Hn2, G2 = ops.hist_gram(Ud, gd, Hd, torch.ones(1, dtype=torch.int32, device=gpu), out=out)
    assert Hn2 is out and torch.equal(out, Hn) and torch.equal(G2, G)


@pytest.mark.parametrize("n,P", [(3, 63), (17, 1025), (64, 4099)])
def test_hist_gram_enable_zero_keeps_the_old_bits(gpu, n, P):
    U, g, H = make_hist(n, P)
    H[0, :3] = torch.tensor([-0.0, 0.0, 1e-45][:min(3, P)])  # (selected, not added to zero)
    U[n - 1] = float("nan")  # a faulted client's row in the failed round
    off = torch.zeros(1, dtype=torch.int32, device=gpu)
    Hn, G = ops.hist_gram(U.to(gpu), g.to(gpu), H.to(gpu), off)
    assert torch.equal(bits(Hn), bits(H))
    assert torch.equal(G, ops.gram_anchored(Hn, torch.zeros(P, device=gpu)))


def test_65_rows_take_the_composite(gpu):
    U, g, H = make_hist(65, 33)
    Hn, G = ops.hist_gram(U.to(gpu), g.to(gpu), H.to(gpu), None)
    assert Hn.is_cuda and torch.equal(bits(Hn), bits(H + (U - g[None])))
    ref = Hn.cpu().double() @ Hn.cpu().double().t()
    assert (G.cpu() - ref).abs().max().item() <= 1e-9 * ref.abs().max().item()
    a0 = torch.full((65,), 1.0 / 65, dtype=torch.float64)
    al, v, c = ops.foolsgold_weights(G, a0.to(gpu), 1.0)
    ral, rv, rc = C.foolsgold_weights(G.cpu(), a0, 1.0)
    assert al.is_cuda and (al.cpu() - ral).abs().max().item() <= 1e-9 and (c.cpu() - rc).abs().max().item() <= 1e-9
    res = agg.foolsgold(U.to(gpu), None, g.to(gpu), H.to(gpu), 1.0)
    ref = R.result_loop(U, g, None, R.foolsgold_loop(H + (U - g[None]), 1.0)[0])
    assert R.close(res.params.cpu(), ref, 1e-6)


# ---------------------------------------------------------------------------------- k_foolsgold_weights
@pytest.mark.parametrize("n", WEIGHT_NS)
def test_foolsgold_weights_match_composite_on_device_gram(gpu, n):
    f = {1: 0, 2: 0, 3: 1, 8: 2, 33: 8, 64: 16}[n]
    rows, sizes = R.reference(n, f, 1025)
    a0 = (sizes.double() / sizes.double().sum())
    worst = 0.0
    for _, _, _, H_new, _, _, _ in rows:
        G = ops.gram_anchored(H_new.to(gpu), torch.zeros(1025, device=gpu))
        for kappa in (0.5, 1.0, 2.0):
            al, v, c = ops.foolsgold_weights(G, a0.to(gpu), kappa)
            ral, rv, rc = C.foolsgold_weights(G.cpu(), a0, kappa)
            assert al.is_cuda and al.dtype == torch.float64 and al.shape == (n,) and c.shape == (n,)
            errs = [(x.cpu() - y).abs().max().item() for x, y in ((al, ral), (v, rv), (c, rc))]
            worst = max(worst, *errs)
            assert max(errs) <= 1e-9, (kappa, errs)
            again = ops.foolsgold_weights(G, a0.to(gpu), kappa)
            assert all(torch.equal(x, y) for x, y in zip(again, (al, v, c)))
    print(f"foolsgold_weights n={n}: worst difference {worst:.3e}")


def test_foolsgold_weights_degenerate_grams(gpu):
    """Every history parallel (alpha = 0), a zero row (cosine 0, not NaN), orthogonal rows (alpha = 1)."""
    a0 = torch.full((8,), 0.125, dtype=torch.float64, device=gpu)
    x = torch.tensor([1.0, -2.0, 0.5, 3.0, -1.0, 2.0, 4.0, -0.25], dtype=torch.float64, device=gpu)
    al, v, c = ops.foolsgold_weights(x[:, None] * x[None, :], a0, 1.0)
    assert al.tolist() == [0.0] * 8 and c.tolist() == [0.0] * 8 and v.tolist() == [1.0] * 8
    G = torch.eye(8, dtype=torch.float64, device=gpu)
    al, v, c = ops.foolsgold_weights(G, a0, 1.0)
    assert al.tolist() == [1.0] * 8 and v.tolist() == [0.0] * 8 and torch.equal(c, a0)
    G[3, 3] = 0.0
    al, v, _ = ops.foolsgold_weights(G, a0, 1.0)
    ral, rv, _ = C.foolsgold_weights(G.cpu(), a0.cpu(), 1.0)
    assert bool(torch.isfinite(al).all()) and torch.equal(al.cpu(), ral) and torch.equal(v.cpu(), rv)


# ---------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("n,f,P", R.CASES)
def test_foolsgold_matches_parameter_space_loop(gpu, n, f, P):
    rows, sizes = R.reference(n, f, P)
    R.check_conditions(n, f, P, rows)
    H, count = None, torch.zeros((), dtype=torch.int64, device=gpu)
    for U, g, H_old, H_new, alpha, v, ref in rows:
        Ud, gd = U.to(gpu), g.to(gpu)
        res = agg.foolsgold(Ud, sizes, gd, H, 1.0, rounds=count)
        got = res.info["history"]
        assert res.params.is_cuda and res.params.dtype == torch.float32 and got.is_cuda
        assert torch.equal(bits(got), bits(H_new))
        assert all(res.info[k].is_cuda for k in ("alpha", "max_cos", "rounds"))  # (device values until host_info)
        assert (res.info["alpha"].cpu() - torch.tensor(alpha, dtype=torch.float64)).abs().max().item() <= 1e-9
        assert (res.info["max_cos"].cpu() - torch.tensor(v, dtype=torch.float64)).abs().max().item() <= 1e-9
        assert R.close(res.params.cpu(), ref, 1e-6)
        ptrs = {t.untyped_storage().data_ptr() for t in (Ud, gd) + (() if H is None else (H,))}
        assert res.params.untyped_storage().data_ptr() not in ptrs and got.untyped_storage().data_ptr() not in ptrs
        # two identical calls give identical bits; device sizes (the several-rank path) too
        again = agg.foolsgold(Ud, sizes, gd, H, 1.0, rounds=count)
        dev = agg.foolsgold(Ud, sizes.to(gpu), gd, H, 1.0, rounds=count)
        for other in (again, dev):
            assert torch.equal(other.params, res.params) and torch.equal(other.info["alpha"], res.info["alpha"])
            assert torch.equal(other.info["history"], got)
        H, count = got, res.info["rounds"]
    info = agg.host_info({k: x for k, x in res.info.items() if k != "history"})
    assert info["rounds"] == len(rows) and len(info["alpha"]) == n == len(info["max_cos"])


def test_no_centre_and_enable_on_the_device(gpu):
    rows, sizes = R.reference(8, 2, 1025)
    U, g, H_old, H_new, _, _, _ = rows[1]
    Ud, gd, Hd = U.to(gpu), g.to(gpu), H_old.to(gpu)
    res = agg.foolsgold(Ud, sizes, None, Hd, 1.0, rounds=1)
    assert torch.equal(res.params, ops.fedavg(Ud, sizes)) and res.info["history"] is Hd
    assert res.info["alpha"].tolist() == [1.0] * 8 and int(res.info["rounds"]) == 1
    off = torch.zeros(1, dtype=torch.int32, device=gpu)
    res = agg.foolsgold(Ud, sizes, gd, Hd, 1.0, enable=off, rounds=1)
    assert torch.equal(bits(res.info["history"]), bits(H_old)) and int(res.info["rounds"]) == 1
    on = torch.ones(1, dtype=torch.int32, device=gpu)
    res = agg.foolsgold(Ud, sizes, gd, Hd, 1.0, enable=on, rounds=1)
    assert torch.equal(bits(res.info["history"]), bits(H_new)) and int(res.info["rounds"]) == 2


def test_bad_arguments_are_refused(gpu):
    nat = ops.native()
    U, g, H = (t.to(gpu) for t in make_hist(8, 100))
    en = torch.ones(1, dtype=torch.int32, device=gpu)
    out = torch.empty_like(H)
    a8 = torch.full((8,), 0.125, dtype=torch.float64, device=gpu)
    G = torch.eye(8, dtype=torch.float64, device=gpu)
    with pytest.raises(RuntimeError):  # n = 65
        z = torch.zeros(65, 100, device=gpu)
        nat.hist_gram(z, g, z.clone(), en, z.clone())
    with pytest.raises(RuntimeError):  # the history written over itself
        nat.hist_gram(U, g, H, en, H)
    with pytest.raises(RuntimeError):  # a centre of the wrong length
        nat.hist_gram(U, g[:99].contiguous(), H, en, out)
    with pytest.raises(RuntimeError):  # a history of another shape
        nat.hist_gram(U, g, H[:7].contiguous(), en, out)
    with pytest.raises(RuntimeError):
        nat.hist_gram(U, g, H, en, out[:7].contiguous())
    with pytest.raises(RuntimeError):  # host tensors never reach a launch
        nat.hist_gram(U, g, H, en.cpu(), out)
    with pytest.raises(RuntimeError):
        nat.foolsgold_weights(torch.eye(65, dtype=torch.float64, device=gpu),
                              torch.full((65,), 1.0 / 65, dtype=torch.float64, device=gpu), 1.0)
    with pytest.raises(RuntimeError):
        nat.foolsgold_weights(G, a8[:7].contiguous(), 1.0)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError):
            nat.foolsgold_weights(G, a8, bad)


# ---------------------------------------------------------------------------------- engine
def _engine(tmp_path, sub, spec, fault):
    d = {
        "server": {"num-round": 4, "clients": 5, "mode": "foolsgold", "model": "TransformerModel", "data-name": "ICU",
                   "genuine-rate": 1.0, "random-seed": 11, "data-distribution": {"num-data-range": [300, 500]}},
        "learning": {"epoch": 2, "batch-size": 128},
        "data": {"synthetic": True, "train-size": 4000, "test-size": 1000},
        "engine": {"checkpoint-dir": str(tmp_path / sub), "trainer": "auto", "seed": 3, "speculative": spec,
                   "fault-inject": [{"client": 1, "round": 3}] if fault else []},
        "log_path": str(tmp_path / sub),
    }
    cfg = from_dict(d)
    return FLEngine(cfg, device="cuda", table=build_client_table(cfg, 1, parse_attackers("4:Min-Max:2")),
                    verbose=False)


@pytest.mark.parametrize("fault", [False, True])
def test_early_launch_matches_serial_schedule(gpu, tmp_path, fault):
    """5 clients, one Min-Max attacker from round 2, fused trainer: the early launch (server step and next launch before
    the host knows the round's outcome, the device deciding whether the history advances) gives the serial schedule's
    rounds, checkpoints, history and count of rounds bit for bit, also when a client fails in round 3."""
    def run(spec, sub):
        eng = _engine(tmp_path, sub, spec, fault)
        assert eng._speculative == spec and eng.trainer.kind == "fused"
        seen = R._capture(eng)
        hist = eng.run()
        assert not spec or any(r.get("path") == "early-launch" for r in hist)
        H, count, g = eng.server.history.detach().cpu().clone(), int(eng.server.rounds), eng.global_params.detach().cpu().clone()
        eng.close()
        ck = torch.load(os.path.join(tmp_path, sub, "TransformerModel.pth"), weights_only=True)
        return [(r["ok"], None if r["metric"] != r["metric"] else r["metric"], r.get("alpha")) for r in hist], \
            H, count, g, ck, seen

    h0, H0, n0, g0, ck0, seen0 = run(False, "serial")
    h1, H1, n1, g1, ck1, _ = run(True, "spec")
    assert [ok for ok, _, _ in h0] == ([True, True, False, True, True] if fault else [True] * 4)
    assert h0 == h1 and n0 == n1 == 3
    assert torch.equal(bits(H0), bits(H1)) and torch.equal(g0, g1)
    assert list(ck0) == list(ck1) and all(torch.equal(ck0[k], ck1[k]) for k in ck0)
    # the serial run's history is the sum over its successful rounds of (row - START), in the torch expression's bits
    H = torch.zeros_like(H0)
    for U, g in seen0:
        if g is not None:
            H = H + (U.cpu() - g.cpu()[None])
    assert bool(H.any()) and torch.equal(bits(H0), bits(H))
    assert all(a is not None and len(a) == 5 for ok, _, a in h0 if ok)
