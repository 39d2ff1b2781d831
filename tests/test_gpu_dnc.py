"""DnC on the device: ``k_dnc_gram`` against the fp64 composite (and, on all columns, against the independent
``centred_gram`` kernel), ``k_dnc_select`` against the composite on the device's own Grams, the tie / NaN / empty
rules, bit reproducibility, ``k_top_pc`` unchanged by the shared Jacobi body (values recorded from the commit before
it, tests/golden/top_pc_parent.pt), the aggregate, and the engine (captured rounds; early launch against serial).

Bounds.  Gram: 1e-9 max diag(G_ref), the project's fp64 distance standard (worst-case accumulation error
b 2^-53 <= 1.2e-12 for b <= 1e4).  Scores: 1e-9 lambda_1 on the device's own G (with lambda_1 / lambda_2 >= 4 the
eigenvector perturbation bound at n = 64 is under 3e-10 lambda_1).  Aggregate: 1e-6 max(1, |ref|_inf), multi_krum's."""
import os

import pytest
import torch

import test_dnc as R
from attackfl_amd import agg, ops
from attackfl_amd.config import from_dict
from attackfl_amd.fl.engine import EARLY_AGGREGATORS, FLEngine, build_client_table
from attackfl_amd.ops import composite as C
from launch import parse_attackers

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "top_pc_parent.pt")


def rows(n, P, seed=0):
    g = torch.Generator().manual_seed(7000 * n + P + seed)
    return 0.3 * torch.randn(1, P, generator=g) + 0.01 * torch.randn(n, P, generator=g)


def gram_err(got, ref):
    scale = ref.diagonal(dim1=-2, dim2=-1).max().item()
    return (got.cpu() - ref).abs().max().item() / max(scale, 1e-300)


# ---------------------------------------------------------------------------------- Gram
@pytest.mark.parametrize("n", [1, 2, 3, 8, 17, 33, 64])
def test_gram_matches_composite(gpu, n):
    worst = 0.0
    for P in (1, 63, 1025, 4099):
        U = rows(n, P)
        Ud = U.to(gpu)
        for b in (1, 16, 1023, 1024, 1025, P, P + 7):
            for iters in (1, 3):
                ref = C.dnc_gram(U, b, iters, R.SEED)
                got = ops.dnc_gram(Ud, b, iters, R.SEED)
                assert got.shape == (iters, n, n) and got.dtype == torch.float64
                if n == 1:  # one row: centred on itself
                    assert not bool(ref.any()) and not bool(got.any())
                    continue
                err = gram_err(got, ref)
                worst = max(worst, err)
                assert err <= 1e-9, (n, P, b, iters, err)
                assert torch.equal(got, got.transpose(1, 2))
            if b >= P and n > 1 and P > 1:  # all columns: the independent Gram kernel
                assert gram_err(ops.dnc_gram(Ud, b, 1, R.SEED)[0], ops.centred_gram(Ud).cpu()) <= 1e-9
    print(f"dnc_gram n={n}: worst error {worst:.3e} max diag")


def test_gram_non_contiguous_view_and_seed(gpu):
    base = rows(8, 2 * 1025).to(gpu)
    view = base[:, ::2]
    assert not view.is_contiguous()
    ref = C.dnc_gram(view.cpu(), 257, 3, R.SEED)
    assert gram_err(ops.dnc_gram(view, 257, 3, R.SEED), ref) <= 1e-9
    assert gram_err(ops.dnc_gram(base.t()[:1025].t(), 257, 3, R.SEED), C.dnc_gram(base[:, :1025].cpu(), 257, 3, R.SEED)) <= 1e-9
    big = (1 << 63) + 12345  # a seed with the top bit set reaches the kernel unchanged
    U = rows(8, 1025)
    assert gram_err(ops.dnc_gram(U.to(gpu), 100, 2, big), C.dnc_gram(U, 100, 2, big)) <= 1e-9
    assert not torch.equal(ops.dnc_gram(U.to(gpu), 100, 1, 1), ops.dnc_gram(U.to(gpu), 100, 1, 2))
    for bad in ((0, 1), (1, 0)):  # the launcher refuses instead of launching
        with pytest.raises(RuntimeError):
            ops.dnc_gram(U.to(gpu), bad[0], bad[1], 0)
    with pytest.raises(RuntimeError):
        ops.native().dnc_run(torch.zeros(65, 8, device=gpu), 4, 1, 0, 0, torch.ones(65, dtype=torch.float64, device=gpu),
                             False)
    with pytest.raises(RuntimeError):
        ops.native().dnc_run(U.to(gpu), 4, 1, 0, 8, torch.ones(8, dtype=torch.float64, device=gpu), False)


# ---------------------------------------------------------------------------------- scores and selection
@pytest.mark.parametrize("n,f,P,b", R.SHAPES)
def test_scores_match_composite_on_device_gram(gpu, n, f, P, b):
    U, sizes, ref, lam = R.reference(n, f, P, b)  # (asserts the gaps on the fp64 reference)
    Ud = U.to(gpu)
    G = ops.dnc_gram(Ud, b, R.ITERS, R.SEED)
    assert gram_err(G, C.dnc_gram(U, b, R.ITERS, R.SEED)) <= 1e-9
    keep, scores, w = ops.dnc_select(G, f, sizes)
    ck, cs, cw = C.dnc_select(G.cpu(), f, sizes)
    ratio = ((scores.cpu() - cs).abs().max(dim=1).values / lam).max().item()
    print(f"dnc_select n={n} P={P} b={b}: scores within {ratio:.3e} lambda_1 of the composite")
    assert ratio <= 1e-9
    want = torch.arange(n) < n - f
    assert torch.equal(keep.cpu(), ck) and torch.equal(ck, want)
    assert (w.cpu() - cw).abs().max().item() <= 1e-14
    # the two-launch form (partials straight into the select kernel) is the same computation, bit for bit
    k2, s2, w2 = ops.dnc_filter(Ud, b, R.ITERS, R.SEED, f, sizes)
    assert torch.equal(k2, keep) and torch.equal(s2, scores) and torch.equal(w2, w)
    k1, s1, _ = ops.dnc_filter(Ud, b, 1, R.SEED, f, sizes)
    assert torch.equal(k1.cpu(), want) and torch.equal(s1[0], scores[0])


def test_tie_rule_and_nan(gpu):
    R.check_ties_and_nan(gpu)


def test_empty_intersection_keeps_every_row(gpu):
    R.check_empty_intersection(gpu)


def test_bit_reproducible(gpu):
    U, sizes, _, _ = R.reference(33, 8, 2049, 1025)
    Ud = U.to(gpu)
    a = agg.dnc(Ud, sizes, byz_f=8, dnc_iters=3, dnc_sub_dim=1025, seed=R.SEED)
    b = agg.dnc(Ud, sizes.to(gpu), byz_f=8, dnc_iters=3, dnc_sub_dim=1025, seed=R.SEED)  # (the several-rank path)
    assert torch.equal(a.params, b.params) and torch.equal(a.info["scores"], b.info["scores"])
    assert torch.equal(a.info["selected"], b.info["selected"])
    assert torch.equal(ops.dnc_gram(Ud, 1025, 3, R.SEED), ops.dnc_gram(Ud, 1025, 3, R.SEED))


# ---------------------------------------------------------------------------------- k_top_pc unchanged
def test_top_pc_bits_unchanged(gpu):
    gold = torch.load(GOLDEN, weights_only=True)
    for n in (8, 33):
        for sweeps in (12, 2):
            z = ops.top_pc(gold[f"G{n}"].to(gpu), sweeps).cpu()
            assert torch.equal(z, gold[f"z{n}_s{sweeps}"]), (n, sweeps)


# ---------------------------------------------------------------------------------- aggregate
@pytest.mark.parametrize("n,f,P,b", [s for s in R.SHAPES if s[0] >= 2 * s[1] + 3])
def test_aggregate_matches_composite(gpu, n, f, P, b):
    U, sizes, _, _ = R.reference(n, f, P, b)
    ref = agg.dnc(U, sizes, byz_f=f, dnc_iters=R.ITERS, dnc_sub_dim=b, seed=R.SEED)
    Ud = U.to(gpu)
    res = agg.dnc(Ud, sizes, byz_f=f, dnc_iters=R.ITERS, dnc_sub_dim=b, seed=R.SEED)
    assert torch.equal(res.info["selected"].cpu(), ref.info["selected"]) and res.info["drop"] == f
    assert not bool(res.info["selected"][n - f:].any())
    err = (res.params.double().cpu() - ref.params.double()).abs().max().item()
    assert err <= 1e-6 * max(1.0, ref.params.abs().max().item())
    assert res.params.untyped_storage().data_ptr() != Ud.untyped_storage().data_ptr()
    zero = agg.dnc(Ud, sizes, byz_f=0)  # drop = 0 is FedAvg itself
    assert torch.equal(zero.params, ops.fedavg(Ud, sizes))


# ---------------------------------------------------------------------------------- engine
def _engine(tmp_path, rounds, sub, **engine_kw):
    d = {
        "server": {"num-round": rounds, "clients": 7, "mode": "dnc", "model": "TransformerModel", "data-name": "ICU",
                   "genuine-rate": 1.0, "random-seed": 11, "data-distribution": {"num-data-range": [300, 500]}},
        "learning": {"epoch": 2, "batch-size": 128},
        "data": {"synthetic": True, "train-size": 4000, "test-size": 1000},
        "engine": {"checkpoint-dir": str(tmp_path / sub), "trainer": "auto", "seed": 3, "dnc-iters": 2, **engine_kw},
        "log_path": str(tmp_path / sub),
    }
    cfg = from_dict(d)
    return FLEngine(cfg, device="cuda", table=build_client_table(cfg, 1, parse_attackers("6:Min-Max:2")),
                    verbose=False)


def test_engine_rounds_match_composite(gpu, tmp_path, monkeypatch):
    """7 clients, f auto (= 1), one Min-Max attacker from round 2, fused trainer: every round's device aggregate and
    mask against the CPU composite on the captured rows; the rule runs in the early launch."""
    eng = _engine(tmp_path, 3, "e2e")
    assert eng.trainer.kind == "fused" and "dnc" in EARLY_AGGREGATORS
    seen = []
    orig_fn = agg.AGGREGATORS["dnc"]

    def capture(U, sizes, **kw):
        rows_ = U.detach().cpu().clone()
        res = orig_fn(U, sizes, **kw)
        seen.append((rows_, sizes.detach().cpu().clone(), res.params.detach().cpu().clone(), kw))
        return res

    monkeypatch.setitem(agg.AGGREGATORS, "dnc", capture)
    hist = eng.run()
    eng.close()
    assert [r["ok"] for r in hist] == [True, True, True] and len(seen) == 3
    assert any(r.get("path") == "early-launch" for r in hist)
    assert all(0.0 <= r["metric"] <= 1.0 for r in hist)
    assert "attack" in hist[1] and "attack" in hist[2]
    for k, (rows_, sizes, got, kw) in enumerate(seen):
        assert (kw["byz_f"], kw["dnc_iters"], kw["dnc_sub_dim"], kw["dnc_c"]) == ("auto", 2, 10000, 1.0)
        ref = orig_fn(rows_, sizes, **kw)
        assert (got.double() - ref.params.double()).abs().max().item() <= 1e-6 * max(1.0, ref.params.abs().max().item())
        assert hist[k]["f"] == 1 and hist[k]["drop"] == 1
        assert hist[k]["selected"] == torch.nonzero(ref.info["selected"]).reshape(-1).tolist(), k


def test_early_launch_matches_serial_schedule(gpu, tmp_path):
    def run(spec, sub):
        eng = _engine(tmp_path, 4, sub, speculative=spec)
        assert eng._speculative == spec
        hist = eng.run()
        out = eng.global_params.detach().cpu().clone()
        assert not spec or any(r.get("path") == "early-launch" for r in hist)
        eng.close()
        return [(r["ok"], r["metric"]) for r in hist], out

    h0, p0 = run(False, "serial")
    h1, p1 = run(True, "spec")
    assert len(h0) == 4 and all(ok for ok, _ in h0)
    assert h0 == h1
    assert torch.equal(p0, p1)
