"""Centred clipping on the device: the anchored fp64-MFMA Gram against ``(U - a)(U - a)^T`` in fp64, ``k_cclip_weights``
against the composite on the device's own Gram, ``agg.cclip`` (Gram pass, weights, ``k_anchored_rows``) against the
parameter-space loop of tests/test_cclip.py, bit reproducibility, non-finite rows, refused arguments, and the engine
(captured rounds against the composite; the early launch against the serial schedule).

Bounds.  Gram: 1e-9 max |G|, the bound tests/test_gpu_dnc.py holds the same pass to (worst-case accumulation error
P 2^-53 <= 5.3e-12 at P = 47693).  Coefficients: 1e-9 absolute on c in [0, 1]; the one cancellation is
G_ii - 2 (G c)_i + c^T G c, about 1e3 : 1 for these rows, so fp64 leaves orders of margin.  Worst values seen on an
MI355X: Gram 4.1e-15 max |G| (n = 48, P = 2049); coefficients 1.1e-16 (n <= 3), 5.6e-17 at n = 8, 1.4e-17 at n = 64."""
import pytest
import torch

import test_cclip as R
from attackfl_amd import agg, ops
from attackfl_amd.config import from_dict
from attackfl_amd.fl.engine import EARLY_AGGREGATORS, FLEngine, build_client_table
from attackfl_amd.ops import composite as C
from launch import parse_attackers

pytestmark = pytest.mark.gpu

GRAM_SHAPES = [(1, 7), (3, 7), (16, 1024), (17, 1025), (33, 100), (48, 2049), (64, 1000)]
WEIGHT_NS = [1, 2, 3, 8, 33, 64]


def close(got, ref, tol):
    return (got.double().cpu() - ref.double()).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


def gram_err(got, ref):
    return (got.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


def alpha_of(sizes):
    return sizes.double() / sizes.double().sum()


# ---------------------------------------------------------------------------------- anchored Gram
@pytest.mark.parametrize("n,P", GRAM_SHAPES)
def test_gram_anchored_matches_fp64(gpu, n, P):
    U, _, centre = R.make_rows(n, P)
    Y = U.double() - centre.double()[None, :]
    ref = Y @ Y.t()
    got = ops.gram_anchored(U.to(gpu), centre.to(gpu))
    assert got.shape == (n, n) and got.dtype == torch.float64
    err = gram_err(got, ref)
    print(f"gram_anchored n={n} P={P}: error {err:.3e} max |G|")
    assert err <= 1e-9
    assert torch.equal(got, got.t()) and torch.equal(got, ops.gram_anchored(U.to(gpu), centre.to(gpu)))
    assert gram_err(got, C.gram_anchored(U, centre)) <= 1e-9


@pytest.mark.parametrize("n,P,bad", [(3, 7, 0), (17, 1025, 16), (33, 100, 5), (64, 1000, 63)])
def test_gram_anchored_nan_row_poisons_its_own_row_and_column(gpu, n, P, bad):
    U, _, centre = R.make_rows(n, P)
    clean = ops.gram_anchored(U.to(gpu), centre.to(gpu)).cpu()
    U = U.clone()
    U[bad] = float("nan")
    got = ops.gram_anchored(U.to(gpu), centre.to(gpu)).cpu()
    mask = torch.zeros(n, n, dtype=torch.bool)
    mask[bad, :] = True
    mask[:, bad] = True
    assert bool(torch.isnan(got[mask]).all())
    assert torch.equal(got[~mask], clean[~mask])


def test_existing_gram_callers_are_reproducible(gpu):
    """The centre argument is optional: ``centred_gram`` and ``pairwise_sqdist`` go through the same kernel without it
    (their own suites hold their values); two calls give the same bits, with an anchored pass in between."""
    for n, P in ((3, 7), (17, 1025), (64, 1000)):
        U, _, centre = R.make_rows(n, P)
        Ud = U.to(gpu)
        g0, d0 = ops.centred_gram(Ud), ops.pairwise_sqdist(Ud)
        ops.gram_anchored(Ud, centre.to(gpu))
        assert torch.equal(ops.centred_gram(Ud), g0) and torch.equal(ops.pairwise_sqdist(Ud), d0)
        assert gram_err(g0, C.centred_gram(U)) <= 1e-9
        assert gram_err(d0, C.pairwise_l2(U) ** 2) <= 1e-9


# ---------------------------------------------------------------------------------- k_cclip_weights
def check_weights(G, alpha, c0, iters, tau):
    """The kernel against the composite on the same (device-made) Gram -> the worst coefficient difference."""
    c, t, clipped, fin = ops.cclip_weights(G, alpha, c0, iters, tau)
    rc, rt, rclipped, rfin = C.cclip_weights(G.cpu(), alpha.cpu(), c0.cpu(), iters, 0.0 if tau == "auto" else tau)
    assert c.dtype == torch.float64 and c.is_cuda and t.is_cuda and clipped.is_cuda
    err = (c.cpu() - rc).abs().max().item()
    assert err <= 1e-9, (iters, tau, err)
    assert bool((c >= 0).all()) and bool((c <= 1.0 + 1e-15).all())
    assert abs(float(t) - float(rt)) <= 1e-12 * abs(float(rt)), (iters, tau, float(t), float(rt))
    assert int(clipped) == int(rclipped), (iters, tau)
    assert int(fin) == int(rfin)
    c2, t2, clipped2, _ = ops.cclip_weights(G, alpha, c0, iters, tau)
    assert torch.equal(c2, c) and float(t2) == float(t) and int(clipped2) == int(clipped)
    return err


@pytest.mark.parametrize("n", WEIGHT_NS)
def test_cclip_weights_match_composite_on_device_gram(gpu, n):
    U, sizes, centre = R.make_rows(n, 1000)
    Ud, alpha = U.to(gpu), alpha_of(sizes).to(gpu)
    worst = 0.0
    for G, c0 in ((ops.gram_anchored(Ud, centre.to(gpu)), torch.zeros_like(alpha)), (ops.centred_gram(Ud), alpha)):
        for iters in R.ITERS:
            for tau in R.TAUS:
                worst = max(worst, check_weights(G, alpha, c0, iters, tau))
    print(f"cclip_weights n={n}: worst coefficient difference {worst:.3e}")


def test_cclip_weights_tied_distances_and_zero_radius(gpu):
    U, sizes, centre = R.make_rows(8, 1000)
    alpha, g = alpha_of(sizes).to(gpu), centre.to(gpu)
    tied = U.clone()
    for r in (1, 2, 3):
        tied[r] = tied[0]  # four identical rows: the lower median falls among their equal distances
    G = ops.gram_anchored(tied.to(gpu), g)
    for iters in R.ITERS:
        check_weights(G, alpha, torch.zeros_like(alpha), iters, "auto")
    c, t, clipped, _ = ops.cclip_weights(G, alpha, torch.zeros_like(alpha), 1, "auto")
    assert float(t) == float(G[0, 0].sqrt()) and int(clipped) <= 4
    assert float(c[0] / alpha[0]) == float(c[1] / alpha[1]) == 1.0  # (s = 1 on the tied rows)
    zero = U.clone()
    for r in range(5):
        zero[r] = centre  # a majority of rows equal to the centre: tau = 0, the others get s = 0
    G = ops.gram_anchored(zero.to(gpu), g)
    for iters in R.ITERS:
        check_weights(G, alpha, torch.zeros_like(alpha), iters, "auto")
        c, t, clipped, _ = ops.cclip_weights(G, alpha, torch.zeros_like(alpha), iters, "auto")
        assert float(t) == 0.0 and int(clipped) == 3 and c[5:].tolist() == [0.0, 0.0, 0.0]
        assert bool(torch.isfinite(c).all())
    res = agg.cclip(zero.to(gpu), sizes, centre=g)
    assert torch.equal(res.params, g)


# ---------------------------------------------------------------------------------- the rule
_REF = {}


def reference(n, P, iters, tau, anchored):
    key = (n, P, iters, tau, anchored)
    if key not in _REF:
        U, sizes, centre = R.rows_of(n, P)
        _REF[key] = R.cclip_param_space(U, sizes, centre if anchored else None, iters, tau)
    return _REF[key]


@pytest.mark.parametrize("anchored", [True, False])
@pytest.mark.parametrize("n,P", R.SHAPES)
def test_cclip_matches_parameter_space_loop(gpu, n, P, anchored):
    U, sizes, centre = R.rows_of(n, P)
    Ud = U.to(gpu)
    g = centre.to(gpu) if anchored else None
    for iters in R.ITERS:
        for tau in R.TAUS:
            ref, t, clipped, _ = reference(n, P, iters, tau, anchored)
            res = agg.cclip(Ud, sizes, centre=g, cclip_iters=iters, cclip_tau=tau)
            assert res.params.dtype == torch.float32 and res.params.is_cuda
            assert close(res.params, ref, 1e-6), (iters, tau)
            assert float(res.info["tau"]) == pytest.approx(t, rel=1e-9)
            if iters == 1:
                assert int(res.info["clipped"]) == clipped
            # never a row of U, never the centre
            assert res.params.untyped_storage().data_ptr() != Ud.untyped_storage().data_ptr()
            assert not anchored or res.params.untyped_storage().data_ptr() != g.untyped_storage().data_ptr()
            again = agg.cclip(Ud, sizes, centre=g, cclip_iters=iters, cclip_tau=tau)
            assert torch.equal(again.params, res.params) and torch.equal(again.info["weights"], res.info["weights"])
            dev = agg.cclip(Ud, sizes.to(gpu), centre=g, cclip_iters=iters, cclip_tau=tau)  # (the several-rank path)
            assert torch.equal(dev.params, res.params) and torch.equal(dev.info["weights"], res.info["weights"])


def test_both_branches_on_the_device(gpu):
    U, sizes, centre = R.rows_of(8, 47693)
    res = agg.cclip(U.to(gpu), sizes, centre=centre.to(gpu), cclip_iters=1, cclip_tau="auto")
    assert int(res.info["clipped"]) == 4
    info = agg.host_info(res.info)
    assert len(info["weights"]) == 8 and info["tau"] > 0.0 and info["clipped"] == 4 and info["iters"] == 1


@pytest.mark.parametrize("tau", R.TAUS)
@pytest.mark.parametrize("bad", [0, 3, 7])
def test_nan_row_with_a_centre_is_left_out(gpu, bad, tau):
    U, sizes, centre = R.rows_of(8, 257)
    U = U.clone()
    U[bad] = float("nan")
    res = agg.cclip(U.to(gpu), sizes, centre=centre.to(gpu), cclip_iters=3, cclip_tau=tau)
    ref, t, _, _ = R.cclip_param_space(U, sizes, centre, 3, tau, skip=(bad,))
    assert bool(torch.isfinite(res.params).all()) and close(res.params, ref, 1e-6)
    w = res.info["weights"]
    assert float(w[bad]) == 0.0 and bool(torch.isfinite(w).all())
    assert float(res.info["tau"]) == pytest.approx(t, rel=1e-9)


def test_all_nan_rows_and_no_centre(gpu):
    U, sizes, centre = R.rows_of(5, 257)
    g = centre.to(gpu)
    res = agg.cclip(torch.full_like(U, float("nan")).to(gpu), sizes, centre=g)
    assert torch.equal(res.params, g) and res.params.untyped_storage().data_ptr() != g.untyped_storage().data_ptr()
    assert res.info["weights"].tolist() == [0.0] * 5 and int(res.info["clipped"]) == 0
    U = U.clone()
    U[2] = float("nan")
    for tau in R.TAUS:
        assert not bool(torch.isfinite(agg.cclip(U.to(gpu), sizes, centre=None, cclip_tau=tau).params).any())


def test_bad_arguments_are_refused(gpu):
    nat = ops.native()
    U = torch.zeros(8, 100, device=gpu)
    a8 = torch.full((8,), 0.125, dtype=torch.float64, device=gpu)
    G = torch.eye(8, dtype=torch.float64, device=gpu)
    with pytest.raises(RuntimeError):  # n = 65
        nat.gram_anchored(torch.zeros(65, 100, device=gpu), torch.zeros(100, device=gpu))
    with pytest.raises(RuntimeError):
        nat.cclip_weights(torch.eye(65, dtype=torch.float64, device=gpu),
                          torch.full((65,), 1.0 / 65, dtype=torch.float64, device=gpu),
                          torch.zeros(65, dtype=torch.float64, device=gpu), 3, 0.0)
    with pytest.raises(RuntimeError):  # L = 0
        nat.cclip_weights(G, a8, torch.zeros_like(a8), 0, 1.0)
    with pytest.raises(RuntimeError):  # a NaN radius
        nat.cclip_weights(G, a8, torch.zeros_like(a8), 3, float("nan"))
    with pytest.raises(RuntimeError):  # alpha / c0 of the wrong length
        nat.cclip_weights(G, a8[:7].contiguous(), torch.zeros_like(a8), 3, 1.0)
    with pytest.raises(RuntimeError):  # an anchor of the wrong length
        nat.gram_anchored(U, torch.zeros(99, device=gpu))
    with pytest.raises(RuntimeError):
        nat.anchored_rows(U, a8, torch.zeros(101, device=gpu))
    with pytest.raises(RuntimeError):  # a c of the wrong length
        nat.anchored_rows(U, a8[:7].contiguous(), torch.zeros(100, device=gpu))
    with pytest.raises(RuntimeError):  # host tensors never reach a launch
        nat.anchored_rows(U, a8.cpu(), torch.zeros(100, device=gpu))


# ---------------------------------------------------------------------------------- engine
def _engine(tmp_path, rounds, sub, **engine_kw):
    d = {
        "server": {"num-round": rounds, "clients": 7, "mode": "cclip", "model": "TransformerModel", "data-name": "ICU",
                   "genuine-rate": 1.0, "random-seed": 11, "data-distribution": {"num-data-range": [300, 500]}},
        "learning": {"epoch": 2, "batch-size": 128},
        "data": {"synthetic": True, "train-size": 4000, "test-size": 1000},
        "engine": {"checkpoint-dir": str(tmp_path / sub), "trainer": "auto", "seed": 3, **engine_kw},
        "log_path": str(tmp_path / sub),
    }
    cfg = from_dict(d)
    return FLEngine(cfg, device="cuda", table=build_client_table(cfg, 1, parse_attackers("6:Min-Max:2")),
                    verbose=False)


def test_cclip_end_to_end(gpu, tmp_path, monkeypatch):
    """7 clients, one Min-Max attacker from round 2, fused trainer: every round's device aggregate against the CPU
    composite on the captured rows, sizes and centre; the rule runs in the early launch, and from round 2 on its
    centre is the previous round's global model."""
    eng = _engine(tmp_path, 3, "e2e")
    assert eng.trainer.kind == "fused" and "cclip" in EARLY_AGGREGATORS
    seen = []
    orig_fn = agg.AGGREGATORS["cclip"]

    def capture(U, sizes, **kw):
        rows = U.detach().cpu().clone()
        centre = kw["centre"].detach().cpu().clone() if kw.get("centre") is not None else None
        res = orig_fn(U, sizes, **kw)
        seen.append((rows, sizes.detach().cpu().clone(), centre, res.params.detach().cpu().clone(), kw))
        return res

    monkeypatch.setitem(agg.AGGREGATORS, "cclip", capture)
    hist = eng.run()
    eng.close()
    assert [r["ok"] for r in hist] == [True, True, True] and len(seen) == 3
    assert any(r.get("path") == "early-launch" for r in hist)
    assert all(0.0 <= r["metric"] <= 1.0 for r in hist)
    assert "attack" in hist[1] and "attack" in hist[2]
    for k, (rows, sizes, centre, got, kw) in enumerate(seen):
        assert kw["cclip_iters"] == 3 and kw["cclip_tau"] == "auto"
        if k >= 1:
            assert centre is not None and torch.equal(centre, seen[k - 1][3]), k
        ref = orig_fn(rows, sizes, **{**kw, "centre": centre})
        assert close(got, ref.params, 1e-6), k
        assert len(hist[k]["weights"]) == 7 and hist[k]["tau"] > 0.0 and hist[k]["iters"] == 3
        assert hist[k]["clipped"] == int(ref.info["clipped"]), k
        assert hist[k]["tau"] == pytest.approx(float(ref.info["tau"]), rel=1e-9)


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
