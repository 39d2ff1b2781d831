"""Pre-aggregation on the device: ``k_mix_rows`` against stacked ``weighted_rows`` calls (the same bits) and against the
fp64 loop of tests/test_preagg.py, ``k_nnm_weights`` against the composite on the device's own distances (equal),
``agg.nnm`` / ``agg.bucketing`` in front of median / Multi-Krum / the geometric median / centred clipping against the
same chain on the CPU, the composite path beyond 64 rows, bit reproducibility, and the engine (the early launch
against the serial schedule).

Bounds: those of tests/test_preagg.py (one fp32 rounding after an fp64 sum; the neighbour margin of 1e-6 of max D on
the fp64 reference) and, for the chains, the tolerances ``test_robust_modes_end_to_end`` holds the rules to: 1e-6 for
median and Multi-Krum, 2e-5 for geomed and cclip.  Where Multi-Krum selects, the gap between the last score taken and
the first left out is asserted on the CPU side (>= 1e-6 of the largest score) before the two selections are compared."""
import pytest
import torch

import test_preagg as R
from attackfl_amd import agg, ops
from attackfl_amd.config import from_dict
from attackfl_amd.fl.engine import EARLY_AGGREGATORS, FLEngine, build_client_table
from attackfl_amd.ops import composite as C
from launch import parse_attackers

pytestmark = pytest.mark.gpu

MIX_NS = [1, 8, 9, 16, 17, 32, 33, 64]
MIX_PS = [1, 255, 257, 1025]
CHAIN_SHAPES = [(8, 2, 257), (17, 4, 1025), (33, 7, 63), (64, 15, 1025)]
RULES = {"median": 1e-6, "multi_krum": 1e-6, "geomed": 2e-5, "cclip": 2e-5}


def make_w(R_, n, seed):
    """Dense fp64 weights with signs, a third of them exactly zero."""
    g = torch.Generator().manual_seed(1000 * n + R_ + seed)
    W = torch.randn(R_, n, generator=g, dtype=torch.float64)
    return W * (torch.rand(R_, n, generator=g) > 1.0 / 3.0)


def stacked(U, W):
    return torch.stack([ops.weighted_rows(U, W[r].contiguous()) for r in range(W.shape[0])])


def close(got, ref, tol):
    return (got.double().cpu() - ref.double().cpu()).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


# ---------------------------------------------------------------------------------- mix_rows
def check_mix(gpu, n, R_, P):
    U = R.make_rows(n, 0, P, False, seed=n)
    W = make_w(R_, n, P)
    Ud, Wd = U.to(gpu), W.to(gpu)
    Y = ops.mix_rows(Wd, Ud)
    assert Y.shape == (R_, P) and Y.dtype == torch.float32 and Y.is_cuda
    assert torch.equal(Y, stacked(Ud, Wd)), (n, R_, P)
    ref, bound = R.mix_fp64(W.tolist(), U)
    assert R.within(Y, ref, bound), (n, R_, P)
    assert torch.equal(Y, ops.mix_rows(Wd, Ud))


@pytest.mark.parametrize("n", MIX_NS)
def test_mix_rows_is_stacked_weighted_rows(gpu, n):
    for R_ in sorted({1, n, -(-n // 3)}):
        for P in MIX_PS:
            check_mix(gpu, n, R_, P)


def test_mix_rows_at_the_model_size(gpu):
    check_mix(gpu, 8, 8, 47693)


def test_mix_rows_sixty_four_mixed_rows_of_few(gpu):
    """R above n: more mixed rows than rows (no rule asks for it; the kernel's two bounds are independent)."""
    check_mix(gpu, 3, 64, 257)


@pytest.mark.parametrize("n,R_,P", [(8, 8, 257), (17, 6, 1025), (64, 64, 255)])
def test_mix_rows_zero_rows_and_columns(gpu, n, R_, P):
    U = R.make_rows(n, 0, P, False, seed=3).to(gpu)
    W = make_w(R_, n, 1)
    W[R_ // 2] = 0.0
    W[:, n // 2] = 0.0
    W[:, n - 1] = 0.0
    Wd = W.to(gpu)
    Y = ops.mix_rows(Wd, U)
    assert torch.equal(Y, stacked(U, Wd))
    assert not bool(Y[R_ // 2].any()) and not bool(torch.signbit(Y[R_ // 2]).any())  # (+0.0, as weighted_rows)
    # a zero weight still multiplies its row: a non-finite row poisons every mixed row, as in weighted_rows
    U2 = U.clone()
    U2[n // 2, 0] = float("nan")
    Y2 = ops.mix_rows(Wd, U2)
    assert bool(torch.isnan(Y2[:, 0]).all()) and torch.equal(Y2[:, 1:], Y[:, 1:])
    assert bool(torch.isnan(stacked(U2, Wd)[:, 0]).all())


def test_mix_rows_non_contiguous_views(gpu):
    U = R.make_rows(17, 0, 1025, False, seed=5).to(gpu)
    W = make_w(6, 17, 2).to(gpu)
    Ut = U.t().contiguous().t()  # [17, 1025] with strides (1, 17)
    Wt = W.t().contiguous().t()
    assert not Ut.is_contiguous() and not Wt.is_contiguous()
    assert torch.equal(ops.mix_rows(Wt, Ut), ops.mix_rows(W, U))
    assert torch.equal(ops.mix_rows(W.cpu(), U), ops.mix_rows(W, U))  # (host weights go up pinned)


def test_refused_arguments(gpu):
    nat = ops.native()
    U = torch.zeros(8, 100, device=gpu)
    W = torch.zeros(3, 8, dtype=torch.float64, device=gpu)
    with pytest.raises(RuntimeError):
        nat.mix_rows(W[:, :7].contiguous(), U)
    with pytest.raises(RuntimeError):
        nat.mix_rows(W.float(), U)
    with pytest.raises(RuntimeError):
        nat.mix_rows(W.cpu(), U)
    with pytest.raises(RuntimeError):
        nat.mix_rows(torch.zeros(65, 8, dtype=torch.float64, device=gpu), U)
    with pytest.raises(RuntimeError):
        nat.mix_rows(torch.zeros(1, 65, dtype=torch.float64, device=gpu), torch.zeros(65, 10, device=gpu))
    D = torch.zeros(8, 8, dtype=torch.float64, device=gpu)
    for f in (-1, 8):
        with pytest.raises(RuntimeError):
            nat.nnm_weights(D, f)
    with pytest.raises(RuntimeError):
        nat.nnm_weights(torch.zeros(65, 65, dtype=torch.float64, device=gpu), 1)


# ---------------------------------------------------------------------------------- nnm_weights
@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("n,f,P", R.SHAPES)
def test_nnm_weights_equal_the_composite(gpu, n, f, P, planted):
    U = R.rows_of(n, f, P, planted)
    Wref, margin, _ = R.nnm_param_space(U, f)
    print(f"nnm n={n} f={f} P={P} planted={planted}: margin {margin:.3e}")
    assert margin >= R.MARGIN
    D = ops.pairwise_sqdist(U.to(gpu))
    W, nbr = ops.nnm_weights(D, f)
    Wc, nbrc = C.nnm_weights(D, f)  # (the composite on the device's own distances)
    assert W.dtype == torch.float64 and nbr.dtype == torch.int64 and W.is_cuda
    assert torch.equal(W, Wc) and torch.equal(nbr, nbrc)
    assert torch.equal(W.cpu(), torch.as_tensor(Wref, dtype=torch.float64))


def test_nnm_weights_nan_and_ties(gpu):
    """A NaN distance ranks as +inf; equal distances fall to the lower index (all-equal rows: every distance 0)."""
    D = ops.pairwise_sqdist(R.rows_of(8, 2, 257, False).to(gpu)).clone()
    D[1, 5] = float("nan")
    D[0, 3] = float("nan")
    W, nbr = ops.nnm_weights(D, 2)
    Wc, nbrc = C.nnm_weights(D, 2)
    assert torch.equal(W, Wc) and torch.equal(nbr, nbrc) and float(W[1, 5]) == 0.0 and float(W[5, 1]) == 0.0
    Z = torch.zeros(64, 64, dtype=torch.float64, device=gpu)
    W, nbr = ops.nnm_weights(Z, 15)
    Wc, nbrc = C.nnm_weights(Z, 15)
    assert torch.equal(W, Wc) and torch.equal(nbr, nbrc)
    assert (W > 0).sum(dim=1).tolist() == [49] * 64 and bool((W[0, 1:49] > 0).all()) and float(W[63, 63]) == 1.0 / 49


# ---------------------------------------------------------------------------------- chains
def mk_gap(info):
    sc, keep = info["scores"], info["selected"]
    return float("inf") if bool(keep.all()) else float((sc[~keep].min() - sc[keep].max()) / sc.max())


def check_chain(gpu, pre, U, sizes, byz_f):
    """``pre`` then every rule of RULES on the device against the same chain on the CPU."""
    Yc, sc, ic = pre(U, sizes)
    Yd, sd, idv = pre(U.to(gpu), sizes)
    assert Yd.is_cuda and torch.equal(idv["weights"].cpu(), ic["weights"].cpu())
    ref, bound = R.mix_fp64(ic["weights"].tolist(), U)
    assert R.within(Yd, ref, bound) and R.within(Yc, ref, bound)
    assert torch.equal(torch.as_tensor(sd).cpu(), torch.as_tensor(sc))
    for rule, tol in RULES.items():
        want = agg.AGGREGATORS[rule](Yc, sc, byz_f=byz_f, seed=5, centre=None)
        got = agg.AGGREGATORS[rule](Yd, sd, byz_f=byz_f, seed=5, centre=None)
        assert got.params.is_cuda and close(got.params, want.params, tol), rule
        if rule == "multi_krum":
            gap = mk_gap(want.info)
            print(f"{ic['kind']} n={U.shape[0]} -> {Yc.shape[0]} rows: Multi-Krum score gap {gap:.3e}")
            assert gap >= 1e-6
            assert torch.equal(got.info["selected"].cpu(), want.info["selected"])


@pytest.mark.parametrize("n,f,P", CHAIN_SHAPES)
def test_nnm_then_rule(gpu, n, f, P):
    U = R.rows_of(n, f, P, True)
    _, margin, _ = R.nnm_param_space(U, f)
    assert margin >= R.MARGIN
    check_chain(gpu, lambda X, s: agg.nnm(X, s, f), U, R.make_sizes(n), f)


@pytest.mark.parametrize("n,f,P", CHAIN_SHAPES[1:])
def test_bucketing_then_rule(gpu, n, f, P):
    """Buckets of 2; the rule sees ceil(n / 2) rows and takes its f from them (``auto``)."""
    check_chain(gpu, lambda X, s: agg.bucketing(X, s, 2, 5), R.rows_of(n, f, P, True), R.make_sizes(n), "auto")


def test_bucketing_device_sizes(gpu):
    """``sizes`` on the device (the several-rank early launch): W and the size sums are built there."""
    U, sizes = R.rows_of(17, 4, 1025, True), R.make_sizes(17)
    Yc, sc, ic = agg.bucketing(U, sizes, 3, 9)
    Yd, sd, idv = agg.bucketing(U.to(gpu), sizes.to(gpu).double(), 3, 9)
    assert sd.is_cuda and idv["weights"].is_cuda and sd.dtype == torch.float64
    assert torch.equal(idv["weights"].cpu(), ic["weights"]) and torch.equal(sd.cpu(), sc.double())
    assert torch.equal(Yd, ops.mix_rows(ic["weights"], U.to(gpu)))


def test_sixty_five_rows_take_the_composite(gpu):
    n, f, P = 65, 15, 255
    U = R.make_rows(n, f, P, True)
    Wref, margin, _ = R.nnm_param_space(U, f)
    assert margin >= R.MARGIN
    Yd, _, info = agg.nnm(U.to(gpu), None, f)
    assert Yd.is_cuda and Yd.shape == (n, P) and info["rows"] == n
    assert torch.equal(info["weights"].cpu(), torch.as_tensor(Wref, dtype=torch.float64))
    ref, bound = R.mix_fp64(Wref, U)
    assert R.within(Yd, ref, bound)
    Yb, sb, ib = agg.bucketing(U.to(gpu), R.make_sizes(n), 1, 0)
    assert Yb.shape == (n, P) and ib["rows"] == n
    W = make_w(3, n, 0)
    assert R.within(ops.mix_rows(W.to(gpu), U.to(gpu)), *R.mix_fp64(W.tolist(), U))


def test_two_calls_give_the_same_bits(gpu):
    U = R.rows_of(33, 7, 63, True).to(gpu)
    sizes = R.make_sizes(33)
    for pre in (lambda: agg.nnm(U, sizes, 7), lambda: agg.bucketing(U, sizes, 2, 5)):
        (y0, _, i0), (y1, _, i1) = pre(), pre()
        assert torch.equal(y0, y1) and torch.equal(i0["weights"].cpu(), i1["weights"].cpu())
        assert y0.untyped_storage().data_ptr() != U.untyped_storage().data_ptr()


# ---------------------------------------------------------------------------------- engine
def _engine(tmp_path, mode, sub, **engine_kw):
    d = {
        "server": {"num-round": 3, "clients": 5, "mode": mode, "model": "TransformerModel", "data-name": "ICU",
                   "genuine-rate": 1.0, "random-seed": 11, "data-distribution": {"num-data-range": [300, 500]}},
        "learning": {"epoch": 2, "batch-size": 128},
        "data": {"synthetic": True, "train-size": 4000, "test-size": 1000},
        "engine": {"checkpoint-dir": str(tmp_path / sub), "trainer": "auto", "seed": 3, "byz-f": 1, "pre-agg": "nnm",
                   **engine_kw},
        "log_path": str(tmp_path / sub),
    }
    cfg = from_dict(d)
    return FLEngine(cfg, device="cuda", table=build_client_table(cfg, 1, parse_attackers("4:Min-Max:2")),
                    verbose=False)


@pytest.mark.parametrize("mode", ["multi_krum", "median"])
def test_engine_early_launch_matches_serial_schedule(gpu, tmp_path, mode):
    """5 clients, byz-f 1, NNM in front of the rule, one Min-Max attacker from round 2, fused trainer: the rule keeps
    launching early with pre-aggregation on, and the early schedule gives the serial schedule's rounds exactly."""
    assert mode in EARLY_AGGREGATORS

    def run(spec, sub):
        eng = _engine(tmp_path, mode, sub, speculative=spec)
        assert eng.trainer.kind == "fused" and eng._speculative == spec
        hist = eng.run()
        out = eng.global_params.detach().cpu().clone()
        assert not spec or any(r.get("path") == "early-launch" for r in hist)
        eng.close()
        for r in hist:
            p = r["pre_agg"]
            assert p["kind"] == "nnm" and p["f"] == 1 and p["rows"] == 5
            assert all(sorted(w) == [0.0, 0.25, 0.25, 0.25, 0.25] for w in p["weights"])
        return [(r["ok"], r["metric"], r["pre_agg"]["weights"]) for r in hist], out

    h0, p0 = run(False, "serial")
    h1, p1 = run(True, "spec")
    assert len(h0) == 3 and all(ok for ok, _, _ in h0)
    assert h0 == h1
    assert torch.equal(p0, p1)
