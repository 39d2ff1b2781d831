"""FLAME on the device: ``k_flame_select`` against the fp64 mirror on the device's own Gram, the device Gram against
the CPU Gram, the single cases, ``k_flame_rows`` against ``k_anchored_rows`` (no noise: bit-equal) and against the
mirror (noise), refusals, the aggregate, bit reproducibility, the engine (captured rounds; early launch against serial) and two
ranks against one process.

Bounds.  Gram: 1e-9 relative to sqrt(G_ii G_jj), the project's fp64 Gram standard.  Given the same G the kernel and the
mirror do the same correctly rounded operations in the same order: keep, d*, S and sigma are bit-equal, c within 1e-9.
Across the two Grams keep is compared where the mirror's margin is >= 1e-6 (a Gram error of 1e-9 moves a cosine
distance by less than 3e-9).  Rows: 1e-6 max(1, |ref|_inf), multi_krum's and cclip's bound, plus 6.7e-6 sigma for the
draw: ``test_philox_noise_matches_cpu_mirror`` allows a draw 2e-6 at sigma = 0.3 (the device's log, sin and cos against
numpy's, then the fp32 rounding of the draw)."""
import pytest
import torch

import test_flame as R
from attackfl_amd import agg, ops
from attackfl_amd.config import from_dict
from attackfl_amd.fl.engine import EARLY_AGGREGATORS, FLEngine, build_client_table
from attackfl_amd.ops import composite as C
from launch import parse_attackers

pytestmark = pytest.mark.gpu

DRAW = 6.7e-6  # (2e-6 / 0.3)


def rows(n, P, seed=0):
    gen = torch.Generator().manual_seed(7100 * n + P + seed)
    g = 0.3 * torch.randn(P, generator=gen)
    _, H = R.honest_rows(n, P, gen)
    return g, (g.double()[None, :] + 0.01 * H).float()


def row_bound(ref, sigma=0.0):
    return 1e-6 * max(1.0, ref.abs().max().item()) + DRAW * sigma


# ---------------------------------------------------------------------------------- decisions
@pytest.mark.parametrize("n", [1, 2, 3, 4, 8, 17, 33, 64])
def test_select_matches_mirror_on_device_gram(gpu, n):
    sizes = R.sizes_of(n)
    alpha = sizes / sizes.sum()
    for P in (63, 1025, 4099):
        g, U = rows(n, P)
        Gd = ops.gram_anchored(U.to(gpu), g.to(gpu))
        # the device Gram against the CPU fp64 Gram
        Gc = C.gram_anchored(U, g)
        scale = Gc.diagonal().sqrt()
        gerr = ((Gd.cpu() - Gc).abs() / (scale[:, None] * scale[None, :])).max().item()
        keep, c, info = ops.flame_select(Gd, alpha, R.LAM)
        # the same G: the same bits
        rk, rc, rinfo, _ = C.flame_select(Gd.cpu(), alpha, R.LAM)
        cerr = (c.cpu() - rc).abs().max().item()
        print(f"flame_select n={n} P={P}: Gram {gerr:.2e} relative, weights {cerr:.2e}, d* {float(info[2]):.6f}")
        assert gerr <= 1e-9
        assert keep.dtype == torch.bool and c.dtype == torch.float64 and info.shape == (5,)
        assert torch.equal(keep.cpu(), rk) and torch.equal(info.cpu().view(torch.int64), rinfo.view(torch.int64))
        assert cerr <= 1e-9 and int(info[3]) == n // 2 + 1 and int(info[4]) == n
        # the CPU Gram: the same rows kept wherever the mirror's decision has a margin
        ck, _, cinfo, margin = C.flame_select(Gc, alpha, R.LAM)
        if margin >= R.MARGIN:
            assert torch.equal(keep.cpu(), ck), (n, P, margin)
        assert abs(float(info[2]) - float(cinfo[2])) <= 3e-9
        assert abs(float(info[0]) - float(cinfo[0])) <= 1e-9 * float(cinfo[0])


@pytest.mark.parametrize("n,m,P", R.SHAPES)
def test_select_on_the_reference(gpu, n, m, P):
    g, U, sizes, (rk, rc, rinfo, margin) = R.reference(n, m, P)  # (asserts the margin on the fp64 reference)
    assert margin >= R.MARGIN
    keep, c, info = ops.flame_filter(U.to(gpu), g.to(gpu), sizes / sizes.sum(), R.LAM)
    assert torch.equal(keep.cpu(), rk) and not keep[n - m:].any()
    assert (c.cpu() - rc).abs().max().item() <= 1e-9 and (info.cpu() - rinfo).abs().max().item() <= 3e-9


def test_single_cases(gpu):
    R.check_single_cases(gpu)


def test_refusals(gpu):
    nat = ops.native()
    f64 = lambda *s: torch.ones(*s, dtype=torch.float64, device=gpu)
    for n in (65, 0):  # the launcher refuses instead of launching
        with pytest.raises(RuntimeError):
            nat.flame_select(f64(n, n), f64(n), 0.001)
    for lam in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            nat.flame_select(f64(4, 4), f64(4), lam)
    with pytest.raises(RuntimeError):
        nat.flame_select(f64(4, 4), f64(3), 0.001)
    with pytest.raises(RuntimeError):  # sigma on the host
        nat.flame_rows(torch.zeros(2, 8, device=gpu), f64(2), torch.zeros(8, device=gpu),
                       torch.zeros(1, dtype=torch.float64), 0)
    # beyond the kernel's rows the dispatch goes to the mirror
    g, U = rows(65, 63)
    keep, c, info = ops.flame_filter(U.to(gpu), g.to(gpu), torch.full((65,), 1.0 / 65, dtype=torch.float64), R.LAM)
    rk, rc, rinfo = C.flame_filter(U, g, torch.full((65,), 1.0 / 65, dtype=torch.float64), R.LAM)
    assert keep.is_cuda and int(info[3]) == 33 and int(keep.sum()) >= 33
    assert (info.cpu() - rinfo).abs().max().item() <= 3e-9


# ---------------------------------------------------------------------------------- rows
@pytest.mark.parametrize("P", [1, 3, 4, 5, 1025, 4099])
def test_rows_match_anchored_rows_and_mirror(gpu, P):
    n = 9
    g, U = rows(n, P)
    gen = torch.Generator().manual_seed(P)
    c = torch.rand(n, generator=gen, dtype=torch.float64) / n
    c[2] = 0.0
    c[7] = 0.0
    U[2, 0] = float("nan")  # a c with zeros skips NaN rows
    U[7, :] = float("inf")
    Ud, gd, cd = U.to(gpu), g.to(gpu), c.to(gpu)
    want0 = ops.anchored_rows(Ud, cd, gd)
    for sigma in (0.0, torch.zeros(1, dtype=torch.float64, device=gpu)):
        got0 = ops.flame_rows(Ud, cd, gd, sigma, R.SEED)
        assert torch.equal(got0.view(torch.int32), want0.view(torch.int32)) and bool(torch.isfinite(got0).all())
    worst = 0.0
    for sigma in (1e-5, 0.3):
        ref = C.flame_rows(U, c, g, sigma, R.SEED)
        for s in (sigma, torch.tensor([sigma], dtype=torch.float64, device=gpu)):
            got = ops.flame_rows(Ud, cd, gd, s, R.SEED)
            err = (got.double().cpu() - ref.double()).abs().max().item()
            worst = max(worst, err / row_bound(ref, sigma))
            assert got.shape == (P,) and err <= row_bound(ref, sigma), (P, sigma, err)
        assert not torch.equal(got, want0)
    print(f"flame_rows P={P}: worst error {worst:.3f} of the bound")
    assert not torch.equal(ops.flame_rows(Ud, cd, gd, 0.3, R.SEED + 1), got) or P < 2


def test_rows_of_a_view(gpu):
    g, base = rows(8, 2 * 1028)
    c = torch.linspace(0.05, 0.2, 8, dtype=torch.float64)
    view = base.to(gpu)[:, ::2]
    assert not view.is_contiguous()
    ref = C.flame_rows(base[:, ::2].contiguous(), c, g[::2].contiguous(), 0.01, R.SEED)
    got = ops.flame_rows(view, c.to(gpu), g.to(gpu)[::2], 0.01, R.SEED)
    assert (got.double().cpu() - ref.double()).abs().max().item() <= row_bound(ref, 0.01)


# ---------------------------------------------------------------------------------- aggregate
@pytest.mark.parametrize("n,m,P", R.SHAPES)
def test_aggregate_matches_composite(gpu, n, m, P):
    g, U, sizes, _ = R.reference(n, m, P)
    ref = agg.flame(U, sizes, centre=g, seed=R.SEED, flame_noise=R.LAM)
    Ud = U.to(gpu)
    res = agg.flame(Ud, sizes, centre=g.to(gpu), seed=R.SEED, flame_noise=R.LAM)
    assert set(res.info) == R.INFO_KEYS and torch.equal(res.info["kept"].cpu(), ref.info["kept"])
    sigma = float(ref.info["sigma"])
    err = (res.params.double().cpu() - ref.params.double()).abs().max().item()
    print(f"agg.flame n={n} P={P}: error {err:.3e}, bound {row_bound(ref.params, sigma):.3e}, sigma {sigma:.3e}")
    assert err <= row_bound(ref.params, sigma) and sigma > 0.0
    assert abs(float(res.info["sigma"]) - sigma) <= 1e-9 * sigma
    assert res.params.untyped_storage().data_ptr() != Ud.untyped_storage().data_ptr()
    assert torch.equal(Ud.cpu(), U)
    # without noise: the bits of cclip's row pass on the same weights
    quiet = agg.flame(Ud, sizes, centre=g.to(gpu), seed=R.SEED, flame_noise=0.0)
    assert torch.equal(quiet.params, ops.anchored_rows(Ud, quiet.info["weights"], g.to(gpu)))
    assert torch.equal(quiet.info["weights"], res.info["weights"]) and float(quiet.info["sigma"]) == 0.0


def test_bit_reproducible(gpu):
    g, U, sizes, _ = R.reference(33, 8, 2049)
    Ud, gd = U.to(gpu), g.to(gpu)
    a = agg.flame(Ud, sizes, centre=gd, seed=R.SEED)
    b = agg.flame(Ud, sizes.to(gpu), centre=gd, seed=R.SEED)  # (the several-rank path)
    for x, y in ((a, b), (a, agg.flame(Ud, sizes, centre=gd, seed=R.SEED))):
        assert torch.equal(x.params, y.params) and torch.equal(x.info["weights"], y.info["weights"])
        assert torch.equal(x.info["kept"], y.info["kept"]) and torch.equal(x.info["sigma"], y.info["sigma"])
    assert not torch.equal(a.params, agg.flame(Ud, sizes, centre=gd, seed=R.SEED + 1).params)


# ---------------------------------------------------------------------------------- engine
def _engine(tmp_path, rounds, sub, **engine_kw):
    d = {
        "server": {"num-round": rounds, "clients": 7, "mode": "flame", "model": "TransformerModel",
                   "data-name": "ICU", "genuine-rate": 1.0, "random-seed": 11,
                   "data-distribution": {"num-data-range": [300, 500]}},
        "learning": {"epoch": 2, "batch-size": 128},
        "data": {"synthetic": True, "train-size": 4000, "test-size": 1000},
        "engine": {"checkpoint-dir": str(tmp_path / sub), "trainer": "auto", "seed": 3, **engine_kw},
        "log_path": str(tmp_path / sub),
    }
    cfg = from_dict(d)
    return FLEngine(cfg, device="cuda", table=build_client_table(cfg, 1, parse_attackers("6:Min-Max:2")),
                    verbose=False)


def test_engine_rounds_match_composite(gpu, tmp_path, monkeypatch):
    """7 clients, one Min-Max attacker from round 2, fused trainer: every round's device aggregate and kept rows against
    the CPU composite on the captured rows; the rule runs in the early launch."""
    eng = _engine(tmp_path, 3, "e2e")
    assert eng.trainer.kind == "fused" and "flame" in EARLY_AGGREGATORS
    seen = []
    orig_fn = agg.AGGREGATORS["flame"]

    def capture(U, sizes, **kw):
        rows_ = U.detach().cpu().clone()
        res = orig_fn(U, sizes, **kw)
        kw = {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in kw.items()}
        seen.append((rows_, sizes.detach().cpu().clone(), res.params.detach().cpu().clone(), kw))
        return res

    monkeypatch.setitem(agg.AGGREGATORS, "flame", capture)
    hist = eng.run()
    eng.close()
    assert [r["ok"] for r in hist] == [True, True, True] and len(seen) == 3
    assert any(r.get("path") == "early-launch" for r in hist)
    assert all(0.0 <= r["metric"] <= 1.0 for r in hist)
    assert "attack" in hist[1] and "attack" in hist[2]
    for k, (rows_, sizes, got, kw) in enumerate(seen):
        assert kw["flame_noise"] == 0.001 and (kw["centre"] is None) == (k == 0)
        ref = orig_fn(rows_, sizes, **kw)
        sigma = float(ref.info["sigma"])
        assert (sigma > 0.0) == (k > 0)
        assert (got.double() - ref.params.double()).abs().max().item() <= row_bound(ref.params, sigma), k
        margin = R.MARGIN if k == 0 else C.flame_select(C.gram_anchored(rows_, kw["centre"]),
                                                        sizes.double() / sizes.double().sum(), 0.001)[3]
        if margin >= R.MARGIN:  # (else the kept rows of two Grams need not agree)
            assert hist[k]["kept"] == torch.nonzero(ref.info["kept"]).reshape(-1).tolist(), k
        print(f"round {k}: margin {margin:.2e}, kept {hist[k]['kept']}, sigma {sigma:.3e}")
        assert abs(hist[k]["sigma"] - sigma) <= 1e-9 * max(sigma, 1e-300) and hist[k]["majority"] == 4
        assert abs(hist[k]["threshold"] - float(ref.info["threshold"])) <= 3e-9


def test_early_launch_matches_serial_schedule(gpu, tmp_path):
    def run(spec, sub):
        eng = _engine(tmp_path, 4, sub, speculative=spec)
        assert eng._speculative == spec
        hist = eng.run()
        out = eng.global_params.detach().cpu().clone()
        assert not spec or any(r.get("path") == "early-launch" for r in hist)
        eng.close()
        return [(r["ok"], r["metric"], r["kept"], r["sigma"]) for r in hist], out

    h0, p0 = run(False, "serial")
    h1, p1 = run(True, "spec")
    assert len(h0) == 4 and all(r[0] for r in h0) and h0[-1][3] > 0.0
    assert h0 == h1
    assert torch.equal(p0, p1)  # (noise included)


def test_two_ranks_match_single_process_bitwise(gpu, tmp_path, monkeypatch):
    """A 2-rank flame run (2 processes sharing the GPU) against the single-process checkpoint, bit for bit: the
    several-rank test's own body on a flame case."""
    import test_gpu_multirank as M

    monkeypatch.setitem(M.CASES, "tf-flame-minmax", ("TransformerModel", "flame", {5: {"mode": "Min-Max", "round": 2}}))
    M.test_ranks_sharing_gpu_match_single_process_bitwise(gpu, tmp_path, 2, "tf-flame-minmax")
