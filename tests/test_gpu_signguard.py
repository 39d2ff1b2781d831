"""SignGuard on the device: ``k_sign_stats`` against the fp64 mirror at edge windows, ``k_signguard_select`` against the
mirror on the device's own statistics, the single cases, the aggregate, bit reproducibility, and the engine (captured
rounds; early launch against serial).

Bounds.  Counts: exact.  Squared norms: 1e-9 relative, the project's fp64 Gram standard (worst-case accumulation error
P 2^-53 <= 5e-13 for P <= 4099).  Features: bit-equal (an integer over b, one correctly rounded division).  M and h:
1e-12 relative (one square root and a sum of n <= 64 terms).  Weights: 1e-9.  Aggregate: 1e-6 max(1, |ref|_inf),
multi_krum's and dnc's.  Decisions are compared only where the mirror's margin is >= 1e-6 (``R.reference`` asserts it)."""
import pytest
import torch

import test_signguard as R
from attackfl_amd import agg, ops
from attackfl_amd.config import from_dict
from attackfl_amd.fl.engine import EARLY_AGGREGATORS, FLEngine, build_client_table
from attackfl_amd.ops import composite as C
from launch import parse_attackers

pytestmark = pytest.mark.gpu


def rows(n, P, seed=0):
    gen = torch.Generator().manual_seed(7000 * n + P + seed)
    g = 0.3 * torch.randn(P, generator=gen)
    return g, g[None, :] + 0.01 * torch.randn(n, P, generator=gen)


def windows(P, chunk):
    """(s, b): one column, all columns, a window ending on a block's chunk boundary and one column past it, a wrap."""
    out = {(0, 1), (P - 1, 1), (0, P), (P // 2, 1)}
    if P > chunk:
        out |= {(chunk - 24, 24), (chunk - 24, 25), (chunk, 7), (chunk - 1, 1), (chunk - 1, 2)}
    if P >= 10:
        out |= {(P - 3, 10), (P - 1, P - 1)}
    return sorted(out)


def check_stats(U, g, Ud, gd, s, b):
    q, pos, neg = ops.sign_stats(Ud, gd, s, b)
    rq, rpos, rneg = C.sign_stats(U, g, s, b)
    assert q.dtype == torch.float64 and pos.dtype == torch.int64
    assert torch.equal(pos.cpu(), rpos) and torch.equal(neg.cpu(), rneg), (U.shape, s, b)
    fin = torch.isfinite(rq)
    assert torch.equal(torch.isfinite(q.cpu()), fin)
    err = ((q.cpu() - rq).abs() / rq.clamp_min(1e-300))[fin]
    assert not err.numel() or err.max().item() <= 1e-9, (U.shape, s, b, err.max().item())
    kind = lambda t: torch.nan_to_num(t[~fin], nan=0.0, posinf=1.0, neginf=-1.0)  # NaN stays NaN, +inf stays +inf
    assert torch.equal(kind(q.cpu()), kind(rq))
    return err.max().item() if err.numel() else 0.0


# ---------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("n", [1, 2, 3, 8, 17, 33, 64])
def test_sign_stats_match_mirror(gpu, n):
    chunk = ops.native().sign_stats_chunk()
    worst = 0.0
    for P in (1, 63, 1025, 4099):
        assert ops.native().sign_stats_nblocks(P) == -(-P // chunk)
        g, U = rows(n, P)
        if P > 8:
            U[0, 3] = g[3]  # an exact zero
        Ud, gd = U.to(gpu), g.to(gpu)
        for s, b in windows(P, chunk):
            worst = max(worst, check_stats(U, g, Ud, gd, s, b))
    print(f"sign_stats n={n}: worst squared-norm error {worst:.3e} relative")


def test_sign_stats_views_and_non_finite(gpu):
    g, base = rows(8, 2 * 1025)
    view = base.to(gpu)[:, ::2]
    assert not view.is_contiguous()
    check_stats(base[:, ::2].contiguous(), g[::2].contiguous(), view, g.to(gpu)[::2], 1020, 10)
    g, U = rows(8, 1025)
    U[1, 2] = float("nan")
    U[2, 1000:1010] = float("inf")
    U[3, 1000:1010] = float("-inf")
    for s, b in ((0, 1025), (995, 20), (1020, 10), (0, 4)):
        check_stats(U, g, U.to(gpu), g.to(gpu), s, b)
    q, pos, neg = ops.sign_stats(U.to(gpu), g.to(gpu), 995, 20)
    assert int(pos[2]) >= 10 and int(neg[3]) >= 10 and int(pos[1] + neg[1]) == 20
    assert bool(torch.isnan(q[1])) and q[2:4].tolist() == [float("inf")] * 2 and bool(torch.isfinite(q[4:]).all())
    q, pos, neg = ops.sign_stats(U.to(gpu), g.to(gpu), 0, 4)  # the NaN difference is neither positive nor negative
    assert int(pos[1] + neg[1]) == 3
    g[7] = float("inf")  # finite - inf = -inf in every row but row 4's, whose inf - inf is a NaN
    U[4, 7] = float("inf")
    check_stats(U, g, U.to(gpu), g.to(gpu), 0, 16)


def test_window_seed_and_refusals(gpu):
    g, U = rows(8, 4099)
    Ud, gd = U.to(gpu), g.to(gpu)
    al = torch.full((8,), 0.125, dtype=torch.float64, device=gpu)
    for seed in (0, 1, R.SEED, (1 << 63) + 12345, (1 << 64) - 1):  # the native mixer is the mirror's, top bit included
        assert int(ops.native().signguard_start(ops._seed64(seed), 4099)) == C.signguard_mix(seed) % 4099
        assert ops.signguard_window(4099, 0.25, seed, native_mix=True) == C.signguard_window(4099, 0.25, seed)
    big = (1 << 63) + 12345
    assert ops.signguard_filter(Ud, gd, 0.25, big, al, R.LO, R.HI)[7] == C.signguard_window(4099, 0.25, big)
    assert C.signguard_window(4099, 0.25, big) != C.signguard_window(4099, 0.25, 12345)
    nat = ops.native()
    for s, b in ((0, 0), (0, 4100), (4099, 1), (-1, 1)):  # the launcher refuses instead of launching
        with pytest.raises(RuntimeError):
            nat.signguard_run(Ud, gd, s, b, al, R.LO, R.HI)
    with pytest.raises(RuntimeError):
        nat.signguard_run(torch.zeros(65, 8, device=gpu), torch.zeros(8, device=gpu), 0, 8,
                          torch.ones(65, dtype=torch.float64, device=gpu), R.LO, R.HI)
    with pytest.raises(RuntimeError):
        nat.signguard_run(Ud, gd, 0, 8, al, 2.0, 1.0)


# ---------------------------------------------------------------------------------- decisions
@pytest.mark.parametrize("n,m,P,frac", R.SHAPES)
def test_select_matches_mirror_on_device_statistics(gpu, n, m, P, frac):
    g, U, sizes, (s, b), _ = R.reference(n, m, P, frac)  # (asserts the margins on the fp64 reference)
    Ud, gd = U.to(gpu), g.to(gpu)
    alpha = sizes / sizes.sum()
    q, pos, neg = ops.sign_stats(Ud, gd, s, b)
    keep, ok, label, F, c, M, h = ops.signguard_select(q, pos, neg, b, alpha, R.LO, R.HI)
    rk, rok, rlabel, rF, rc, rM, rh, margin = C.signguard_select(q.cpu(), pos.cpu(), neg.cpu(), b, alpha, R.LO, R.HI)
    assert margin >= 1e-6
    assert torch.equal(keep.cpu(), rk) and torch.equal(ok.cpu(), rok) and rk.tolist() == [i < n - m for i in range(n)]
    assert R.same_partition(label.cpu().tolist(), rlabel.tolist()) and torch.equal(label.cpu(), rlabel)
    assert torch.equal(F.cpu(), rF)
    assert abs(float(M) - float(rM)) <= 1e-12 * float(rM) and abs(float(h) - float(rh)) <= 1e-12 * float(rh)
    assert (c.cpu() - rc).abs().max().item() <= 1e-9
    print(f"signguard_select n={n}: M {abs(float(M) - float(rM)) / float(rM):.1e}, h {abs(float(h) - float(rh)) / float(rh):.1e}, "
          f"weights {(c.cpu() - rc).abs().max().item():.1e}, margin {margin:.2e}")
    # the two-launch form (partials straight into the select kernel) is the same computation, bit for bit
    out = ops.signguard_filter(Ud, gd, frac, R.SEED, alpha, R.LO, R.HI)
    assert out[7] == (s, b)
    for a, bb in zip(out[:7], (keep, ok, label, F, c, M, h)):
        assert torch.equal(a, bb)


def test_single_cases(gpu):
    R.check_single_cases(gpu)


# ---------------------------------------------------------------------------------- aggregate
@pytest.mark.parametrize("n,m,P,frac", R.SHAPES)
def test_aggregate_matches_composite(gpu, n, m, P, frac):
    g, U, sizes, _, _ = R.reference(n, m, P, frac)
    ref = agg.signguard(U, sizes, centre=g, seed=R.SEED, signguard_frac=frac)
    Ud = U.to(gpu)
    res = agg.signguard(Ud, sizes, centre=g.to(gpu), seed=R.SEED, signguard_frac=frac)
    assert torch.equal(res.info["kept"].cpu(), ref.info["kept"]) and res.info["window"] == ref.info["window"]
    err = (res.params.double().cpu() - ref.params.double()).abs().max().item()
    assert err <= 1e-6 * max(1.0, ref.params.abs().max().item())
    assert res.params.untyped_storage().data_ptr() != Ud.untyped_storage().data_ptr()
    assert torch.equal(Ud.cpu(), U)


def test_majority_non_finite_returns_the_centre(gpu):
    g, U, sizes, _, _ = R.reference(8, 2, 4099, 0.25)
    U = U.clone()
    U[:5, 7] = float("nan")
    res = agg.signguard(U.to(gpu), sizes, centre=g.to(gpu), seed=R.SEED)
    assert torch.equal(res.params.cpu(), g) and not bool(res.info["kept"].any())


def test_bit_reproducible(gpu):
    g, U, sizes, _, _ = R.reference(33, 8, 2049, 0.5)
    Ud, gd = U.to(gpu), g.to(gpu)
    a = agg.signguard(Ud, sizes, centre=gd, seed=R.SEED, signguard_frac=0.5)
    b = agg.signguard(Ud, sizes.to(gpu), centre=gd, seed=R.SEED, signguard_frac=0.5)  # (the several-rank path)
    for x, y in ((a, b), (a, agg.signguard(Ud, sizes, centre=gd, seed=R.SEED, signguard_frac=0.5))):
        assert torch.equal(x.params, y.params) and torch.equal(x.info["weights"], y.info["weights"])
        assert torch.equal(x.info["scores"], y.info["scores"]) and torch.equal(x.info["kept"], y.info["kept"])


# ---------------------------------------------------------------------------------- engine
def _engine(tmp_path, rounds, sub, **engine_kw):
    d = {
        "server": {"num-round": rounds, "clients": 7, "mode": "signguard", "model": "TransformerModel",
                   "data-name": "ICU", "genuine-rate": 1.0, "random-seed": 11,
                   "data-distribution": {"num-data-range": [300, 500]}},
        "learning": {"epoch": 2, "batch-size": 128},
        "data": {"synthetic": True, "train-size": 4000, "test-size": 1000},
        "engine": {"checkpoint-dir": str(tmp_path / sub), "trainer": "auto", "seed": 3, "signguard-frac": 0.2,
                   **engine_kw},
        "log_path": str(tmp_path / sub),
    }
    cfg = from_dict(d)
    return FLEngine(cfg, device="cuda", table=build_client_table(cfg, 1, parse_attackers("6:Min-Max:2")),
                    verbose=False)


def test_engine_rounds_match_composite(gpu, tmp_path, monkeypatch):
    """7 clients, one Min-Max attacker from round 2, fused trainer: every round's device aggregate and masks against
    the CPU composite on the captured rows; the rule runs in the early launch."""
    eng = _engine(tmp_path, 3, "e2e")
    assert eng.trainer.kind == "fused" and "signguard" in EARLY_AGGREGATORS
    seen = []
    orig_fn = agg.AGGREGATORS["signguard"]

    def capture(U, sizes, **kw):
        rows_ = U.detach().cpu().clone()
        res = orig_fn(U, sizes, **kw)
        kw = {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in kw.items()}
        seen.append((rows_, sizes.detach().cpu().clone(), res.params.detach().cpu().clone(), kw))
        return res

    monkeypatch.setitem(agg.AGGREGATORS, "signguard", capture)
    hist = eng.run()
    eng.close()
    assert [r["ok"] for r in hist] == [True, True, True] and len(seen) == 3
    assert any(r.get("path") == "early-launch" for r in hist)
    assert all(0.0 <= r["metric"] <= 1.0 for r in hist)
    assert "attack" in hist[1] and "attack" in hist[2]
    for k, (rows_, sizes, got, kw) in enumerate(seen):
        assert (kw["signguard_frac"], kw["signguard_lo"], kw["signguard_hi"]) == (0.2, 0.1, 3.0)
        assert (kw["centre"] is None) == (k == 0)
        ref = orig_fn(rows_, sizes, **kw)
        assert (got.double() - ref.params.double()).abs().max().item() <= 1e-6 * max(1.0, ref.params.abs().max().item())
        assert hist[k]["kept"] == torch.nonzero(ref.info["kept"]).reshape(-1).tolist(), k
        assert hist[k]["norm_ok"] == torch.nonzero(ref.info["norm_ok"]).reshape(-1).tolist(), k
        assert hist[k]["window"] == ref.info["window"] and "scores" not in hist[k]


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
