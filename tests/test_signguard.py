"""The SignGuard server mode on the CPU: the window, the host mirror's mean shift against sklearn, the rule's behaviour
on planted sign-shifted rows, the single cases (filter bounds, non-finite rows, ties, clipping), config, the engine.

Shared data (also used by tests/test_gpu_signguard.py): ``reference(n, m, P, frac)``, n - m honest rows g + 0.01 N(0, I)
and m rows g + 0.01 (N(0, I) - 0.8), whose sign balance is about 0.21 / 0.79 and whose norm is about 1.3 times the honest
one.  The helper asserts on the fp64 mirror that every decision it took has a relative margin >= 1e-6 and that exactly
the honest rows are kept, so no test passes by comparing two arbitrary answers.  ``check_single_cases(dev)`` runs the
single cases on any device."""
import functools
import json
import math

import pytest
import torch

from attackfl_amd import agg, ops
from attackfl_amd.config import SIGNGUARD_FRAC, SIGNGUARD_HI, SIGNGUARD_LO, from_dict
from attackfl_amd.fl.engine import EARLY_AGGREGATORS, FLEngine, build_client_table
from attackfl_amd.ops import composite as C
from launch import parse_attackers

# (n, m, P, frac)
SHAPES = [(8, 2, 4099, 0.25), (7, 1, 1025, 1.0), (33, 8, 2049, 0.5), (64, 15, 1025, 1.0)]
SEED = 77
LO, HI = 0.1, 3.0
INFO_KEYS = {"kept", "norm_ok", "cluster", "scores", "weights", "median_norm", "bandwidth", "window"}


def sizes_of(n):
    return torch.tensor([300.0 + 37.0 * ((5 * i) % 7) for i in range(n)], dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def reference(n, m, P, frac, seed=0):
    """(g, U, sizes, (s, b), the mirror's results on them), computed once and never modified."""
    gen = torch.Generator().manual_seed(100000 * n + 1000 * m + P % 997 + seed)
    g = torch.randn(P, generator=gen)
    U = g[None, :] + 0.01 * torch.randn(n, P, generator=gen)
    U[n - m:] -= 0.008
    sizes = sizes_of(n)
    s, b = C.signguard_window(P, frac, SEED)
    q, pos, neg = C.sign_stats(U, g, s, b)
    out = C.signguard_select(q, pos, neg, b, sizes / sizes.sum(), LO, HI)
    assert out[7] >= 1e-6, (n, m, P, frac, out[7])
    assert out[0].tolist() == [i < n - m for i in range(n)], (n, m, P, frac, out[0].tolist())
    return g, U, sizes, (s, b), out


def same_partition(a, b):
    a, b = [int(x) for x in a], [int(x) for x in b]
    return len(a) == len(b) and len(set(zip(a, b))) == len(set(a)) == len(set(b))


# ---------------------------------------------------------------------------------- window
def test_window_sizes_and_start():
    for P in (1, 2, 10, 1025):
        for frac in (1e-9, 0.1, 0.5, 1, 7):
            s, b = C.signguard_window(P, frac, SEED)
            assert b == min(P, max(1, math.ceil(frac * P))) and 0 <= s < P, (P, frac, s, b)
            assert s == (0 if b == P else C.signguard_mix(SEED) % P)
            assert (s, b) == ops.signguard_window(P, frac, SEED)
    assert C.signguard_window(10, 0.1, 3)[1] == 1 and C.signguard_window(1025, 0.1, 3)[1] == 103
    assert C.signguard_window(4099, 0.25, 5) == C.signguard_window(4099, 0.25, 5)
    assert C.signguard_window(4099, 0.25, 1)[0] != C.signguard_window(4099, 0.25, 2)[0]
    assert C.signguard_window(4099, 0.25, (1 << 63) + 5)[0] != C.signguard_window(4099, 0.25, 5)[0]  # (the high word counts)
    for bad in ((0, 0.1), (10, 0.0), (10, -1.0), (10, float("nan"))):
        with pytest.raises(ValueError):
            C.signguard_window(bad[0], bad[1], 0)


def test_window_wraps():
    P, frac = 10, 0.5
    seed = next(k for k in range(1000) if C.signguard_window(P, frac, k)[0] > P - 5)
    s, b = C.signguard_window(P, frac, seed)
    cols = [(s + k) % P for k in range(b)]
    assert b == 5 and min(cols) == 0 and max(cols) == P - 1  # (it wraps)
    gen = torch.Generator().manual_seed(4)
    U, g = torch.randn(3, P, generator=gen), torch.randn(P, generator=gen)
    q, pos, neg = C.sign_stats(U, g, s, b)
    d = U.double() - g.double()
    assert pos.tolist() == [sum(1 for c in cols if d[i, c] > 0) for i in range(3)]
    assert neg.tolist() == [sum(1 for c in cols if d[i, c] < 0) for i in range(3)]
    assert torch.allclose(q, (d * d).sum(dim=1), rtol=1e-14, atol=0)
    for bad in ((0, 0), (0, P + 1), (P, 1), (-1, 1)):
        with pytest.raises(ValueError):
            C.sign_stats(U, g, *bad)


# ---------------------------------------------------------------------------------- mean shift against sklearn
@pytest.mark.parametrize("n,m,P,frac", SHAPES)
def test_mean_shift_matches_sklearn(n, m, P, frac):
    from sklearn.cluster import MeanShift, estimate_bandwidth

    _, _, _, (s, b), out = reference(n, m, P, frac)
    label, F, h = out[2], out[3].numpy(), float(out[6])
    sk = MeanShift(bandwidth=h, bin_seeding=False, cluster_all=True).fit(F).labels_
    assert same_partition(label.tolist(), sk.tolist()) and len(set(label.tolist())) == 2
    assert int(0.5 * n) >= 1 and h > 1.0 / b  # (the floor of one count is not active: h is the mean radius itself)
    assert abs(h - estimate_bandwidth(F, quantile=0.5)) <= 1e-12 * h


# ---------------------------------------------------------------------------------- rule behaviour
@pytest.mark.parametrize("n,m,P,frac", SHAPES)
def test_planted_sign_shift_is_dropped(n, m, P, frac):
    g, U, sizes, (s, b), out = reference(n, m, P, frac)
    keep, ok, label, F, c, M, h, _ = out
    assert ok.all() and (F[: n - m, 2] < 0.6).all() and (F[n - m:, 2] > 0.7).all()  # (inside [lo, hi]; the balance moved)
    keep0 = U.clone()
    res = agg.signguard(U, sizes, centre=g, seed=SEED, signguard_frac=frac)
    assert torch.equal(U, keep0) and res.params.data_ptr() != U.data_ptr()
    assert set(res.info) == INFO_KEYS and res.info["window"] == [s, b]
    assert torch.equal(res.info["kept"], keep) and torch.equal(res.info["weights"], c)
    # by hand, in fp64: the kept rows' clipped, size-weighted mean about g
    d = U.double() - g.double()
    norm = (d * d).sum(dim=1).sqrt()
    med = torch.sort(norm).values[(n - 1) // 2]
    a = sizes / sizes.sum()
    w = keep.double() * a * torch.clamp(med / norm, max=1.0)
    want = g.double() + (w[:, None] * d).sum(dim=0) / (keep.double() * a).sum()
    assert abs(float(M) - float(med)) <= 1e-12 * float(med)
    assert (res.params.double() - want).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item())


# ---------------------------------------------------------------------------------- single cases
def balanced_signs(n, P, gen):
    """[n, P] of +-1, every row with (P + 1) // 2 positives at places of its own: the rows' sign features are equal."""
    pattern = torch.cat([torch.ones((P + 1) // 2), -torch.ones(P // 2)])
    return torch.stack([pattern[torch.randperm(P, generator=gen)] for _ in range(n)])


def base(n=8, P=257, seed=0):
    """Honest rows about a Gaussian g whose differences have Gaussian sizes (never below 1e-5, so that none vanishes in
    fp32) and balanced signs: one cluster whatever the draw, so a single case shows the one thing it changes."""
    gen = torch.Generator().manual_seed(9000 + 10 * n + seed)
    g = torch.randn(P, generator=gen)
    U = g[None, :] + 0.01 * torch.randn(n, P, generator=gen).abs().clamp_min(1e-3) * balanced_signs(n, P, gen)
    return g, U, sizes_of(n)


def run(dev, g, U, sizes, **kw):
    kw = {"signguard_frac": 1.0, **kw}
    before = U.clone()
    Ud = U.to(dev)
    res = agg.signguard(Ud, sizes, centre=g.to(dev), seed=SEED, **kw)
    assert torch.equal(Ud.cpu().view(torch.int32), before.view(torch.int32))  # U is read-only (bits: NaN rows too)
    assert set(res.info) == INFO_KEYS and res.params.dtype == torch.float32
    assert res.params.untyped_storage().data_ptr() != Ud.untyped_storage().data_ptr()
    return res, {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in res.info.items()}


def check_single_cases(dev):
    n = 8
    every = [True] * n
    # a 10 x norm row is dropped by hi, a 0.01 x norm row by lo
    for factor in (10.0, 0.01):
        g, U, sizes = base()
        U[3] = g + factor * (U[3] - g)
        res, info = run(dev, g, U, sizes)
        assert info["norm_ok"].tolist() == [i != 3 for i in range(n)], factor
        assert info["kept"].tolist() == [i != 3 for i in range(n)] and float(info["weights"][3]) == 0.0
        assert bool(torch.isfinite(res.params).all()) and not torch.equal(res.params.cpu(), g)
        assert run(dev, g, U, sizes, signguard_lo=0.001, signguard_hi=20.0)[1]["norm_ok"].tolist() == every
    # a NaN row and an inf row are dropped and never reach the sum
    g, U, sizes = base()
    U[2, 5] = float("nan")
    U[6, :] = float("inf")
    res, info = run(dev, g, U, sizes)
    assert info["kept"].tolist() == [i not in (2, 6) for i in range(n)] and info["norm_ok"].tolist() == info["kept"].tolist()
    assert info["scores"][6].tolist() == [1.0, 0.0, 0.0] and int(info["cluster"][6]) != int(info["cluster"][0])
    assert bool(torch.isfinite(res.params).all()) and math.isfinite(float(info["median_norm"]))
    # more than half the rows non-finite: M = +inf, no row passes, the round makes no step
    g, U, sizes = base()
    U[:5, 0] = float("nan")
    res, info = run(dev, g, U, sizes)
    assert math.isinf(float(info["median_norm"])) and not info["kept"].any() and not info["weights"].any()
    assert torch.equal(res.params.cpu(), g)
    # every row equal to g
    g, U, sizes = base()
    U = g[None, :].expand(n, -1).clone()
    res, info = run(dev, g, U, sizes)
    assert info["kept"].tolist() == every and float(info["median_norm"]) == 0.0 and torch.equal(res.params.cpu(), g)
    assert info["scores"].tolist() == [[0.0, 1.0, 0.0]] * n and float(info["bandwidth"]) == 1.0 / 257
    assert (info["weights"] - sizes / sizes.sum()).abs().max().item() <= 1e-15
    # n = 1, 2, 3
    for k in (1, 2, 3):
        g, U, sizes = base(k)
        res, info = run(dev, g, U, sizes)
        assert res.params.shape == g.shape and bool(torch.isfinite(res.params).all())
        assert info["kept"].shape == (k,) and bool(info["kept"][0]) and float(info["bandwidth"]) > 0.0
    # exact zeros in the window show up in the middle feature
    g, U, sizes = base()
    U[1, 100:110] = g[100:110]
    _, info = run(dev, g, U, sizes)
    assert float(info["scores"][1, 1]) == 10.0 / 257 and not info["scores"][[0, 2, 3], 1].any()
    assert (info["scores"].sum(dim=1) - 1.0).abs().max().item() <= 1e-15
    # clipping: powers of two about g = 0, every norm exactly M but row 3's, which is exactly 2 M -> scale 1/2
    P = 256
    gen = torch.Generator().manual_seed(5)
    g = torch.zeros(P)
    U = 0.0078125 * balanced_signs(n, P, gen)
    U[3] *= 2.0
    sizes = sizes_of(n)
    res, info = run(dev, g, U, sizes)
    a = sizes / sizes.sum()
    assert info["kept"].tolist() == every and float(info["median_norm"]) == 0.0078125 * 16.0
    scale = torch.ones(n, dtype=torch.float64)
    scale[3] = 0.5
    assert (info["weights"] - a * scale).abs().max().item() <= 1e-15
    want = ((a * scale)[:, None] * U.double()).sum(dim=0)
    assert (res.params.double().cpu() - want).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item())
    # the tie rules, on the statistics themselves: two clusters of equal size and equal counts -> the lower index wins
    q = torch.ones(4, dtype=torch.float64, device=dev)
    al = torch.full((4,), 0.25, dtype=torch.float64, device=dev)
    for first in ([0, 1], [0, 3], [0, 2]):
        pos = torch.tensor([10 if i in first else 0 for i in range(4)], device=dev)
        keep, ok, label, F, c, M, h = ops.signguard_select(q, pos, 10 - pos, 10, al, LO, HI)
        assert keep.cpu().tolist() == [i in first for i in range(4)] and ok.cpu().tolist() == [True] * 4
        assert label.cpu().tolist() == [0 if i in first else 1 for i in range(4)]
        assert float(h) == 0.1 and float(M) == 1.0 and c.cpu().tolist() == [0.5 if i in first else 0.0 for i in range(4)]
    pos = torch.tensor([0, 10], device=dev)  # two singletons: row 0's cluster
    keep = ops.signguard_select(q[:2], pos, 10 - pos, 10, al[:2], LO, HI)[0]
    assert keep.cpu().tolist() == [True, False]


def test_single_cases():
    check_single_cases("cpu")


def test_margin_reports_a_tie():
    q = torch.ones(4, dtype=torch.float64)
    pos = torch.tensor([10, 10, 0, 0])
    assert C.signguard_select(q, pos, 10 - pos, 10, torch.full((4,), 0.25, dtype=torch.float64), LO, HI)[7] == 0.0


def test_no_centre_is_fedavg_and_registered():
    assert "signguard" in agg.AGGREGATORS and "signguard" in EARLY_AGGREGATORS
    g, U, sizes = base()
    before = U.clone()
    res = agg.signguard(U, sizes, seed=SEED)
    assert torch.equal(res.params, ops.fedavg(U, sizes)) and torch.equal(U, before)
    assert set(res.info) == INFO_KEYS and res.info["kept"].tolist() == [True] * 8
    assert torch.equal(res.info["weights"], sizes / sizes.sum())
    assert agg.signguard(U, None, centre=g).info["kept"].shape == (8,)  # (no sizes: equal weights)
    for kw in ({"signguard_frac": 0.0}, {"signguard_lo": -1.0}, {"signguard_hi": float("nan")},
               {"signguard_lo": 2.0, "signguard_hi": 1.0}):
        with pytest.raises(ValueError):
            agg.signguard(U, sizes, centre=g, **kw)


# ---------------------------------------------------------------------------------- config
def test_config_keys():
    cfg = from_dict({"server": {"mode": "signguard"}})
    assert cfg.mode == "signguard"
    assert (cfg.engine["signguard-frac"], cfg.engine["signguard-lo"], cfg.engine["signguard-hi"]) == (0.1, 0.1, 3.0)
    assert (SIGNGUARD_FRAC.default, SIGNGUARD_LO.default, SIGNGUARD_HI.default) == (0.1, 0.1, 3.0)
    for key in ("signguard-frac", "signguard-lo", "signguard-hi"):
        for bad in (True, [0.5], 0, -1.0, "x", None):
            with pytest.raises(ValueError, match=f"engine.{key} must be"):
                from_dict({"server": {"mode": "signguard"}, "engine": {key: bad}})
    with pytest.raises(ValueError, match="signguard-lo"):
        from_dict({"server": {"mode": "signguard"}, "engine": {"signguard-lo": 4.0}})
    ok = from_dict({"server": {"mode": "signguard"}, "engine": {"signguard-frac": "1e-1", "signguard-lo": 1, "signguard-hi": 1}})
    assert ok.engine["signguard-frac"] == "1e-1"
    assert from_dict({"server": {"mode": "signguard"}, "engine": {"pre-agg": "nnm"}}).engine["pre-agg"] == "nnm"


# ---------------------------------------------------------------------------------- engine
def test_engine_three_rounds(tmp_path, monkeypatch):
    d = {
        "server": {"num-round": 3, "clients": 7, "mode": "signguard", "model": "TransformerModel",
                   "genuine-rate": 1.0, "data-distribution": {"num-data-range": [150, 260]}},
        "learning": {"epoch": 1, "batch-size": 64},
        "data": {"synthetic": True, "train-size": 1500, "test-size": 400},
        "engine": {"checkpoint-dir": str(tmp_path), "trainer": "eager", "max-retries": 3, "signguard-frac": "2e-1",
                   "signguard-lo": 0.2, "signguard-hi": 2.5, "metrics": str(tmp_path / "metrics.jsonl")},
        "log_path": str(tmp_path),
    }
    seen = []
    orig = agg.AGGREGATORS["signguard"]

    def capture(U, sizes, **kw):
        seen.append(kw)
        return orig(U, sizes, **kw)

    monkeypatch.setitem(agg.AGGREGATORS, "signguard", capture)
    cfg = from_dict(d)
    eng = FLEngine(cfg, device="cpu", table=build_client_table(cfg, 1, parse_attackers("6:Min-Max:2")), verbose=False)
    hist = eng.run()
    sel = eng.selected
    assert eng.server.early_ok()  # (the device path would take the early launch; not beyond the kernel's 64 rows,
    eng.selected = list(range(65))  # where the rule is its host mirror, which reads the statistics back)
    assert not eng.server.early_ok()
    eng.selected = sel
    eng.close()
    assert [r["ok"] for r in hist] == [True] * 3 and all(0.0 <= r["metric"] <= 1.0 for r in hist)
    assert len(seen) == 3 and seen[0]["centre"] is None and seen[1]["centre"] is not None
    assert len({kw["seed"] for kw in seen}) == 3  # a fresh window every round
    P = eng.P
    for kw, r in zip(seen, hist):
        assert (kw["signguard_frac"], kw["signguard_lo"], kw["signguard_hi"]) == (0.2, 0.2, 2.5)
        assert r["window"][1] == math.ceil(0.2 * P) and 0 <= r["window"][0] < P
    with open(tmp_path / "metrics.jsonl") as fh:
        recs = [json.loads(line) for line in fh if line.strip()]
    recs = [r for r in recs if "kept" in r]
    assert len(recs) == 3
    for r in recs:
        assert (INFO_KEYS - {"scores"}) <= set(r) and "scores" not in r
        assert len(r["cluster"]) == 7 and len(r["weights"]) == 7 and set(r["kept"]) <= set(range(7))
