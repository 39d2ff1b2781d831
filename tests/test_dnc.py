"""The Divide-and-Conquer (DnC) server mode on the CPU: the keyed column map, the composite's scores against the
parameter-space SVD, planted colluders, the tie / NaN / empty-intersection rules, config and dispatch, the engine.

Shared data (also used by tests/test_gpu_dnc.py): rows base(std 0.3) + 0.01 randn whose last f rows collude along ONE
shared random sign vector d, row k of them by 0.03 (1 + 0.02 k) d.  Every comparison first asserts on the fp64
reference that the problem is well posed (lambda_1 / lambda_2 >= 4, a gap at the cut >= 1e-3 lambda_1), so no test
passes by comparing two arbitrary answers."""
import functools
import math

import pytest
import torch

from attackfl_amd import agg, ops
from attackfl_amd.config import from_dict
from attackfl_amd.fl.engine import EARLY_AGGREGATORS, FLEngine
from attackfl_amd.ops import composite as C

# (n, f, P, b)
SHAPES = [(3, 1, 64, 64), (8, 1, 257, 100), (8, 2, 1025, 257), (17, 4, 1100, 1024), (33, 8, 2049, 1025),
          (64, 16, 4099, 1024), (8, 1, 47693, 10000)]
ITERS = 3  # (iters = 1 is the first iteration of the same keyed subsets)
SEED = 77


@functools.lru_cache(maxsize=None)
def planted(n, f, P, seed=0):
    g = torch.Generator().manual_seed(100000 * n + 1000 * f + P % 997 + seed)
    U = 0.3 * torch.randn(1, P, generator=g) + 0.01 * torch.randn(n, P, generator=g)
    d = torch.sign(torch.randn(P, generator=g))
    for k in range(f):
        U[n - f + k] += 0.03 * (1.0 + 0.02 * k) * d
    sizes = torch.tensor([300.0 + 37.0 * ((5 * i) % 7) for i in range(n)])
    return U, sizes


def svd_scores(U, cols):
    """The paper's form in parameter space, fp64: squared projections on the top right singular vector."""
    X = U[:, cols].double()
    Xc = X - X.mean(dim=0, keepdim=True)
    _, S, Vh = torch.linalg.svd(Xc, full_matrices=False)
    return (Xc @ Vh[0]) ** 2, S ** 2


@functools.lru_cache(maxsize=None)
def reference(n, f, P, b, seed=0):
    """fp64 reference of the ITERS iterations, computed once: (U, sizes, scores [ITERS, n], lambda_1 [ITERS]), after
    asserting that every iteration is well posed."""
    U, sizes = planted(n, f, P, seed)
    scores, lam = [], []
    for t in range(ITERS):
        s, ev = svd_scores(U, C.dnc_columns(P, b, t, SEED))
        l1, l2 = float(ev[0]), float(ev[1]) if len(ev) > 1 else 0.0
        assert l1 >= 4.0 * l2, (n, f, P, b, t, l1 / max(l2, 1e-300))
        srt = torch.sort(s, descending=True).values
        assert float(srt[f - 1] - srt[f]) >= 1e-3 * l1, (n, f, P, b, t, float(srt[f - 1] - srt[f]) / l1)
        scores.append(s)
        lam.append(l1)
    return U, sizes, torch.stack(scores), torch.tensor(lam, dtype=torch.float64)


def keep_masks(scores, drop):
    """Per-iteration keep masks from scores, written out the slow way: drop the ``drop`` largest (score, index)."""
    out = []
    for s in scores.tolist():
        key = sorted(range(len(s)), key=lambda i: (math.inf if s[i] != s[i] else s[i], i), reverse=True)
        gone = set(key[:drop])
        out.append([i not in gone for i in range(len(s))])
    return torch.tensor(out)


# ---------------------------------------------------------------------------------- column map
@pytest.mark.parametrize("P", [1, 2, 63, 4099])
def test_column_mirror(P):
    for b in sorted({1, max(P - 1, 1), P, P + 1}):
        cols = ops.dnc_columns(P, b, 0, SEED)
        assert cols.dtype == torch.int64 and cols.shape == (min(b, P),)
        assert int(cols.min()) >= 0 and int(cols.max()) < P
        assert len(set(cols.tolist())) == cols.numel()
        assert torch.equal(cols, ops.dnc_columns(P, b, 0, SEED))
        if b >= P:
            assert cols.tolist() == list(range(P))
    if P == 4099:
        a = ops.dnc_columns(P, 100, 0, SEED)
        assert not torch.equal(a, ops.dnc_columns(P, 100, 1, SEED))
        assert not torch.equal(a, ops.dnc_columns(P, 100, 0, SEED + 1))
        assert not torch.equal(a, ops.dnc_columns(P, 100, 0, SEED + (1 << 32)))  # (the seed's high word counts)
        assert a.tolist() != list(range(100))
        # a prefix of the same permutation: position order does not depend on b
        assert torch.equal(a[:10], ops.dnc_columns(P, 10, 0, SEED))
    with pytest.raises(ValueError):
        ops.dnc_columns(P, 0, 0, SEED)


# ---------------------------------------------------------------------------------- scores, planted rows
@pytest.mark.parametrize("n,f,P,b", SHAPES)
def test_scores_match_parameter_space_svd(n, f, P, b):
    U, sizes, ref, lam = reference(n, f, P, b)
    G = ops.dnc_gram(U, b, ITERS, SEED)
    assert G.shape == (ITERS, n, n) and G.dtype == torch.float64
    _, scores, _ = ops.dnc_select(G, f, sizes)
    worst = ((scores - ref).abs().max(dim=1).values / lam).max().item()
    print(f"dnc composite vs SVD n={n} P={P} b={b}: {worst:.3e} lambda_1")
    assert worst <= 1e-12


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("n,f,P,b", SHAPES)
def test_planted_rows_are_dropped(n, f, P, b, iters):
    U, sizes, ref, _ = reference(n, f, P, b)
    want = torch.arange(n) < n - f
    keep, scores, w = ops.dnc_filter(U, b, iters, SEED, f, sizes)
    assert keep.dtype == torch.bool and torch.equal(keep, want)
    assert scores.shape == (iters, n) and torch.equal(keep_masks(scores, f).all(dim=0), want)
    assert abs(float(w.sum()) - 1.0) <= 1e-12 and torch.equal(w > 0, want)
    if n >= 2 * f + 3:  # the rule itself, where byz-f admits this f
        res = agg.dnc(U, sizes, byz_f=f, dnc_iters=iters, dnc_sub_dim=b, seed=SEED)
        assert torch.equal(res.info["selected"], want) and res.info["f"] == f and res.info["drop"] == f
        assert torch.equal(res.info["scores"], scores)
        sw = sizes.double() * want
        mean = ((sw / sw.sum())[:, None] * U.double()).sum(dim=0)
        assert (res.params.double() - mean).abs().max().item() <= 1e-6 * max(1.0, mean.abs().max().item())


# ---------------------------------------------------------------------------------- ties, NaN
def check_ties_and_nan(dev):
    n = 6
    w = torch.ones(n, dtype=torch.float64)
    G = torch.diag(torch.tensor([3.0] + [1.0] * (n - 1), dtype=torch.float64)).to(dev)
    keep, scores, wt = ops.dnc_select(G, 2, w)  # (no centring: G is taken as it is)
    assert scores.cpu().tolist() == [[3.0, 0.0, 0.0, 0.0, 0.0, 0.0]]
    assert keep.cpu().tolist() == [False, True, True, True, True, False]  # the top row and the HIGHEST tied index
    assert wt.cpu().tolist() == [0.0, 0.25, 0.25, 0.25, 0.25, 0.0]
    keep, scores, _ = ops.dnc_select(torch.zeros(2, n, n, dtype=torch.float64, device=dev), 2, w)
    assert keep.cpu().tolist() == [True, True, True, True, False, False] and not bool(scores.any())
    # centring on request: the Gram of the rows centred on row 0 gives the scores of the mean-centred one
    U, sizes, ref, lam = reference(8, 2, 1025, 257)
    X = U[:, C.dnc_columns(1025, 257, 0, SEED)].double()
    H = ((X - X[0:1]) @ (X - X[0:1]).t()).to(dev)
    keep_c, scores_c, _ = ops.dnc_select(H, 2, sizes, centre=True)
    assert keep_c.cpu().tolist() == [True] * 6 + [False] * 2
    assert (scores_c.cpu()[0] - ref[0]).abs().max().item() <= 1e-9 * float(lam[0])
    # a NaN row: every score NaN (= +inf), the ranked drop falls back on the index, exactly n - drop rows per iteration
    U, sizes = planted(8, 2, 257)
    U = U.clone()
    U[3] = float("nan")
    for iters, drop in ((1, 2), (3, 2), (2, 7), (1, 0)):
        keep, scores, wt = ops.dnc_filter(U.to(dev), 100, iters, SEED, drop, sizes)
        assert scores.shape == (iters, 8) and bool(torch.isnan(scores).all())
        assert keep.cpu().tolist() == [i < 8 - drop for i in range(8)]
        assert keep_masks(scores.cpu(), drop).sum(dim=1).tolist() == [8 - drop] * iters
        assert bool((wt[keep] > 0).all()) and not bool(wt[~keep].any())


def test_tie_rule_and_nan():
    check_ties_and_nan("cpu")


# ---------------------------------------------------------------------------------- empty intersection
def empty_case():
    """7 benign rows, f = auto = 1, c = 100 -> drop = 6: each iteration keeps the one row with the smallest score."""
    g = torch.Generator().manual_seed(31)
    U = 0.3 * torch.randn(1, 300, generator=g) + 0.01 * torch.randn(7, 300, generator=g)
    sizes = torch.tensor([300.0 + 37.0 * ((5 * i) % 7) for i in range(7)])
    return U, sizes, dict(byz_f="auto", dnc_iters=8, dnc_sub_dim=50, dnc_c=100.0, seed=SEED)


def check_empty_intersection(dev):
    U, sizes, kw = empty_case()
    res = agg.dnc(U.to(dev), sizes, **kw)
    assert res.info["f"] == 1 and res.info["drop"] == 6
    masks = keep_masks(res.info["scores"].cpu(), 6)
    assert masks.sum(dim=1).tolist() == [1] * 8 and not bool(masks.all(dim=0).any())  # empty before the fallback
    assert res.info["selected"].cpu().tolist() == [True] * 7
    _, _, w = ops.dnc_filter(U.to(dev), 50, 8, SEED, 6, sizes)
    assert bool((w > 0).all()) and abs(float(w.sum()) - 1.0) <= 1e-12
    mean = ((sizes.double() / sizes.double().sum())[:, None] * U.double()).sum(dim=0)
    assert (res.params.double().cpu() - mean).abs().max().item() <= 1e-6 * max(1.0, mean.abs().max().item())


def test_empty_intersection_keeps_every_row():
    check_empty_intersection("cpu")


# ---------------------------------------------------------------------------------- config and dispatch
def test_registered_and_f0_is_fedavg():
    assert "dnc" in agg.AGGREGATORS and "dnc" in EARLY_AGGREGATORS
    U, sizes = planted(8, 2, 257)
    res = agg.dnc(U, sizes, byz_f=0)
    assert torch.equal(res.params, ops.fedavg(U, sizes)) and res.info["drop"] == 0
    assert res.info["selected"].tolist() == [True] * 8
    assert set(res.info) == {"selected", "f", "drop", "scores"}
    assert set(agg.dnc(U, sizes, byz_f=2).info) == set(res.info)
    auto = agg.dnc(U[:5], sizes[:5])  # auto f = (5 - 3) // 4 = 0
    assert auto.info["f"] == 0 and torch.equal(auto.params, ops.fedavg(U[:5], sizes[:5]))
    assert agg.dnc(U, sizes).info["f"] == 1
    assert agg.dnc(U, None, byz_f=1).info["drop"] == 1  # (no sizes: the unweighted mean)
    assert agg.dnc(U, sizes, byz_f=2, dnc_c=1.2).info["drop"] == 3  # ceil(c f)
    assert agg.dnc(U, sizes, byz_f=2, dnc_c=100.0).info["drop"] == 7  # capped at n - 1
    one = agg.dnc(U[:1], sizes[:1])
    assert torch.equal(one.params, U[0]) and one.params.data_ptr() != U.data_ptr()


def test_bad_arguments():
    U, sizes = planted(8, 2, 257)
    with pytest.raises(ValueError, match="dnc"):
        agg.dnc(U[:6], sizes[:6], byz_f=2)  # n >= 2 f + 3
    with pytest.raises(ValueError):
        agg.dnc(U, sizes, byz_f=-1)
    for kw in ({"dnc_iters": 0}, {"dnc_sub_dim": 0}, {"dnc_c": 0.0}, {"dnc_c": -1.0}, {"dnc_c": float("nan")}):
        with pytest.raises(ValueError):
            agg.dnc(U, sizes, **kw)


def test_config_keys():
    cfg = from_dict({"server": {"mode": "dnc"}})
    assert cfg.mode == "dnc"
    assert (cfg.engine["dnc-iters"], cfg.engine["dnc-sub-dim"], cfg.engine["dnc-c"]) == (1, 10000, 1.0)
    ok = from_dict({"server": {"mode": "dnc"}, "engine": {"dnc-iters": 3, "dnc-sub-dim": 1, "dnc-c": 2}})
    assert ok.engine["dnc-iters"] == 3
    for key, bad in (("dnc-iters", 0), ("dnc-iters", True), ("dnc-iters", 1.5), ("dnc-iters", "2"), ("dnc-sub-dim", 0),
                     ("dnc-sub-dim", -3), ("dnc-sub-dim", 2.0), ("dnc-c", 0), ("dnc-c", -0.5), ("dnc-c", "x"),
                     ("dnc-c", True), ("dnc-c", None)):
        with pytest.raises(ValueError, match=key):
            from_dict({"engine": {key: bad}})


# ---------------------------------------------------------------------------------- engine
def test_engine_two_rounds(tmp_path, monkeypatch):
    d = {
        "server": {"num-round": 2, "clients": 7, "mode": "dnc", "model": "TransformerModel",
                   "data-distribution": {"num-data-range": [150, 260]}},
        "learning": {"epoch": 1, "batch-size": 64},
        "data": {"synthetic": True, "train-size": 1500, "test-size": 400},
        "engine": {"checkpoint-dir": str(tmp_path), "trainer": "eager", "max-retries": 3, "dnc-iters": 2,
                   "dnc-sub-dim": 2000, "dnc-c": 1.5},
        "log_path": str(tmp_path),
    }
    seen = []
    orig = agg.AGGREGATORS["dnc"]

    def capture(U, sizes, **kw):
        seen.append(kw)
        return orig(U, sizes, **kw)

    monkeypatch.setitem(agg.AGGREGATORS, "dnc", capture)
    eng = FLEngine(from_dict(d), device="cpu", verbose=False)
    hist = eng.run()
    eng.close()
    assert [r["ok"] for r in hist] == [True, True] and all(0.0 <= r["metric"] <= 1.0 for r in hist)
    assert len(seen) == 2 and seen[0]["seed"] != seen[1]["seed"]  # a fresh column sub-sample every round
    for kw, r in zip(seen, hist):
        assert (kw["dnc_iters"], kw["dnc_sub_dim"], kw["dnc_c"], kw["byz_f"]) == (2, 2000, 1.5, "auto")
        assert r["f"] == 1 and r["drop"] == 2 and 3 <= len(r["selected"]) <= 5
