"""multi_krum, bulyan and geomed on the CPU: the composites of ``ops/composite.py`` against literal, loop-by-loop
statements of the rules' definitions (docs/PARITY.md, "beyond the reference") written here and sharing no code with
them; the tie rules; the config keys; two engine rounds per mode."""
import json
import math

import numpy as np
import pytest
import torch

from attackfl_amd import agg
from attackfl_amd.config import from_dict
from attackfl_amd.fl.engine import EARLY_AGGREGATORS, FLEngine
from attackfl_amd.ops import composite as C

CASES = [(7, 1, 257), (8, 1, 5000), (11, 2, 100), (15, 3, 1000), (5, 0, 7)]


def make_rows(n, f, P, seed=0):
    """base + 0.1 noise, the last f rows replaced by outliers (far from the benign cluster and from each other);
    non-uniform sizes."""
    g = torch.Generator().manual_seed(1000 * n + 10 * f + seed)
    U = torch.randn(1, P, generator=g) + 0.1 * torch.randn(n, P, generator=g)
    for r in range(n - f, n):
        U[r] = 3.0 * torch.randn(P, generator=g) + 2.0
    sizes = torch.tensor([300.0 + 37.0 * ((5 * i) % 7) for i in range(n)])
    return U, sizes


# ---------------------------------------------------------------------------------- literal statements
def lit_sqdist(U):
    X = U.double()
    n = X.shape[0]
    return [[float(((X[i] - X[j]) ** 2).sum()) if i != j else 0.0 for j in range(n)] for i in range(n)]


def lit_scores(D, active, f):
    m = len(active)
    k = max(m - f - 2, 1)
    out = {}
    for i in active:
        vals = sorted(D[i][j] for j in active if j != i)
        s = 0.0
        for v in vals[:k]:  # ascending order of value
            s += v
        out[i] = s
    return out


def lit_select(D, f, rounds, iterated):
    n = len(D)
    active = list(range(n))
    sel = []
    sc = first = None
    for t in range(rounds):
        if t == 0 or iterated:
            sc = lit_scores(D, active if iterated else list(range(n)), f)
            if t == 0:
                first = [sc[i] for i in range(n)]
        best = min(active, key=lambda i: (sc[i], i))
        sel.append(best)
        active.remove(best)
    return sel, first


def lit_multi_krum(U, sizes, f):
    n = U.shape[0]
    sel, _ = lit_select(lit_sqdist(U), f, n - f, False)
    tot = sum(float(sizes[i]) for i in sel)
    out = torch.zeros(U.shape[1], dtype=torch.float64)
    for i in sorted(sel):
        out += float(sizes[i]) / tot * U[i].double()
    return sorted(sel), out


def lit_bulyan_column(vals, beta):
    xs = sorted(np.float32(v) for v in vals)
    med = xs[(len(xs) - 1) // 2]
    keyed = sorted(xs, key=lambda x: (np.float32(abs(np.float32(x - med))), x))
    return sum(float(x) for x in keyed[:beta]) / beta


def lit_bulyan(U, f):
    n = U.shape[0]
    theta = n - 2 * f
    sel, _ = lit_select(lit_sqdist(U), f, theta, True)
    cols = U[sel].numpy()
    out = [lit_bulyan_column(cols[:, c], theta - 2 * f) for c in range(U.shape[1])]
    return sel, torch.tensor(out, dtype=torch.float64)


def weiszfeld_param_space(U, sizes, iters=100, nu=1e-6):
    """Smoothed Weiszfeld on the rows themselves (fp64): the reference of the Gram-space form."""
    X = U.double()
    a = sizes.double() / sizes.double().sum()
    z = (a[:, None] * X).sum(0)
    prev = math.inf
    for _ in range(iters):
        d = torch.linalg.vector_norm(X - z[None, :], dim=1)
        obj = float((a * d).sum())
        b = a / d.clamp_min(nu)
        b = b / b.sum()
        z = (b[:, None] * X).sum(0)
        if abs(obj - prev) <= 1e-9 * obj:
            break
        prev = obj
    return z, b


def close(got, ref, tol):
    return (got.double() - ref.double()).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


# ---------------------------------------------------------------------------------- composites against the statements
@pytest.mark.parametrize("n,f,P", CASES)
def test_multi_krum_matches_literal_statement(n, f, P):
    U, sizes = make_rows(n, f, P)
    res = agg.multi_krum(U, sizes, byz_f=f)
    sel, ref = lit_multi_krum(U, sizes, f)
    got_sel = torch.nonzero(res.info["selected"]).reshape(-1).tolist()
    assert got_sel == sel and res.info["f"] == f
    assert all(r not in got_sel for r in range(n - f, n))  # the outliers are excluded
    assert close(res.params, ref, 1e-6)
    _, first = lit_select(lit_sqdist(U), f, n - f, False)
    assert torch.allclose(res.info["scores"], torch.tensor(first, dtype=torch.float64), rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("n,f,P", CASES)
def test_bulyan_matches_literal_statement(n, f, P):
    U, sizes = make_rows(n, f, P)
    res = agg.bulyan(U, sizes, byz_f=f)
    sel, ref = lit_bulyan(U, f)
    got_sel = torch.nonzero(res.info["selected"]).reshape(-1).tolist()
    assert got_sel == sorted(sel) and len(sel) == n - 2 * f
    assert all(r not in got_sel for r in range(n - f, n))  # the outliers are excluded
    # the composite's selection ORDER too (the coordinate step does not depend on it, the kernel's output does)
    order, _, _ = C.krum_select(C.pairwise_l2(U) ** 2, f, n - 2 * f, True)
    assert order.tolist() == sel
    assert close(res.params, ref, 1e-6)
    if f >= 1:
        # not vacuous: with an outlier row the plain mean is off by O(1) somewhere, and the mean of the beta values
        # next to the median differs from the median and from the mean of all theta selected values by a sizeable
        # fraction of the 0.1 noise in at least one of >= 100 columns
        S = U[sel]
        for other in (U.mean(0), U.median(0).values, S.mean(0)):
            assert (res.params - other).abs().max().item() > 0.01


@pytest.mark.parametrize("n,f,P", CASES + [(5, 0, 64)])
def test_geomed_matches_parameter_space_weiszfeld(n, f, P):
    U, sizes = make_rows(n, f, P)
    if P == 64:  # three identical rows: their distance to the iterate can reach the smoothing floor
        U[1] = U[0]
        U[2] = U[0]
    res = agg.geomed(U, sizes)
    ref, b = weiszfeld_param_space(U, sizes)
    assert close(res.params, ref, 2e-5)
    w = res.info["weights"]
    assert abs(float(w.sum()) - 1.0) <= 1e-12
    if P != 64:  # (identical rows may share their joint weight differently)
        assert torch.allclose(w, b, rtol=1e-6, atol=1e-12)
    assert 1 <= int(res.info["iters"]) <= 100 and float(res.info["objective"]) >= 0.0
    if f >= 1:  # an outlier's weight falls below its FedAvg share
        a = sizes.double() / sizes.double().sum()
        assert all(float(w[r]) < float(a[r]) for r in range(n - f, n))


# ---------------------------------------------------------------------------------- tie rules
def test_equal_scores_go_to_the_lower_index():
    g = torch.Generator().manual_seed(5)
    U = 0.1 * torch.randn(6, 40, generator=g)
    U[3] = U[1]  # rows 1 and 3 identical and central: equal scores, the smallest
    U[1] *= 0.0
    U[3] *= 0.0
    D = C.pairwise_l2(U) ** 2
    for iterated in (False, True):
        sel, mask, scores = C.krum_select(D, 1, 4, iterated)
        assert float(scores[1]) == float(scores[3])
        assert float(scores[1]) == float(scores.min())
        assert sel[0].item() == 1
        lit, first = lit_select(D.tolist(), 1, 4, iterated)
        assert sel.tolist() == lit and scores.tolist() == first
        assert torch.nonzero(mask).reshape(-1).tolist() == sorted(lit)
    sel, _, _ = C.krum_select(D, 1, 4, False)
    assert sel.tolist()[:2] == [1, 3]
    # a single row: score 0, selected
    sel, mask, scores = C.krum_select(torch.zeros(1, 1, dtype=torch.float64), 0, 1, True)
    assert sel.tolist() == [0] and mask.tolist() == [True] and scores.tolist() == [0.0]


@pytest.mark.parametrize("seed", range(8))
def test_bulyan_last_picks_tie_between_mutual_nearest_rows(seed):
    """Benign rows only.  At Bulyan's last picks k = 1: the two rows that are each other's nearest neighbour have the
    same score, D[i][j], and the lower index goes — also when D comes out of a matrix product whose two halves
    differ in the last bit (the composite reads D as symmetric)."""
    U, sizes = make_rows(7, 0, 300, seed)
    lit, _ = lit_select(lit_sqdist(U), 1, 5, True)
    D = C.pairwise_l2(U) ** 2
    assert C.krum_select(D, 1, 5, True)[0].tolist() == lit
    assert C.krum_select(torch.triu(D, 1) + torch.tril(D, -1) * (1.0 + 1e-12), 1, 5, True)[0].tolist() == lit
    res = agg.bulyan(U, sizes, byz_f=1)
    assert torch.nonzero(res.info["selected"]).reshape(-1).tolist() == sorted(lit)
    assert close(res.params, lit_bulyan(U, 1)[1], 1e-6)


def test_equidistant_neighbours_keep_the_smaller_value():
    # column 0: 1..5, median 3: 2 and 4 (then 1 and 5) are equidistant, the smaller one is taken
    # column 1: no tie (median 0, neighbours -1 and 3)
    U = torch.tensor([[4.0, 3.0], [1.0, -8.0], [5.0, 0.0], [2.0, -1.0], [3.0, 9.0], [100.0, 100.0]])
    sel = torch.tensor([0, 1, 2, 3, 4])
    assert C.bulyan_coord(U, sel, 1).tolist() == [3.0, 0.0]
    assert C.bulyan_coord(U, sel, 2).tolist() == [2.5, -0.5]
    assert C.bulyan_coord(U, sel, 3).tolist() == [3.0, pytest.approx(2.0 / 3.0, rel=1e-6)]
    assert C.bulyan_coord(U, sel, 4).tolist() == [2.5, pytest.approx((0.0 - 1.0 + 3.0 - 8.0) / 4.0, rel=1e-6)]
    assert C.bulyan_coord(U, sel, 5).tolist() == [3.0, pytest.approx(0.6, rel=1e-6)]
    for beta in range(1, 6):
        for c in range(2):
            assert float(C.bulyan_coord(U, sel, beta)[c]) == pytest.approx(lit_bulyan_column(U[:5, c].tolist(), beta),
                                                                           rel=1e-6)


# ---------------------------------------------------------------------------------- config
def test_config_keys_and_byzantine_count():
    for mode in ("multi_krum", "bulyan", "geomed"):
        cfg = from_dict({"server": {"mode": mode}, "engine": {"byz-f": 2, "geomed-iters": 50, "geomed-nu": 1e-5}})
        assert cfg.mode == mode and cfg.engine["byz-f"] == 2 and cfg.engine["geomed-iters"] == 50
        assert mode in agg.AGGREGATORS and mode in EARLY_AGGREGATORS
    d = from_dict({}).engine
    assert d["byz-f"] == "auto" and d["geomed-iters"] == 100 and d["geomed-nu"] == 1e-6
    for bad in (-1, 1.5, "two", True):
        with pytest.raises(ValueError):
            from_dict({"engine": {"byz-f": bad}})
    with pytest.raises(ValueError):
        from_dict({"engine": {"geomed-iters": 0}})
    with pytest.raises(ValueError):
        from_dict({"engine": {"geomed-nu": 0.0}})
    assert agg.byzantine_count(7) == 1 and agg.byzantine_count(8) == 1 and agg.byzantine_count(6) == 0
    U = torch.randn(6, 9, generator=torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match=r"n = 6.*4 f \+ 3 = 7"):
        agg.bulyan(U, torch.ones(6), byz_f=1)
    with pytest.raises(ValueError, match=r"n = 6.*2 f \+ 3 = 7"):
        agg.multi_krum(U, torch.ones(6), byz_f=2)
    assert agg.multi_krum(U, torch.ones(6), byz_f=1).info["f"] == 1
    assert agg.bulyan(U, torch.ones(6)).info["f"] == 0  # auto
    # krum keeps the reference's f = 0 (A-11)
    assert agg.krum(U, torch.ones(6), byz_f=1).info["f"] == 0


# ---------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("mode", ["multi_krum", "bulyan", "geomed"])
def test_cpu_engine_rounds(tmp_path, mode):
    d = {
        "server": {"num-round": 2, "clients": 7, "mode": mode, "model": "TransformerModel",
                   "data-distribution": {"num-data-range": [300, 500]}},
        "learning": {"epoch": 1, "batch-size": 128},
        "data": {"synthetic": True, "train-size": 4000, "test-size": 500},
        "engine": {"checkpoint-dir": str(tmp_path), "trainer": "eager", "max-retries": 3,
                   "metrics": str(tmp_path / "m.jsonl")},
        "comm": {"attackers": {6: {"mode": "Min-Max", "round": 2}}},
        "log_path": str(tmp_path),
    }
    eng = FLEngine(from_dict(d), device="cpu", verbose=False)
    hist = eng.run()
    eng.close()
    assert [r["ok"] for r in hist] == [True, True]
    assert all(0.0 <= r["metric"] <= 1.0 for r in hist)
    recs = [json.loads(line) for line in open(tmp_path / "m.jsonl")]
    assert len(recs) == 2
    for r in recs:
        if mode == "geomed":
            assert len(r["weights"]) == 7 and abs(sum(r["weights"]) - 1.0) < 1e-9 and r["iters"] >= 1
        else:
            assert r["f"] == 1 and len(r["selected"]) == (6 if mode == "multi_krum" else 5)
            assert all(0 <= i < 7 for i in r["selected"])
