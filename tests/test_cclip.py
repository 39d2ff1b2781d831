"""Centred clipping (``agg.cclip``) on the CPU: the Gram-space composites of ``ops/composite.py`` against a literal
parameter-space statement of the rule (docs/PARITY.md, "beyond the reference") written here in fp64 and sharing no
code with them; the rule's limits; non-finite rows; the config keys; two engine rounds."""
import json
import math

import pytest
import torch

from attackfl_amd import agg, ops
from attackfl_amd.config import from_dict
from attackfl_amd.fl.engine import EARLY_AGGREGATORS, FLEngine

SHAPES = [(1, 7), (2, 5), (3, 7), (5, 257), (8, 47693), (37, 100), (64, 1000), (65, 33)]
ITERS = (1, 3, 10)
TAUS = ("auto", 1.0)


def make_rows(n, P, seed=0):
    """base + 0.1 noise, the last f = (n - 3) // 4 rows replaced by outliers, non-uniform sizes; the centre is
    base + 0.05 noise (the model the round started from: close to the benign rows, not among them)."""
    f = max(0, (n - 3) // 4)
    g = torch.Generator().manual_seed(1000 * n + 10 * f + seed)
    base = torch.randn(1, P, generator=g)
    U = base + 0.1 * torch.randn(n, P, generator=g)
    for r in range(n - f, n):
        U[r] = 3.0 * torch.randn(P, generator=g) + 2.0
    sizes = torch.tensor([300.0 + 37.0 * ((5 * i) % 7) for i in range(n)])
    centre = base[0] + 0.05 * torch.randn(P, generator=g)
    return U, sizes, centre


def cclip_param_space(U, sizes, centre, iters, tau, skip=()):
    """The rule on the rows themselves, one statement per line of its text -> (v fp64, tau, clipped in the last
    iteration, s of the first iteration).  ``skip``: rows left out of every sum and of the median (alpha as it was)."""
    X = U.double()
    n = X.shape[0]
    a = [1.0 / n] * n if sizes is None else [float(s) / float(sizes.double().sum()) for s in sizes]
    rows = [i for i in range(n) if i not in skip]
    if centre is not None:
        v = centre.double().clone()
    else:
        v = torch.zeros(X.shape[1], dtype=torch.float64)
        for i in rows:
            v += a[i] * X[i]
    t, clipped, first = tau, 0, None
    for it in range(iters):
        d = {i: float(torch.linalg.vector_norm(X[i] - v)) for i in rows}
        if it == 0 and tau == "auto":
            vals = sorted(d[i] for i in rows)
            t = vals[(len(vals) - 1) // 2] if vals else 0.0
        s = {i: 1.0 if d[i] <= t else t / d[i] for i in rows}
        step = torch.zeros_like(v)
        for i in rows:
            step += a[i] * s[i] * (X[i] - v)
        v = v + step
        clipped = sum(1 for i in rows if s[i] < 1.0)
        first = s if it == 0 else first
    return v, t, clipped, first


def close(got, ref, tol):
    return (got.double() - ref.double()).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


_ROWS = {}


def rows_of(n, P):
    if (n, P) not in _ROWS:
        _ROWS[(n, P)] = make_rows(n, P)
    return _ROWS[(n, P)]


# ---------------------------------------------------------------------------------- the rule against its statement
@pytest.mark.parametrize("anchored", [True, False])
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("n,P", SHAPES)
def test_cclip_matches_parameter_space_loop(n, P, iters, tau, anchored):
    U, sizes, centre = rows_of(n, P)
    centre = centre if anchored else None
    keep = (U.clone(), centre.clone() if anchored else None)
    res = agg.cclip(U, sizes, centre=centre, cclip_iters=iters, cclip_tau=tau)
    ref, t, clipped, _ = cclip_param_space(U, sizes, centre, iters, tau)
    assert res.params.dtype == torch.float32 and close(res.params, ref, 1e-6)
    info = agg.host_info(res.info)
    assert info["iters"] == iters and len(info["weights"]) == n
    assert info["tau"] == pytest.approx(t, rel=1e-9) and isinstance(info["clipped"], int)
    assert all(-1e-15 <= w <= 1.0 + 1e-15 for w in info["weights"])
    if not anchored:
        assert abs(sum(info["weights"]) - 1.0) <= 1e-12  # (c0 = alpha and the update keep sum c = 1)
    if iters == 1:
        assert info["clipped"] == clipped
    # the inputs are untouched and the result is a new tensor
    assert torch.equal(U, keep[0]) and (not anchored or torch.equal(centre, keep[1]))
    assert res.params.untyped_storage().data_ptr() != U.untyped_storage().data_ptr()
    assert not anchored or res.params.untyped_storage().data_ptr() != centre.untyped_storage().data_ptr()


def test_inputs_exercise_both_branches():
    """(8, 47693), a centre, auto tau, one iteration: the median rule clips the rows beyond the lower median and
    leaves the others whole, so the comparison above cannot pass with the clipping switched off."""
    U, sizes, centre = rows_of(8, 47693)
    res = agg.cclip(U, sizes, centre=centre, cclip_iters=1, cclip_tau="auto")
    _, t, clipped, s = cclip_param_space(U, sizes, centre, 1, "auto")
    assert any(v < 1.0 for v in s.values()) and any(v == 1.0 for v in s.values())
    assert int(res.info["clipped"]) == clipped == 4
    assert float(res.info["tau"]) == pytest.approx(t, rel=1e-9) and t > 0.0
    assert not close(res.params, ops.fedavg(U, sizes), 1e-3)  # (FedAvg follows the outlier row)


def test_uniform_weights_when_sizes_is_none():
    U, _, centre = rows_of(5, 257)
    for c in (centre, None):
        res = agg.cclip(U, None, centre=c, cclip_iters=3, cclip_tau=1.0)
        assert close(res.params, cclip_param_space(U, None, c, 3, 1.0)[0], 1e-6)


# ---------------------------------------------------------------------------------- limits
@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("anchored", [True, False])
def test_huge_radius_is_fedavg(iters, anchored):
    for n, P in ((5, 257), (37, 100)):
        U, sizes, centre = rows_of(n, P)
        res = agg.cclip(U, sizes, centre=centre if anchored else None, cclip_iters=iters, cclip_tau=1e30)
        assert close(res.params, ops.fedavg(U, sizes), 1e-6)
        assert int(res.info["clipped"]) == 0


def test_one_iteration_is_norm_bounding():
    for n, P in ((5, 257), (37, 100)):
        U, sizes, centre = rows_of(n, P)
        X, g, a = U.double(), centre.double(), sizes.double() / sizes.double().sum()
        for tau in (0.5, 1.0, 3.0):
            nb = g + (a * (tau / torch.linalg.vector_norm(X - g, dim=1)).clamp_max(1.0))[:, None].mul(X - g).sum(0)
            res = agg.cclip(U, sizes, centre=centre, cclip_iters=1, cclip_tau=tau)
            assert close(res.params, nb, 1e-6)


def test_small_radius_bounds_the_step():
    """tau far below every distance, one iteration: every row is clipped to length tau, so the centre moves by at
    most sum alpha_i tau = tau (plus the fp32 rounding of the result, at most 2^-24 per unit of each coordinate)."""
    U, sizes, centre = rows_of(37, 100)
    tau = 1e-3
    assert float(torch.linalg.vector_norm(U.double() - centre.double(), dim=1).min()) > 100 * tau
    res = agg.cclip(U, sizes, centre=centre, cclip_iters=1, cclip_tau=tau)
    assert int(res.info["clipped"]) == 37
    moved = float(torch.linalg.vector_norm(res.params.double() - centre.double()))
    assert 0.0 < moved <= tau + 2.0 ** -24 * float(torch.linalg.vector_norm(res.params.double()))


# ---------------------------------------------------------------------------------- non-finite rows
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("bad", [0, 3, 7])
def test_nan_row_with_a_centre_is_left_out(bad, tau):
    U, sizes, centre = rows_of(8, 257)
    U = U.clone()
    U[bad] = float("nan")
    res = agg.cclip(U, sizes, centre=centre, cclip_iters=3, cclip_tau=tau)
    ref, t, _, _ = cclip_param_space(U, sizes, centre, 3, tau, skip=(bad,))
    assert bool(torch.isfinite(res.params).all()) and close(res.params, ref, 1e-6)
    w = res.info["weights"]
    assert float(w[bad]) == 0.0 and bool(torch.isfinite(w).all())
    assert float(res.info["tau"]) == pytest.approx(t, rel=1e-9)


def test_all_rows_nan_gives_the_centre():
    U, sizes, centre = rows_of(5, 257)
    res = agg.cclip(torch.full_like(U, float("nan")), sizes, centre=centre)
    assert torch.equal(res.params, centre)
    assert res.params.untyped_storage().data_ptr() != centre.untyped_storage().data_ptr()
    assert res.info["weights"].tolist() == [0.0] * 5 and int(res.info["clipped"]) == 0


def test_nan_row_without_a_centre_is_not_finite():
    U, sizes, _ = rows_of(5, 257)
    U = U.clone()
    U[2] = float("nan")
    for tau in TAUS:
        assert not bool(torch.isfinite(agg.cclip(U, sizes, centre=None, cclip_tau=tau).params).any())


# ---------------------------------------------------------------------------------- config
def test_config_keys():
    d = from_dict({}).engine
    assert d["cclip-iters"] == 3 and d["cclip-tau"] == "auto"
    cfg = from_dict({"server": {"mode": "cclip"}, "engine": {"cclip-iters": 1, "cclip-tau": 0.5}})
    assert cfg.mode == "cclip" and cfg.engine["cclip-iters"] == 1 and cfg.engine["cclip-tau"] == 0.5
    assert "cclip" in agg.AGGREGATORS and "cclip" in EARLY_AGGREGATORS
    for good in ("auto", 2, 1e-3, "1e-3"):  # (YAML 1.1 reads 1e-3, without a dot, as a string)
        from_dict({"engine": {"cclip-tau": good}})
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            from_dict({"engine": {"cclip-iters": bad}})
    for bad in (0, -1, "x", True):
        with pytest.raises(ValueError):
            from_dict({"engine": {"cclip-tau": bad}})
    U, sizes, centre = rows_of(5, 257)
    for kw in ({"cclip_iters": 0}, {"cclip_tau": 0.0}, {"cclip_tau": -1.0}, {"cclip_tau": float("nan")}):
        with pytest.raises(ValueError):
            agg.cclip(U, sizes, centre=centre, **kw)


# ---------------------------------------------------------------------------------- engine
def test_cpu_engine_rounds(tmp_path):
    d = {
        "server": {"num-round": 2, "clients": 7, "mode": "cclip", "model": "TransformerModel",
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
        assert len(r["weights"]) == 7 and all(math.isfinite(w) for w in r["weights"])
        assert r["tau"] > 0.0 and 0 <= r["clipped"] <= 7 and r["iters"] == 3
