"""multi_krum, bulyan and geomed on the device: ``k_krum_select`` against its host mirror (exact), ``k_bulyan_coord``
against the CPU composite on the same selection, ``k_geomed_weights`` + ``weighted_rows`` against parameter-space
Weiszfeld in fp64, bit-reproducibility, and the engine (captured rounds against the composites; the early launch
against the serial schedule)."""
import math

import pytest
import torch

from attackfl_amd import agg, ops
from attackfl_amd.config import from_dict
from attackfl_amd.fl.engine import EARLY_AGGREGATORS, FLEngine, build_client_table
from attackfl_amd.ops import composite as C
from launch import parse_attackers

pytestmark = pytest.mark.gpu

MODES = ("multi_krum", "bulyan", "geomed")
TOL = {"multi_krum": 1e-6, "bulyan": 1e-6, "geomed": 2e-5}


def make_rows(n, f, P, seed=0):
    g = torch.Generator().manual_seed(1000 * n + 10 * f + seed)
    U = torch.randn(1, P, generator=g) + 0.1 * torch.randn(n, P, generator=g)
    for r in range(n - f, n):
        U[r] = 3.0 * torch.randn(P, generator=g) + 2.0
    sizes = torch.tensor([300.0 + 37.0 * ((5 * i) % 7) for i in range(n)])
    return U, sizes


def close(got, ref, tol):
    return (got.double().cpu() - ref.double()).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


# ---------------------------------------------------------------------------------- krum_select
def mirror_select(D, f, rounds, iterated):
    """Host mirror of k_krum_select on the device's own D: the same ascending-order fp64 sums."""
    n = len(D)
    D = [[D[min(i, j)][max(i, j)] for j in range(n)] for i in range(n)]  # (read as symmetric, like the kernel)
    active = list(range(n))
    sel, sc, first = [], None, None
    for t in range(rounds):
        if t == 0 or iterated:
            rows = active if iterated else list(range(n))
            k = max(len(rows) - f - 2, 1)
            sc = {}
            for i in rows:
                s = 0.0
                for v in sorted(D[i][j] for j in rows if j != i)[:k]:
                    s += v
                sc[i] = s
            if t == 0:
                first = [sc[i] for i in range(n)]
        best = min(active, key=lambda i: (sc[i], i))
        sel.append(best)
        active.remove(best)
    return sel, first


def check_select(D_dev, f, rounds, iterated):
    sel, mask, scores = ops.krum_select(D_dev, f, rounds, iterated)
    assert sel.dtype == torch.int32 and mask.dtype == torch.bool and scores.dtype == torch.float64
    ref_sel, ref_scores = mirror_select(D_dev.cpu().tolist(), f, rounds, iterated)
    assert sel.cpu().tolist() == ref_sel, (f, rounds, iterated)
    assert torch.nonzero(mask).reshape(-1).cpu().tolist() == sorted(ref_sel)
    assert scores.cpu().tolist() == ref_scores
    return ref_sel


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 33, 64])
def test_krum_select_matches_host_mirror(gpu, n):
    U, _ = make_rows(n, max(0, (n - 3) // 4), 300)
    D = ops.pairwise_sqdist(U.to(gpu))
    for f in range(0, max(0, (n - 3) // 2) + 1):  # one-shot ranking: n >= 2 f + 3
        check_select(D, f, n - f, False)
    for f in range(0, max(0, (n - 3) // 4) + 1):  # iterated selection: n >= 4 f + 3
        check_select(D, f, n - 2 * f, True)
    check_select(D, 0, 1, False)  # (plain Krum with the first pick only)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_bulyan_last_picks_tie_between_mutual_nearest_rows(gpu, seed):
    """Benign rows only: at the last picks k = 1, so the two rows that are each other's nearest neighbour tie exactly
    and the lower index goes; the device selection order is the composite's (whose D comes from a matrix product
    that is not symmetric to the last bit)."""
    U, _ = make_rows(7, 0, 300, seed)
    D = ops.pairwise_sqdist(U.to(gpu))
    want, _, _ = C.krum_select(C.pairwise_l2(U) ** 2, 1, 5, True)
    assert check_select(D, 1, 5, True) == want.tolist()
    Dl = D.clone()
    Dl.tril_(-1).mul_(1.0 + 1e-12)  # a lower triangle off by a few bits changes nothing
    assert ops.krum_select(D.triu(1) + Dl, 1, 5, True)[0].cpu().tolist() == want.tolist()


def test_krum_select_ties_and_bad_arguments(gpu):
    g = torch.Generator().manual_seed(5)
    U = 0.1 * torch.randn(6, 40, generator=g)
    U[1] = 0.0
    U[3] = 0.0  # rows 1 and 3 identical and central: equal (smallest) scores, the lower index goes first
    D = ops.pairwise_sqdist(U.to(gpu))
    assert check_select(D, 1, 4, False)[:2] == [1, 3]
    assert check_select(D, 1, 4, True)[0] == 1
    scores = ops.krum_select(D, 1, 4, False)[2]
    assert float(scores[1]) == float(scores[3]) == float(scores.min())
    for f, rounds in ((0, 7), (0, 0), (-1, 3), (7, 3)):  # the launcher refuses instead of launching
        with pytest.raises(RuntimeError):
            ops.native().krum_select(D, f, rounds, False)
    with pytest.raises(RuntimeError):
        ops.native().krum_select(torch.zeros(65, 65, dtype=torch.float64, device=gpu), 0, 1, False)


# ---------------------------------------------------------------------------------- bulyan_coord
# (33, 4, 129): theta = 25, the 32-value variant of the kernel, which the other cases do not reach
@pytest.mark.parametrize("n,f,P", [(3, 0, 7), (7, 1, 257), (8, 1, 47693), (15, 3, 1000), (64, 15, 100), (33, 4, 129)])
def test_bulyan_coord_matches_composite(gpu, n, f, P):
    U, _ = make_rows(n, f, P)
    theta, beta = n - 2 * f, n - 4 * f
    sel, _, _ = C.krum_select(C.pairwise_l2(U) ** 2, f, theta, True)
    ref = C.bulyan_coord(U, sel, beta)
    got = ops.bulyan_coord(U.to(gpu), sel.to(gpu), beta)
    assert close(got, ref, 1e-6)
    assert torch.equal(got, ops.bulyan_coord(U.to(gpu), sel.to(gpu), beta))
    # the whole rule: the device selection is the composite's, so is the aggregate
    Ud = U.to(gpu)
    res = agg.bulyan(Ud, torch.ones(n), byz_f=f)
    assert torch.nonzero(res.info["selected"]).reshape(-1).cpu().tolist() == sorted(sel.tolist())
    assert close(res.params, ref, 1e-6)
    assert res.params.untyped_storage().data_ptr() != Ud.untyped_storage().data_ptr()  # never a row of U


def test_bulyan_coord_equidistant_tie(gpu):
    U = torch.tensor([[4.0, 3.0], [1.0, -8.0], [5.0, 0.0], [2.0, -1.0], [3.0, 9.0], [100.0, 100.0]])
    sel = torch.tensor([0, 1, 2, 3, 4])
    for beta, want0 in ((1, 3.0), (2, 2.5), (3, 3.0), (4, 2.5), (5, 3.0)):
        got = ops.bulyan_coord(U.to(gpu), sel.to(gpu), beta).cpu()
        assert float(got[0]) == want0
        assert close(got, C.bulyan_coord(U, sel, beta), 1e-6)
    # the index list is honoured in any order, and a bad one is refused
    assert torch.equal(ops.bulyan_coord(U.to(gpu), sel.flip(0).to(gpu), 3), ops.bulyan_coord(U.to(gpu), sel.to(gpu), 3))
    with pytest.raises(RuntimeError):
        ops.native().bulyan_coord(U.to(gpu), sel.to(gpu, torch.int32), 6)
    with pytest.raises(RuntimeError):
        ops.native().bulyan_coord(U[:3].to(gpu).contiguous(), sel.to(gpu, torch.int32), 2)


# ---------------------------------------------------------------------------------- geomed
def weiszfeld_param_space(U, sizes, iters=100, nu=1e-6):
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
    return z


@pytest.mark.parametrize("n,P,same", [(3, 7, False), (5, 257, False), (8, 47693, False), (37, 100, False),
                                      (64, 1000, False), (5, 64, True)])
def test_geomed_matches_parameter_space_weiszfeld(gpu, n, P, same):
    U, sizes = make_rows(n, max(0, (n - 3) // 4), P)
    if same:  # three identical rows
        U[1] = U[0]
        U[2] = U[0]
    res = agg.geomed(U.to(gpu), sizes)
    assert close(res.params, weiszfeld_param_space(U, sizes), 2e-5)
    w = res.info["weights"]
    assert w.dtype == torch.float64 and abs(float(w.sum()) - 1.0) <= 1e-12 and bool((w >= 0).all())
    assert 1 <= int(res.info["iters"]) <= 100
    again = agg.geomed(U.to(gpu), sizes)
    assert torch.equal(again.params, res.params) and torch.equal(again.info["weights"], w)
    assert int(again.info["iters"]) == int(res.info["iters"])
    assert float(again.info["objective"]) == float(res.info["objective"])
    one = agg.geomed(U.to(gpu), sizes, geomed_iters=1)  # one iteration: the bound is honoured
    assert int(one.info["iters"]) == 1


def test_geomed_weights_bad_arguments(gpu):
    G = torch.eye(4, dtype=torch.float64, device=gpu)
    a = torch.full((4,), 0.25, dtype=torch.float64, device=gpu)
    for iters, nu in ((0, 1e-6), (10, 0.0), (10, -1.0)):
        with pytest.raises(RuntimeError):
            ops.native().geomed_weights(G, a, iters, nu)
    with pytest.raises(RuntimeError):
        ops.native().geomed_weights(G, a[:3].contiguous(), 10, 1e-6)


@pytest.mark.parametrize("n,f,P", [(7, 1, 257), (8, 1, 47693), (33, 7, 100)])
def test_multi_krum_matches_composite_and_is_deterministic(gpu, n, f, P):
    U, sizes = make_rows(n, f, P)
    ref = agg.multi_krum(U, sizes, byz_f=f)
    res = agg.multi_krum(U.to(gpu), sizes, byz_f=f)
    assert torch.equal(res.info["selected"].cpu(), ref.info["selected"])
    assert not bool(res.info["selected"][n - f:].any())
    assert close(res.params, ref.params, 1e-6)
    again = agg.multi_krum(U.to(gpu), sizes.to(gpu), byz_f=f)  # (sizes on the device: the several-rank path)
    assert torch.equal(again.params, res.params) and torch.equal(again.info["scores"], res.info["scores"])


# ---------------------------------------------------------------------------------- engine
def _engine(tmp_path, mode, rounds, sub, **engine_kw):
    d = {
        "server": {"num-round": rounds, "clients": 7, "mode": mode, "model": "TransformerModel", "data-name": "ICU",
                   "genuine-rate": 1.0, "random-seed": 11, "data-distribution": {"num-data-range": [300, 500]}},
        "learning": {"epoch": 2, "batch-size": 128},
        "data": {"synthetic": True, "train-size": 4000, "test-size": 1000},
        "engine": {"checkpoint-dir": str(tmp_path / sub), "trainer": "auto", "seed": 3, **engine_kw},
        "log_path": str(tmp_path / sub),
    }
    cfg = from_dict(d)
    return FLEngine(cfg, device="cuda", table=build_client_table(cfg, 1, parse_attackers("6:Min-Max:2")),
                    verbose=False)


@pytest.mark.parametrize("mode", MODES)
def test_new_modes_end_to_end(gpu, tmp_path, monkeypatch, mode):
    """7 clients, f auto (= 1), one Min-Max attacker from round 2, fused trainer: every round's device aggregate and
    selection against the CPU composite on the captured rows; the rule runs in the early launch."""
    eng = _engine(tmp_path, mode, 3, "e2e")
    assert eng.trainer.kind == "fused" and mode in EARLY_AGGREGATORS
    seen = []
    orig_fn = agg.AGGREGATORS[mode]

    def capture(U, sizes, **kw):
        rows = U.detach().cpu().clone()
        res = orig_fn(U, sizes, **kw)
        seen.append((rows, sizes.detach().cpu().clone(), res.params.detach().cpu().clone(), kw))
        return res

    monkeypatch.setitem(agg.AGGREGATORS, mode, capture)
    hist = eng.run()
    eng.close()
    assert [r["ok"] for r in hist] == [True, True, True] and len(seen) == 3
    assert any(r.get("path") == "early-launch" for r in hist)
    assert all(0.0 <= r["metric"] <= 1.0 for r in hist)
    assert "attack" in hist[1] and "attack" in hist[2]
    for k, (rows, sizes, got, kw) in enumerate(seen):
        assert kw["byz_f"] == "auto" and kw["geomed_iters"] == 100 and kw["geomed_nu"] == 1e-6
        ref = orig_fn(rows, sizes, **kw)
        assert close(got, ref.params, TOL[mode]), (mode, k)
        if mode == "geomed":
            assert len(hist[k]["weights"]) == 7 and abs(sum(hist[k]["weights"]) - 1.0) <= 1e-9
        else:  # the selection the round recorded is the composite's on the same rows (attacker in or out alike)
            assert hist[k]["f"] == 1
            assert hist[k]["selected"] == torch.nonzero(ref.info["selected"]).reshape(-1).tolist(), (mode, k)


@pytest.mark.parametrize("mode", MODES)
def test_early_launch_matches_serial_schedule(gpu, tmp_path, mode):
    def run(spec, sub):
        eng = _engine(tmp_path, mode, 4, sub, speculative=spec)
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
