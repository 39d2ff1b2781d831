"""Pre-aggregation (``agg.nnm``, ``agg.bucketing``; docs/PARITY.md) on the CPU: the composites of ``ops/composite.py``
against a literal parameter-space statement of the two rules written here in fp64 and sharing no code with them; the
rules' invariants; the config keys; engine rounds.

Bounds.  A mixed row is one fp32 rounding of an fp64 sum of n terms: |Y - ref| <= 2^-24 |ref| + n 2^-52 sum_j |W_rj
U_jp|, elementwise.  Every comparison that depends on which neighbours come first asserts a margin on the fp64
reference: per row, (the first key left out - the last key taken) / max D >= 1e-6, 1000 times the 1e-9 that
``pairwise_sqdist`` is held to; a case that misses it is an error, never a skip.  Bucketing followed by FedAvg is a
convex combination of the rows rounded to fp32 once in between: within 2^-23 max |U| of FedAvg itself."""
import json
import math

import pytest
import torch

from attackfl_amd import agg, ops
from attackfl_amd.config import from_dict
from attackfl_amd.fl.engine import EARLY_AGGREGATORS, FLEngine
from attackfl_amd.ops import composite as C

SHAPES = [(3, 0, 1), (5, 1, 7), (8, 1, 255), (8, 2, 257), (9, 2, 1025), (17, 4, 1025), (33, 7, 63), (64, 15, 1025),
          (64, 30, 255)]
MARGIN = 1e-6


def make_rows(n, f, P, planted, seed=0):
    """base (std 0.3) + 0.01 noise; planted: the last f rows = base + 0.05 sign vector + 0.001 noise."""
    g = torch.Generator().manual_seed(seed)
    base = 0.3 * torch.randn(1, P, generator=g)
    U = base + 0.01 * torch.randn(n, P, generator=g)
    if planted and f:
        sign = torch.where(torch.rand(P, generator=g) < 0.5, -1.0, 1.0)
        U[n - f:] = base + 0.05 * sign[None, :] + 0.001 * torch.randn(f, P, generator=g)
    return U.to(torch.float32)


def make_sizes(n):
    return torch.tensor([300.0 + 37.0 * ((5 * i) % 7) for i in range(n)])


_ROWS = {}


def rows_of(n, f, P, planted):
    key = (n, f, P, planted)
    if key not in _ROWS:
        _ROWS[key] = make_rows(n, f, P, planted)
    return _ROWS[key]


def sqdist_fp64(U):
    """D [n][n] by the difference form in fp64, a list of lists."""
    X = U.double()
    n = X.shape[0]
    return [[float(((X[i] - X[j]) ** 2).sum()) for j in range(n)] for i in range(n)]


def nnm_param_space(U, f, D=None):
    """The rule of docs/PARITY.md line by line -> (W as a list of lists, the worst margin, the neighbour sets)."""
    n = U.shape[0]
    D = sqdist_fp64(U) if D is None else D
    dmax = max(max(r) for r in D)
    W, margin, sets = [], math.inf, []
    for i in range(n):
        key = lambda j: (math.inf if D[i][j] != D[i][j] else D[i][j], j)
        ranked = sorted((j for j in range(n) if j != i), key=key)
        taken = ranked[:n - f - 1]
        if len(taken) < len(ranked) and dmax > 0:
            last = key(taken[-1])[0] if taken else 0.0
            margin = min(margin, (key(ranked[len(taken)])[0] - last) / dmax)
        members = {i} | set(taken)
        sets.append(members)
        W.append([1.0 / (n - f) if j in members else 0.0 for j in range(n)])
    return W, margin, sets


def mix_fp64(W, U):
    """(Y fp64 by an ascending-j loop, the elementwise error bound of one fp32 rounding after an fp64 sum)."""
    X = U.double()
    Wt = torch.as_tensor(W, dtype=torch.float64)
    R, n = Wt.shape
    Y = torch.zeros(R, X.shape[1], dtype=torch.float64)
    S = torch.zeros_like(Y)
    for j in range(n):
        Y += Wt[:, j, None] * X[j][None, :]
        S += (Wt[:, j, None] * X[j][None, :]).abs()
    return Y, 2.0 ** -24 * Y.abs() + n * 2.0 ** -52 * S


def within(got, ref, bound):
    return bool(((got.double().cpu() - ref).abs() <= bound).all())


def bucket_param_space(sizes, n, s, seed):
    """pi = the indices sorted by (u_i, i); bucket r = pi[r s : (r + 1) s] -> (W list of lists, size sums, buckets)."""
    u = C.afl_uniform(seed, n).tolist()
    pi = sorted(range(n), key=lambda i: (u[i], i))
    a = [1.0] * n if sizes is None else [float(x) for x in sizes]
    buckets = [pi[k:k + s] for k in range(0, n, s)]
    W, tot = [], []
    for b in buckets:
        t = sum(a[k] for k in b)
        tot.append(t)
        W.append([a[j] / t if j in b else 0.0 for j in range(n)])
    return W, tot, buckets


# ---------------------------------------------------------------------------------- the rules against their statement
@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("n,f,P", SHAPES)
def test_nnm_matches_parameter_space_loop(n, f, P, planted):
    U = rows_of(n, f, P, planted)
    keep = U.clone()
    Wref, margin, _ = nnm_param_space(U, f)
    print(f"nnm n={n} f={f} P={P} planted={planted}: margin {margin:.3e}")
    assert margin >= MARGIN
    W, nbr = C.nnm_weights(ops.pairwise_sqdist(U), f)
    assert W.dtype == torch.float64 and torch.equal(W, torch.as_tensor(Wref, dtype=torch.float64))
    masks = [sum(1 << j for j in range(n) if Wref[i][j]) for i in range(n)]
    assert nbr.tolist() == [m - (1 << 64) if m >> 63 else m for m in masks]  # (64 bits held in an int64)
    sizes = make_sizes(n)
    Y, s_out, info = agg.nnm(U, sizes, f)
    ref, bound = mix_fp64(Wref, U)
    assert Y.dtype == torch.float32 and Y.shape == (n, P) and within(Y, ref, bound)
    assert s_out is sizes and torch.equal(U, keep)
    assert info["kind"] == "nnm" and info["f"] == f and info["rows"] == n and torch.equal(info["weights"], W)
    assert within(C.mix_rows(W, U), ref, bound)


@pytest.mark.parametrize("sized", [True, False])
@pytest.mark.parametrize("s", [2, 3, 5])
@pytest.mark.parametrize("n,f,P", SHAPES)
def test_bucketing_matches_parameter_space_loop(n, f, P, s, sized):
    U = rows_of(n, f, P, False)
    sizes = make_sizes(n) if sized else None
    seed = 13 * 3 + n
    Wref, tot, buckets = bucket_param_space(sizes, n, s, seed)
    Y, s_out, info = agg.bucketing(U, sizes, s, seed)
    R = -(-n // s)
    assert len(buckets) == R and Y.shape == (R, P) and Y.dtype == torch.float32
    assert torch.equal(info["weights"], torch.as_tensor(Wref, dtype=torch.float64))
    assert s_out.tolist() == tot and s_out.dtype == (sizes.dtype if sized else torch.float64)
    assert info["kind"] == "bucketing" and info["bucket_size"] == s and info["rows"] == R
    ref, bound = mix_fp64(Wref, U)
    assert within(Y, ref, bound)


# ---------------------------------------------------------------------------------- invariants
@pytest.mark.parametrize("n,P", [(3, 1), (8, 257), (33, 63)])
def test_nnm_without_byzantine_rows_is_the_mean(n, P):
    U = rows_of(n, 0, P, False)
    Y, _, info = agg.nnm(U, None, 0)
    ref, bound = mix_fp64([[1.0 / n] * n] * n, U)
    assert within(Y, ref, bound)
    assert all(torch.equal(Y[0], Y[r]) for r in range(n))
    assert torch.equal(info["weights"], torch.full((n, n), 1.0 / n, dtype=torch.float64))


@pytest.mark.parametrize("n,f,P", [s for s in SHAPES if s[1]])
def test_planted_rows_never_enter_an_honest_neighbour_set(n, f, P):
    U = rows_of(n, f, P, True)
    _, margin, sets = nnm_param_space(U, f)
    assert margin >= MARGIN
    W = agg.nnm(U, None, f)[2]["weights"]
    for i in range(n - f):
        assert sets[i].isdisjoint(range(n - f, n))
        assert float(W[i, n - f:].abs().sum()) == 0.0 and float(W[i, i]) == 1.0 / (n - f)


def test_nnm_nan_distance_ranks_last():
    U = rows_of(8, 2, 257, False)
    D = ops.pairwise_sqdist(U).clone()
    D[1, 5] = float("nan")  # (the upper triangle stands for both halves)
    W, _ = C.nnm_weights(D, 2)
    Dl = D.tolist()
    for i in range(8):
        for j in range(i):
            Dl[i][j] = Dl[j][i]
    Wref, _, sets = nnm_param_space(U, 2, Dl)
    assert torch.equal(W, torch.as_tensor(Wref, dtype=torch.float64))
    assert 5 not in sets[1] and 1 not in sets[5]


def test_nnm_admissibility():
    U = rows_of(8, 2, 257, False)
    assert agg.nnm(U, None, "auto")[2]["f"] == 1  # (max(0, (8 - 3) // 4))
    with pytest.raises(ValueError):
        agg.nnm(U, None, 3)  # (8 < 2 * 3 + 3)
    with pytest.raises(ValueError):
        agg.nnm(U, None, -1)
    with pytest.raises(ValueError):
        agg.pre_aggregate("mean", U)


@pytest.mark.parametrize("n,s", [(5, 2), (7, 3), (17, 2), (64, 5)])
def test_bucketing_then_fedavg_is_fedavg(n, s):
    U = rows_of(n, 0, 1025, False)
    sizes = make_sizes(n)
    Y, s2, _ = agg.bucketing(U, sizes, s, 7)
    got = agg.fedavg(Y, s2).params
    ref = agg.fedavg(U, sizes).params
    assert float((got.double() - ref.double()).abs().max()) <= 2.0 ** -23 * float(U.abs().max())
    assert float(s2.double().sum()) == float(sizes.double().sum())


def test_bucket_sizes_and_the_short_last_bucket():
    U = rows_of(7, 0, 33, False)
    Y, s2, info = agg.bucketing(U, None, 3, 11)
    W = info["weights"]
    assert Y.shape == (3, 33) and info["rows"] == 3 and s2.tolist() == [3.0, 3.0, 1.0]
    assert (W > 0).sum(dim=1).tolist() == [3, 3, 1] and (W > 0).sum(dim=0).tolist() == [1] * 7
    pi = C.bucket_permutation(11, 7).tolist()
    assert sorted(pi) == list(range(7))
    assert torch.equal(Y[2], U[pi[6]])  # (the short bucket holds one row, weight 1.0)
    assert [sorted(torch.nonzero(W[r]).reshape(-1).tolist()) for r in range(3)] == [sorted(pi[0:3]), sorted(pi[3:6]),
                                                                                  sorted(pi[6:7])]


def test_bucket_size_one_is_the_identity():
    U = rows_of(8, 1, 255, False)
    sizes = make_sizes(8)
    Y, s2, info = agg.bucketing(U, sizes, 1, 3)
    assert Y is U and s2 is sizes and info["rows"] == 8 and info["bucket_size"] == 1
    assert torch.equal(info["weights"], torch.eye(8, dtype=torch.float64))


def test_bucket_permutation_follows_the_seed():
    a, b, c = (C.bucket_permutation(s, 33).tolist() for s in (5, 5, 6))
    assert a == b and a != c and sorted(a) == list(range(33))
    U = rows_of(33, 7, 63, False)
    y5, y5b, y6 = (agg.bucketing(U, None, 2, s)[0] for s in (5, 5, 6))
    assert torch.equal(y5, y5b) and not torch.equal(y5, y6)


def test_bucketing_refuses_bad_sizes():
    U = rows_of(8, 1, 255, False)
    for bad in (0, -1, 1.5, True, "2"):
        with pytest.raises(ValueError):
            agg.bucketing(U, None, bad, 0)


def test_host_info_reads_the_nested_dict():
    U = rows_of(5, 1, 7, False)
    _, _, info = agg.nnm(U, None, 1)
    h = agg.host_info({"pre_agg": info})["pre_agg"]
    assert h["kind"] == "nnm" and h["f"] == 1 and h["rows"] == 5
    assert len(h["weights"]) == 5 and all(abs(sum(r) - 1.0) <= 1e-15 for r in h["weights"])
    json.dumps(h)


# ---------------------------------------------------------------------------------- config
def test_config_keys():
    d = from_dict({}).engine
    assert d["pre-agg"] == "none" and d["bucket-size"] == 2
    cfg = from_dict({"server": {"mode": "median"}, "engine": {"pre-agg": "bucketing", "bucket-size": 3}})
    assert cfg.engine["pre-agg"] == "bucketing" and cfg.engine["bucket-size"] == 3
    for mode in EARLY_AGGREGATORS:
        if mode != "gmm":
            from_dict({"server": {"mode": mode}, "engine": {"pre-agg": "nnm"}})
    for bad in ("NNM", "mean", "", None, True, 1):
        with pytest.raises(ValueError):
            from_dict({"server": {"mode": "median"}, "engine": {"pre-agg": bad}})
    for bad in (0, -1, 1.5, True, "2", None):
        with pytest.raises(ValueError):
            from_dict({"server": {"mode": "median"}, "engine": {"bucket-size": bad}})
    for mode in ("fedavg", "hyper", "FLTrust", "gmm"):
        from_dict({"server": {"mode": mode}})
        for kind in ("nnm", "bucketing"):
            with pytest.raises(ValueError):
                from_dict({"server": {"mode": mode}, "engine": {"pre-agg": kind}})


def _engine_dict(tmp_path, mode, **engine_kw):
    return {
        "server": {"num-round": 3, "clients": 5, "mode": mode, "model": "TransformerModel",
                   "data-distribution": {"num-data-range": [300, 500]}},
        "learning": {"epoch": 1, "batch-size": 128},
        "data": {"synthetic": True, "train-size": 4000, "test-size": 500},
        "engine": {"checkpoint-dir": str(tmp_path), "trainer": "eager", "max-retries": 3, "byz-f": 1,
                   "metrics": str(tmp_path / "m.jsonl"), **engine_kw},
        "comm": {"attackers": {4: {"mode": "Min-Max", "round": 2}}},
        "log_path": str(tmp_path),
    }


def test_rule_args_keys_unchanged(tmp_path):
    eng = FLEngine(from_dict(_engine_dict(tmp_path, "multi_krum", **{"pre-agg": "nnm"})), device="cpu", verbose=False)
    kw = eng._rule_args()
    eng.close()
    assert set(kw) == {"seed", "gmm_rank", "byz_f", "geomed_iters", "geomed_nu", "dnc_iters", "dnc_sub_dim", "dnc_c",
                       "cclip_iters", "cclip_tau", "centre"}


# ---------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("kind,rows", [("nnm", 5), ("bucketing", 3)])
def test_cpu_engine_rounds(tmp_path, kind, rows):
    """5 clients, byz-f 1, Multi-Krum, one Min-Max attacker from round 2.  (Bucketing: Multi-Krum sees 3 bucket means,
    where an explicit f = 1 needs 5; the engine key is ``auto`` there, which is 0 for 3 rows.)"""
    kw = {"pre-agg": kind} if kind == "nnm" else {"pre-agg": kind, "byz-f": "auto"}
    eng = FLEngine(from_dict(_engine_dict(tmp_path, "multi_krum", **kw)), device="cpu", verbose=False)
    hist = eng.run()
    eng.close()
    assert [r["ok"] for r in hist] == [True, True, True]
    assert all(0.0 <= r["metric"] <= 1.0 for r in hist)
    recs = [json.loads(line) for line in open(tmp_path / "m.jsonl")]
    assert len(recs) == 3
    for r in recs:
        p = r["pre_agg"]
        assert p["kind"] == kind and p["rows"] == rows and len(p["weights"]) == rows
        assert all(len(w) == 5 and abs(sum(w) - 1.0) <= 1e-12 for w in p["weights"])
        assert (p["f"] == 1) if kind == "nnm" else (p["bucket_size"] == 2)
        assert len(r["selected"]) == rows - r["f"]  # (the rule's mask indexes the mixed rows)
