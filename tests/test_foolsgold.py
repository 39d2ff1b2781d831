"""FoolsGold (``agg.foolsgold``) on the CPU: the history step and the Gram-space weights of ``ops/composite.py`` against a
literal statement of the rule (docs/PARITY.md, "beyond the reference") written here as plain loops in fp64 over the
parameter space, sharing no code with them; three rounds of colluders per shape, so the history matters; the rule's edge
cases; the config keys; the CPU engine's history over rounds, a failed round, stop and resume, a subset selection, two
gloo ranks."""
import json
import math
import os

import pytest
import torch

from attackfl_amd import agg, ops
from attackfl_amd.config import SERVER_MODES, from_dict
from attackfl_amd.fl.engine import FLEngine

# (n rows, f sybils at the end, P)
CASES = [(1, 0, 7), (2, 0, 63), (3, 1, 63), (4, 2, 1025), (8, 2, 1025), (8, 2, 4099), (17, 4, 1025), (33, 8, 63),
         (64, 16, 1025), (8, 0, 1)]
ROUNDS = 3


def make_rounds(n, f, P, seed=0, rounds=ROUNDS):
    """Per round r: the starting model g_r = base + 0.02 r randn (base = 0.3 randn), the updates delta = 0.01 randn;
    for n >= 4 rows 0 and 1 become 0.01 (0.7 h + 0.7 randn) with a shared h redrawn every round (two clients that lean
    the same way, not copies); the last f rows become 0.01 s + 0.001 randn with ONE sign vector s for all rounds (sybils
    pushing one direction).  -> [(U, g)], sizes."""
    gen = torch.Generator().manual_seed(seed)
    base = 0.3 * torch.randn(P, generator=gen)
    s = torch.sign(torch.randn(P, generator=gen))
    out = []
    for r in range(rounds):
        g = base + 0.02 * r * torch.randn(P, generator=gen)
        d = 0.01 * torch.randn(n, P, generator=gen)
        for i in range(n - f, n):  # (drawn before the leaning pair: with this order every case meets check_conditions)
            d[i] = 0.01 * s + 0.001 * torch.randn(P, generator=gen)
        if n >= 4:
            h = torch.randn(P, generator=gen)
            for i in (0, 1):
                d[i] = 0.01 * (0.7 * h + 0.7 * torch.randn(P, generator=gen))
        out.append((g[None, :] + d, g))
    sizes = torch.tensor([300.0 + 37.0 * ((5 * i) % 7) for i in range(n)])
    return out, sizes


def foolsgold_loop(H, kappa):
    """The rule's steps 2 - 7 on the histories themselves -> (alpha, v) as lists of floats; every cosine is a dot
    product of two rows in fp64."""
    X = H.double()
    n = X.shape[0]
    if n == 1:
        return [1.0], [0.0]
    nrm = [math.sqrt(float(torch.dot(X[i], X[i]))) for i in range(n)]
    cs = [[0.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            if i != j and nrm[i] > 0.0 and nrm[j] > 0.0 and math.isfinite(nrm[i]) and math.isfinite(nrm[j]):
                cs[i][j] = max(-1.0, min(1.0, float(torch.dot(X[i], X[j])) / (nrm[i] * nrm[j])))
    v = [max(cs[i][j] for j in range(n) if j != i) for i in range(n)]
    a = []
    for i in range(n):
        worst = -math.inf
        for j in range(n):
            if j == i:
                continue
            c = cs[i][j]
            if v[j] > v[i] and v[j] != 0.0:
                c = c * v[i] / v[j]
            worst = max(worst, c)
        a.append(max(0.0, min(1.0, 1.0 - worst)))
    M = max(a)
    if M <= 0.0:
        return [0.0] * n, v
    alpha = []
    for x in a:
        x = x / M
        x = 0.99 if x == 1.0 else x
        y = -math.inf if x == 0.0 else kappa * (math.log(x / (1.0 - x)) + 0.5)
        alpha.append(max(0.0, min(1.0, y)))
    return alpha, v


def result_loop(U, g, sizes, alpha):
    X, c = U.double(), g.double()
    n = X.shape[0]
    a0 = [1.0 / n] * n if sizes is None else [float(s) / float(sizes.double().sum()) for s in sizes]
    out = c.clone()
    for j in range(n):
        if a0[j] * alpha[j] != 0.0:
            out += a0[j] * alpha[j] * (X[j] - c)
    return out


def close(got, ref, tol):
    return (got.double() - ref.double()).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


_REF = {}


def reference(n, f, P, kappa=1.0):
    """The rounds of a case with the fp64 loop's answers, computed once: [(U, g, H_old, H_new, alpha, v, result)]."""
    key = (n, f, P, kappa)
    if key not in _REF:
        rounds, sizes = make_rounds(n, f, P)
        H = torch.zeros(n, P)
        rows = []
        for U, g in rounds:
            Hn = H + (U - g[None])
            alpha, v = foolsgold_loop(Hn, kappa)
            rows.append((U, g, H, Hn, alpha, v, result_loop(U, g, sizes, alpha)))
            H = Hn
        _REF[key] = (rows, sizes)
    return _REF[key]


def check_conditions(n, f, P, rows):
    """What makes a case worth running, asserted on the fp64 reference: the sybils are silenced, the independent rows
    keep full weight, and the two leaning rows sit strictly inside the logit's slope."""
    if P == 1:
        return
    for r, (_, _, _, _, alpha, _, _) in enumerate(rows):
        lean = (0, 1) if n >= 4 else ()
        if f >= 2:
            assert all(alpha[i] == 0.0 for i in range(n - f, n)), (n, f, P, r, alpha)
        assert all(alpha[i] == 1.0 for i in range(n - f) if i not in lean), (n, f, P, r, alpha)
        if n >= 8:
            assert all(0.05 < alpha[i] < 0.95 for i in lean), (n, f, P, r, alpha[:2])


# ---------------------------------------------------------------------------------- the rule against its statement
@pytest.mark.parametrize("n,f,P", CASES)
def test_three_rounds_match_the_loop(n, f, P):
    rows, sizes = reference(n, f, P)
    check_conditions(n, f, P, rows)
    H, count = None, 0
    for U, g, H_old, H_new, alpha, v, ref in rows:
        keep = (U.clone(), g.clone(), None if H is None else H.clone())
        res = agg.foolsgold(U, sizes, g, H, 1.0, rounds=count)
        got = res.info["history"]
        assert got.dtype == torch.float32 and torch.equal(got, H_new)  # the bits of H + (U - g[None])
        assert res.info["alpha"].dtype == torch.float64 and res.info["alpha"].shape == (n,)
        assert (res.info["alpha"] - torch.tensor(alpha, dtype=torch.float64)).abs().max().item() <= 1e-9
        assert (res.info["max_cos"] - torch.tensor(v, dtype=torch.float64)).abs().max().item() <= 1e-9
        assert res.params.dtype == torch.float32 and close(res.params, ref, 1e-6)
        count += 1
        assert int(res.info["rounds"]) == count
        # the inputs are untouched, the history and the result are new tensors
        assert torch.equal(U, keep[0]) and torch.equal(g, keep[1]) and (H is None or torch.equal(H, keep[2]))
        ptrs = {t.untyped_storage().data_ptr() for t in (U, g) + (() if H is None else (H,))}
        assert res.params.untyped_storage().data_ptr() not in ptrs and got.untyped_storage().data_ptr() not in ptrs
        H = got


def test_history_changes_the_answer():
    """Round 3 of (8, 2, 1025) judged on that round's rows alone (a zero history) weighs the leaning rows differently
    from the run with memory: the comparison above cannot pass with the accumulation switched off."""
    rows, sizes = reference(8, 2, 1025)
    U, g, _, _, alpha, _, _ = rows[2]
    alone = agg.foolsgold(U, sizes, g, None, 1.0).info["alpha"]
    assert max(abs(float(alone[i]) - alpha[i]) for i in (0, 1)) > 1e-3


@pytest.mark.parametrize("kappa", [0.5, 1.0, 2.0])
def test_kappa_scales_the_logit(kappa):
    rows, sizes = reference(8, 2, 1025, kappa)
    H = None
    for U, g, _, H_new, alpha, _, ref in rows:
        res = agg.foolsgold(U, sizes, g, H, kappa)
        assert (res.info["alpha"] - torch.tensor(alpha, dtype=torch.float64)).abs().max().item() <= 1e-9
        assert close(res.params, ref, 1e-6)
        H = res.info["history"]
    # (not vacuous: a weight inside the slope at kappa = 1 is half of that at 0.5)
    a = {k: reference(8, 2, 1025, k)[0][2][4] for k in (0.5, 1.0)}
    assert any(0.0 < a[1.0][i] < 1.0 and abs(a[0.5][i] - 0.5 * a[1.0][i]) <= 1e-12 for i in range(8))


def test_uniform_weights_when_sizes_is_none():
    rows, _ = reference(8, 2, 1025)
    U, g, H_old, _, alpha, _, _ = rows[1]
    res = agg.foolsgold(U, None, g, H_old, 1.0)
    assert close(res.params, result_loop(U, g, None, alpha), 1e-6)


# ---------------------------------------------------------------------------------- edge cases
def test_one_column_every_history_is_parallel():
    """P = 1: every cosine is +-1, every row has a parallel partner after pardoning, so alpha = 0 and the result is the
    centre itself, as a new tensor."""
    rows, sizes = reference(8, 0, 1)
    H = None
    for U, g, _, _, alpha, _, _ in rows:
        assert alpha == [0.0] * 8
        res = agg.foolsgold(U, sizes, g, H, 1.0)
        assert res.info["alpha"].tolist() == [0.0] * 8
        assert torch.equal(res.params, g) and res.params.untyped_storage().data_ptr() != g.untyped_storage().data_ptr()
        H = res.info["history"]


def test_one_row_has_full_weight():
    rows, sizes = reference(1, 0, 7)
    U, g = rows[0][0], rows[0][1]
    res = agg.foolsgold(U, sizes, g, None, 1.0)
    assert res.info["alpha"].tolist() == [1.0] and res.info["max_cos"].tolist() == [0.0]
    assert close(res.params, U[0], 1e-6)


def test_identical_histories_get_no_weight_and_all_ones_is_fedavg_about_the_centre():
    gen = torch.Generator().manual_seed(5)
    g = torch.randn(257, generator=gen)
    U = g[None] + 0.01 * torch.randn(1, 257, generator=gen).expand(4, 257).contiguous()
    res = agg.foolsgold(U, None, g, None, 1.0)  # four copies: every cosine 1
    assert res.info["alpha"].tolist() == [0.0] * 4 and torch.equal(res.params, g)
    # orthogonal histories: every alpha 1, the result is FedAvg about g
    U = g[None] + 0.01 * torch.eye(4, 257)
    sizes = torch.tensor([1.0, 2.0, 3.0, 4.0])
    res = agg.foolsgold(U, sizes, g, None, 1.0)
    assert res.info["alpha"].tolist() == [1.0] * 4
    assert close(res.params, ops.fedavg(U, sizes), 1e-6)


def test_zero_history_row_counts_as_unrelated():
    """A row equal to the centre has a zero history: its pairs get cosine 0, not NaN."""
    rows, sizes = reference(8, 2, 1025)
    U, g = rows[0][0].clone(), rows[0][1]
    U[3] = g
    res = agg.foolsgold(U, sizes, g, None, 1.0)
    alpha, v = foolsgold_loop(U - g[None], 1.0)
    assert bool(torch.isfinite(res.info["alpha"]).all()) and float(res.info["max_cos"][3]) == 0.0 == v[3]
    assert (res.info["alpha"] - torch.tensor(alpha, dtype=torch.float64)).abs().max().item() <= 1e-9


def test_no_centre_is_fedavg_and_leaves_the_history():
    rows, sizes = reference(8, 2, 1025)
    U, _, _, H_new, _, _, _ = rows[0]
    for H in (None, H_new):
        res = agg.foolsgold(U, sizes, None, H, 1.0, rounds=4)
        assert torch.equal(res.params, ops.fedavg(U, sizes))
        assert res.info["alpha"].tolist() == [1.0] * 8 and int(res.info["rounds"]) == 4
        assert (H is None and not bool(res.info["history"].any())) or res.info["history"] is H


def test_enable_zero_keeps_the_history_bits():
    rows, sizes = reference(8, 2, 1025)
    U, g, _, H_new, _, _, _ = rows[1]
    H = H_new.clone()
    H[0, :3] = torch.tensor([-0.0, 0.0, 1e-45])  # (a selected, not an added, zero: -0.0 and a denormal survive)
    off, on = torch.zeros(1, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    res = agg.foolsgold(U, sizes, g, H, 1.0, enable=off, rounds=2)
    assert torch.equal(res.info["history"].view(torch.int32), H.view(torch.int32)) and int(res.info["rounds"]) == 2
    U_bad = U.clone()
    U_bad[5] = float("nan")  # (a faulted client's row in a failed round never reaches the history)
    assert torch.equal(agg.foolsgold(U_bad, sizes, g, H, 1.0, enable=off).info["history"].view(torch.int32),
                       H.view(torch.int32))
    res = agg.foolsgold(U, sizes, g, H, 1.0, enable=on, rounds=2)
    assert torch.equal(res.info["history"], H + (U - g[None])) and int(res.info["rounds"]) == 3
    out = torch.empty_like(H)
    res = agg.foolsgold(U, sizes, g, H, 1.0, out=out)
    assert res.info["history"] is out and torch.equal(out, H + (U - g[None]))


def test_ops_composites_directly():
    rows, sizes = reference(17, 4, 1025)
    U, g, H_old, H_new, alpha, v, _ = rows[2]
    Hn, G = ops.hist_gram(U, g, H_old, None)
    assert torch.equal(Hn, H_new) and G.dtype == torch.float64
    assert torch.equal(G, ops.gram_anchored(Hn, torch.zeros(1025)))
    a0 = sizes.double() / sizes.double().sum()
    al, vv, c = ops.foolsgold_weights(G, a0, 1.0)
    assert (al - torch.tensor(alpha, dtype=torch.float64)).abs().max().item() <= 1e-9
    assert torch.equal(c, a0 * al) and (vv - torch.tensor(v, dtype=torch.float64)).abs().max().item() <= 1e-9


# ---------------------------------------------------------------------------------- config
def test_config_keys_and_errors():
    assert "foolsgold" in SERVER_MODES and "foolsgold" not in agg.AGGREGATORS  # (AGGREGATORS: the stateless rules)
    assert from_dict({}).engine["foolsgold-kappa"] == 1.0
    cfg = from_dict({"server": {"mode": "foolsgold"}, "engine": {"foolsgold-kappa": 2}})
    assert cfg.mode == "foolsgold" and cfg.engine["foolsgold-kappa"] == 2
    from_dict({"engine": {"foolsgold-kappa": "0.5"}})  # (YAML 1.1 may hand a number over as a string)
    for bad in (0, -1.0, "x", True, [1]):
        with pytest.raises(ValueError, match="engine.foolsgold-kappa must be "):
            from_dict({"engine": {"foolsgold-kappa": bad}})
    for pre in ("nnm", "bucketing"):  # mixing destroys the client identity the history is keyed by
        with pytest.raises(ValueError, match="pre-agg"):
            from_dict({"server": {"mode": "foolsgold"}, "engine": {"pre-agg": pre}})
    rows, sizes = reference(8, 2, 1025)
    U, g = rows[0][0], rows[0][1]
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            agg.foolsgold(U, sizes, g, None, bad)
    with pytest.raises(ValueError):
        agg.foolsgold(U, sizes, g, torch.zeros(7, 1025), 1.0)


# ---------------------------------------------------------------------------------- engine
def _cfg(path, rounds, **engine):
    return {
        "server": {"num-round": rounds, "clients": 4, "mode": "foolsgold", "model": "TransformerModel",
                   "data-distribution": {"num-data-range": [150, 260]}},
        "learning": {"epoch": 1, "batch-size": 64},
        "data": {"synthetic": True, "train-size": 1500, "test-size": 400},
        "engine": {"checkpoint-dir": str(path), "trainer": "eager", "max-retries": 3, **engine},
        "log_path": str(path),
    }


def _capture(eng):
    """Every server step's rows and START model, taken before the step."""
    seen, orig = [], eng.server.foolsgold

    def cap(U, sizes, ok_all):
        seen.append((U.detach().clone(), None if eng.global_params is None else eng.global_params.detach().clone()))
        return orig(U, sizes, ok_all)

    eng.server.foolsgold = cap
    return seen


def test_cpu_engine_history_is_the_sum_over_successful_rounds(tmp_path):
    d = _cfg(tmp_path, 3, metrics=str(tmp_path / "m.jsonl"))
    d["engine"]["fault-inject"] = [{"client": 2, "round": 2}]
    eng = FLEngine(from_dict(d), device="cpu", verbose=False)
    seen = _capture(eng)
    oks, hists = [], []
    while eng.rounds_left > 0:
        before = eng.server.history.clone()
        rec = eng.run_round()
        oks.append(rec["ok"])
        hists.append((before, eng.server.history.clone()))
    eng.ckpt_writer.flush()
    assert oks == [True, False, True, True]
    # round 1 starts without a global model: FedAvg, nothing accumulated; the failed round never reached the rule
    assert len(seen) == 3 and seen[0][1] is None
    assert not bool(hists[0][1].any()) and torch.equal(hists[1][0], hists[1][1])
    H = torch.zeros(4, eng.P)
    for U, g in seen[1:]:
        H = H + (U - g[None])
    assert bool(H.any()) and torch.equal(eng.server.history, H) and int(eng.server.rounds) == 2
    eng.close()
    recs = [json.loads(line) for line in open(tmp_path / "m.jsonl")]
    ok_recs = [r for r in recs if r["ok"]]
    assert [r["rounds"] for r in ok_recs] == [0, 1, 2]
    assert all(len(r["alpha"]) == 4 and all(0.0 <= a <= 1.0 for a in r["alpha"]) and len(r["max_cos"]) == 4
               for r in ok_recs)
    assert "alpha" not in recs[1] and "history" not in ok_recs[-1]


def test_cpu_engine_stop_and_resume_is_exact(tmp_path):
    """4 rounds in one run == 2 rounds, then a fresh engine resuming from the state files for 2 more: the history, the
    count of rounds and the checkpoint bit for bit."""
    full = tmp_path / "full"
    eng = FLEngine(from_dict(_cfg(full, 4)), device="cpu", verbose=False)
    eng.run()
    H_ref, n_ref = eng.server.history.clone(), int(eng.server.rounds)
    eng.close()
    ref = torch.load(os.path.join(full, "TransformerModel.pth"), weights_only=True)

    part = tmp_path / "part"
    eng = FLEngine(from_dict(_cfg(part, 4, **{"save-state": True})), device="cpu", verbose=False)
    eng.run(max_rounds=2)
    eng.close()
    eng2 = FLEngine(from_dict(_cfg(part, 4, **{"save-state": True, "resume": True})), device="cpu", verbose=False)
    assert eng2.round_no == 3 and eng2.rounds_left == 2 and int(eng2.server.rounds) == 1 and bool(eng2.server.history.any())
    hist = eng2.run()
    assert [r["round"] for r in hist] == [3, 4]
    assert n_ref == 3 == int(eng2.server.rounds) and torch.equal(eng2.server.history, H_ref)
    eng2.close()
    got = torch.load(os.path.join(part, "TransformerModel.pth"), weights_only=True)
    assert list(ref) == list(got) and all(torch.equal(ref[k], got[k]) for k in ref)


def test_engine_subset_selection_is_keyed_by_client_id(tmp_path):
    """A selection that is a strict subset of the clients: its rows are gathered from and scattered to the history by
    client id, the other clients' rows are carried over."""
    eng = FLEngine(from_dict(_cfg(tmp_path, 2)), device="cpu", verbose=False)
    gen = torch.Generator().manual_seed(3)
    P = eng.P
    eng.global_params = g = torch.randn(P, generator=gen)
    sizes = torch.tensor([200.0, 180.0, 250.0])
    eng.selected = [0, 2, 3]
    U1 = g[None] + 0.01 * torch.randn(3, P, generator=gen)
    new, info = eng.server.foolsgold(U1, sizes, None)
    want = agg.foolsgold(U1, sizes, g, None, 1.0)
    assert torch.equal(new, want.params) and torch.equal(info["alpha"], want.info["alpha"]) and "history" not in info
    assert torch.equal(eng.server.history[[0, 2, 3]], U1 - g[None]) and not bool(eng.server.history[1].any())
    eng.selected = [1, 3]
    U2 = g[None] + 0.01 * torch.randn(2, P, generator=gen)
    new, info = eng.server.foolsgold(U2, sizes[:2], torch.ones((), dtype=torch.bool))
    H = torch.zeros(4, P)
    H[[0, 2, 3]] = U1 - g[None]
    want = agg.foolsgold(U2, sizes[:2], g, H[[1, 3]], 1.0)
    H[[1, 3]] = H[[1, 3]] + (U2 - g[None])
    assert torch.equal(eng.server.history, H) and torch.equal(new, want.params) and int(eng.server.rounds) == 2
    before = eng.server.history.clone()
    eng.server.foolsgold(U2, sizes[:2], torch.zeros((), dtype=torch.bool))  # a round the device saw fail
    assert torch.equal(eng.server.history, before) and int(eng.server.rounds) == 2
    eng.close()


def test_two_ranks_carry_the_history(tmp_path):
    """The packed launch over two gloo ranks (two clients each): the replicated server step runs on the gathered rows on
    every rank, the leader's state file carries the history and the count of rounds, and both agree with the same run
    in one process (up to the CPU GEMMs' thread-count dependent summation order, as tests/test_engine.py allows)."""
    import subprocess
    import sys

    import test_engine as E

    d = _cfg(tmp_path / "mp", 3, **{"save-state": True})
    d["comm"] = {"backend": "gloo"}
    os.makedirs(tmp_path / "mp")
    cfg_path = E._write_cfg(tmp_path, d)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(E._free_port()), os.path.join(E.ROOT, "launch.py"), "--config", cfg_path,
           "--device", "cpu"]
    r = subprocess.run(cmd, env=E._env(), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    srv = torch.load(tmp_path / "mp" / "TransformerModel.state.pt", weights_only=True)
    eng = FLEngine(from_dict(_cfg(tmp_path / "sp", 3)), device="cpu", verbose=False)
    eng.run()
    H, count = eng.server.history.clone(), int(eng.server.rounds)
    eng.close()
    assert srv["fg_rounds"] == count == 2 and srv["fg_history"].shape == H.shape and bool(H.any())
    assert torch.allclose(srv["fg_history"], H, atol=1e-4)
    mp = torch.load(tmp_path / "mp" / "TransformerModel.pth", weights_only=True)
    sp = torch.load(tmp_path / "sp" / "TransformerModel.pth", weights_only=True)
    assert all(torch.allclose(sp[k], mp[k], atol=1e-4) for k in sp)
