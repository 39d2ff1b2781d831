"""The AGR-tailored attacks on the device: ``k_agr_bisect`` against the fp64 composite on identical inputs (equal, not
close), the whole attack through the fused launch, the generic device loop and the CPU, n' = 65 on the composite path,
the binding's argument checks, and the engine (bit-reproducible; the early launch against the serial schedule).

As in test_agr_attacks.py every comparison first asserts its margin condition on the fp64 reference."""
import pytest
import torch

from attackfl_amd import ops
from attackfl_amd.attacks import host_info, run_attack
from attackfl_amd.config import from_dict
from attackfl_amd.fl.engine import FLEngine, build_client_table
from attackfl_amd.ops import composite as C
from launch import parse_attackers
from test_agr_attacks import CASES, GAMMA0, KRUM_SHAPES, TARGET, gamma_succ, inputs, reference_trace

pytestmark = pytest.mark.gpu


def kernel_trace(gpu, K, P, kind, m, f, target):
    _, _, _, Dg, A, B, Cc = inputs(K, P, kind)
    st = ops.agr_bisect_fused(Dg.to(gpu), A.to(gpu), B.to(gpu), Cc.to(gpu), m, f, target, 9, GAMMA0)
    assert st is not None and st.shape == (40,) and st.dtype == torch.float64
    return st.cpu().tolist()


def check_kernel(gpu, mode, K, m, f, P, kind=0):
    trace = reference_trace(mode, K, m, f, P, kind)
    for g, _, margin in trace:  # (the two sides differ by the rounding of d_j at most: about 1e-16)
        assert margin >= 1e-9, (g, margin)
    st = kernel_trace(gpu, K, P, kind, m, f, TARGET[mode])
    assert st[4:13] == [g for g, _, _ in trace]
    assert st[20:29] == [1.0 if acc else 0.0 for _, acc, _ in trace]
    assert st[1] == gamma_succ(trace) and st[2] == trace[-1][0]
    assert st[13:20] == [0.0] * 7 and st[29:] == [0.0] * 11
    return trace


# ------------------------------------------------------------------------------- 5. kernel against composite
@pytest.mark.parametrize("P", [63, 1025])
@pytest.mark.parametrize("mode,K,m", CASES)
def test_kernel_equals_composite_on_identical_inputs(gpu, mode, K, m, P):
    trace = check_kernel(gpu, mode, K, m, m, P)
    assert any(acc for _, acc, _ in trace) and not all(acc for _, acc, _ in trace)


def test_kernel_smallest_system_and_deviation_kinds(gpu):
    check_kernel(gpu, "AGR-Krum", 2, 1, 0, 63)  # n' = 3, the smallest the rule admits (f = 0)
    for K, m in KRUM_SHAPES[:3]:
        check_kernel(gpu, "AGR-Krum", K, m, 0, 63)  # f = 0: this project's server.mode krum
    for kind in (0, 1, 2):
        check_kernel(gpu, "AGR-Krum", 7, 2, 2, 63, kind)
        check_kernel(gpu, "AGR-MKrum", 7, 2, 2, 63, kind)


def test_kernel_rejects_nan_coefficients(gpu):
    _, _, _, Dg, A, B, Cc = inputs(7, 63)
    for k in range(3):
        bad = [A.clone(), B.clone(), Cc.clone()]
        bad[k].reshape(-1)[-1] = float("nan")
        st = ops.agr_bisect_fused(Dg.to(gpu), *[t.to(gpu) for t in bad], 2, 2, "mkrum", 9, GAMMA0).cpu()
        assert st[20:29].tolist() == [0.0] * 9 and float(st[1]) == 0.0  # every γ rejected, γ halves down
        assert st[4:13].tolist() == [GAMMA0 / 2 ** i for i in range(9)]


# ------------------------------------------------------------------------------- 6. whole attack on the device
DEVICE_SHAPES = [(4, 1), (7, 2), (13, 3), (29, 3)]


@pytest.mark.parametrize("P", [63, 1025])
@pytest.mark.parametrize("mode,K,m", [(mode, K, m) for mode in TARGET for K, m in DEVICE_SHAPES
                                      if C.agr_admissible(K + m, m, TARGET[mode])])
def test_fused_attack_matches_generic_and_cpu(gpu, monkeypatch, mode, K, m, P):
    G = inputs(K, P)[0]
    trace = reference_trace(mode, K, m, m, P)
    for g, _, margin in trace:  # 100x the 1e-9 relative bound docs/PARITY.md holds pairwise_sqdist to
        assert margin >= 1e-7, (g, margin)
    cpu = host_info(run_attack(mode, [m, m], G[0], G, None).info)
    assert cpu["gammas"] == [g for g, _, _ in trace] and cpu["accepted"] == [acc for _, acc, _ in trace]
    Gd = G.to(gpu)
    launches = []
    orig = ops.agr_bisect_fused
    monkeypatch.setattr(ops, "agr_bisect_fused", lambda *a: launches.append(1) or orig(*a))
    fused = run_attack(mode, [m, m], Gd[0], Gd, None)
    assert launches == [1] and fused.params.is_cuda and fused.info["gamma_succ"].is_cuda
    monkeypatch.setattr(ops, "agr_bisect_fused", lambda *a: None)  # force the generic device loop
    gen = run_attack(mode, [m, m], Gd[0], Gd, None)
    hf, hg = host_info(fused.info), host_info(gen.info)
    assert hf["gammas"] == hg["gammas"] == cpu["gammas"]
    assert hf["accepted"] == hg["accepted"] == cpu["accepted"]
    assert hf["gamma"] == hg["gamma"] == cpu["gamma"] == hf["gamma_succ"] == gamma_succ(trace)
    assert torch.equal(fused.params, gen.params)
    assert torch.equal(Gd.cpu(), G)


# ------------------------------------------------------------------------------- 7. beyond the kernel's 64 rows
@pytest.mark.parametrize("mode", list(TARGET))
def test_65_rows_take_the_composite_path(gpu, mode):
    K, m, P = 62, 3, 1025
    G, _, _, Dg, A, B, Cc = inputs(K, P)
    trace = reference_trace(mode, K, m, m, P)
    for g, _, margin in trace:
        assert margin >= 1e-7, (g, margin)
    assert ops.agr_bisect_fused(Dg.to(gpu), A.to(gpu), B.to(gpu), Cc.to(gpu), m, m, TARGET[mode], 9, GAMMA0) is None
    Gd = G.to(gpu)
    res = run_attack(mode, [m, m], Gd[0], Gd, None)
    info = host_info(res.info)
    assert info["gammas"] == [g for g, _, _ in trace] and info["accepted"] == [acc for _, acc, _ in trace]
    assert info["gamma_succ"] == gamma_succ(trace) > 0
    cpu = run_attack(mode, [m, m], G[0], G, None)
    assert (res.params.cpu() - cpu.params).abs().max().item() <= 1e-6


# ------------------------------------------------------------------------------- 8. bad arguments
def test_bad_arguments_raise_before_any_launch(gpu):
    _, _, _, Dg, A, B, Cc = inputs(7, 63)
    Dg, A, B, Cc = Dg.to(gpu), A.to(gpu), B.to(gpu), Cc.reshape(1).to(gpu)
    st = torch.zeros(40, dtype=torch.float64, device=gpu)
    st[:1].fill_(GAMMA0)
    before = st.clone()
    nat = ops.native()
    big = torch.zeros(62, 62, dtype=torch.float64, device=gpu)
    vec = torch.zeros(62, dtype=torch.float64, device=gpu)
    bad = [
        (st, big, vec, vec, Cc, 3, 3, 1, 9),                # n' = 65
        (st, Dg, A, B, Cc, 0, 1, 1, 9),                     # m < 1
        (st, Dg, A, B, Cc, 2, -1, 0, 9),                    # f < 0
        (st, Dg, A, B, Cc, 2, 4, 1, 9),                     # n' = 9 < 2 f + 3
        (st, Dg, A, B, Cc, 2, 2, 2, 9),                     # Bulyan: n' = 9 < 4 f + 3
        (st, Dg, A, B, Cc, 2, 2, 3, 9), (st, Dg, A, B, Cc, 2, 2, -1, 9),   # no such target
        (st, Dg, A, B, Cc, 2, 2, 1, 0), (st, Dg, A, B, Cc, 2, 2, 1, 17),   # n_iter outside [1, 16]
        (st, Dg.float(), A, B, Cc, 2, 2, 1, 9),             # dtype
        (st, Dg, A.float(), B, Cc, 2, 2, 1, 9),
        (st[:39], Dg, A, B, Cc, 2, 2, 1, 9),                # state too short
        (st, Dg[:6], A, B, Cc, 2, 2, 1, 9),                 # Dg not square
        (st, Dg, A[:6], B, Cc, 2, 2, 1, 9), (st, Dg, A, B[:6], Cc, 2, 2, 1, 9),
        (st, Dg, A, B, torch.zeros(2, dtype=torch.float64, device=gpu), 2, 2, 1, 9),
        (st, Dg.t(), A, B, Cc, 2, 2, 1, 9),                 # not contiguous
        (st, Dg.cpu(), A, B, Cc, 2, 2, 1, 9), (st.cpu(), Dg, A, B, Cc, 2, 2, 1, 9),   # not on the device
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            nat.agr_bisect(*args, GAMMA0)
    torch.cuda.synchronize()
    assert torch.equal(st, before)  # nothing ran
    nat.agr_bisect(st, Dg, A, B, Cc, 2, 2, 1, 9, GAMMA0)
    assert float(st[2]) > 0 and not torch.equal(st, before)


# ------------------------------------------------------------------------------- 9. engine
def _engine(tmp_path, sub, **engine_kw):
    d = {
        "server": {"num-round": 4, "clients": 8, "mode": "multi_krum", "model": "TransformerModel", "data-name": "ICU",
                   "genuine-rate": 1.0, "random-seed": 11, "data-distribution": {"num-data-range": [300, 500]}},
        "learning": {"epoch": 2, "batch-size": 128},
        "data": {"synthetic": True, "train-size": 4000, "test-size": 1000},
        "engine": {"checkpoint-dir": str(tmp_path / sub), "trainer": "auto", "seed": 3, **engine_kw},
        "log_path": str(tmp_path / sub),
    }
    cfg = from_dict(d)
    return FLEngine(cfg, device="cuda", table=build_client_table(cfg, 1, parse_attackers("7:AGR-MKrum:2")),
                    verbose=False)


def test_engine_rounds_with_an_agr_attacker(gpu, tmp_path):
    def run(spec, sub):
        eng = _engine(tmp_path, sub, speculative=spec)
        assert eng.trainer.kind == "fused" and eng._speculative == spec
        hist = eng.run()
        out = eng.global_params.detach().cpu().clone()
        eng.close()
        return hist, out

    h1, p1 = run(True, "spec")
    h2, p2 = run(True, "again")
    h0, p0 = run(False, "serial")
    assert len(h1) == 4 and all(r["ok"] for r in h1)
    assert any(r.get("path") == "early-launch" for r in h1)
    assert "attack" not in h1[0]
    for r in h1[1:]:
        a = r["attack"]
        assert a["gamma_succ"] == a["gamma"] and len(a["gammas"]) == len(a["accepted"]) == a["iters"] == 9
        assert a["gammas"][0] == 10.0 and (a["m"], a["f"]) == (1, 1)
        assert a["gamma_succ"] in [0.0] + [g for g, acc in zip(a["gammas"], a["accepted"]) if acc][-1:]
    key = lambda h: [(r["ok"], r["metric"], r.get("attack")) for r in h]
    assert key(h1) == key(h2) and torch.equal(p1, p2)   # two runs are bit-identical
    assert key(h1) == key(h0) and torch.equal(p1, p0)   # the early launch equals the serial schedule
