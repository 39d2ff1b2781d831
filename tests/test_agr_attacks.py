"""The AGR-tailored attacks on Krum / Multi-Krum / Bulyan (docs/PARITY.md) on the CPU: the closed-form oracle against
the rule run in parameter space, the result conventions, the attack against the aggregators it models, and the CLIs.

Every comparison first asserts its margin condition on the fp64 reference (``composite.agr_oracle_margin``): a decision
whose margin is far above the rounding differences between two sides is the same on both.  The seeds in ``SEEDS`` were
chosen so that the conditions hold; a case whose condition fails is an error, never skipped."""
import functools

import pytest
import torch

from attackfl_amd import agg, attacks
from attackfl_amd.attacks import bisect_iterations, host_info, run_attack
from attackfl_amd.config import AttackSpec
from attackfl_amd.ops import composite as C

GAMMA0, TAU = 10.0, 0.02
TARGET = {"AGR-Krum": "krum", "AGR-MKrum": "mkrum", "AGR-Bulyan": "bulyan"}
KRUM_SHAPES = [(4, 1), (6, 1), (7, 2), (13, 3), (61, 3)]
BULYAN_SHAPES = [(6, 1), (13, 3), (61, 3)]
CASES = ([("AGR-Krum", K, m) for K, m in KRUM_SHAPES] + [("AGR-MKrum", K, m) for K, m in KRUM_SHAPES]
         + [("AGR-Bulyan", K, m) for K, m in BULYAN_SHAPES])
# seed per (K, P): the margin conditions of this file and of test_gpu_agr_attacks.py hold for every mode at these
SEEDS = {(4, 1025): 1, (6, 1025): 5, (7, 1025): 2, (13, 63): 1, (13, 1025): 7}  # (0 elsewhere)


def make_G(K, P, seed):
    g = torch.Generator().manual_seed(seed)
    base = 0.3 * torch.randn(P, generator=g)
    return base[None] + 0.01 * torch.randn(K, P, generator=g)


def deviation(G, kind):
    st = attacks.column_stats(G)
    if kind == 2:
        return st.mean, st.mean / torch.linalg.vector_norm(st.mean)
    return st.mean, (st.std, st.sign)[kind]


@functools.lru_cache(maxsize=None)
def inputs(K, P, kind=0, seed=None):
    """The attack's closed-form inputs on the CPU, computed once per shape: G, mean, dev, Dg, A, B, C."""
    G = make_G(K, P, SEEDS.get((K, P), 0) if seed is None else seed)
    mean, dev = deviation(G, kind)
    A, B, Cc = C.attack_coeffs(G, mean, dev)
    return G, mean, dev, C.pairwise_l2(G) ** 2, A, B, Cc


@functools.lru_cache(maxsize=None)
def reference_trace(mode, K, m, f, P, kind=0, seed=None):
    """The bisection on the fp64 composite with the diagnostic twin -> [(γ, accept, margin)] for every tried γ."""
    _, _, _, Dg, A, B, Cc = inputs(K, P, kind, seed)
    g, step, out = GAMMA0, GAMMA0, []
    for _ in range(bisect_iterations(GAMMA0, TAU)):
        acc, margin = C.agr_oracle_margin(Dg, A, B, Cc, g, m, f, TARGET[mode])
        out.append((g, acc, margin))
        g = g + step / 2 if acc else g - step / 2
        step /= 2
    return out


def gamma_succ(trace):
    return next((g for g, acc, _ in reversed(trace) if acc), 0.0)


def brute_force(G, mean, dev, gamma, m, f, target):
    """The rule in parameter space: the rows [G; c(γ) x m] in fp64, difference-form distances, krum_select."""
    K = G.shape[0]
    c = mean.double() - gamma * dev.double()
    X = torch.cat([G.double(), c[None].expand(m, -1)])
    D = torch.stack([((X - X[i][None]) ** 2).sum(dim=1) for i in range(K + m)])
    rounds, iterated = C.agr_rounds(K + m, f, target)
    sel, mask, _ = C.krum_select(D, f, rounds, iterated)
    return bool(sel[0] >= K) if target == "krum" else bool(mask[K:].all())


# ------------------------------------------------------------------------------- 1. closed form vs parameter space
@pytest.mark.parametrize("P", [63, 1025])
@pytest.mark.parametrize("mode,K,m", CASES)
def test_oracle_matches_rule_in_parameter_space(mode, K, m, P):
    G, mean, dev, Dg, A, B, Cc = inputs(K, P)
    trace = reference_trace(mode, K, m, m, P)
    assert len(trace) == 9
    assert any(acc for _, acc, _ in trace) and not all(acc for _, acc, _ in trace)
    for g, acc, margin in trace:
        assert margin >= 1e-9, (g, margin)
        got = C.agr_oracle(Dg, A, B, Cc, g, m, m, TARGET[mode])
        assert got.dtype == torch.bool and got.dim() == 0
        assert bool(got) == acc == brute_force(G, mean, dev, g, m, m, TARGET[mode]), g


def test_oracle_rejects_nan_coefficients():
    _, _, _, Dg, A, B, Cc = inputs(7, 63)
    g = gamma_succ(reference_trace("AGR-MKrum", 7, 2, 2, 63))
    assert bool(C.agr_oracle(Dg, A, B, Cc, g, 2, 2, "mkrum"))
    for k in range(3):
        bad = [A.clone(), B.clone(), Cc.clone()]
        bad[k].reshape(-1)[0] = float("nan")
        assert not bool(C.agr_oracle(Dg, *bad, g, 2, 2, "mkrum"))
        assert not C.agr_oracle_margin(Dg, *bad, g, 2, 2, "mkrum")[0]


# ------------------------------------------------------------------------------- 2. result conventions
@pytest.mark.parametrize("mode,K,m", [c for c in CASES if c[1] <= 13])
def test_result_is_the_last_accepted_candidate(mode, K, m):
    G, mean, dev, *_ = inputs(K, 63)
    trace = reference_trace(mode, K, m, m, 63)
    res = run_attack(mode, [m, m], G[0], G, None)
    info = host_info(res.info)
    assert info["gammas"] == [g for g, _, _ in trace] and info["accepted"] == [acc for _, acc, _ in trace]
    succ = gamma_succ(trace)
    assert succ > 0 and info["gamma"] == info["gamma_succ"] == succ and info["iters"] == 9
    assert (info["m"], info["f"], info["target"]) == (m, m, TARGET[mode])
    assert torch.equal(res.params, mean - succ * dev)
    assert res.ok and res.params.dtype == torch.float32
    assert torch.equal(G, make_G(K, 63, SEEDS.get((K, 63), 0)))  # nothing is written into G[0] (A-7 does not apply)


def test_all_rejected_returns_the_mean():
    # K = 2, m = 1, f = 0: k = 1, every score is the distance to the nearest neighbour.  The genuine row nearest to
    # the copy scores at most the copy's own score and has the lower index, so no γ is ever accepted
    G = make_G(2, 63, 0)
    res = run_attack("AGR-Krum", [1, 0], G[0], G, None)
    info = host_info(res.info)
    assert info["accepted"] == [False] * 9 and info["gamma_succ"] == 0.0 and info["gamma"] == 0.0
    assert torch.equal(res.params, G.mean(dim=0))


def test_inadmissible_systems_return_own():
    G = make_G(4, 63, 0)
    own = torch.full((63,), 7.0)
    for mode, args in (("AGR-Krum", [1, 2]), ("AGR-MKrum", [1, 2]), ("AGR-Bulyan", [1, 1]), ("AGR-Bulyan", [2, 1])):
        res = run_attack(mode, args, own, G, None)  # n' = 5 < 2 f + 3 = 7; Bulyan: n' = 5, 6 < 4 f + 3 = 7
        assert torch.equal(res.params, own) and res.params is not own
        assert res.info["gamma"] == 0.0 and res.info["iters"] == 0
    res = run_attack("AGR-MKrum", [1, 1], own, G[:1], None)  # K <= 1, as the bisection attacks
    assert torch.equal(res.params, own) and res.info["iters"] == 0
    assert run_attack("AGR-Bulyan", [3, 1], own, G, None).info["iters"] == 9  # n' = 7 = 4 f + 3 is admitted


def test_f_zero_only_for_agr_krum():
    assert AttackSpec("AGR-Krum", 2, [1, 0]).args == [1.0, 0.0]
    G = make_G(4, 63, 0)
    assert run_attack("AGR-Krum", [1, 0], G[0], G, None).info["f"] == 0
    for mode in ("AGR-MKrum", "AGR-Bulyan"):
        with pytest.raises(ValueError):
            AttackSpec(mode, 2, [1, 0])
        with pytest.raises(ValueError):
            run_attack(mode, [1, 0], G[0], G, None)


@pytest.mark.parametrize("args", [[0], [1.5], [2, 1.5], [2, -1], [1, 1, 3], [1, 1, 0.5], [1, 1, 0, 0], [float("nan")]])
def test_bad_attack_args_raise_when_the_spec_is_built(args):
    assert AttackSpec("AGR-MKrum", 2, [2, 2, 1]).args == [2.0, 2.0, 1.0]  # (a good one is taken)
    for mode in TARGET:
        with pytest.raises(ValueError):
            AttackSpec(mode, 2, args)
    from launch import parse_attackers
    with pytest.raises(ValueError):
        parse_attackers("7:AGR-MKrum:2:" + ":".join(str(a) for a in args))


def test_spec_defaults():
    assert AttackSpec("Min-Max", 2).to_dict() == {"mode": "Min-Max", "round": 2, "args": [], "gamma": 50.0, "tau": 1.0}
    for mode in ("Random", "LIE", "Min-Sum", "Opt-Fang"):
        assert (AttackSpec(mode, 1).gamma, AttackSpec(mode, 1).tau) == (50.0, 1.0)
    for mode in TARGET:
        d = AttackSpec(mode, 2).to_dict()
        assert (d["gamma"], d["tau"]) == (10.0, 0.02) and bisect_iterations(d["gamma"], d["tau"]) == 9
        assert AttackSpec.from_dict(d).to_dict() == d
        assert AttackSpec.from_dict({"mode": mode, "round": 2}).to_dict() == d
    a = AttackSpec.from_dict({"mode": "AGR-MKrum", "round": 3, "args": [2, 2, 1], "gamma": 4.0, "tau": 0.5})
    assert (a.gamma, a.tau, a.args) == (4.0, 0.5, [2.0, 2.0, 1.0])  # an explicit value wins
    assert AttackSpec("AGR-Krum", 2).args == [] and attacks.ATTACKS[-3:] == tuple(TARGET)


def test_deviation_kinds():
    G = make_G(7, 63, 3)
    st = attacks.column_stats(G)
    for kind, dev in ((0, st.std), (1, st.sign), (2, st.mean / torch.linalg.vector_norm(st.mean))):
        res = run_attack("AGR-MKrum", [2, 2, kind], G[0], G, None)
        succ = float(res.info["gamma_succ"])
        assert torch.equal(res.params, st.mean - succ * dev)


# ------------------------------------------------------------------------------- 3. the attack does what it claims
@pytest.mark.parametrize("P", [63, 1025])
@pytest.mark.parametrize("mode,K,m,f", [(mode, K, m, m) for mode, K, m in CASES if K <= 13 and mode != "AGR-Krum"]
                         + [("AGR-Krum", K, m, 0) for K, m in KRUM_SHAPES if K <= 13])
def test_attack_passes_the_aggregator_it_models(mode, K, m, f, P):
    G, _, _, Dg, A, B, Cc = inputs(K, P)
    res = run_attack(mode, [m, f], G[0], G, None)
    succ = float(res.info["gamma_succ"])
    assert succ > 0
    _, margin = C.agr_oracle_margin(Dg, A, B, Cc, succ, m, f, TARGET[mode])
    assert margin >= 1e-4, margin  # (the fp32 result moves the distances by about 1e-7 relative)
    U = torch.cat([G, res.params[None].expand(m, -1)]).contiguous()
    sizes = torch.ones(K + m)
    if mode == "AGR-Krum":
        out = agg.krum(U, sizes)
        assert out.info["f"] == 0 and int(out.info["selected"]) >= K
        assert torch.equal(out.params, res.params)
    else:
        out = (agg.multi_krum if mode == "AGR-MKrum" else agg.bulyan)(U, sizes, byz_f=f)
        assert out.info["f"] == f and bool(out.info["selected"][K:].all())


# ------------------------------------------------------------------------------- 4. the CLIs
def test_cli_parses_the_new_modes():
    import client
    from launch import parse_attackers

    for mode in TARGET:
        a = client.parse_args(["--attack", "True", "--attack_mode", mode, "--attack_round", "2", "--attack_args", "2", "2"])
        assert a.attack and a.attack_mode == mode and a.attack_args == [2.0, 2.0]
    spec = parse_attackers("7:AGR-MKrum:2:2")[7]
    assert (spec.mode, spec.round, spec.args, spec.gamma, spec.tau) == ("AGR-MKrum", 2, [2.0], 10.0, 0.02)
    assert parse_attackers("3:AGR-Bulyan:2:3:1:2")[3].args == [3.0, 1.0, 2.0]
