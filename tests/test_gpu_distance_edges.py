"""The attack-distance kernels (``csrc/kernels/linalg.hip``: the direct spectral norm, the Gram-form family, the fused
bisection) and the ROC-AUC kernels (``csrc/kernels/metrics.hip``) at edge spectra, scales and shapes, against the fp64
oracles, case tables and derived bounds of ``tests/test_distance_oracles.py``.  Every spectral assertion is
|got - ref| ≤ truncation + rounding allowance per (row, slot); measured ratios in ``docs/DISTANCE_TEST_BOUNDS.md``."""
import math

import pytest
import torch

import test_distance_oracles as R
from attackfl_amd import attacks, ops
from attackfl_amd.models import ParamLayout, TensorSlot

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _same_bits(a, b):
    """torch.equal on the bit patterns (a NaN equals the same NaN)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _scalar(g, gpu):
    return torch.tensor(float(g), dtype=F64, device=gpu)


def _values(case, gpu):
    """Every API over one case (a single slot at an unaligned offset) -> {(api, family, γ): [M] fp64 on the host}."""
    X, slots = R.pack([case])
    Xd, s = X.to(gpu), slots[0]
    out = {("batched", False, None): ops.batched_spectral_norm(R.slot_matrix(Xd, s).contiguous()),
           ("slots", False, None): ops._spectral_slots_direct(Xd, slots)}
    fam = ops.SpectralFamily(Xd, slots)
    out[("sum", True, None)] = ops.spectral_norm_sum(Xd, slots)
    out[("family", True, None)] = fam(None)
    if case.D is not None:
        dev = torch.zeros(X.shape[1])
        dev[s.offset:s.offset + s.numel] = case.D.reshape(-1)
        famd = ops.SpectralFamily(Xd, slots, dev.to(gpu))
        for g in case.gammas:
            out[("family-dev", True, g)] = famd(g)
            out[("family-dev-scalar", True, g)] = famd(_scalar(g, gpu))
    return {k: v.cpu() for k, v in out.items()}


def _check_case(case, gpu, worst, one_sided=False):
    vals = _values(case, gpu)
    assert _same_bits(vals[("family", True, None)], vals[("sum", True, None)])
    for g in (case.gammas if case.D is not None else ()):
        assert torch.equal(vals[("family-dev", True, g)], vals[("family-dev-scalar", True, g)])
    recs = {}
    for (api, family, g), got in vals.items():
        key = (R.path(*case.X.shape[1:], family), g)
        if key not in recs:
            recs[key] = R.bound_of(case.X, case.D, g, family)
        R.check(got.tolist(), recs[key], f"{case.name} {api} γ={g}", one_sided=one_sided, worst=worst)


@pytest.mark.parametrize("n", R.SIZES)
def test_padding_and_tiles(gpu, n):
    """k in {n, n + 1, 3n + 5}, both orientations and square: the n8 padding of spectral_one, the n16 padding and the
    tile grid of k_spec_eval, Gram form -> direct at 64/65 (and at the LDS fit 64 x 319 / 320), kernels -> library at
    128/129, the LDS opt-in above 64 KB.  With a deviation at γ = 0 the family returns the bits it returns without."""
    worst = [0.0]
    for case in R.size_cases(n):
        _check_case(case, gpu, worst)
        X, slots = R.pack([case])
        Xd = X.to(gpu)
        dev = torch.full((X.shape[1],), 0.5, device=gpu)
        assert torch.equal(ops.SpectralFamily(Xd, slots, dev)(0.0), ops.SpectralFamily(Xd, slots)(None))
    print(f"padding and tiles n={n}: worst err/bound {worst[0]:.3f}")


@pytest.mark.parametrize("n", R.GAP_N)
def test_gap_sweep_stays_inside_the_closed_form_truncation(gpu, n):
    """σ2/σ1 = 1 - 2^-j, a flat top and 2·I: the error is the 4096 power iterations' own, bounded by the closed form,
    and one-sided: a Rayleigh quotient cannot exceed the top eigenvalue by more than the Gram's rounding."""
    worst = [0.0]
    for case in R.gap_cases(n):
        _check_case(case, gpu, worst, one_sided=True)
    print(f"gap sweep n={n}: worst err/bound {worst[0]:.3f}")


@pytest.mark.parametrize("shape", R.SCALE_SHAPES)
def test_scale_contract(gpu, shape):
    """The same matrix times 10^e on every path: relative bound wherever the path's Gram is representable (fp32 Gram:
    σ in about [1e-18, 1e18]; fp64 Gram and the library: every e); outside it 0 below and non-finite above, never a
    finite wrong number."""
    worst = [0.0]
    for case in R.scale_cases(shape):
        vals = _values(case, gpu)
        assert _same_bits(vals[("family", True, None)], vals[("sum", True, None)])
        for (api, family, g), got in vals.items():
            p = R.path(*shape, family)
            rec = R.bound_of(case.X, None, None, family)[0]
            dom, v = R.in_domain(case, p), got.item()
            if dom == "in":
                R.check([v], [rec], f"{case.name} {api} ({p})", worst=worst)
            elif dom == "below":
                assert v == 0.0 or abs(v - rec.ref) <= rec.bound, (case.name, api, v, rec.ref)
            else:
                assert not math.isfinite(v), (case.name, api, v, rec.ref)
    print(f"scale {shape}: worst err/bound {worst[0]:.3f}")


@pytest.mark.parametrize("shape", R.RANGE_SHAPES)
def test_dynamic_range(gpu, shape):
    """Rank one plus 1e-6 noise, a dominant row, a dominant column, zero, a single entry, all entries equal."""
    worst = [0.0]
    for case in R.range_cases(shape):
        _check_case(case, gpu, worst)
        if case.name.endswith("-b"):
            z = _values(case, gpu)
            assert all(v[0].item() == 0.0 for v in z.values())  # the zero matrix is exactly 0, not NaN
    print(f"dynamic range {shape}: worst err/bound {worst[0]:.3f}")


@pytest.mark.parametrize("shape", R.CANCEL_SHAPES)
def test_gram_form_cancellation(gpu, shape):
    """X_j = γ0·D + E with ‖E‖/‖X‖ down to 1e-6 at γ0 and γ0(1 ± 2^-20): A - γS + γ²C is the small difference of large
    terms; the reference is the fp64-materialised rows, the bound the derived one (loose at 1e-6)."""
    worst = [0.0]
    for case in R.cancel_cases(shape):
        _check_case(case, gpu, worst)
    print(f"cancellation {shape}: worst err/bound {worst[0]:.3e}")


def test_family_with_deviation_on_and_off_the_gram_form(gpu):
    worst = [0.0]
    for case in R.family_cases():
        _check_case(case, gpu, worst)
    print(f"family: worst err/bound {worst[0]:.3f}")


# ------------------------------------------------------------------------------------------------ packed launches
def _direct_packed(Xd, slots):
    tab, max_n, scr, _ = ops._spectral_table(slots, Xd.device)
    return ops.native().spectral_norm_slots(Xd, tab, max_n, scr)


def _gram_packed(Xd, slots, dev=None, gamma=None):
    fam = ops.SpectralFamily(Xd, slots, dev)
    return ops.native().spec_eval(fam.arena, fam.tab, fam.sumq, Xd.shape[0], gamma)


def test_ragged_launch_gives_each_slot_the_bits_it_has_alone(gpu):
    """n = 1, 9, 64, 65, 128, 129 and a vector slot in one layout: k_spectral_slots sizes LDS by the largest n, each
    workgroup uses its own; every (row, slot) has the bits of that slot launched alone, twice."""
    cases = R.ragged_cases()
    X, slots = R.pack(cases, vector=7)
    Xd = X.to(gpu)
    small = [s for s in slots if min(s.shape[0], s.numel // s.shape[0]) <= R.DIRECT_NMAX]
    gram = [s for s in slots if R.gram_form(s.shape[0], s.numel // s.shape[0])]
    assert len(small) == len(slots) - 1 and len(gram) == 4
    for packed, group in ((_direct_packed, small), (_gram_packed, gram)):
        a, b = packed(Xd, group), packed(Xd, group)
        assert torch.equal(a, b)
        for i, s in enumerate(group):
            assert torch.equal(packed(Xd, [s])[:, 0], a[:, i]), s.name
    worst = [0.0]
    for family, fn in ((False, ops._spectral_slots_direct), (True, ops.spectral_norm_sum)):
        got = fn(Xd, slots).cpu()
        recs = [R.bound_of(R.slot_matrix(X, s), None, None, family) for s in slots]
        tot = [R.NS(ref=sum(r[m].ref for r in recs), bound=sum(r[m].bound for r in recs), round=0.0) for m in range(3)]
        R.check(got.tolist(), tot, f"ragged family={family}", worst=worst)
    print(f"ragged: worst err/bound {worst[0]:.3f}")


@pytest.mark.parametrize("kind", R.POISONS)
def test_non_finite_slot_gives_nan_and_leaves_the_rest_alone(gpu, kind):
    """One NaN entry, one +Inf entry or a whole NaN row in one (row, slot) of a packed launch: that (row, slot) is NaN
    (never distance 0, which a bisection would accept), every other one keeps its bits."""
    X, slots = R.pack(R.poison_cases(), vector=7)
    Xd, M = X.to(gpu), X.shape[0]
    g = torch.Generator().manual_seed(4)
    dev = (torch.rand(X.shape[1], generator=g) * 0.01).to(gpu)
    small = [s for s in slots if s.name != "poison-129x130"]
    gram = [s for s in slots if R.gram_form(s.shape[0], s.numel // s.shape[0])]
    two = _scalar(2.0, gpu)
    runs = {"direct": lambda Y: _direct_packed(Y, small), "gram": lambda Y: _gram_packed(Y, gram),
            "gram-dev": lambda Y: _gram_packed(Y, gram, dev, two)}
    sums = {"slots": lambda Y: ops._spectral_slots_direct(Y, slots), "sum": lambda Y: ops.spectral_norm_sum(Y, slots),
            "family-dev": lambda Y: ops.SpectralFamily(Y, slots, dev)(two)}
    clean = {k: f(Xd).cpu() for k, f in {**runs, **sums}.items()}
    assert all(bool(torch.isfinite(v).all()) for v in clean.values())
    for s in slots:
        if s.name == "vec":
            continue
        Yd = R.poison(X, s, 1, kind).to(gpu)
        for name, group in (("direct", small), ("gram", gram), ("gram-dev", gram)):
            got = runs[name](Yd).cpu()
            for i, t in enumerate(group):
                for m in range(M):
                    if (m, t.name) == (1, s.name):
                        assert math.isnan(got[m, i].item()), (name, kind, s.name, got[m, i].item())
                    else:
                        assert got[m, i].item() == clean[name][m, i].item(), (name, kind, s.name, t.name, m)
        for name, f in sums.items():
            got = f(Yd).cpu()
            assert math.isnan(got[1].item()), (name, kind, s.name, got[1].item())
            assert got[0].item() == clean[name][0].item() and got[2].item() == clean[name][2].item(), (name, kind, s.name)
        b = ops.batched_spectral_norm(R.slot_matrix(Yd, s).contiguous()).cpu()
        c = ops.batched_spectral_norm(R.slot_matrix(Xd, s).contiguous()).cpu()
        assert math.isnan(b[1].item()) and b[0].item() == c[0].item() and b[2].item() == c[2].item(), (kind, s.name)
    # a non-finite deviation or γ poisons every slot it touches
    bad = dev.clone()
    bad[gram[0].offset] = R.INF
    got = _gram_packed(Xd, gram, bad, two).cpu()
    assert bool(torch.isnan(got[:, 0]).all()) and torch.equal(got[:, 1:], clean["gram-dev"][:, 1:])
    assert bool(torch.isnan(_gram_packed(Xd, gram, dev, _scalar(R.NAN, gpu))).all())


# ------------------------------------------------------------------------------------------------ fused bisection
def _state(gamma0, gpu):
    st = torch.zeros(40, dtype=F64, device=gpu)
    st[0] = float(gamma0)
    return st


def _assert_state(st, n, want, label):
    tried, accs, succ, last = want
    st = st.cpu()
    assert st[4:4 + n].tolist() == tried, (label, st[4:4 + n].tolist(), tried)
    assert [x > 0.5 for x in st[20:20 + n].tolist()] == accs, (label, st[20:20 + n].tolist(), accs)
    assert st[1].item() == succ and st[2].item() == last, (label, st[1].item(), succ, st[2].item(), last)


def _coeffs(K, Sv, seed):
    """A_j = ‖x_j‖², B_j = <x_j, d>, C = ‖d‖² per vector slot, and the distances' decisive quantities at γ = 17."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(K, Sv, 6, dtype=F64, generator=g)
    d = torch.rand(Sv, 6, dtype=F64, generator=g) * 0.2
    vA, vB, vC = (x * x).sum(-1), (x * d[None]).sum(-1), (d * d).sum(-1)
    dist = torch.sqrt((vA - 2 * 17.0 * vB + 17.0 ** 2 * vC).clamp_min(0.0)).sum(1)
    dist[0] = 0.0
    return vA, vB, vC, dist


@pytest.mark.parametrize("K", [2, 3, 64, 65, 256, 257, 300])
def test_bisect_vec_matches_the_host_loop(gpu, K):
    """One wave, a wave boundary and the strided loop past 256 threads; Sv 1 and 3; max and sum of squares; 1, 6 and
    16 iterations: the tried γs, the decisions, st[1] and st[2] of an fp64 host loop on the same inputs.  Row 0 is
    ignored whatever its coefficients."""
    nat = ops.native()
    for Sv in (1, 3):
        vA, vB, vC, dist = _coeffs(K, Sv, 10 * K + Sv)
        for kind in (0, 1):
            thr = float((dist * dist).sum()) if kind else float(dist.max())
            for n_iter in (1, 6, 16):
                want = R.bisect_ref(vA, vB, vC, None, thr, kind, n_iter, 50.0)
                for row0 in (None, R.NAN, 1e300):
                    A = vA.clone()
                    if row0 is not None:
                        A[0] = row0
                    st = _state(50.0, gpu)
                    nat.bisect_vec(st, A.to(gpu), vB.to(gpu), vC.to(gpu), torch.tensor([thr], dtype=F64, device=gpu), K,
                                   kind, n_iter, 50.0)
                    _assert_state(st, n_iter, want, (K, Sv, kind, n_iter, row0))
                if n_iter == 16:
                    assert True in want[1] and False in want[1]  # the sweep sees both decisions
    with pytest.raises(RuntimeError):
        nat.bisect_vec(_state(50.0, gpu), vA.to(gpu), vB.to(gpu), vC.to(gpu), torch.tensor([1.0], dtype=F64, device=gpu),
                       K, 0, 17, 50.0)


def test_bisect_vec_strictness_clamp_and_nan(gpu):
    """A threshold exactly equal to the decisive quantity rejects (exactly representable A, B, C), one ulp above
    accepts; a negative A - 2γB + γ²C counts as 0; a NaN coefficient rejects every γ."""
    nat = ops.native()
    t = lambda v: torch.tensor(v, dtype=F64, device=gpu)

    def run(vA, vB, vC, thr, kind, n=1, g0=4.0):
        st = _state(g0, gpu)
        nat.bisect_vec(st, t(vA), t(vB), t(vC), t([thr]), len(vA), kind, n, g0)
        return st

    # γ = 4, Sv = 1: row 1 25 - 16 + 16 = 25, row 2 9 + 16 = 25 -> max 5, Σ d² = 50
    vA, vB, vC = [[999.0], [25.0], [9.0]], [[5.0], [2.0], [0.0]], [1.0]
    for kind, q in ((0, 5.0), (1, 50.0)):
        for thr, acc in ((q, False), (math.nextafter(q, R.INF), True), (math.nextafter(q, 0.0), False)):
            st = run(vA, vB, vC, thr, kind)
            _assert_state(st, 1, R.bisect_ref(t(vA).cpu(), t(vB).cpu(), t(vC).cpu(), None, thr, kind, 1, 4.0), (kind, thr))
            assert (st[20].item() > 0.5) == acc
    # Sv = 3: 3 + 4 + 5 = 12 exactly
    A3, B3, C3 = [[0.0] * 3, [9.0, 16.0, 25.0]], [[0.0] * 3, [2.0, 2.0, 2.0]], [1.0, 1.0, 1.0]
    assert run(A3, B3, C3, 12.0, 0)[20].item() == 0.0 and run(A3, B3, C3, math.nextafter(12.0, R.INF), 0)[20].item() == 1.0
    assert run(A3, B3, C3, 144.0, 1)[20].item() == 0.0 and run(A3, B3, C3, math.nextafter(144.0, R.INF), 1)[20].item() == 1.0
    # 1 - 16 < 0: clamped, distance 0 < any positive threshold
    assert run([[0.0], [1.0]], [[0.0], [2.0]], [0.0], 1e-300, 0)[20].item() == 1.0
    # a NaN in vA (row >= 1): every γ of 6 iterations is rejected, γ walks down
    vA, vB, vC, dist = _coeffs(9, 2, 5)
    vA[4, 1] = R.NAN
    for kind in (0, 1):
        st = _state(50.0, gpu)
        nat.bisect_vec(st, vA.to(gpu), vB.to(gpu), vC.to(gpu), t([1e300]), 9, kind, 6, 50.0)
        _assert_state(st, 6, R.bisect_ref(vA, vB, vC, None, 1e300, kind, 6, 50.0), ("nan", kind))
        assert st[20:26].tolist() == [0.0] * 6 and st[1].item() == 0.0


_BIS_SHAPES = ((9, 12), (16, 16), (33, 20), (5, 40), (17, 3), (1, 6), (64, 10), (8, 8), (12, 9))


def _bisect_layout(S, M, seed, gpu):
    slots, off = [], 0
    for i in range(S):
        r, c = _BIS_SHAPES[i]
        slots.append(TensorSlot(f"s{i}", (r, c), off, r * c))
        off += r * c
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(M, off, generator=g) * 0.05
    dev = torch.rand(off, generator=g) * 0.01
    return slots, X, dev


def _run_spec_bisect(fam, M, vec, thr, kind, gpu, n=10, gamma0=50.0):
    """n spec_bisect launches against spec_eval at the same γ plus the host decision -> the final state."""
    nat = ops.native()
    st, ctr = _state(gamma0, gpu), torch.zeros(1, dtype=torch.int32, device=gpu)
    vd = [None if v is None else v.to(gpu) for v in vec]
    thr_d = torch.tensor([thr], dtype=F64, device=gpu)
    step, seen = gamma0, {}
    for it in range(n):
        g = st[0].item()
        out = nat.spec_bisect(fam.arena, fam.tab, fam.sumq, M, st, ctr, vd[0], vd[1], vd[2], thr_d, kind, it, step)
        ref = nat.spec_eval(fam.arena, fam.tab, fam.sumq, M, _scalar(g, gpu))
        assert _same_bits(out, ref), (it, g)  # to the bit, a NaN included
        assert ctr.item() == 0, (it, ctr.item())  # the arrival counter is back at 0 after every launch
        seen[g] = ref.cpu()
        step /= 2.0
    want = R.bisect_ref(vec[0], vec[1], vec[2], lambda gg: seen[gg], thr, kind, n, gamma0)
    _assert_state(st, n, want, (M, kind))
    return st, want


@pytest.mark.parametrize("M,S", [(1, 1), (1, 5), (4, 1), (9, 7), (40, 9)])
def test_spec_bisect_matches_spec_eval_and_the_host_decision(gpu, M, S):
    """All 10 launches of a γ0 = 50, τ = 0.05 run; (1, 1): the only workgroup is also the last arrival, (40, 9): 360
    workgroups fan in.  Each launch's ``out`` has the bits of spec_eval at that γ; the decisions are the host's."""
    assert attacks.bisect_iterations(50.0, 0.05) == 10
    slots, X, dev = _bisect_layout(S, M, 100 * M + S, gpu)
    fam = ops.SpectralFamily(X.to(gpu), slots, dev.to(gpu))
    assert not fam.rest
    base = fam(17.0).cpu()
    for with_vec in (False, True):
        vec, dist = (None, None, None), torch.cat([torch.zeros(1, dtype=F64), base])
        if with_vec:
            vA, vB, vC, dv = _coeffs(M + 1, 2, M + S)
            vec, dist = (vA * 0.01, vB * 0.01, vC * 0.01), dist + 0.1 * dv
        for kind in (0, 1):
            thr = float((dist * dist).sum()) if kind else float(dist.max())
            st, want = _run_spec_bisect(fam, M, vec, thr, kind, gpu)
            assert True in want[1] and False in want[1]
    # a NaN slot in one row: every γ is rejected
    Xn = X.clone()
    Xn[M - 1, slots[S - 1].offset + 1] = R.NAN
    famn = ops.SpectralFamily(Xn.to(gpu), slots, dev.to(gpu))
    for kind in (0, 1):
        st, want = _run_spec_bisect(famn, M, (None, None, None), 1e300, kind, gpu)
        assert want[1] == [False] * 10 and st[1].item() == 0.0


@pytest.mark.parametrize("K", [2, 9, 33])
@pytest.mark.parametrize("fn", [attacks.min_max, attacks.min_sum, attacks.opt_fang])
def test_fused_bisection_matches_generic_and_cpu_on_small_slots(gpu, K, fn, monkeypatch):
    """fused == generic device loop == CPU on a layout of small slots (n = 9, 16, 33 and a vector) at K other than 5."""
    lay = ParamLayout([TensorSlot("a", (9, 14), 0, 126), TensorSlot("v", (7,), 126, 7), TensorSlot("b", (16, 16), 133, 256),
                       TensorSlot("c", (40, 33), 389, 1320)])
    g = torch.Generator().manual_seed(K)
    G = torch.randn(1, lay.P, generator=g) * 0.3 + 0.1 * torch.randn(K, lay.P, generator=g)
    eng = attacks.DistanceEngine(lay, "spectral")
    cpu = attacks.host_info(fn(G, G[0], eng).info)
    Gd = G.to(gpu)
    fused = fn(Gd, Gd[0], eng)
    hf = attacks.host_info(fused.info)
    monkeypatch.setattr(attacks, "_bisect_fused", lambda *a, **k: None)  # force the generic device loop
    gen = fn(Gd, Gd[0], eng)
    hg = attacks.host_info(gen.info)
    assert hf["gammas"] == hg["gammas"] == cpu["gammas"]
    assert hf["accepted"] == hg["accepted"] == cpu["accepted"]
    assert hf["gamma"] == cpu["gamma"] and hf["gamma_succ"] == cpu["gamma_succ"]
    assert torch.equal(fused.params, gen.params)


# ------------------------------------------------------------------------------------------------ ROC-AUC
def _auc_exact(got, s, y, label):
    """The kernels' sums are exact integers: 2U reconstructed from the result equals the oracle's, and the quotient is
    within one ulp of the oracle's fp64 quotient."""
    two_u, P, N = R.auc_two_u(s, y)
    if P == 0 or N == 0:
        assert math.isnan(got), (label, got)
        return
    want = two_u / (2.0 * P * N)
    assert round(got * 2.0 * P * N) == two_u and abs(got - want) <= math.ulp(want), (label, got, want, two_u, P, N)


@pytest.mark.parametrize("n", R.AUC_LENGTHS)
def test_auc_lengths(gpu, n):
    """A wave (64), a block (256), the j chunk (1024), two chunks and a tail (2049), the pair/sort switch (32768/9)."""
    s, y = R.auc_data(n)
    got, flag = ops.roc_auc_checked(s.to(gpu), y.to(gpu))
    assert flag is False
    _auc_exact(got, s, y, n)
    assert ops.roc_auc_checked(s.to(gpu), y.to(gpu))[0] == got or math.isnan(got)


def test_auc_pair_and_sort_paths_agree(gpu):
    """n = 32769 is an n = 32768 case plus one sample: both oracles, both paths, and the difference is the appended
    sample's own pair count."""
    s, y = R.auc_data(32768)
    for extra_s, extra_y in ((0.5, 1.0), (0.5, 0.0), (-1.0, 1.0), (9.0, 0.0)):
        s2, y2 = torch.cat([s, torch.tensor([extra_s])]), torch.cat([y, torch.tensor([extra_y])])
        a = ops.roc_auc_checked(s.to(gpu), y.to(gpu))[0]
        b = ops.roc_auc_checked(s2.to(gpu), y2.to(gpu))[0]
        _auc_exact(a, s, y, "pairs")
        _auc_exact(b, s2, y2, "sort")
        ua, ub = R.auc_two_u(s, y), R.auc_two_u(s2, y2)
        other = s[y < 0.5] if extra_y > 0.5 else s[y > 0.5]
        lt = (other < extra_s) if extra_y > 0.5 else (other > extra_s)
        assert ub[0] - ua[0] == int(2 * lt.sum() + (other == extra_s).sum())
        assert round(b * 2.0 * ub[1] * ub[2]) - round(a * 2.0 * ua[1] * ua[2]) == ub[0] - ua[0]


@pytest.mark.parametrize("n", [300, 32769])
def test_auc_values(gpu, n):
    """All tied (0.5), two values, ±Inf, -0.0 against +0.0, denormals, a single positive / negative, one class (NaN),
    labels 0.49 / 0.51, on the pair path and on the sort path."""
    for name, (s, y, want) in R.auc_value_cases(n).items():
        got, flag = ops.roc_auc_checked(s.to(gpu), y.to(gpu))
        assert flag is False, name
        _auc_exact(got, s, y, name)
        if want is not None:
            assert (math.isnan(want) and math.isnan(got)) or got == want, (name, got, want)


@pytest.mark.parametrize("n,idx", [(2049, 0), (2049, 1023), (2049, 1024), (2049, 2047), (2049, 2048), (32769, 0),
                                   (32769, 32768)])
def test_auc_nan_score_raises_the_flag(gpu, n, idx):
    """A NaN score on a positive and on a negative, at the first and the last index of a chunk: the flag is the contract."""
    s, y = R.auc_data(n)
    for label in (1.0, 0.0):
        s2, y2 = s.clone(), y.clone()
        s2[idx], y2[idx] = R.NAN, label
        assert ops.roc_auc_checked(s2.to(gpu), y2.to(gpu))[1] is True, (n, idx, label)
