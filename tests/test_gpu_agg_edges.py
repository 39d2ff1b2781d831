"""The aggregation kernels of ``csrc/kernels/agg.hip`` at the shapes and values where kernels go wrong — sizes around
every tile, chunk and template boundary, one row, outlier rows, ties, signed zeros, infinities, NaN — against the fp64
references of ``tests/test_agg_oracles.py`` (plain torch, checked there against the composites on the CPU).  Bounds
come from the number formats and the kernels' summation, not from the kernels' output."""
import math

import pytest
import torch

import test_agg_oracles as R
from attackfl_amd import agg, ops
from attackfl_amd.models import TensorSlot
from attackfl_amd.ops import native

pytestmark = pytest.mark.gpu


def rel_err(got, ref):
    """Worst |got - ref| / ref over the off-diagonal pairs."""
    off = ~torch.eye(ref.shape[0], dtype=torch.bool)
    return float(((got - ref).abs() / ref)[off].max()) if ref.shape[0] > 1 else 0.0


def check_distance_matrix(got, ref, what):
    rel = rel_err(got, ref)
    print(f"{what}: worst relative error {rel:.3e}")
    assert rel <= 1e-9, (what, rel)
    assert torch.equal(got, got.t()) and bool((got.diagonal() == 0).all()), what


# ------------------------------------------------------------------------------------------ pairwise distances
@pytest.mark.parametrize("scale", [1, 1000])
@pytest.mark.parametrize("P", [5, 3001])
@pytest.mark.parametrize("K,n_out", R.MINORITY)
def test_gram_distances_with_minority_outliers(gpu, K, n_out, P, scale):
    """Every pair within 1e-9 relative (no absolute term) of the fp64 difference form wherever the outlier rows sit:
    with the outliers first, row 0 — the first pass's centre — is one of them."""
    got = {}
    for first in (True, False):
        G = R.outlier_rows(K, n_out, P, scale, first)
        Gd = G.to(gpu)
        D = native().pairwise_sqdist_gram(Gd)
        got[first] = D.cpu()
        check_distance_matrix(got[first], R.ref_sqdist(G), f"gram K={K} out={n_out} P={P} scale={scale} first={first}")
        assert torch.equal(native().pairwise_sqdist_gram(Gd), D)  # bit-identical run to run
        assert torch.equal(ops.pairwise_sqdist(Gd), D)            # the dispatcher takes this path
    perm = R.first_to_last(K, n_out)
    a, b = got[True][perm][:, perm], got[False]
    assert rel_err(a, b) <= 1e-9  # the client index of the attackers does not matter


@pytest.mark.parametrize("K,P", [(2, 5), (2, 3001), (9, 5), (9, 3001)])
def test_gram_distances_iid_rows(gpu, K, P):
    """Rows all mutually far apart (no typical row to centre on): the same bound."""
    G = torch.randn(K, P, generator=R._gen(K, P, 31))
    D = native().pairwise_sqdist_gram(G.to(gpu))
    check_distance_matrix(D.cpu(), R.ref_sqdist(G), f"gram iid K={K} P={P}")
    assert torch.equal(native().pairwise_sqdist_gram(G.to(gpu)), D)


def test_gram_distances_two_distant_clusters(gpu):
    """The documented limit of the Gram form: with two tight clusters 1000 apart no centre is close to every row, so
    the far cluster's within-cluster distances carry an absolute error of eps64 times the squared gap.  Held to the
    existing tolerance form rtol = 1e-9, atol = 1e-12 (max(ref) + 1), not to the relative bound alone."""
    G = R.cluster_rows()
    got = native().pairwise_sqdist_gram(G.to(gpu)).cpu()
    ref = R.ref_sqdist(G)
    print(f"two clusters: worst relative error {rel_err(got, ref):.3e}, worst absolute "
          f"{float((got - ref).abs().max()):.3e}")
    assert torch.allclose(got, ref, rtol=1e-9, atol=1e-12 * float(ref.max() + 1))
    assert torch.equal(got, got.t()) and bool((got.diagonal() == 0).all())


def test_gram_distances_with_a_nan_row(gpu):
    """A NaN row (a faulted client) as documented in agg.hip: its own distances come out 0 (the clamp), it is never
    the second pass's centre and the other rows keep the 1e-9 bound, also with an outlier in row 0; a NaN row 0, the
    first pass's centre, gives an all-zero matrix."""
    G = R.outlier_rows(9, 1, 3001, 1000, True).clone()
    G[4] = float("nan")
    got = native().pairwise_sqdist_gram(G.to(gpu)).cpu()
    keep = [i for i in range(9) if i != 4]
    assert bool((got[4] == 0).all()) and bool((got[:, 4] == 0).all())
    check_distance_matrix(got[keep][:, keep], R.ref_sqdist(G[keep]), "gram with a NaN row 4")
    G = R.outlier_rows(9, 0, 3001, 1, True).clone()
    G[0, 7] = float("nan")
    assert bool((native().pairwise_sqdist_gram(G.to(gpu)) == 0).all())


def test_gram_centred_with_outlier_in_row_0(gpu):
    """gram_centred reads the Gram of the final centre; the double centring gives the mean-centred Gram whichever
    row that is."""
    U = R.outlier_rows(9, 1, 3001, 1000, True)
    got = native().gram_centred(U.to(gpu))[0].cpu()
    ref = R.ref_gram_centred(U)
    assert torch.allclose(got, ref, rtol=1e-9, atol=1e-9 * float(ref.abs().max()))


@pytest.mark.parametrize("P", [5, 257, 3001])
@pytest.mark.parametrize("K", [2, 9, 64, 65, 128])
def test_difference_kernel(gpu, K, P):
    """k_pair_sqdist directly (the route of 65 - 128 rows, more than 64 KB of LDS from K = 64 on): the difference and
    the square are fp64, so the worst case is P * 2^-53 relative."""
    for n_out in (0, max(1, K // 4)):
        G = R.outlier_rows(K, n_out, P, 1000, True)
        D = native().pairwise_sqdist(G.to(gpu))
        check_distance_matrix(D.cpu(), R.ref_sqdist(G), f"difference K={K} P={P} out={n_out}")
        assert torch.equal(native().pairwise_sqdist(G.to(gpu)), D)


def test_difference_kernel_limits_and_dispatch(gpu):
    one = native().pairwise_sqdist(torch.randn(1, 300).to(gpu))
    assert one.shape == (1, 1) and one.dtype == torch.float64 and float(one) == 0.0
    with pytest.raises(RuntimeError):
        native().pairwise_sqdist(torch.randn(129, 40).to(gpu))
    G = R.outlier_rows(70, 3, 257, 1000, True).to(gpu)
    assert torch.equal(ops.pairwise_sqdist(G), native().pairwise_sqdist(G))  # K > 64 takes the difference kernel


def _far_rows():
    g = R._gen(70, 3001, 41)
    U = torch.randn(1, 3001, generator=g) + 0.1 * torch.randn(70, 3001, generator=g)
    for r in (0, 33, 69):
        U[r] = 3.0 * torch.randn(3001, generator=g) + 2.0
    return U


def test_krum_and_multi_krum_beyond_64_rows(gpu):
    """n = 70 (difference kernel, composite selection on the device) with three far rows: the device runs select what
    the CPU runs select."""
    U = _far_rows()
    cpu, dev = agg.krum(U), agg.krum(U.to(gpu))
    assert int(dev.info["selected"]) == int(cpu.info["selected"]) and int(cpu.info["selected"]) not in (0, 33, 69)
    assert torch.equal(dev.params.cpu(), cpu.params)
    sizes = torch.tensor([300.0 + 37.0 * ((5 * i) % 7) for i in range(70)])
    cpu, dev = agg.multi_krum(U, sizes), agg.multi_krum(U.to(gpu), sizes)
    keep = cpu.info["selected"]
    assert torch.equal(dev.info["selected"].cpu(), keep) and not bool(keep[[0, 33, 69]].any())
    assert int(keep.sum()) == 70 - cpu.info["f"]
    assert torch.allclose(dev.params.cpu(), cpu.params, rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------ median / trimmed mean
@pytest.mark.parametrize("N,P", R.SELECT_SHAPES)
def test_median_and_trimmed_mean_shapes(gpu, N, P):
    U = R.select_rows(N, P)
    Ud = U.to(gpu)
    med = ops.coord_median(Ud).cpu()
    assert torch.equal(med, R.ref_median(U)) and torch.equal(med, torch.median(U, dim=0).values)
    for trim in R.trims(N):
        ref, bound = R.ref_trimmed(U, trim)
        got = ops.trimmed_mean(Ud, trim).cpu()
        print(f"trimmed N={N} P={P} trim={trim}: worst error / bound "
              f"{float(((got.double() - ref).abs() / bound).max()):.3f}")
        assert R.within(got, ref, bound), (N, P, trim)


@pytest.mark.parametrize("N", [3, 8, 11])
def test_median_and_trimmed_mean_special_columns(gpu, N):
    """Heavy ties, -0.0 against 0.0 (values, not sign bits), real infinities, one and two NaNs per column: the median is
    NaN wherever a NaN is present (torch.median), the trimmed mean NaN iff the column holds more NaNs than trim
    (torch.sort places NaN last) and the mean of the sorted slice otherwise."""
    U, nn = R.special_columns(N)
    Ud = U.to(gpu)
    med = ops.coord_median(Ud).cpu()
    assert R.same_values(med, R.ref_median(U)) and R.same_values(med, torch.median(U, dim=0).values)
    assert bool((torch.isnan(med) == (nn > 0)).all())
    for trim in R.trims(N):
        got = ops.trimmed_mean(Ud, trim).cpu()
        ref, bound = R.ref_trimmed(U, trim)
        assert bool((torch.isnan(got)[8:] == (nn > trim)[8:]).all()), (N, trim, got)
        assert R.within(got, ref, bound), (N, trim, got, ref)
        s32 = torch.sort(U, dim=0).values[trim:N - trim].mean(0)
        assert R.within(got, s32, 2 * bound), (N, trim, got, s32)  # (both within ``bound`` of the fp64 mean)


def test_coord_select_refuses_65_rows(gpu):
    with pytest.raises(RuntimeError):
        ops.coord_median(torch.randn(65, 10).to(gpu))
    with pytest.raises(RuntimeError):
        ops.trimmed_mean(torch.randn(65, 10).to(gpu), 1)


@pytest.mark.parametrize("theta", [5, 8, 11])
def test_bulyan_coord_nan_follows_composite(gpu, theta):
    """NaN in the selected rows as composite.bulyan_coord: NaN once beta exceeds the real values of the column, the
    beta smallest values when the median itself is NaN, the real values closest to the median otherwise."""
    U = R.bulyan_nan_rows(theta)
    sel = torch.arange(theta).flip(0)
    for beta in (1, 2, theta - 2, theta):
        got = ops.bulyan_coord(U.to(gpu), sel.to(gpu), beta).cpu()
        for c in range(U.shape[1]):
            want = R.ref_bulyan_column(U[:theta, c].tolist(), beta)
            if math.isnan(want):
                assert math.isnan(float(got[c])), (theta, beta, c, got)
            else:
                assert abs(float(got[c]) - want) <= 2.0 ** -23 * abs(want) + 1e-12, (theta, beta, c, got)


# ------------------------------------------------------------------------------------------ column statistics
@pytest.mark.parametrize("P", [1, 255, 256, 257])
@pytest.mark.parametrize("K", [1, 2, 3, 64, 100])
def test_colstats_and_lie(gpu, K, P):
    """Mean and std within one fp32 ulp of the rounded fp64 two-pass reference, also on columns of mean 1e4 and
    spread 1e-2; the LIE candidate within one ulp of its two terms."""
    G = R.colstat_rows(K, P)
    mean, std = R.ref_colstats(G)
    m32, s32 = mean.float().double(), std.float().double()
    gm, gs = ops.column_mean_std(G.to(gpu))
    gm, gs = gm.cpu().double(), gs.cpu().double()
    assert bool(((gm - m32).abs() <= R.EPS32 * m32.abs()).all())
    if K == 1:
        assert torch.isnan(gs).all()
    else:
        assert bool(((gs - s32).abs() <= R.EPS32 * s32.abs()).all())
    for z in (0.74, -1.5):
        out = ops.lie_candidate(G.to(gpu), z).cpu().double()
        if K == 1:
            assert torch.isnan(out).all()
            continue
        want = m32 + z * s32  # (the rounded fp64 reference, not the kernel's own mean and std)
        err, bound = (out - want).abs(), R.EPS32 * (m32.abs() + (z * s32).abs())
        print(f"lie K={K} P={P} z={z}: worst error / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())


# ------------------------------------------------------------------------------------------ weighted rows
@pytest.mark.parametrize("P", [1, 255, 256, 257])
@pytest.mark.parametrize("N", [1, 2, 64, 100])
def test_weighted_rows(gpu, N, P):
    U, w = R.weighted_case(N, P)
    ref, bound = R.ref_weighted(U, w)
    got = ops.weighted_rows(U.to(gpu), w.to(gpu)).cpu()
    assert R.within(got, ref, bound), float((got.double() - ref.double()).abs().max())


@pytest.mark.parametrize("N", [1, 3])
def test_weighted_rows_ok_entries(gpu, N):
    """The fallback is taken iff any ``ok`` entry is <= 0 (0 and -1), bit-equal to ``fallback``; 2 counts as success."""
    U, w = R.weighted_case(N, 257)
    fb = torch.randn(257, generator=R._gen(N, 43))
    Ud, wd, fbd = U.to(gpu), w.to(gpu), fb.to(gpu)
    plain = ops.weighted_rows(Ud, wd)
    for bad in (0, -1):
        for pos in range(N):
            ok = torch.full((N,), 2, dtype=torch.int32)
            ok[pos] = bad
            assert torch.equal(ops.weighted_rows(Ud, wd, ok.to(gpu), fbd).cpu(), fb), (bad, pos)
    for good in (1, 2):
        ok = torch.full((N,), good, dtype=torch.int32)
        assert torch.equal(ops.weighted_rows(Ud, wd, ok.to(gpu), fbd), plain)
    ref, bound = R.ref_weighted(U, w)
    assert R.within(plain.cpu(), ref, bound)


# ------------------------------------------------------------------------------------------ row dots
@pytest.mark.parametrize("P", [1, 255, 8191, 8192, 8193, 16385])
@pytest.mark.parametrize("N", [1, 3])
def test_row_dots_around_the_chunk(gpu, N, P):
    U, r = R.dots_case(N, P)
    Ud = U.to(gpu)
    ref = R.ref_dots(U, r)
    assert torch.allclose(native().row_dots(Ud, r.to(gpu), 1).cpu(), ref, rtol=1e-9, atol=0)
    assert torch.allclose(ops.row_norms(Ud).cpu(), ref[:, 0].sqrt(), rtol=1e-9, atol=0)
    cos = ops.cosine_to(Ud, r.to(gpu)).cpu()
    assert torch.allclose(cos, R.ref_cosine(U, r), rtol=0, atol=1e-9)
    if N > 1:
        assert float(cos[1]) == 0.0  # the all-zero row
    assert ops.cosine_to(Ud, torch.zeros(P).to(gpu)).cpu().tolist() == [0.0] * N  # an all-zero reference vector


# ------------------------------------------------------------------------------------------ segment reductions
def check_segments(gpu, G, mean, dev, slots):
    A, B, Cc, L2 = R.ref_segments(G, mean, dev, slots)
    a, b, c = ops.attack_coeffs_segments(G.to(gpu), mean.to(gpu), dev.to(gpu), slots)
    assert torch.allclose(a.cpu(), A, rtol=1e-9, atol=0) and torch.allclose(c.cpu(), Cc, rtol=1e-9, atol=0)
    assert torch.allclose(b.cpu(), B, rtol=1e-9, atol=1e-9)
    assert torch.allclose(ops.segment_l2_sum(G.to(gpu), slots).cpu(), L2, rtol=1e-9, atol=0)


@pytest.mark.parametrize("K", [1, 4])
def test_segments_around_the_tile(gpu, K):
    """Slots of 1 .. 8193 columns around the 4096 tile with unused columns between two of them and after the last."""
    slots, P = R.edge_layout()
    G, mean, dev = R.segment_case(K, P)
    check_segments(gpu, G, mean, dev, slots)
    whole = [TensorSlot("all", (P,), 0, P)]
    A, B, Cc, _ = R.ref_segments(G, mean, dev, whole)
    a, b, c = ops.attack_coeffs(G.to(gpu), mean.to(gpu), dev.to(gpu))
    assert torch.allclose(a.cpu(), A[:, 0], rtol=1e-9, atol=0) and torch.allclose(b.cpu(), B[:, 0], rtol=1e-9, atol=1e-9)
    assert torch.allclose(c.cpu(), Cc[0], rtol=1e-9, atol=0)


@pytest.mark.parametrize("K", [1, 4])
def test_segments_single_column(gpu, K):
    G, mean, dev = R.segment_case(K, 1)
    check_segments(gpu, G, mean, dev, [TensorSlot("all", (1,), 0, 1)])


# ------------------------------------------------------------------------------------------ flat Adam
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_adam_flat_edges(gpu, n, scale):
    """Steps 1 .. 5 and one at step 1000 against fp64 Adam; one element has a zero gradient (v = 0: the denominator is
    eps) and must not move."""
    p0, gr = R.adam_case(n)
    pd, md, vd = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    p, m, v = p0.clone().to(gpu), torch.zeros(n).to(gpu), torch.zeros(n).to(gpu)
    for step in R.ADAM_STEPS:
        ops.adam_step_scaled(p, gr.to(gpu), m, v, step, 1e-3, scale)
        pd, md, vd = R.ref_adam(pd, gr, md, vd, step, 1e-3, scale)
        assert torch.allclose(p.cpu().double(), pd, rtol=0, atol=1e-6), step
    # the moments: the kernel forms 1 - beta in fp32 from the rounded beta, an error of up to 2^-25 / (1 - beta) relative
    # (3e-7 for beta1 = 0.9, 3e-5 for beta2 = 0.999) on top of a few fp32 roundings per step
    assert torch.allclose(m.cpu().double(), md, rtol=2e-6, atol=1e-7)
    assert torch.allclose(v.cpu().double(), vd, rtol=1e-4, atol=1e-10)
    if n > 1:
        assert float(p[n // 2]) == float(p0[n // 2])
