"""fp64 references of the aggregation kernels (``csrc/kernels/agg.hip``), written out with plain torch operations, and
their CPU checks: every reference against the composite it is meant to agree with (so a wrong oracle shows on a
machine without a GPU), plus the composite behaviours the kernels follow (``torch.median`` propagates NaN,
``torch.sort`` places NaN last, the composite distances stay accurate on benign rows).

``tests/test_gpu_agg_edges.py`` holds the same references against the kernels.  No reference goes through ``ops``.
"""
import functools
import math

import pytest
import torch

from attackfl_amd.models import TensorSlot
from attackfl_amd.ops import composite as C

NAN, INF = float("nan"), float("inf")
EPS32, EPS64 = 2.0 ** -23, 2.0 ** -52


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------ pairwise distances
def ref_sqdist(G):
    """fp64 difference form ((Gd[:, None] - Gd[None]) ** 2).sum(-1), one row of the result at a time."""
    Gd = G.double()
    return torch.stack([((Gd[i][None, :] - Gd) ** 2).sum(-1) for i in range(Gd.shape[0])])


@functools.lru_cache(maxsize=None)
def outlier_rows(K, n_out, P, scale, first, seed=0):
    """Rows base + 1e-3 randn, n_out of them replaced by base + scale randn, the outliers placed first or last (the
    same rows in both orders).  n_out = 0: benign rows only.  The base has std 0.3 (model weights): the kernels
    remove it exactly, but the composite's raw Gram form carries an error of about
    2^-53 (|G_i|^2 + |G_j|^2) / D_ij = 2^-53 * 0.09 / 1e-6 = 1e-11 per rounding with it (1e-10 with a base of std 1,
    where it was measured at 1.06e-9 for K = 64, P = 257: past the 1e-9 the distances are held to)."""
    g = _gen(K, n_out, P, int(scale), seed)
    base = 0.3 * torch.randn(1, P, generator=g)
    benign = base + 1e-3 * torch.randn(K - n_out, P, generator=g)
    out = base + float(scale) * torch.randn(n_out, P, generator=g)
    return torch.cat([out, benign] if first else [benign, out]).contiguous()


def first_to_last(K, n_out):
    """Row permutation p with outlier_rows(first=False) == outlier_rows(first=True)[p]."""
    return list(range(n_out, K)) + list(range(n_out))


def pick_centre(D):
    """The Gram path's second centre: argmin_i lowermedian_{j != i} D[i][j], ties to the lowest index."""
    K = D.shape[0]
    if K < 2:
        return 0
    off = D.double().masked_fill(torch.eye(K, dtype=torch.bool), INF)
    med = torch.sort(off, dim=1).values[:, (K - 2) // 2]
    return int(torch.argmin(med))  # (the first minimum)


@functools.lru_cache(maxsize=None)
def cluster_rows(P=3001):
    """Two tight clusters of four rows, their bases 1000 apart."""
    g = _gen(8, P, 77)
    base = torch.randn(1, P, generator=g)
    d = torch.randn(1, P, generator=g)
    far = base + 1000.0 * d / d.norm()
    return torch.cat([base + 1e-3 * torch.randn(4, P, generator=g), far + 1e-3 * torch.randn(4, P, generator=g)])


def ref_gram_centred(U):
    X = U.double()
    Xc = X - X.mean(dim=0, keepdim=True)
    return Xc @ Xc.t()


MINORITY = [(5, 2), (8, 1), (8, 3), (17, 4), (64, 15)]


@pytest.mark.parametrize("K,n_out", MINORITY)
@pytest.mark.parametrize("P", [5, 3001])
@pytest.mark.parametrize("scale", [1, 1000])
def test_outlier_rows_and_centre_rule(K, n_out, P, scale):
    """The two orders hold the same rows; with a minority of outliers (K - 1 - n_out >= (K - 2) // 2 + 1) the centre
    rule applied to the exact distances picks a benign row."""
    assert K - 1 - n_out >= (K - 2) // 2 + 1
    a, b = outlier_rows(K, n_out, P, scale, True), outlier_rows(K, n_out, P, scale, False)
    perm = first_to_last(K, n_out)
    assert torch.equal(a[perm], b)
    Da, Db = ref_sqdist(a), ref_sqdist(b)
    assert torch.equal(Da[perm][:, perm], Db)
    assert pick_centre(Da) >= n_out and pick_centre(Db) < K - n_out


@pytest.mark.parametrize("K,P", [(2, 5), (9, 3001), (64, 257), (70, 3001)])
def test_composite_distances_accurate_on_benign_rows(K, P):
    """composite.pairwise_l2 ** 2 (raw Gram form in fp64) within 1e-9 relative of the difference form on benign rows."""
    G = outlier_rows(K, 0, P, 1, True)
    ref = ref_sqdist(G)
    got = C.pairwise_l2(G) ** 2
    off = ~torch.eye(K, dtype=torch.bool)
    rel = ((got - ref).abs() / ref)[off].max().item()
    print(f"composite vs difference form, K={K} P={P}: worst relative error {rel:.3e}")
    assert rel <= 1e-9
    assert bool((got.diagonal() == 0).all())


def test_gram_centred_reference_matches_composite_route():
    U = outlier_rows(9, 1, 3001, 1000, True)
    X = U.double()
    H = (X - X[4]) @ (X - X[4]).t()  # any centre row: the double centring removes it
    Cc = H - H.mean(0, keepdim=True) - H.mean(1, keepdim=True) + H.mean()
    ref = ref_gram_centred(U)
    assert torch.allclose(Cc, ref, rtol=1e-9, atol=1e-9 * float(ref.abs().max()))


# ------------------------------------------------------------------------------------------ median / trimmed mean
def ref_median(U):
    """Lower median, sort(U.double(), 0)[(N - 1) // 2] cast back; NaN for a column that holds a NaN."""
    N = U.shape[0]
    med = torch.sort(U.double(), dim=0).values[(N - 1) // 2]
    return torch.where(torch.isnan(U).any(dim=0), torch.full_like(med, NAN), med).to(U.dtype)


def ref_trimmed(U, trim):
    """(fp64 mean of the sorted slice [trim, N - trim), error bound of a sequential fp32 sum of its m terms plus one
    division: m * 2^-24 * sum|kept| / m + 2^-23 |ref|).  torch.sort places NaN last: NaN iff NaNs > trim."""
    N = U.shape[0]
    kept = torch.sort(U.double(), dim=0).values[trim:N - trim]
    m = N - 2 * trim
    ref = kept.mean(dim=0)
    bound = (m * 2.0 ** -24 * kept.abs().sum(dim=0)) / m + EPS32 * ref.abs()
    return ref, bound


def same_values(a, b):
    """Elementwise equal as values: -0.0 == 0.0, NaN matches NaN."""
    a, b = a.double(), b.double()
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def within(got, ref, bound):
    """|got - ref| <= bound where ref is finite; the same infinity or NaN where it is not."""
    got, ref = got.double(), ref.double()
    fin = torch.isfinite(ref)
    ok_fin = (got - ref).abs() <= bound
    ok_non = (got == ref) | (torch.isnan(got) & torch.isnan(ref))
    return bool(torch.where(fin, ok_fin, ok_non).all())


@functools.lru_cache(maxsize=None)
def select_rows(N, P):
    g = _gen(N, P, 3)
    return torch.randn(N, P, generator=g) * 0.1 + torch.randn(1, P, generator=g)


@functools.lru_cache(maxsize=None)
def special_columns(N):
    """[N, 12] columns: 0-2 heavy ties (three levels), 3-4 signed zeros, 5 +inf, 6 -inf, 7 both, 8-9 one NaN (first /
    last row), 10-11 two NaNs.  -> (U, NaNs per column)."""
    g = _gen(N, 5)
    U = torch.randn(N, 12, generator=g)
    U[:, 0:3] = torch.tensor([-1.5, 0.25, 2.0])[torch.randint(0, 3, (N, 3), generator=g)]
    U[:, 3] = torch.tensor([-0.0, 0.0])[torch.arange(N) % 2]
    U[:, 4] = torch.tensor([0.0, -0.0, 1.0])[torch.arange(N) % 3]
    U[0, 5] = INF
    U[N - 1, 6] = -INF
    U[1, 7], U[0, 7] = INF, -INF
    U[0, 8] = NAN
    U[N - 1, 9] = NAN
    U[0, 10], U[1, 10] = NAN, NAN
    U[N // 2, 11], U[N - 1, 11] = NAN, NAN
    return U, torch.isnan(U).sum(dim=0)


SELECT_SHAPES = [(n, 257) for n in (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)] + \
    [(n, p) for n in (8, 9) for p in (1, 255, 256)]


def trims(N):
    return sorted({0, 1, (N - 1) // 2} & set(range((N + 1) // 2)))


def test_torch_median_propagates_nan_and_sort_places_nan_last():
    x = torch.tensor([[3.0], [NAN], [1.0], [2.0], [0.5]])
    assert torch.isnan(torch.median(x, dim=0).values).all()
    assert torch.isnan(C.coord_median(x)).all()
    s = torch.sort(x, dim=0).values[:, 0]
    assert s[:4].tolist() == [0.5, 1.0, 2.0, 3.0] and math.isnan(float(s[4]))
    assert float(C.trimmed_mean(x, 1)[0]) == 2.0          # one NaN, trimmed away
    assert math.isnan(float(C.trimmed_mean(x, 0)[0]))      # more NaNs than trim


@pytest.mark.parametrize("N,P", [(1, 257), (2, 257), (8, 255), (9, 256), (33, 257), (64, 257)])
def test_select_references_match_composites(N, P):
    U = select_rows(N, P)
    assert torch.equal(ref_median(U), C.coord_median(U))
    for trim in trims(N):
        ref, bound = ref_trimmed(U, trim)
        # torch's fp32 mean sums in another order: the same first-order bound holds for any order
        assert within(C.trimmed_mean(U, trim), ref, bound), (N, trim)


@pytest.mark.parametrize("N", [3, 8, 11])
def test_select_references_match_composites_on_special_columns(N):
    U, nn = special_columns(N)
    assert same_values(ref_median(U), C.coord_median(U))
    assert bool((torch.isnan(ref_median(U)) == (nn > 0)).all())
    for trim in trims(N):
        ref, bound = ref_trimmed(U, trim)
        assert bool((torch.isnan(ref)[8:] == (nn > trim)[8:]).all())
        assert within(C.trimmed_mean(U, trim), ref, bound), (N, trim)


def ref_bulyan_column(vals, beta):
    """Bulyan's coordinate step on one column with NaN as torch.sort orders it (last, a NaN distance last too): NaN
    when beta exceeds the real values; the beta smallest when the median itself is NaN; otherwise the beta real
    values with the smallest key (|x - med| in fp32, x)."""
    real = sorted(v for v in vals if not math.isnan(v))
    theta, mid = len(vals), (len(vals) - 1) // 2
    if beta > len(real):
        return NAN
    if mid >= len(real):
        return sum(real[:beta]) / beta
    med = real[mid]
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    keyed = sorted(real, key=lambda x: (abs(f32(f32(x) - f32(med))), x))
    return sum(keyed[:beta]) / beta


@functools.lru_cache(maxsize=None)
def bulyan_nan_rows(theta):
    """[theta + 2, 6] rows; over the selected rows 0 .. theta - 1: column 0 no NaN, 1 one NaN, 2 two NaNs, 3 NaNs in
    half the rows (the median itself is NaN), 4 all but one NaN, 5 all NaN."""
    g = _gen(theta, 9)
    U = torch.randn(theta + 2, 6, generator=g)
    U[0, 1] = NAN
    U[1, 2], U[theta - 1, 2] = NAN, NAN
    U[:(theta + 2) // 2, 3] = NAN
    U[1:theta, 4] = NAN
    U[:theta, 5] = NAN
    return U


@pytest.mark.parametrize("theta", [5, 8, 11])
def test_bulyan_reference_matches_composite_on_nan(theta):
    U = bulyan_nan_rows(theta)
    sel = torch.arange(theta).flip(0)
    for beta in (1, 2, theta - 2, theta):
        got = C.bulyan_coord(U, sel, beta)
        for c in range(U.shape[1]):
            want = ref_bulyan_column(U[:theta, c].tolist(), beta)
            if math.isnan(want):
                assert math.isnan(float(got[c])), (theta, beta, c)
            else:
                assert float(got[c]) == pytest.approx(want, rel=1e-6, abs=1e-7), (theta, beta, c)


# ------------------------------------------------------------------------------------------ column statistics
@functools.lru_cache(maxsize=None)
def colstat_rows(K, P):
    """Benign columns; every third column has a large offset (mean 1e4, spread 1e-2), where an fp32 mean / std is
    itself inaccurate."""
    g = _gen(K, P, 11)
    G = torch.randn(K, P, generator=g) * 0.1 + torch.randn(1, P, generator=g)
    G[:, ::3] = 1e4 + 1e-2 * torch.randn(K, len(range(0, P, 3)), generator=g)
    return G


def ref_colstats(G):
    """fp64 two-pass mean and unbiased std (NaN for one row)."""
    Gd = G.double()
    K = Gd.shape[0]
    mean = Gd.sum(dim=0) / K
    ss = ((Gd - mean[None, :]) ** 2).sum(dim=0)
    std = (ss / (K - 1)).sqrt() if K > 1 else torch.full_like(mean, NAN)
    return mean, std


@pytest.mark.parametrize("K,P", [(1, 257), (2, 256), (3, 255), (64, 257), (100, 2)])
def test_colstats_reference_matches_composite_on_benign_columns(K, P):
    G = colstat_rows(K, P)
    mean, std = ref_colstats(G)
    cm, cs = C.column_mean_std(G)
    benign = torch.ones(P, dtype=torch.bool)
    benign[::3] = False
    # fp32 composite: a K-term fp32 sum, first-order bound (K - 1) 2^-24 sum|x| / K plus the rounding of the result
    mb = (K * 2.0 ** -24 * G.double().abs().sum(0)) / K + EPS32 * mean.abs()
    assert bool(((cm.double() - mean).abs() <= mb)[benign].all())
    if K == 1:
        assert torch.isnan(cs).all() and torch.isnan(std).all()
    else:
        assert torch.allclose(cs.double()[benign], std[benign], rtol=1e-4)
        assert torch.allclose(C.lie_candidate(G, 0.74).double()[benign], (mean + 0.74 * std)[benign], rtol=1e-4,
                              atol=1e-6)


# ------------------------------------------------------------------------------------------ weighted rows
@functools.lru_cache(maxsize=None)
def weighted_case(N, P):
    """(U, fp64 weights): zeros and a negative weight from three rows on; [1, -1] on nearly equal rows for two."""
    g = _gen(N, P, 13)
    U = torch.randn(N, P, generator=g)
    w = torch.rand(N, generator=g, dtype=torch.float64) + 0.1
    if N == 2:
        U[1] = U[0] + 1e-6 * torch.randn(P, generator=g)
        w = torch.tensor([1.0, -1.0], dtype=torch.float64)
    if N >= 3:
        w[1] = 0.0
        w[2] = -0.3
        w[N - 1] = 0.0
    return U, w


def ref_weighted(U, w):
    """(the fp64 sum rounded to fp32, bound 2^-23 |ref| + N 2^-52 sum_i |w_i u_i|)."""
    terms = w.double()[:, None] * U.double()
    ref = terms.sum(dim=0).float()
    return ref, EPS32 * ref.double().abs() + U.shape[0] * EPS64 * terms.abs().sum(dim=0)


@pytest.mark.parametrize("N,P", [(1, 1), (2, 257), (64, 255), (100, 256)])
def test_weighted_reference_matches_composite(N, P):
    U, w = weighted_case(N, P)
    ref, bound = ref_weighted(U, w)
    # composite.fedavg accumulates in fp64 too: sizes s give the weights s / sum s
    if bool((w > 0).all()):
        got = C.fedavg(U, w)
        r2, b2 = ref_weighted(U, w / w.sum())
        assert within(got, r2, b2)
    # composite.weighted_rows runs in fp32: N fp32 products and an N-term fp32 sum
    loose = bound + (N + 1) * 2.0 ** -24 * (w.double()[:, None] * U.double()).abs().sum(dim=0)
    assert within(C.weighted_rows(U, w), ref, loose)


# ------------------------------------------------------------------------------------------ row dots
@functools.lru_cache(maxsize=None)
def dots_case(N, P):
    g = _gen(N, P, 17)
    ref = torch.randn(P, generator=g)
    U = ref[None, :] + 0.1 * torch.randn(N, P, generator=g)
    if N >= 2:
        U[1] = 0.0  # an all-zero row: its cosine is 0 through the eps clamp
    return U.contiguous(), ref


def ref_dots(U, r):
    Ud, rd = U.double(), r.double()
    return torch.stack([(Ud * Ud).sum(1), (Ud * rd[None, :]).sum(1), (rd * rd).sum().expand(U.shape[0])], dim=1)


def ref_cosine(U, r, eps=1e-8):
    d = ref_dots(U, r)
    return d[:, 1] / torch.clamp(d[:, 0].sqrt() * d[:, 2].sqrt(), min=eps)


@pytest.mark.parametrize("N,P", [(1, 1), (3, 255), (3, 8193)])
def test_dots_reference_matches_composite(N, P):
    U, r = dots_case(N, P)
    assert torch.allclose(ref_cosine(U, r), C.cosine_to(U, r), rtol=1e-12, atol=1e-15)
    assert torch.allclose(ref_dots(U, r)[:, 0].sqrt(), C.row_norms(U), rtol=1e-12)
    zero = torch.zeros_like(r)
    assert ref_cosine(U, zero).tolist() == [0.0] * N == C.cosine_to(U, zero).tolist()


# ------------------------------------------------------------------------------------------ segment reductions
def edge_layout():
    """Slots of 1, 255, 256, 4095, 4096, 4097 and 8193 columns (around the 4096 tile), seven unused columns between
    the third and the fourth and five after the last.  -> (slots, P)"""
    slots, off = [], 0
    for i, n in enumerate((1, 255, 256, 4095, 4096, 4097, 8193)):
        if i == 3:
            off += 7
        slots.append(TensorSlot(f"s{i}", (n,), off, n))
        off += n
    return slots, off + 5


@functools.lru_cache(maxsize=None)
def segment_case(K, P):
    g = _gen(K, P, 19)
    G = torch.randn(K, P, generator=g) * 0.1 + torch.randn(1, P, generator=g)
    mean = G.mean(dim=0)
    dev = torch.rand(P, generator=g) * 0.01
    return G, mean, dev


def ref_segments(G, mean, dev, slots):
    """Per slot in fp64: A_k = sum (m - g_k)^2, B_k = sum (m - g_k) d, C = sum d^2; L2_k = sum over slots ||g_k||."""
    K, S = G.shape[0], len(slots)
    A = torch.zeros(K, S, dtype=torch.float64)
    B = torch.zeros(K, S, dtype=torch.float64)
    Cc = torch.zeros(S, dtype=torch.float64)
    L2 = torch.zeros(K, dtype=torch.float64)
    for i, s in enumerate(slots):
        sl = slice(s.offset, s.offset + s.numel)
        r = mean[sl].double()[None, :] - G[:, sl].double()
        d = dev[sl].double()
        A[:, i] = (r * r).sum(dim=1)
        B[:, i] = (r * d[None, :]).sum(dim=1)
        Cc[i] = (d * d).sum()
        L2 += (G[:, sl].double() ** 2).sum(dim=1).sqrt()
    return A, B, Cc, L2


@pytest.mark.parametrize("K", [1, 4])
def test_segment_reference_matches_composite(K):
    slots, P = edge_layout()
    G, mean, dev = segment_case(K, P)
    A, B, Cc, L2 = ref_segments(G, mean, dev, slots)
    Ar, Br, Cr = C.attack_coeffs_segments(G, mean, dev, slots)
    assert torch.allclose(A, Ar, rtol=1e-12) and torch.allclose(B, Br, rtol=1e-9, atol=1e-12)
    assert torch.allclose(Cc, Cr, rtol=1e-12)
    assert torch.allclose(L2, C.segment_l2_sum(G, slots), rtol=1e-12)


# ------------------------------------------------------------------------------------------ flat Adam
def ref_adam(p, g, m, v, step, lr, scale, b1=0.9, b2=0.999, eps=1e-8):
    """One fp64 Adam step (torch.optim.Adam's formula) on fp64 copies -> (p, m, v)."""
    g = g.double() * scale
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


@functools.lru_cache(maxsize=None)
def adam_case(n):
    g = _gen(n, 23)
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)
    if n > 1:
        gr[n // 2] = 0.0  # a zero gradient: v = 0, the denominator is eps
    return p, gr


ADAM_STEPS = (1, 2, 3, 4, 5, 1000)


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_adam_reference_matches_composite(n, scale):
    p0, gr = adam_case(n)
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    pd, md, vd = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in ADAM_STEPS:
        C.adam_step_scaled(p, gr, m, v, step, 1e-3, scale)
        pd, md, vd = ref_adam(pd, gr, md, vd, step, 1e-3, scale)
        assert torch.allclose(p.double(), pd, rtol=0, atol=1e-6)
    if n > 1:
        assert float(pd[n // 2]) == float(p0[n // 2])
