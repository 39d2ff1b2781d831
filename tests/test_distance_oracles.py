"""Oracles, case tables and error bounds for the attack-distance kernels (``csrc/kernels/linalg.hip``) and the ROC-AUC
kernels (``csrc/kernels/metrics.hip``); ``tests/test_gpu_distance_edges.py`` runs the kernels through them.

Everything here runs on the CPU.  The bound of a case is *truncation allowance + rounding allowance*, both derived from
the algorithm and the number formats (``docs/DISTANCE_TEST_BOUNDS.md``), never from a kernel's output:

- reference: ``torch.linalg.matrix_norm(., ord=2)`` in fp64; for the family the fp64-materialised rows X - γ·D;
- truncation: 12 squarings are 4096 power iterations.  With the eigen-decomposition (λ_i, u_i) of the Gram, column j of
  Gram^4096 has squared norm Σ_i λ_i^8192 u_i[j]² and Rayleigh quotient Σ_i λ_i^8193 u_i[j]² / Σ_i λ_i^8192 u_i[j]²
  (closed form, λ_1 = 1); the allowance is the largest 1 - sqrt(quotient_j) over the columns whose closed-form norm is
  at least half the largest.  The decomposition is the fp64 ``eigh`` of the fp32-rounded matrix's Gram, so the
  constructed spectra are seen as the kernels see them;
- rounding, direct path: ½·k·2⁻²⁴·(‖|X|‖₂/‖X‖₂)² for the sequential fp32 Gram, a second-order term for the fp32 image
  and the fp32 denormal floor of the Gram;
- rounding, Gram form: |ΔG| ≤ (k + 3)·2⁻⁵³·(|A| + |γ||S| + γ²|C|) entrywise, ‖ΔG‖₂ ≤ n·max|ΔG|,
  |σ̂ - σ| ≤ min(‖ΔG‖₂/σ, sqrt(‖ΔG‖₂)).

The fp32 emulations of the two algorithms show, on the CPU, that the algorithm alone stays inside every case's bound
with at least 2x headroom.
"""
import math
from types import SimpleNamespace as NS

import pytest
import torch

from attackfl_amd.ops import composite

U32, U64 = 2.0 ** -24, 2.0 ** -53
SQUARINGS = 12
POWER = 2 ** (SQUARINGS + 1)  # a column of Gram^4096 weighs eigenvector i by λ_i^4096; its squared norm by λ_i^8192
GRAM_NMAX, GRAM_LDS_FLOATS, DIRECT_NMAX = 64, 40 * 1024, 128
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------ paths
def small_side(r, c):
    return (r, c) if r <= c else (c, r)


def gram_form(r, c):
    """A slot the family evaluates in Gram form (k_spec_grams / k_spec_eval)."""
    n, k = small_side(r, c)
    return n <= GRAM_NMAX and 2 * n * (k + 1) <= GRAM_LDS_FLOATS


def path(r, c, family):
    """'gram' (fp64 Gram, family only), 'direct' (spectral_one, fp32 Gram) or 'lib' (the library's fp64 SVD)."""
    if family and gram_form(r, c):
        return "gram"
    return "direct" if min(r, c) <= DIRECT_NMAX else "lib"


# ------------------------------------------------------------------------------------------------ reference
def ref_norm(M):
    """fp64 spectral norms of [..., r, c] (any dtype; converted exactly)."""
    return torch.linalg.matrix_norm(M.double(), ord=2)


def rows_of(X, D, gamma):
    """fp64-materialised rows X - γ·D (X [M, r, c] fp32, D [r, c] fp32 or None)."""
    return X.double() if D is None or gamma is None else X.double() - float(gamma) * D.double()[None]


def _small(M):
    """[r, c] -> [n, k] with the smaller side first."""
    return M if M.shape[0] <= M.shape[1] else M.t()


def truncation(G, delta=0.0):
    """(smallest, largest) 1 - sqrt(Rayleigh quotient) of the candidate columns of G^4096, closed form, G fp64 PSD.
    ``delta``: a relative perturbation of the eigenvalue ratios λ_i/λ_1 that rounding can cause before the powers are
    taken (``ratio_shift``); the range then covers the ratios scaled by 1 - δ .. 1 + δ (the truncation is not monotone
    in the ratio, so the interval is sampled)."""
    lam, U = torch.linalg.eigh(G)
    l1 = lam[-1].item()
    if not l1 > 0.0:
        return 0.0, 0.0
    W = U * U  # W[j, i] = u_i[j]²
    lo, hi = INF, 0.0
    for f in ((0.0,) if delta == 0.0 else (-1.0, -0.5, 0.0, 0.5, 1.0)):
        lr = ((lam / l1) * (1.0 + f * delta)).clamp(0.0, 1.0)
        lr[-1] = 1.0
        p = lr ** POWER  # (underflow of the dominated powers is harmless)
        den, num = W @ p, W @ (p * lr)
        cand = den >= 0.5 * den.max()
        t = 1.0 - torch.sqrt(num[cand] / den[cand])
        lo, hi = min(lo, t.min().item()), max(hi, t.max().item())
    return max(lo, 0.0), max(hi, 0.0)


def ratio_shift(G, gram_rel, image_unit):
    """Relative shift of the eigenvalue ratios seen through the powers.  The Gram's own rounding moves each eigenvalue by
    at most ``gram_rel``·λ_1, a ratio by twice that.  The image after squaring t (eigenvalues ∝ λ^(2^t)) is rounded by at
    most ``image_unit``·trace, i.e. η_t = image_unit·Σ_i (λ_i/λ_1)^(2^t) relative to its top eigenvalue, a ratio by 2η_t,
    and 12 - t further squarings multiply that shift by 2^(12 - t): as a shift of the original ratios (divide by 4096)
    Σ_t 2^(1 - t)·η_t (t = 0: the fp32 image of the Gram itself)."""
    lam = torch.linalg.eigvalsh(G)
    l1 = lam[-1].item()
    if not l1 > 0.0:
        return 0.0
    lr = (lam / l1).clamp(0.0, 1.0)
    shift = 2.0 * gram_rel
    for t in range(SQUARINGS + 1):
        shift += 2.0 ** (1 - t) * image_unit * (lr ** (2 ** t)).sum().item()
    return shift


def _second_order(G, n):
    """Relative error in σ from the fp32 rounding of the image: the last squaring injects an error of at most
    (n + 2)·2⁻²⁴·trace(B) (|ΔB_ij| ≤ (n + 2)u·sqrt(B_ii B_jj) for a PSD image) into a column of norm at least
    ‖B‖₂/sqrt(n), earlier ones are squared away (factor 4/3 for the geometric tail): an angle θ, a quotient deficit of
    at most θ², half of that in σ.  trace(B)/‖B‖₂ = Σ_i (λ_i/λ_1)^4096."""
    lam = torch.linalg.eigvalsh(G)
    l1 = lam[-1].item()
    if not l1 > 0.0:
        return 0.0
    reff = ((lam / l1).clamp(0.0, 1.0) ** (POWER // 2)).sum().item()
    n8 = (n + 15) & ~15
    theta = (4.0 / 3.0) * math.sqrt(n8) * (n8 + 2) * U32 * max(reff, 1.0)
    return 0.5 * theta * theta


def bound_direct(M):
    """M [r, c] (the fp32 matrix the kernel reads) -> NS(ref, trunc, round, bound, lo_trunc), absolute values.
    round = ref·(½·k·2⁻²⁴·(‖|M|‖₂/‖M‖₂)² + second order) + the denormal floor ½·n·k·2⁻¹⁴⁹/ref."""
    Y = _small(M.double())
    n, k = Y.shape
    ref = ref_norm(Y).item()
    if not ref > 0.0:
        return NS(ref=0.0, trunc=0.0, lo_trunc=0.0, round=0.0, bound=0.0)
    G = Y @ Y.t()
    absn = ref_norm(Y.abs()).item()
    gram_rel = k * U32 * (absn / ref) ** 2
    n8 = (n + 7) & ~7
    tlo, thi = truncation(G, ratio_shift(G, gram_rel, (n8 + 2) * U32))
    rel = 0.5 * gram_rel + _second_order(G, n) + 4 * (n + 4) * U64
    rnd = rel * ref + 0.5 * n * k * 2.0 ** -149 / ref
    return NS(ref=ref, trunc=thi * ref, lo_trunc=tlo * ref, round=rnd, bound=thi * ref + rnd, nominal=truncation(G)[1])


def bound_gram(X, D, gamma):
    """X [r, c] fp32, D [r, c] fp32 or None, γ -> the same record for the Gram form."""
    Y = _small(X.double())
    n, k = Y.shape
    A = Y @ Y.t()
    mag = A.abs()
    G = A
    if D is not None and gamma is not None:
        E, g = _small(D.double()), float(gamma)
        S, C = Y @ E.t() + E @ Y.t(), E @ E.t()
        mag = mag + abs(g) * S.abs() + g * g * C.abs()
        R = Y - g * E
        G = R @ R.t()  # the Gram of the fp64-materialised rows: what the kernel's A - γS + γ²C approximates
        ref = ref_norm(R).item()
    else:
        ref = ref_norm(Y).item()
    dG = n * (k + 3) * U64 * mag.max().item()
    if not ref > 0.0:
        rnd = math.sqrt(dG)
        return NS(ref=0.0, trunc=0.0, lo_trunc=0.0, round=rnd, bound=rnd)
    tlo, thi = truncation(G, ratio_shift(G, dG / (ref * ref), 2 * U32))
    rnd = min(dG / ref, math.sqrt(dG)) + ref * (_second_order(G, n) + 4 * (n + 4) * U64)
    return NS(ref=ref, trunc=thi * ref, lo_trunc=tlo * ref, round=rnd, bound=thi * ref + rnd, nominal=truncation(G)[1])


def bound_lib(M):
    """The library path (n > 128): a backward-stable fp64 SVD, |σ̂ - σ| ≤ 8·max(r, c)·2⁻⁵³·σ."""
    ref = ref_norm(M).item()
    rnd = 8 * max(M.shape) * U64 * ref
    return NS(ref=ref, trunc=0.0, lo_trunc=0.0, round=rnd, bound=rnd)


def materialised(X, D, gamma):
    """The fp32 rows SpectralFamily hands the direct path for a slot outside the Gram form, and the spectral-norm
    distance of those rows from the fp64 ones (at most its Frobenius norm)."""
    if D is None or gamma is None:
        return X, 0.0
    rows = X - (float(gamma) * D.double()).float()[None]
    extra = torch.linalg.matrix_norm(rows.double() - rows_of(X, D, gamma), ord="fro", dim=(-2, -1))
    return rows, extra


def bound_of(X, D, gamma, family):
    """Bound records of every row of X [M, r, c] for the path the slot takes -> list of NS (ref is always the norm of the
    fp64-materialised row)."""
    r, c = X.shape[1:]
    p = path(r, c, family)
    if p == "gram":
        return [bound_gram(X[m], D, gamma) for m in range(X.shape[0])]
    rows, extra = materialised(X, D, gamma)
    out = []
    for m in range(X.shape[0]):
        b = bound_direct(rows[m]) if p == "direct" else bound_lib(rows[m])
        e = float(extra[m]) if torch.is_tensor(extra) else 0.0
        b.ref = ref_norm(rows_of(X[m:m + 1], D, gamma))[0].item()
        b.round += e
        b.bound += e
        out.append(b)
    return out


# ------------------------------------------------------------------------------------------------ fp32 emulations
def emulate_direct(M):
    """``spectral_one`` on the CPU: sequential fp32 Gram, power-of-two prescale, 12 normalised fp32 squarings, best
    column, fp64 Rayleigh quotient against the fp32 Gram."""
    Y = _small(M.float())
    n, k = Y.shape
    G = torch.zeros(n, n)
    for t in range(k):
        G.addr_(Y[:, t], Y[:, t])
    if not torch.isfinite(G).all():
        return NAN
    gm = G.abs().max().item()
    if gm == 0.0:
        return 0.0
    A = (G.double() * 2.0 ** (1 - math.frexp(gm)[1])).float()  # (exact: max|A| in [1, 2))
    for _ in range(SQUARINGS):
        B = A @ A
        A = B * (torch.tensor(1.0) / B.abs().max())
    col = int((A * A).sum(0).argmax())
    v = A[:, col].double()
    lam = (v @ (G.double() @ v) / (v @ v)).item()
    return math.sqrt(lam) if lam > 0 else 0.0


def emulate_gram(X, D=None, gamma=None):
    """``k_spec_grams`` + ``k_spec_eval`` on the CPU: fp64 Grams, G = (A - γS) + γ²C, fp32 image with fp64 products."""
    Y = _small(X.double())
    G = Y @ Y.t()
    if D is not None and gamma is not None:
        E, g = _small(D.double()), float(gamma)
        G = (G - g * (Y @ E.t() + E @ Y.t())) + (g * g) * (E @ E.t())
    if not torch.isfinite(G).all():
        return NAN
    mx = G.abs().max().item()
    if mx == 0.0:
        return 0.0
    F = (G * (1.0 / mx)).float()
    for _ in range(SQUARINGS):
        B = F.double() @ F.double()
        F = (B * (1.0 / B.abs().max().item())).float()
    col = int((F * F).sum(0).argmax())
    v = F[:, col].double()
    lam = (v @ (G @ v) / (v @ v)).item()
    return math.sqrt(lam) if lam > 0 else 0.0


# ------------------------------------------------------------------------------------------------ constructed spectra
def constructed(r, c, s, seed):
    """U diag(s) V^T in fp64 from seeded QR factors, rounded to fp32 -> [r, c]; s has min(r, c) entries."""
    n, k = small_side(r, c)
    g = torch.Generator().manual_seed(seed)
    U = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, generator=g))[0]
    V = torch.linalg.qr(torch.randn(k, n, dtype=torch.float64, generator=g))[0]
    Y = (U * torch.as_tensor(s, dtype=torch.float64)[None, :]) @ V.t()  # [n, k]
    return (Y if r <= c else Y.t()).contiguous().float()


def separated(n):
    """σ_1 = 2, every other singular value at most half of it."""
    return [2.0] + torch.linspace(1.0, 0.2, max(n - 1, 0), dtype=torch.float64).tolist()[:n - 1]


def gap_spectrum(n, j):
    return [2.0, 2.0 * (1.0 - 2.0 ** -j)] + torch.linspace(1.0, 0.2, n - 2, dtype=torch.float64).tolist()


def _case(name, kind, X, D=None, gammas=(None,), shape=None):
    """X [M, r, c] fp32; ``shape``: the slot's tensor shape where it is not [r, c] (a 3-D slot)."""
    return NS(name=name, kind=kind, X=X, D=D, gammas=tuple(gammas), shape=tuple(shape or X.shape[1:]))


def _stack(r, c, spec, seeds):
    return torch.stack([constructed(r, c, spec, s) for s in seeds])


SIZES = (1, 2, 7, 8, 9, 15, 16, 17, 31, 33, 48, 63, 64, 65, 127, 128, 129)
GAP_J = (4, 10, 12, 13, 14, 15, 16, 18, 22)
GAP_N = (16, 64, 128)
SCALE_E = (-25, -18, -12, -6, 0, 6, 12, 18, 25)  # (25: past the fp32 Gram on the large side)
SCALE_SHAPES = ((24, 40), (72, 80), (130, 131))  # Gram form / direct on every API / the library
CANCEL_RATIOS = (1e-2, 1e-4, 1e-6)
GAMMA0 = 7.25


def size_cases(n):
    """Padding and tiles: the long side k in {n, n + 1, 3n + 5}, both orientations, one square case; 2 rows."""
    out = [_case(f"size-{n}x{n}", "size", _stack(n, n, separated(n), (n, n + 1000)))]
    for k in (n + 1, 3 * n + 5):
        out.append(_case(f"size-{n}x{k}", "size", _stack(n, k, separated(n), (n + k, n + k + 1000))))
        out.append(_case(f"size-{k}x{n}", "size", _stack(k, n, separated(n), (n + 2 * k, n + 2 * k + 1000))))
    if n == 15:  # a 3-D slot: (16, 3, 5) is read as 16 x 15
        out.append(_case("size-16x3x5", "size", _stack(16, 15, separated(15), (5, 6)), shape=(16, 3, 5)))
    if n == 64:  # the LDS fit boundary of the Gram table, 2 n (k + 1) = 40960 floats exactly, and one over
        for k in (319, 320):
            out.append(_case(f"size-64x{k}", "size", _stack(64, k, separated(64), (k,))))
            out.append(_case(f"size-{k}x64", "size", _stack(k, 64, separated(64), (k + 1,))))
    return out


def gap_cases(n):
    out = [_case(f"gap-n{n}-j{j}", "gap", _stack(n, n + 1, gap_spectrum(n, j), (100 * n + j,))) for j in GAP_J]
    if n == 16:
        flat = [2.0] * 5 + torch.linspace(1.0, 0.2, 11, dtype=torch.float64).tolist()
        out.append(_case("gap-flat-top", "gap", _stack(16, 21, flat, (77,))))
        out.append(_case("gap-2I", "gap", (2.0 * torch.eye(16))[None].clone()))
    return out


def scale_cases(shape):
    r, c = shape
    Y = constructed(r, c, separated(min(r, c)), 31 * r + c).double()
    return [_case(f"scale-{r}x{c}-e{e}", "scale", (Y * 10.0 ** e).float()[None].clone()) for e in SCALE_E]


def range_cases(shape):
    """Dynamic range: rank one plus 1e-6 noise, a dominant row, a dominant column | zero, one entry, all equal."""
    r, c = shape
    g = torch.Generator().manual_seed(7 * r + c)
    a, b = torch.randn(r, 1, generator=g), torch.randn(1, c, generator=g)
    rank1 = a * b + 1e-6 * torch.randn(r, c, generator=g)
    row, col = torch.randn(r, c, generator=g), torch.randn(r, c, generator=g)
    row[r // 2] *= 1e4
    col[:, c - 1] *= 1e4
    one = torch.zeros(r, c)
    one[r - 1, 1] = -3.5
    return [_case(f"range-{r}x{c}-a", "range", torch.stack([rank1, row, col])),
            _case(f"range-{r}x{c}-b", "range", torch.stack([torch.zeros(r, c), one, torch.full((r, c), 0.37)]))]


RANGE_SHAPES = ((33, 50), (50, 33), (72, 75), (130, 131))  # Gram form twice, direct, the library


def cancel_cases(shape):
    """X_j = γ0·D + E with ‖E‖/‖X‖ = 1e-2, 1e-4, 1e-6 (one row each), at γ0, γ0(1 ± 2⁻²⁰), 0, -3 and 50."""
    r, c = shape
    g = torch.Generator().manual_seed(r + 3 * c)
    D = (torch.rand(r, c, generator=g, dtype=torch.float64) * 0.01 + 0.001).float()
    rows = []
    for ratio in CANCEL_RATIOS:
        E = torch.randn(r, c, generator=g, dtype=torch.float64)
        E *= ratio * GAMMA0 * ref_norm(D).item() / ref_norm(E).item()
        rows.append((GAMMA0 * D.double() + E).float())
    gam = (GAMMA0, GAMMA0 * (1 + 2.0 ** -20), GAMMA0 * (1 - 2.0 ** -20), 0.0, -3.0, 50.0)
    return [_case(f"cancel-{r}x{c}", "cancel", torch.stack(rows), D, gam)]


CANCEL_SHAPES = ((32, 48), (48, 32))


def family_cases():
    """The family with a deviation at the γs a bisection visits, on a separated spectrum: Gram form and a slot outside it."""
    out = []
    for r, c in ((9, 14), (40, 33), (70, 66)):
        g = torch.Generator().manual_seed(r * c)
        D = (torch.rand(r, c, generator=g) * 0.01)
        out.append(_case(f"family-{r}x{c}", "family", _stack(r, c, separated(min(r, c)), (r, c)) * 0.05, D,
                         (50.0, 25.0, 37.5, 0.0, -3.0)))
    return out


def all_cases():
    out = []
    for n in SIZES:
        out += size_cases(n)
    for n in GAP_N:
        out += gap_cases(n)
    for s in SCALE_SHAPES:
        out += scale_cases(s)
    for s in RANGE_SHAPES:
        out += range_cases(s)
    for s in CANCEL_SHAPES:
        out += cancel_cases(s)
    return out + family_cases()


def in_domain(case, p):
    """The stated scale contract: the direct path is relative where its fp32 Gram is representable."""
    if case.kind != "scale" or p != "direct":
        return "in"
    e = int(case.name.rsplit("-e", 1)[1])
    return "in" if -18 <= e <= 18 else ("below" if e < 0 else "above")


# ------------------------------------------------------------------------------------------------ packed layouts
def pack(cases, vector=None):
    """Cases with the same number of rows side by side in one [M, P] matrix -> (X [M, P], slots); ``vector``: the
    length of a 1-D slot put in the middle.  The first slot starts at offset 3 (nothing is aligned)."""
    from attackfl_amd.models import TensorSlot

    M = cases[0].X.shape[0]
    cols, slots, off = [torch.full((M, 3), 9.0)], [], 3
    for i, cs in enumerate(cases):
        if vector and i == len(cases) // 2:
            g = torch.Generator().manual_seed(vector)
            cols.append(torch.randn(M, vector, generator=g))
            slots.append(TensorSlot("vec", (vector,), off, vector))
            off += vector
        numel = cs.X[0].numel()
        cols.append(cs.X.reshape(M, numel))
        slots.append(TensorSlot(cs.name, cs.shape, off, numel))
        off += numel
    return torch.cat(cols, dim=1).contiguous(), slots


def slot_matrix(X, s):
    return X[:, s.offset:s.offset + s.numel].reshape(X.shape[0], s.shape[0], -1)


def ragged_cases():
    """n = 1, 9, 64, 65, 128 and 129 in one launch (LDS is sized by the largest n, each workgroup uses its own)."""
    shapes = ((1, 6), (9, 20), (64, 70), (90, 65), (128, 130), (129, 131))
    return [_case(f"ragged-{r}x{c}", "ragged", _stack(r, c, separated(min(r, c)), (r, c, r + c))) for r, c in shapes]


def poison_cases():
    shapes = ((9, 12), (70, 64), (65, 80), (129, 130))  # Gram form twice, direct, the library
    return [_case(f"poison-{r}x{c}", "poison", _stack(r, c, separated(min(r, c)), (r, c + 1, r + c))) for r, c in shapes]


POISONS = ("nan", "inf", "nanrow")


def poison(X, slot, row, kind):
    """A copy of X [M, P] with one NaN entry, one +Inf entry or a whole NaN matrix row in (row, slot)."""
    X = X.clone()
    m = X[row, slot.offset:slot.offset + slot.numel].view(slot.shape[0], -1)
    if kind == "nan":
        m[m.shape[0] - 1, m.shape[1] // 2] = NAN
    elif kind == "inf":
        m[0, m.shape[1] - 1] = INF
    else:
        m[m.shape[0] // 2, :] = NAN
    return X


# ------------------------------------------------------------------------------------------------ checking
def check(got, recs, label, one_sided=False, worst=None):
    """|got - ref| ≤ bound for every record (one-sided: also got ≤ ref + round, a Rayleigh quotient cannot exceed the
    top eigenvalue); returns and records the worst err / bound."""
    w = 0.0
    for i, (g, b) in enumerate(zip(got, recs)):
        g = float(g)
        err = abs(g - b.ref)
        assert math.isfinite(g) and err <= b.bound, f"{label}[{i}]: got {g!r} ref {b.ref!r} err {err:.3e} bound {b.bound:.3e}"
        if one_sided:
            assert g <= b.ref + b.round, f"{label}[{i}]: {g!r} exceeds ref {b.ref!r} by more than rounding {b.round:.3e}"
        w = max(w, err / b.bound if b.bound > 0 else 0.0)
    if worst is not None:
        worst[0] = max(worst[0], w)
    return w


# ------------------------------------------------------------------------------------------------ bisection oracle
def bisect_ref(vA, vB, vC, spec, thr, kind, n_iter, gamma0):
    """The fused bisection's decisions in fp64 on the host.  vA, vB [K, Sv] and vC [Sv] (or None), ``spec(γ)`` -> the
    [K - 1, S] spectral distances at γ (or None), kind 0: max_j d_j < thr, 1: Σ_j d_j² < thr; row 0 is the candidate
    itself (distance 0); a NaN distance rejects.  -> (tried, accepted, last accepted γ, last tried γ)."""
    g, step, succ, last = float(gamma0), float(gamma0), 0.0, float(gamma0)
    tried, accs = [], []
    for _ in range(n_iter):
        K = vA.shape[0] if vA is not None else spec(g).shape[0] + 1
        d = torch.zeros(K, dtype=torch.float64)
        if vA is not None:
            for v in range(vA.shape[1]):
                q = (vA[:, v] - 2.0 * g * vB[:, v]) + g * g * vC[v]
                d = d + torch.sqrt(q.clamp_min(0.0))  # (clamp_min keeps a NaN, as in the generic torch loop)
        if spec is not None:
            sp = spec(g)
            for s in range(sp.shape[1]):
                d[1:] = d[1:] + sp[:, s]
        d[0] = 0.0
        bad = bool(torch.isnan(d).any())
        acc = (not bad) and (float((d * d).sum()) < thr if kind == 1 else float(d.max()) < thr)
        tried.append(g)
        accs.append(acc)
        last = g
        if acc:
            succ = g
        g = g + step / 2.0 if acc else g - step / 2.0
        step *= 0.5
    return tried, accs, succ, last


# ------------------------------------------------------------------------------------------------ ROC-AUC oracle
def auc_two_u(s, y):
    """2U = 2·#(s_neg < s_pos) + #(s_neg == s_pos) over (positive, negative) pairs, exact integers, and (P, N).
    O(n²) pair counts for n ≤ 4096, the tie-corrected rank sum (fp64 scores, int64 sums) above."""
    s, pos = s.reshape(-1).double(), y.reshape(-1) > 0.5
    P, N = int(pos.sum()), int((~pos).sum())
    if s.numel() <= 4096:
        sp, sn = s[pos][:, None], s[~pos][None, :]
        return int(2 * (sn < sp).sum() + (sn == sp).sum()), P, N
    srt = torch.sort(s).values
    lo = torch.searchsorted(srt, s[pos], right=False)
    hi = torch.searchsorted(srt, s[pos], right=True)
    return int((lo + 1 + hi).sum()) - P * (P + 1), P, N


def auc_ref(s, y):
    two_u, P, N = auc_two_u(s, y)
    return two_u / (2.0 * P * N) if P > 0 and N > 0 else NAN


AUC_LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 32768, 32769, 32770)


def auc_data(n, seed=0):
    """Scores with many ties, about 30 % positives, both classes present from n = 2 on."""
    g = torch.Generator().manual_seed(1000 + n + seed)
    y = (torch.rand(n, generator=g) < 0.3).float()
    if n >= 2:
        y[0], y[n - 1] = 1.0, 0.0
    s = ((torch.rand(n, generator=g) + 0.3 * y) * 50).round() / 50
    return s, y


def auc_value_cases(n=300):
    """name -> (scores, labels, expected AUC or None for 'the oracle's'), n samples."""
    g = torch.Generator().manual_seed(9)
    y = (torch.rand(n, generator=g) < 0.4).float()
    y[:2] = torch.tensor([1.0, 0.0])
    r = torch.rand(n, generator=g)
    den = torch.tensor([1e-45, 3e-45, 1e-41, 1e-39, 0.0, -1e-45, -1e-40])[torch.randint(0, 7, (n,), generator=g)]
    pm = torch.where(r < 0.3, torch.tensor(-INF), torch.where(r > 0.7, torch.tensor(INF), r))
    single = torch.zeros(n)
    single[n // 2] = 1.0
    return {
        "tied": (torch.full((n,), 0.25), y, 0.5),
        "two-values": ((r < 0.5).float() * 0.5 - 1.0, y, None),
        "inf": (pm, y, None),
        "signed-zero": (torch.where(r < 0.5, torch.tensor(-0.0), torch.tensor(0.0)), y, 0.5),
        "signed-zero-mixed": (torch.where(r < 0.3, torch.tensor(-0.0), torch.where(r < 0.6, torch.tensor(0.0), r - 0.8)), y, None),
        "denormals": (den, y, None),
        "single-positive": (r, single, None),
        "single-negative": (r, 1.0 - single, None),
        "one-class-pos": (r, torch.ones(n), NAN),
        "one-class-neg": (r, torch.zeros(n), NAN),
        "labels-0.49-0.51": (r, torch.where(y > 0.5, torch.tensor(0.51), torch.tensor(0.49)), None),
    }


# ================================================================================================ CPU checks
def _emulate(case, p, m, gamma):
    if p == "gram":
        return emulate_gram(case.X[m], case.D, gamma)
    return emulate_direct(materialised(case.X, case.D, gamma)[0][m])


def evaluations(case):
    """(family, γ) pairs of a case: the direct API on X itself, and the family at every γ of the case (γ = None where
    the slot is outside the Gram form is the direct API's computation again)."""
    out = [(False, None)]
    for gamma in case.gammas:
        if gamma is not None or path(*case.X.shape[1:], True) == "gram":
            out.append((True, gamma))
    return out


def _sweep(cases):
    """Emulated err / bound over cases and the paths each slot can take -> worst ratio; asserts
    err ≤ truncation + ½·rounding."""
    worst = 0.0
    for cs in cases:
        r, c = cs.X.shape[1:]
        for family, gamma in evaluations(cs):
            p = path(r, c, family)
            if p == "lib":
                continue
            for m, b in enumerate(bound_of(cs.X, cs.D, gamma, family)):
                dom = in_domain(cs, p)
                got = _emulate(cs, p, m, gamma)
                if dom == "below":
                    assert got == 0.0 or abs(got - b.ref) <= b.bound, (cs.name, got)
                    continue
                if dom == "above":
                    assert not math.isfinite(got), (cs.name, got)
                    continue
                err = abs(got - b.ref)
                # (the truncation is the algorithm's own, documented error: the headroom is asked of the rounding part)
                assert err <= b.trunc + 0.5 * b.round, f"{cs.name} {p} γ={gamma} row {m}: emulated err {err:.3e}, {b}"
                if cs.kind == "gap":
                    assert got <= b.ref + b.round, (cs.name, p, got, b.ref)
                worst = max(worst, err / b.bound if b.bound > 0 else 0.0)
    return worst


@pytest.mark.parametrize("kind", ["size", "gap", "scale", "range", "cancel", "family", "ragged", "poison"])
def test_emulated_algorithm_stays_inside_half_the_bound(kind):
    cases = [c for c in all_cases() + ragged_cases() + poison_cases() if c.kind == kind]
    assert cases
    w = _sweep(cases)
    print(f"emulated worst err/bound, {kind}: {w:.3f} over {len(cases)} cases")


def test_truncation_is_negligible_outside_the_gap_class():
    for cs in all_cases():
        if cs.kind == "gap":
            continue
        for gamma in cs.gammas:
            R = rows_of(cs.X, cs.D, gamma)
            for m in range(R.shape[0]):
                Y = _small(R[m])
                assert truncation(Y @ Y.t())[1] < 1e-12, (cs.name, gamma, m)


@pytest.mark.parametrize("n", GAP_N)
def test_closed_form_truncation_reproduces_the_emulation_on_the_gap_sweep(n):
    """(ref - emulated) lies in [lowest, highest candidate-column truncation] up to the rounding allowance; at j = 15
    the truncation alone is above the 2e-5 the random-matrix tests use."""
    seen = {}
    for cs in gap_cases(n):
        for emu, bnd in ((emulate_direct, bound_direct), (emulate_gram, lambda M: bound_gram(M, None, None))):
            b = bnd(cs.X[0])
            miss = b.ref - emu(cs.X[0])
            assert b.lo_trunc - b.round <= miss <= b.trunc + b.round, (cs.name, miss, b)
            seen[cs.name] = b.nominal
    for j in (4, 10):
        assert seen[f"gap-n{n}-j{j}"] < 1e-10
    assert 1e-5 < seen[f"gap-n{n}-j15"] < 4e-5  # (above the 2e-5 of the random-matrix tests at n = 16 and 64)
    assert seen[f"gap-n{n}-j22"] < 3e-7
    print(f"truncation (relative) n={n}: " + " ".join(f"j{j}={seen[f'gap-n{n}-j{j}']:.2e}" for j in GAP_J))


def test_constructed_spectra_are_what_they_claim():
    X = constructed(16, 21, gap_spectrum(16, 10), 3)
    s = torch.linalg.svdvals(X.double())
    assert torch.allclose(s, torch.tensor(gap_spectrum(16, 10), dtype=torch.float64), rtol=0, atol=1e-6)
    assert constructed(21, 16, separated(16), 3).shape == (21, 16)
    assert abs(ref_norm(constructed(129, 130, separated(129), 1)).item() - 2.0) < 1e-6


def test_path_table():
    assert path(64, 319, True) == "gram" and 2 * 64 * 320 == GRAM_LDS_FLOATS
    assert path(64, 320, True) == "direct" and path(320, 64, True) == "direct"
    assert path(65, 66, True) == "direct" and path(64, 64, True) == "gram" and path(64, 64, False) == "direct"
    assert path(128, 500, True) == "direct" and path(129, 130, True) == "lib" and path(129, 130, False) == "lib"
    from attackfl_amd import ops
    from attackfl_amd.models import TensorSlot

    slots = [TensorSlot("a", (64, 319), 0, 64 * 319), TensorSlot("b", (320, 64), 64 * 319, 64 * 320),
             TensorSlot("c", (16, 3, 5), 64 * 639, 240), TensorSlot("d", (129, 130), 64 * 639 + 240, 129 * 130)]
    tab, sumq, lds, rest = ops._gram_table(slots, "cpu")
    assert tab[:, 0].tolist() == [0, 64 * 639] and [s.name for s in rest] == ["b", "d"] and lds == GRAM_LDS_FLOATS
    tab, max_n, scr, big = ops._spectral_table(slots, "cpu")
    assert tab.shape[0] == 3 and max_n == 64 and [s.name for s in big] == ["d"]


def test_composite_returns_nan_for_exactly_the_non_finite_matrices():
    """The CPU composite (LAPACK raises on such input) gives NaN for the poisoned matrix, the SVD value for the rest,
    and the CPU bisection's comparison then rejects."""
    X, slots = pack(poison_cases(), vector=7)
    clean = [composite.batched_spectral_norm(slot_matrix(X, s)) for s in slots]
    for kind in POISONS:
        for si, s in enumerate(slots):
            if s.name == "vec":
                continue
            Xp = poison(X, s, 1, kind)
            for sj, t in enumerate(slots):
                got = composite.batched_spectral_norm(slot_matrix(Xp, t))
                for m in range(X.shape[0]):
                    if (m, sj) == (1, si):
                        assert math.isnan(got[m].item())
                    else:
                        assert got[m].item() == clean[sj][m].item()
    z = composite.batched_spectral_norm(torch.zeros(2, 5, 4))
    assert z.tolist() == [0.0, 0.0] and z.dtype == torch.float64
    d = torch.tensor([0.0, NAN, 1.0], dtype=torch.float64)
    assert not bool(d.max() < 5.0) and not bool((d * d).sum() < 5.0)  # (torch.max keeps the NaN: NaN < thr is False)


def test_bisect_oracle_strictness_and_clamp():
    vA = torch.tensor([[999.0], [25.0], [9.0]], dtype=torch.float64)
    vB = torch.tensor([[5.0], [2.0], [0.0]], dtype=torch.float64)
    vC = torch.tensor([1.0], dtype=torch.float64)
    # γ = 4: row 1 25 - 16 + 16 = 25, row 2 9 + 16 = 25 -> max 5, Σ d² = 50
    assert bisect_ref(vA, vB, vC, None, 5.0, 0, 1, 4.0)[1] == [False]
    assert bisect_ref(vA, vB, vC, None, math.nextafter(5.0, INF), 0, 1, 4.0)[1] == [True]
    assert bisect_ref(vA, vB, vC, None, 50.0, 1, 1, 4.0)[1] == [False]
    assert bisect_ref(vA, vB, vC, None, math.nextafter(50.0, INF), 1, 1, 4.0)[1] == [True]
    tried, acc, succ, last = bisect_ref(vA, vB, vC, None, 5.5, 0, 3, 4.0)
    assert tried == [4.0, 6.0, 5.0] and last == 5.0 and acc[0] and succ == (5.0 if acc[2] else 4.0)
    neg = torch.tensor([[0.0], [1.0]], dtype=torch.float64)
    assert bisect_ref(neg, torch.tensor([[0.0], [2.0]], dtype=torch.float64), torch.zeros(1, dtype=torch.float64), None,
                      1e-300, 0, 1, 4.0)[1] == [True]  # 1 - 16 < 0 is clamped to 0


def test_auc_oracles_agree_with_each_other_and_with_sklearn_conventions():
    for n in (2, 3, 65, 1025):
        s, y = auc_data(n)
        two_u, P, N = auc_two_u(s, y)
        srt = torch.sort(s.double()).values
        pos = y > 0.5
        rank = int((torch.searchsorted(srt, s.double()[pos]) + 1 + torch.searchsorted(srt, s.double()[pos], right=True)).sum())
        assert two_u == rank - P * (P + 1) and P + N == n
    s, y = auc_data(4096)
    s2, y2 = torch.cat([s, s[:1]]), torch.cat([y, 1 - y[:1]])
    a, b = auc_two_u(s, y), auc_two_u(s2, y2)  # pair counts vs rank sums on nearly the same data
    assert b[0] - a[0] == int(2 * (s[y > 0.5] > s[0]).sum() + (s[y > 0.5] == s[0]).sum())
    assert auc_ref(torch.tensor([0.2, 0.2, 0.7]), torch.tensor([1.0, 0.0, 1.0])) == 0.75
    for name, (sc, lab, want) in auc_value_cases().items():
        got = auc_ref(sc, lab)
        if want is not None:
            assert (math.isnan(got) and math.isnan(want)) or got == want, name
        else:
            assert 0.0 <= got <= 1.0, name
