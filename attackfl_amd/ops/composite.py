"""Plain-PyTorch composites of every native op.

These are the CPU implementations *and* the numerical oracles that the HIP kernels in
``csrc/kernels`` are tested against (fp32/fp64 PyTorch references of the same op).
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch


# ---------------------------------------------------------------- loss
class _BCE(torch.autograd.Function):
    """``nn.BCELoss`` (mean) forward AND backward, minus the [0, 1] input-range check.

    Forward: ``-(y·max(log p, -100) + (1-y)·max(log1p(-p), -100))``, mean.  Backward: torch's
    ``(p - y) / max(p (1 - p), 1e-12)`` per element over N — finite where the sigmoid saturates to exactly
    0 or 1 in fp32.  Autograd through the clamped logs instead gives ``0 · inf = NaN`` there (the derivative
    of the clamped branch is 0, of the log ∓inf), a NaN gradient the reference (``client.py:76`` BCELoss)
    never produces: after an Opt-Fang round that turned a healthy reference client into a NaN-loss failure.
    A NaN input still yields a NaN loss (the NaN abort test, ``client.py:100-102``)."""

    @staticmethod
    def forward(ctx, p, y):
        ctx.save_for_backward(p, y)
        lv = -(y * torch.clamp(torch.log(p), min=-100.0) + (1 - y) * torch.clamp(torch.log1p(-p), min=-100.0))
        return lv.mean()

    @staticmethod
    def backward(ctx, g):
        p, y = ctx.saved_tensors
        gp = g * (p - y) / torch.clamp((1 - p) * p, min=1e-12) / p.numel()
        return gp, None


def bce_loss(p: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Mean BCE of probabilities ``p`` against targets ``y`` with ``nn.BCELoss``'s gradient (``_BCE``)."""
    return _BCE.apply(p, y.to(p.dtype).expand_as(p))


# ---------------------------------------------------------------- column statistics / attacks
def column_mean_std(G: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    mean = G.mean(dim=0)
    std = G.std(dim=0) if G.shape[0] > 1 else torch.full_like(mean, float("nan"))
    return mean, std


def lie_candidate(G: torch.Tensor, z: float) -> torch.Tensor:
    mean, std = column_mean_std(G)
    return mean + z * std


def pairwise_l2(G: torch.Tensor) -> torch.Tensor:
    Gd = G.double()
    sq = (Gd * Gd).sum(dim=1)
    gram = Gd @ Gd.t()
    d2 = (sq[:, None] + sq[None, :] - 2.0 * gram).clamp_min(0.0)
    d2.fill_diagonal_(0.0)
    return d2.sqrt()


def gram(G: torch.Tensor) -> torch.Tensor:
    Gd = G.double()
    return Gd @ Gd.t()


def segment_l2_sum(diffs: torch.Tensor, slots) -> torch.Tensor:
    out = torch.zeros(diffs.shape[0], dtype=torch.float64, device=diffs.device)
    for s in slots:
        seg = diffs[:, s.offset:s.offset + s.numel].double()
        out += torch.linalg.vector_norm(seg, dim=1)
    return out


def batched_spectral_norm(mats: torch.Tensor) -> torch.Tensor:
    """[..., r, c] -> [...] fp64 ord-2 norms; NaN for exactly the matrices that hold a non-finite entry (LAPACK
    refuses those), so a poisoned model is at distance NaN, which every bisection comparison rejects."""
    m = mats.double()
    bad = ~torch.isfinite(m).flatten(-2).all(dim=-1)
    val = torch.linalg.matrix_norm(m.masked_fill(bad[..., None, None], 0.0), ord=2).to(torch.float64)
    return val.masked_fill(bad, float("nan"))


def attack_coeffs(G: torch.Tensor, mean: torch.Tensor, dev: torch.Tensor):
    Gd, md, dd = G.double(), mean.double(), dev.double()
    r = md[None, :] - Gd
    A = (r * r).sum(dim=1)
    B = (r * dd[None, :]).sum(dim=1)
    C = (dd * dd).sum()
    return A, B, C


def attack_coeffs_segments(G: torch.Tensor, mean: torch.Tensor, dev: torch.Tensor, slots):
    K = G.shape[0]
    S = len(slots)
    A = torch.zeros(K, S, dtype=torch.float64, device=G.device)
    B = torch.zeros(K, S, dtype=torch.float64, device=G.device)
    C = torch.zeros(S, dtype=torch.float64, device=G.device)
    for i, s in enumerate(slots):
        sl = slice(s.offset, s.offset + s.numel)
        a, b, c = attack_coeffs(G[:, sl], mean[sl], dev[sl])
        A[:, i], B[:, i], C[i] = a, b, c
    return A, B, C


# ---------------------------------------------------------------- aggregation
def weighted_rows(U: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """sum_i w_i U_i  (w already normalised by the caller)."""
    return (w.to(U.dtype)[:, None] * U).sum(dim=0)


def fedavg(U: torch.Tensor, sizes: torch.Tensor) -> torch.Tensor:
    s = sizes.to(torch.float64)
    return ((s[:, None] * U.double()).sum(dim=0) / s.sum()).to(U.dtype)


def coord_median(U: torch.Tensor) -> torch.Tensor:
    return torch.median(U, dim=0).values


def trimmed_mean(U: torch.Tensor, trim_k: int) -> torch.Tensor:
    n = U.shape[0]
    s, _ = torch.sort(U, dim=0)
    return s[trim_k:n - trim_k].mean(dim=0)


def krum_select(D: torch.Tensor, f: int, rounds: int, iterated: bool):
    """Krum's selection on the squared-distance matrix ``D [n, n]`` (``agg.hip`` ``k_krum_select``): score(i) on an
    active set of m rows = the k = max(m - f - 2, 1) smallest D[i][j] over the active j != i, summed in ascending
    order (0 for m = 1); a pick is the active row with the smallest (score, index).  ``iterated`` False: scored once,
    ``rounds`` picks by that ranking (Multi-Krum); True: re-scored on the rows still active before every pick
    (Bulyan).  -> (sel [rounds] int64 in selection order, mask [n] bool, first-pass scores [n] fp64).  Tensor ops
    only (no host read), so it also serves device tensors beyond the kernel's 64 rows."""
    n = D.shape[0]
    # D is read as symmetric, the upper triangle standing for both halves: at k = 1 (Bulyan's last picks) two rows that
    # are each other's nearest neighbour tie exactly, which a D[i][j] != D[j][i] in the last bit would decide
    D = torch.triu(D.double(), 1)
    D = D + D.t()
    inf = float("inf")
    idx = torch.arange(n, device=D.device)
    eye = idx[:, None] == idx[None, :]
    active = torch.ones(n, dtype=torch.bool, device=D.device)
    sel, first, sc = [], None, None
    for t in range(rounds):
        if t == 0 or iterated:
            m = n - t if iterated else n
            k = max(m - f - 2, 1)
            if m == 1:
                sc = torch.zeros(n, dtype=torch.float64, device=D.device)
            else:
                W = D.masked_fill(eye | ~active[None, :], inf)
                sc = torch.cumsum(torch.sort(W, dim=1).values, dim=1)[:, k - 1]
            if t == 0:
                first = sc
        i = torch.argmin(torch.where(active, sc, torch.full_like(sc, inf)))  # (ties: the first, lowest index)
        sel.append(i)
        active = active & (idx != i)
    return torch.stack(sel), ~active, first


# ---------------------------------------------------------------- pre-aggregation (docs/PARITY.md)
def mix_rows(W: torch.Tensor, U: torch.Tensor) -> torch.Tensor:
    """Y = W U for a small dense W [R, n] (fp64) and rows U [n, P] (``agg.hip`` ``k_mix_rows``): an fp64 sum in
    ascending j over every j, zero weights included (a non-finite row poisons every mixed row), rounded to fp32 once.
    Tensor ops only, so it also serves device tensors beyond the kernel's 64 rows."""
    W = W.to(device=U.device, dtype=torch.float64)
    acc = torch.zeros(W.shape[0], U.shape[1], dtype=torch.float64, device=U.device)
    for j in range(U.shape[0]):
        acc += W[:, j, None] * U[j].double()[None, :]
    return acc.to(torch.float32)


def nnm_weights(D: torch.Tensor, f: int):
    """Nearest-neighbour mixing's W [n, n] fp64 from the squared distances ``D [n, n]`` (``agg.hip`` ``k_nnm_weights``):
    D read as symmetric from its upper triangle, a NaN entry as +inf; row i mixes itself and the first n - f - 1 other
    rows by (D_ij, j) ascending with weight 1 / (n - f) each.  -> (W, the neighbour sets [n] as int64 bit masks).
    Tensor ops only (no host read)."""
    n = D.shape[0]
    D = torch.triu(D.double(), 1)
    D = D + D.t()
    key = torch.where(torch.isnan(D), torch.full_like(D, float("inf")), D)
    order = torch.sort(key, dim=1, stable=True).indices
    idx = torch.arange(n, device=D.device)
    other = order != idx[:, None]
    take = other & (torch.cumsum(other, dim=1) <= n - f - 1)
    member = torch.zeros(n, n, dtype=torch.bool, device=D.device).scatter_(1, order, take) | (idx[:, None] == idx[None, :])
    W = member.double() * (1.0 / (n - f))
    return W, (member.long() << idx[None, :]).sum(dim=1)


def bucket_permutation(seed: int, n: int) -> torch.Tensor:
    """Bucketing's shuffle: the row indices sorted by (u_i, i), u = ``afl_uniform(seed, n)`` (host, int64)."""
    return torch.sort(afl_uniform(seed, n), stable=True).indices


def bucket_weights(sizes: Optional[torch.Tensor], n: int, s: int, seed: int):
    """Bucketing's W [R, n] fp64, R = ceil(n / s): bucket r = pi[r s : (r + 1) s] of ``bucket_permutation``,
    W_rj = sizes_j / (the bucket's size sum) for j in bucket r (uniform when ``sizes`` is None).  -> (W, the buckets'
    size sums [R] fp64), both where ``sizes`` lives (the host when None): pi depends on (seed, n) only and goes up
    pinned; no device value is read back."""
    from .layers import upload

    pi = bucket_permutation(seed, n)
    R = -(-n // s)
    bucket = torch.empty(n, dtype=torch.int64)
    bucket[pi] = torch.arange(n, dtype=torch.int64) // s
    a = torch.ones(n, dtype=torch.float64) if sizes is None else sizes.to(torch.float64)
    member = upload(bucket[None, :] == torch.arange(R, dtype=torch.int64)[:, None], a.device)
    M = member.double() * a[None, :]
    tot = M.sum(dim=1)
    return M / tot[:, None], tot


AGR_TARGETS = ("krum", "mkrum", "bulyan")  # (the kernel's target 0 / 1 / 2)


def agr_admissible(n: int, f: int, target: str) -> bool:
    """Whether the rule ``target`` runs on n rows with f assumed Byzantine ones: n >= 2 f + 3 (Krum, Multi-Krum),
    n >= 4 f + 3 (Bulyan)."""
    return f >= 0 and n >= (4 * f + 3 if target == "bulyan" else 2 * f + 3)


def agr_rounds(n: int, f: int, target: str):
    """(rounds, iterated) of ``krum_select`` for the rule: Krum 1 pick, Multi-Krum n - f picks of one ranking, Bulyan
    n - 2 f picks re-scored every time."""
    return {"krum": (1, False), "mkrum": (n - f, False), "bulyan": (n - 2 * f, True)}[target]


def agr_matrix(Dg: torch.Tensor, A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, gamma, m: int) -> torch.Tensor:
    """The modelled system's squared distances [K + m, K + m] fp64: the K genuine rows first (``Dg``, read as
    symmetric from its upper triangle), then m identical copies of c(γ) = mean - γ·dev at squared distance
    max(A_j - 2γB_j + γ²C, 0) from genuine row j (``attack_coeffs``) and 0 from each other."""
    K = Dg.shape[0]
    Dg = torch.triu(Dg.double(), 1)
    d = (A.double() - 2.0 * gamma * B.double() + gamma * gamma * C.double()).clamp_min(0.0)
    D = torch.zeros(K + m, K + m, dtype=torch.float64, device=Dg.device)
    D[:K, :K] = Dg + Dg.t()
    D[:K, K:] = d[:, None]
    D[K:, :K] = d[None, :]
    return D


def agr_oracle(Dg: torch.Tensor, A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, gamma, m: int, f: int,
               target: str) -> torch.Tensor:
    """Would the rule still select the attacker's rows at this γ (``agg.hip`` ``k_agr_bisect``)?  ``krum_select`` on
    ``agr_matrix`` with ``agr_rounds``: Krum accepts when the pick is a copy (index >= K), Multi-Krum and Bulyan when
    all m copies are selected; a NaN in A, B or C rejects.  The copies hold the last indices, so every index tie goes
    against the attacker.  -> 0-d bool tensor; tensor ops only (no host read)."""
    K = Dg.shape[0]
    rounds, iterated = agr_rounds(K + m, f, target)
    sel, mask, _ = krum_select(agr_matrix(Dg, A, B, C, gamma, m), f, rounds, iterated)
    acc = (sel[0] >= K) if target == "krum" else mask[K:].all()
    nan = torch.isnan(A).any() | torch.isnan(B).any() | torch.isnan(C).any()
    return acc & ~nan


def agr_oracle_margin(Dg: torch.Tensor, A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, gamma, m: int, f: int,
                      target: str):
    """``agr_oracle``'s diagnostic twin (host reads; for tests and studies) -> (accept bool, decision margin float).
    The same picks, written out, with at every pick gap = |score(picked) - the smallest score among the other active
    rows| / the largest finite first-pass score; when the picked row is a copy the other copies (whose scores are the
    same bits) are left out of the others.  The margin is the smallest non-zero gap over the picks (inf when there is
    none): perturbations of the scores below it cannot change a pick.  A zero gap is an exact tie (identical copies,
    or the k = 1 mutual-nearest tie ``krum_select`` documents) that the index decides the same way on every side."""
    K = Dg.shape[0]
    n = K + m
    rounds, iterated = agr_rounds(n, f, target)
    D = agr_matrix(Dg, A, B, C, gamma, m).cpu()
    inf = float("inf")
    idx = torch.arange(n)
    eye = idx[:, None] == idx[None, :]
    active = torch.ones(n, dtype=torch.bool)
    sel, sc, scale, margin = [], None, 1.0, inf
    for t in range(rounds):
        if t == 0 or iterated:
            k = max((n - t if iterated else n) - f - 2, 1)
            if iterated and n - t == 1:
                sc = torch.zeros(n, dtype=torch.float64)
            else:
                W = D.masked_fill(eye | ~active[None, :], inf)
                sc = torch.cumsum(torch.sort(W, dim=1).values, dim=1)[:, k - 1]
            if t == 0:
                fin = sc[torch.isfinite(sc)]
                scale = float(fin.max()) if fin.numel() and float(fin.max()) > 0 else 1.0
        i = int(torch.argmin(torch.where(active, sc, torch.full_like(sc, inf))))
        others = active & (idx != i)
        if i >= K:
            others = others & (idx < K)
        if bool(others.any()):
            gap = abs(float(sc[i]) - float(sc[others].min())) / scale
            if gap > 0.0:
                margin = min(margin, gap)
        sel.append(i)
        active = active & (idx != i)
    acc = (sel[0] >= K) if target == "krum" else all(not bool(active[j]) for j in range(K, n))
    nan = bool(torch.isnan(A).any() | torch.isnan(B).any() | torch.isnan(C).any())
    return bool(acc) and not nan, margin


def bulyan_coord(U: torch.Tensor, sel: torch.Tensor, beta: int) -> torch.Tensor:
    """Bulyan's coordinate step over the rows ``sel`` of U: per column the mean of the ``beta`` values with the
    smallest key (|x - med| in fp32, x), med the lower median (``k_bulyan_coord``)."""
    S = torch.sort(U.index_select(0, sel.long()), dim=0).values
    med = S[(S.shape[0] - 1) // 2]
    # S ascends, so a stable sort of the distances breaks their ties towards the smaller value
    order = torch.sort((S - med[None, :]).abs(), dim=0, stable=True).indices[:beta]
    return (S.gather(0, order).double().sum(dim=0) / beta).to(U.dtype)


def geomed_weights(G: torch.Tensor, alpha: torch.Tensor, iters: int, nu: float):
    """Smoothed Weiszfeld in Gram space (``k_geomed_weights``): G the centred Gram [n, n], alpha on the simplex ->
    (weights [n] fp64, iterations, objective).  The stop test is kept on the tensor's device (a CPU run also
    leaves the loop at it)."""
    G, a = G.double(), alpha.double()
    diag = G.diagonal()
    b = a.clone()
    obj = torch.zeros((), dtype=torch.float64, device=G.device)
    prev = torch.full_like(obj, float("inf"))
    it = torch.zeros((), dtype=torch.int32, device=G.device)
    done = torch.zeros((), dtype=torch.bool, device=G.device)
    for _ in range(int(iters)):
        gb = G @ b
        d = (diag - 2.0 * gb + b @ gb).clamp_min(0.0).sqrt()
        o = (a * d).sum()
        nb = a / d.clamp_min(nu)
        b = torch.where(done, b, nb / nb.sum())
        obj = torch.where(done, obj, o)
        it = it + (~done).to(torch.int32)
        done = done | ((o - prev).abs() <= 1e-9 * o)
        prev = o
        if not G.is_cuda and bool(done):
            break
    return b, it, obj


def centred_gram(U: torch.Tensor) -> torch.Tensor:
    """n x n Gram of the rows centred on their mean (fp64; ``k_gram_f64`` + double centring on the device)."""
    X = U.double()
    Xc = X - X.mean(dim=0, keepdim=True)
    return Xc @ Xc.t()


def gram_anchored(U: torch.Tensor, anchor: torch.Tensor) -> torch.Tensor:
    """n x n Gram of the rows about an external centre, <U_i - anchor, U_j - anchor> (fp64; ``k_gram_f64`` with an
    anchor on the device)."""
    Y = U.double() - anchor.double()[None, :]
    return Y @ Y.t()


def cclip_weights(G: torch.Tensor, alpha: torch.Tensor, c0: torch.Tensor, iters: int, tau: float):
    """Centred clipping in Gram space (``k_cclip_weights``; rule text in docs/PARITY.md): ``iters`` times
    d_i^2 = max(0, G_ii - 2 (G c)_i + c^T G c), s_i = 1 when d_i <= tau else tau / d_i, c <- (1 - S) c + alpha s with
    S = sum alpha s, from c = c0.  ``tau`` <= 0: the lower median (sorted position (m - 1) // 2) of the m finite rows'
    d_i of the first iteration.  A row whose G_ii is not finite has s = 0 and c = 0 and is left out of every sum and
    of the median; alpha is not renormalised.  -> (c [n] fp64, tau, rows with s < 1 in the last iteration, finite
    rows), the last three 0-d tensors.  Tensor ops only (no host read), so it also serves device tensors beyond the
    kernel's 64 rows."""
    G, a, c = G.double(), alpha.double(), c0.double()
    n = G.shape[0]
    diag = G.diagonal()
    fin = torch.isfinite(diag)
    zero = torch.zeros((), dtype=torch.float64, device=G.device)
    Gf = torch.where(fin[:, None] & fin[None, :], G, zero)  # (a skipped row or column adds nothing)
    diag = torch.where(fin, diag, zero)
    a = torch.where(fin, a, zero)
    c = torch.where(fin, c, zero)
    m = fin.sum()
    t = torch.full((), float(tau), dtype=torch.float64, device=G.device)
    clipped = torch.zeros((), dtype=torch.int64, device=G.device)
    for it in range(int(iters)):
        gc = (Gf * c[None, :]).sum(dim=1)  # (row by row in one order: identical rows get identical bits)
        d = (diag - 2.0 * gc + (c * gc).sum()).clamp_min(0.0).sqrt()
        if it == 0 and not float(tau) > 0.0:
            key = torch.sort(torch.where(fin, d, torch.full_like(d, float("inf")))).values
            t = torch.where(m > 0, key.gather(0, ((m - 1) // 2).clamp_min(0).reshape(1))[0], zero)
        s = torch.where(fin, torch.where(d <= t, torch.ones_like(d), t / d), zero)  # (d > t >= 0 where divided)
        c = torch.where(fin, (1.0 - (a * s).sum()) * c + a * s, zero)
        clipped = (fin & (s < 1.0)).sum()
    return c, t, clipped, m


def anchored_rows(U: torch.Tensor, c: torch.Tensor, anchor: torch.Tensor) -> torch.Tensor:
    """anchor + sum_{j: c_j != 0} c_j (U_j - anchor), the differences and the sum in fp64, rows in ascending order
    (``k_anchored_rows``).  A row with c_j == 0 is left out, not multiplied by zero."""
    g = anchor.double()
    c = c.to(device=U.device, dtype=torch.float64)
    acc = torch.zeros_like(g)
    for j in range(U.shape[0]):
        acc = acc + torch.where(c[j] != 0, c[j] * (U[j].double() - g), torch.zeros_like(g))
    return (g + acc).to(U.dtype)


def hist_gram(U: torch.Tensor, g: torch.Tensor, H: torch.Tensor, enable: Optional[torch.Tensor] = None):
    """FoolsGold's history step (``k_hist_gram``; rule text in docs/PARITY.md): H_new = H + (U - g[None]) in fp32, the
    difference rounded first and the sum second; ``enable`` (one int32, None = 1) of 0 keeps the bits of H -> (H_new, a
    new tensor, and the Gram H_new H_new^T in fp64).  Tensor ops only (no host read)."""
    H = H.to(torch.float32)
    Hn = H + (U.to(torch.float32) - g.to(device=U.device, dtype=torch.float32)[None, :])
    if enable is not None:
        Hn = torch.where(enable.to(H.device).reshape(()) != 0, Hn, H)
    return Hn, gram_anchored(Hn, torch.zeros_like(Hn[0]))


def foolsgold_weights(G: torch.Tensor, alpha0: torch.Tensor, kappa: float):
    """FoolsGold's weights from the Gram of the histories (``k_foolsgold_weights``; rule text in docs/PARITY.md):
    cosines cs_ij (0 for a pair with a zero or non-finite norm, clamped to [-1, 1]), v_i = max_{j != i} cs_ij, pardoning
    cs_ij v_i / v_j where v_j > v_i (a v_j of exactly 0 pardons nothing), a_i = clamp(1 - max_{j != i} cs'_ij, 0, 1),
    rescaled by their maximum M (M <= 0: every alpha is 0), an a_i of exactly 1 -> 0.99, alpha_i =
    clamp(kappa (ln(a_i / (1 - a_i)) + 0.5), 0, 1); one row: alpha = 1, v = 0 -> (alpha, v, alpha0 * alpha), fp64 [n].
    Tensor ops only (no host read), so it also serves device tensors beyond the kernel's 64 rows."""
    G, a0 = G.double(), alpha0.double()
    n = G.shape[0]
    if n == 1:
        one = torch.ones(1, dtype=torch.float64, device=G.device)
        return one, torch.zeros_like(one), a0 * one
    diag = G.diagonal()
    zero = torch.zeros((), dtype=torch.float64, device=G.device)
    nrm = torch.where(torch.isfinite(diag) & (diag > 0), diag.clamp_min(0.0).sqrt(), zero)
    live = (nrm[:, None] > 0) & (nrm[None, :] > 0)
    den = nrm[:, None] * nrm[None, :]
    cs = torch.where(live, G / torch.where(live, den, torch.ones_like(den)), zero).clamp(-1.0, 1.0)
    off = ~torch.eye(n, dtype=torch.bool, device=G.device)
    ninf = torch.full_like(cs, float("-inf"))
    v = torch.where(off, cs, ninf).max(dim=1).values
    vi, vj = v[:, None].expand(n, n), v[None, :].expand(n, n)
    pard = (vj > vi) & (vj != 0)
    csp = torch.where(pard, cs * vi / torch.where(pard, vj, torch.ones_like(vj)), cs)
    a = (1.0 - torch.where(off, csp, ninf).max(dim=1).values).clamp(0.0, 1.0)
    M = a.max()
    a = a / torch.where(M > 0, M, torch.ones_like(M))
    a = torch.where(a == 1.0, torch.full_like(a, 0.99), a)
    alpha = (float(kappa) * (torch.log(a / (1.0 - a)) + 0.5)).clamp(0.0, 1.0)
    alpha = torch.where(M > 0, alpha, torch.zeros_like(alpha))
    return alpha, v, a0 * alpha


def top_pc(G: torch.Tensor) -> torch.Tensor:
    """First principal-component scores v sqrt(lambda) from the centred Gram (``k_top_pc``, up to the sign)."""
    ev, V = torch.linalg.eigh(G)
    return V[:, -1] * torch.sqrt(ev[-1].clamp_min(0.0))


def _gmm_chol(S, r):
    Lc = np.zeros((4, 4))
    for i in range(r):
        for j in range(i + 1):
            s = S[i][j]
            for k in range(j):
                s -= Lc[i][k] * Lc[j][k]
            if i == j:
                if not s > 0.0:
                    return None
                Lc[i][i] = math.sqrt(s)
            else:
                Lc[i][j] = s / Lc[j][j]
    return Lc


def _gmm_md2(Lc, r, x, mu):
    y = [0.0] * r
    s = 0.0
    for i in range(r):
        v = x[i] - mu[i]
        for k in range(i):
            v -= Lc[i][k] * y[k]
        y[i] = v / Lc[i][i]
        s += y[i] * y[i]
    return s


def gmm_filter_ref(G: np.ndarray, att: np.ndarray, rank: Optional[int] = None):
    """Host mirror of ``agg.hip`` ``k_gmm_filter`` (same algorithm and operation order, fp64): returns
    (keep [n] bool, threshold, kept, ok).  See the kernel for the algorithm and its reference mapping.
    ``rank`` > 0 sets the PCA rank r = min(rank, 4, n); None / 0: r = max(1, min(4, n // 2 - 1)) (the
    sensitivity study: profiles/gmm_rank_study_r6.md)."""
    n = G.shape[0]
    A = [list(map(float, row)) for row in G]
    V = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    for _ in range(12):
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p][q]
                if abs(apq) < 1e-300:
                    continue
                th = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = (1.0 if th >= 0.0 else -1.0) / (abs(th) + math.sqrt(th * th + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                sn = t * c
                for k in range(n):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = c * akp - sn * akq
                    A[k][q] = sn * akp + c * akq
                for k in range(n):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = c * apk - sn * aqk
                    A[q][k] = sn * apk + c * aqk
                for k in range(n):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - sn * vkq
                    V[k][q] = sn * vkp + c * vkq
    order = sorted(range(n), key=lambda i: -A[i][i])  # stable: ties keep index order (as the insertion sort)
    ev = [A[i][i] for i in order]
    r = min(int(rank), 4, n) if rank else max(1, min(4, n // 2 - 1))
    Z = [[V[i][order[k]] * math.sqrt(max(ev[k], 1e-30)) for k in range(r)] for i in range(n)]
    zmax = max(1e-30, max(abs(z) for row in Z for z in row))
    Z = [[z / zmax for z in row] for row in Z]
    idx = [i for i in range(n) if not att[i]]
    nb = len(idx)
    idx += [i for i in range(n) if att[i]]
    X = [Z[i] for i in idx]
    m = len(X)
    K = 2 if m >= 2 else 1
    mu = [list(X[0]), list(X[0])]
    resp = [[1.0, 0.0] for _ in range(m)]
    if K == 2:
        far, best = 0, -1.0
        for i in range(m):
            d = sum((X[i][k] - X[0][k]) * (X[i][k] - X[0][k]) for k in range(r))
            if d > best:
                best, far = d, i
        mu[1] = list(X[far])
        for _ in range(10):
            s = [[0.0] * r, [0.0] * r]
            cnt = [0.0, 0.0]
            for i in range(m):
                d0 = d1 = 0.0
                for k in range(r):
                    d0 += (X[i][k] - mu[0][k]) * (X[i][k] - mu[0][k])
                    d1 += (X[i][k] - mu[1][k]) * (X[i][k] - mu[1][k])
                lab = 1 if d1 < d0 else 0
                resp[i] = [1.0 if lab == 0 else 0.0, 1.0 if lab == 1 else 0.0]
                cnt[lab] += 1.0
                for k in range(r):
                    s[lab][k] += X[i][k]
            for cc in range(2):
                if cnt[cc] > 0.0:
                    mu[cc] = [s[cc][k] / cnt[cc] for k in range(r)]
    eps10, reg, LOG2PI = 10.0 * 2.220446049250313e-16, 1e-6, 1.8378770664093453
    st = {"w": [0.0, 0.0], "Lc": [None, None], "logdet": [0.0, 0.0], "ok": True}

    def mstep():
        nks = 0.0
        for cc in range(K):
            nk = eps10
            for i in range(m):
                nk += resp[i][cc]
            for k in range(r):
                sm = 0.0
                for i in range(m):
                    sm += resp[i][cc] * X[i][k]
                mu[cc][k] = sm / nk
            cov = [[0.0] * 4 for _ in range(4)]
            for a_ in range(r):
                for b_ in range(r):
                    sm = 0.0
                    for i in range(m):
                        sm += resp[i][cc] * (X[i][a_] - mu[cc][a_]) * (X[i][b_] - mu[cc][b_])
                    cov[a_][b_] = sm / nk + (reg if a_ == b_ else 0.0)
            st["w"][cc] = nk
            nks += nk
            Lc = _gmm_chol(cov, r)
            if Lc is None:
                st["ok"] = False
                Lc = np.eye(4)
            st["Lc"][cc] = Lc
            st["logdet"][cc] = 2.0 * sum(math.log(Lc[k][k]) for k in range(r))
        for cc in range(K):
            st["w"][cc] /= nks

    def wlogp(x, cc):
        return math.log(st["w"][cc]) - 0.5 * (r * LOG2PI + _gmm_md2(st["Lc"][cc], r, x, mu[cc]) + st["logdet"][cc])

    mstep()
    lb = -math.inf
    it = 0
    while it < 100 and st["ok"]:
        prev = lb
        tot = 0.0
        for i in range(m):
            lp = [wlogp(X[i], 0), wlogp(X[i], 1) if K == 2 else -math.inf]
            mx = max(lp)
            lse = mx + math.log(math.exp(lp[0] - mx) + math.exp(lp[1] - mx))
            tot += lse
            resp[i] = [math.exp(lp[0] - lse), math.exp(lp[1] - lse) if K == 2 else 0.0]
        mstep()
        lb = tot / m
        it += 1
        if abs(lb - prev) < 1e-3:
            break
    mds = [math.sqrt(_gmm_md2(st["Lc"][0], r, X[i], mu[0])) for i in range(nb)]
    if nb:
        mb = sum(mds) / nb
        thr = 3.0 * math.sqrt(sum((d - mb) ** 2 for d in mds) / nb)
    else:
        thr = math.inf
    keep = np.zeros(n, dtype=bool)
    for i in range(n):
        cc = 1 if (K == 2 and wlogp(Z[i], 1) > wlogp(Z[i], 0)) else 0
        keep[i] = st["ok"] and math.sqrt(_gmm_md2(st["Lc"][cc], r, Z[i], mu[cc])) <= thr
    return keep, thr, int(keep.sum()), st["ok"]


def gmm_filter(G: torch.Tensor, att: torch.Tensor, rank: int = 0):
    """``gmm_filter_ref`` in the kernel's form: (keep [n] bool, info [3] fp64 = threshold, kept, ok) on G's device
    (the filter itself runs on the host)."""
    keep, thr, kept, ok = gmm_filter_ref(G.cpu().numpy(), att.cpu().numpy(), rank=rank)
    return (torch.from_numpy(keep).to(G.device),
            torch.tensor([thr, float(kept), float(ok)], dtype=torch.float64, device=G.device))


def row_norms(U: torch.Tensor) -> torch.Tensor:
    return torch.linalg.vector_norm(U.double(), dim=1)


def cosine_to(U: torch.Tensor, ref: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    Ud, rd = U.double(), ref.double()
    num = Ud @ rd
    den = torch.clamp(torch.linalg.vector_norm(Ud, dim=1) * torch.linalg.vector_norm(rd), min=eps)
    return num / den


def _mix64(z):
    """``afl_mix64`` (csrc/common.h, splitmix64 finaliser) on a numpy uint64 array."""
    import numpy as np

    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def afl_uniform(seed: int, n: int) -> torch.Tensor:
    """The [n] fp32 uniforms ``afl_uniform(seed, 0..n-1)`` of the device kernels (bit-identical)."""
    import numpy as np

    ctr = np.arange(n, dtype=np.uint64)
    x = _mix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ _mix64(ctr)) >> np.uint64(40)
    return torch.from_numpy((x.astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32))


def stochastic_quantize(U: torch.Tensor, seed=None):
    """ScionFL 1-bit quantisation per row: returns (sigma [N,P] {0,1}, smin [N], smax [N]).  ``seed`` (int):
    the device kernel's counter-based uniforms ``afl_uniform(seed, row * P + col)`` — the same bits as
    ``k_stoch_quant``; a ``torch.Generator`` or None draws with torch instead."""
    smin = U.min(dim=1).values
    smax = U.max(dim=1).values
    probs = (U - smin[:, None]) / (smax - smin + 1e-6)[:, None]
    if isinstance(seed, int):
        u = afl_uniform(seed, U.numel()).reshape(U.shape).to(U.device)
    elif seed is not None:
        u = torch.rand(U.shape, generator=seed, device=U.device, dtype=U.dtype)
    else:
        u = torch.rand_like(U)
    sigma = (u < probs).to(U.dtype)
    return sigma, smin, smax


# ---------------------------------------------------------------- optimizer
def adam_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int, lr: float,
              beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8) -> None:
    """In-place Adam (torch.optim.Adam default, non-foreach math)."""
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (v.sqrt() / (bc2 ** 0.5)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)


# ---------------------------------------------------------------- metrics
def roc_auc(scores: torch.Tensor, labels: torch.Tensor) -> float:
    """ROC-AUC with sklearn's tie handling (trapezoid over distinct thresholds)."""
    s = scores.reshape(-1).double()
    y = labels.reshape(-1).double()
    order = torch.argsort(s, descending=True, stable=True)
    s, y = s[order], y[order]
    tps = torch.cumsum(y, 0)
    fps = torch.cumsum(1 - y, 0)
    # keep the last index of every run of equal scores
    last = torch.ones_like(s, dtype=torch.bool)
    last[:-1] = s[1:] != s[:-1]
    tps, fps = tps[last], fps[last]
    P, N = tps[-1], fps[-1]
    if P <= 0 or N <= 0:
        return float("nan")
    tpr = torch.cat([tps.new_zeros(1), tps / P])
    fpr = torch.cat([fps.new_zeros(1), fps / N])
    return float(torch.trapz(tpr, fpr).item())


def adam_step_scaled(p, g, m, v, step: int, lr: float, scale: float, beta1=0.9, beta2=0.999, eps=1e-8) -> None:
    adam_step(p, g * scale, m, v, step, lr, beta1, beta2, eps)


# ---------------------------------------------------------------- hypernetwork
def hyper_delta_vjp(W: torch.Tensor, b: torch.Tensor, feat: torch.Tensor, u: torch.Tensor):
    """delta = W f + b - u  and  W^T delta (one pass over W in the native kernel)."""
    delta = torch.addmv(b, W, feat) - u
    return delta, W.t() @ delta


def hyper_adam_outer(W, b, m_wb, v_wb, delta, feat, step: int, lr: float, scale: float, beta1=0.9, beta2=0.999,
                     eps=1e-8) -> None:
    """Adam on the packed heads with grad(W) = scale·δ⊗f, grad(b) = scale·δ (never materialised natively)."""
    P, H = W.shape
    gW = torch.outer(delta, feat) * scale
    adam_step(W.view(-1), gW.view(-1), m_wb[:P * H], v_wb[:P * H], step, lr, beta1, beta2, eps)
    adam_step(b, delta * scale, m_wb[P * H:P * H + P], v_wb[P * H:P * H + P], step, lr, beta1, beta2, eps)


# ---------------------------------------------------------------- Philox noise (Random attack, K-G10)
_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF


def philox4x32(counter_lo, seed: int):
    """Philox4x32-10 of counters (lo, hi, 0, 0) for a uint64 numpy array ``counter_lo`` -> 4 uint32 arrays
    (the exact integers ``k_noise_philox`` draws; ``agg.hip``)."""
    import numpy as np

    g = counter_lo.astype(np.uint64)
    c0, c1 = g & np.uint64(_M32), g >> np.uint64(32)
    c2 = np.zeros_like(c0)
    c3 = np.zeros_like(c0)
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    for _ in range(10):
        p0 = c0 * np.uint64(_PHILOX_M0)
        p1 = c2 * np.uint64(_PHILOX_M1)
        h0, l0 = p0 >> np.uint64(32), p0 & np.uint64(_M32)
        h1, l1 = p1 >> np.uint64(32), p1 & np.uint64(_M32)
        c0, c1, c2, c3 = h1 ^ c1 ^ np.uint64(k0), l1, h0 ^ c3 ^ np.uint64(k1), l0
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return c0, c1, c2, c3


def philox_normal(n: int, seed: int):
    """N(0, 1) draws of ``k_noise_philox``: Box-Muller on (x + 1) * 2^-32 uniforms in fp64 -> [n] float64."""
    import numpy as np

    groups = (n + 3) // 4
    c0, c1, c2, c3 = philox4x32(np.arange(groups, dtype=np.uint64), seed)
    u = [(c.astype(np.float64) + 1.0) * 2.0 ** -32 for c in (c0, c1, c2, c3)]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    t0, t1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    z = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=1).reshape(-1)
    return z[:n]


def noise(own: torch.Tensor, sigma: float, seed: int) -> torch.Tensor:
    z = torch.from_numpy(philox_normal(own.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF)).to(torch.float32)
    return own + float(sigma) * z.reshape(own.shape).to(own.device)


# ---------------------------------------------------------------- DnC (docs/PARITY.md)
def dnc_keys(seed: int, t: int):
    """The two Feistel keys of DnC iteration ``t`` from the round's seed (mirror of plan_perm.h ``pl_dnc_keys``; the
    one place the derivation is written down on the Python side)."""
    from ..fl.trainers import _M32, _mix_i

    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a, b = _mix_i((seed & _M32) ^ 0x2545F491), _mix_i((seed >> 32) ^ 0x7F4A7C15)
    return _mix_i(a ^ ((0x165667B1 * (t + 1)) & _M32)), _mix_i((b + 0xD3A2646C * (t + 1)) & _M32)


def dnc_columns(P: int, b: int, t: int, seed: int) -> torch.Tensor:
    """Columns of DnC iteration ``t`` in summation (position) order, int64 [min(b, P)]: all of 0..P-1 in natural order
    when b >= P, else pi_t(0..b-1), pi_t the keyed Feistel permutation of [0, P) (bit-for-bit ``k_dnc_gram``'s)."""
    from ..fl.trainers import _perm_t

    P, b = int(P), int(b)
    if P < 1 or b < 1:
        raise ValueError(f"dnc_columns needs P >= 1 and b >= 1 (got {P}, {b})")
    i = torch.arange(min(b, P), dtype=torch.int64)
    if b >= P:
        return i
    k0, k1 = dnc_keys(seed, t)
    return _perm_t(i, P, k0, k1)


def dnc_gram(U: torch.Tensor, b: int, iters: int, seed: int) -> torch.Tensor:
    """[iters, n, n] fp64: per iteration the Gram of the sub-sampled rows centred on their column mean."""
    out = []
    for t in range(int(iters)):
        X = U.index_select(1, dnc_columns(U.shape[1], b, t, seed).to(U.device)).double()
        Xc = X - X.mean(dim=0, keepdim=True)
        out.append(Xc @ Xc.t())
    return torch.stack(out)


def dnc_select(G: torch.Tensor, drop: int, w: torch.Tensor, centre: bool = False):
    """DnC's select-and-intersect on the centred Grams ``G [iters, n, n]`` (``k_dnc_select``): scores
    s_t[i] = lambda_1 u_i^2 of the top eigenpair, the ``drop`` rows with the largest (score, index) dropped per
    iteration (NaN = +inf; on a tie the higher index goes), the masks ANDed, every row kept when none survives ->
    (keep [n] bool, scores [iters, n] fp64, weights [n] fp64 = w keep / sum).  ``centre``: double-centre G first.
    Tensor ops only (no host read), so it also serves device tensors beyond the kernel's 64 rows."""
    G = G.double()
    G = G[None] if G.dim() == 2 else G
    n = G.shape[1]
    if centre:
        G = G - G.mean(dim=1, keepdim=True) - G.mean(dim=2, keepdim=True) + G.mean(dim=(1, 2), keepdim=True)
    fin = torch.isfinite(G)
    bad = ~fin.all(dim=2).all(dim=1)  # a non-finite Gram: every score of the iteration is NaN
    ev, V = torch.linalg.eigh(torch.where(fin, G, torch.zeros_like(G)))
    u = V[:, :, -1]
    s = ev[:, -1].clamp_min(0.0)[:, None] * (u * u)
    s = torch.where(bad[:, None], torch.full_like(s, float("nan")), s)
    key = torch.where(torch.isnan(s), torch.full_like(s, float("inf")), s)
    idx = torch.arange(n, device=G.device)
    above = (key[:, None, :] > key[:, :, None]) | ((key[:, None, :] == key[:, :, None]) & (idx[None, :] > idx[:, None]))
    keep_t = above.sum(dim=2) >= int(drop)  # [iters, n]: row i stays when >= drop rows rank above it
    keep = keep_t.all(dim=0)
    keep = torch.where(keep.any(), keep, torch.ones_like(keep))
    wk = w.to(device=G.device, dtype=torch.float64) * keep.double()
    return keep, s, wk / wk.sum()


# ---------------------------------------------------------------- SignGuard (docs/PARITY.md)
def signguard_mix(seed: int) -> int:
    """The 32-bit word the window's first column comes from (mirror of plan_perm.h ``pl_signguard_mix``; the one place
    the derivation is written down on the Python side)."""
    from ..fl.trainers import _M32, _mix_i

    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a, b = _mix_i((seed & _M32) ^ 0x5347D1A3), _mix_i((seed >> 32) ^ 0x6A09E667)
    return _mix_i((a + 0x9E3779B9 * b) & _M32)


def signguard_window(P: int, frac: float, seed: int):
    """SignGuard's sampled columns as (s, b): the contiguous window s, s + 1, ..., s + b - 1 taken mod P, with
    b = min(P, max(1, ceil(frac P))) and s = mix(seed) mod P; all columns (b = P) start at s = 0."""
    P, frac = int(P), float(frac)
    if P < 1 or not frac > 0.0:
        raise ValueError(f"signguard_window needs P >= 1 and frac > 0 (got {P}, {frac})")
    b = P if frac >= 1.0 else min(P, max(1, math.ceil(frac * P)))
    return (0, P) if b >= P else (signguard_mix(seed) % P, b)


def sign_stats(U: torch.Tensor, g: torch.Tensor, s: int, b: int):
    """SignGuard's per-row statistics about the centre g (``k_sign_stats``) -> (q [n] fp64 = sum_p d_ip^2 over all P
    columns, pos [n], neg [n] int64 = the counts of d_ip > 0 and d_ip < 0 over the window (s, b)), d = U - g in fp64.
    A NaN difference is neither positive nor negative; an infinite one counts by its sign."""
    P, s, b = U.shape[1], int(s), int(b)
    if P < 1 or not 1 <= b <= P or not 0 <= s < P:
        raise ValueError(f"sign_stats needs 1 <= b <= P and 0 <= s < P (got s = {s}, b = {b}, P = {P})")
    d = U.double() - g.to(device=U.device).double()[None, :]
    q = (d * d).sum(dim=1)
    dw = d.index_select(1, (s + torch.arange(b, device=U.device)) % P)
    return q, (dw > 0).sum(dim=1), (dw < 0).sum(dim=1)


def _sg_margin(x: float, y: float) -> float:
    """The relative margin |x - y| / max(|x|, |y|) of a comparison between x and y (0 when they are equal, 1 against
    an infinite side)."""
    if x == y:
        return 0.0
    m = max(abs(x), abs(y))
    return 1.0 if math.isinf(m) else abs(x - y) / m


def _sg_d2(a, c) -> float:
    """Squared distance in the feature plane, in the kernel's expression shape ((dx dx + dy dy) + dz dz)."""
    dx, dy, dz = a[0] - c[0], a[1] - c[1], a[2] - c[2]
    return (dx * dx + dy * dy) + dz * dz


SIGNGUARD_MAX_ITER = 300


def signguard_select(q: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, b: int, alpha: torch.Tensor, lo: float,
                     hi: float):
    """SignGuard's decisions from the rows' statistics (``k_signguard_select``; steps 3 to 5 of the rule text in
    docs/PARITY.md): the norm filter about the lower median norm M, deterministic flat-kernel mean shift on the sign
    features F = (pos, b - pos - neg, neg) / b with the bandwidth h, the largest cluster, and the clipped weights
    c_i = keep_i alpha_i s_i / sum_kept alpha -> (keep [n] bool, norm_ok [n] bool, label [n] int64, F [n, 3] fp64,
    c [n] fp64, M, h (0-d fp64), margin).  Plain Python floats (IEEE fp64, no contraction) in the kernel's expression
    shapes and summation orders: distances are compared squared, sums run in index order.  It reads its inputs back to
    the host, so it serves any device and any n; the results go back to ``q``'s device.

    ``margin`` (a float) is the smallest relative margin |x - y| / max(|x|, |y|) met by any comparison whose outcome a
    rounding error could change: a finite norm against lo M and hi M, every squared distance against h^2 (the mean-shift
    memberships and counts, the dedup), every squared move against (1e-3 h)^2, a row's nearest centre against its
    second nearest, and the largest cluster's size against the runner-up's.  The counts that order the seeds are
    integers, the same on both sides whenever the memberships are; a tie among them goes to the lower index and changes
    the outcome only through a label or size tie, which is in the margin."""
    dev = q.device
    n, b, lo, hi = int(q.numel()), int(b), float(lo), float(hi)
    if n < 1 or b < 1:
        raise ValueError(f"signguard_select needs n >= 1 and b >= 1 (got {n}, {b}); lo <= hi is ``agg.signguard``'s check")
    ql = q.detach().double().cpu().reshape(-1).tolist()
    pl = [int(v) for v in pos.detach().cpu().reshape(-1).tolist()]
    nl = [int(v) for v in neg.detach().cpu().reshape(-1).tolist()]
    al = alpha.detach().double().cpu().reshape(-1).tolist()
    margin = [1.0]

    def le(x, y):  # x <= y, its margin recorded
        margin[0] = min(margin[0], _sg_margin(x, y))
        return x <= y

    # 3. norm filter
    inf = float("inf")
    norm = [math.sqrt(v) if math.isfinite(v) else inf for v in ql]
    M = sorted(norm)[(n - 1) // 2]
    ok = [math.isfinite(v) and math.isfinite(M) and le(lo * M, v) and le(v, hi * M) for v in norm]
    scale = [1.0 if v <= M else M / v for v in norm]
    # 4. features and bandwidth
    F = [(pl[i] / b, (b - pl[i] - nl[i]) / b, nl[i] / b) for i in range(n)]
    k = max(1, int(0.5 * n))
    rsum = 0.0
    for i in range(n):
        rsum += math.sqrt(sorted(_sg_d2(F[j], F[i]) for j in range(n))[k - 1])
    h = max(rsum / n, 1.0 / b)
    h2, tol = h * h, 1e-3 * h
    conv2 = tol * tol
    centres, cnt = [], []
    for i in range(n):
        c = F[i]
        for _ in range(SIGNGUARD_MAX_ITER):
            mem = [j for j in range(n) if le(_sg_d2(F[j], c), h2)]
            if not mem:
                break
            s0 = s1 = s2 = 0.0
            for j in mem:
                s0, s1, s2 = s0 + F[j][0], s1 + F[j][1], s2 + F[j][2]
            new = (s0 / len(mem), s1 / len(mem), s2 / len(mem))
            mv2, c = _sg_d2(new, c), new
            if le(mv2, conv2):
                break
        centres.append(c)
        cnt.append(sum(1 for j in range(n) if le(_sg_d2(F[j], c), h2)))
    # dedup, labels, the largest cluster
    order = sorted(range(n), key=lambda i: (-cnt[i], i))
    alive = [True] * n
    for p, sp in enumerate(order):
        if alive[sp]:
            for sq in order[p + 1:]:
                if alive[sq] and le(_sg_d2(centres[sq], centres[sp]), h2):
                    alive[sq] = False
    surv = [sp for sp in order if alive[sp]]
    label = []
    for i in range(n):
        d = [_sg_d2(F[i], centres[sp]) for sp in surv]
        best = min(range(len(surv)), key=lambda t: (d[t], t))
        if len(surv) > 1:
            margin[0] = min(margin[0], _sg_margin(d[best], min(v for t, v in enumerate(d) if t != best)))
        label.append(best)
    size = [sum(1 for v in label if v == t) for t in range(len(surv))]
    top = min(range(len(surv)), key=lambda t: (-size[t], t))
    if len(surv) > 1:
        margin[0] = min(margin[0], _sg_margin(float(size[top]), float(max(v for t, v in enumerate(size) if t != top))))
    # 5. weights
    keep = [ok[i] and label[i] == top for i in range(n)]
    den = 0.0
    for i in range(n):
        den += al[i] if keep[i] else 0.0
    c = [(al[i] * scale[i]) / den if keep[i] else 0.0 for i in range(n)]
    t64 = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)
    return (torch.tensor(keep, dtype=torch.bool, device=dev), torch.tensor(ok, dtype=torch.bool, device=dev),
            torch.tensor(label, dtype=torch.int64, device=dev), t64(F).reshape(n, 3), t64(c), t64(M), t64(h), margin[0])


def signguard_filter(U: torch.Tensor, g: torch.Tensor, frac: float, seed: int, alpha: torch.Tensor, lo: float,
                     hi: float):
    """``signguard_select`` on ``sign_stats`` over ``signguard_window`` -> its results without the margin, then the
    window (s, b)."""
    s, b = signguard_window(U.shape[1], frac, seed)
    q, pos, neg = sign_stats(U, g, s, b)
    return signguard_select(q, pos, neg, b, alpha, lo, hi)[:7] + ((s, b),)


# ---------------------------------------------------------------- FLAME (docs/PARITY.md)
def flame_key(seed: int) -> int:
    """The 64-bit Philox key of FLAME's server-side noise from the round's seed (the one place the derivation is written
    down: the native side takes the key).  The seed goes through the project's 32-bit mixer with constants of its own,
    so the stream is neither the Random attack's (keyed by its seed itself) nor scionfl's."""
    from ..fl.trainers import _M32, _mix_i

    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a, b = _mix_i((seed & _M32) ^ 0x464C414D), _mix_i((seed >> 32) ^ 0x3C6EF372)
    return _mix_i((a + 0x9E3779B9 * b) & _M32) | (_mix_i((b + 0xC2B2AE35 * a + 1) & _M32) << 32)


def flame_select(G: torch.Tensor, alpha: torch.Tensor, lam: float):
    """FLAME's decisions from the Gram G [n, n] of the updates about the centre (``k_flame_select``; steps 1 to 4 of the
    rule text in docs/PARITY.md, sigma of step 5) -> (keep [n] bool, c [n] fp64, info [5] fp64 = {S, sigma, d*, m, n'},
    margin).  Finite rows are those with a finite G_ii (n' of them, m = n' // 2 + 1); D_ij = 1 - G_ij / (sqrt(G_ii)
    sqrt(G_jj)) from the upper triangle of G, 1 when either norm is 0, +inf when the quotient is NaN; d* is the smallest
    threshold at which the graph D <= t on the finite rows has a component of >= m rows, and that component is kept; S
    is the lower median of the finite rows' norms, c_i = (alpha_i min(1, S / e_i)) / sum_kept alpha, sigma = lam S.
    Plain Python floats (IEEE fp64, correctly rounded sqrt and division, sums in index order): given the same G the
    kernel returns the same bits.  The threshold is found by a plain scan: the pairs in ascending order of D, a whole
    group of equal D united at a time, the components' sizes looked at after each group.  It reads G back to the host,
    so it serves any device and any n; the results go back to G's device.

    ``margin`` (a float): 0 when more than one pair attains d*, else the smallest |D_ij - d*| over the finite rows'
    pairs with D_ij != d* (+inf when there is none).  A perturbation of D below it changes neither the set of pairs
    under d* nor the pair at d*, so the kept set stands."""
    dev = G.device
    Gl = G.detach().double().cpu().tolist()
    n, lam = len(Gl), float(lam)
    if n < 1 or not (0.0 <= lam < math.inf):
        raise ValueError(f"flame_select needs n >= 1 and a finite lam >= 0 (got {n}, {lam})")
    al = alpha.detach().double().cpu().reshape(-1).tolist()
    fin = [i for i in range(n) if math.isfinite(Gl[i][i])]
    nf = len(fin)
    m = nf // 2 + 1
    e = [math.sqrt(Gl[i][i]) if i in fin and Gl[i][i] > 0.0 else 0.0 for i in range(n)]
    pairs = []
    for x, i in enumerate(fin):
        for j in fin[x + 1:]:
            d = 1.0
            if e[i] != 0.0 and e[j] != 0.0:
                d = 1.0 - Gl[i][j] / (e[i] * e[j])
                d = d if d == d else math.inf
            pairs.append((d, i, j))
    pairs.sort()
    comp = {i: {i} for i in fin}  # row -> its component (shared sets)
    kept, dstar, k = (set(fin) if nf == 1 else set()), 0.0, 0
    while k < len(pairs) and not kept:
        t = pairs[k][0]
        while k < len(pairs) and pairs[k][0] == t:
            _, i, j = pairs[k]
            if comp[i] is not comp[j]:
                comp[i] |= comp[j]
                for r in comp[j]:
                    comp[r] = comp[i]
            k += 1
        big = [s for s in comp.values() if len(s) >= m]
        if big:
            kept, dstar = big[0], t
    at = sum(1 for d, _, _ in pairs if d == dstar) if nf > 1 else 1
    gaps = [abs(d - dstar) for d, _, _ in pairs if d != dstar] if nf > 1 else []
    margin = 0.0 if at > 1 else (min(gaps) if gaps else math.inf)
    S = sorted(e[i] for i in fin)[(nf - 1) // 2] if nf else 0.0
    den = 0.0
    for i in range(n):
        den += al[i] if i in kept else 0.0
    c = [(al[i] * (1.0 if e[i] <= S else S / e[i])) / den if i in kept else 0.0 for i in range(n)]
    t64 = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)
    return (torch.tensor([i in kept for i in range(n)], dtype=torch.bool, device=dev), t64(c),
            t64([S, lam * S, dstar, float(m), float(nf)]), margin)


def flame_rows(U: torch.Tensor, c: torch.Tensor, anchor: torch.Tensor, sigma, seed: int) -> torch.Tensor:
    """anchor + sum_{j: c_j != 0} c_j (U_j - anchor) + sigma z (``k_flame_rows``): ``anchored_rows``' sum in fp64, then
    z = ``philox_normal`` under ``flame_key(seed)`` (column p takes draw p), one rounding to U's dtype.  sigma (a number
    or a one-element tensor) of 0: no draw, the bits of ``anchored_rows``."""
    s = float(sigma.reshape(-1)[0]) if torch.is_tensor(sigma) else float(sigma)
    if s == 0.0:
        return anchored_rows(U, c, anchor)
    g = anchor.double()
    c = c.to(device=U.device, dtype=torch.float64)
    acc = torch.zeros_like(g)
    for j in range(U.shape[0]):
        acc = acc + torch.where(c[j] != 0, c[j] * (U[j].double() - g), torch.zeros_like(g))
    z = torch.from_numpy(philox_normal(U.shape[1], flame_key(seed))).to(U.device)
    return ((g + acc) + s * z).to(U.dtype)


def flame_filter(U: torch.Tensor, g: torch.Tensor, alpha: torch.Tensor, lam: float):
    """``flame_select`` on ``gram_anchored`` -> its results without the margin."""
    return flame_select(gram_anchored(U, g.to(U.device)), alpha, lam)[:3]
