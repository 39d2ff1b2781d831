"""Op dispatch: HIP kernels for device tensors, PyTorch composites for CPU tensors.

Rule: a CUDA (ROCm) tensor ALWAYS goes to the native gfx950 kernel in ``attackfl_amd/_C.so``;
if that extension is missing on a GPU box the call raises (no silent eager fallback).  CPU
tensors run the composites in ``ops/composite.py``, which double as the numerical oracles in
the test-suite.
"""
from __future__ import annotations

import os
from typing import List, Sequence, Tuple, Optional

import torch

from . import composite

_NATIVE = None


def native():
    """Return the loaded native extension or raise with build instructions."""
    global _NATIVE
    if _NATIVE is None:
        try:
            variant = os.environ.get("AFL_NATIVE_SO")  # A/B builds (tools/ab_native.sh): another in-tree .so
            if variant:
                import importlib.machinery
                import importlib.util

                loader = importlib.machinery.ExtensionFileLoader("attackfl_amd._C", variant)
                spec = importlib.util.spec_from_file_location("attackfl_amd._C", variant, loader=loader)
                _C = importlib.util.module_from_spec(spec)
                loader.exec_module(_C)
            else:
                from .. import _C  # noqa: F401

            _NATIVE = _C
        except Exception as e:  # pragma: no cover - depends on build state
            _NATIVE = e
    if isinstance(_NATIVE, Exception):
        raise RuntimeError("attackfl_amd native extension (_C.so) is not built/loadable; run "
                           "`python -m attackfl_amd._build`: " + repr(_NATIVE))
    return _NATIVE


def native_available() -> bool:
    try:
        native()
        return True
    except RuntimeError:
        return False


def _dev(t: torch.Tensor) -> bool:
    return t.is_cuda


def _tiles(slots, P: int, tile: int = 4096):
    """Split [0, P) into tiles that never cross a slot boundary -> int32 [T, 3] (seg, start, end)."""
    rows = []
    for si, s in enumerate(slots):
        a, b = s.offset, s.offset + s.numel
        while a < b:
            e = min(b, a + tile)
            rows.append((si, a, e))
            a = e
    return torch.tensor(rows, dtype=torch.int32)


_TILE_CACHE = {}


def _tile_table(slots, P: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    key = (tuple((s.offset, s.numel) for s in slots), P, str(device))
    if key not in _TILE_CACHE:
        t = _tiles(slots, P)
        # segment -> [first tile, last tile) ranges for the deterministic second pass
        seg_first = torch.zeros(len(slots) + 1, dtype=torch.int32)
        for i in range(t.shape[0]):
            seg_first[int(t[i, 0]) + 1] = i + 1
        for si in range(1, len(slots) + 1):
            seg_first[si] = max(int(seg_first[si]), int(seg_first[si - 1]))
        _TILE_CACHE[key] = (t.to(device), seg_first.to(device))
    return _TILE_CACHE[key]


class _WholeSlot:
    def __init__(self, P):
        self.offset, self.numel, self.shape = 0, P, (P,)


# ---------------------------------------------------------------- column statistics / attacks
def column_mean_std(G: torch.Tensor):
    if _dev(G):
        out = native().colstats(G.contiguous(), 0, 0.0)
        return out[0], out[1]
    return composite.column_mean_std(G)


def lie_candidate(G: torch.Tensor, z: float) -> torch.Tensor:
    if _dev(G):
        return native().colstats(G.contiguous(), 1, float(z))[2]
    return composite.lie_candidate(G, z)


def pairwise_sqdist(G: torch.Tensor) -> torch.Tensor:
    """[K, K] fp64 squared L2 distances between rows.  Device: the Gram matrix of the rows centred on a robustly
    chosen row, on fp64 MFMA, for K <= 64 (``k_gram_f64``), the fp64 difference loop beyond (K <= 128)."""
    if _dev(G):
        if G.shape[0] <= 64:
            return native().pairwise_sqdist_gram(G.contiguous())
        return native().pairwise_sqdist(G.contiguous())
    return composite.pairwise_l2(G) ** 2


def pairwise_l2(G: torch.Tensor) -> torch.Tensor:
    if _dev(G):
        return pairwise_sqdist(G).clamp_min(0.0).sqrt()
    return composite.pairwise_l2(G)


def noise(own: torch.Tensor, sigma: float, seed: int) -> torch.Tensor:
    """``own + sigma * N(0, 1)`` from Philox4x32-10 keyed by ``seed`` (Random attack); the CPU mirror draws
    the same uniforms."""
    if _dev(own):
        return native().noise_philox(own.contiguous(), float(sigma),
                                     (int(seed) & 0xFFFFFFFFFFFFFFFF) - (1 << 64) if (int(seed) & (1 << 63))
                                     else int(seed) & 0xFFFFFFFFFFFFFFFF)
    return composite.noise(own, sigma, seed)


def segment_l2_sum(diffs: torch.Tensor, slots) -> torch.Tensor:
    if _dev(diffs):
        tiles, segf = _tile_table(slots, diffs.shape[1], diffs.device)
        sq = native().segment_sqsum(diffs.contiguous(), tiles, segf, len(slots))  # [M, S] fp64
        return sq.clamp_min(0.0).sqrt().sum(dim=1)
    return composite.segment_l2_sum(diffs, slots)


def batched_spectral_norm(mats: torch.Tensor) -> torch.Tensor:
    if _dev(mats):
        return native().spectral_norm(mats.contiguous())
    return composite.batched_spectral_norm(mats)


_SPEC_CACHE = {}


def _spectral_table(slots, device):
    """(tab [S', 4] int32 for slots with min(r, c) <= 128, max n, scratch floats per row, big slots)."""
    key = (tuple((s.offset, s.numel, s.shape[0]) for s in slots), str(device))
    if key not in _SPEC_CACHE:
        rows, big, scr, max_n = [], [], 0, 0
        for s in slots:
            r = int(s.shape[0])
            c = s.numel // r
            n = min(r, c)
            if n > 128:
                big.append(s)
                continue
            n8 = (n + 7) & ~7
            rows.append((s.offset, r, c, scr))
            scr += n8 * n8
            max_n = max(max_n, n)
        tab = torch.tensor(rows, dtype=torch.int32).reshape(-1, 4).to(device)
        _SPEC_CACHE[key] = (tab, max_n, scr, big)
    return _SPEC_CACHE[key]


_GRAM_CACHE = {}
_GRAM_NMAX = 64
_GRAM_LDS_FLOATS = 40 * 1024  # X and D of one slot staged whole in LDS (160 KB)


def _gram_table(slots, device):
    """Gram-form slots (n = min(r, c) <= 64, X and D fit in LDS): (tab [S', 4] int32 {offset, r, c, arena
    offset}, sumq, max LDS floats, the remaining slots)."""
    key = (tuple((s.offset, s.numel, s.shape[0]) for s in slots), str(device))
    if key not in _GRAM_CACHE:
        rows, rest, sumq, lds = [], [], 0, 0
        for s in slots:
            r = int(s.shape[0])
            c = s.numel // r
            n, k = min(r, c), max(r, c)
            need = 2 * n * (k + 1)
            if n > _GRAM_NMAX or need > _GRAM_LDS_FLOATS:
                rest.append(s)
                continue
            n16 = (n + 15) & ~15
            rows.append((s.offset, r, c, sumq))
            sumq += n16 * n16
            lds = max(lds, need)
        tab = torch.tensor(rows, dtype=torch.int32).reshape(-1, 4).to(device)
        _GRAM_CACHE[key] = (tab, sumq, lds, rest)
    return _GRAM_CACHE[key]


class SpectralFamily:
    """sum over matrix slots of ||X[m, slot] - γ·dev[slot]||_2 for every row m, for any γ (device).

    Reference: the per-tensor ord-2 norms of src/Utils.py:47 inside the bisections of src/Utils.py:101-204.
    The n x n Grams of X, X D^T + D X^T and D D^T are formed ONCE (``k_spec_grams``); each γ then costs one
    small launch (``k_spec_eval``: A - γS + γ²C, squarings on fp64 MFMA, Rayleigh quotient) that reads γ from
    device memory.  Slots outside the Gram form (n > 64) fall back to materialised rows per γ."""

    def __init__(self, X: torch.Tensor, slots, dev: Optional[torch.Tensor] = None):
        self.X = X.contiguous()
        self.dev = dev.contiguous() if dev is not None else None
        self.slots = slots
        self.tab, self.sumq, lds, self.rest = _gram_table(slots, X.device)
        self.arena = None
        if self.tab.shape[0] and X.shape[0]:
            self.arena = native().spec_grams(self.X, self.dev, self.tab, lds, self.sumq)

    def __call__(self, gamma=None) -> torch.Tensor:
        M = self.X.shape[0]
        out = torch.zeros(M, dtype=torch.float64, device=self.X.device)
        if M == 0:
            return out
        g = None
        if gamma is not None and self.dev is not None:
            g = gamma if torch.is_tensor(gamma) else torch.tensor(float(gamma), dtype=torch.float64)
            g = g.to(device=self.X.device, dtype=torch.float64).reshape(())
        if self.arena is not None:
            out += native().spec_eval(self.arena, self.tab, self.sumq, M, g).sum(dim=1)
        if self.rest:
            rows = self.X if g is None else self.X - (g * self.dev.double()).float()[None, :]
            out += _spectral_slots_direct(rows, self.rest)
        return out


def _spectral_slots_direct(diffs: torch.Tensor, slots) -> torch.Tensor:
    diffs = diffs.contiguous()
    tab, max_n, scr, big = _spectral_table(slots, diffs.device)
    out = torch.zeros(diffs.shape[0], dtype=torch.float64, device=diffs.device)
    if tab.shape[0]:
        out += native().spectral_norm_slots(diffs, tab, max_n, scr).sum(dim=1)
    for s in big:
        mats = diffs[:, s.offset:s.offset + s.numel].reshape(diffs.shape[0], s.shape[0], -1)
        out += native().spectral_norm(mats.contiguous())
    return out


def spectral_norm_sum(diffs: torch.Tensor, slots) -> torch.Tensor:
    """sum over matrix slots of ||diffs[m, slot]||_2 (slot viewed as [shape[0], -1]) -> [M] fp64.

    Device: the Gram form (two launches for every (row, slot) pair, reference src/Utils.py:47 per-tensor
    norm); slots with n > 64 through the direct ragged launch."""
    if _dev(diffs):
        return SpectralFamily(diffs, slots)()
    out = torch.zeros(diffs.shape[0], dtype=torch.float64, device=diffs.device)
    for s in slots:
        mats = diffs[:, s.offset:s.offset + s.numel].reshape(diffs.shape[0], s.shape[0], -1)
        out += composite.batched_spectral_norm(mats)
    return out


def attack_coeffs(G: torch.Tensor, mean: torch.Tensor, dev: torch.Tensor):
    if _dev(G):
        A, B, C = attack_coeffs_segments(G, mean, dev, [_WholeSlot(G.shape[1])])
        return A[:, 0], B[:, 0], C[0]
    return composite.attack_coeffs(G, mean, dev)


def attack_coeffs_segments(G: torch.Tensor, mean: torch.Tensor, dev: torch.Tensor, slots):
    if _dev(G):
        tiles, segf = _tile_table(slots, G.shape[1], G.device)
        A, B, C = native().attack_coeffs(G.contiguous(), mean.contiguous(), dev.contiguous(), tiles, segf, len(slots))
        return A, B, C
    return composite.attack_coeffs_segments(G, mean, dev, slots)


# ---------------------------------------------------------------- aggregation
def weighted_rows(U: torch.Tensor, w: torch.Tensor, ok: Optional[torch.Tensor] = None,
                  fallback: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sum_i w_i U_i; with ``ok`` / ``fallback``: ``fallback`` unless every ``ok`` > 0 (one pass on the device)."""
    if _dev(U):
        if ok is not None:
            return native().weighted_rows(U.contiguous(), w.to(device=U.device, dtype=torch.float64).contiguous(),
                                          ok.to(torch.int32).contiguous(), fallback.contiguous())
        return native().weighted_rows(U.contiguous(), w.to(device=U.device, dtype=torch.float64).contiguous())
    out = composite.weighted_rows(U, w)
    return out if ok is None else torch.where((ok > 0).all(), out, fallback)


def fedavg(U: torch.Tensor, sizes: torch.Tensor) -> torch.Tensor:
    s = sizes.to(torch.float64)
    if _dev(U):
        return weighted_rows(U, s / s.sum())
    return composite.fedavg(U, sizes)


def coord_median(U: torch.Tensor) -> torch.Tensor:
    if _dev(U):
        return native().coord_select(U.contiguous(), 0, 0)
    return composite.coord_median(U)


def trimmed_mean(U: torch.Tensor, trim_k: int) -> torch.Tensor:
    if _dev(U):
        return native().coord_select(U.contiguous(), 1, int(trim_k))
    return composite.trimmed_mean(U, trim_k)


def krum_select(D: torch.Tensor, f: int, rounds: int, iterated: bool):
    """Krum selection on the squared-distance matrix -> (sel [rounds] in selection order, mask [n] bool, first-pass
    scores [n] fp64).  Device, n <= 64: ``k_krum_select`` (one launch, no host read); the composite beyond."""
    if _dev(D) and D.shape[0] <= 64:
        sel, mask, scores = native().krum_select(D.to(torch.float64).contiguous(), int(f), int(rounds), bool(iterated))
        return sel, mask.bool(), scores
    return composite.krum_select(D, int(f), int(rounds), bool(iterated))


def mix_rows(W: torch.Tensor, U: torch.Tensor) -> torch.Tensor:
    """Y [R, P] = W U for a small dense W [R, n] (fp64) and rows U [n, P] (fp32): pre-aggregation's row mix, fp64
    accumulation in ascending j over every j.  Device, n <= 64 and R <= 64: ``k_mix_rows``, one pass over U, every
    Y[r] the bits of ``weighted_rows(U, W[r])``; a host W goes up pinned.  The composite beyond."""
    if _dev(U):
        from .layers import upload

        W = W.to(torch.float64)
        W = W if W.is_cuda else upload(W, U.device)
        if 1 <= U.shape[0] <= 64 and 1 <= W.shape[0] <= 64:
            return native().mix_rows(W.contiguous(), U.to(torch.float32).contiguous())
    return composite.mix_rows(W, U)


def nnm_weights(D: torch.Tensor, f: int):
    """Nearest-neighbour mixing's weights on the squared-distance matrix -> (W [n, n] fp64, the neighbour sets [n] as
    int64 bit masks).  Device, n <= 64: ``k_nnm_weights`` (one launch, no host read); the composite beyond."""
    if _dev(D) and D.shape[0] <= 64:
        W, nbr = native().nnm_weights(D.to(torch.float64).contiguous(), int(f))
        return W, nbr
    return composite.nnm_weights(D, int(f))


def agr_bisect_fused(Dg: torch.Tensor, A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, m: int, f: int, target: str,
                     n_iter: int, gamma: float) -> Optional[torch.Tensor]:
    """The AGR-tailored bisection as ONE launch (``agg.hip`` ``k_agr_bisect``) -> the state ``st [40]`` fp64 (st[1] last
    accepted γ, st[2] last tried, st[4 + i] tried, st[20 + i] accepted), or None where the kernel does not apply (CPU
    tensors, n' = K + m > 64, more than 16 iterations or none).  No host read and no pageable scalar copy."""
    if not _dev(Dg) or Dg.shape[0] + m > 64 or not 1 <= n_iter <= 16:
        return None
    f64 = lambda t: t.to(device=Dg.device, dtype=torch.float64).contiguous()
    st = torch.zeros(40, dtype=torch.float64, device=Dg.device)
    st[:1].fill_(float(gamma))  # (st[0] = x is a pageable scalar copy: a host wait for the side stream)
    native().agr_bisect(st, f64(Dg), f64(A).reshape(-1), f64(B).reshape(-1), f64(C).reshape(1), int(m), int(f),
                        composite.AGR_TARGETS.index(target), int(n_iter), float(gamma))
    return st


def agr_bisect(Dg: torch.Tensor, A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, m: int, f: int, target: str,
               gamma: float, tau: float):
    """Bisection on γ with the oracle "the rule ``target`` still selects the m copies of mean - γ·dev"
    (``composite.agr_oracle``) -> (last tried γ, iterations, last accepted γ, tried γs [n], decisions [n]) with the γs as
    fp64 tensors on the inputs' device.  Device, n' <= 64: ``k_agr_bisect``; otherwise the unrolled loop with
    device-side state (``attacks._bisect_device``) over the composite.  Neither reads a value back."""
    from ..attacks import _bisect_device, bisect_iterations

    n = bisect_iterations(gamma, tau)
    st = agr_bisect_fused(Dg, A, B, C, m, f, target, n, gamma)
    if st is not None:
        return st[2], n, st[1], st[4:4 + n], st[20:20 + n] > 0.5
    return _bisect_device(lambda g: composite.agr_oracle(Dg, A, B, C, g, m, f, target), gamma, tau, Dg.device)


def bulyan_coord(U: torch.Tensor, sel: torch.Tensor, beta: int) -> torch.Tensor:
    """Per column, the mean of the ``beta`` values closest to the lower median over the rows ``sel`` of U (a device
    index list on the device path: ``k_bulyan_coord`` reads the selected rows in place)."""
    if _dev(U) and sel.numel() <= 64:
        return native().bulyan_coord(U.contiguous(), sel.to(device=U.device, dtype=torch.int32).contiguous(), int(beta))
    return composite.bulyan_coord(U, sel, int(beta))


def geomed_weights(G: torch.Tensor, alpha: torch.Tensor, iters: int = 100, nu: float = 1e-6):
    """Smoothed-Weiszfeld weights from the centred Gram matrix -> (weights [n] fp64, iterations, objective), the
    last two 0-d tensors.  Device, n <= 64: ``k_geomed_weights``."""
    if _dev(G) and G.shape[0] <= 64:
        w, info = native().geomed_weights(G.to(torch.float64).contiguous(),
                                          alpha.to(device=G.device, dtype=torch.float64).contiguous(), int(iters),
                                          float(nu))
        return w, info[0].to(torch.int32), info[1]
    return composite.geomed_weights(G, alpha.to(G.device), int(iters), float(nu))


def gram_anchored(U: torch.Tensor, anchor: torch.Tensor) -> torch.Tensor:
    """n x n Gram of the rows about an external centre, <U_i - anchor, U_j - anchor> (fp64).  Device, n <= 64: one
    pass of the fp64-MFMA Gram kernel centred on ``anchor`` (``afl_gram_anchored``)."""
    if _dev(U) and 1 <= U.shape[0] <= 64:
        return native().gram_anchored(U.to(torch.float32).contiguous(),
                                      anchor.to(device=U.device, dtype=torch.float32).contiguous())
    return composite.gram_anchored(U, anchor.to(U.device))


def cclip_weights(G: torch.Tensor, alpha: torch.Tensor, c0: torch.Tensor, iters: int = 3, tau="auto"):
    """Centred-clipping coefficients from a Gram matrix -> (c [n] fp64, tau, rows clipped in the last iteration, finite
    rows), the last three 0-d tensors on G's device.  ``tau``: ``"auto"`` (the lower median of the first iteration's
    finite distances, found on the device) or a number > 0.  Device, n <= 64: ``k_cclip_weights``."""
    t = 0.0 if tau is None or (isinstance(tau, str) and tau == "auto") else float(tau)
    if _dev(G) and G.shape[0] <= 64:
        f64 = lambda x: x.to(device=G.device, dtype=torch.float64).contiguous()
        c, info = native().cclip_weights(f64(G), f64(alpha), f64(c0), int(iters), t)
        return c, info[0], info[1].to(torch.int32), info[2].to(torch.int32)
    return composite.cclip_weights(G, alpha.to(G.device), c0.to(G.device), int(iters), t)


def anchored_rows(U: torch.Tensor, c: torch.Tensor, anchor: torch.Tensor) -> torch.Tensor:
    """anchor + sum_{j: c_j != 0} c_j (U_j - anchor) with fp64 weights on the rows' device (``k_anchored_rows``)."""
    if _dev(U):
        return native().anchored_rows(U.to(torch.float32).contiguous(),
                                      c.to(device=U.device, dtype=torch.float64).contiguous(),
                                      anchor.to(device=U.device, dtype=torch.float32).contiguous())
    return composite.anchored_rows(U, c, anchor)


def hist_gram(U: torch.Tensor, g: torch.Tensor, H: torch.Tensor, enable: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None):
    """FoolsGold's history step -> (H_new, G): H_new = H + (U - g[None]) in fp32 (the bits of that torch expression;
    ``enable``, one int32 on the device, None = 1: with 0 the bits of H) and G = H_new H_new^T in fp64.  Device,
    n <= 64: one pass over U, g and H (``k_hist_gram``, then ``k_gram_reduce``), G bit-equal to
    ``gram_anchored(H_new, zeros)``; H_new goes to ``out`` when given (a second [n, P] fp32 buffer, never H)."""
    if _dev(U) and 1 <= U.shape[0] <= 64:
        f32 = lambda t: t.to(device=U.device, dtype=torch.float32).contiguous()
        en = (torch.ones(1, dtype=torch.int32, device=U.device) if enable is None
              else enable.to(device=U.device, dtype=torch.int32).reshape(1))
        Hn = out if out is not None else torch.empty(U.shape, dtype=torch.float32, device=U.device)
        return Hn, native().hist_gram(f32(U), f32(g), f32(H), en, Hn)
    Hn, G = composite.hist_gram(U, g, H.to(U.device), enable)
    if out is not None:
        Hn = out.copy_(Hn)
    return Hn, G


def foolsgold_weights(G: torch.Tensor, alpha0: torch.Tensor, kappa: float = 1.0):
    """FoolsGold's weights from the Gram of the histories -> (alpha [n], max cosine v [n], c = alpha0 * alpha [n]), fp64
    on G's device.  Device, n <= 64: ``k_foolsgold_weights`` (one launch, no host read); the composite beyond."""
    if not float(kappa) > 0.0:
        raise ValueError(f"foolsgold_weights: kappa must be a number > 0 (got {kappa!r})")
    if _dev(G) and G.shape[0] <= 64:
        out = native().foolsgold_weights(G.to(torch.float64).contiguous(),
                                         alpha0.to(device=G.device, dtype=torch.float64).contiguous(), float(kappa))
        return out[0], out[1], out[2]
    return composite.foolsgold_weights(G, alpha0.to(G.device), float(kappa))


def centred_gram(U: torch.Tensor) -> torch.Tensor:
    """n x n Gram of the rows centred on their mean (fp64).  Device, n <= 64: the fp64-MFMA Gram pass of ``agg.hip``
    (rows centred on one of them, then double-centred) instead of a generic fp64 GEMM with M = N = n and
    K = P (~50 k), a shape the library GEMM handles poorly."""
    if _dev(U) and 1 <= U.shape[0] <= 64:
        return native().gram_centred(U.to(torch.float32).contiguous())[0]
    return composite.centred_gram(U)


def gmm_filter(G: torch.Tensor, att: torch.Tensor, rank: int = 0):
    """The GMM gradient filter on the centred Gram -> (keep [n] bool, info [3] fp64 = threshold, kept, ok).  Device,
    n <= 64: ``k_gmm_filter``, one launch and no host read; host flags ``att`` go up pinned, never through a
    pageable copy that would wait for the stream.  Otherwise its host mirror (``composite.gmm_filter_ref``)."""
    if _dev(G) and G.shape[0] <= 64:
        from .layers import upload

        att = att.to(torch.uint8)
        att = att if att.is_cuda else upload(att, G.device)
        keep, info = native().gmm_filter(G.contiguous(), att.contiguous(), int(rank or 0))
        return keep.bool(), info
    return composite.gmm_filter(G, att, int(rank or 0))


def top_pc(G: torch.Tensor, sweeps: int = 12) -> torch.Tensor:
    """First principal-component scores from the centred Gram.  Device, n <= 64: a fixed-sweep Jacobi
    eigen-decomposition (``k_top_pc``, no host read); ``torch.linalg.eigh`` on the CPU / for larger n."""
    if _dev(G) and G.shape[0] <= 64:
        return native().top_pc(G.contiguous(), int(sweeps))
    return composite.top_pc(G)


def _seed64(seed: int) -> int:
    """A 64-bit seed as the signed integer the bindings take."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s - (1 << 64) if s & (1 << 63) else s


def _dnc_native(t: torch.Tensor, n: int) -> bool:
    return _dev(t) and 1 <= n <= 64


def dnc_columns(P: int, b: int, t: int, seed: int) -> torch.Tensor:
    """Columns of DnC iteration ``t`` in summation order (the host mirror of ``k_dnc_gram``'s keyed Feistel map)."""
    return composite.dnc_columns(P, b, t, seed)


def dnc_gram(U: torch.Tensor, b: int, iters: int, seed: int) -> torch.Tensor:
    """[iters, n, n] fp64 Grams of the rows over each iteration's ``b`` keyed columns, centred on the column mean.
    Device, n <= 64: ``k_dnc_gram`` + the double centring of ``k_dnc_select``."""
    if _dnc_native(U, U.shape[0]):
        ones = torch.ones(U.shape[0], dtype=torch.float64, device=U.device)
        return native().dnc_run(U.to(torch.float32).contiguous(), int(b), int(iters), _seed64(seed), 0, ones, False)[3]
    return composite.dnc_gram(U, int(b), int(iters), seed)


def dnc_select(G: torch.Tensor, drop: int, w: torch.Tensor, centre: bool = False):
    """DnC scores, ranked drop and mask intersection on centred Grams [iters, n, n] -> (keep [n] bool, scores
    [iters, n] fp64, weights [n] fp64 = w keep / sum).  Device, n <= 64: ``k_dnc_select`` (one launch, no host read)."""
    G = G[None] if G.dim() == 2 else G
    if _dnc_native(G, G.shape[1]):
        keep, scores, weights, _ = native().dnc_run(G.to(torch.float64).contiguous(), 0, 0, 0, int(drop),
                                                    w.to(device=G.device, dtype=torch.float64).contiguous(),
                                                    bool(centre))
        return keep.bool(), scores, weights
    return composite.dnc_select(G, int(drop), w, bool(centre))


def dnc_filter(U: torch.Tensor, b: int, iters: int, seed: int, drop: int, w: torch.Tensor):
    """``dnc_select(dnc_gram(U, ...), drop, w)``; on the device (n <= 64) two launches for any ``iters``: the Gram
    partials go straight into the select kernel."""
    if _dnc_native(U, U.shape[0]):
        keep, scores, weights, _ = native().dnc_run(U.to(torch.float32).contiguous(), int(b), int(iters), _seed64(seed),
                                                    int(drop), w.to(device=U.device, dtype=torch.float64).contiguous(),
                                                    False)
        return keep.bool(), scores, weights
    return composite.dnc_select(composite.dnc_gram(U, int(b), int(iters), seed), int(drop), w)


def _sg_native(t: torch.Tensor, n: int) -> bool:
    return _dev(t) and 1 <= n <= 64


def _sg_out(out):
    keep, ok, label, F, c, info = out[:6]
    return keep.bool(), ok.bool(), label.to(torch.int64), F, c, info[0], info[1]


def signguard_window(P: int, frac: float, seed: int, native_mix: bool = False):
    """SignGuard's sampled window (s, b) of (seed, P) (``composite.signguard_window``); ``native_mix``: s from the
    native twin of the mixer (plan_perm.h ``pl_signguard_start``), which the device path uses."""
    s, b = composite.signguard_window(P, frac, seed)
    if native_mix and b < int(P):
        s = int(native().signguard_start(_seed64(seed), int(P)))
    return s, b


def sign_stats(U: torch.Tensor, g: torch.Tensor, s: int, b: int):
    """SignGuard's row statistics about the centre g -> (q [n] fp64 squared norms of U - g, pos [n], neg [n] int64 sign
    counts on the window (s, b)).  Device, n <= 64: ``k_sign_stats``, one pass over U and g, its block partials summed
    in block order by ``k_signguard_select``: this call runs both launches of ``signguard_filter`` (with equal weights
    and lo = hi = 1) and returns the statistics the second one summed, so it costs what ``signguard_filter`` costs and
    is there for tests and tools, not for a round.  A non-contiguous view is made contiguous first."""
    if _sg_native(U, U.shape[0]):
        one = torch.ones(U.shape[0], dtype=torch.float64, device=U.device)
        out = native().signguard_run(U.to(torch.float32).contiguous(),
                                     g.to(device=U.device, dtype=torch.float32).contiguous(), int(s), int(b), one,
                                     1.0, 1.0)
        return out[6], out[7][:, 0].to(torch.int64), out[7][:, 1].to(torch.int64)
    return composite.sign_stats(U, g, int(s), int(b))


def signguard_select(q: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, b: int, alpha: torch.Tensor, lo: float,
                     hi: float):
    """SignGuard's decisions from the row statistics -> (keep [n] bool, norm_ok [n] bool, label [n] int64, features
    [n, 3] fp64, c [n] fp64, M, h), the last two 0-d fp64.  Device, n <= 64: ``k_signguard_select`` (one launch, no
    host read); otherwise the host mirror, which reads the statistics back."""
    if _sg_native(q, q.numel()):
        i32 = lambda t: t.to(device=q.device, dtype=torch.int32).contiguous()
        return _sg_out(native().signguard_select(q.to(torch.float64).contiguous(), i32(pos), i32(neg), int(b),
                                                 alpha.to(device=q.device, dtype=torch.float64).contiguous(),
                                                 float(lo), float(hi)))
    return composite.signguard_select(q, pos, neg, int(b), alpha, float(lo), float(hi))[:7]


def signguard_filter(U: torch.Tensor, g: torch.Tensor, frac: float, seed: int, alpha: torch.Tensor, lo: float,
                     hi: float):
    """``signguard_select`` on ``sign_stats`` over the window of (frac, seed) -> its seven results, then the window
    (s, b).  Device, n <= 64: two launches (``k_sign_stats``, ``k_signguard_select``), no host read."""
    if _sg_native(U, U.shape[0]):
        s, b = signguard_window(U.shape[1], frac, seed, native_mix=True)
        out = native().signguard_run(U.to(torch.float32).contiguous(),
                                     g.to(device=U.device, dtype=torch.float32).contiguous(), s, b,
                                     alpha.to(device=U.device, dtype=torch.float64).contiguous(), float(lo), float(hi))
        return _sg_out(out) + ((s, b),)
    return composite.signguard_filter(U, g, frac, seed, alpha.to(U.device), float(lo), float(hi))


def flame_select(G: torch.Tensor, alpha: torch.Tensor, lam: float):
    """FLAME's decisions from the Gram about the centre -> (keep [n] bool, c [n] fp64, info [5] fp64 = {S the lower
    median norm, sigma = lam S, d* the threshold, m the majority, n' the finite rows}) on G's device.  Device, n <= 64:
    ``k_flame_select`` (one launch, no host read); otherwise the host mirror, which reads G back."""
    if _dev(G) and 1 <= G.shape[0] <= 64:
        keep, c, info = native().flame_select(G.to(torch.float64).contiguous(),
                                              alpha.to(device=G.device, dtype=torch.float64).contiguous(), float(lam))
        return keep.bool(), c, info
    return composite.flame_select(G, alpha, float(lam))[:3]


def flame_filter(U: torch.Tensor, g: torch.Tensor, alpha: torch.Tensor, lam: float):
    """``flame_select`` on ``gram_anchored(U, g)``.  Device, n <= 64: three launches (``k_gram_f64``, ``k_gram_reduce``,
    ``k_flame_select``), no host read."""
    return flame_select(gram_anchored(U, g), alpha, lam)


def flame_rows(U: torch.Tensor, c: torch.Tensor, anchor: torch.Tensor, sigma, seed: int) -> torch.Tensor:
    """anchor + sum_{j: c_j != 0} c_j (U_j - anchor) + sigma z, z the Philox normals under ``composite.flame_key(seed)``
    (``k_flame_rows``: one pass over U; sigma, a number or a one-element fp64 tensor such as ``flame_select``'s
    info[1:2], is read on the device).  sigma = 0: the bits of ``anchored_rows``."""
    if _dev(U):
        s = (sigma.to(device=U.device, dtype=torch.float64).reshape(-1) if torch.is_tensor(sigma)
             else torch.full((1,), float(sigma), dtype=torch.float64, device=U.device))
        return native().flame_rows(U.to(torch.float32).contiguous(),
                                   c.to(device=U.device, dtype=torch.float64).contiguous(),
                                   anchor.to(device=U.device, dtype=torch.float32).contiguous(), s,
                                   _seed64(composite.flame_key(seed)))
    return composite.flame_rows(U, c, anchor, sigma, seed)


def row_norms(U: torch.Tensor) -> torch.Tensor:
    if _dev(U):
        return native().row_dots(U.contiguous(), U.new_zeros(0), 0)[:, 0].clamp_min(0).sqrt()
    return composite.row_norms(U)


def cosine_to(U: torch.Tensor, ref: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    if _dev(U):
        d = native().row_dots(U.contiguous(), ref.contiguous(), 1)  # [N, 3]: <u,u>, <u,r>, <r,r>
        den = torch.clamp(d[:, 0].sqrt() * d[:, 2].sqrt(), min=eps)
        return d[:, 1] / den
    return composite.cosine_to(U, ref, eps)


def stochastic_quantize(U: torch.Tensor, seed: int):
    if _dev(U):
        sigma, smin, smax = native().stoch_quant(U.contiguous(), int(seed) & 0x7FFFFFFFFFFFFFFF)
        return sigma, smin, smax
    return composite.stochastic_quantize(U, int(seed) & 0x7FFFFFFFFFFFFFFF)  # (the kernel's uniforms)


# ---------------------------------------------------------------- optimizer
def adam_step(p, g, m, v, step: int, lr: float, beta1=0.9, beta2=0.999, eps=1e-8) -> None:
    if _dev(p):
        native().adam_flat(p, g, m, v, int(step), float(lr), float(beta1), float(beta2), float(eps), 1.0)
        return
    composite.adam_step(p, g, m, v, step, lr, beta1, beta2, eps)


# ---------------------------------------------------------------- metrics
def roc_auc(scores: torch.Tensor, labels: torch.Tensor) -> float:
    if _dev(scores):
        return float(native().roc_auc(scores.reshape(-1).float().contiguous(), labels.reshape(-1).float().contiguous()))
    return composite.roc_auc(scores, labels)


def roc_auc_checked(scores: torch.Tensor, labels: torch.Tensor):
    """(ROC-AUC, any NaN score) with ONE host synchronisation on the device path."""
    if _dev(scores):
        r = native().roc_auc_dev(scores.reshape(-1).float().contiguous(), labels.reshape(-1).float().contiguous())
        auc, nan = r.cpu().tolist()
        return auc, nan > 0.5
    nan = bool(torch.isnan(scores).any())
    return (float("nan") if nan else composite.roc_auc(scores, labels)), nan


def adam_step_scaled(p, g, m, v, step: int, lr: float, scale: float, beta1=0.9, beta2=0.999, eps=1e-8) -> None:
    if _dev(p):
        native().adam_flat(p, g, m, v, int(step), float(lr), float(beta1), float(beta2), float(eps), float(scale))
        return
    composite.adam_step_scaled(p, g, m, v, step, lr, scale, beta1, beta2, eps)


# ---------------------------------------------------------------- hypernetwork
def hyper_delta_vjp(W: torch.Tensor, b: torch.Tensor, feat: torch.Tensor, u: torch.Tensor):
    if _dev(W):
        out = native().hyper_delta_vjp(W, b, feat.contiguous(), u.contiguous())
        return out[0], out[1]
    return composite.hyper_delta_vjp(W, b, feat, u)


def hyper_adam_outer(W, b, m_wb, v_wb, delta, feat, step: int, lr: float, scale: float) -> None:
    if _dev(W):
        native().hyper_adam_outer(W, b, m_wb, v_wb, delta.contiguous(), feat.contiguous(), int(step), float(lr),
                                  0.9, 0.999, 1e-8, float(scale))
        return
    composite.hyper_adam_outer(W, b, m_wb, v_wb, delta, feat, step, lr, scale)


def hyper_server_update(arena, m, v, U, urows, clients, layout, step0: int, lr: float, clip: float,
                        beta1=0.9, beta2=0.999, eps=1e-8, enable: Optional[torch.Tensor] = None, gen=()):
    """Sequential pFedHN server update of a whole round on the device (no host sync) -> (info [n, 2],
    generated [len(gen), P]).  ``enable``: optional device int32 word; 0 leaves arena / moments untouched (decided
    on the device).  ``gen``: clients whose models the updated hypernetwork generates inside the update's last
    launches (the next START; <= 32)."""
    info, out = native().hyper_server_update(arena, m, v, U.contiguous(), [int(r) for r in urows],
                                             [int(c) for c in clients], [int(x) for x in layout], int(step0),
                                             float(lr), float(clip), float(beta1), float(beta2), float(eps), enable,
                                             [int(c) for c in gen])
    return info, out


def hyper_features(arena, clients, layout) -> torch.Tensor:
    return native().hyper_features(arena, [int(c) for c in clients], [int(x) for x in layout])


def hyper_generate_many(arena, clients, layout) -> torch.Tensor:
    """Models [n, P] of ``clients`` generated from the packed hypernetwork arena (device; the same per-row
    arithmetic as the generation fused into ``hyper_server_update``)."""
    return native().hyper_generate_many(arena, [int(c) for c in clients], [int(x) for x in layout])


def hyper_generate(W: torch.Tensor, b: torch.Tensor, feat: torch.Tensor) -> torch.Tensor:
    if _dev(W):
        return native().hyper_generate(W, b, feat.contiguous())
    return torch.addmv(b, W, feat)
