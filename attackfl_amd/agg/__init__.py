"""Server aggregation rules / robust defenses on the gathered update matrix ``U [N, P]``.

Each rule returns ``AggResult(params [P] | None, ok, info)``.  Rows are in client-index order;
``sizes [N]`` are the clients' reported sample counts; ``attackers [N]`` the oracle attacker flags
(only GMM uses them, as the reference does).  Reference sites:

* fedavg        ``server.py:751-775``      size-weighted mean (fp64 accumulation)
* trimmed_mean  ``src/Utils.py:267-302``   coordinate-wise, trim int(0.1·N) per side
* median        ``src/Utils.py:344-357``   coordinate-wise lower median (``torch.median``)
* krum          ``server.py:373-389``, ``src/Utils.py:326-342``  f = int(N·0.0) (A-11)
* shieldfl      ``server.py:306-350``      cosine-to-mean inverse-deviation weights
* gmm           ``server.py:352-372``, ``src/Utils.py:250-323``  (crashes in the reference, A-8;
  here: 2-component GMM in the rank-(N-1) principal subspace = low-rank Mahalanobis)
* scionfl       ``server.py:436-492``, ``src/Utils.py:371-387``  1-bit stochastic quantisation +
  norm clip + cosine filter + FedAvg of the kept originals
* fltracer      ``src/Utils.py:359-369`` (dormant in the reference)  PCA(1) + MAD z-score
* byzantine     ``src/Utils.py:218-248`` (dead code in the reference) cosine ≥ 0.9 to model 0
Beyond the reference (docs/PARITY.md): multi_krum, bulyan, dnc (assumed Byzantine count ``byz-f``), geomed (RFA) and
cclip (centred clipping about the global model the round started from) and signguard (SignGuard: a norm filter about the
median norm and a mean-shift clustering of the rows' sign statistics) and flame (FLAME: the majority cluster of the
updates' cosine distances, clipping to the median norm, Gaussian noise); the last three are the rules that take
``centre``.
Pre-aggregation in front of a rule (engine ``pre-agg``): ``nnm`` (nearest-neighbour mixing) and ``bucketing``.
``foolsgold`` (FoolsGold) is the one stateful rule: it takes and returns the clients' update history, so it is called by
name (``fl/server_modes.py`` ``FoolsGoldMode``) and is not an entry of AGGREGATORS, the table of stateless rules.
FLTrust and the hypernetwork are server modes of their own (``fl/server_modes.py``, ``fl/hyper_server.py``): they train.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, Optional, Union

import torch

from .. import ops
from ..config import BUCKET_SIZE, FOOLSGOLD_KAPPA, KNOB, PRE_AGG_KINDS  # (a knob's default and check: stated once, in config)
from ..config import FLAME_NOISE, SIGNGUARD_FRAC, SIGNGUARD_HI, SIGNGUARD_LO
from ..ops.composite import gmm_filter_ref  # noqa: F401  (the kernel's host mirror: tools and tests import it here)


@dataclass
class AggResult:
    params: Optional[torch.Tensor]
    ok: Union[bool, torch.Tensor] = True  # a 0-d device bool where the rule decides on the device (gmm)
    info: Dict = field(default_factory=dict)


def fedavg(U: torch.Tensor, sizes: torch.Tensor, **_) -> AggResult:
    if U.shape[0] == 0:
        return AggResult(None, True, {"n": 0})
    return AggResult(ops.fedavg(U, sizes), True, {"n": int(U.shape[0])})


def mean_of(U: torch.Tensor) -> torch.Tensor:
    w = torch.full((U.shape[0],), 1.0 / U.shape[0], dtype=torch.float64, device=U.device)
    return ops.weighted_rows(U, w)


def host_info(info: Dict) -> Dict:
    """An aggregator's info with device values read back (the engine calls it where the host waits anyway,
    after validation): bool masks become index lists, 0-d tensors numbers, vectors lists; a nested dict
    (``pre_agg``) likewise."""
    out = {}
    for k, v in info.items():
        if isinstance(v, dict):
            v = host_info(v)
        elif torch.is_tensor(v):
            v = v.cpu()
            if v.dtype == torch.bool:
                v = torch.nonzero(v).reshape(-1).tolist() if v.dim() else bool(v)
            elif v.dim() == 0:
                v = int(v) if not v.is_floating_point() else float(v)
            else:
                v = v.tolist()
        out[k] = v
    return out


def _device_weights(sizes: Optional[torch.Tensor], device, n: int = 0) -> torch.Tensor:
    """Host sizes (None: n ones) -> a device fp64 vector without a synchronising pageable copy."""
    s = torch.ones(n, dtype=torch.float64) if sizes is None else sizes.to(torch.float64)
    if torch.device(device).type == "cuda" and s.device.type == "cpu":
        s = s.pin_memory().to(device, non_blocking=True)
    return s.to(device)


def _masked_mean(U: torch.Tensor, keep: torch.Tensor, w: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weighted mean over the rows where ``keep`` (all rows when none is kept), on the device."""
    keep = torch.where(keep.any(), keep, torch.ones_like(keep))
    w = keep.double() if w is None else keep.double() * w
    return ops.weighted_rows(U, w / w.sum())


def trimmed_mean(U: torch.Tensor, sizes=None, trim_ratio: float = 0.1, **_) -> AggResult:
    n = U.shape[0]
    k = int(n * trim_ratio)
    if 2 * k >= n:
        raise ValueError("Too few clients for the chosen trim_ratio.")
    return AggResult(ops.trimmed_mean(U, k), True, {"trim_k": k})


def median(U: torch.Tensor, sizes=None, **_) -> AggResult:
    return AggResult(ops.coord_median(U), True, {})


def krum(U: torch.Tensor, sizes=None, f_rate: float = 0.0, **_) -> AggResult:
    """Krum without a host read: fp64 Gram distances, each row's own distance pushed to +inf, a row sort,
    the n-f-2 smallest summed and the argmin (first minimum, like ``np.argmin``) selected on the device."""
    n = U.shape[0]
    f = int(n * f_rate)
    m = max(n - f - 2, 0)
    d2 = ops.pairwise_sqdist(U).double()
    d2 = d2 + torch.diag(torch.full((n,), float("inf"), dtype=torch.float64, device=d2.device))
    scores = torch.sort(d2, dim=1).values[:, :m].sum(dim=1)
    sel = torch.argmin(scores)
    return AggResult(U.index_select(0, sel.reshape(1))[0], True, {"selected": sel, "f": f, "scores": scores})


def byzantine_count(n: int, byz_f=KNOB["byz_f"].default, per_f: int = 4, rule: str = "bulyan") -> int:
    """The assumed number f of Byzantine rows (engine ``byz-f``).  ``auto``: max(0, (n - 3) // 4), the largest f
    Bulyan admits.  An explicit f >= 1 must leave n >= per_f * f + 3 rows (2 f + 3 for Multi-Krum, 4 f + 3 for
    Bulyan); f = 0 claims no tolerance and is admitted for any n."""
    f = KNOB["byz_f"].check(byz_f, coerce=True)
    if f == "auto":
        return max(0, (n - 3) // 4)
    if f > 0 and n < per_f * f + 3:
        raise ValueError(f"Too few clients for {rule} with byz-f = {f}: n = {n}, needs n >= {per_f} f + 3 = "
                         f"{per_f * f + 3}.")
    return f


def multi_krum(U: torch.Tensor, sizes=None, byz_f=KNOB["byz_f"].default, **_) -> AggResult:
    """Multi-Krum (Blanchard et al., NeurIPS 2017; beyond the reference, whose ``krum`` keeps f = 0, A-11): Krum scores
    with k = max(n - f - 2, 1) neighbours on all rows, the n - f rows with the smallest (score, index), their
    size-weighted mean.  One ``k_krum_select`` launch on the Gram-form distances; no host read."""
    n = U.shape[0]
    f = byzantine_count(n, byz_f, 2, "multi_krum")
    _, keep, scores = ops.krum_select(ops.pairwise_sqdist(U), f, n - f, False)
    w = _device_weights(sizes, U.device, n) * keep.double()
    return AggResult(ops.weighted_rows(U, w / w.sum()), True, {"selected": keep, "f": f, "scores": scores})


def bulyan(U: torch.Tensor, sizes=None, byz_f=KNOB["byz_f"].default, **_) -> AggResult:
    """Bulyan (El Mhamdi et al., ICML 2018; beyond the reference): theta = n - 2 f rows by iterated Krum (re-scored on
    the rows still active before every pick), then per column the unweighted mean of the beta = theta - 2 f values
    closest to the lower median of the selected ones.  Two launches after the distances (``k_krum_select``,
    ``k_bulyan_coord`` on the device index list); no host read: theta, beta and the kernel variant follow from n, f."""
    n = U.shape[0]
    f = byzantine_count(n, byz_f, 4, "bulyan")
    theta = n - 2 * f
    sel, keep, scores = ops.krum_select(ops.pairwise_sqdist(U), f, theta, True)
    return AggResult(ops.bulyan_coord(U, sel, theta - 2 * f), True, {"selected": keep, "f": f, "scores": scores})


def geomed(U: torch.Tensor, sizes=None, geomed_iters: int = KNOB["geomed_iters"].default,
           geomed_nu: float = KNOB["geomed_nu"].default, **_) -> AggResult:
    """Geometric median by the smoothed Weiszfeld iteration of RFA (Pillutla et al., 2022; beyond the reference),
    weighted by alpha = sizes / sum sizes, run in Gram space on the n x n centred Gram (``k_geomed_weights``): the
    rows are read by the Gram pass and by the final ``weighted_rows`` only.  No host read."""
    n = U.shape[0]
    a = _device_weights(sizes, U.device, n)
    w, iters, obj = ops.geomed_weights(ops.centred_gram(U), a / a.sum(), int(geomed_iters), float(geomed_nu))
    return AggResult(ops.weighted_rows(U, w), True, {"weights": w, "iters": iters, "objective": obj})


def cclip(U: torch.Tensor, sizes=None, centre: Optional[torch.Tensor] = None,
          cclip_iters: int = KNOB["cclip_iters"].default, cclip_tau=KNOB["cclip_tau"].default, **_) -> AggResult:
    """Centred clipping (Karimireddy, He & Jaggi, ICML 2021; one iteration = norm bounding, Sun et al. 2019; beyond the
    reference, rule text in docs/PARITY.md): from v = ``centre`` (the global model the round started from; the
    alpha-weighted mean of the rows when None), ``cclip_iters`` times v <- v + sum_i alpha_i s_i (x_i - v) with
    s_i = min(1, tau / ||x_i - v||), alpha = sizes / sum sizes.  ``cclip_tau``: a radius > 0 or ``"auto"``, the lower
    median of the first iteration's distances.  Run in Gram space (``k_cclip_weights`` on the Gram about the centre,
    ``afl_gram_anchored``): the rows are read by the Gram pass and by the final row pass only.  No host read.  With a
    centre a non-finite row is left out (its alpha not redistributed) and the result is the centre when no row is
    finite; without one it makes the result non-finite, as FedAvg's is.  Always a new tensor."""
    n = U.shape[0]
    iters, tau = (KNOB[k].check(v, coerce=True) for k, v in (("cclip_iters", cclip_iters), ("cclip_tau", cclip_tau)))
    a = _device_weights(sizes, U.device, n)
    alpha = a / a.sum()
    if centre is None:
        c, t, clipped, _ = ops.cclip_weights(ops.centred_gram(U), alpha, alpha, iters, tau)
        out = ops.weighted_rows(U, c)
    else:
        g = centre.to(device=U.device, dtype=torch.float32)
        c, t, clipped, _ = ops.cclip_weights(ops.gram_anchored(U, g), alpha, torch.zeros_like(alpha), iters, tau)
        out = ops.anchored_rows(U, c, g)
    return AggResult(out, True, {"weights": c, "tau": t, "clipped": clipped, "iters": iters})


def foolsgold(U: torch.Tensor, sizes=None, centre: Optional[torch.Tensor] = None,
              history: Optional[torch.Tensor] = None, kappa=FOOLSGOLD_KAPPA.default,
              enable: Optional[torch.Tensor] = None, rounds=0, out: Optional[torch.Tensor] = None) -> AggResult:
    """FoolsGold (Fung, Yoon & Beschastnikh, RAID 2020; beyond the reference, rule text in docs/PARITY.md), the rule
    with memory: ``history`` H [n, P] fp32 (None: zeros) holds every row's accumulated updates, H_i <- H_i + (x_i - g)
    about ``centre`` g, the global model the round started from; the cosines of the NEW histories give every row a
    weight alpha_i in [0, 1] (``kappa``: the logit's scale) and the result is g + sum_j alpha0_j alpha_j (x_j - g),
    alpha0 = sizes / sum sizes.  Four launches on the device for n <= 64 (``k_hist_gram``, ``k_gram_reduce``,
    ``k_foolsgold_weights``, ``k_anchored_rows``), no host read.  ``enable`` (one int32 on the device, None = 1): with 0
    the new history has the bits of the old one (the caller keeps the old model: a failed round never reaches the
    history).  ``out``: the buffer the new history goes to (never ``history``).  ``rounds``: the successful rounds
    accumulated so far.  info = {alpha, max_cos, rounds (a 0-d int64 tensor), history (the new H)}.  Without a centre
    the result is FedAvg, the history is returned untouched and alpha is all ones.  Always a new tensor."""
    n = U.shape[0]
    kappa = FOOLSGOLD_KAPPA.check(kappa, coerce=True)
    rounds = torch.as_tensor(rounds, dtype=torch.int64).to(U.device)
    H = torch.zeros_like(U, dtype=torch.float32) if history is None else history
    if tuple(H.shape) != tuple(U.shape):
        raise ValueError(f"foolsgold: history {tuple(H.shape)} does not match the rows {tuple(U.shape)}")
    a = _device_weights(sizes, U.device, n)
    if centre is None:
        one = torch.ones(n, dtype=torch.float64, device=U.device)
        return AggResult(ops.fedavg(U, a if sizes is None else sizes), True, {"alpha": one, "max_cos": torch.zeros_like(one), "rounds": rounds,
                                                  "history": H})
    g = centre.to(device=U.device, dtype=torch.float32)
    Hn, G = ops.hist_gram(U, g, H, enable, out=out)
    alpha, v, c = ops.foolsgold_weights(G, a / a.sum(), kappa)
    done = 1 if enable is None else (enable.to(U.device).reshape(()) != 0).to(torch.int64)
    return AggResult(ops.anchored_rows(U, c, g), True, {"alpha": alpha, "max_cos": v, "rounds": rounds + done,
                                                         "history": Hn})


def dnc(U: torch.Tensor, sizes=None, byz_f=KNOB["byz_f"].default, dnc_iters: int = KNOB["dnc_iters"].default,
        dnc_sub_dim: int = KNOB["dnc_sub_dim"].default, dnc_c: float = KNOB["dnc_c"].default, seed: int = 0,
        **_) -> AggResult:
    """Divide-and-Conquer (Shejwalkar & Houmansadr, NDSS 2021; beyond the reference, rule text in docs/PARITY.md):
    ``dnc_iters`` times, the Gram of the rows on ``dnc_sub_dim`` keyed random columns (all of them in natural order
    when that is >= P), scores lambda_1 u_i^2 from its top eigenpair, the drop = min(ceil(c f), n - 1) rows with the
    largest (score, index) dropped; the size-weighted mean of the rows kept in every iteration (of all rows when none
    is).  Device, n <= 64: three launches for any ``dnc_iters`` (``k_dnc_gram``, ``k_dnc_select``, ``weighted_rows``);
    no host read.  drop = 0 is FedAvg itself."""
    n = U.shape[0]
    f = byzantine_count(n, byz_f, 2, "dnc")
    iters, b, c = (KNOB[k].check(v, coerce=True)
                   for k, v in (("dnc_iters", dnc_iters), ("dnc_sub_dim", dnc_sub_dim), ("dnc_c", dnc_c)))
    drop = min(math.ceil(c * f), n - 1)
    s = _device_weights(sizes, U.device, n)
    keep, scores, w = ops.dnc_filter(U, b, iters, seed, drop, s)
    out = ops.fedavg(U, s) if drop == 0 else ops.weighted_rows(U, w)
    return AggResult(out, True, {"selected": keep, "f": f, "drop": drop, "scores": scores})


def signguard(U: torch.Tensor, sizes=None, centre: Optional[torch.Tensor] = None, seed: int = 0,
              signguard_frac=SIGNGUARD_FRAC.default, signguard_lo=SIGNGUARD_LO.default,
              signguard_hi=SIGNGUARD_HI.default, **_) -> AggResult:
    """SignGuard (Xu, Huang, Qu & Song, ICDCS 2022; beyond the reference, rule text in docs/PARITY.md) about ``centre``
    g, the global model the round started from: a row passes when its norm ||x_i - g|| lies in [lo M, hi M], M the
    lower median norm, and when it falls into the largest mean-shift cluster of the rows' sign statistics (the shares of
    positive, zero and negative differences on a window of ceil(frac P) contiguous columns placed by ``seed``); the
    result is g + sum_i c_i (x_i - g) over the kept rows with c_i = alpha_i min(1, M / norm_i) / sum_kept alpha,
    alpha = sizes / sum sizes, and g itself when no row is kept.  Device, n <= 64: three launches (``k_sign_stats``,
    ``k_signguard_select``, ``k_anchored_rows``), no host read.  Without a centre the result is FedAvg, every row kept.
    info = {kept, norm_ok, cluster, scores (the features [n, 3]), weights, median_norm, bandwidth, window [s, b]}.
    Always a new tensor."""
    n, P = U.shape
    frac, lo, hi = (k.check(v, coerce=True) for k, v in ((SIGNGUARD_FRAC, signguard_frac), (SIGNGUARD_LO, signguard_lo),
                                                         (SIGNGUARD_HI, signguard_hi)))
    if lo > hi:
        raise ValueError(f"signguard: signguard-lo must be <= signguard-hi (got {lo}, {hi})")
    a = _device_weights(sizes, U.device, n)
    alpha = a / a.sum()
    if centre is None:
        s, b = ops.signguard_window(P, frac, seed)
        one = torch.ones(n, dtype=torch.bool, device=U.device)
        zero = torch.zeros((), dtype=torch.float64, device=U.device)
        return AggResult(ops.fedavg(U, a if sizes is None else sizes), True,
                         {"kept": one, "norm_ok": one.clone(), "cluster": torch.zeros(n, dtype=torch.int64, device=U.device),
                          "scores": torch.zeros(n, 3, dtype=torch.float64, device=U.device), "weights": alpha,
                          "median_norm": zero, "bandwidth": zero.clone(), "window": [s, b]})
    g = centre.to(device=U.device, dtype=torch.float32)
    keep, ok, label, F, c, M, h, (s, b) = ops.signguard_filter(U, g, frac, seed, alpha, lo, hi)
    return AggResult(ops.anchored_rows(U, c, g), True,
                     {"kept": keep, "norm_ok": ok, "cluster": label, "scores": F, "weights": c, "median_norm": M,
                      "bandwidth": h, "window": [s, b]})


def flame(U: torch.Tensor, sizes=None, centre: Optional[torch.Tensor] = None, seed: int = 0,
          flame_noise=FLAME_NOISE.default, **_) -> AggResult:
    """FLAME (Nguyen et al., USENIX Security 2022; beyond the reference, rule text in docs/PARITY.md) about ``centre``
    g, the global model the round started from: the rows kept are the majority cluster of the updates' cosine
    distances (the first connected component of >= n' // 2 + 1 of the n' finite rows as the distance threshold grows:
    HDBSCAN with min_cluster_size = n // 2 + 1, min_samples = 1, allow_single_cluster), each clipped to the lower
    median S of all finite rows' norms, c_i = alpha_i min(1, S / ||x_i - g||) / sum_kept alpha, alpha = sizes / sum
    sizes, and the result is g + sum_i c_i (x_i - g) + sigma z with sigma = ``flame_noise`` S and z the Philox normals
    keyed by ``seed`` (``flame_noise`` 0: no noise); g itself when no row is finite.  Device, n <= 64: four launches
    (``k_gram_f64``, ``k_gram_reduce``, ``k_flame_select``, ``k_flame_rows``), no host read.  Without a centre the
    result is FedAvg, every row kept, no noise.  info = {kept, weights, median_norm, sigma, threshold, majority}.
    Always a new tensor."""
    n = U.shape[0]
    lam = FLAME_NOISE.check(flame_noise, coerce=True)
    a = _device_weights(sizes, U.device, n)
    alpha = a / a.sum()
    if centre is None:
        zero = torch.zeros((), dtype=torch.float64, device=U.device)
        return AggResult(ops.fedavg(U, a if sizes is None else sizes), True,
                         {"kept": torch.ones(n, dtype=torch.bool, device=U.device), "weights": alpha,
                          "median_norm": zero, "sigma": zero.clone(), "threshold": zero.clone(),
                          "majority": torch.full((), n // 2 + 1, dtype=torch.int64, device=U.device)})
    g = centre.to(device=U.device, dtype=torch.float32)
    keep, c, info = ops.flame_filter(U, g, alpha, lam)
    return AggResult(ops.flame_rows(U, c, g, info[1:2], seed), True,
                     {"kept": keep, "weights": c, "median_norm": info[0], "sigma": info[1], "threshold": info[2],
                      "majority": info[3].to(torch.int64)})


def shieldfl(U: torch.Tensor, sizes=None, **_) -> AggResult:
    norms = ops.row_norms(U).to(U.device)
    Un = U / (norms.to(U.dtype)[:, None] + 1e-8)
    ref = mean_of(Un)
    cos = ops.cosine_to(Un, ref, eps=1e-8).float()
    dev = 1.0 - cos
    w = 1.0 / (dev + 1e-6)
    w = w / w.sum()
    return AggResult(ops.weighted_rows(U, w.double()), True, {"weights": w, "cos": cos})


def gmm(U: torch.Tensor, sizes=None, attackers: Optional[torch.Tensor] = None, seed: int = 0,
        gmm_rank: Optional[int] = None, **_) -> AggResult:
    """GMM gradient filter (reference server.py:352-370; its full-covariance fit on raw P-dim updates crashes, A-8):
    a 2-component GMM on the updates' leading PCA scores, deterministic (``ops.gmm_filter``: one fused launch on
    the device, its mirror on the host).  The mean of the kept rows; the round fails when no row is kept (reference
    ``round_result = False``).  Device, n <= 64: no host read, ``ok`` is a 0-d device bool (and ``params`` the mean
    of all rows when none is kept) — the caller reads it where it waits anyway; ``attackers`` on the host or the
    device.  ``gmm_rank``: the PCA rank (engine ``gmm-rank``; None / 0 = max(1, min(4, n // 2 - 1)))."""
    n = U.shape[0]
    att = attackers if attackers is not None else torch.zeros(n, dtype=torch.bool)
    keep, inf = ops.gmm_filter(ops.centred_gram(U), att, int(gmm_rank or 0))
    if U.is_cuda and n <= 64:
        return AggResult(_masked_mean(U, keep), inf[1] > 0, {"kept": keep, "threshold": inf[0]})
    # the host form keeps the sum over the kept rows only: in fp32 it differs from the masked sum in the last bit
    idx = torch.nonzero(keep).reshape(-1)
    if not idx.numel():
        return AggResult(None, False, {"kept": []})
    return AggResult(mean_of(U[idx]), True, {"kept": idx.tolist(), "threshold": float(inf[0])})


def scionfl(U: torch.Tensor, sizes: torch.Tensor, seed: int = 0, **_) -> AggResult:
    """All on the device: quantisation, L2-from-counts, the 3x-mean clip, the cosine-distance threshold
    (the int(0.5 n)-th largest score) and the size-weighted FedAvg of the kept originals."""
    n = U.shape[0]
    sigma, smin, smax = ops.stochastic_quantize(U, seed)
    smin = smin.double()
    smax = smax.double()
    ones = sigma.double().sum(dim=1)
    zeros = U.shape[1] - ones
    l2 = torch.sqrt(zeros * smin ** 2 + ones * smax ** 2)
    MU, TOPK = 3.0, 0.5
    lim = MU * l2.mean()
    fac = torch.where(l2 > lim, lim / l2, torch.ones_like(l2))
    smin = smin * fac
    smax = smax * fac
    deq = smin.to(U.dtype)[:, None] + sigma * (smax - smin).to(U.dtype)[:, None]
    agg = mean_of(deq)
    cosd = 1.0 - ops.cosine_to(deq, agg, eps=1e-8).double()
    thr = torch.sort(cosd, descending=True).values[int(TOPK * n)] if n > 0 else torch.zeros((), device=U.device)
    keep = cosd > thr
    # (no client kept: the reference would crash; all clients are averaged instead)
    out = _masked_mean(U, keep, _device_weights(sizes, U.device))
    return AggResult(out, True, {"kept": keep, "scores": cosd, "threshold": thr})


def _median(x: torch.Tensor) -> torch.Tensor:
    """np.median: the mean of the two middle values for an even count."""
    s = torch.sort(x).values
    n = s.shape[0]
    return 0.5 * (s[(n - 1) // 2] + s[n // 2])


_centred_gram = ops.centred_gram  # (the name tools and tests know)


def _top_pc_scores(U: torch.Tensor, sweeps: int = 12) -> torch.Tensor:
    """First principal-component scores of the rows (sklearn ``PCA(1).fit_transform`` up to the sign) with no
    host synchronisation: the leading eigenpair of the n x n Gram of the centred rows (``ops.top_pc``),
    score = v sqrt(lambda).  Exact for any spectrum gap (repeated squaring, the round-4 form, let the second
    eigenvector leak in when the top two eigenvalues are close)."""
    return ops.top_pc(ops.centred_gram(U), sweeps)


def fltracer(U: torch.Tensor, sizes: torch.Tensor, threshold: float = 2.5, **_) -> AggResult:
    """FLTracer anomaly filter (reference ``fltracer_detect_anomalies``, src/Utils.py:363-369): robust z-score
    |z - median| / (1.4826 MAD + 1e-6) of the first-PC scores, rows above ``threshold`` dropped, size-weighted
    FedAvg of the rest (every row when all are flagged).  All on the device."""
    z = _top_pc_scores(U)
    med = _median(z)
    mad = _median((z - med).abs())
    scores = (z - med).abs() / (1.4826 * mad + 1e-6)
    bad = scores > threshold
    out = _masked_mean(U, ~bad, _device_weights(sizes, U.device))
    return AggResult(out, True, {"anomalies": bad, "scores": scores})


def byzantine(U: torch.Tensor, sizes=None, threshold: float = 0.9, **_) -> AggResult:
    """Cosine >= 0.9 to model 0, mean of the kept rows (all rows when none passes), on the device."""
    keep = ops.cosine_to(U, U[0], eps=1e-8) >= threshold
    return AggResult(_masked_mean(U, keep), True, {"kept": keep})


# ---------------------------------------------------------------------------------- pre-aggregation
# In front of a robust rule (engine ``pre-agg``; rule text in docs/PARITY.md): (U, sizes) -> (Y, sizes', info), the
# rule then runs on (Y, sizes') with its usual keywords.  Both are one row mix Y = W U (``ops.mix_rows``: one pass
# over U on the device); neither reads a device value back; ``U`` stays read-only.
def nnm(U: torch.Tensor, sizes=None, byz_f=KNOB["byz_f"].default):
    """Nearest-neighbour mixing (Allouah et al., AISTATS 2023): every row becomes the unweighted mean of its n - f
    nearest rows by (squared distance, index), itself included; f as Multi-Krum takes it (``byz-f``, n >= 2 f + 3).
    ``sizes`` passes through.  Device, n <= 64: the Gram-form distances, ``k_nnm_weights``, ``k_mix_rows``.  f = 0
    gives n copies of the mean, by the same three steps."""
    n = U.shape[0]
    f = byzantine_count(n, byz_f, 2, "nnm")
    W, _ = ops.nnm_weights(ops.pairwise_sqdist(U), f)
    return ops.mix_rows(W, U), sizes, {"kind": "nnm", "f": f, "weights": W, "rows": n}


def bucketing(U: torch.Tensor, sizes=None, bucket_size=BUCKET_SIZE.default, seed: int = 0):
    """Bucketing (Karimireddy, He & Jaggi, ICLR 2022): the rows shuffled by the permutation of (seed, n) and averaged,
    size-weighted, in buckets of ``bucket_size`` (the last one may be short) -> the R = ceil(n / bucket_size) bucket
    means and the buckets' size sums (in ``sizes``' dtype, where it lives; fp64 counts when it is None).
    ``bucket_size`` 1 returns ``U`` and ``sizes`` themselves."""
    n = U.shape[0]
    s = BUCKET_SIZE.check(bucket_size)
    if s == 1:
        return U, sizes, {"kind": "bucketing", "bucket_size": 1, "rows": n,
                          "weights": torch.eye(n, dtype=torch.float64, device=U.device)}
    W, tot = ops.composite.bucket_weights(sizes, n, s, seed)
    return (ops.mix_rows(W, U), tot if sizes is None else tot.to(sizes.dtype),
            {"kind": "bucketing", "bucket_size": s, "weights": W, "rows": int(W.shape[0])})


def pre_aggregate(kind: str, U: torch.Tensor, sizes=None, byz_f=KNOB["byz_f"].default,
                  bucket_size=BUCKET_SIZE.default, seed: int = 0, **_):
    """``nnm`` or ``bucketing`` by name, each taking its own keywords -> (Y, sizes', info)."""
    if kind == "nnm":
        return nnm(U, sizes, byz_f)
    if kind == "bucketing":
        return bucketing(U, sizes, bucket_size, seed)
    raise ValueError(f"pre-aggregation '{kind}' is not valid (choose from {PRE_AGG_KINDS[1:]}).")


# Contract of every aggregator: ``U`` is READ-ONLY and may be the live client-model rows (single rank: the
# engine hands ``local_params`` itself, ``Launch.plain``) — never write it in place; a returned tensor may
# alias one of its rows (Krum), which the engine clones before the next launch overwrites the rows.
AGGREGATORS = {
    "fedavg": fedavg,
    "trimmed_mean": trimmed_mean,
    "median": median,
    "krum": krum,
    "multi_krum": multi_krum,
    "bulyan": bulyan,
    "geomed": geomed,
    "dnc": dnc,
    "cclip": cclip,
    "signguard": signguard,
    "flame": flame,
    "shieldfl": shieldfl,
    "gmm": gmm,
    "scionfl": scionfl,
    "fltracer": fltracer,
    "byzantine": byzantine,
}
