"""fp64 references of the client-batched layer ops (``csrc/kernels/layers.hip``), their error bounds, and the inputs
at which the kernels are tested.

Every ``ref_*`` is plain torch in float64 and returns, per output, a pair ``(value, tol)``.  ``tol`` is elementwise
and never looks at the output under test: it is ``n_ops * 2^-23 * companion`` where ``companion`` is the same formula
evaluated on absolute values (the size of the terms that were rounded), plus first-order propagation of the
errors of the inputs of a later stage and the measured budgets ``T`` of the device's transcendental functions.  The
derivations and the measured figures are in ``docs/LAYER_TEST_BOUNDS.md``.

``cases_*`` build the inputs (edge shapes, strides, saturated values), ``run_*`` runs an op of
``attackfl_amd.ops.layers`` on them — the fp32 composite for ``dev="cpu"``, the HIP kernel for a GPU — so this
file's CPU tests and ``tests/test_gpu_layer_edges.py`` (``import test_layer_oracles as R``) hold the composite and
the kernels to the same references at the same inputs.

CPU tests here: every reference agrees with the composite within its bound at every input set, and a list of
deliberately wrong variants each FAILS its bound."""
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from attackfl_amd.ops import layers as Lx
from attackfl_amd.ops import masks

U = 2.0 ** -23      # one fp32 rounding (covers truncation as well as round-to-nearest)
TINY = 2.0 ** -126  # results below the smallest normal fp32 may be flushed to zero
INF = float("inf")
# transcendental budgets in units of U * |f(x)|: next power of two at or above twice the worst error measured on
# the device against float64 over the tests' input ranges (docs/LAYER_TEST_BOUNDS.md); none may exceed 64
T = {"erf": 2, "tanh": 4, "exp": 2, "log": 4, "log1p": 2, "pow": 2, "rsqrt": 2}
assert max(T.values()) <= 64
SEEDS = [7 + 3 * c for c in range(130)]


def f32(x):
    return float(np.float32(x))


def gen(*k):
    return torch.Generator().manual_seed(hash(tuple(int(x) for x in k)) % (2 ** 31))


def randn(g, *shape):
    return torch.randn(*shape, generator=g)


def ratio(got, ref, tol):
    """Worst ``|got - ref| / tol`` over EVERY element.  NaN / infinity must sit in the same places; where ``tol`` is
    zero the values must be equal.  inf when any of that is violated."""
    got, ref = got.detach().double().cpu(), ref.double()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(ref)
    if got.shape != ref.shape:
        return INF
    if ref.numel() == 0:
        return 0.0
    nf = ~torch.isfinite(ref)
    if not bool(torch.where(torch.isnan(ref), torch.isnan(got), got == ref)[nf].all()):
        return INF
    e, t = (got - ref).abs()[~nf], tol[~nf]
    if e.numel() == 0:
        return 0.0
    r = torch.where(e == 0, torch.zeros_like(e), e / t)
    return float(torch.nan_to_num(r, nan=INF, posinf=INF).max())


OPTIONAL = {"g_zeroed"}  # outputs only the device path has


def worst(out, ref, what=""):
    """{name: ratio} of a run's outputs against a reference's; prints the figures.  ``*_int`` references are integer
    tensors the output of that name must equal."""
    res = {}
    for k in ref:
        if k.endswith("_int"):
            assert torch.equal(out[k[:-4]], ref[k]), f"{what}: {k[:-4]} {out[k[:-4]].tolist()} != {ref[k].tolist()}"
        elif k in out or k not in OPTIONAL:
            res[k] = ratio(out[k], *ref[k])
    print(f"{what}: " + " ".join(f"{k}={v:.3g}" for k, v in res.items()))
    return res


def check(out, ref, what=""):
    res = worst(out, ref, what)
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, f"{what}: err/bound {bad}"
    return max(res.values()) if res else 0.0


# ------------------------------------------------------------------------------------------ placement helpers
def place(t, dev, layout="k", unaligned=False, off=1, stride=None, fill=7.0):
    """Logical ``[C, R, W]`` values as a device view.  layout 'm': stored transposed (the view's last index is the
    strided one).  unaligned: a view ``off`` floats into a flat arena with row stride 67 (or the next stride = 3
    mod 4 that fits) — rows not 16-byte aligned; the arena's other entries hold ``fill``."""
    s = t if layout == "k" else t.transpose(1, 2)
    C, R, W = s.shape
    if not unaligned:
        v = s.contiguous().to(dev)
    else:
        st = stride or (67 if W <= 66 else (W + 4) // 4 * 4 + 3)
        width = (off + R * st + 3) // 4 * 4
        arena = torch.full((C, width), fill, device=dev)
        v = arena.as_strided((C, R, W), (width, st, 1), off)
        v.copy_(s)
    return v if layout == "k" else v.transpose(1, 2)


def make_ctl(C, dev, step=0, min_bs=2, nan_abort=True):
    ctl = Lx.StepCtl.create(SEEDS[:C], "cpu", min_bs=min_bs, nan_abort=nan_abort)
    ctl.stepctl[0] = step
    return Lx.StepCtl(ctl.seeds.to(dev), ctl.stepctl.to(dev))


def drop_scale(C, step, layer, nrows, ncols, p, col0=0):
    """float64 ``[C, nrows, ncols]`` multipliers ``keep * fp32(1 / (1 - p))`` of site (layer, row, col0 + col)."""
    if p <= 0.0:
        return None
    r, c = np.arange(nrows)[:, None], np.arange(ncols)[None, :] + col0
    inv = f32(1.0 / (1.0 - p))
    return torch.stack([masks.keep(masks.step_key(SEEDS[ci] & masks.M32, step), layer, r, c, p).double() * inv
                        for ci in range(C)])


# ================================================================================================== GEMM
def bf16_rne(x):
    return x.bfloat16().double()


def bf16_trunc(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32).double()


def ref_act(z, tz, act):
    if act == 1:
        return torch.where(z < 0, torch.zeros_like(z), z), tz  # Lipschitz 1, NaN kept
    if act == 2:
        e = torch.erf(z * math.sqrt(0.5))
        # Lipschitz constant of gelu <= 1.13; evaluation: erff budget and 4 roundings on 0.5 |z| (1 + |erf|)
        return 0.5 * z * (1 + e), 1.13 * tz + (T["erf"] + 4) * U * 0.5 * z.abs() * (1 + e.abs())
    return z, tz


def ref_actd(G, gact):
    """act'(G) and its evaluation error."""
    G = G.double()
    if gact == 1:
        return (G > 0).double(), torch.zeros_like(G)
    if gact == 2:
        e = torch.erf(G * math.sqrt(0.5))
        cdf = 0.5 * (1 + e)
        tail = G * 0.3989422804014327 * torch.exp(-0.5 * G * G)
        # fast exponential of x = g^2 / 2: (2 + x) U relative, its argument carries 2 roundings (x 2U more)
        return cdf + tail, (T["erf"] + 3) * U * 0.5 * (1 + e.abs()) + tail.abs() * (6 + 1.5 * G * G) * U
    return torch.ones_like(G), torch.zeros_like(G)


def gemm_case(C, M, N, K, la="k", lb="k", ua=False, ub=False, cs=1, bias=True, Z=True, act=0, p=0.0, gact=0, gs=1,
              accum=0, alpha=1.0, splitk=1, nan_row=None, asum=False, generic=True, step=0, layer=5, a_off=1,
              a_stride=None, seed=0):
    g = gen(C, M, N, K, seed, 11)
    c = NS(C=C, M=M, N=N, K=K, la=la, lb=lb, ua=ua, ub=ub, cs=cs, act=act, p=p, gact=gact, gs=gs, accum=accum,
           alpha=alpha, splitk=splitk, asum=asum, generic=generic, step=step, layer=layer, a_off=a_off,
           a_stride=a_stride, has_Z=Z)
    c.A, c.B = randn(g, C, M, K), randn(g, C, N, K) * 0.5
    if nan_row is not None:
        c.A[:, nan_row, :] = float("nan")
    c.bias = randn(g, C, N) if bias else None
    Gm = randn(g, C, M, N)
    Gm = torch.where(Gm.abs() < 2.0 ** -6, torch.full_like(Gm, 2.0 ** -6), Gm)  # |G| >= 2^-6 ...
    Gm[torch.rand(C, M, N, generator=g) < 0.05] = 0.0                            # ... or exactly 0: relu' is 0 there
    c.G = Gm if gact else None
    c.fillC, c.fillZ = randn(g, C, M, N * cs), randn(g, C, M, N * cs)
    c.id = (f"C{C} M{M} N{N} K{K} A{la}{'u' if ua else 'a'} B{lb}{'u' if ub else 'a'} cs{cs} act{act} p{p} "
            f"g{gact} acc{accum} al{alpha} sk{splitk}" + (" asum" if asum else "") + ("" if generic else " ts"))
    return c


def run_gemm(c, dev, one=False):
    C = 1 if one else c.C
    A, B = c.A[:C], c.B[:C]
    if str(dev) == "cpu":  # the composite does not round its operands: feed it the rounded ones
        A, B = A.bfloat16().float(), B.bfloat16().float()
    Ad = place(A, dev, c.la, c.ua, off=c.a_off, stride=c.a_stride)
    Bd = place(B, dev, c.lb, c.ub)
    bufC, bufZ = c.fillC[:C].clone().to(dev), c.fillZ[:C].clone().to(dev)
    Cm, Zm = bufC[:, :, ::c.cs], bufZ[:, :, ::c.cs]
    Gd = None
    if c.G is not None:
        Gd = c.G[:C].to(dev) if c.gs == 1 else c.G[:C].repeat_interleave(c.gs, dim=2).to(dev)[:, :, ::c.gs]
    asum = torch.ones(C, c.K, device=dev) if c.asum else None
    if c.asum and str(dev) == "cpu":  # the column sums are of the unrounded A
        asum.add_(c.A[:C].sum(1))
    Lx.bgemm(Ad, Bd, Cm, bias=None if c.bias is None else c.bias[:C].to(dev), Z=Zm if c.has_Z else None, G=Gd,
             act=c.act, gact=c.gact, accum=c.accum, splitk=c.splitk, alpha=c.alpha, ctl=make_ctl(C, dev, c.step),
             layer=c.layer, p=c.p, generic=c.generic, asum=None if str(dev) == "cpu" else asum)
    out = {"C": Cm.cpu(), "bufC": bufC.cpu()}
    if c.has_Z:
        out["Z"], out["bufZ"] = Zm.cpu(), bufZ.cpu()
    if c.asum:
        out["asum"] = asum.cpu()
    return out


def ref_gemm(c, one=False, rnd=bf16_rne):
    C = 1 if one else c.C
    A, B = rnd(c.A[:C]), rnd(c.B[:C])
    al = f32(c.alpha)
    z = al * torch.bmm(A, B.transpose(1, 2))
    zc = abs(al) * torch.bmm(A.abs(), B.abs().transpose(1, 2))
    if c.bias is not None:
        z = z + c.bias[:C].double()[:, None, :]
        zc = zc + c.bias[:C].double().abs()[:, None, :]
    kchunk = ((c.K + c.splitk - 1) // c.splitk + 31) // 32 * 32
    nsplit = (c.K + kchunk - 1) // kchunk
    # bf16 x bf16 products are exact in fp32: K additions in any order, + 8 for alpha and the bias
    tz = (c.K + 8) * U * zc
    v, tv = ref_act(z, tz, c.act)
    sc = drop_scale(C, c.step, c.layer, c.M, c.N, c.p)
    if sc is not None:
        v = v * sc
        tv = tv * sc + 2 * U * v.abs()
    if c.G is not None:
        d, td = ref_actd(c.G[:C], c.gact)
        tv = tv * d.abs() + v.abs() * td + U * (v * d).abs()
        v = v * d
    fillC, fillZ = c.fillC[:C].double(), c.fillZ[:C].double()
    bufC, bufZ = fillC.clone(), fillZ.clone()
    if c.accum:
        c0 = fillC[:, :, ::c.cs]
        tv = tv + (nsplit + 1) * U * (c0.abs() + (zc if c.splitk > 1 else v.abs()))
        v = c0 + v
    res = {"C": (v, tv)}
    bufC[:, :, ::c.cs] = v
    bt = torch.zeros_like(bufC)  # the entries between the output's columns keep their prefill
    bt[:, :, ::c.cs] = tv
    res["bufC"] = (bufC, bt)
    if c.has_Z:
        res["Z"] = (z, tz)
        bufZ[:, :, ::c.cs] = z
        bz = torch.zeros_like(bufZ)
        bz[:, :, ::c.cs] = tz
        res["bufZ"] = (bufZ, bz)
    if c.asum:
        Ad = c.A[:C].double()
        res["asum"] = (1 + Ad.sum(1), (c.M + 8) * U * (1 + Ad.abs().sum(1)))
    return res


GEMM_M, GEMM_N, GEMM_K = [1, 63, 64, 65, 130], [1, 63, 64, 65], [1, 7, 8, 9, 31, 32, 33, 65]
LAYOUTS = [(la, lb, ua, ub) for la in "km" for lb in "km" for ua, ub in ((False, False), (True, True))]
# (bias, Z, act, p, gact, accum, alpha)
EPILOGUES = [(True, True, 0, 0.0, 0, 0, 1.0), (True, True, 1, 0.3, 0, 0, 0.125), (True, True, 2, 0.0, 0, 1, 0.3),
             (True, False, 2, 0.3, 1, 0, 1.0), (False, True, 0, 0.0, 2, 1, 0.3), (True, True, 1, 0.0, 2, 1, 0.125),
             (True, True, 0, 0.3, 1, 0, 0.3), (False, False, 0, 0.0, 0, 0, 1.0), (True, True, 2, 0.3, 2, 1, 1.0),
             (True, True, 1, 0.3, 1, 1, 1.0), (True, True, 0, 0.3, 0, 1, 0.125)]


def cases_bgemm_shapes():
    """The cross product of tile-edge shapes; layouts, alignment, output stride and epilogues cycle over it (each of
    the 8 x 11 layout / epilogue pairs occurs: 160 shapes, periods 8 and 11 coprime)."""
    i = 0
    for M in GEMM_M:
        for N in GEMM_N:
            for K in GEMM_K:
                la, lb, ua, ub = LAYOUTS[i % len(LAYOUTS)]
                bias, Z, act, p, gact, accum, alpha = EPILOGUES[i % len(EPILOGUES)]
                yield gemm_case(2, M, N, K, la, lb, ua, ub, cs=2 if i % 3 == 0 else 1, bias=bias, Z=Z, act=act, p=p,
                                gact=gact, accum=accum, alpha=alpha, step=i % 3, seed=i)
                i += 1


def cases_bgemm_layouts():
    """Every operand layout x alignment x epilogue at one shape with partial tiles in M, N and K."""
    i = 0
    for lay in LAYOUTS:
        for epi in EPILOGUES:
            bias, Z, act, p, gact, accum, alpha = epi
            yield gemm_case(2, 65, 66, 41, *lay, cs=1 + i % 2, bias=bias, Z=Z, act=act, p=p, gact=gact, accum=accum,
                            alpha=alpha, seed=1000 + i)
            i += 1


def cases_bgemm_splitk():
    for K, sk in ((40, 2), (33, 6), (3, 8), (2053, 6)):
        for lay in ((("k", "k", False, False), ("m", "m", False, False)) if K != 2053 else (("m", "m", False, False),)):
            yield gemm_case(2, 65, 33, K, *lay, bias=False, Z=False, accum=2, splitk=sk, seed=K)


def cases_bgemm_nan():
    yield gemm_case(2, 65, 33, 40, nan_row=64, act=1, p=0.3, gact=1, accum=1, seed=5)
    yield gemm_case(2, 130, 65, 9, "m", "k", nan_row=3, act=2, gact=2, seed=6)


TS_SHAPES = [(64, 64), (128, 64), (192, 64), (256, 64), (64, 128), (64, 192), (64, 256)]
TS_EPI = dict(bias=True, Z=True, act=1, p=0.1, gact=1, accum=1, layer=4, generic=False)


def cases_tsgemm():
    for N, K in TS_SHAPES:
        for lb in "km":
            for M in (1, 15, 16, 17, 1007):
                yield gemm_case(3, M, N, K, lb=lb, asum=True, seed=M + N, **TS_EPI)


def cases_tsgemm_tiles():
    """More than one row tile per wave: the loop-carried prefetch (K = 64) and the last, partial tile."""
    for N, K in ((64, 64), (64, 256)):
        yield gemm_case(64, 2071, N, K, seed=77, **TS_EPI)


def cases_tsgemm_colsums():
    """Fused ordered column sums over several tiles per wave (TS_ASUM_PARTS = 128 blocks per client)."""
    for N, K in ((64, 64), (64, 256)):
        yield gemm_case(2, 24581, N, K, asum=True, seed=78, bias=True, Z=False, act=1, generic=False)
    yield gemm_case(2, 1007, 256, 64, asum=True, seed=79, **TS_EPI)  # N = 256: the separate column-sum pass


def cases_tsgemm_fallback():
    """Each k_tsgemm precondition false in turn: the launcher must fall back to k_bgemm and still meet the bound."""
    yield gemm_case(2, 100, 64, 64, ua=True, a_off=1, a_stride=68, seed=80, **TS_EPI)   # A base off by one float
    yield gemm_case(2, 100, 64, 64, ua=True, a_off=0, a_stride=67, seed=81, **TS_EPI)   # sAm % 4 != 0
    yield gemm_case(2, 100, 64, 64, gs=2, seed=82, **TS_EPI)                            # G column stride 2
    yield gemm_case(2, 100, 64, 64, cs=2, seed=83, **TS_EPI)                            # output column stride 2


# ================================================================================================== column sums
def cases_colsum():
    for M in (1, 255, 256, 257, 1025):
        for N in (1, 63, 64, 65, 130):
            g = gen(M, N, 21)
            yield NS(C=5, M=M, N=N, Y=randn(g, 5, M, N + 5), out0=randn(g, 5, N), id=f"M{M} N{N}")


def run_colsum(c, dev, one=False):
    C = 1 if one else c.C
    Y = c.Y[:C].to(dev)[:, :, :c.N]  # row stride N + 5
    out = c.out0[:C].clone().to(dev)
    Lx.colsum(Y, out)
    return {"out": out.cpu()}


def ref_colsum(c, one=False):
    C = 1 if one else c.C
    Y, o = c.Y[:C, :, :c.N].double(), c.out0[:C].double()
    return {"out": (o + Y.sum(1), (c.M + 8) * U * (o.abs() + Y.abs().sum(1)))}


# ================================================================================================== gathers
def cases_gather():
    for step in (0, 2):
        for mask in (False, True):
            g = gen(step, mask, 31)
            C, B, S, NR = 3, 5, 3, 40  # C * B * 24 = 360: not a multiple of 256
            rows = randn(g, NR, 24)
            rows[torch.rand(NR, 24, generator=g) < 0.2] = -2.0
            rows[::3, 23] = -2.0  # the label column must survive the mask
            idx = torch.randint(0, NR, (S, C, B), generator=g, dtype=torch.int32)
            idx[:, 1, 3:] = -1
            idx[:, 2, :] = -1
            yield NS(kind="icu", C=C, B=B, rows=rows, idx=idx, step=step, mask=mask, id=f"icu step{step} mask{mask}")
    for F_ in (1, 561):
        for step in (0, 2):
            g = gen(F_, step, 32)
            C, B, S, NR = 3, 5, 3, 40
            idx = torch.randint(0, NR, (S, C, B), generator=g, dtype=torch.int32)
            idx[:, 0, 4] = -1
            idx[:, 2, 1:] = -1
            yield NS(kind="har", C=C, B=B, F=F_, x=randn(g, NR, F_), idx=idx, step=step,
                     y=torch.randint(-2 ** 40, 2 ** 40, (NR,), generator=g, dtype=torch.int64),
                     id=f"har F{F_} step{step}")


def run_gather(c, dev):
    ctl = make_ctl(c.C, dev, c.step)
    if c.kind == "icu":
        vit, lab, y = (torch.full((c.C, c.B, w), 9.0, device=dev) for w in (7, 16, 1))
        Lx.gather_icu(c.rows.to(dev), c.idx.to(dev), ctl, c.mask, vit, lab, y)
        return {"vit": vit.cpu(), "lab": lab.cpu(), "y": y.cpu()}
    ox = torch.full((c.C, c.B, c.F), 9.0, device=dev)
    oy = torch.full((c.C, c.B), 9, dtype=torch.int64, device=dev)
    Lx.gather_har(c.x.to(dev), c.y.to(dev), c.idx.to(dev), ctl, ox, oy)
    return {"ox": ox.cpu(), "oy": oy.cpu()}


def ref_gather(c):
    """Exact (tol 0).  int64 labels are compared as integers by the caller (``oy_int``)."""
    ix = c.idx[c.step].long()
    z = torch.zeros(())
    if c.kind == "icu":
        r = torch.stack([torch.stack([c.rows[int(i)] if i >= 0 else torch.zeros(24) for i in row]) for row in ix])
        feat = r[..., :23].clone()
        if c.mask:
            feat[feat == -2.0] = 0.0
        return {"vit": (feat[..., :7].double(), z), "lab": (feat[..., 7:].double(), z), "y": (r[..., 23:].double(), z)}
    ox = torch.stack([torch.stack([c.x[int(i)] if i >= 0 else torch.zeros(c.F) for i in row]) for row in ix])
    oy = torch.tensor([[int(c.y[int(i)]) if i >= 0 else 0 for i in row] for row in ix], dtype=torch.int64)
    return {"ox": (ox.double(), z), "oy_int": oy}


# ================================================================================================== conv patches / pool
CONV_L = [1, 2, 3, 4, 5, 7, 16, 17]


def cases_conv():
    i = 0
    for L in CONV_L:
        for Cin, Ch in ((1, 1), (32, 128)):
            for relu in ("none", "zeros", "nan"):
                g = gen(L, Cin, i, 41)
                C, B = 2, 3
                c = NS(C=C, B=B, L=L, Cin=Cin, Ch=Ch, relu=relu, p=0.3 if i % 2 else 0.0, col0=4 * Ch if i % 3 else 0,
                       step=i % 3, id=f"L{L} Cin{Cin} Ch{Ch} relu-{relu}")
                c.x = randn(g, C, B * L, Cin + 3)  # row stride Cin + 3
                c.dcols = randn(g, C, B * L, 3 * Cin)
                src = randn(g, C, B * L, Cin + 1)
                h = randn(g, C, B * L, Ch)
                for t in (src, h):
                    if relu != "none":
                        t[torch.rand(t.shape, generator=g) < 0.2] = 0.0
                    if relu == "nan":
                        t[torch.rand(t.shape, generator=g) < 0.1] = float("nan")
                c.src, c.h = src, h
                c.W = 4 * Ch + c.col0 + 3
                c.out0, c.dout = randn(g, C, B, c.W), randn(g, C, B, c.W)
                yield c
                i += 1


def run_conv(c, dev):
    C, B, L, Cin, Ch = c.C, c.B, c.L, c.Cin, c.Ch
    x = c.x.to(dev)[:, :, :Cin]
    cols = torch.full((C, B * L, 3 * Cin), 9.0, device=dev)
    Lx.im2col3(x, B, L, cols)
    dx = torch.full((C, B * L, Cin), 9.0, device=dev)
    Lx.col2im3(c.dcols.to(dev), B, L, Cin, None if c.relu == "none" else c.src.to(dev)[:, :, :Cin], dx)
    ctl = make_ctl(C, dev, c.step)
    out = c.out0.clone().to(dev)
    Lx.pool4_fwd(c.h.to(dev), B, L, out, c.col0, ctl, layer=1, p=c.p)
    dh = torch.full((C, B * L, Ch), 9.0, device=dev)
    Lx.pool4_bwd(c.dout.to(dev), c.col0, c.h.to(dev), B, L, dh, ctl, layer=1, p=c.p)
    return {"cols": cols.cpu(), "dx": dx.cpu(), "pool": out.cpu(), "dh": dh.cpu()}


def pool_bins(L, shift=0):
    """AdaptiveAvgPool1d(4) bins [floor(p L / 4), ceil((p + 1) L / 4)); ``shift`` moves the upper edges (mutant)."""
    return [((p * L) // 4, min(L, ((p + 1) * L + 3) // 4 + (shift if p < 3 else 0))) for p in range(4)]


def ref_conv(c, bins_shift=0):
    C, B, L, Cin, Ch = c.C, c.B, c.L, c.Cin, c.Ch
    x = c.x[:, :, :Cin].double().reshape(C, B, L, Cin)
    cols = torch.zeros(C, B, L, Cin, 3, dtype=torch.float64)
    for j in range(3):  # column ci * 3 + j = input position l + j - 1
        lo, hi = max(0, 1 - j), min(L, L + 1 - j)
        cols[:, :, lo:hi, :, j] = x[:, :, lo + j - 1:hi + j - 1, :]
    d = c.dcols.double().reshape(C, B, L, Cin, 3)
    dx, dxa = torch.zeros(C, B, L, Cin, dtype=torch.float64), torch.zeros(C, B, L, Cin, dtype=torch.float64)
    for j in range(3):  # adjoint: input l receives tap j of output l - j + 1
        lo, hi = max(0, 1 - j), min(L, L + 1 - j)
        dx[:, :, lo + j - 1:hi + j - 1] += d[:, :, lo:hi, :, j]
        dxa[:, :, lo + j - 1:hi + j - 1] += d[:, :, lo:hi, :, j].abs()
    dx, dxa = dx.reshape(C, B * L, Cin), dxa.reshape(C, B * L, Cin)
    if c.relu != "none":
        keep = (c.src[:, :, :Cin] > 0).double()  # !(x > 0) zeroes: NaN zeroes too
        dx, dxa = dx * keep, dxa * keep
    h = c.h.double().reshape(C, B, L, Ch)
    bins = pool_bins(L, bins_shift)
    sc = drop_scale(C, c.step, 1, B, 4 * Ch, c.p, c.col0)
    sc = torch.ones(C, B, 4 * Ch, dtype=torch.float64) if sc is None else sc
    nd = 2 if c.p > 0 else 0
    pool, pt = c.out0.double().clone(), torch.zeros(C, B, c.W, dtype=torch.float64)
    dh, dha = torch.zeros_like(h), torch.zeros_like(h)
    dout = c.dout.double()
    for p, (lo, hi) in enumerate(bins):
        col = slice(c.col0 + p, c.col0 + 4 * Ch, 4)
        s = sc[:, :, p::4]
        pool[:, :, col] = h[:, :, lo:hi].sum(2) / (hi - lo) * s
        pt[:, :, col] = (hi - lo + 1 + nd) * U * h[:, :, lo:hi].abs().sum(2) / (hi - lo) * s
        gcol = (dout[:, :, col] / (hi - lo) * s)[:, :, None, :]
        dh[:, :, lo:hi] += gcol
        dha[:, :, lo:hi] += gcol.abs()
    keep = (c.h > 0).double().reshape(C, B, L, Ch)
    dh, dha = (dh * keep).reshape(C, B * L, Ch), (dha * keep).reshape(C, B * L, Ch)
    return {"cols": (cols.reshape(C, B * L, 3 * Cin), torch.zeros(())), "dx": (dx, 3 * U * dxa),
            "pool": (pool, pt), "dh": (dh, (4 + 1 + nd + 1) * U * dha)}


# ================================================================================================== LayerNorm(64)
LN_ROWS = [1, 15, 16, 17, 255, 256, 257, 513]


def ln_case(R, strided=False, has_a=True, has_s=True, accum=0, has_da=True, special="mixed", C=5, seed=0):
    g = gen(R, seed, 51)
    c = NS(C=C, R=R, strided=strided, has_a=has_a, has_s=has_s, accum=accum, has_da=has_da, p_a=0.1 if has_a else 0.0,
           p_o=0.3, step=seed % 3, id=f"R{R} {'s67' if strided else 'al'} a{int(has_a)} s{int(has_s)} acc{accum} "
                                      f"da{int(has_da)} {special}")
    x = randn(g, C, R, 64)
    kind = {"mixed": None, "const": 2, "mean1e4": 3, "tiny": 4, "normal": 0}[special]
    for r in range(R):
        k = r % 5 if kind is None else kind
        if k == 2:
            x[:, r] = x[:, r, :1]  # constant row: variance 0
        elif k == 3:
            x[:, r] += 1e4          # mean 1e4, unit spread
        elif k == 4:
            x[:, r] *= 1e-20
    c.x = x
    c.a = randn(g, C, R, 64) * x.abs().amax(-1, keepdim=True).clamp(max=1.0) if has_a else None
    c.gamma, c.beta = 1 + 0.1 * randn(g, C, 64), 0.1 * randn(g, C, 64)
    c.dy, c.dx0 = randn(g, C, R, 64), randn(g, C, R, 64)
    c.dg0, c.db0 = randn(g, C, 64), randn(g, C, 64)
    return c


def cases_ln():
    opts = [(False, True, True, 0, True), (True, True, True, 1, True), (False, False, True, 0, False),
            (True, False, False, 1, False), (False, True, False, 1, True), (True, True, True, 0, False)]
    i = 0
    for R in LN_ROWS:
        for k in range(2):
            yield ln_case(R, *opts[i % len(opts)], special="mixed" if R > 1 else "normal", seed=i)
            i += 1
    for sp in ("const", "mean1e4", "tiny"):
        yield ln_case(1, False, False, True, 0, False, special=sp, seed=i)  # a absent: the row is what the name says
        yield ln_case(17, True, False, True, 1, False, special=sp, seed=i + 1)
        i += 2


def ln_core(s, ts, eps=1e-5):
    """mean, centred rows and rstd of ``s`` (known to ``ts``) with their bounds: 64 additions for each mean, the
    cancellation in ``s - mean`` (companion |s| + |mean|), first-order propagation into the variance and rstd."""
    mean = s.mean(-1, keepdim=True)
    tmean = ts.mean(-1, keepdim=True) + (64 + 8) * U * s.abs().mean(-1, keepdim=True)
    d = s - mean
    td = ts + tmean + U * (s.abs() + mean.abs())
    var = (d * d).mean(-1, keepdim=True)
    tvar = (2 * d.abs() * td).mean(-1, keepdim=True) + (64 + 8) * U * var + TINY
    q = var + eps
    rstd = q ** -0.5 if eps > 0 else torch.where(var > 0, var ** -0.5, torch.full_like(var, INF))
    trstd = rstd * (0.5 * tvar / q + (T["rsqrt"] + 2) * U)
    return mean, tmean, d, td, rstd, trstd


def ref_ln_fwd(c, one=False, eps=1e-5):
    C = 1 if one else c.C
    x = c.x[:C].double()
    s, ts = x, torch.zeros_like(x)
    if c.a is not None:
        av = c.a[:C].double()
        sa = drop_scale(C, c.step, 3, c.R, 64, c.p_a)
        av = av * sa if sa is not None else av
        s = x + av
        ts = 3 * U * (x.abs() + av.abs())  # inv_keep, the product, the sum
    gm, bt = c.gamma[:C].double()[:, None, :], c.beta[:C].double()[:, None, :]
    mean, tmean, d, td, rstd, trstd = ln_core(s, ts, eps)
    core = d * rstd * gm
    ty = gm.abs() * (td * rstd + d.abs() * trstd) + 4 * U * core.abs() + U * bt.abs()
    y = core + bt
    so = drop_scale(C, c.step, 4, c.R, 64, c.p_o)
    if so is not None:
        ty = ty * so + 2 * U * (y * so).abs()
        y = y * so
    res = {"y": (y, ty), "stats": (torch.cat([mean, rstd], -1), torch.cat([tmean, trstd], -1))}
    if c.has_s:
        res["s"] = (s, ts)
    return res


def ln_saved(c):
    """The fp32 (s, stats) the backward is given: the forward reference rounded to fp32 (inputs, not results)."""
    hs, c.has_s = c.has_s, True
    r = ref_ln_fwd(c)
    c.has_s = hs
    return r["s"][0].float(), r["stats"][0].float()


def ref_ln_bwd(c, one=False, with_a2=True):
    C = 1 if one else c.C
    # the backward of LayerNorm at the saved fp32 ``s``: an implementation may read the saved (mean, rstd) or
    # recompute them, so the statistics carry the forward's bound
    s = ln_saved(c)[0][:C].double()
    mean, tmean, d, td, rstd, trstd = ln_core(s, torch.zeros_like(s))
    gm = c.gamma[:C].double()[:, None, :]
    g, tg = c.dy[:C].double(), torch.zeros(())
    so = drop_scale(C, c.step, 4, c.R, 64, c.p_o)
    if so is not None:
        g = g * so
        tg = 2 * U * g.abs()
    xh = d * rstd
    txh = td * rstd + d.abs() * trstd + U * xh.abs()
    dxh = g * gm
    tdxh = gm.abs() * tg + U * dxh.abs()
    m = lambda t: t.mean(-1, keepdim=True)
    a1, a2 = m(dxh), m(dxh * xh)
    ta1 = m(tdxh) + (64 + 8) * U * m(dxh.abs())
    ta2 = m(tdxh * xh.abs() + dxh.abs() * txh) + (64 + 8) * U * m((dxh * xh).abs())
    if not with_a2:
        a2 = torch.zeros_like(a2)
    inner = dxh - a1 - xh * a2
    tin = tdxh + ta1 + txh * a2.abs() + xh.abs() * ta2 + 3 * U * (dxh.abs() + a1.abs() + (xh * a2).abs())
    dx = rstd * inner
    tdx = rstd * tin + trstd * inner.abs() + U * dx.abs()
    res = {}
    if c.has_da:
        sa = drop_scale(C, c.step, 3, c.R, 64, c.p_a)
        res["da"] = (dx * sa, tdx * sa + 2 * U * (dx * sa).abs()) if sa is not None else (dx, tdx)
    if c.accum:
        d0 = c.dx0[:C].double()
        tdx = tdx + U * (d0.abs() + dx.abs())
        dx = d0 + dx
    res["dx"] = (dx, tdx)
    dg0, db0 = c.dg0[:C].double(), c.db0[:C].double()
    res["dgamma"] = (dg0 + (g * xh).sum(1), (tg * xh.abs() + g.abs() * txh + U * (g * xh).abs()).sum(1)
                     + (c.R + 8) * U * (dg0.abs() + (g * xh).abs().sum(1)))
    res["dbeta"] = (db0 + g.sum(1), (tg + torch.zeros_like(g)).sum(1) + (c.R + 8) * U * (db0.abs() + g.abs().sum(1)))
    return res


def _rows(t, dev, strided):
    return place(t, dev, "k", unaligned=True, off=1, stride=67) if strided else t.clone().to(dev)


def run_ln_fwd(c, dev, one=False):
    C = 1 if one else c.C
    s = torch.full((C, c.R, 64), 9.0, device=dev) if c.has_s else None
    y = _rows(torch.full((C, c.R, 64), 9.0), dev, c.strided)
    st = torch.full((C, c.R, 2), 9.0, device=dev)
    Lx.ln_fwd(_rows(c.x[:C], dev, c.strided), None if c.a is None else _rows(c.a[:C], dev, c.strided), s, y, st,
              c.gamma[:C].to(dev), c.beta[:C].to(dev), make_ctl(C, dev, c.step), layer_a=3, p_a=c.p_a, layer_o=4,
              p_o=c.p_o)
    out = {"y": y.cpu(), "stats": st.cpu()}
    if c.has_s:
        out["s"] = s.cpu()
    return out


def run_ln_bwd(c, dev, one=False):
    C = 1 if one else c.C
    s32, st32 = ln_saved(c)
    dx = _rows(c.dx0[:C], dev, c.strided)
    da = _rows(torch.full((C, c.R, 64), 9.0), dev, c.strided) if c.has_da else None
    dg, db = c.dg0[:C].clone().to(dev), c.db0[:C].clone().to(dev)
    Lx.ln_bwd(_rows(c.dy[:C], dev, c.strided), _rows(s32[:C], dev, c.strided), st32[:C].contiguous().to(dev),
              c.gamma[:C].to(dev), dx, c.accum, da, dg, db, make_ctl(C, dev, c.step), layer_a=3, p_a=c.p_a, layer_o=4,
              p_o=c.p_o)
    out = {"dx": dx.cpu(), "dgamma": dg.cpu(), "dbeta": db.cpu()}
    if c.has_da:
        out["da"] = da.cpu()
    return out


# ================================================================================================== GRU cell
def ref_sigm(x, tx):
    """sigmoid through the fast exponential: e = exp(-x) within (2 + |x|) U relative."""
    s = torch.sigmoid(x)
    return s, s * (1 - s) * ((2 + x.abs()) * U + tx) + 2 * U * s + TINY


def cases_gru():
    for i, B in enumerate((1, 7, 8, 9, 33, 300)):
        g = gen(B, 61)
        C = 5
        c = NS(C=C, B=B, col0=32 * (i % 2), off=5 + i, id=f"B{B} col0 {32 * (i % 2)}")
        gi = randn(g, C, B, 96) * 2
        sel = torch.randint(0, 16, (C, B, 96), generator=g)
        for k, v in enumerate((30.0, -30.0, 90.0, -90.0)):  # saturated pre-activations
            gi[sel == k] = v
        c.gi, c.flat = gi, randn(g, C, 400)  # bhh = flat[:, off:off + 96]: a row of a flat arena
        c.h0, c.dh, c.gflat = randn(g, C, B, 64), randn(g, C, B, 64), randn(g, C, 400)
        yield c


def _gru_parts(c, C):
    gi, bh = c.gi[:C].double(), c.flat[:C, c.off:c.off + 96].double()[:, None, :]
    xr, xz = gi[..., :32] + bh[..., :32], gi[..., 32:64] + bh[..., 32:64]
    r, tr = ref_sigm(xr, U * xr.abs())
    z, tz = ref_sigm(xz, U * xz.abs())
    bn = bh[..., 64:]
    a = gi[..., 64:] + r * bn
    ta = bn.abs() * tr + 2 * U * (gi[..., 64:].abs() + (r * bn).abs())
    n = torch.tanh(a)
    tn = (1 - n * n) * ta + T["tanh"] * U * n.abs() + TINY
    return r, tr, z, tz, n, tn, bn


def ref_gru(c, one=False):
    C = 1 if one else c.C
    r, tr, z, tz, n, tn, bn = _gru_parts(c, C)
    h, th = c.h0[:C].double().clone(), torch.zeros(C, c.B, 64, dtype=torch.float64)
    hv = (1 - z) * n
    h[..., c.col0:c.col0 + 32] = hv
    th[..., c.col0:c.col0 + 32] = n.abs() * tz + (1 - z) * tn + 2 * U * hv.abs() + U * n.abs()
    d = c.dh[:C, :, c.col0:c.col0 + 32].double()
    omn = 1 - n * n
    tomn = 2 * n.abs() * tn + 2 * U  # n * n and the subtraction from 1
    dan = d * (1 - z) * omn
    tdan = d.abs() * (omn * (tz + U) + (1 - z) * tomn) + 3 * U * dan.abs() + TINY
    rr = r * (1 - r)
    dar = dan * bn * rr
    tdar = bn.abs() * (rr * tdan + dan.abs() * (tr + 2 * U * rr + U * r)) + 4 * U * dar.abs() + TINY
    zz = z * (1 - z)
    daz = -d * n * zz
    tdaz = d.abs() * (zz * tn + n.abs() * (tz + 2 * U * zz + U * z)) + 4 * U * daz.abs() + TINY
    dgi = torch.cat([dar, daz, dan], -1)
    tdgi = torch.cat([tdar, tdaz, tdan], -1)
    nB = (c.B + 8) * U
    dbih = dgi.sum(1)
    tdbih = tdgi.sum(1) + nB * dgi.abs().sum(1)
    dnh = (dan * r).sum(1)
    tdnh = (tdan * r + dan.abs() * tr + U * (dan * r).abs()).sum(1) + nB * (dan * r).abs().sum(1)
    gf = c.gflat[:C].double()
    gi_, gh_ = gf.clone(), gf.clone()
    ti, thh = torch.zeros_like(gf), torch.zeros_like(gf)
    gi_[:, c.off:c.off + 96], ti[:, c.off:c.off + 96] = dbih, tdbih
    gh_[:, c.off:c.off + 96] = torch.cat([dbih[:, :64], dnh], -1)
    thh[:, c.off:c.off + 96] = torch.cat([tdbih[:, :64], tdnh], -1)
    return {"h": (h, th), "dgi": (dgi, tdgi), "dbih": (gi_, ti), "dbhh": (gh_, thh)}


def run_gru(c, dev, one=False):
    C = 1 if one else c.C
    flat = c.flat[:C].to(dev)
    bhh = flat[:, c.off:c.off + 96]
    gi = c.gi[:C].to(dev)
    h = c.h0[:C].clone().to(dev)
    Lx.gru_fwd(gi, bhh, h, c.col0)
    dgi = torch.full((C, c.B, 96), 9.0, device=dev)
    ga, gb = c.gflat[:C].clone().to(dev), c.gflat[:C].clone().to(dev)
    Lx.gru_bwd(c.dh[:C].to(dev), c.col0, gi, bhh, dgi, ga[:, c.off:c.off + 96], gb[:, c.off:c.off + 96])
    return {"h": h.cpu(), "dgi": dgi.cpu(), "dbih": ga.cpu(), "dbhh": gb.cpu()}


# ================================================================================================== losses
LOSS_B = [1, 255, 256, 257, 600]


def loss_case(kind, B, K=1, min_bs=2, step=1, nan_abort=True, nan_at=None, sat=None, seed=0):
    """Clients: bs = B, B - 1, 2, 1, 0, and a sixth (bs = B) that has already failed.  S = 2 steps."""
    g = gen(B, K, min_bs, step, seed, 71)
    C, S, E = 6, 2, 3
    c = NS(kind=kind, C=C, B=B, K=K, S=S, E=E, min_bs=min_bs, step=step, nan_abort=nan_abort, nan_at=nan_at,
           id=f"{kind} B{B} K{K} min_bs{min_bs} step{step} abort{int(nan_abort)} nan{nan_at} sat{sat}")
    bs = [min(B, max(0, v)) for v in (B, B - 1, 2, 1, 0, B)]
    c.bsz = torch.tensor([[1] * C, bs], dtype=torch.int32)
    c.epoch = torch.randint(0, E, (S, C), generator=g, dtype=torch.int32)
    c.nb = torch.randint(1, 9, (C,), generator=g, dtype=torch.int32)
    c.failed = torch.tensor([0, 0, 0, 0, 0, 1], dtype=torch.int32)
    c.losses0 = randn(g, C, E)
    if kind == "bce":
        z = (torch.rand(C, B, generator=g) * 16 - 8)
        y = (torch.rand(C, B, generator=g) < 0.5).float()
        if sat is not None:      # B = 1: one saturated logit per case
            z[:], y[:] = sat[0], sat[1]
        elif B >= 16:            # +-50 / +-200 against both labels
            for k, v in enumerate((50.0, -50.0, 200.0, -200.0)):
                z[:, 3 + 2 * k], z[:, 4 + 2 * k] = v, v
                y[:, 3 + 2 * k], y[:, 4 + 2 * k] = 0.0, 1.0
        if nan_at is not None:
            z[1, 0 if nan_at == "first" else min(B, bs[1]) - 1] = float("nan")
        c.z, c.y = z, y
    else:
        x = torch.rand(C, B, K, generator=g) * 16 - 8
        if B >= 16:
            x[:, 3], x[:, 4] = 80.0, -80.0
            x[:, 5, ::2], x[:, 5, 1::2] = 80.0, -80.0
        c.y = torch.randint(0, K, (C, B), generator=g, dtype=torch.int64)
        if nan_at is not None:
            x[1, 2 % B, 0 if nan_at == "first" else K - 1] = float("nan")
        c.z = x
    return c


def cases_loss(kind):
    Ks = (1,) if kind == "bce" else (1, 2, 6)
    i = 0
    for B in LOSS_B:
        for K in Ks:
            for min_bs, step in ((2, 1), (1, 1), (2, 2)):  # step = S - 1 and S (S = 2)
                yield loss_case(kind, B, K, min_bs, step, seed=i)
                i += 1
    if kind == "bce":
        for zv in (50.0, -50.0, 200.0, -200.0):
            for yv in (0.0, 1.0):
                yield loss_case(kind, 1, 1, 1, 1, sat=(zv, yv), seed=i)
                i += 1
    for K in Ks:
        for nan_at in ("first", "last"):
            for abort in (True, False):
                yield loss_case(kind, 257, K, 2, 1, nan_abort=abort, nan_at=nan_at, seed=i)
                i += 1


def ref_loss(c, mean_over_B=False):
    """(losses, dz, failed): activity rule ``bs >= max(min_bs, 1)``, not failed, ``step < S``; ``losses[c, epoch] +=
    loss / nb``; a NaN loss sets ``failed`` (losses untouched, dz zero) when ``nan_abort`` is on."""
    C, B, K = c.C, c.B, c.K
    losses, tl = c.losses0.double().clone(), torch.zeros(C, c.E, dtype=torch.float64)
    failed = c.failed.clone()
    shape = (C, B) if c.kind == "bce" else (C, B, K)
    dz, tdz = torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64)
    for ci in range(C):
        bs = int(c.bsz[c.step, ci]) if c.step < c.S else 0
        if not (bs >= max(c.min_bs, 1) and int(c.failed[ci]) == 0):
            continue
        den = B if mean_over_B else bs
        if c.kind == "bce":
            z, t = c.z[ci, :bs].double(), c.y[ci, :bs].double()
            e = torch.exp(-z)
            sat = e * (1 + 8 * U) < 2.0 ** -26            # 1 + e rounds to 1 in fp32: p = 1 exactly
            p = torch.where(sat, torch.ones_like(z), 1 / (1 + e))
            q = torch.where(sat, torch.zeros_like(z), e / (1 + e))  # 1 - p
            dp = torch.where(sat, torch.zeros_like(z), p * (q * (T["exp"] + 1) * U + 2 * U)) + TINY
            lp = torch.where(p < 0.5, torch.log(p), torch.log1p(-q))
            lq = torch.where(p < 0.5, torch.log1p(-p), torch.log(q))
            # conditioning: d log(1 - p) = dp / (1 - p) = (p / q) dp; the clamp at -100 is exact
            t1 = torch.where(lp < -100, torch.zeros_like(z), dp / p.clamp(min=TINY) + T["log"] * U * lp.abs())
            t2 = torch.where(sat | (lq < -100), torch.zeros_like(z),
                             dp / q.clamp(min=TINY) + U * (p / q.clamp(min=TINY)) + T["log1p"] * U * lq.abs())
            a1, a2 = t * lp.clamp(min=-100), (1 - t) * lq.clamp(min=-100)
            a1, a2 = torch.where(t == 0, torch.zeros_like(z), a1), torch.where(t == 1, torch.zeros_like(z), a2)
            row = -(a1 + a2)
            trow = t * t1 + (1 - t) * t2 + 3 * U * (a1.abs() + a2.abs())
            w = p * q
            gexact = (p - t) / w.clamp(min=1e-12) * w / den
            big = w >= 1e-12
            relw = dp / p.clamp(min=TINY) + dp / q.clamp(min=TINY)
            tg = torch.where(big, (dp + 6 * U * (p - t).abs()) / den,
                             gexact.abs() * (relw + 8 * U) + dp * w / 1e-12 / den) + TINY
            tg = torch.where(sat, torch.zeros_like(z), tg)
            gnan = torch.isnan(z)
        else:
            x = c.z[ci, :bs].double()
            yy = c.y[ci, :bs]
            mx = torch.nan_to_num(x, nan=-INF).amax(-1, keepdim=True)
            ex = torch.exp(x - mx)
            tex = ex * (T["exp"] + 1 + (x - mx).abs()) * U + TINY
            se = ex.sum(-1, keepdim=True)
            tse = tex.sum(-1, keepdim=True) + K * U * se
            xy = x.gather(1, yy[:, None])
            lse = torch.log(se)
            row = (lse + mx - xy)[:, 0]
            trow = (tse / se + T["log"] * U * lse.abs() + 2 * U * (lse.abs() + mx.abs() + xy.abs()))[:, 0]
            sm = ex / se
            oh = F.one_hot(yy, K).double()
            gexact = (sm - oh) / den
            tg = (tex / se + sm * (tse / se + 2 * U) + U * (sm - oh).abs()) / den + TINY
            gnan = torch.isnan(x).any(-1, keepdim=True).expand_as(x)
        loss = row.sum() / den
        tloss = trow.sum() / den + (bs + 8) * U * row.abs().sum() / den
        if bool(torch.isnan(loss)) and c.nan_abort:
            failed[ci] = 1
            continue
        ep, nb = int(c.epoch[c.step, ci]), int(c.nb[ci])
        tl[ci, ep] = tloss / nb + 2 * U * (losses[ci, ep].abs() + loss.abs() / nb)
        losses[ci, ep] += loss / nb
        dz[ci, :bs] = torch.where(gnan, torch.full_like(gexact, float("nan")), gexact)
        tdz[ci, :bs] = tg
    return {"losses": (losses, tl), "dz": (dz, tdz), "failed_int": failed}


def run_loss(c, dev, one=False):
    C = 1 if one else c.C
    ctl = make_ctl(C, dev, c.step, c.min_bs, c.nan_abort)
    failed, losses = c.failed[:C].clone().to(dev), c.losses0[:C].clone().to(dev)
    dz = torch.full(c.z[:C].shape, 9.0, device=dev)
    fn = Lx.bce if c.kind == "bce" else Lx.ce
    fn(c.z[:C].to(dev), c.y[:C].to(dev), c.bsz[:, :C].contiguous().to(dev), c.epoch[:, :C].contiguous().to(dev),
       c.nb[:C].to(dev), ctl, failed, losses, dz)
    return {"losses": losses.cpu(), "dz": dz.cpu(), "failed": failed.cpu()}


# ================================================================================================== optimizer
def cases_adam():
    i = 0
    for P in (1, 2, 3, 5, 1003):
        # client 1's row starts at P floats: P = 1003 -> 1 head entry, the last group is the tail
        skips = [(0, 0), (0, 1), (P - 1, P)] + ([(1, 2), (P - 2, P - 1), (500, 509)] if P == 1003 else [])
        for skip in skips:
            for tcount, sgd, gzero in ((0, 0.0, False), (5000, 0.0, False), (0, 0.05, False), (5000, 0.0, True)):
                g = gen(P, i, 81)
                c = NS(C=3, P=P, skip=skip, tcount=tcount, sgd=sgd, lr=1e-2, id=f"P{P} skip{skip} t{tcount} sgd{sgd} "
                                                                               f"g0{int(gzero)}")
                c.p, c.g, c.m = randn(g, 3, P), randn(g, 3, P) * (0.0 if gzero else 1.0), randn(g, 3, P) * 0.1
                c.v = randn(g, 3, P) ** 2 * 0.01
                c.bsz = torch.tensor([[8, 8, 1]], dtype=torch.int32)  # client 2: batch of 1 < min_bs -> inactive
                yield c
                i += 1


def ref_adam(c, t_offset=1):
    p, g, m, v = (t.double() for t in (c.p, c.g, c.m, c.v))
    keep = torch.ones(c.P, dtype=torch.bool)
    keep[c.skip[0]:c.skip[1]] = False
    act = torch.tensor([True, True, False])[:, None] & keep[None, :]
    z = torch.zeros_like(p)
    if c.sgd > 0:
        lr = f32(c.sgd)
        pn, tp = p - lr * g, 3 * U * (p.abs() + (lr * g).abs())
        mn, vn, tm, tv = m, v, z, z
    else:
        t = c.tcount + t_offset
        mn = m + 0.1 * (g - m)
        tm = 4 * U * (m.abs() + 0.1 * (g.abs() + m.abs()))
        vn = 0.999 * v + 0.001 * g * g
        tv = 5 * U * vn
        b1t, b2t = 0.9 ** t, 0.999 ** t
        # beta^t: powf budget, and the fp32 constant's representation error (<= U / 4) grows t-fold
        bc1, bc2 = torch.tensor(1 - b1t, dtype=torch.float64), torch.tensor(1 - b2t, dtype=torch.float64)
        rel1 = (b1t * (T["pow"] + 1 + t / 4) * U + U * bc1) / bc1
        rel2 = (b2t * (T["pow"] + 1 + t / 4) * U + U * bc2) / bc2
        a = f32(c.lr) / bc1
        sq = vn.sqrt() / bc2.sqrt()
        den = sq + 1e-8
        tden = sq * (0.5 * torch.where(vn > 0, tv / vn.clamp(min=TINY), z) + 0.5 * rel2 + 4 * U) + U * den
        u = a * mn / den
        tu = u.abs() * (rel1 + 2 * U + tden / den + 3 * U) + a * tm / den
        pn, tp = p - u, tu + U * (p.abs() + u.abs())
    w = lambda new, old: torch.where(act, new, old)
    return {"p": (w(pn, p), w(tp, z)), "m": (w(mn, m), w(tm, z)), "v": (w(vn, v), w(tv, z)),
            "g_zeroed": (torch.where(act, z, g), z)}


def run_adam(c, dev):
    p, g, m, v = (t.clone().to(dev) for t in (c.p, c.g, c.m, c.v))
    tcount = torch.full((3,), c.tcount, dtype=torch.int32, device=dev)
    failed = torch.zeros(3, dtype=torch.int32, device=dev)
    Lx.adam_clients(p, g, m, v, tcount, c.bsz.to(dev), make_ctl(3, dev, 0), failed, c.lr, c.skip, c.sgd,
                    zero_grads=True)
    out = {"p": p.cpu(), "m": m.cpu(), "v": v.cpu()}
    if str(dev) != "cpu":  # zero_grads is the device path's (the composite leaves the gradients alone)
        out["g_zeroed"] = g.cpu()
    return out


# ================================================================================================== HAR stem / mean
CONV_PE_BL = [(1, 1), (3, 2), (3, 17), (65, 16), (2, 561)]  # the last two cross the 1024-row block


def cases_conv_pe():
    for B, L in CONV_PE_BL:
        g = gen(B, L, 91)
        C = 5
        c = NS(C=C, B=B, L=L, w_off=5, b_off=199, pe_off=266, P=266 + 64 * L + 3, id=f"B{B} L{L}")  # offsets % 4 != 0
        c.x, c.params, c.dh, c.grads0 = randn(g, C, B, L), randn(g, C, c.P), randn(g, C, B * L, 64), randn(g, C, c.P)
        yield c


def ref_conv_pe(c, one=False, l0_taps_shifted=False):
    C, B, L = 1 if one else c.C, c.B, c.L
    x, pr = c.x[:C].double(), c.params[:C].double()
    w = pr[:, c.w_off:c.w_off + 192].reshape(C, 64, 3)
    b, pe = pr[:, c.b_off:c.b_off + 64], pr[:, c.pe_off:c.pe_off + 64 * L].reshape(C, 1, L, 64)
    xs = torch.zeros(C, B, L, 3, dtype=torch.float64)  # xs[..., j] = x[l + j - 1]
    xs[:, :, 1:, 0], xs[:, :, :, 1], xs[:, :, :-1, 2] = x[:, :, :-1], x, x[:, :, 1:]
    if l0_taps_shifted:  # mutant: at l = 0 the taps start at w[0] instead of skipping it
        xs[:, :, 0, 0], xs[:, :, 0, 1], xs[:, :, 0, 2] = xs[:, :, 0, 1].clone(), xs[:, :, 0, 2].clone(), 0.0
    wt = w
    h = torch.einsum("cblj,coj->cblo", xs, wt) + b[:, None, None, :] + pe
    ha = torch.einsum("cblj,coj->cblo", xs.abs(), wt.abs()) + b.abs()[:, None, None, :] + pe.abs()
    dh = c.dh[:C].double().reshape(C, B, L, 64)
    g0 = c.grads0[:C].double()
    grads, tg = g0.clone(), torch.zeros_like(g0)
    n = (B * L + 8) * U
    dw, dwa = torch.einsum("cblo,cblj->coj", dh, xs), torch.einsum("cblo,cblj->coj", dh.abs(), xs.abs())
    sw, sb = slice(c.w_off, c.w_off + 192), slice(c.b_off, c.b_off + 64)
    grads[:, sw] += dw.reshape(C, 192)
    tg[:, sw] = n * (g0[:, sw].abs() + dwa.reshape(C, 192)) + U * dwa.reshape(C, 192)
    grads[:, sb] += dh.sum((1, 2))
    tg[:, sb] = n * (g0[:, sb].abs() + dh.abs().sum((1, 2)))
    return {"h": (h.reshape(C, B * L, 64), 8 * U * ha.reshape(C, B * L, 64)), "grads": (grads, tg)}


def run_conv_pe(c, dev, one=False):
    C = 1 if one else c.C
    h = torch.full((C, c.B * c.L, 64), 9.0, device=dev)
    Lx.conv_pe_fwd(c.x[:C].to(dev), c.params[:C].to(dev), c.w_off, c.b_off, c.pe_off, h)
    grads = c.grads0[:C].clone().to(dev)
    Lx.conv_pe_bwd(c.x[:C].to(dev), c.dh[:C].to(dev), grads, c.w_off, c.b_off)
    return {"h": h.cpu(), "grads": grads.cpu()}


def cases_mean_rows():
    for L in (1, 15, 16, 17, 561):
        for B in (1, 3):
            g = gen(L, B, 95)
            yield NS(C=5, B=B, L=L, h=randn(g, 5, B * L, 64), dout=randn(g, 5, B, 64), id=f"L{L} B{B}")


def ref_mean_rows(c, one=False, div=None):
    C, L = 1 if one else c.C, c.L
    h = c.h[:C].double().reshape(C, c.B, L, 64)
    div = div or L
    dh = (c.dout[:C].double()[:, :, None, :] / div).expand(C, c.B, L, 64).reshape(C, c.B * L, 64)
    return {"out": (h.sum(2) / div, (L + 8) * U * h.abs().sum(2) / div), "dh": (dh, 2 * U * dh.abs())}


def run_mean_rows(c, dev, one=False):
    C = 1 if one else c.C
    out, dh = torch.full((C, c.B, 64), 9.0, device=dev), torch.full((C, c.B * c.L, 64), 9.0, device=dev)
    Lx.mean_rows_fwd(c.h[:C].to(dev), c.B, c.L, out)
    Lx.mean_rows_bwd(c.dout[:C].to(dev), c.B, c.L, dh)
    return {"out": out.cpu(), "dh": dh.cpu()}


# ================================================================================================== step_end
def cases_step_end():
    for C in (1, 64, 65, 130):
        for min_bs in (2, 1):
            g = gen(C, min_bs, 99)
            S = 3
            yield NS(C=C, S=S, min_bs=min_bs, bsz=torch.randint(0, 4, (S, C), generator=g, dtype=torch.int32),
                     failed=(torch.rand(C, generator=g) < 0.3).int(), id=f"C{C} min_bs{min_bs}",
                     tcount=torch.randint(0, 100, (C,), generator=g, dtype=torch.int32))


def ref_step_end(c):
    """Two calls from step S - 1: the second one is past S (nobody is active, the counter still advances)."""
    bs = c.bsz[c.S - 1]
    act = (bs >= max(c.min_bs, 1)) & (c.failed == 0)
    return c.tcount + act.int(), [c.S, c.S + 1]


def run_step_end(c, dev):
    ctl = make_ctl(c.C, dev, c.S - 1, c.min_bs)
    tcount = c.tcount.clone().to(dev)
    steps = []
    for _ in range(2):
        Lx.step_end(ctl, tcount, c.bsz.to(dev), c.failed.to(dev))
        steps.append(int(ctl.stepctl[0]))
    return tcount.cpu(), steps, ctl.stepctl.cpu()


# ================================================================================================== CPU tests
# ---- the composite passes: the references are right, and an honest fp32 implementation meets the bounds
def _all(cases, run, ref, name):
    w = 0.0
    for c in cases:
        w = max(w, check(run(c, "cpu"), ref(c), f"{name} [{c.id}]"))
    print(f"{name}: worst err/bound {w:.3g}")


@pytest.mark.parametrize("family", ["shapes", "layouts", "splitk", "nan"])
def test_composite_meets_gemm_reference(family):
    _all(globals()["cases_bgemm_" + family](), run_gemm, ref_gemm, "bgemm " + family)


@pytest.mark.parametrize("family", ["tsgemm", "tsgemm_tiles", "tsgemm_colsums", "tsgemm_fallback"])
def test_composite_meets_tall_skinny_reference(family):
    _all(globals()["cases_" + family](), run_gemm, ref_gemm, family)


def test_composite_meets_colsum_and_gather_references():
    _all(cases_colsum(), run_colsum, ref_colsum, "colsum")
    for c in cases_gather():
        assert check(run_gather(c, "cpu"), ref_gather(c), "gather " + c.id) == 0.0


def test_composite_meets_conv_and_pool_references():
    _all(cases_conv(), run_conv, ref_conv, "conv/pool")


def test_composite_meets_layernorm_references():
    _all(cases_ln(), run_ln_fwd, ref_ln_fwd, "ln_fwd")
    _all(cases_ln(), run_ln_bwd, ref_ln_bwd, "ln_bwd")


def test_composite_meets_gru_reference():
    _all(cases_gru(), run_gru, ref_gru, "gru")


@pytest.mark.parametrize("kind", ["bce", "ce"])
def test_composite_meets_loss_references(kind):
    _all(cases_loss(kind), run_loss, ref_loss, kind)


def test_composite_meets_adam_reference():
    _all(cases_adam(), run_adam, ref_adam, "adam")


def test_composite_meets_har_stem_and_mean_references():
    _all(cases_conv_pe(), run_conv_pe, ref_conv_pe, "conv_pe")
    _all(cases_mean_rows(), run_mean_rows, ref_mean_rows, "mean_rows")


def test_composite_meets_step_end_reference():
    for c in cases_step_end():
        tcount, steps, ctl = run_step_end(c, "cpu")
        want, wsteps = ref_step_end(c)
        assert torch.equal(tcount, want) and steps == wsteps and ctl.tolist()[1:] == [c.min_bs, 1], c.id


# ---- mutants fail: a subtle error does not fit under the bounds
def standin_gemm(c, mutant=None):
    """fp32 stand-in for the GEMM kernels — bf16-rounded operands, fp32 accumulation and epilogue — optionally wrong
    in one way."""
    rnd = bf16_trunc if mutant == "bf16_truncation" else bf16_rne
    A, B = rnd(c.A).float(), rnd(c.B).float()
    v = np.float32(c.alpha).item() * torch.bmm(A, B.transpose(1, 2))
    if c.bias is not None:
        v = v + (c.bias.roll(1, 0) if mutant == "neighbour_bias" else c.bias)[:, None, :]
    if mutant == "row_scaled":
        v[:, -1] *= 1.01
    z = v.clone()
    if c.act == 1:
        v = F.relu(v)
    elif c.act == 2:
        v = F.gelu(v, approximate="tanh" if mutant == "gelu_tanh" else "none")
    sc = drop_scale(c.C, c.step, c.layer, c.M, c.N, c.p)
    if sc is not None:
        v = v * (sc.float() if mutant != "dropout_unscaled" else (sc > 0).float())
    if c.G is not None:
        if c.gact == 1:
            v = v * ((c.G >= 0) if mutant == "relu_ge" else (c.G > 0)).float()
        else:
            v = v * ref_actd(c.G, c.gact)[0].float()
    if c.accum:
        v = c.fillC[:, :, ::c.cs] + v
    return {"C": v, "Z": z}


GEMM_MUTANTS = ["bf16_truncation", "row_scaled", "neighbour_bias", "dropout_unscaled", "gelu_tanh", "relu_ge"]


@pytest.mark.parametrize("mutant", GEMM_MUTANTS)
def test_gemm_mutants_fail(mutant):
    """The issue's own shape (C=3, M=150, K=45, N=70): the honest stand-in passes, the mutant does not."""
    c = gemm_case(3, 150, 70, 45, act=2 if mutant == "gelu_tanh" else 1, p=0.3, gact=1, accum=1, seed=3)
    ref = {k: v for k, v in ref_gemm(c).items() if k in ("C", "Z")}
    honest = worst(standin_gemm(c), ref, "honest stand-in")
    wrong = worst(standin_gemm(c, mutant), ref, mutant)
    assert max(honest.values()) <= 1.0
    assert max(wrong.values()) > 1.0, f"{mutant} passes: {wrong}"


def _fails(value, ref):
    return ratio(value, *ref) > 1.0


def test_layer_mutants_fail():
    ln = [c for c in cases_ln()]
    # LayerNorm variance without the 1e-5: visible where the variance is small (constant and 1e-20 rows)
    assert any(_fails(ref_ln_fwd(c, eps=0.0)["y"][0], ref_ln_fwd(c)["y"]) for c in ln)
    assert all(_fails(ref_ln_bwd(c, with_a2=False)["dx"][0], ref_ln_bwd(c)["dx"]) for c in ln if "mixed" in c.id)
    pool = [c for c in cases_conv() if c.L == 5]
    assert pool and all(_fails(ref_conv(c, bins_shift=1)["pool"][0], ref_conv(c)["pool"]) for c in pool)
    assert all(_fails(ref_conv(c, bins_shift=1)["dh"][0], ref_conv(c)["dh"]) for c in pool if c.relu == "none")
    bce = [c for c in cases_loss("bce") if c.B >= 255 and c.step == 1 and c.nan_at is None]
    assert bce and all(_fails(ref_loss(c, mean_over_B=True)["losses"][0], ref_loss(c)["losses"]) for c in bce)
    assert all(_fails(ref_loss(c, mean_over_B=True)["dz"][0], ref_loss(c)["dz"]) for c in bce)
    adam = [c for c in cases_adam() if c.sgd == 0 and c.tcount == 0 and c.skip == (0, 0)]
    assert adam and all(_fails(ref_adam(c, t_offset=0)["p"][0], ref_adam(c)["p"]) for c in adam)
    adam = [c for c in cases_adam() if c.sgd == 0 and c.tcount == 5000 and c.P == 1003 and float(c.g.abs().max()) > 0]
    assert adam and all(_fails(ref_adam(c, t_offset=100)["p"][0], ref_adam(c)["p"]) for c in adam)
    for c in cases_conv_pe():
        assert _fails(ref_conv_pe(c, l0_taps_shifted=True)["h"][0], ref_conv_pe(c)["h"]), c.id
    for c in cases_mean_rows():
        assert _fails(ref_mean_rows(c, div=c.L + 1)["out"][0], ref_mean_rows(c)["out"]), c.id
        assert _fails(ref_mean_rows(c, div=c.L + 1)["dh"][0], ref_mean_rows(c)["dh"]), c.id
