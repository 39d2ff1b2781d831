"""fp64 references of the ten bf16 HAR encoder kernels (``csrc/kernels/har.hip``), their error bounds, torch models of
the kernels' rounding points, deliberately wrong variants, and the inputs at which all of them are tested.

One formula per kernel (``f_*``), written once over a small value type ``Q`` with two modes:

* **ref** (``ref_*``): float64 values on exactly what the kernel reads, each with an elementwise ``tol`` that never
  looks at the output under test.  Every arithmetic step adds one fp32 rounding ``U |result|`` (a sum or dot product
  of n terms: ``(n + 1) U`` times the same sum on absolute values) and carries its inputs' bounds forward to first
  order; ``Q.bf()`` — every place where the kernel rounds an intermediate or a stored result to bf16
  (``pack_bf2`` is ``v_cvt_pk_bf16_f32``: round to nearest even, not truncation) — adds half a bf16 ulp of the value
  (``half_ulp_bf16``) and does NOT round the value.  The three device transcendentals add their measured budgets ``T`` (docs/HAR_TEST_BOUNDS.md).
  Weights are rounded to bf16 exactly where the kernel builds its LDS image (``build_img``): elementwise on an input.
  Dropout multipliers come from ``masks.keep`` / ``masks.keep_rc`` and are exact.
* **model** (``model_*``): fp32 torch arithmetic that really rounds to bf16 at every ``Q.bf()``.  ``mut=...`` selects a
  deliberately wrong variant.

``cases_*`` build inputs, ``run_*`` run the raw ``native().har_*`` bindings on a GPU; ``tests/test_gpu_har_edges.py``
(``import test_har_oracles as R``) holds the kernels to these references.  The CPU tests here show that the model (and,
where ``attackfl_amd/ops/layers.py`` has one, the fp32 composite with scheme "rc") stays within ``tol`` at every case,
that every backward formula is the derivative of its forward (float64 autograd), and that every variant in ``MUTANTS``
leaves the bound on at least one case."""
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from attackfl_amd.ops import layers as Lx
from attackfl_amd.ops import masks

U = 2.0 ** -23       # one fp32 rounding
TINY = 2.0 ** -126   # v_exp_f32 flushes results below the smallest normal
INF = float("inf")
# device transcendental budgets in units of U |f|: next power of two at or above twice the worst error measured on the
# device against float64 over the tests' input ranges (docs/HAR_TEST_BOUNDS.md); none may exceed 64
T = {"exp2": 2, "rsq": 2, "log2": 2}
assert max(T.values()) <= 64
SEEDS = [7 + 3 * c for c in range(8)]
LOG2E = float(np.float32(1.4426950408889634))
QS = float(np.float32(0.25 * 1.4426950408889634))  # the q scale the program passes (as the kernel's float)
IQ = float(np.float32(1.0) / np.float32(1.4426950408889634))
EPS = float(np.float32(1e-5))
POST_NG, QKV_NG = 64 * 64 + 256 * 64 + 64 * 256 + 640, 192 * 64 + 192
G_WO, G_W1, G_W2, G_VEC = 0, 4096, 4096 + 16384, 4096 + 2 * 16384
V_BO, V_G1, V_BE1, V_B1, V_B2, V_G2, V_BE2 = 0, 64, 128, 192, 448, 512, 576
LAYER_SIZES = [192 * 64, 192, 64 * 64, 64, 64, 64, 256 * 64, 256, 64 * 256, 64, 64, 64]
PRE = 7.0      # prefill of memory a kernel must not touch (bf16-exact)
WS_PRE = 3.0e4  # prefill of the partial buffers (large, finite)


def f32(x):
    return float(np.float32(x))


def half_ulp_bf16(a):
    """Half a bf16 ulp of the magnitudes ``a`` (8 significant bits: 2^(e - 8) for a in [2^e, 2^(e + 1))), the exact
    bound of one round-to-nearest-even — between 2^-9 a and 2^-8 a.  (2^-9 |value| itself is NOT a bound of RNE: 1 + 2^-8
    rounds to 1 with error 2^-8.)"""
    _, e = torch.frexp(a)
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), e - 9), torch.zeros_like(a))


def gen(*k):
    return torch.Generator().manual_seed(hash(tuple(int(x) for x in k)) % (2 ** 31))


def bfx(t):
    """bf16-exact fp32 values."""
    return t.float().bfloat16().float()


def ceil64(n):
    return (n + 63) // 64 * 64


def inv_keep(p):
    return f32(1.0 / (1.0 - p)) if p > 0.0 else 1.0


def key_of(ci, step):
    return masks.step_key(SEEDS[ci] & masks.M32, step)


def make_ctl(C, dev, step=0):
    ctl = Lx.StepCtl.create(SEEDS[:C], "cpu")
    ctl.stepctl[0] = step
    return Lx.StepCtl(ctl.seeds.to(dev), ctl.stepctl.to(dev))


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


def worst(out, ref, what=""):
    res = {k: ratio(out[k], *ref[k]) for k in ref}
    print(f"{what}: " + " ".join(f"{k}={v:.3g}" for k, v in res.items()))
    return res


def check(out, ref, what=""):
    res = worst(out, ref, what)
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, f"{what}: err/bound {bad}"
    return max(res.values()) if res else 0.0


# ================================================================================================ the value type
class Q:
    """ref mode: float64 value ``v`` with first-order error bound ``t``; model mode (``t is None``): fp32 value."""

    def __init__(self, v, t=None):
        self.v, self.t = v, t

    @property
    def ref(self):
        return self.t is not None

    def _c(self, o):
        if isinstance(o, Q):
            return o
        o = torch.as_tensor(o)
        return Q(o.double(), torch.zeros_like(o, dtype=torch.float64)) if self.ref else Q(o.float())

    def _r(self, v, t):  # one fp32 rounding of a result
        return Q(v, t + U * v.abs())

    def __add__(self, o):
        o = self._c(o)
        return self._r(self.v + o.v, self.t + o.t) if self.ref else Q(self.v + o.v)

    def __sub__(self, o):
        o = self._c(o)
        return self._r(self.v - o.v, self.t + o.t) if self.ref else Q(self.v - o.v)

    def __mul__(self, o):
        o = self._c(o)
        if not self.ref:
            return Q(self.v * o.v)
        return self._r(self.v * o.v, self.t * o.v.abs() + self.v.abs() * o.t)

    def times(self, k):
        """Multiply by an exact 0 / 1 flag tensor: no rounding."""
        return Q(self.v * k.double(), self.t * k.double()) if self.ref else Q(self.v * k.float())

    def mm(self, o):
        """``self @ o`` accumulated in fp32: K + 1 roundings on the absolute-value product."""
        if not self.ref:
            return Q(self.v @ o.v)
        K = self.v.shape[-1]
        av, bv = self.v.abs(), o.v.abs()
        return Q(self.v @ o.v, self.t @ bv + av @ o.t + (K + 1) * U * (av @ bv))

    def sum(self, dim, keepdim=False):
        if not self.ref:
            return Q(self.v.sum(dim, keepdim))
        n = self.v.shape[dim]
        return Q(self.v.sum(dim, keepdim), self.t.sum(dim, keepdim) + (n + 1) * U * self.v.abs().sum(dim, keepdim))

    def bf(self):
        """A bf16 rounding point of the kernel (MFMA operand or store)."""
        if not self.ref:
            return Q(self.v.bfloat16().float())
        return Q(self.v, self.t + half_ulp_bf16(self.v.abs() + self.t))

    def relu(self):
        return Q(self.v.clamp_min(0), self.t)

    def rsq(self):
        if not self.ref:
            return Q(self.v.rsqrt())
        v = self.v ** -0.5
        return Q(v, 0.5 * v / self.v * self.t + T["rsq"] * U * v)

    def exp2(self):
        if not self.ref:
            return Q(torch.exp2(self.v))
        v = torch.exp2(self.v)
        return Q(v, v * (math.log(2.0) * self.t + T["exp2"] * U) + TINY)

    def log2(self):
        if not self.ref:
            return Q(torch.log2(self.v))
        v = torch.log2(self.v)
        return Q(v, self.t / (self.v * math.log(2.0)) + T["log2"] * U * v.abs())

    def recip(self):
        if not self.ref:
            return Q(1.0 / self.v)
        v = 1.0 / self.v
        return Q(v, self.t * v * v + 4 * U * v.abs())

    def _map(self, fn):
        return Q(fn(self.v), None if self.t is None else fn(self.t))

    def T_(self):
        return self._map(lambda x: x.transpose(-1, -2))

    def reshape(self, *s):
        return self._map(lambda x: x.reshape(*s))

    def permute(self, *s):
        return self._map(lambda x: x.permute(*s))

    def __getitem__(self, i):
        return self._map(lambda x: x[i])

    def out(self):
        return (self.v, self.t) if self.ref else self.v


def lift(x, ref):
    x = torch.as_tensor(x)
    return Q(x.double(), torch.zeros_like(x, dtype=torch.float64)) if ref else Q(x.float())


def qcat(qs, dim):
    return Q(torch.cat([q.v for q in qs], dim), None if qs[0].t is None else torch.cat([q.t for q in qs], dim))


def qstack(qs, dim):
    return Q(torch.stack([q.v for q in qs], dim), None if qs[0].t is None else torch.stack([q.t for q in qs], dim))


def outs(d):
    return {k: (v.out() if isinstance(v, Q) else v) for k, v in d.items()}


def sub(c, idx):
    """The case restricted to clients ``idx`` (every tensor named in ``c.CT`` has the client axis first)."""
    d = dict(vars(c))
    for n in c.CT:
        if d[n] is not None:
            d[n] = d[n][idx].clone()
    d["C"] = len(idx)
    d["clients"] = [c.clients[i] for i in idx]
    return NS(**d)


def _case(**kw):
    c = NS(**kw)
    c.clients = list(range(c.C))
    c.rep = 1
    return c


def replicate(c, n):
    """The case with its clients repeated n times along the client axis (same seeds: ``clients`` repeats too).  Used
    where only MANY clients reach a path (the forward row passes' grid cap of 256 / C workgroups per client): the
    references are computed once on the base case."""
    d = dict(vars(c))
    for name in c.CT:
        if d[name] is not None:
            d[name] = d[name].repeat(n, *([1] * (d[name].dim() - 1)))
    d["C"], d["clients"], d["rep"] = c.C * n, c.clients * n, 1
    return NS(**d)


def guarded(shape, dtype, dev, fill=PRE, guard=256):
    """A prefilled device tensor of ``shape`` that is the head of a longer prefilled buffer -> (tensor, buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + guard,), fill, dtype=dtype, device=dev)
    return buf[:n].view(*shape), buf


def tail(buf, t, fill=PRE):
    """(the guard elements after tensor ``t`` in its buffer, the prefill they must still hold)"""
    return buf[t.numel():].cpu(), fill


def param_row(C, blocks, g, odd=True):
    """A synthetic parameter table ``[C, P]``: the blocks ``(n, scale, base)`` in order, each one float after the
    previous (offsets not 16-byte aligned), the gaps NaN (a read outside a block poisons the result), P odd."""
    offs, o = [], 1
    for n, _, _ in blocks:
        offs.append(o)
        o += n + 1
    P = o + (1 if (o % 2 == 0) == odd else 0)
    p = torch.full((C, P), float("nan"))
    for (n, sc, base), off in zip(blocks, offs):
        p[:, off:off + n] = base + sc * torch.randn(C, n, generator=g)
    return p, offs


# ================================================================================================ stem
def stem_case(L, B, C=3):
    g = gen(1, L, B)
    params, (w_off, b_off, pe_off) = param_row(C, [(192, 0.5, 0.0), (64, 0.5, 0.0), (64 * L, 1.0, 0.0)], g)
    return _case(name=f"stem L{L} B{B}", C=C, B=B, L=L, x=bfx(torch.randn(C, B, L, generator=g)), params=params,
                 w_off=w_off, b_off=b_off, pe_off=pe_off, CT=["x", "params"])


def cases_stem():
    # (B L straddles the 32-row block: R = 1 .. 99; the two long rows once, at B = 1)
    return [stem_case(L, B) for L in (1, 2, 3, 31, 32, 33, 561, 600) for B in (1, 3) if not (L > 33 and B > 1)]


def f_stem(c, ref, mut=None):
    C, B, L = c.x.shape
    w = c.params[:, c.w_off:c.w_off + 192].reshape(C, 64, 3)
    b = c.params[:, c.b_off:c.b_off + 64]
    pe = c.params[:, c.pe_off:c.pe_off + 64 * L].reshape(C, L, 64)
    if mut == "pe_row_plus_1":
        pe = torch.roll(pe, -1, 1)
    xm, xp = torch.zeros_like(c.x), torch.zeros_like(c.x)
    xm[:, :, 1:], xp[:, :, :-1] = c.x[:, :, :-1], c.x[:, :, 1:]
    if mut == "taps_not_padded":  # l = 0 / l = L - 1 read the neighbouring sample's element
        flat = c.x.reshape(C, B * L)
        xm, xp = torch.roll(flat, 1, 1).reshape(C, B, L), torch.roll(flat, -1, 1).reshape(C, B, L)
    q = lambda t: lift(t, ref)
    s = q(b)[:, None, None, :] + q(pe)[:, None]
    s = s + q(w[:, :, 0])[:, None, None, :] * q(xm)[..., None]
    s = s + q(w[:, :, 1])[:, None, None, :] * q(c.x)[..., None]
    s = s + q(w[:, :, 2])[:, None, None, :] * q(xp)[..., None]
    return outs({"h": s.bf().reshape(C, B * L, 64)})


def composite_stem(c):
    h = torch.zeros(c.C, c.B * c.L, 64)
    Lx.conv_pe_fwd(c.x, torch.nan_to_num(c.params), c.w_off, c.b_off, c.pe_off, h)
    return {"h": h}


def run_stem(c, dev):
    out, buf = guarded((c.C, c.B * c.L, 64), torch.bfloat16, dev)
    Lx._native().har_stem(c.x.to(dev), c.params.to(dev), c.w_off, c.b_off, c.pe_off, out)
    return {"h": out.cpu()}, {"h_tail": tail(buf, out)}


# ================================================================================================ pool
def pool_case(L, C=3):
    B = 1 if L == 561 else 2
    y = bfx(torch.randn(C, B * L, 64, generator=gen(2, L)) + 0.5)
    return _case(name=f"pool L{L}", C=C, B=B, L=L, y=y, CT=["y"])


def cases_pool():
    return [pool_case(L) for L in (1, 31, 32, 33, 63, 64, 65, 95, 97, 561)]


def f_pool(c, ref, mut=None):
    C = c.y.shape[0]
    s = lift(c.y, ref).reshape(C, c.B, c.L, 64).sum(2)
    div = ceil64(c.L) if mut == "pool_div_Lp" else c.L
    return outs({"pool": s * lift(torch.tensor(f32(1.0 / div)), ref)})


def composite_pool(c):
    out = torch.zeros(c.C, c.B, 64)
    Lx.mean_rows_fwd(c.y, c.B, c.L, out)
    return {"pool": out}


def run_pool(c, dev):
    out, buf = guarded((c.C, c.B, 64), torch.float32, dev)
    Lx._native().har_pool(c.y.to(dev).bfloat16(), c.B, c.L, out)
    return {"pool": out.cpu()}, {"pool_tail": tail(buf, out)}


# ================================================================================================ reduce
def reduce_case(G, n, segs, P, C=3):
    return _case(name=f"reduce G{G} n{n}", C=C, G=G, n=n, segs=segs, P=P, ws=torch.randn(C, G, n, generator=gen(3, G, n)),
                 CT=["ws"])


def cases_reduce():
    # segments (ws offset, parameter offset, n): a gap between segments (100 .. 129 of ws belong to none), n not a
    # multiple of 256, a one-element segment, G = 1
    return [reduce_case(1, 300, [(0, 5, 100), (130, 200, 170)], 401), reduce_case(3, 300, [(0, 5, 100), (130, 200, 170)], 401),
            reduce_case(32, 1000, [(0, 0, 256), (256, 300, 1), (300, 600, 700)], 1301), reduce_case(2, 7, [(2, 1, 3)], 9)]


def f_reduce(c, ref, mut=None):
    C = c.ws.shape[0]
    ws = c.ws.double() if ref else c.ws.float()
    G = c.G - 1 if (mut == "reduce_skips_last" and c.G > 1) else c.G
    v = torch.full((C, c.P), PRE, dtype=ws.dtype)
    t = torch.zeros(C, c.P, dtype=torch.float64)
    for wo, po, n in c.segs:
        v[:, po:po + n] = ws[:, :G, wo:wo + n].sum(1)
        t[:, po:po + n] = (c.G + 1) * U * c.ws[:, :, wo:wo + n].double().abs().sum(1)
    return {"grads": (v, t) if ref else v}


def run_reduce(c, dev):
    grads, buf = guarded((c.C, c.P), torch.float32, dev)
    ws = torch.full((c.C * c.G * c.n + 5,), WS_PRE, device=dev)  # (beyond the partials: must not be summed)
    ws[:c.C * c.G * c.n] = c.ws.reshape(-1).to(dev)
    Lx._native().har_reduce(ws, c.G, c.n, torch.tensor(c.segs, dtype=torch.int32, device=dev), grads)
    return {"grads": grads.cpu()}, {"grads_tail": tail(buf, grads)}


# ================================================================================================ q | k | v
# (B, L): R = 1, 15, 16, 17, 63, 64, 65, 127, 129, 35 (L = 5: a 16-row tile spans four samples) and 561
R_SET = [(1, 1), (3, 5), (1, 16), (1, 17), (7, 9), (1, 64), (5, 13), (1, 127), (3, 43), (7, 5), (1, 561)]
# Two tiles per wave in the forward row passes: the launcher gives a client min(ceil(tiles / 8), 256 / C, 64)
# workgroups, so only many clients make a wave loop.  26 clients (2 distinct, replicated 13 times): 9 workgroups each;
# q|k|v (8 waves): R = 2440 = 153 tiles over 72 waves; post (16 waves): R = 4636 = 290 tiles over 144 waves
TWO_TILE_REP = 13


def qkv_case(B, L, Lp, C=2):
    g = gen(4, B, L, Lp)
    params, (w_off, b_off) = param_row(C, [(192 * 64, 0.15, 0.0), (192, 0.3, 0.0)], g)
    return _case(name=f"qkv B{B} L{L} Lp{Lp}", C=C, B=B, L=L, Lp=Lp, x=bfx(torch.randn(C, B * L, 64, generator=g)),
                 params=params, w_off=w_off, b_off=b_off, CT=["x", "params"])


def cases_qkv():
    out = []
    for (B, L) in R_SET + [(40, 61)]:
        for Lp in ((64, 128) if L <= 64 else (ceil64(L),)):
            if Lp == 128 and B * L not in (15, 35, 64):
                continue
            out.append(qkv_case(B, L, Lp))
            if (B, L) == (40, 61):
                out[-1].rep = TWO_TILE_REP
    return out


def to_headmajor(z, B, L):
    """[C, B*L, 192] -> [C, B, 4, 3, L, 16]"""
    return z.reshape(z.v.shape[0] if isinstance(z, Q) else z.shape[0], B, L, 3, 4, 16).permute(0, 1, 4, 3, 2, 5)


def from_headmajor(hm, L):
    """[C, B, 4, 3, Lp, 16] -> [C, B*L, 192] of the valid rows"""
    C, B = hm.shape[0], hm.shape[1]
    return hm[:, :, :, :, :L].permute(0, 1, 4, 3, 2, 5).reshape(C, B * L, 192)


def f_qkv(c, ref, mut=None):
    C = c.x.shape[0]
    W = bfx(c.params[:, c.w_off:c.w_off + 192 * 64].reshape(C, 192, 64))  # build_img
    b = c.params[:, c.b_off:c.b_off + 192]
    q = lambda t: lift(t, ref)
    z = q(c.x).mm(q(W).T_()) + q(b)[:, None, :]
    sc = torch.ones(192)
    sc[:64] = QS
    if mut == "qscale_on_k":
        sc[:64], sc[64:128] = 1.0, QS
    if mut == "qscale_missing":
        sc[:] = 1.0
    hm = to_headmajor((z * q(sc)).bf(), c.B, c.L)
    if mut == "head_columns_swapped":
        hm = hm[:, :, [1, 0, 3, 2]]
    return outs({"qkv": hm})


def run_qkv(c, dev):
    qkv = torch.full((c.C * c.B * 4, 3, c.Lp, 16), PRE, dtype=torch.bfloat16, device=dev)
    Lx._native().har_qkv(c.x.to(dev).bfloat16(), c.params.to(dev), c.w_off, c.b_off, qkv, c.B, c.L, 0.25 * 1.4426950408889634)
    full = qkv.cpu().reshape(c.C, c.B, 4, 3, c.Lp, 16)
    return {"qkv": full[..., :c.L, :]}, {"qkv_pad": (full[..., c.L:, :], PRE)}


# ================================================================================================ attention
ATTN_L = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 561)


def keep_rc_grid(c, ncols=None):
    """bool [C, B, 4, L, ncols] keep flags of the attention probabilities (rows (b 4 + h) L + q)."""
    L = c.L
    rows = (np.arange(c.B * 4)[:, None] * L + np.arange(L)[None, :]).reshape(c.B, 4, L, 1)
    cols = np.arange(ncols or L).reshape(1, 1, 1, -1)
    return torch.stack([masks.keep_rc(key_of(ci, c.step), c.layer, rows, cols, c.p) for ci in c.clients])


def attn_case(L, p, kind="rand", Lp=None, C=2, B=None, seed=0):
    B = B or (1 if L >= 191 else 2)
    Lp = Lp or ceil64(L)
    g = gen(5, L, int(p * 100), seed, Lp)
    z = torch.randn(C, B * L, 192, generator=g)
    if kind == "flat":
        z[:, :, :64] = 0.0
    if kind == "saturated":  # key 0 wins every row by ~60 in the log2 domain: q = 4 e0 (x QS), k0 = 11 e0, others 0 on e0
        z[:, :, :128] *= 0.05
        z[:, :, 0:64:16] = 4.0
        zz = z.reshape(C, B, L, 192)
        zz[:, :, :, 64:128:16] = 0.0
        zz[:, :, 0, 64:128:16] = 42.0
    if kind == "const_v":  # every value row within a few bf16 ulps of one vector: O is NOT bf16-exact and dP ~ Delta
        zz = z.reshape(C, B, L, 192)
        v0 = bfx(zz[:, :, :1, 128:].clone())
        step_ = torch.ldexp(torch.ones_like(v0), torch.frexp(v0)[1] - 8)  # one bf16 ulp of v0
        zz[:, :, :, 128:] = v0 + step_ * torch.randint(-2, 3, (C, B, L, 64), generator=g).float()
    z[:, :, :64] *= QS
    hm = torch.full((C, B, 4, 3, Lp, 16), 0.75)  # padding rows: a finite, non-zero, bf16-exact prefill
    hm[..., :L, :] = to_headmajor(bfx(z), B, L)
    c = _case(name=f"attn L{L} Lp{Lp} p{p} {kind}", C=C, B=B, L=L, Lp=Lp, p=p, step=3, layer=10, qkv=hm,
              dout=bfx(torch.randn(C, B * L, 64, generator=g)), CT=["qkv", "dout", "lse2", "delta"], lse2=None, delta=None)
    # the backward's inputs: the forward's lse2 (fp32) and Delta = rowsum(dO o O) of the STORED bf16 O, as k_har_post_bwd
    # computes it — both from the fp32 model of the forward
    m = f_attn_fwd(c, False)
    c.lse2 = m["lse2"].float()
    c.delta = (c.dout * m["o"]).reshape(C, B, L, 4, 16).sum(-1).permute(0, 1, 3, 2).contiguous().float()
    return c


_ATTN = {}


def cases_attn():
    if "c" not in _ATTN:
        out = [attn_case(L, (0.0, 0.1, 0.5)[i % 3]) for i, L in enumerate(ATTN_L)]
        out += [attn_case(L, p) for L in (33, 65) for p in (0.0, 0.1, 0.5) if not any(
            c.L == L and c.p == p for c in out)]
        out += [attn_case(70, 0.1, "saturated"), attn_case(33, 0.0, "saturated"), attn_case(70, 0.1, "flat"),
                attn_case(17, 0.0, "flat"), attn_case(40, 0.0, "const_v")]
        out += [attn_case(33, 0.1, Lp=128), attn_case(5, 0.5, Lp=192), attn_case(64, 0.1, Lp=128)]  # Lp > ceil64(L)
        out += [attn_case(840, 0.1, Lp=896, C=1, B=1)]  # the largest admitted Lp
        _ATTN["c"] = out
    return _ATTN["c"]


def f_attn_fwd(c, ref, mut=None):
    L, hm = c.L, c.qkv
    q = lambda t: lift(t, ref)
    nk = L + 1 if (mut == "tail_mask_off_by_one" and L < c.Lp) else L  # `> L` instead of `>= L`: key L takes part
    qq, k, v = q(hm[:, :, :, 0, :L]), q(hm[:, :, :, 1, :nk]), q(hm[:, :, :, 2, :nk])
    s = qq.mm(k.T_())
    m = s.v.max(-1, keepdim=True).values  # (the result does not depend on the shift; the kernel's running maximum
    pr = (s - q(m)).exp2()                # and its per-chunk rescales are covered by the sum's n roundings)
    l = pr.sum(-1, keepdim=True)
    lse2 = l.log2() + q(m)
    pd = pr.times(keep_rc_grid(c, nk)) if c.p > 0.0 else pr
    inv = 1.0 if mut == "inv_keep_O" else inv_keep(c.p)
    o = pd.bf().mm(v) * (l.recip() * q(torch.tensor(inv)))
    if mut != "o_not_rounded":  # (not a variant of the forward: the fp32 O that variant 14 of the backward reads)
        o = o.bf()
    C, B = hm.shape[0], hm.shape[1]
    return outs({"o": o.permute(0, 1, 3, 2, 4).reshape(C, B * L, 64), "lse2": lse2[..., 0]})


def attn_composite_inputs(c):
    z = from_headmajor(c.qkv, c.L).clone()
    z[:, :, :64] = z[:, :, :64] / QS
    ctl = NS(key=lambda ci: key_of(c.clients[ci], c.step))
    return z, ctl


def composite_attn_fwd(c):
    z, ctl = attn_composite_inputs(c)
    o, lse = Lx._attn_ref(z, c.B, c.L, ctl, c.layer, c.p, "rc")
    return {"o": o, "lse2": lse / math.log(2.0)}


def f_attn_bwd(c, ref, mut=None):
    L, hm = c.L, c.qkv
    C, B = hm.shape[0], hm.shape[1]
    q = lambda t: lift(t, ref)
    ik = inv_keep(c.p)

    delta = c.delta
    if mut == "delta_from_fp32_O":  # Delta of the forward's fp32 O instead of the stored bf16 O
        o32 = f_attn_fwd(c, False, "o_not_rounded")["o"]
        delta = (c.dout * o32).reshape(C, B, L, 4, 16).sum(-1).permute(0, 1, 3, 2)

    def core(nk):
        qq, k, v = q(hm[:, :, :, 0, :L]), q(hm[:, :, :, 1, :nk]), q(hm[:, :, :, 2, :nk])
        do = q(c.dout.reshape(C, B, L, 4, 16).permute(0, 1, 3, 2, 4))
        pr = (qq.mm(k.T_()) - q(c.lse2)[..., None]).exp2()
        kp = keep_rc_grid(c, nk) if c.p > 0.0 else torch.ones(C, B, 4, L, nk, dtype=torch.bool)
        dp = do.mm(v.T_()).times(kp) * q(torch.tensor(1.0 if mut == "inv_keep_dP" else ik))
        ds = pr * (dp - q(delta)[..., None])
        return qq, k, do, pr.times(kp), ds

    qq, k, do, pd, ds = core(L)
    dv = (pd.bf().T_().mm(do) * q(torch.tensor(1.0 if mut == "inv_keep_dV" else ik))).bf()
    dk = (ds.bf().T_().mm(qq) * q(torch.tensor(1.0 if mut == "iq_missing_dK" else IQ))).bf()
    if mut == "dq_tail_keys_unmasked":  # the keys of the last partial 32-key step up to its end take part in dq
        _, k, _, _, ds = core(min((L + 31) // 32 * 32, c.Lp))
    dq = (ds.bf().mm(k) * q(torch.tensor(1.0 if mut == "quarter_missing_dq" else 0.25))).bf()
    return outs({"dqkv": qstack([dq, dk, dv], 3)})


def composite_attn_bwd(c, dtype=torch.float32):
    z, ctl = attn_composite_inputs(c)
    x = z.to(dtype).requires_grad_(True)
    with torch.enable_grad():
        o, _ = Lx._attn_ref(x, c.B, c.L, ctl, c.layer, c.p, "rc")
        (g,) = torch.autograd.grad(o, x, c.dout.to(dtype))
    # (d(q projection) = 1/4 dS k and d(k projection) = dS^T (q / 4): what the kernel stores, no rescaling)
    return {"dqkv": to_headmajor(g, c.B, c.L)}


def decode_keep_words(words, L, Lp):
    """[Lp/16, Lp/64, 4, 4] int64 ballot words of one (client, sample, head) -> bool [L, L] (query, key) — the decoder
    of tests/test_gpu_har.py."""
    w = words.reshape(Lp // 16, Lp // 64, 4, 4).numpy().view(np.uint64)
    bits = ((w[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    bits = bits.reshape(Lp // 16, Lp // 64, 4, 4, 4, 16)
    return bits.transpose(0, 5, 1, 2, 4, 3).reshape(Lp, Lp)[:L, :L]


def run_attn(c, dev, mask_fill=0):
    """Forward, then the backward on the case's own lse2 / Delta and the forward's keep words."""
    nat = Lx._native()
    C, B, L, Lp = c.C, c.B, c.L, c.Lp
    ctl = make_ctl(max(c.clients) + 1, dev, c.step)
    seeds = ctl.seeds[c.clients].contiguous() if c.p > 0.0 else None
    stepctl = ctl.stepctl if c.p > 0.0 else None
    hm = c.qkv.to(dev).bfloat16().reshape(C * B * 4, 3, Lp, 16)
    o, obuf = guarded((C, B * L, 64), torch.bfloat16, dev)
    lse2 = torch.full((C * B * 4, Lp), PRE, device=dev)
    mask = None
    if c.p > 0.0:
        mask = torch.full((C * B * 4, int(nat.har_mask_words(Lp))), mask_fill, dtype=torch.int64, device=dev)
    nat.har_attn_fwd(hm, o, lse2, B, L, seeds, stepctl, c.layer, c.p, mask)
    lin = torch.full((C, B, 4, Lp), INF, device=dev)
    lin[..., :L] = c.lse2.to(dev)
    delta = torch.full((C, B, 4, Lp), PRE, device=dev)
    delta[..., :L] = c.delta.to(dev)
    dqkv = torch.full((C * B * 4, 3, Lp, 16), PRE, dtype=torch.bfloat16, device=dev)
    nat.har_attn_bwd(hm, lin.reshape(C * B * 4, Lp), c.dout.to(dev).bfloat16(), delta.reshape(C * B * 4, Lp), dqkv, B, L,
                     seeds, stepctl, c.layer, c.p, mask)
    lse_full = lse2.cpu().reshape(C, B, 4, Lp)
    d_full = dqkv.cpu().reshape(C, B, 4, 3, Lp, 16)
    out = {"o": o.cpu(), "lse2": lse_full[..., :L], "dqkv": d_full[..., :L, :]}
    # (the forward writes lse2 = +inf for the padding queries: the backward's exp2(s - inf) = 0 relies on it)
    extra = {"lse2_pad": (lse_full[..., L:], INF), "dqkv_pad": (d_full[..., L:, :], PRE), "o_tail": tail(obuf, o),
             "qkv_after": (hm.cpu().float().reshape(c.qkv.shape), c.qkv),
             "mask": None if mask is None else mask.cpu().reshape(C, B, 4, -1)}
    return out, extra


# ================================================================================================ row passes
def layer_params(C, g, odd=True):
    blocks = [(192 * 64, 0.15, 0.0), (192, 0.3, 0.0), (4096, 0.15, 0.0), (64, 0.3, 0.0), (64, 0.3, 1.0), (64, 0.3, 0.0),
              (16384, 0.15, 0.0), (256, 0.3, 0.0), (16384, 0.08, 0.0), (64, 0.3, 0.0), (64, 0.3, 1.0), (64, 0.3, 0.0)]
    return param_row(C, blocks, g, odd)


def row_keep(c, site, ncols):
    """float [C, R, ncols] 0 / 1 flags of row-pass dropout site 1 (out_proj), 2 (FFN), 3 (linear2)."""
    if c.p <= 0.0:
        return None
    r, cc = np.arange(c.R)[:, None], np.arange(ncols)[None, :]
    return torch.stack([masks.keep(key_of(ci, c.step), c.layer + site, r, cc, c.p) for ci in c.clients])


def encode_kbits(c):
    """int32 [C, R, 16] keep words as k_har_post stores them: lane g's word 0 = site 1 (bit 4t + i = feature
    16t + 4g + i) | site 3 << 16, words 1-2 = the FFN's tiles 0-7 / 8-15, word 3 = 0."""
    k1, kf, k2 = (row_keep(c, s, n).numpy().astype(np.uint32) for s, n in ((1, 64), (2, 256), (3, 64)))
    w = np.zeros((c.C, c.R, 4, 4), dtype=np.uint32)
    for gg in range(4):
        for t in range(16):
            for i in range(4):
                col = 16 * t + 4 * gg + i
                if t < 4:
                    w[:, :, gg, 0] |= (k1[:, :, col] << np.uint32(4 * t + i)) | (k2[:, :, col] << np.uint32(16 + 4 * t + i))
                w[:, :, gg, 1 + (t >> 3)] |= kf[:, :, col] << np.uint32(4 * (t & 7) + i)
    return torch.from_numpy(w.reshape(c.C, c.R, 16).view(np.int32).copy())


def unpack_layer(c, ref):
    C = c.params.shape[0]
    P = lambda i, *s: c.params[:, c.w[i]:c.w[i] + LAYER_SIZES[i]].reshape(C, *s)
    q = lambda t: lift(t, ref)
    return NS(Wo=q(bfx(P(2, 64, 64))), bo=q(P(3, 1, 64)), g1=q(P(4, 1, 64)), be1=q(P(5, 1, 64)), W1=q(bfx(P(6, 256, 64))),
              b1=q(P(7, 1, 256)), W2=q(bfx(P(8, 64, 256))), b2=q(P(9, 1, 64)), g2=q(P(10, 1, 64)), be2=q(P(11, 1, 64)))


def post_case(B, L, p, G=32, dpool=False, C=2, seed=0, near_const=False, Lp=None):
    R = B * L
    g = gen(6, B, L, int(p * 100), seed)
    params, w = layer_params(C, g)
    x = torch.randn(C, R, 64, generator=g)
    if near_const:  # row 0: variance ~ 1e-4 mean^2 (LayerNorm 1 subtracts a mean 100 x the deviations)
        x[:, 0] = 8.0 + 0.08 * torch.randn(C, 64, generator=g)
        params[:, w[3]:w[3] + 64] *= 0.01  # (an out_proj bias of the usual size would be most of that row's variance)
    c = _case(name=f"post B{B} L{L} p{p} G{G}{' dpool' if dpool else ''}{' nearconst' if near_const else ''}", C=C, B=B,
              L=L, R=R, Lp=Lp or ceil64(L), p=p, G=G, step=2, layer=10, params=params, w=w, near_const=near_const,
              o=bfx(0.5 * torch.randn(C, R, 64, generator=g) if not near_const else 0.01 * torch.randn(C, R, 64, generator=g)),
              x=bfx(x), dy=None, dpool=None, CT=["params", "o", "x", "dy", "dpool", "xh1", "xh2", "rs"],
              xh1=None, xh2=None, rs=None)
    if dpool:
        c.dpool = torch.randn(C, B, 64, generator=g)
    else:
        c.dy = torch.randn(C, R, 64, generator=g)
    m = f_post(c, False)  # the backward's saved inputs: the fp32 model's stored values (bf16 xhat, fp32 rstd)
    c.xh1, c.xh2, c.rs = m["xh1"], m["xh2"], m["rs"].float()
    return c


_POST = {}


def cases_post():
    if "c" not in _POST:
        out = []
        ps, Gs = (0.0, 0.1, 0.5), (1, 3, 32)
        for i, (B, L) in enumerate(R_SET[:-1]):
            out.append(post_case(B, L, ps[i % 3], Gs[i % 3], dpool=(L in (1, 5))))
        out += [post_case(70, 1, 0.1, 3, dpool=True), post_case(2, 64, 0.1, 3, dpool=True), post_case(3, 64, 0.5, 1, dpool=True), post_case(26, 5, 0.1, 1, dpool=True),
                post_case(7, 9, 0.1, 1), post_case(3, 43, 0.5, 32), post_case(1, 17, 0.0, 3, near_const=True),
                post_case(1, 561, 0.1, 32), post_case(5, 13, 0.1, 1), post_case(1, 127, 0.0, 32),
                post_case(24, 16, 0.1, 3, seed=1), post_case(3, 43, 0.1, 2, seed=2), post_case(76, 61, 0.1, 32)]
        out[-1].rep = TWO_TILE_REP
        _POST["c"] = out
    return _POST["c"]


def ln_q(s, eps=EPS):
    i64 = f32(1.0 / 64.0)
    mean = s.sum(-1, True) * i64
    d = s - mean
    rstd = ((d * d).sum(-1, True) * i64 + eps).rsq()
    return d * rstd, rstd


def lnb_q(dy, xh, rstd, gamma):
    i64 = f32(1.0 / 64.0)
    g = dy * gamma
    am, bm = g.sum(-1, True) * i64, (g * xh).sum(-1, True) * i64
    return (g - am - xh * bm) * rstd


def drop_q(x, k, inv):
    return x if k is None else x.times(k) * inv


def f_post(c, ref, mut=None):
    q = lambda t: lift(t, ref)
    w = unpack_layer(c, ref)
    k1, kf, k2 = row_keep(c, 1, 64), row_keep(c, 2, 256), row_keep(c, 3, 64)
    inv = {s: (1.0 if mut == f"inv_keep_{s}" else inv_keep(c.p)) for s in ("d1", "df", "d2")}
    a = q(c.o).mm(w.Wo.T_()) + w.bo
    s1 = q(c.x) + drop_q(a, k1, inv["d1"])
    xh1, rs1 = ln_q(s1, f32(1e-6) if mut == "ln_eps_1e-6" else EPS)
    h1 = xh1 * w.g1 + w.be1
    z = h1.bf().mm(w.W1.T_()) + w.b1
    f = drop_q(z.relu(), kf, inv["df"])
    s2 = h1 + drop_q(f.bf().mm(w.W2.T_()) + w.b2, k2, inv["d2"])
    xh2, rs2 = ln_q(s2, f32(1e-6) if mut == "ln_eps_1e-6" else EPS)
    y = xh2 * w.g2 + w.be2
    rs = qcat([rs2, rs1] if mut == "rs_slots_swapped" else [rs1, rs2], -1)
    return outs({"xh1": xh1.bf(), "xh2": xh2.bf(), "rs": rs, "y": y.bf()})


def run_post(c, dev):
    nat = Lx._native()
    C, R = c.C, c.R
    bf = torch.bfloat16
    ctl = make_ctl(max(c.clients) + 1, dev, c.step)
    seeds = ctl.seeds[c.clients].contiguous() if c.p > 0.0 else None
    (xh1, b1), (xh2, b2), (y, b3) = (guarded((C, R, 64), bf, dev) for _ in range(3))
    rs, b4 = guarded((C, R, 2), torch.float32, dev)
    kb = torch.full((C, R, 16), -1, dtype=torch.int32, device=dev) if c.p > 0.0 else None
    nat.har_post(c.o.to(dev).bfloat16(), c.x.to(dev).bfloat16(), xh1, xh2, rs, y, c.params.to(dev), c.w, seeds,
                 ctl.stepctl if c.p > 0.0 else None, c.layer, c.p, kb)
    return ({"xh1": xh1.cpu(), "xh2": xh2.cpu(), "rs": rs.cpu(), "y": y.cpu()},
            {"kbits": None if kb is None else kb.cpu(), "xh1_tail": tail(b1, xh1), "xh2_tail": tail(b2, xh2),
             "y_tail": tail(b3, y), "rs_tail": tail(b4, rs)})


def partial_rows(R, G, g, mut=None):
    """Row indices that workgroup g of G serves: the 64-row blocks blk = g, g + G, ..."""
    nblk = (R + 63) // 64
    rows = []
    for blk in range(g, nblk, G):
        lo, hi = 64 * blk, min(R, 64 * blk + 64)
        if mut == "last_partial_block_dropped" and hi - lo < 64 and blk == nblk - 1:
            continue
        rows += list(range(lo, hi))
        if mut == "padding_rows_contribute" and hi - lo < 64 and blk == nblk - 1:
            rows += [0] * (64 - (hi - lo))  # the padding lanes take row 0's inputs instead of zeros
    return rows


def stale_group(R, G):
    """An idle workgroup (no 64-row block of its own), or None."""
    nblk = (R + 63) // 64
    return G - 1 if G > nblk else None


def f_post_bwd(c, ref, mut=None):
    q = lambda t: lift(t, ref)
    w = unpack_layer(c, ref)
    C, R, B, L = c.params.shape[0], c.R, c.B, c.L
    k1, kf, k2 = row_keep(c, 1, 64), row_keep(c, 2, 256), row_keep(c, 3, 64)
    inv = {s: (1.0 if mut == f"bwd_inv_keep_{s}" else inv_keep(c.p)) for s in ("d1", "df", "d2")}
    if c.dpool is not None:
        dy = q(c.dpool)[:, :, None, :] * q(torch.tensor(f32(1.0 / L)))
        dy = Q(dy.v.expand(C, B, L, 64).reshape(C, R, 64), None if not ref else dy.t.expand(C, B, L, 64).reshape(C, R, 64))
    else:
        dy = q(c.dy)
    xh1, xh2 = q(c.xh1), q(c.xh2)
    rs1, rs2 = q(c.rs[..., 0:1]), q(c.rs[..., 1:2])
    if mut == "bwd_rs_slots_swapped":
        rs1, rs2 = rs2, rs1
    ds2 = lnb_q(dy, xh2, rs2, w.g2)
    df2 = drop_q(ds2, k2, inv["d2"])
    h1 = xh1 * w.g1 + w.be1
    z = h1.bf().mm(w.W1.T_()) + w.b1
    f = drop_q(z.relu(), kf, inv_keep(c.p))
    pos = (z.v > 0)
    dfu = drop_q(df2.bf().mm(w.W2), kf, inv["df"])
    dfz = dfu.times(pos)
    if ref:  # a pre-activation within its own bound of zero may take either side of ReLU'
        dfz = Q(dfz.v, torch.where(z.v.abs() <= z.t, dfz.t + dfu.v.abs() + dfu.t, dfz.t))
    dh1 = dfz.bf().mm(w.W1) + ds2
    ds1 = lnb_q(dh1, xh1, rs1, w.g1)
    da = drop_q(ds1, k1, inv["d1"])
    dout = da.bf().mm(w.Wo).bf()
    o = q(c.o)
    delta = (dout * o).reshape(C, B, L, 4, 16).sum(-1).permute(0, 1, 3, 2)  # [C, B, 4, L]
    # ---- per-workgroup partials
    fb, df2b, dfzb, h1b, dab = f.bf(), df2.bf(), dfz.bf(), h1.bf(), da.bf()
    parts = []
    for g in range(c.G):
        rows = partial_rows(R, c.G, g, mut)
        if not rows:
            z0 = torch.zeros(C, POST_NG, dtype=torch.float64 if ref else torch.float32)
            parts.append(Q(z0, torch.zeros_like(z0) if ref else None))
            continue
        S = lambda x: x[:, rows]
        pieces = [S(dab).T_().mm(S(o)).reshape(C, -1), S(dfzb).T_().mm(S(h1b)).reshape(C, -1),
                  S(df2b).T_().mm(S(fb)).reshape(C, -1), S(da).sum(1), S(dh1 * xh1).sum(1), S(dh1).sum(1), S(dfz).sum(1),
                  S(df2).sum(1), S(dy * xh2).sum(1), S(dy).sum(1)]
        parts.append(qcat(pieces, -1))
    ws = qstack(parts, 1)  # [C, G, NG]
    sg = stale_group(R, c.G)
    if mut == "idle_partial_stale" and sg is not None:
        ws.v[:, sg] = WS_PRE
    return outs({"dres": ds1, "dout": dout, "delta": delta, "ws": ws})


def run_post_bwd(c, dev, ws=None):
    nat = Lx._native()
    C, R, B, L, Lp = c.C, c.R, c.B, c.L, c.Lp
    bf = torch.bfloat16
    ctl = make_ctl(max(c.clients) + 1, dev, c.step)
    drop = c.p > 0.0
    seeds = ctl.seeds[c.clients].contiguous() if drop else None
    dres, b1 = guarded((C, R, 64), torch.float32, dev)
    dout, b2 = guarded((C, R, 64), bf, dev)
    delta = torch.full((C * B * 4, Lp), PRE, device=dev)
    if ws is None:
        ws = torch.full((C * c.G * POST_NG + 64,), WS_PRE, device=dev)
    kb = encode_kbits(c).to(dev) if drop else None
    nat.har_post_bwd(None if c.dy is None else c.dy.to(dev), None if c.dpool is None else c.dpool.to(dev), B, L,
                     c.o.to(dev).bfloat16(), c.xh1.to(dev).bfloat16(), c.xh2.to(dev).bfloat16(), c.rs.to(dev), dres, dout,
                     delta, ws, c.params.to(dev), c.w, seeds, ctl.stepctl if drop else None, c.layer, c.p, c.G, kb)
    dl = delta.cpu().reshape(C, B, 4, Lp)
    wsc = ws.cpu()
    return ({"dres": dres.cpu(), "dout": dout.cpu(), "delta": dl[..., :L], "ws": wsc[:C * c.G * POST_NG].reshape(C, c.G, POST_NG)},
            {"delta_pad": (dl[..., L:], PRE), "ws_tail": (wsc[C * c.G * POST_NG:], WS_PRE), "dres_tail": tail(b1, dres),
             "dout_tail": tail(b2, dout)})


# ---- q | k | v backward
def qkvb_case(B, L, G, Lp=None, C=2, seed=0):
    R, Lp = B * L, Lp or ceil64(L)
    g = gen(7, B, L, G, seed)
    params, w = layer_params(C, g)
    hm = torch.full((C, B, 4, 3, Lp, 16), PRE)
    hm[..., :L, :] = to_headmajor(bfx(torch.randn(C, R, 192, generator=g)), B, L)
    return _case(name=f"qkv_bwd B{B} L{L} Lp{Lp} G{G}", C=C, B=B, L=L, R=R, Lp=Lp, G=G, params=params, w_off=w[0], dqkv=hm,
                 dres=torch.randn(C, R, 64, generator=g), x=bfx(torch.randn(C, R, 64, generator=g)),
                 CT=["params", "dqkv", "dres", "x"])


_QKVB = {}


def cases_qkv_bwd():
    if "c" not in _QKVB:
        Gs = (1, 2, 64)
        out = [qkvb_case(B, L, Gs[i % 3]) for i, (B, L) in enumerate(R_SET)]
        out += [qkvb_case(3, 43, 1), qkvb_case(3, 43, 2, seed=1), qkvb_case(1, 64, 2), qkvb_case(3, 5, 1, Lp=128),
                qkvb_case(7, 5, 2, Lp=128), qkvb_case(13, 61, 2), qkvb_case(1, 17, 64), qkvb_case(2, 100, 2),
                qkvb_case(70, 61, 64)]  # R = 4270 > 64 G: three workgroups serve two blocks
        _QKVB["c"] = out
    return _QKVB["c"]


def f_qkv_bwd(c, ref, mut=None):
    q = lambda t: lift(t, ref)
    C = c.params.shape[0]
    W = q(bfx(c.params[:, c.w_off:c.w_off + 192 * 64].reshape(C, 192, 64)))
    d, x = q(from_headmajor(c.dqkv, c.L)), q(c.x)
    dx = d.mm(W)
    if mut != "dres_not_added":
        dx = q(c.dres) + dx
    parts = []
    for g in range(c.G):
        rows = partial_rows(c.R, c.G, g, mut)
        if not rows:
            z0 = torch.zeros(C, QKV_NG, dtype=torch.float64 if ref else torch.float32)
            parts.append(Q(z0, torch.zeros_like(z0) if ref else None))
            continue
        parts.append(qcat([d[:, rows].T_().mm(x[:, rows]).reshape(C, -1), d[:, rows].sum(1)], -1))
    ws = qstack(parts, 1)
    sg = stale_group(c.R, c.G)
    if mut == "idle_partial_stale" and sg is not None:
        ws.v[:, sg] = WS_PRE
    return outs({"dx": dx, "ws": ws})


def run_qkv_bwd(c, dev):
    C, R, G = c.C, c.R, c.G
    dx, b1 = guarded((C, R, 64), torch.float32, dev)
    ws = torch.full((C * G * QKV_NG + 64,), WS_PRE, device=dev)
    Lx._native().har_qkv_bwd(c.dqkv.to(dev).bfloat16().reshape(C * c.B * 4, 3, c.Lp, 16), c.dres.to(dev),
                             c.x.to(dev).bfloat16(), dx, ws, c.params.to(dev), c.w_off, c.B, c.L, G)
    wsc = ws.cpu()
    return ({"dx": dx.cpu(), "ws": wsc[:C * G * QKV_NG].reshape(C, G, QKV_NG)},
            {"ws_tail": (wsc[C * G * QKV_NG:], WS_PRE), "dx_tail": tail(b1, dx)})


# ================================================================================================ the kernel table
KERNELS = {
    "stem": NS(cases=cases_stem, f=f_stem, composite=composite_stem, run=run_stem),
    "pool": NS(cases=cases_pool, f=f_pool, composite=composite_pool, run=run_pool),
    "reduce": NS(cases=cases_reduce, f=f_reduce, composite=None, run=run_reduce),
    "qkv": NS(cases=cases_qkv, f=f_qkv, composite=None, run=run_qkv),
    "attn_fwd": NS(cases=cases_attn, f=f_attn_fwd, composite=composite_attn_fwd, run=run_attn),
    # bwd_kv (dk, dv) and bwd_dq (dq).  The backward READS Delta of the stored bf16 O and the forward's fp32 lse2; the
    # composite's autograd uses its own unrounded O, so it is held to the formula in float64 instead
    # (test_attn_bwd_formula_is_the_forward_derivative), like the two backward row passes
    "attn_bwd": NS(cases=cases_attn, f=f_attn_bwd, composite=None, run=run_attn),
    "post": NS(cases=cases_post, f=f_post, composite=None, run=run_post),
    "post_bwd": NS(cases=cases_post, f=f_post_bwd, composite=None, run=run_post_bwd),
    "qkv_bwd": NS(cases=cases_qkv_bwd, f=f_qkv_bwd, composite=None, run=run_qkv_bwd),
}
# every variant must leave the bound of its kernel on at least one case (numbers: the issue's list)
MUTANTS = {
    "stem": ["pe_row_plus_1", "taps_not_padded"],                                               # 11, 12
    "pool": ["pool_div_Lp"],                                                                    # 13
    "reduce": ["reduce_skips_last"],
    "qkv": ["qscale_on_k", "qscale_missing", "head_columns_swapped"],                           # 7, 17
    "attn_fwd": ["inv_keep_O", "tail_mask_off_by_one"],                                         # 1, 2
    "attn_bwd": ["inv_keep_dV", "inv_keep_dP", "dq_tail_keys_unmasked", "iq_missing_dK", "quarter_missing_dq",  # 1, 3, 8
                 "delta_from_fp32_O"],                                                          # 14
    "post": ["inv_keep_d1", "inv_keep_df", "inv_keep_d2", "ln_eps_1e-6", "rs_slots_swapped"],   # 1, 9, 10
    "post_bwd": ["bwd_inv_keep_d1", "bwd_inv_keep_df", "bwd_inv_keep_d2", "bwd_rs_slots_swapped",  # 1, 10
                 "last_partial_block_dropped", "padding_rows_contribute", "idle_partial_stale"],   # 4, 5, 6
    "qkv_bwd": ["dres_not_added", "last_partial_block_dropped", "idle_partial_stale"],          # 15, 4, 6
}


def packing_cases():
    """One small five-client case per kernel (more than one block or tile per client, dropout on)."""
    post = post_case(3, 43, 0.1, 3, C=5, seed=5)
    attn = attn_case(33, 0.1, C=5, seed=5)
    return {"stem": stem_case(33, 3, C=5), "pool": pool_case(65, C=5),
            "reduce": reduce_case(3, 300, [(0, 5, 100), (130, 200, 170)], 401, C=5), "qkv": qkv_case(3, 43, 192, C=5),
            "attn_fwd": attn, "attn_bwd": attn, "post": post, "post_bwd": post, "qkv_bwd": qkvb_case(3, 43, 2, C=5, seed=5)}


def poison_client(c, ci=1):
    """The case with every input of client ``ci`` (its parameters included) NaN."""
    d = dict(vars(c))
    for name in c.CT:
        if d[name] is not None:
            d[name] = d[name].clone()
            d[name][ci] = float("nan")
    return NS(**d)


def ref_of(kernel, c):
    return KERNELS[kernel].f(c, True)


def model_of(kernel, c, mut=None):
    return KERNELS[kernel].f(c, False, mut)


# ref_stem(c), model_stem(c, mut=None), ... : the two modes of each formula under the names of the sibling suites
for _k in KERNELS:
    globals()[f"ref_{_k}"] = (lambda k: lambda c: ref_of(k, c))(_k)
    globals()[f"model_{_k}"] = (lambda k: lambda c, mut=None: model_of(k, c, mut))(_k)


# ================================================================================================ CPU tests
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_model_and_composite_within_bound(kernel):
    k = KERNELS[kernel]
    top = 0.0
    for c in k.cases():
        ref = ref_of(kernel, c)
        top = max(top, check(model_of(kernel, c), ref, f"model {c.name}"))
        if k.composite is not None:
            top = max(top, check(k.composite(c), ref, f"composite {c.name}"))
    print(f"{kernel}: worst err/bound {top:.3g}")


@pytest.mark.parametrize("kernel,mut", [(k, m) for k, ms in MUTANTS.items() for m in ms])
def test_mutant_leaves_bound(kernel, mut):
    caught = []
    for c in KERNELS[kernel].cases():
        ref = ref_of(kernel, c)
        res = {n: ratio(v, *ref[n]) for n, v in model_of(kernel, c, mut).items()}
        if any(not r <= 1.0 for r in res.values()):
            caught.append(c.name)
    print(f"{kernel}/{mut}: caught at {len(caught)} cases, e.g. {caught[:3]}")
    assert caught, f"no case catches {kernel}/{mut}: a case is missing"


def _f64_post(c, o, x):
    """The row pass's forward in float64 torch (autograd-able), no bf16 anywhere but the weights' images."""
    w = unpack_layer(c, True)
    k1, kf, k2 = row_keep(c, 1, 64), row_keep(c, 2, 256), row_keep(c, 3, 64)
    ik = inv_keep(c.p)
    d = lambda t, k: t if k is None else t * k.double() * ik

    def ln(s):
        dd = s - s.mean(-1, keepdim=True)
        r = (dd.pow(2).mean(-1, keepdim=True) + EPS).rsqrt()
        return dd * r, r

    s1 = x + d(o @ w.Wo.v.transpose(1, 2) + w.bo.v, k1)
    xh1, r1 = ln(s1)
    h1 = xh1 * w.g1.v + w.be1.v
    f = d(torch.relu(h1 @ w.W1.v.transpose(1, 2) + w.b1.v), kf)
    s2 = h1 + d(f @ w.W2.v.transpose(1, 2) + w.b2.v, k2)
    xh2, r2 = ln(s2)
    return xh2 * w.g2.v + w.be2.v, xh1, xh2, torch.cat([r1, r2], -1)


def test_post_bwd_formula_is_the_forward_derivative():
    """f_post_bwd's VALUE path against float64 autograd of the forward, fed the forward's unrounded saved tensors."""
    for c in cases_post():
        if c.near_const or c.R > 200:
            continue
        o = c.o.double().requires_grad_(True)
        x = c.x.double().requires_grad_(True)
        prm = c.params.double().requires_grad_(False)
        with torch.enable_grad():
            y, xh1, xh2, rs = _f64_post(c, o, x)
            dy = c.dy.double() if c.dy is not None else (c.dpool.double()[:, :, None, :] / c.L).expand(
                c.C, c.B, c.L, 64).reshape(c.C, c.R, 64)
            go, gx = torch.autograd.grad(y, (o, x), dy)
        d = dict(vars(c))
        d.update(xh1=xh1.detach(), xh2=xh2.detach(), rs=rs.detach())
        if c.dpool is not None:
            d.update(dpool=c.dpool.double())
        got = f_post_bwd(NS(**d), True)
        # d(x) = the residual path's ds1; d(o) = dout
        for name, want in (("dres", gx), ("dout", go)):
            v = got[name][0]
            err = (v - want).abs().max().item() / (want.abs().max().item() + 1e-30)
            assert err < 1e-5, (c.name, name, err)  # (1/L and inv_keep are the kernel's fp32 constants)
        del prm


def test_qkv_bwd_formula_is_the_forward_derivative():
    for c in cases_qkv_bwd()[:6]:
        W = bfx(c.params[:, c.w_off:c.w_off + 192 * 64].reshape(c.C, 192, 64)).double().requires_grad_(True)
        x = c.x.double().requires_grad_(True)
        d = from_headmajor(c.dqkv, c.L).double()
        with torch.enable_grad():
            z = x @ W.transpose(1, 2)
            gx, gW = torch.autograd.grad(z, (x, W), d)
        got = f_qkv_bwd(c, True)
        assert torch.allclose(got["dx"][0], gx + c.dres.double(), rtol=1e-12, atol=1e-12)
        assert torch.allclose(got["ws"][0].sum(1)[:, :192 * 64].reshape(c.C, 192, 64), gW, rtol=1e-10, atol=1e-10)
        assert torch.allclose(got["ws"][0].sum(1)[:, 192 * 64:], d.sum(1), rtol=1e-10, atol=1e-10)


def test_attn_bwd_formula_is_the_forward_derivative():
    """float64: f_attn_bwd on the float64 forward's lse2 / Delta equals autograd of the composite."""
    for c in cases_attn():
        if c.L > 70:
            continue
        fw = f_attn_fwd(c, True)
        d = dict(vars(c))
        d["lse2"] = fw["lse2"][0]
        d["delta"] = (c.dout.double() * fw["o"][0]).reshape(c.C, c.B, c.L, 4, 16).sum(-1).permute(0, 1, 3, 2)
        got = f_attn_bwd(NS(**d), True)["dqkv"][0]
        want = composite_attn_bwd(c, torch.float64)["dqkv"]
        err = (got - want).abs().max().item() / (want.abs().max().item() + 1e-30)
        assert err < 1e-5, (c.name, err)


def test_keep_word_decoder_and_kbits_encoder_roundtrip():
    c = post_case(1, 17, 0.5)
    w = encode_kbits(c).numpy().view(np.uint32).reshape(c.C, c.R, 4, 4)
    k1 = row_keep(c, 1, 64).numpy()
    for gg in range(4):
        for t in range(4):
            for i in range(4):
                assert ((w[:, :, gg, 0] >> np.uint32(4 * t + i)) & 1 == k1[:, :, 16 * t + 4 * gg + i]).all()
    assert (w[..., 3] == 0).all()
