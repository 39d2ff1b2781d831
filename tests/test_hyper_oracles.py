"""float64 oracle of the hypernetwork server update (``csrc/kernels/hyper.hip``, ``fl/hyper_server.py``), the edge
layouts at which the kernels are tested, and the error bounds.

``oracle_round`` is plain torch in float64 with no closed forms: per client the MLP forward, ``delta = W f + b - u``,
the whole gradient vector materialised (the ``P x H`` outer product included), its norm, the clip coefficient
``clip / (total + 1e-6)`` and Adam over the whole arena.  A CPU test ties it to the reference semantics (autograd on
``models.hyper.HyperNetwork``, ``clip_grad_norm_``, ``torch.optim.Adam``) to 1e-12, so it does not lean on the
formulas of ``hyper_server.py``.

``CASES`` holds the smallest layouts that reach each kernel path (docs/PARITY.md, "Hypernetwork server kernels:
which layout takes which path").  ``scenario`` builds a case's rounds (inputs and oracle results) once; this file's
CPU tests run the fp32 CPU composite through them, ``tests/test_gpu_hyper_edges.py`` (``import test_hyper_oracles as
R``) runs the HIP kernels through the same rounds.

Bounds: every constant of ``BOUND`` is 8x the worst error of the fp32 CPU composite against the oracle over all
native-eligible cases (the larger of a single-threaded and an 8-thread run, since the BLAS summation order depends on
the thread count; rounded up to one significant digit); the composite, pinned to one thread so that the figure is
reproducible, must stay within constant / 8 (asserted here), the device gets the whole constant.  The factor covers
the device's other fp32 summation order (up to 256 block partials, 16 waves and half-wave trees against one GEMV); an
indexing error moves ``m`` or ``v`` by the order of their maximum.  No constant comes from device output.  The
measured figures are in ``profiles/hyper_edges.md``."""
import contextlib
import functools
import math
from collections import OrderedDict
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn as nn

from attackfl_amd.fl.hyper_server import HyperServer
from attackfl_amd.models.hyper import HyperNetwork
from attackfl_amd.ops import composite as C

LR = 0.01
CLIPS = (0.05, 0.0)   # engaged / off
B1, B2, EPS = 0.9, 0.999, 1e-8

# name -> (P, clients, E, H, n_hidden), one-tensor target state dict of P values
CASES = OrderedDict()
for _p in (1, 3, 63, 64, 65, 131):
    CASES[f"tile{_p}"] = (_p, 4, 4, 8, 1)            # row tails, P below one sweep
CASES["tiny"] = (3, 4, 4, 4, 0)                      # L = 1, one active lane per half-wave
CASES["base"] = (131, 5, 8, 100, 2)                  # flat small-net Adam, production MLP
CASES["e6"] = (67, 6, 6, 100, 2)                     # non-flat: layer 0 scalar, layers 1-2 float4 (offW = 20936)
CASES["big-n"] = (131, 440, 8, 100, 2)               # non-flat by size (nsmall = 24620), client ids >= 256
CASES["cap"] = (131, 946, 8, 100, 2)                 # nsmall = 28668 <= 28672: the last native client count
CASES["over"] = (131, 947, 8, 100, 2)                # past the LDS capacity: composite loop on the device
CASES["hmax"] = (257, 6, 8, 124, 1)                  # the largest H the native path admits
CASES["deep"] = (131, 3, 8, 32, 7)                   # L = 8
CASES["stride"] = (32771, 4, 8, 4, 2)                # second iteration of every row loop
CASES["h102"] = (131, 5, 8, 102, 2)                  # H % 4 != 0: scalar k_hyper_rows / k_hyper_adam
NOT_NATIVE = ("over", "h102")
NATIVE_CASES = [c for c in CASES if c not in NOT_NATIVE]
SELECT = {"big-n": ([439, 256, 0], [256, 300])}
STRIDE_STEP = 7       # the teacher-forced round of ``stride`` starts here

# quantity -> bound for the device (8x the worst composite error, see the module docstring and
# profiles/hyper_edges.md).  gn / cs: relative; m_*, v_*: scaled by the oracle's max over the region; a_*, gen,
# feat: absolute.  rows_* / adam_*: the stand-alone rows and head-Adam kernels (delta, dfeat, m, v scaled by the
# oracle's max; W and b absolute).
BOUND = {
    "gn": 8 * 9e-7, "cs": 8 * 8e-7,
    "m_small": 8 * 5e-6, "m_head": 8 * 2e-6, "v_small": 8 * 4e-6, "v_head": 8 * 2e-6,
    "a_small": 8 * 4e-6, "a_head": 8 * 4e-7, "gen": 8 * 2e-6, "feat": 8 * 3e-6,
    "rows_delta": 8 * 6e-7, "rows_dfeat": 8 * 3e-6, "rows_gen": 8 * 5e-7,
    "adam_w": 8 * 3e-7, "adam_m": 8 * 2e-7, "adam_v": 8 * 3e-7,
}


# ------------------------------------------------------------------------------------------------ the oracle
def parse_layout(lay):
    """``HyperServer.layout_vec()`` -> named offsets."""
    lay = [int(x) for x in lay]
    L = lay[-7]
    assert len(lay) == 1 + 2 * L + 7
    return NS(emb=lay[0], w=[lay[1 + 2 * l] for l in range(L)], b=[lay[2 + 2 * l] for l in range(L)], L=L,
              E=lay[-6], H=lay[-5], n=lay[-4], offW=lay[-3], offB=lay[-2], P=lay[-1])


def _mlp(A, d, l):
    din = d.E if l == 0 else d.H
    return A[d.w[l]:d.w[l] + d.H * din].view(d.H, din), A[d.b[l]:d.b[l] + d.H]


def oracle_acts(A, d, c):
    """Inputs of every MLP layer and the features: acts[0] = embedding of client c, acts[L] = f."""
    acts = [A[d.emb + c * d.E:d.emb + (c + 1) * d.E]]
    for l in range(d.L):
        Wl, bl = _mlp(A, d, l)
        z = Wl @ acts[-1] + bl
        acts.append(torch.relu(z) if l < d.L - 1 else z)
    return acts


def oracle_heads(A, d):
    return A[d.offW:d.offW + d.P * d.H].view(d.P, d.H), A[d.offB:d.offB + d.P]


def oracle_features(A, d, clients):
    return torch.stack([oracle_acts(A, d, c)[-1] for c in clients])


def oracle_generate(A, d, clients):
    W, b = oracle_heads(A, d)
    return torch.stack([W @ oracle_acts(A, d, c)[-1] + b for c in clients])


def oracle_round(arena64, m64, v64, layout_vec, selected, U64, step0, lr, clip):
    """The sequential server update of one round in float64 -> ([(grad_norm, clip_scale)], arena, m, v).
    ``U64[k]`` is the update of ``selected[k]``.  The gradient is materialised in full and its norm taken from it."""
    d = parse_layout(layout_vec)
    A, m, v = arena64.clone(), m64.clone(), v64.clone()
    assert A.dtype == torch.float64 and A.numel() == d.offB + d.P
    info = []
    for k, c in enumerate(selected):
        acts = oracle_acts(A, d, c)
        f = acts[-1]
        W, b = oracle_heads(A, d)
        delta = W @ f + b - U64[k]
        g = torch.zeros_like(A)
        g[d.offW:d.offW + d.P * d.H] = torch.outer(delta, f).reshape(-1)
        g[d.offB:d.offB + d.P] = delta
        dz = W.t() @ delta
        for l in reversed(range(d.L)):
            Wl, _ = _mlp(A, d, l)
            g[d.w[l]:d.w[l] + Wl.numel()] = torch.outer(dz, acts[l]).reshape(-1)
            g[d.b[l]:d.b[l] + d.H] = dz
            da = Wl.t() @ dz
            if l > 0:
                dz = torch.where(acts[l] > 0, da, torch.zeros_like(da))
            else:
                g[d.emb + c * d.E:d.emb + (c + 1) * d.E] = da
        total = float(torch.sqrt((g * g).sum()))
        scale = 1.0
        if clip > 0:
            coef = clip / (total + 1e-6)
            if coef < 1.0:          # (false for a NaN norm: no scaling, as clip_grad_norm_'s clamp)
                scale = coef
        g = g * scale
        step = step0 + k + 1
        m = B1 * m + (1 - B1) * g
        v = B2 * v + (1 - B2) * g * g
        bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
        A = A - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + EPS)
        info.append((total, scale))
    return info, A, m, v


# ------------------------------------------------------------------------------------------------ scenarios
def make_server(case, clip, device):
    P, n, E, H, nh = CASES[case]
    sd = OrderedDict(w=torch.zeros(P))
    return HyperServer(sd, n, LR, clip, device, seed=3, embedding_dim=E, hidden_dim=H, n_hidden=nh)


def selections(case):
    n = CASES[case][1]
    return SELECT.get(case, ([n - 1, n // 2, 0], [1, n - 1]))


def probe_clients(case):
    """Clients whose generated models and features are compared after every round."""
    n = CASES[case][1]
    return [0, n - 1, 1]


def _updates(A64, d, sel, seed):
    """Generated models (fp32) minus 0.1 sign(r) (0.5 + |r|): |delta| >= 0.05 keeps the head gradients away from
    Adam's sign-like regime, where a rounding-sized delta would turn into an O(lr) parameter difference."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(len(sel), d.P, generator=g)
    return oracle_generate(A64, d, sel).float() - 0.1 * torch.sign(r) * (0.5 + r.abs())


@functools.lru_cache(maxsize=None)
def scenario(case, clip, nan=False):
    """The rounds of a case: inputs (fp32) and the oracle's results (fp64).  Chained cases run 3 clients, then 2
    (the second round starts at step 3).  ``stride`` does not chain (a multi-step comparison at large P is
    ill-conditioned): one client from the fresh state, then a teacher-forced round of two clients from the oracle's
    state rounded to fp32 at step ``STRIDE_STEP``.  Treat the result as read-only."""
    srv = make_server(case, clip, "cpu")
    lay = srv.layout_vec()
    d = parse_layout(lay)
    arena0 = srv.hnet.arena.detach().clone()
    A, m, v = arena0.double(), torch.zeros_like(arena0).double(), torch.zeros_like(arena0).double()
    s1, s2 = selections(case)
    plan = [(s1[:1], 0, False), (s2, STRIDE_STEP, True)] if case == "stride" else [(s1, 0, False), (s2, 3, False)]
    rounds = []
    for ri, (sel, step0, forced) in enumerate(plan):
        load = None
        if forced:
            load = (A.float(), m.float(), v.float())
            A, m, v = (t.double() for t in load)
        U = _updates(A, d, sel, 1000 * ri + 17)
        if nan and ri == 0:
            U[1, min(7, d.P - 1)] = float("nan")
        info, A, m, v = oracle_round(A, m, v, lay, sel, U.double(), step0, LR, clip)
        pc = probe_clients(case)
        rounds.append(NS(sel=sel, U=U, step0=step0, load=load, info=info, A=A, m=m, v=v,
                         gen=oracle_generate(A, d, pc), feat=oracle_features(A, d, pc)))
    return NS(case=case, clip=clip, lay=lay, d=d, arena0=arena0, rounds=rounds)


def begin_round(srv, rd):
    """Teacher forcing: load the round's start state into a server (no-op for chained rounds)."""
    if rd.load is not None:
        dev = srv.hnet.arena.device
        srv.load_arena(rd.load[0].to(dev))
        srv.m.copy_(rd.load[1].to(dev))
        srv.v.copy_(rd.load[2].to(dev))
        srv.step = rd.step0
    assert srv.step == rd.step0


def train_per_client(srv, rd):
    """``HyperServer.train`` one client at a time (the update is sequential, so this is the same round) ->
    every client's (grad_norm, clip_scale)."""
    dev = srv.hnet.arena.device
    U = rd.U.to(dev)
    info = []
    for k, c in enumerate(rd.sel):
        srv.train([c], {c: U[k]})
        li = srv.last_info
        info.append((li["grad_norm"], li["clip_scale"]))
    return info


def _rel(a, b):
    return abs(a - b) / abs(b)


def _scaled(x, ref):
    return float((x.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def _abs(x, ref):
    return float((x.detach().double().cpu() - ref).abs().max())


def state_errors(rd, d, info, arena, m, v, gen=None, feat=None):
    """{quantity: error} of a server's state after round ``rd`` against the oracle."""
    s, h = slice(0, d.offW), slice(d.offW, d.offB + d.P)
    e = {"gn": max(_rel(float(a[0]), o[0]) for a, o in zip(info, rd.info)),
         "cs": max(_rel(float(a[1]), o[1]) for a, o in zip(info, rd.info))}
    assert len(info) == len(rd.info)
    for q, x, ref in (("m", m, rd.m), ("v", v, rd.v)):
        e[f"{q}_small"], e[f"{q}_head"] = _scaled(x[s], ref[s]), _scaled(x[h], ref[h])
    e["a_small"], e["a_head"] = _abs(arena[s], rd.A[s]), _abs(arena[h], rd.A[h])
    if gen is not None:
        e["gen"] = _abs(gen, rd.gen)
    if feat is not None:
        e["feat"] = _abs(feat, rd.feat)
    return e


def merge(worst, e):
    for k, x in e.items():
        worst[k] = x if math.isnan(x) else max(worst.get(k, 0.0), x)
    return worst


def fmt(e):
    return " ".join(f"{k}={x:.2e}" for k, x in e.items())


def check(e, what, frac=1.0):
    """Every error within ``frac`` of its bound (NaN fails); prints the figures first."""
    print(f"{what}: {fmt(e)}")
    bad = {k: (x, BOUND[k] * frac) for k, x in e.items() if not x <= BOUND[k] * frac}
    assert not bad, f"{what}: error, bound {bad}"


@contextlib.contextmanager
def one_thread():
    """The composite's GEMV summation order, and with it its error, depends on the BLAS thread count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def composite_errors(case, clip):
    """The fp32 CPU composite run through a case's rounds -> worst {quantity: error} against the oracle."""
    with one_thread():
        return _composite_errors(case, clip)


def _composite_errors(case, clip):
    sc = scenario(case, clip)
    srv = make_server(case, clip, "cpu")
    assert torch.equal(srv.hnet.arena, sc.arena0)
    pc = probe_clients(case)
    worst = {}
    for rd in sc.rounds:
        begin_round(srv, rd)
        info = train_per_client(srv, rd)
        feat = torch.stack([srv.hnet.features(c)[1] for c in pc])
        merge(worst, state_errors(rd, sc.d, info, srv.hnet.arena, srv.m, srv.v, srv.hnet.generate_many(pc), feat))
    return worst


# ---------------------------------------------------------------- stand-alone rows / head-Adam kernel inputs
ROWS_H = (1, 7, 100, 102, 128)
ROWS_P = (1, 63, 64, 65, 16385)   # 16385: past the 256-block cap, k_hyper_rows visits a second tile
ADAM_SHAPES = ((65, 7), (131, 100), (16385, 128))  # the last: just past the 8192-block grid cap


@functools.lru_cache(maxsize=None)
def rows_inputs(P, H):
    g = torch.Generator().manual_seed(100003 * H + P)
    W = torch.randn(P, H, generator=g) * 0.1
    b, f, u = torch.randn(P, generator=g), torch.randn(H, generator=g), torch.randn(P, generator=g)
    delta = W.double() @ f.double() + b.double() - u.double()
    return NS(W=W, b=b, f=f, u=u, delta=delta, dfeat=W.double().t() @ delta,
              gen=W.double() @ f.double() + b.double())


def rows_errors(x, delta, dfeat, gen):
    return {"rows_delta": _scaled(delta, x.delta), "rows_dfeat": _scaled(dfeat, x.dfeat),
            "rows_gen": _scaled(gen, x.gen)}


@functools.lru_cache(maxsize=None)
def adam_inputs(P, H):
    """Three head-Adam steps with carried moments in float64 (torch.optim.Adam's arithmetic) on the gradient
    scale * delta_s (x) f_s; |delta| >= 0.05 as in ``_updates``."""
    g = torch.Generator().manual_seed(7919 * H + P)
    W, b = torch.randn(P, H, generator=g) * 0.1, torch.randn(P, generator=g)
    steps, scale, lr = [], 0.3, 1e-3
    p = torch.cat([W.reshape(-1), b]).double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in (1, 2, 3):
        r = torch.randn(P, generator=g)
        delta, f = 0.1 * torch.sign(r) * (0.5 + r.abs()), torch.randn(H, generator=g)
        gr = scale * torch.cat([torch.outer(delta.double(), f.double()).reshape(-1), delta.double()])
        m = B1 * m + (1 - B1) * gr
        v = B2 * v + (1 - B2) * gr * gr
        p = p - (lr / (1 - B1 ** step)) * m / (v.sqrt() / math.sqrt(1 - B2 ** step) + EPS)
        steps.append(NS(step=step, delta=delta, f=f, p=p, m=m, v=v))
    return NS(W=W, b=b, scale=scale, lr=lr, steps=steps)


def adam_errors(st, W, b, m, v):
    return {"adam_w": _abs(torch.cat([W.reshape(-1), b]), st.p), "adam_m": _scaled(m, st.m),
            "adam_v": _scaled(v, st.v)}


# ------------------------------------------------------------------------------------------------ CPU tests
class _Target(nn.Module):
    """A frozen one-tensor target: ``w`` is in the state dict and not a parameter."""

    def __init__(self, P):
        super().__init__()
        self.register_buffer("w", torch.zeros(P))


def _pack(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors])


@pytest.mark.parametrize("layout,clip", [((13, 3, 4, 8, 1), 0.05), ((7, 4, 6, 12, 2), 0.0), ((5, 3, 4, 4, 0), 0.05)])
def test_oracle_matches_autograd_clip_and_adam(layout, clip):
    """oracle_round == autograd on HyperNetwork + clip_grad_norm_ + torch.optim.Adam in float64, over two rounds
    (the dense embedding gradient moves rows whose gradient is zero once their moments are non-zero)."""
    P, n, E, H, nh = layout
    srv = HyperServer(OrderedDict(w=torch.zeros(P)), n, LR, clip, "cpu", seed=5, embedding_dim=E, hidden_dim=H,
                      n_hidden=nh)
    lay = srv.layout_vec()
    hnet = HyperNetwork(_Target(P), n, E, H, False, nh).double()
    hnet.load_state_dict({k: t.double() for k, t in srv.hnet.state_dict().items()})
    params = [hnet.embeddings.weight]
    for i in range(nh + 1):
        params += [hnet.mlp[2 * i].weight, hnet.mlp[2 * i].bias]
    params += [hnet.hyper_layers["w"].weight, hnet.hyper_layers["w"].bias]   # the arena's order
    assert len(params) == len(list(hnet.parameters()))
    opt = torch.optim.Adam(params, lr=LR, foreach=False)
    A = srv.hnet.arena.detach().double()
    assert torch.equal(_pack(params), A)
    m, v = torch.zeros_like(A), torch.zeros_like(A)
    g = torch.Generator().manual_seed(11)
    step0 = 0
    for sel in ([n - 1, 0, 1], [1, n - 1]):
        U = (torch.randn(len(sel), P, generator=g) * 0.3).double()
        ref_info = []
        for k, c in enumerate(sel):
            out, _ = hnet(torch.tensor(c))
            gen = out["w"].reshape(-1)
            grads = torch.autograd.grad(gen, params, grad_outputs=(gen - U[k]).detach())
            for p, gr in zip(params, grads):
                p.grad = gr
            if clip > 0:
                total = float(torch.nn.utils.clip_grad_norm_(params, clip))
                scale = min(1.0, clip / (total + 1e-6))
            else:
                total, scale = float(torch.linalg.vector_norm(_pack(grads))), 1.0
            opt.step()
            ref_info.append((total, scale))
        info, A, m, v = oracle_round(A, m, v, lay, sel, U, step0, LR, clip)
        step0 += len(sel)
        for (a, s), (ra, rs) in zip(info, ref_info):
            assert _rel(a, ra) <= 1e-12 and _rel(s, rs) <= 1e-12
        assert _scaled(_pack(params), A) <= 1e-12
        assert _scaled(_pack([opt.state[p]["exp_avg"] for p in params]), m) <= 1e-12
        assert _scaled(_pack([opt.state[p]["exp_avg_sq"] for p in params]), v) <= 1e-12
        if clip > 0:
            assert all(s < 1.0 for _, s in info)     # the clip is engaged


def test_case_table_reaches_the_paths_it_names():
    """The layouts' arithmetic: which small-net kernel, which side of the LDS capacity, how many row sweeps."""
    cap, flat_max = 28 * 1024, 4 * 6 * 1024          # HS_SMEM ; HS_PF * HS_NT float4 chunks
    for case, (P, n, E, H, nh) in CASES.items():
        d = scenario(case, CLIPS[0]).d
        nsmall = d.offW - d.emb
        native = H % 4 == 0 and d.offW % 4 == 0 and H <= 127 and nsmall <= cap
        assert native == (case not in NOT_NATIVE), case
        flat = E % 4 == 0 and nsmall % 4 == 0 and (n * E) % 4 == 0 and nsmall <= flat_max
        assert flat == (case not in ("e6", "big-n", "cap", "over", "h102")), case
    assert scenario("e6", CLIPS[0]).d.offW == 20936
    assert scenario("big-n", CLIPS[0]).d.offW == 24620 and scenario("cap", CLIPS[0]).d.offW == 28668
    assert scenario("over", CLIPS[0]).d.offW == 28676
    assert CASES["stride"][0] > 4 * 2 * 256 * 16       # HR4_U sweeps of the capped grid: a second iteration
    assert scenario("deep", CLIPS[0]).d.L == 8 and scenario("tiny", CLIPS[0]).d.L == 1
    for case in CASES:
        for clip in CLIPS:
            for rd in scenario(case, clip).rounds:
                assert all((s < 1.0) == (clip > 0) for _, s in rd.info), (case, clip)


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("case", NATIVE_CASES)
def test_composite_within_an_eighth_of_the_bounds(case, clip):
    check(composite_errors(case, clip), f"composite {case} clip={clip}", frac=1 / 8)


def test_rows_and_adam_composites_within_an_eighth_of_the_bounds():
    worst = {}
    with one_thread():
        _rows_and_adam_composites(worst)
    check(worst, "composite rows / head Adam", frac=1 / 8)


def _rows_and_adam_composites(worst):
    for H in ROWS_H:
        for P in ROWS_P:
            x = rows_inputs(P, H)
            delta, dfeat = C.hyper_delta_vjp(x.W, x.b, x.f, x.u)
            merge(worst, rows_errors(x, delta, dfeat, torch.addmv(x.b, x.W, x.f)))
    for P, H in ADAM_SHAPES:
        x = adam_inputs(P, H)
        W, b = x.W.clone(), x.b.clone()
        m, v = torch.zeros(P * H + P), torch.zeros(P * H + P)
        for st in x.steps:
            C.hyper_adam_outer(W, b, m, v, st.delta, st.f, st.step, x.lr, x.scale)
            merge(worst, adam_errors(st, W, b, m, v))


def test_a_wrong_index_is_far_outside_the_bounds():
    """What the margin of 8 is set against: the head gradient of one row taken from its neighbour moves m and v by
    the order of their maximum."""
    sc = scenario("base", CLIPS[0])
    rd, d = sc.rounds[0], sc.d
    m = rd.m.clone()
    W = m[d.offW:d.offW + d.P * d.H].view(d.P, d.H)
    W[5] = W[6]
    e = state_errors(rd, d, rd.info, rd.A, m, rd.v)
    assert e["m_head"] > 1000 * BOUND["m_head"]
