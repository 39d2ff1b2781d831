"""The hypernetwork server kernels (``csrc/kernels/hyper.hip``) at edge layouts against the float64 oracle of
``tests/test_hyper_oracles.py``: the non-flat small-net Adam, the LDS capacity boundary and the composite loop past
it, the scalar rows kernel, row tails and the second iteration of the row loops, L = 1 and L = 8, H = 4 and H = 124,
client ids >= 256, the generation / feature batching loops and NaN propagation.  Bounds: ``R.BOUND`` (8x the fp32
CPU composite's own error, never derived from device output); measured figures in ``profiles/hyper_edges.md``."""
from collections import OrderedDict
from types import SimpleNamespace as NS

import pytest
import torch

import test_hyper_oracles as R
from attackfl_amd import ops
from attackfl_amd.fl.hyper_server import HyperServer

pytestmark = pytest.mark.gpu

CLIP = R.CLIPS[0]


def _state(srv):
    return srv.hnet.arena, srv.m, srv.v


def _native_round(srv, rd, gen=(), enable=None, permute=False):
    """One ``ops.hyper_server_update`` over a round's clients -> (info [n, 2] on the host, generated [ngen, P]).
    permute: the updates are rows n, n-1, .., 1 of a gathered matrix whose row 0 is not an update."""
    dev = srv.hnet.arena.device
    n = len(rd.sel)
    if permute:
        G = torch.full((n + 1, rd.U.shape[1]), 7.0)
        urows = [n - k for k in range(n)]
        G[urows] = rd.U
        assert urows != list(range(n))
    else:
        G, urows = rd.U, list(range(n))
    info, out = ops.hyper_server_update(srv.hnet.arena, srv.m, srv.v, G.to(dev), urows, rd.sel, srv.layout_vec(),
                                        srv.step, srv.lr, srv.clip, enable=enable, gen=gen)
    srv.step += n
    srv._gen_cache = None
    return info.double().cpu().tolist(), out


@pytest.mark.parametrize("clip", R.CLIPS)
@pytest.mark.parametrize("case", list(R.CASES))
def test_server_update_matches_fp64_oracle(gpu, case, clip):
    """Two rounds (3 clients, then 2; ``stride``: 1 from the fresh state, then 2 teacher-forced at step 7): every
    client's grad norm and clip scale, and after each round the arena, m and v by region, the generated models and
    the features, against the oracle."""
    sc = R.scenario(case, clip)
    srv = R.make_server(case, clip, gpu)
    native = case not in R.NOT_NATIVE
    assert srv._native_ok() == native
    assert torch.equal(srv.hnet.arena.cpu(), sc.arena0)
    pc = R.probe_clients(case)
    worst = {}
    for rd in sc.rounds:
        R.begin_round(srv, rd)
        if native:
            info, _ = _native_round(srv, rd, permute=case == "base")
            gen = ops.hyper_generate_many(srv.hnet.arena, pc, srv.layout_vec())
            feat = ops.hyper_features(srv.hnet.arena, pc, srv.layout_vec())
        else:  # the composite loop on the device: k_hyper_rows(4), k_hyper_reduce, adam_flat, k_hyper_adam
            info = R.train_per_client(srv, rd)
            gen, feat = srv.generate_many(pc), None
        assert srv.step == rd.step0 + len(rd.sel)
        R.merge(worst, R.state_errors(rd, sc.d, info, *_state(srv), gen, feat))
    R.check(worst, f"device {case} clip={clip}")


@pytest.mark.parametrize("case", ["e6", "big-n", "stride"])
def test_update_is_bit_reproducible_and_disable_keeps_bits(gpu, case):
    sc = R.scenario(case, CLIP)
    srv = [R.make_server(case, CLIP, gpu) for _ in range(2)]
    for s in srv:
        for rd in sc.rounds:
            R.begin_round(s, rd)
            U = rd.U.to(gpu)
            s.train(rd.sel, {c: U[k] for k, c in enumerate(rd.sel)})
    for a, b in zip(_state(srv[0]), _state(srv[1])):
        assert torch.equal(a, b)
    assert not torch.equal(srv[0].hnet.arena.cpu(), sc.arena0)
    before = [t.clone() for t in _state(srv[0])]
    rd = sc.rounds[-1]
    U = rd.U.to(gpu)
    srv[0].train(rd.sel, {c: U[k] for k, c in enumerate(rd.sel)}, enable=torch.zeros(1, dtype=torch.int32, device=gpu))
    for a, b in zip(_state(srv[0]), before):
        assert torch.equal(a, b)


@pytest.mark.parametrize("ngen", [1, 8, 9, 32])
@pytest.mark.parametrize("case", ["tile65", "e6", "cap", "stride"])
def test_fused_generation_equals_plain(gpu, case, ngen):
    """The START generated inside the update (features in the last small-net launch, the heads sweep fused with the
    last head Adam) equals ``hyper_generate_many`` from the updated arena bitwise, leaves the update's own bits alone
    and is within the bound of the oracle's ``W f + b``."""
    sc = R.scenario(case, CLIP)
    rd = sc.rounds[-1] if case == "stride" else sc.rounds[0]
    n = R.CASES[case][1]
    gen = [(5 * k + 1) % n for k in range(ngen)]
    a, b = (R.make_server(case, CLIP, gpu) for _ in range(2))
    for s in (a, b):
        R.begin_round(s, rd)
    _, fused = _native_round(a, rd, gen=gen, enable=torch.ones(1, dtype=torch.int32, device=gpu))
    _native_round(b, rd)
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    plain = ops.hyper_generate_many(b.hnet.arena, gen, b.layout_vec())
    assert fused.shape == (ngen, sc.d.P) and torch.equal(fused, plain)
    R.check({"gen": R._abs(fused, R.oracle_generate(rd.A, sc.d, gen))}, f"fused generation {case} ngen={ngen}")


def test_generate_many_batches_and_position(gpu):
    """40 clients: two k_hyper_gen4 launches, the last group of 8; 70 clients: two k_hyper_feat_many launches.  A
    client's row does not depend on its slot (bitwise equal to the single-client call)."""
    srv = HyperServer(OrderedDict(w=torch.zeros(131)), 80, R.LR, CLIP, gpu, seed=3)
    assert srv._native_ok()
    lay, d = srv.layout_vec(), R.parse_layout(srv.layout_vec())
    A64 = srv.hnet.arena.double().cpu()
    c40 = [(7 * k + 3) % 80 for k in range(40)]
    c40[5], c40[39] = c40[0], c40[33]          # repeats, one of them across the two launches
    many = ops.hyper_generate_many(srv.hnet.arena, c40, lay)
    single = {c: ops.hyper_generate_many(srv.hnet.arena, [c], lay)[0] for c in set(c40)}
    for k, c in enumerate(c40):
        assert torch.equal(many[k], single[c]), (k, c)
    c70 = [(11 * k + 5) % 80 for k in range(70)]
    c70[69] = c70[2]
    feats = ops.hyper_features(srv.hnet.arena, c70, lay)
    fsingle = {c: ops.hyper_features(srv.hnet.arena, [c], lay)[0] for c in set(c70)}
    for k, c in enumerate(c70):
        assert torch.equal(feats[k], fsingle[c]), (k, c)
    R.check({"gen": R._abs(many, R.oracle_generate(A64, d, c40)), "feat": R._abs(feats, R.oracle_features(A64, d, c70))},
            "generate_many 40 / features 70")


@pytest.mark.parametrize("clip", R.CLIPS)
def test_single_client_round(gpu, clip):
    """n = 1: only the k == 0 rows launch, then k_hyper_adam_v (no generation) or k_hyper_gen4<true>."""
    sc = R.scenario("base", clip)
    r0 = sc.rounds[0]
    z = torch.zeros_like(sc.arena0).double()
    info, A, m, v = R.oracle_round(sc.arena0.double(), z, z, sc.lay, r0.sel[:1], r0.U[:1].double(), 0, R.LR, clip)
    pc = [2, 0, 4]
    rd = NS(sel=r0.sel[:1], U=r0.U[:1], step0=0, load=None, info=info, A=A, m=m, v=v,
            gen=R.oracle_generate(A, sc.d, pc), feat=None)
    a, b = (R.make_server("base", clip, gpu) for _ in range(2))
    ia, _ = _native_round(a, rd)
    ib, fused = _native_round(b, rd, gen=pc)
    assert ia == ib
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    assert torch.equal(fused, ops.hyper_generate_many(a.hnet.arena, pc, a.layout_vec()))
    R.check(R.state_errors(rd, sc.d, ia, *_state(a), fused), f"device single client clip={clip}")


def _rows_check(gpu, H, unaligned=False):
    worst = {}
    for P in R.ROWS_P:
        x = R.rows_inputs(P, H)
        if unaligned:  # W one float into a larger buffer: not 16-byte aligned, so the scalar kernel
            buf = torch.full((P * H + 5,), 7.0, device=gpu)
            W = buf[1:1 + P * H].view(P, H)
            W.copy_(x.W)
            assert W.data_ptr() % 16 == 4
        else:
            W = x.W.to(gpu)
        b, f, u = x.b.to(gpu), x.f.to(gpu), x.u.to(gpu)
        delta, dfeat = ops.hyper_delta_vjp(W, b, f, u)
        e = R.rows_errors(x, delta, dfeat, ops.hyper_generate(W, b, f))
        print(f"rows P={P} H={H} unaligned={unaligned}: {R.fmt(e)}")
        R.merge(worst, e)
    R.check(worst, f"device rows H={H} unaligned={unaligned}")


@pytest.mark.parametrize("H", R.ROWS_H)
def test_rows_kernels_vs_fp64(gpu, H):
    """k_hyper_rows4 (H % 4 == 0) and the scalar k_hyper_rows with its reduction, P in {1, 63, 64, 65, 16385}."""
    _rows_check(gpu, H)


def test_rows_kernels_vs_fp64_unaligned(gpu):
    _rows_check(gpu, 100, unaligned=True)


@pytest.mark.parametrize("P,H", R.ADAM_SHAPES)
def test_hyper_adam_outer_steps(gpu, P, H):
    """The scalar head Adam (k_hyper_adam) over steps 1 to 3 with carried moments."""
    x = R.adam_inputs(P, H)
    W, b = x.W.to(gpu), x.b.to(gpu)
    m, v = torch.zeros(P * H + P, device=gpu), torch.zeros(P * H + P, device=gpu)
    worst = {}
    for st in x.steps:
        ops.hyper_adam_outer(W, b, m, v, st.delta.to(gpu), st.f.to(gpu), st.step, x.lr, x.scale)
        e = R.adam_errors(st, W, b, m, v)
        print(f"adam P={P} H={H} step={st.step}: {R.fmt(e)}")
        R.merge(worst, e)
    R.check(worst, f"device head Adam P={P} H={H}")


def test_nan_update_follows_oracle(gpu):
    """One NaN in the second client's update: its grad norm is NaN and its clip scale 1 (``coef < 1`` is false), as in
    the oracle; the NaNs land where the oracle's do; the same call disabled on the device leaves every bit alone."""
    sc = R.scenario("base", CLIP, nan=True)
    rd = sc.rounds[0]
    assert torch.isnan(rd.U).sum() == 1 and rd.info[1][0] != rd.info[1][0] and rd.info[1][1] == 1.0
    srv = R.make_server("base", CLIP, gpu)
    before = [t.clone() for t in _state(srv)]
    _native_round(srv, rd, enable=torch.zeros(1, dtype=torch.int32, device=gpu))
    for a, b in zip(_state(srv), before):
        assert torch.equal(a, b)
    srv.step = 0
    info, _ = _native_round(srv, rd)
    assert R._rel(info[0][0], rd.info[0][0]) <= R.BOUND["gn"] and R._rel(info[0][1], rd.info[0][1]) <= R.BOUND["cs"]
    for k in (1, 2):
        assert info[k][0] != info[k][0] and info[k][1] == 1.0, info
    for x, ref in zip(_state(srv), (rd.A, rd.m, rd.v)):
        assert torch.equal(torch.isnan(x.cpu()), torch.isnan(ref))
    assert torch.isnan(rd.A).any() and not torch.isnan(rd.A).all()
