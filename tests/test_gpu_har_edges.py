"""The ten bf16 HAR encoder kernels (``csrc/kernels/har.hip``), one by one, against the fp64 references and bounds of
``tests/test_har_oracles.py`` at edge shapes.  For every case: every element within ``tol`` (NaN / inf in the same
places), a second run gives the same bits, and memory the kernel must not touch keeps its prefill (padding rows
``[L, Lp)`` of the head-major buffers, rows beyond R, partials beyond ``G * NG``).  Each test prints its worst
err / bound ratio.  Derivations, measured budgets and the worst ratios: docs/HAR_TEST_BOUNDS.md."""
import numpy as np
import pytest
import torch

import test_har_oracles as R
from attackfl_amd.ops import native

pytestmark = pytest.mark.gpu

GARBAGE = 0x5A5A5A5A5A5A5A5A  # prefill of the attention keep words in the second run


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b, what, clients=None):
    for k in a:
        x, y = (a[k], b[k]) if clients is None else (a[k][clients], b[k][clients])
        assert torch.equal(_bits(x), _bits(y)), f"{what}: {k} differs in {int((_bits(x) != _bits(y)).sum())} elements"


def _untouched(extra, what):
    for k, v in extra.items():
        if not isinstance(v, tuple):
            continue
        got, want = v
        if isinstance(want, torch.Tensor):
            assert torch.equal(got.float(), want.float()), f"{what}: {k} was modified"
        else:
            assert bool((got.float() == want).all()), f"{what}: {k} lost its prefill in {int((got.float() != want).sum())} elements"


def _edge(kernels, c, dev, replicate=True, **second):
    """Run case ``c`` twice through ``run`` of ``kernels[0]`` and hold the outputs to the references of ``kernels``."""
    run = R.KERNELS[kernels[0]].run
    cc = R.replicate(c, c.rep) if (replicate and c.rep > 1) else c
    n = cc.C // c.C
    out, extra = run(cc, dev)
    out2, _ = run(cc, dev, **second)
    ref = {}
    for k in kernels:
        ref.update(R.ref_of(k, c))
    top = max(R.check({k: v[i * c.C:(i + 1) * c.C] for k, v in out.items()}, ref, f"{c.name} [{i}]") for i in range(n))
    _same_bits(out, out2, c.name + " second run")
    _untouched(extra, c.name)
    print(f"{c.name}: worst err/bound {top:.3g}")
    return out, extra


def _ids(cases):
    return [c.name.replace(" ", "_") for c in cases]


STEM, POOL, REDUCE, QKV = R.cases_stem(), R.cases_pool(), R.cases_reduce(), R.cases_qkv()
ATTN, POST, QKVB = R.cases_attn(), R.cases_post(), R.cases_qkv_bwd()


@pytest.mark.parametrize("c", STEM, ids=_ids(STEM))
def test_stem(gpu, c):
    _edge(["stem"], c, gpu)


@pytest.mark.parametrize("c", POOL, ids=_ids(POOL))
def test_pool(gpu, c):
    _edge(["pool"], c, gpu)


@pytest.mark.parametrize("c", REDUCE, ids=_ids(REDUCE))
def test_reduce(gpu, c):
    _edge(["reduce"], c, gpu)


@pytest.mark.parametrize("c", QKV, ids=_ids(QKV))
def test_qkv(gpu, c):
    _edge(["qkv"], c, gpu)


@pytest.mark.parametrize("c", QKVB, ids=_ids(QKVB))
def test_qkv_bwd(gpu, c):
    _edge(["qkv_bwd"], c, gpu)


def _check_keep_words(c, mask):
    """The forward's stored flags of every (client, sample, head) are exactly masks.keep_rc."""
    ref = R.keep_rc_grid(c).numpy()
    for ci in range(c.C):
        for b in range(c.B):
            for h in range(4):
                got = R.decode_keep_words(mask[ci, b, h], c.L, c.Lp)
                assert (got == ref[ci, b, h]).all(), (c.name, ci, b, h, int((got != ref[ci, b, h]).sum()))


@pytest.mark.parametrize("c", ATTN, ids=_ids(ATTN))
def test_attention(gpu, c):
    """Forward, dK / dV and dQ.  The second run starts from keep words prefilled with garbage instead of zeros: the words
    the forward never writes (key chunks at or beyond ceil64(L) when Lp is larger) must not reach any output."""
    _, extra = _edge(["attn_fwd", "attn_bwd"], c, gpu, mask_fill=GARBAGE)
    if c.p > 0.0:
        _check_keep_words(c, extra["mask"])


@pytest.mark.parametrize("L", [c.L for c in ATTN[:len(R.ATTN_L)] if c.p == 0.0])
def test_attention_keep_words_at_remaining_lengths(gpu, L):
    """keep words against masks.keep_rc at the lengths whose edge case above runs without dropout."""
    c = R.attn_case(L, 0.5)
    _, extra = R.run_attn(c, gpu)
    _check_keep_words(c, extra["mask"])


@pytest.mark.parametrize("c", POST, ids=_ids(POST))
def test_post(gpu, c):
    _, extra = _edge(["post"], c, gpu)
    if c.p > 0.0:  # the stored keep bits are the three sites' afl_keep draws
        want = R.encode_kbits(c)
        for i in range(c.rep):
            assert torch.equal(extra["kbits"][i * c.C:(i + 1) * c.C], want), c.name


@pytest.mark.parametrize("c", POST, ids=_ids(POST))
def test_post_bwd(gpu, c):
    _edge(["post_bwd"], c, gpu, replicate=False)


def test_post_bwd_two_layers_through_one_ws(gpu):
    """``ws_post`` is one buffer for both layers: after a layer with many row blocks, a layer with fewer blocks than
    workgroups must leave zeros (not the previous layer's partials) in its idle workgroups' slots."""
    a = next(c for c in POST if c.R == 561)
    b = next(c for c in POST if c.R == 16 and c.G == a.G and c.C == a.C)
    ws = torch.full((a.C * a.G * R.POST_NG + 64,), R.WS_PRE, device=gpu)
    R.run_post_bwd(a, gpu, ws=ws)
    out, extra = R.run_post_bwd(b, gpu, ws=ws)
    top = R.check(out, R.ref_of("post_bwd", b), "second layer through the same ws")
    _untouched(extra, "second layer")
    print(f"two layers, one ws: worst err/bound {top:.3g}")


# ------------------------------------------------------------------------------------------------ packing
PACK = R.packing_cases()


@pytest.mark.parametrize("kernel", list(PACK))
def test_client_zero_alone_has_the_same_bits(gpu, kernel):
    """Client 0 launched alone (C = 1) gets the bits it gets in a launch with C = 5: the forward grids depend on C and
    the backward's fixed G promises this independence."""
    c = PACK[kernel]
    run = R.KERNELS[kernel].run
    out5, _ = run(c, gpu)
    out1, _ = run(R.sub(c, [0]), gpu)
    R.check(out5, {k: v for k, v in {**R.ref_of(kernel, c)}.items() if k in out5}, f"packing {kernel}")
    _same_bits({k: v[:1] for k, v in out5.items()}, out1, f"{kernel} C=1 vs C=5")


@pytest.mark.parametrize("kernel", list(PACK))
def test_nan_client_does_not_leak(gpu, kernel):
    """With every input and parameter of client 1 NaN, the other clients' outputs keep their bits."""
    c = PACK[kernel]
    run = R.KERNELS[kernel].run
    clean, _ = run(c, gpu)
    dirty, _ = run(R.poison_client(c, 1), gpu)
    _same_bits(clean, dirty, f"{kernel} with a NaN client", clients=[0, 2, 3, 4])


# ------------------------------------------------------------------------------------------------ host checks
def _raises(fn, *outputs):
    """``fn`` must raise before any launch: the outputs keep their prefill."""
    with pytest.raises(RuntimeError):
        fn()
    torch.cuda.synchronize()
    for t in outputs:
        assert bool((t.float() == R.PRE).all()), "a rejected call wrote to its output"


def test_host_checks_reject_before_launch(gpu):
    nat = native()
    bf, dev = torch.bfloat16, gpu
    full = lambda *s, dtype=torch.float32: torch.full(s, R.PRE, dtype=dtype, device=dev)
    C, B, L, Lp = 2, 2, 20, 64
    Rr = B * L
    params, w = R.layer_params(C, R.gen(99))
    params = torch.nan_to_num(params).to(dev)
    P = params.shape[1]
    ctl = R.make_ctl(C, dev)
    x, qkv, o = full(C, Rr, 64, dtype=bf), full(C * B * 4, 3, Lp, 16, dtype=bf), full(C, Rr, 64, dtype=bf)
    lse2, delta, dqkv = full(C * B * 4, Lp), full(C * B * 4, Lp), full(C * B * 4, 3, Lp, 16, dtype=bf)
    mask = torch.zeros(C * B * 4, int(nat.har_mask_words(Lp)), dtype=torch.int64, device=dev)
    qs = 0.25 * 1.4426950408889634
    # ---- Lp
    for bad_lp, LL in ((96, 20), (64, 70), (0, 20)):
        q2, l2, d2 = full(C * B * 4, 3, bad_lp, 16, dtype=bf), full(C * B * 4, max(bad_lp, 1)), full(C * B * 4, 3, bad_lp, 16, dtype=bf)
        x2 = full(C, B * LL, 64, dtype=bf)
        _raises(lambda: nat.har_qkv(x2, params, w[0], w[1], q2, B, LL, qs), q2)
        _raises(lambda: nat.har_attn_fwd(q2, x2, l2, B, LL, None, None, 0, 0.0, None), x2)
        _raises(lambda: nat.har_attn_bwd(q2, l2, x2, l2, d2, B, LL, None, None, 0, 0.0, None), d2)
        _raises(lambda: nat.har_qkv_bwd(d2, full(C, B * LL, 64), x2, full(C, B * LL, 64), full(C * 2 * R.QKV_NG), params,
                                        w[0], B, LL, 2))
    # above the cap (nothing of this size is ever launched)
    cap = int(nat.har_attn_max_lp)
    assert cap == 896
    big = cap + 64
    qb, lb = full(4, 3, big, 16, dtype=bf), full(4, big)
    ob = full(1, big, 64, dtype=bf)
    _raises(lambda: nat.har_attn_fwd(qb, ob, lb, 1, big, None, None, 0, 0.0, None), ob)
    _raises(lambda: nat.har_attn_bwd(qb, lb, ob, lb, full(4, 3, big, 16, dtype=bf), 1, big, None, None, 0, 0.0, None))
    # ---- dropout without its buffers
    _raises(lambda: nat.har_attn_fwd(qkv, o, lse2, B, L, ctl.seeds, ctl.stepctl, 0, 0.1, None), o)
    _raises(lambda: nat.har_attn_bwd(qkv, lse2, o, delta, dqkv, B, L, ctl.seeds, ctl.stepctl, 0, 0.1, None), dqkv)
    _raises(lambda: nat.har_attn_fwd(qkv, o, lse2, B, L, None, None, 0, 0.1, mask), o)  # no seeds
    xh1, xh2, y, rs = full(C, Rr, 64, dtype=bf), full(C, Rr, 64, dtype=bf), full(C, Rr, 64, dtype=bf), full(C, Rr, 2)
    _raises(lambda: nat.har_post(o, x, xh1, xh2, rs, y, params, w, ctl.seeds, ctl.stepctl, 0, 0.1, None), xh1, xh2, y, rs)
    dres, dout, dy = full(C, Rr, 64), full(C, Rr, 64, dtype=bf), full(C, Rr, 64)
    wsp = full(C * 2 * R.POST_NG)

    def post_bwd(G=2, ww=w, kb=None, p=0.0, dl=delta, prm=params):
        s, sc = (ctl.seeds, ctl.stepctl) if p else (None, None)
        return lambda: nat.har_post_bwd(dy, None, B, L, o, xh1, xh2, rs, dres, dout, dl, wsp, prm, ww, s, sc, 0, p, G, kb)

    _raises(post_bwd(p=0.1), dres, dout, wsp)
    # ---- G < 1
    _raises(post_bwd(G=0), dres, dout, wsp)
    _raises(post_bwd(G=-1), dres, dout, wsp)
    _raises(lambda: nat.har_qkv_bwd(dqkv, dres, x, full(C, Rr, 64), full(C * 2 * R.QKV_NG), params, w[0], B, L, 0))
    _raises(lambda: nat.har_reduce(wsp, 0, 10, torch.tensor([[0, 0, 10]], dtype=torch.int32, device=dev), full(C, P)))
    # ---- delta's Lp
    _raises(post_bwd(dl=full(C * B * 4, 96)), dres, dout, wsp)
    # ---- offsets outside a client's row
    for i in range(2, 12):
        for off in (P - R.LAYER_SIZES[i] + 1, -1):
            ww = list(w)
            ww[i] = off
            _raises(lambda: nat.har_post(o, x, xh1, xh2, rs, y, params, ww, None, None, 0, 0.0, None), xh1, xh2, y, rs)
            _raises(post_bwd(ww=ww), dres, dout, wsp)
    for woff, boff in ((P - 192 * 64 + 1, w[1]), (w[0], P - 191), (-1, w[1]), (w[0], -1)):
        _raises(lambda: nat.har_qkv(x, params, woff, boff, qkv, B, L, qs), qkv)
    _raises(lambda: nat.har_qkv_bwd(dqkv, dres, x, full(C, Rr, 64), full(C * 2 * R.QKV_NG), params, P - 192 * 64 + 1, B, L, 2))
    # the stem: 64 L floats of positional encoding must fit (L = 601 against a 600-row table)
    Ls = 601
    sp = torch.zeros(C, 256 + 64 * 600, device=dev)
    h = full(C, Ls, 64, dtype=bf)
    xs = torch.zeros(C, 1, Ls, device=dev)
    _raises(lambda: nat.har_stem(xs, sp, 0, 192, 256, h), h)
    _raises(lambda: nat.har_stem(xs, sp, sp.shape[1] - 191, 192, 256, h), h)
    _raises(lambda: nat.har_stem(xs, sp, 0, sp.shape[1] - 63, 256, h), h)
    nat.har_stem(xs[:, :, :600].contiguous(), sp, 0, 192, 256, h[:, :600].contiguous())  # the accepted side
    # params with the wrong client count
    _raises(lambda: nat.har_qkv(x, params[:1].contiguous(), w[0], w[1], qkv, B, L, qs), qkv)
    torch.cuda.synchronize()
