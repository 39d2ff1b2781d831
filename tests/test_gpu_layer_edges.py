"""The layer kernels of ``csrc/kernels/layers.hip`` at the shapes, strides and values where kernels go wrong — sizes
around every tile and block boundary, one row, unaligned and transposed views, saturated and non-finite values —
against the fp64 references of ``tests/test_layer_oracles.py`` (plain torch, checked there against the composites on
the CPU).  For every case: the device result is within the reference's bound at EVERY element (bounds come from the
number formats and the count of roundings, never from the kernels' output), a second run has the same bits, and where
a kernel reduces over rows client 0 launched alone has the same bits as in the packed launch.  Each test prints its
worst err/bound ratio (``pytest -s``); ``docs/LAYER_TEST_BOUNDS.md`` records them."""
import pytest
import torch

import test_layer_oracles as R
from attackfl_amd.ops import layers as Lx

pytestmark = pytest.mark.gpu


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in a) and a.keys() == b.keys()


def sweep(cases, run, ref, dev, name, pack=False):
    """Bound, run-to-run bits and (``pack``) client 0 alone vs packed, over every case; prints the worst ratio."""
    w, n = 0.0, 0
    for c in cases:
        out = run(c, dev)
        w = max(w, R.check(out, ref(c), f"{name} [{c.id}]"))
        assert same_bits(out, run(c, dev)), f"{name} [{c.id}]: second run differs"
        if pack:
            assert c.C == 5, c.id
            solo = run(c, dev, one=True)
            for k in solo:
                assert torch.equal(bits(solo[k]), bits(out[k][:1])), f"{name} [{c.id}]: {k} depends on the packing"
        n += 1
    assert n > 0
    print(f"{name}: {n} cases, worst err/bound {w:.3g}")
    return w


# ================================================================================================== k_bgemm
@pytest.mark.parametrize("K", R.GEMM_K)
def test_bgemm_tile_edge_shapes(gpu, K):
    """M x N x K around the 64 x 64 x 32 tile; layouts, alignment, output stride and epilogues cycle over the shapes."""
    sweep((c for c in R.cases_bgemm_shapes() if c.K == K), R.run_gemm, R.ref_gemm, gpu, f"bgemm K={K}")


@pytest.mark.parametrize("lay", range(len(R.LAYOUTS)))
def test_bgemm_layouts_and_epilogues(gpu, lay):
    """All four operand-layout instantiations, the vector and the scalar load path, every epilogue, strided output
    (whose in-between entries must keep their prefill)."""
    cases = [c for i, c in enumerate(R.cases_bgemm_layouts()) if i // len(R.EPILOGUES) == lay]
    sweep(cases, R.run_gemm, R.ref_gemm, gpu, f"bgemm layout {R.LAYOUTS[lay]}")


def test_bgemm_splitk_short_and_empty_splits(gpu):
    sweep(R.cases_bgemm_splitk(), R.run_gemm, R.ref_gemm, gpu, "bgemm split-K")


def test_bgemm_nan_row_stays_in_its_row(gpu):
    """One NaN row of A: that output row is NaN, every other element still within its bound."""
    sweep(R.cases_bgemm_nan(), R.run_gemm, R.ref_gemm, gpu, "bgemm NaN row")


# ================================================================================================== k_tsgemm
@pytest.mark.parametrize("N,K", R.TS_SHAPES)
def test_tsgemm_instantiations(gpu, N, K):
    """Every (N, K) instantiation, B row-major and transposed, M around the 16-row tile, every epilogue on."""
    sweep((c for c in R.cases_tsgemm() if (c.N, c.K) == (N, K)), R.run_gemm, R.ref_gemm, gpu, f"tsgemm {N}x{K}")


@pytest.mark.parametrize("i", [0, 1])
def test_tsgemm_strided_tile_loop(gpu, i):
    """C = 64, M = 2071: 16 blocks per client, 2-3 row tiles per wave (the loop-carried prefetch for K = 64), the last
    tile partial."""
    sweep([list(R.cases_tsgemm_tiles())[i]], R.run_gemm, R.ref_gemm, gpu, "tsgemm tile loop")


def test_tsgemm_fused_column_sums(gpu):
    """Ordered column-sum partials over several tiles per wave, and N = 256 (the separate column-sum pass)."""
    sweep(R.cases_tsgemm_colsums(), R.run_gemm, R.ref_gemm, gpu, "tsgemm column sums")


def test_tsgemm_column_sums_do_not_depend_on_packing(gpu):
    cases = [R.gemm_case(5, 24581, 64, 64, asum=True, seed=90, bias=True, Z=False, act=1, generic=False),
             R.gemm_case(5, 1007, 64, 256, asum=True, seed=91, **R.TS_EPI),
             R.gemm_case(5, 1007, 256, 64, asum=True, seed=92, **R.TS_EPI)]
    sweep(cases, R.run_gemm, R.ref_gemm, gpu, "tsgemm packing", pack=True)


def test_tsgemm_preconditions_fall_back(gpu):
    sweep(R.cases_tsgemm_fallback(), R.run_gemm, R.ref_gemm, gpu, "tsgemm fallback")


# ================================================================================================== the other layers
def test_colsum_edges(gpu):
    sweep(R.cases_colsum(), R.run_colsum, R.ref_colsum, gpu, "colsum", pack=True)


def test_gathers_exact(gpu):
    for c in R.cases_gather():
        out = R.run_gather(c, gpu)
        assert R.check(out, R.ref_gather(c), "gather " + c.id) == 0.0
        assert same_bits(out, R.run_gather(c, gpu))


def test_conv_patches_and_pool_edges(gpu):
    sweep(R.cases_conv(), R.run_conv, R.ref_conv, gpu, "im2col/col2im/pool4")


def test_layernorm_forward_edges(gpu):
    sweep(R.cases_ln(), R.run_ln_fwd, R.ref_ln_fwd, gpu, "ln_fwd", pack=True)


def test_layernorm_backward_edges(gpu):
    sweep(R.cases_ln(), R.run_ln_bwd, R.ref_ln_bwd, gpu, "ln_bwd", pack=True)


def test_gru_cell_edges(gpu):
    sweep(R.cases_gru(), R.run_gru, R.ref_gru, gpu, "gru", pack=True)


@pytest.mark.parametrize("kind", ["bce", "ce"])
def test_loss_edges(gpu, kind):
    """Losses, gradients and the failed flag over batch sizes around the 256-thread block, bs < B, bs < min_bs,
    step >= S, an already failed client, saturated logits and NaN with nan_abort on and off."""
    w = 0.0
    for c in R.cases_loss(kind):
        out = R.run_loss(c, gpu)
        w = max(w, R.check(out, R.ref_loss(c), f"{kind} [{c.id}]"))
        assert same_bits(out, R.run_loss(c, gpu))
        solo = R.run_loss(c, gpu, one=True)
        for k in solo:
            assert torch.equal(bits(solo[k]), bits(out[k][:1])), (c.id, k)
    print(f"{kind}: worst err/bound {w:.3g}")


def test_adam_edges(gpu):
    """Unaligned rows (C = 3, odd P), skip ranges in the head and the tail, step counts 0 and 5000, zero gradients, SGD;
    consumed gradients are zeroed, skipped entries and the inactive client keep their bits."""
    w = 0.0
    for c in R.cases_adam():
        out = R.run_adam(c, gpu)
        w = max(w, R.check(out, R.ref_adam(c), "adam " + c.id))
        assert same_bits(out, R.run_adam(c, gpu))
    print(f"adam: worst err/bound {w:.3g}")


def test_har_stem_edges(gpu):
    sweep(R.cases_conv_pe(), R.run_conv_pe, R.ref_conv_pe, gpu, "conv_pe", pack=True)


def test_mean_rows_edges(gpu):
    sweep(R.cases_mean_rows(), R.run_mean_rows, R.ref_mean_rows, gpu, "mean_rows", pack=True)


def test_step_end_edges(gpu):
    for c in R.cases_step_end():
        tcount, steps, ctl = R.run_step_end(c, gpu)
        want, wsteps = R.ref_step_end(c)
        assert torch.equal(tcount, want) and steps == wsteps and ctl.tolist()[1:] == [c.min_bs, 1], c.id


# ================================================================================================== bindings refuse
def _t(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


def _refused(fn, *a, **k):
    with pytest.raises(RuntimeError):
        fn(*a, **k)
    torch.cuda.synchronize()


def test_bindings_refuse_splitk_with_a_nonlinear_epilogue(gpu):
    """Every split runs the epilogue on its partial sum: a bias would be added once per split."""
    A, B, Cm = _t(2, 65, 40), _t(2, 33, 40), _t(2, 65, 33)
    Lx.bgemm(A, B, Cm, accum=2, splitk=2)
    _refused(Lx.bgemm, A, B, Cm, bias=_t(2, 33), accum=2, splitk=2)
    _refused(Lx.bgemm, A, B, Cm, Z=_t(2, 65, 33), accum=2, splitk=2)
    _refused(Lx.bgemm, A, B, Cm, act=1, accum=2, splitk=2)
    _refused(Lx.bgemm, A, B, Cm, accum=1, splitk=2)


def test_bindings_refuse_conv_pe_and_mean_rows(gpu):
    C, B, L, P = 2, 3, 4, 600
    x, params, h = _t(C, B, L), _t(C, P), _t(C, B * L, 64)
    Lx.conv_pe_fwd(x, params, 4, 200, 300, h)  # the valid call
    _refused(Lx.conv_pe_fwd, x, params, 4, 200, 300, _t(C, B * L - 1, 64))
    _refused(Lx.conv_pe_fwd, x, params, P - 191, 200, 300, h)
    _refused(Lx.conv_pe_fwd, x, params, 4, P - 63, 300, h)
    _refused(Lx.conv_pe_fwd, x, params, 4, 200, P - 64 * L + 1, h)
    _refused(Lx.conv_pe_fwd, x, _t(C + 1, P), 4, 200, 300, h)
    grads = _t(C, P)
    Lx.conv_pe_bwd(x, h, grads, 4, 200)
    _refused(Lx.conv_pe_bwd, x, _t(C, B * L + 1, 64), grads, 4, 200)
    _refused(Lx.conv_pe_bwd, x, h, _t(C, 195), 4, 100)   # grads row too narrow for the taps
    _refused(Lx.conv_pe_bwd, x, h, grads, 4, P - 63)
    out = _t(C, B, 64)
    Lx.mean_rows_fwd(h, B, L, out)
    _refused(Lx.mean_rows_fwd, h, B, L, _t(C, B - 1, 64))
    _refused(Lx.mean_rows_fwd, _t(C, B * L - 1, 64), B, L, out)
    Lx.mean_rows_bwd(out, B, L, h)
    _refused(Lx.mean_rows_bwd, out, B, L, _t(C, B * L - 1, 64))
    _refused(Lx.mean_rows_bwd, _t(C, B + 1, 64), B, L, h)


def test_bindings_refuse_layernorm_and_gru(gpu):
    C, Rw = 2, 5
    x, y, st, gm, bt = _t(C, Rw, 64), _t(C, Rw, 64), _t(C, Rw, 2), _t(C, 64), _t(C, 64)
    Lx.ln_fwd(x, None, None, y, st, gm, bt)
    _refused(Lx.ln_fwd, x, None, None, y, _t(C, Rw - 1, 2), gm, bt)
    _refused(Lx.ln_fwd, x, None, None, y, st, _t(C, 63), _t(C, 63))
    _refused(Lx.ln_fwd, x, None, None, y, st, gm, _t(C, 70)[:, :63])
    _refused(Lx.ln_fwd, x, None, None, y, st, gm.cpu(), bt)
    _refused(Lx.ln_fwd, x, None, None, y, st, gm, bt.cpu())
    dx, dg, db = _t(C, Rw, 64), _t(C, 64), _t(C, 64)
    Lx.ln_bwd(y, x, st, gm, dx, 0, None, dg, db)
    _refused(Lx.ln_bwd, y, x, _t(C, Rw + 1, 2), gm, dx, 0, None, dg, db)
    _refused(Lx.ln_bwd, y, _t(C, Rw - 1, 64), st, gm, dx, 0, None, dg, db)    # s of another shape
    _refused(Lx.ln_bwd, y, x, st, _t(C, 63), dx, 0, None, _t(C, 63), _t(C, 63))
    _refused(Lx.ln_bwd, y, x, st, gm, dx, 0, None, dg.cpu(), db)
    _refused(Lx.ln_bwd, y, x, st, gm, dx, 0, None, dg, db.cpu())
    _refused(Lx.ln_bwd, y, x, st, gm.cpu(), dx, 0, None, dg, db)
    B = 4
    gi, bhh, h = _t(C, B, 96), _t(C, 96), _t(C, B, 64)
    Lx.gru_fwd(gi, bhh, h, 32)
    _refused(Lx.gru_fwd, gi, bhh, h, 33)                  # h.size(2) < col0 + 32
    _refused(Lx.gru_fwd, gi, bhh, _t(C, B, 32), 32)
    _refused(Lx.gru_fwd, gi, _t(C, 95), h, 0)
    dgi, dbi, dbh = _t(C, B, 96), _t(C, 96), _t(C, 96)
    Lx.gru_bwd(h, 32, gi, bhh, dgi, dbi, dbh)
    _refused(Lx.gru_bwd, h, 33, gi, bhh, dgi, dbi, dbh)
    _refused(Lx.gru_bwd, h, 0, gi, _t(C, 95), dgi, _t(C, 95), _t(C, 95))
    _refused(Lx.gru_bwd, h, 0, gi, _t(C, 200)[:, :96], dgi, _t(C, 200)[:, :95], _t(C, 200)[:, :96])
    _refused(Lx.gru_bwd, h, 0, gi, bhh, _t(C, B - 1, 96), dbi, dbh)


def test_bindings_refuse_losses_and_gathers(gpu):
    C, B, S, E, K = 2, 3, 2, 2, 4
    i32 = torch.int32
    bsz, ep, nb = _t(S, C, dtype=i32), _t(S, C, dtype=i32), _t(C, dtype=i32) + 1
    failed, losses = _t(C, dtype=i32), _t(C, E)
    ctl = R.make_ctl(C, gpu)
    z, y, dz = _t(C, B), _t(C, B), _t(C, B)
    Lx.bce(z, y, bsz, ep, nb, ctl, failed, losses, dz)
    x, yl, dx = _t(C, B, K), _t(C, B, dtype=torch.int64), _t(C, B, K)
    Lx.ce(x, yl, bsz, ep, nb, ctl, failed, losses, dx)
    for fn, a, lab, d, bad_a, bad_l, bad_d in ((Lx.bce, z, y, dz, _t(C * B + 1), _t(C, B - 1), _t(C, B + 1)),
                                               (Lx.ce, x, yl, dx, _t(C * B + 1, K), _t(C, B + 1, dtype=torch.int64),
                                                _t(C, B, K + 1))):
        _refused(fn, bad_a, lab, bsz, ep, nb, ctl, failed, losses, d)
        _refused(fn, a, bad_l, bsz, ep, nb, ctl, failed, losses, d)
        _refused(fn, a, lab, bsz, ep, nb, ctl, failed, losses, bad_d)
        _refused(fn, a, lab, bsz, _t(S - 1, C, dtype=i32), nb, ctl, failed, losses, d)      # epoch shape != bsz shape
        _refused(fn, a, lab, bsz, ep, _t(C - 1, dtype=i32) + 1, ctl, failed, losses, d)     # nb length
        _refused(fn, a, lab, bsz, ep, nb, ctl, _t(C - 1, dtype=i32), losses, d)             # failed length
    assert int(failed.sum()) == 0 and float(losses.abs().sum()) == 0.0  # bs = 0 everywhere: nothing was touched
    rows, idx = _t(10, 24), _t(S, C, B, dtype=i32)
    vit, lab, yy = _t(C, B, 7), _t(C, B, 16), _t(C, B)
    Lx.gather_icu(rows, idx, ctl, False, vit, lab, yy)
    short = Lx.StepCtl(ctl.seeds, ctl.stepctl[:2].contiguous())
    empty = _t(0, C, B, dtype=i32)
    _refused(Lx.gather_icu, rows, idx, short, False, vit, lab, yy)
    _refused(Lx.gather_icu, rows, empty, ctl, False, vit, lab, yy)
    hx, hy, ox, oy = _t(10, 5), _t(10, dtype=torch.int64), _t(C, B, 5), _t(C, B, dtype=torch.int64)
    Lx.gather_har(hx, hy, idx, ctl, ox, oy)
    _refused(Lx.gather_har, hx, hy, idx, short, ox, oy)
    _refused(Lx.gather_har, hx, hy, empty, ctl, ox, oy)
