"""The Gram pass, the DnC kernels and the one-wave n <= 64 kernels of agg.hip, pinned bit for bit to the build before
their launch and load steps were shared (gram_for_tiles, lds_load_square, the bindings' one two-pass Gram): every output
tensor of every case hashes to what that build returned (tests/golden/agg_bits.json, recorded on an MI355X with the
kernels of the commit named there).  Any later folding of these kernels has this file to answer to.

    python tests/test_gpu_agg_bits.py <commit> [out.json]      records the golden file

Shapes: K in {1, 2, 3, 16, 17, 33, 64} covers the tile counts T = 1 .. 4 and their edges, P in {1, 5, 1023, 1025, 3001}
a partial 16-column step, one column into a second block and three blocks; K = 9 with an outlier in row 0 runs pass 2
on a centre != 0.  DnC at P = 2049: b = 1 (one position), 1025 (permuted, a second block of one position), 2049 and
5000 (natural order at and beyond P)."""
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

import test_agr_attacks as A
import test_cclip as R
from attackfl_amd import ops
from attackfl_amd.ops import composite as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agg_bits.json")


def _cases():
    out = {}
    for K, P in [(K, 1025) for K in (1, 2, 3, 16, 17, 33, 64)] + [(17, P) for P in (1, 5, 1023, 3001)]:
        out[f"gram_K{K}_P{P}"] = {"op": "gram", "n": K, "P": P, "rows": "plain"}
    out["gram_K9_P3001_outlier0"] = {"op": "gram", "n": 9, "P": 3001, "rows": "outlier0"}
    out["gram_K9_P1025_nan"] = {"op": "gram", "n": 9, "P": 1025, "rows": "nan"}
    for n, b, iters, drop in ((3, 1, 1, 0), (17, 1025, 3, 1), (33, 2049, 1, 32), (64, 5000, 3, 1), (17, 5000, 1, 16)):
        out[f"dnc_n{n}_b{b}"] = {"op": "dnc", "n": n, "P": 2049, "rows": "plain", "b": b, "iters": iters, "drop": drop,
                                 "seed": 77}
    for n in (1, 2, 7, 33, 64):
        for it in (0, 1):
            out[f"krum_n{n}_it{it}"] = {"op": "krum", "n": n, "P": 1025, "rows": "plain", "iterated": it}
    for it in (0, 1):
        out[f"krum_n7_tied_it{it}"] = {"op": "krum", "n": 7, "P": 1025, "rows": "tied", "iterated": it}
    for n in (3, 37, 64):
        out[f"geomed_n{n}"] = {"op": "geomed", "n": n, "P": 1025, "rows": "plain", "iters": 100, "nu": 1e-6}
    for n in (3, 17, 64):
        for tau in ("auto", 1.0):
            out[f"cclip_n{n}_{tau}"] = {"op": "cclip", "n": n, "P": 1025, "rows": "plain", "iters": 3, "tau": tau,
                                        "anchored": 1}
    out["cclip_n17_centred"] = {"op": "cclip", "n": 17, "P": 1025, "rows": "plain", "iters": 3, "tau": "auto",
                                "anchored": 0}
    out["cclip_n17_nan"] = {"op": "cclip", "n": 17, "P": 1025, "rows": "nan", "iters": 3, "tau": "auto", "anchored": 1}
    out["cclip_n17_tied"] = {"op": "cclip", "n": 17, "P": 1025, "rows": "tied", "iters": 3, "tau": "auto",
                             "anchored": 1}
    for target in C.AGR_TARGETS:
        out[f"agr_{target}"] = {"op": "agr", "n": 7, "P": 63, "m": 2, "f": 1, "target": target, "n_iter": 9}
    out["gmm_n8"] = {"op": "gmm", "n": 8, "P": 1025, "rows": "plain", "rank": 0}
    return out


CASES = _cases()


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def rows_of(n, P, kind):
    """test_cclip.make_rows (a seeded CPU generator); ``outlier0``: row 0 far from the bulk; ``nan``: one NaN row;
    ``tied``: rows 1 .. 3 (those that exist) equal to row 0."""
    U, sizes, centre = R.make_rows(n, P)
    U = U.clone()
    if kind == "outlier0":
        U[0] = 50.0 * U[0] + 7.0
    elif kind == "nan":
        U[2] = float("nan")
    elif kind == "tied":
        for r in range(1, min(4, n)):
            U[r] = U[0]
    else:
        assert kind == "plain"
    return U, sizes, centre


def run_case(c, gpu):
    """Runs the case's ops on the device -> {output name: sha256}."""
    if c["op"] == "agr":
        G, _, _, _, a, b, cc = A.inputs(c["n"], c["P"])
        st = ops.agr_bisect_fused(ops.pairwise_sqdist(G.to(gpu)), a.to(gpu), b.to(gpu), cc.to(gpu), c["m"], c["f"],
                                  c["target"], c["n_iter"], A.GAMMA0)
        return {"st": _sha(st)}
    U, sizes, centre = rows_of(c["n"], c["P"], c["rows"])
    Ud, g = U.to(gpu), centre.to(gpu)
    alpha = (sizes.double() / sizes.double().sum()).to(gpu)
    if c["op"] == "gram":
        return {"D": _sha(ops.pairwise_sqdist(Ud)), "centred": _sha(ops.centred_gram(Ud)),
                "anchored": _sha(ops.gram_anchored(Ud, g))}
    if c["op"] == "dnc":
        H = ops.dnc_gram(Ud, c["b"], c["iters"], c["seed"])
        keep, scores, weights = ops.dnc_filter(Ud, c["b"], c["iters"], c["seed"], c["drop"], sizes.double().to(gpu))
        return {"gram": _sha(H), "keep": _sha(keep), "scores": _sha(scores), "weights": _sha(weights)}
    if c["op"] == "krum":
        n = c["n"]
        f = max(0, (n - 3) // 4)
        rounds = max(1, n - 2 * f if c["iterated"] else n - f)
        sel, mask, scores = ops.krum_select(ops.pairwise_sqdist(Ud), f, rounds, bool(c["iterated"]))
        return {"sel": _sha(sel), "mask": _sha(mask), "scores": _sha(scores)}
    if c["op"] == "geomed":
        w, it, obj = ops.geomed_weights(ops.centred_gram(Ud), alpha, c["iters"], c["nu"])
        return {"w": _sha(w), "iters": _sha(it), "objective": _sha(obj)}
    if c["op"] == "cclip":
        G = ops.gram_anchored(Ud, g) if c["anchored"] else ops.centred_gram(Ud)
        c0 = torch.zeros_like(alpha) if c["anchored"] else alpha
        co, tau, clipped, fin = ops.cclip_weights(G, alpha, c0, c["iters"], c["tau"])
        return {"c": _sha(co), "tau": _sha(tau), "clipped": _sha(clipped), "finite": _sha(fin)}
    assert c["op"] == "gmm"
    att = torch.tensor([i >= c["n"] - 2 for i in range(c["n"])])
    keep, info = ops.gmm_filter(ops.centred_gram(Ud), att, c["rank"])
    return {"keep": _sha(keep), "info": _sha(info)}


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_match_parent_build(gpu, name):
    gold = _golden()["cases"][name]
    assert gold["case"] == CASES[name]
    got = run_case(CASES[name], gpu)
    print(got)
    assert got == gold["sha256"]
    assert run_case(CASES[name], gpu) == got  # (a second call: the same bits)


if __name__ == "__main__":
    dev = torch.device("cuda", 0)
    ops.native()
    rec = {"parent_commit": sys.argv[1], "cases": {}}
    for name in sorted(CASES):
        got = run_case(CASES[name], dev)
        assert run_case(CASES[name], dev) == got, name
        rec["cases"][name] = {"case": CASES[name], "sha256": got}
    with open(sys.argv[2] if len(sys.argv) > 2 else GOLDEN, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded", len(rec["cases"]), "cases")
