"""The one table of the server rules' engine knobs (config.RULE_KNOBS): defaults, validation, the engine's keywords and
the rules' signatures all come from it."""
import inspect

import pytest

from attackfl_amd import agg
from attackfl_amd.config import RULE_KNOBS, from_dict
from attackfl_amd.fl.engine import FLEngine


def test_defaults_and_bad_values_per_row():
    engine = from_dict({}).engine
    for k in RULE_KNOBS:
        assert engine[k.key] == k.default and type(engine[k.key]) is type(k.default), k.key
        if k.lo is None and k.kind == "int":
            for v in (0, True):  # (gmm-rank: unchecked, as before the table)
                from_dict({"engine": {k.key: v}})
            continue
        # a bool, a wrong type, a value out of range
        for bad in (True, [1], -1 if k.kind == "int" else 0.0):
            with pytest.raises(ValueError, match=f"engine.{k.key} must be "):
                from_dict({"engine": {k.key: bad}})
        with pytest.raises(ValueError, match=k.key):
            from_dict({"engine": {k.key: "2" if k.kind == "int" else "x"}})
        if k.kind == "number":
            assert from_dict({"engine": {k.key: "1e-6"}}).engine[k.key] == "1e-6"  # (YAML 1.1: a string, a valid number)
        assert (from_dict({"engine": {k.key: "auto"}}).engine[k.key] == "auto") if k.auto else True


def test_rule_args_keys_and_coercion():
    cfg = from_dict({"engine": {"gmm-rank": 2, "byz-f": 1, "geomed-iters": 7, "geomed-nu": "1e-5", "dnc-iters": 2,
                                "dnc-sub-dim": 300, "dnc-c": 2, "cclip-iters": 4, "cclip-tau": "1e-3"}})
    eng = FLEngine.__new__(FLEngine)  # (_rule_args reads these four attributes only)
    eng.cfg, eng.seed, eng.round_no, eng.global_params = cfg, 3, 5, None
    kw = eng._rule_args()
    assert set(kw) == {"seed", "gmm_rank", "byz_f", "geomed_iters", "geomed_nu", "dnc_iters", "dnc_sub_dim", "dnc_c",
                       "centre", "cclip_iters", "cclip_tau"}
    want = {"seed": 3 * 13 + 5, "gmm_rank": 2, "byz_f": 1, "geomed_iters": 7, "geomed_nu": 1e-5, "dnc_iters": 2,
            "dnc_sub_dim": 300, "dnc_c": 2.0, "centre": None, "cclip_iters": 4, "cclip_tau": 1e-3}
    assert kw == want and all(type(kw[n]) is type(v) for n, v in want.items())
    eng.cfg = from_dict({})
    kw = eng._rule_args()
    assert (kw["byz_f"], kw["cclip_tau"], kw["geomed_nu"], kw["dnc_sub_dim"]) == ("auto", "auto", 1e-6, 10000)


def test_every_keyword_reaches_a_rule():
    params = {name for fn in agg.AGGREGATORS.values() for name in inspect.signature(fn).parameters}
    for k in RULE_KNOBS:
        assert k.kw in params, k.kw
