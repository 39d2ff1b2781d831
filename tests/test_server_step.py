"""``FLEngine._server_step`` on a CPU engine: the contract the early launch relies on on the device — with a
success flag the step selects between the serial path's new global model and the old one, bit for bit."""
import pytest
import torch

from attackfl_amd.agg import AGGREGATORS
from attackfl_amd.config import from_dict
from attackfl_amd.fl.engine import FLEngine


@pytest.fixture(scope="module")
def rows():
    """Five update rows around an old global model (the last one an outlier flagged as attacker) and their sizes."""
    from attackfl_amd.models import ParamLayout

    P = ParamLayout.for_model("TransformerModel").P
    g = torch.Generator().manual_seed(0)
    g_old = 0.1 * torch.randn(P, generator=g)
    U = g_old[None, :] + 0.01 * torch.randn(5, P, generator=g)
    U[4] += 0.05 * torch.randn(P, generator=g)
    return g_old, U, torch.tensor([310.0, 420.0, 365.0, 500.0, 300.0], dtype=torch.float64), \
        torch.tensor([False, False, False, False, True])


@pytest.mark.parametrize("mode", sorted(AGGREGATORS))
def test_server_step_flag_selects_new_or_old_model(tmp_path, rows, mode):
    g_old, U, sizes, attackers = rows
    d = {
        "server": {"num-round": 4, "clients": 5, "mode": mode, "model": "TransformerModel", "data-name": "ICU",
                   "data-distribution": {"num-data-range": [300, 500]}},
        "learning": {"epoch": 2, "batch-size": 128},
        "data": {"synthetic": True, "train-size": 4000, "test-size": 1000},
        "engine": {"checkpoint-dir": str(tmp_path), "trainer": "eager", "seed": 3},
        "log_path": str(tmp_path),
    }
    eng = FLEngine(from_dict(d), device="cpu", verbose=False)
    eng.client_selection()

    def step(ok_all):
        eng.global_params = g_old.clone()
        info, rule_ok = eng._server_step(U, sizes, attackers, ok_all)
        assert rule_ok is None or bool(rule_ok)  # (only gmm reports a success of its own; it keeps rows here)
        return info, eng.global_params

    info0, serial = step(None)
    assert "agg_failed" not in info0 and not torch.equal(serial, g_old)  # (the rule ran: the checks below bite)
    assert serial.untyped_storage().data_ptr() != U.untyped_storage().data_ptr()  # (Krum's row: cloned)
    info1, new = step(torch.tensor(True))
    assert torch.equal(new, serial) and new.dtype == torch.float32
    info2, old = step(torch.tensor(False))
    assert torch.equal(old, g_old)
    assert info1.keys() == info0.keys() == info2.keys()
    if mode == "gmm":
        assert info2["kept"] == info0["kept"] and info2["threshold"] == info0["threshold"]
        assert info0["kept"] and info0["threshold"] > 0.0
    eng.close()


def _failed_launch(eng, mark):
    """A hand-built early launch without attackers (``keep`` None) whose round failed, run through the rollback."""
    import numpy as np

    from attackfl_amd.fl.engine import EarlyLaunch

    g_old = torch.zeros(eng.P)
    esl = EarlyLaunch(g_old=g_old, mode_mark=mark, snap=([], eng.server_rng.getstate()), prep=None, keep=None)
    eng.global_params = torch.ones(eng.P)  # (what the step assigned)
    eng._early_launch_failed(esl, np.array([True, False, True, True]))
    return g_old


def _small_engine(tmp_path, mode):
    d = {
        "server": {"num-round": 2, "clients": 4, "mode": mode, "model": "TransformerModel", "data-name": "ICU",
                   "data-distribution": {"num-data-range": [150, 260]}},
        "learning": {"epoch": 1, "batch-size": 64},
        "data": {"synthetic": True, "train-size": 1500, "test-size": 400},
        "engine": {"checkpoint-dir": str(tmp_path), "trainer": "eager"},
        "log_path": str(tmp_path),
    }
    return FLEngine(from_dict(d), device="cpu", verbose=False)


def test_failed_early_launch_hands_the_mark_back(tmp_path):
    """``_early_launch_failed`` restores the global model itself and leaves the rest to the mode: ``undo`` gets the
    very object ``mark`` returned, once."""
    from attackfl_amd.fl.server_modes import ServerMode

    class Stub(ServerMode):
        def __init__(self, eng):
            super().__init__(eng)
            self.token, self.undone = object(), []

        def mark(self):
            return self.token

        def undo(self, mark):
            self.undone.append(mark)

    eng = _small_engine(tmp_path, "fedavg")
    eng.server = stub = Stub(eng)
    g_old = _failed_launch(eng, eng.server.mark())
    assert len(stub.undone) == 1 and stub.undone[0] is stub.token
    assert eng.global_params is g_old
    eng.close()


def test_failed_early_fltrust_round_checks_its_root_training(tmp_path):
    """FLTrust's rollback reads the result of the server model's training before it drops the handle (a hand-off
    timeout raises there too), and puts the server model back."""
    from attackfl_amd.fl.server_modes import FLTrustMode

    class Handle:
        def __init__(self, error=None):
            self.calls, self.error = 0, error

        def result(self):
            self.calls += 1
            if self.error is not None:
                raise self.error
            return [True], torch.zeros(1, 1)

    eng = _small_engine(tmp_path, "FLTrust")
    mode = eng.server
    assert isinstance(mode, FLTrustMode)
    mark = mode.mark()
    assert mark is mode.model
    mode.model, mode.trust, mode._pending = mark + 1.0, torch.ones(4), Handle()  # (what the step left behind)
    handle = mode._pending
    g_old = _failed_launch(eng, mark)
    assert handle.calls == 1 and mode._pending is None
    assert mode.model is mark and mode.trust is None and eng.global_params is g_old
    mode._pending = handle = Handle(RuntimeError("a cross-workgroup hand-off timed out"))
    with pytest.raises(RuntimeError, match="hand-off timed out"):
        _failed_launch(eng, mark)
    assert handle.calls == 1 and mode._pending is None
    eng.close()
