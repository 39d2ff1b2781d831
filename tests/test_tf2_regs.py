"""Register allocation of the on-chip trainers, read from their gfx950 assembly through tools/isa_phase_counts.py
(CPU: hipcc cross-compiles).  tf2.hip's kernels live in one register class: no AGPRs (so no v_accvgpr copies on the
VALU-issue-bound step chain), no scratch, two waves per SIMD.  rnn2.hip keeps its AGPR-resident W_ih tiles: its figures
are those of the commit before tf2.hip changed class.  All three trainers are built from csrc/kernels/onchip.h, so
the allocation of every one of their kernels is pinned here: a change to the shared header that moves any of them
shows up without a GPU."""
import functools
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import isa_phase_counts as I  # noqa: E402

needs_hipcc = pytest.mark.skipif(not shutil.which(I.HIPCC), reason="needs hipcc")

# rnn2.hip / rnn2_stamps.hip at the parent commit (NumVgprs, NumAgprs, ScratchSize, Occupancy)
RNN2_PARENT = {
    ("rnn2.hip", "k_rnn2_train"): (128, 128, 68, 2),
    ("rnn2.hip", "k_rnn2_eval"): (114, 0, 0, 4),
    ("rnn2_stamps.hip", "k_rnn2_train_stamped"): (128, 128, 68, 2),
}
# cnn2.hip and k_tf2_train at the commit before cnn2.hip moved onto onchip.h (the same four figures)
CNN2_PARENT = {
    ("cnn2.hip", "k_cnn2_train"): (230, 0, 0, 2),
    ("cnn2.hip", "k_cnn2_eval"): (172, 0, 0, 2),
}
TF2_PARENT_VGPRS = 256


@functools.lru_cache(maxsize=None)
def _asm(name):
    return I.compile_asm(os.path.join(ROOT, "csrc", "kernels", name))


def _figures(name):
    return {I.short(k): d for k, d in I.kernel_info(_asm(name)).items()}


@needs_hipcc
@pytest.mark.parametrize("name,kernel", [("tf2.hip", "k_tf2_train"), ("tf2_stamps.hip", "k_tf2_train_stamped")])
def test_tf2_one_register_class(name, kernel):
    d = _figures(name)[kernel]
    print(name, kernel, d)
    assert d["NumAgprs"] == 0
    assert d["ScratchSize"] == 0
    assert d["Occupancy"] == 2
    # and no copy between the classes anywhere in the kernel's regions
    for k, regs in I.phase_counts(_asm(name)).items():
        assert sum(cnt["agpr"] for _, _, cnt in regs) == 0, k


@needs_hipcc
def test_tf2_marks_cover_both_branches():
    """The step's marks appear once per branch instantiation, in program order."""
    regs = I.phase_counts(_asm("tf2.hip"))
    (k, rows), = [(k, r) for k, r in regs.items() if r]
    names = [(n, i) for n, i, _ in rows]
    for inst in (0, 1):
        for n in ("fwd..fwd_end", "fwd_end..bwd", "bwd..bwd_end", "upd..upd_end"):
            assert (n, inst) in names
    fwd = {i: c for n, i, c in rows if n == "fwd..fwd_end"}
    assert all(c["mfma"] > 0 and c["valu"] + c["pk"] > 100 for c in fwd.values())


@needs_hipcc
@pytest.mark.parametrize("name,kernel", sorted(RNN2_PARENT))
def test_rnn2_allocation_unchanged(name, kernel):
    d = _figures(name)[kernel]
    print(name, kernel, d)
    assert (d["NumVgprs"], d["NumAgprs"], d["ScratchSize"], d["Occupancy"]) == RNN2_PARENT[(name, kernel)]


@needs_hipcc
@pytest.mark.parametrize("name,kernel", sorted(CNN2_PARENT))
def test_cnn2_allocation_unchanged(name, kernel):
    d = _figures(name)[kernel]
    print(name, kernel, d)
    assert (d["NumVgprs"], d["NumAgprs"], d["ScratchSize"], d["Occupancy"]) == CNN2_PARENT[(name, kernel)]


@needs_hipcc
def test_tf2_vgpr_count_unchanged():
    d = _figures("tf2.hip")["k_tf2_train"]
    print("tf2.hip k_tf2_train", d)
    assert d["NumVgprs"] == TF2_PARENT_VGPRS


ASM = """\
\t.amdhsa_kernel _Z3k_av
_Z3k_av:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\t;MARK a
\tv_add_f32_e32 v1, v2, v3
\tv_pk_mul_f32 v[4:5], v[4:5], v[6:7]
\tv_accvgpr_write_b32 a0, v1
\tv_mfma_f32_16x16x32_bf16 v[0:3], v[4:7], v[8:11], 0
\tv_rcp_f32_e32 v1, v1
.LBB0_1:
\tds_read_b64 v[2:3], v9
\tbuffer_load_dword v1, v2, s[0:3], 0 offen
\ts_waitcnt vmcnt(0)
\ts_nop 1
\ts_add_i32 s0, s0, 1
\t;MARK b
\tv_mov_b32_e32 v1, 0
\t;MARK a
\tv_mov_b32_e32 v1, 0
\tv_mov_b32_e32 v2, 0
\t;MARK b
\ts_endpgm
; NumVgprs: 12
; NumAgprs: 1
; ScratchSize: 0
; Occupancy: 8
"""


def test_counts_by_class_and_instantiation(tmp_path):
    p = tmp_path / "k.s"
    p.write_text(ASM)
    info = I.kernel_info(str(p))["_Z3k_av"]
    assert (info["NumVgprs"], info["NumAgprs"], info["ScratchSize"], info["Occupancy"]) == (12, 1, 0, 8)
    rows = I.phase_counts(str(p))["_Z3k_av"]
    assert [(n, i) for n, i, _ in rows] == [("a..b", 0), ("b..a", 0), ("a..b", 1)]
    c = rows[0][2]
    assert [c[k] for k in I.CLASSES] == [1, 1, 1, 1, 1, 1, 1, 2, 1]
    assert rows[2][2]["valu"] == 2
    assert I.short("_Z3k_av") == "k_a" and I.short("_ZN2r211k_rnn2_evalEPKflS1_iPf") == "k_rnn2_eval"
    assert "| a..b | 1 |" in I.report(str(p), "t")
