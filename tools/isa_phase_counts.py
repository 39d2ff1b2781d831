"""Static instruction counts of a kernel file's gfx950 ISA, per ``;MARK`` region (CPU only: hipcc cross-compiles).

The on-chip trainers' step chains are VALU-issue-bound (docs/ARCHITECTURE.md 2.1b), so the number of instructions a
wave issues per phase is the CPU-side yardstick for a change to them.  The kernels carry ``asm volatile(";MARK x")``
labels at their phase boundaries; this tool compiles one file with the device flags of attackfl_amd/_build.py (plus
optional -D's), and prints for every kernel
  * the register / scratch / occupancy figures of the assembly's kernel-info comments, and
  * for every region between two consecutive marks, and every template instantiation of it (the n-th time the same
    mark appears in the kernel), the instructions by class: VALU, packed VALU, transcendental, AGPR copies, MFMA, LDS,
    vector memory, waits / nops, scalar.
Classes are decided by mnemonic prefix alone.  The counts are static (what lies between the marks in program order):
a loop body counts once, both sides of a branch count.

    python tools/isa_phase_counts.py csrc/kernels/tf2.hip [-DNAME[=V] ...] [--title T]
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from attackfl_amd import _build  # noqa: E402

HIPCC = os.path.join(_build.ROCM, "bin", "hipcc")
CLASSES = ("valu", "pk", "trans", "agpr", "mfma", "lds", "vmem", "wait", "scalar")
HEAD = ("VALU", "packed", "transc.", "AGPR copies", "MFMA", "LDS", "vector mem", "waits / nops", "scalar")
TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")
INFO = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "Occupancy")
INSN = re.compile(r"^\s+([a-z][a-z_0-9]*)(\s|$)")
KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
LABEL = re.compile(r"^([A-Za-z_][\w$.]*):")
MARK = re.compile(r"^\s*;MARK\s+(\S+)")
INFO_RE = re.compile(r"^;\s*(\w+):\s*(\d+)\s*$")


def device_flags(path):
    """The device compile line of attackfl_amd/_build.py for this file (device side only, to assembly)."""
    return _build.device_flags(path) + ["--cuda-device-only", "-S"]


def compile_asm(path, defines=(), out=None):
    """Compile `path` to gfx950 assembly; returns the .s path (in a fresh temporary directory unless `out`)."""
    out = out or os.path.join(tempfile.mkdtemp(prefix="isa_"), os.path.basename(path) + ".s")
    r = subprocess.run([HIPCC] + device_flags(path) + list(defines) + [path, "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"compile failed: {path}\n{r.stderr}")
    return out


def classify(op):
    if op.startswith("v_accvgpr_"):
        return "agpr"
    if op.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if op.startswith("v_pk_"):
        return "pk"
    if op.startswith(TRANS):
        return "trans"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith(("s_waitcnt", "s_nop", "s_sleep", "s_barrier")):
        return "wait"
    if op.startswith("s_"):
        return "scalar"
    return None


def kernel_names(asm_path):
    with open(asm_path) as fh:
        return [m.group(1) for m in map(KERNEL.match, fh) if m]


def kernel_info(asm_path):
    """{kernel: {NumVgprs: ..., NumAgprs: ..., ScratchSize: ..., Occupancy: ...}} from the kernel-info comments"""
    kernels = set(kernel_names(asm_path))
    out, cur = {}, None
    with open(asm_path) as fh:
        for l in fh:
            m = LABEL.match(l)
            if m and m.group(1) in kernels:
                cur = out.setdefault(m.group(1), {})
                continue
            m = INFO_RE.match(l)
            if m and cur is not None and m.group(1) in INFO and m.group(1) not in cur:
                cur[m.group(1)] = int(m.group(2))
    return out


def phase_counts(asm_path):
    """{kernel: [(region, instantiation, Counter by class)]}; region "a..b" runs from mark a to the next mark b"""
    kernels = set(kernel_names(asm_path))
    out, cur, open_region, seen = {}, None, None, None
    with open(asm_path) as fh:
        for l in fh:
            m = LABEL.match(l)
            if m and not m.group(1).startswith(".L"):
                cur = out.setdefault(m.group(1), []) if m.group(1) in kernels else None
                open_region, seen = None, collections.Counter()
                continue
            if cur is None:
                continue
            m = MARK.match(l)
            if m:
                if open_region is not None:
                    name, inst, cnt = open_region
                    cur.append((f"{name}..{m.group(1)}", inst, cnt))
                open_region = (m.group(1), seen[m.group(1)], collections.Counter())
                seen[m.group(1)] += 1
                continue
            m = INSN.match(l)
            if m and open_region is not None:
                if m.group(1) == "s_endpgm":
                    open_region = None
                    continue
                c = classify(m.group(1))
                if c:
                    open_region[2][c] += 1
    return out


def short(name):
    """_Z11k_tf2_train14AflTfTrainArgs -> k_tf2_train, _ZN2r211k_rnn2_evalEPKf... -> k_rnn2_eval (the last component
    of a plain or nested Itanium name; anything else is returned as it is)"""
    m = re.match(r"_ZN?", name)
    pos, last = (m.end() if m else 0), None
    while m:
        n = re.match(r"\d+", name[pos:])
        if not n:
            break
        pos += n.end()
        last = name[pos:pos + int(n.group())]
        pos += int(n.group())
        if not name.startswith("_ZN"):
            break
    return last or name


def report(asm_path, title):
    info, phases = kernel_info(asm_path), phase_counts(asm_path)
    lines = [f"## {title}", "", "| kernel | " + " | ".join(INFO) + " |", "|---|" + "---|" * len(INFO)]
    for k, d in info.items():
        lines.append(f"| `{short(k)}` | " + " | ".join(str(d.get(i, "?")) for i in INFO) + " |")
    for k, regs in phases.items():
        if not regs:
            continue
        lines += ["", f"`{short(k)}`, instructions between marks (static, per wave):", "",
                  "| region | inst. | " + " | ".join(HEAD) + " |", "|---|---|" + "---|" * len(HEAD)]
        for name, inst, cnt in regs:
            lines.append(f"| {name} | {inst} | " + " | ".join(str(cnt[c]) for c in CLASSES) + " |")
    return "\n".join(lines) + "\n"


def main(argv):
    defines = [a for a in argv if a.startswith("-D")]
    rest = [a for a in argv if not a.startswith("-D")]
    title = None
    if "--title" in rest:
        i = rest.index("--title")
        title = rest[i + 1]
        del rest[i:i + 2]
    if len(rest) != 1:
        sys.exit(__doc__)
    path = rest[0]
    title = title or (os.path.relpath(os.path.abspath(path), ROOT) + (" " + " ".join(defines) if defines else ""))
    with tempfile.TemporaryDirectory() as td:
        print(report(compile_asm(path, defines, os.path.join(td, "k.s")), title))


if __name__ == "__main__":
    main(sys.argv[1:])
