"""The issue priorities of the quad kernel (quad_kernel.h: CVXQ_PRIO_ROUND2 / CVXQ_PRIO_BEHIND) in the emitted gfx950 code.

s_setprio is a scalar instruction that ignores EXEC: a raise the compiler emits unconditionally gives every wavefront the same level and is a
no-op, and nothing else would notice -- results do not depend on priorities.  So the code of the SHIPPED library is disassembled (no
compile: the library of cvxpnpl_amd.build is reused) and the kernel of bench.py's default run must hold a raise to a non-zero level, each
one right behind a scalar conditional branch that skips it; and the same translation unit compiled with -DCVXQ_NO_PRIO (the A/B switch; one
device-only compile to assembly, minutes) must hold no s_setprio at all.  No GPU needed: hipcc cross-compiles."""
import os
import re
import shutil
import subprocess
import tempfile

JUDGED = "_ZN4cvxq17solve_quad_kernelILi0ELi2ELi16ELb1ELi0EEEvNS_8QuadArgsE"  # cvxq::solve_quad_kernel<0, 2, 16, true, 0>(cvxq::QuadArgs)


def _llvm_tool(name):
    from cvxpnpl_amd import build as b

    rocm = os.path.dirname(os.path.dirname(os.path.realpath(b.hipcc())))
    for c in (os.path.join(rocm, "llvm", "bin", name), os.path.join(rocm, "lib", "llvm", "bin", name), shutil.which(name)):
        if c and os.path.exists(c):
            return c
    raise RuntimeError(f"{name} not found beside {b.hipcc()}")


def _function(lines, symbol):
    """the instruction lines of one function of a disassembly / an assembly listing"""
    out, inside = [], False
    for l in lines:
        if re.match(r"^(?:[0-9a-f]+ <)?" + re.escape(symbol) + r">?:", l):
            inside = True
            continue
        if inside:
            if re.match(r"^[0-9a-f]+ <[^>+]+>:", l) or l.startswith(".Lfunc_end") or l.lstrip().startswith(".end_amdhsa_kernel"):
                break
            t = l.strip()
            if t and not t.startswith((";", ".", "//")) and not re.match(r"^<?[.\w$]+>?:", t):
                out.append(t)
    return out


def test_shipped_judged_kernel_raises_priority_behind_scalar_branches():
    from cvxpnpl_amd import build as b

    lib = b.build()
    objdump = _llvm_tool("llvm-objdump")
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(lib, so)
        subprocess.run([objdump, "--offloading", so], check=True, capture_output=True)  # writes lib.so.<n>.<target> beside it
        objs = [os.path.join(tmp, f) for f in sorted(os.listdir(tmp)) if "gfx950" in f]
        assert objs, os.listdir(tmp)
        body = []
        for o in objs:
            dis = subprocess.run([objdump, "-d", "--no-show-raw-insn", "--mcpu=gfx950", o], check=True, capture_output=True, text=True).stdout
            body += _function(dis.splitlines(), JUDGED)
    assert len(body) > 5000, len(body)  # (the kernel is ~9 000 instructions)
    raises = [i for i, l in enumerate(body) if l.split()[0] == "s_setprio"]
    levels = [int(body[i].split()[1], 0) for i in raises]
    assert len(raises) == 2 and all(0 < v <= 3 for v in levels), [body[i] for i in raises]
    assert levels[0] < levels[1], levels  # second-round start below the level of a wavefront that is behind
    for i in raises:
        # the instruction in front is the scalar branch that skips the raise (its target: the instruction behind it)
        assert re.match(r"s_cbranch_(scc|vccn?z)", body[i - 1]), body[i - 3:i + 2]
    assert not [l for l in body if re.match(r"s_setprio\s+0\b", l)]  # never lowered again


def test_no_prio_switch_compiles_every_setprio_out():
    from cvxpnpl_amd import build as b

    cmd = b.compile_cmd()
    flags = [c for c in cmd[1:cmd.index("-o")] if c not in ("-shared",) and not c.startswith("-Rpass")]
    with tempfile.TemporaryDirectory() as tmp:
        s = os.path.join(tmp, "noprio.s")
        r = subprocess.run([cmd[0]] + flags + ["-DCVXQ_NO_PRIO", "--cuda-device-only", "-S", "-o", s, b.SRC], stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        text = open(s).read()
    assert len(_function(text.splitlines(), JUDGED)) > 5000
    assert "solve_quad_kernel" in text and "s_setprio" not in text.lower()
