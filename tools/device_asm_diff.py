#!/usr/bin/env python3
"""Is the device code of the working tree the same text as that of a revision?

    python tools/device_asm_diff.py REV [file.hip ...]      (default: the five refinement entry files)

Each .hip is compiled to device assembly twice -- from the working tree and from REV (taken out with `git archive` into a temporary
directory) -- with the flags of its library's compile command in that tree's cvxpnpl_amd/build.py plus
`-fuse-cuid=none --cuda-device-only -S`, and the two texts are compared: per translation unit, and per kernel (the text is split at the
`.globl` of every symbol).  An extraction that moves code between headers without changing what the compiler sees leaves the text
byte-identical, which proves equal behaviour and equal speed without a GPU.  Text only: nothing here looks inside an instruction.
Exit status 0: all identical; 1: a difference; 2: could not compare.
"""
import argparse
import concurrent.futures
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["refine_hip.hip", "refine_grad_hip.hip", "refine_robust_hip.hip", "refine_robust_grad_hip.hip", "refine_robust_auto_hip.hip"]
DROP = {"-shared", "-fPIC", "-Rpass-analysis=kernel-resource-usage"}


def device_cmds(tree):
    """{basename of a .hip: the compiler and flags of the command that compiles it, without sources, output and link flags}"""
    spec = importlib.util.spec_from_file_location("build_of_" + re.sub(r"\W", "_", tree), os.path.join(tree, "cvxpnpl_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cmds = {}
    for name in dir(mod):
        if not name.endswith(("compile_cmd", "_command")):  # (the thirteenth library on names its command ransac_*_command)
            continue
        cmd = getattr(mod, name)("OUT")
        flags = [c for i, c in enumerate(cmd) if c not in DROP and c != "-o" and cmd[i - 1] != "-o" and not c.endswith((".hip", ".cpp"))]
        for c in cmd:
            if c.endswith(".hip"):
                cmds[os.path.basename(c)] = flags
    return cmds


def device_asm(tree, cmds, hip, out):
    if hip not in cmds:
        raise SystemExit(f"{hip}: no compile command in {tree}/cvxpnpl_amd/build.py names it")
    cmd = cmds[hip] + ["-fuse-cuid=none", "--cuda-device-only", "-S", "-o", out, os.path.join(tree, "cvxpnpl_amd", "csrc", hip)]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(f"{hip}: the compile in {tree} failed")
    with open(out) as f:
        return f.read()


def sections(text):
    """[(symbol, text)] in file order: what precedes the first .globl under "(head)", the metadata note under "(metadata)" """
    out, name, cur = [], "(head)", []
    for line in text.splitlines(keepends=True):
        m = re.match(r"\s*\.globl\s+(\S+)", line)
        if m or line.lstrip().startswith(".amdgpu_metadata"):
            out.append((name, "".join(cur)))
            name, cur = (m.group(1) if m else "(metadata)"), []
        cur.append(line)
    out.append((name, "".join(cur)))
    return out


def demangled(names):
    try:
        r = subprocess.run(["c++filt"] + names, capture_output=True, text=True)
        got = r.stdout.splitlines()
        return got if r.returncode == 0 and len(got) == len(names) else names
    except OSError:
        return names


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rev")
    ap.add_argument("files", nargs="*", default=DEFAULT)
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1), help="compiles at a time")
    ap.add_argument("--keep", metavar="DIR", help="leave the assembly texts (NAME.new.s, NAME.old.s) in DIR")
    args = ap.parse_args()
    files = [os.path.basename(f) for f in args.files]
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "old")
        os.mkdir(old)
        ar = subprocess.run(["git", "-C", ROOT, "archive", "--format=tar", args.rev, "cvxpnpl_amd", "include"], stdout=subprocess.PIPE)
        if ar.returncode != 0:
            return 2
        subprocess.run(["tar", "-x", "-C", old], input=ar.stdout, check=True)
        keep = args.keep or tmp
        os.makedirs(keep, exist_ok=True)
        trees = {"new": (ROOT, device_cmds(ROOT)), "old": (old, device_cmds(old))}
        with concurrent.futures.ThreadPoolExecutor(max(1, args.j)) as pool:
            jobs = {(f, side): pool.submit(device_asm, tree, cmds, f, os.path.join(keep, f"{f[:-4]}.{side}.s"))
                    for f in files for side, (tree, cmds) in trees.items()}
            texts = {k: j.result() for k, j in jobs.items()}
    differ = False
    for f in files:
        # (the temporary directory's name appears in the text: the source path of the .file directive)
        new = texts[f, "new"].replace(ROOT, "<tree>")
        was = texts[f, "old"].replace(old, "<tree>")
        same = new == was
        differ |= not same
        print(f"{f}: {'identical' if same else 'DIFFERENT'} ({len(was.splitlines())} -> {len(new.splitlines())} lines)")
        sn, so = dict(sections(new)), dict(sections(was))
        names = [n for n, _ in sections(new)] + [n for n in so if n not in sn]
        for n, shown in zip(names, demangled(names)):
            what = "identical" if sn.get(n) == so.get(n) else "only in " + args.rev if n not in sn else "only in the working tree" if n not in so else "DIFFERENT"
            if not same or what != "identical":
                print(f"    {shown}: {what}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
