#!/usr/bin/env python3
"""Are the kernels of two source trees the same instructions?  The check behind the sharing rule of DESIGN section 23.

usage: python tools/kernel_asm_diff.py <tree A> <tree B>        (needs hipcc, no GPU)

Every ``.hip`` file of ``build.SOURCES`` is compiled in both trees with the flags of ``makani_amd/build.py`` plus
``--cuda-device-only -S``.  Of the assembly only the functions are kept, without assembler directives, comment lines and
lines that name the ``__hip_cuid_*`` symbol, and the two trees are compared function by function as text.  Prints every
function that differs (or that only one tree has) with the number of differing lines, then one summary line; the exit
status is 1 if anything differs.  To compare with a commit, export it first:

    git worktree add /tmp/parent HEAD~1 && python tools/kernel_asm_diff.py /tmp/parent .
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from makani_amd import build  # noqa: E402

JOBS = 16


def assembly(tree, src, out):
    path = os.path.join(tree, "makani_amd", "csrc", src)
    if not os.path.exists(path):
        return None
    cmd = [build._hipcc()] + build.compile_flags() + ["--cuda-device-only", "-S", path, "-o", out]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed on {path}:\n{res.stdout}")
    with open(out) as f:
        return f.read()


def functions(asm):
    """name -> the lines of the function's body that are neither directives nor comments."""
    names = set(re.findall(r"^\s*\.type\s+([^\s,]+),@function", asm, flags=re.M))
    out, cur = {}, None
    for line in asm.splitlines():
        text = line.strip()
        label = re.match(r"([^\s:]+):", line)
        if label and label.group(1) in names:
            cur = out.setdefault(label.group(1), [])
        elif text.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and text and not text.startswith(";") and "__hip_cuid_" not in text \
                and not (text.startswith(".") and not text.endswith(":")):      # a directive; local labels stay
            cur.append(text)
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    trees = [os.path.abspath(t) for t in sys.argv[1:]]
    sources = [s for s in build.SOURCES if s.endswith(".hip")]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(JOBS) as pool:
        jobs = {(i, s): pool.submit(assembly, t, s, os.path.join(tmp, f"{i}_{s}.s")) for i, t in enumerate(trees) for s in sources}
        asm = {k: j.result() for k, j in jobs.items()}
    total = lines = differing = 0
    for s in sources:
        if asm[0, s] is None or asm[1, s] is None:
            print(f"{s}: missing in {trees[0] if asm[0, s] is None else trees[1]}")
            differing += 1
            continue
        a, b = functions(asm[0, s]), functions(asm[1, s])
        for name in sorted(set(a) | set(b)):
            total += 1
            lines += len(b.get(name, ()))
            if a.get(name) != b.get(name):
                differing += 1
                delta = list(difflib.unified_diff(a.get(name, []), b.get(name, []), n=0, lineterm=""))[2:]
                n = sum(1 for d in delta if d[0] in "+-")
                only = "" if name in a and name in b else f" (only in {trees[0] if name in a else trees[1]})"
                print(f"{s}: {name}: {n} differing lines{only}")
    print(f"{len(sources)} .hip files, {total} kernels, {lines} lines compared: {differing} kernels differ")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
