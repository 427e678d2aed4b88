#!/usr/bin/env python3
"""Per-kernel device-code comparison of two source trees, as a markdown table (no GPU needed).

    python tools/device_code_diff.py PARENT_TREE NEW_TREE compress_split.hip encoder_bwd_split.hip ...

Each named file of ``csrc/`` that exists in a tree is compiled for the device only, to assembly, with
the build's flags (``build.FLAGS`` and the per-file extras).  Kernels are matched by demangled name
across all the files, so one that moved to another unit is compared with itself.  Per kernel:

* the VGPR / AGPR / SGPR / scratch / LDS figures of the code object's metadata, parent / new;
* ``body``: the whole instruction sequence with register numbers and labels stripped;
* ``k-loop``: the same for the innermost backward-branch loop(s) that hold the MFMAs (``-``: none);
* where the body differs: whether the instructions outside those loops are the same multiset of
  opcodes, and at how many positions the two sequences differ.

The tool looks for nothing in the assembly but the kernels' boundaries, those metadata fields and the
loops around the MFMAs.  Exit status 0 whatever the table says: it reports, the reader judges.
"""
from __future__ import annotations

import argparse
import collections
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pkg(tree: str) -> str:
    for d in sorted(os.listdir(tree)):
        if os.path.isfile(os.path.join(tree, d, "build.py")) and os.path.isdir(os.path.join(tree, d, "csrc")):
            return os.path.join(tree, d)
    raise SystemExit(f"{tree}: no package with build.py and csrc/")


def _build_module():
    spec = importlib.util.spec_from_file_location("_mrp_build", os.path.join(_pkg(REPO), "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assembly(tree: str, name: str, build, tmp: str, tag: str) -> str | None:
    src = os.path.join(_pkg(tree), "csrc", name)
    if not os.path.exists(src):
        return None
    out = os.path.join(tmp, f"{tag}_{name}.s")
    cmd = [build.hipcc(), f"--offload-arch={build.ARCH}"] + build.FLAGS + build.EXTRA_FLAGS.get(name, []) + [
        "-I", os.path.join(tree, "include"), "--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True)
    with open(out) as f:
        return f.read()


def demangle(names: list[str]) -> dict[str, str]:
    filt = next((c for c in (os.path.join(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "")), "llvm-cxxfilt"),
                             "/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt"))
                 if c and os.path.exists(c)), None)
    if filt is None or not names:
        return {n: n for n in names}
    out = subprocess.run([filt] + names, check=True, capture_output=True, text=True).stdout.split("\n")
    # "void ns::kernel<3>(ns::Args)" -> "ns::kernel<3>"
    clean = [re.sub(r"^void ", "", re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", o.strip())) for o in out]
    return dict(zip(names, clean))


_REG = re.compile(r"\b([vsa])(?:\d+|\[\d+:\d+\])")
_LABEL = re.compile(r"\.LBB\d+_\d+")
_META = {"vgpr": ".vgpr_count", "agpr": ".agpr_count", "sgpr": ".sgpr_count",
         "scratch": ".private_segment_fixed_size", "lds": ".group_segment_fixed_size"}


class Kernel:
    def __init__(self, file: str):
        self.file = file
        self.instrs: list[str] = []   # normalised
        self.labels: dict[str, int] = {}  # label -> index of the next instruction
        self.branches: list[tuple[int, str]] = []
        self.meta: dict[str, str] = {}

    def loops(self) -> list[tuple[int, int]]:
        """[first, last] instruction ranges of the innermost backward-branch loops that hold MFMAs"""
        cand = []
        for at, label in self.branches:
            first = self.labels.get(label)
            if first is not None and first <= at and any("v_mfma" in i for i in self.instrs[first:at + 1]):
                cand.append((first, at))
        return sorted(c for c in cand if not any(o != c and c[0] <= o[0] and o[1] <= c[1] for o in cand))

    def loop_code(self) -> list[list[str]]:
        return [self.instrs[a:b + 1] for a, b in self.loops()]

    def outside(self) -> list[str]:
        inside = set()
        for a, b in self.loops():
            inside.update(range(a, b + 1))
        return [x for i, x in enumerate(self.instrs) if i not in inside]


def parse(asm: str, file: str) -> dict[str, Kernel]:
    """mangled kernel name -> Kernel"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    kernels: dict[str, Kernel] = {}
    cur: Kernel | None = None
    for line in asm.split("\n"):
        text = line.split(";")[0].strip()
        if not text:
            continue
        m = re.match(r"^([\w.$]+):$", text)
        if m:
            if m.group(1) in names:
                cur = kernels[m.group(1)] = Kernel(file)
            elif cur is not None and m.group(1).startswith(".LBB"):
                cur.labels[m.group(1)] = len(cur.instrs)
            elif m.group(1).startswith(".Lfunc_end"):
                cur = None
            continue
        if cur is None or text.startswith("."):
            continue
        tgt = _LABEL.search(text)
        if tgt and text.startswith(("s_cbranch", "s_branch")):
            cur.branches.append((len(cur.instrs), tgt.group(0)))
        cur.instrs.append(_LABEL.sub("L", _REG.sub(r"\1", text)))
    # the code object's metadata: one block per kernel, `.name:` among its fields
    for block in re.split(r"^\s*- \.agpr_count:", asm, flags=re.M)[1:]:
        block = ".agpr_count:" + block
        nm = re.search(r"^\s*\.name:\s+(\S+)", block, re.M)
        if nm and nm.group(1) in kernels:
            for key, field in _META.items():
                v = re.search(r"^\s*" + re.escape(field) + r":\s+(\S+)", block, re.M)
                kernels[nm.group(1)].meta[key] = v.group(1) if v else "?"
    return kernels


def positions(a: list[str], b: list[str]) -> int:
    return sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))


def row(name: str, p: Kernel | None, n: Kernel | None) -> str:
    if p is None or n is None:
        return f"| {name} | only {'new' if p is None else 'parent'} |"
    figs = " | ".join(f"{p.meta.get(k, '?')}/{n.meta.get(k, '?')}" for k in _META)
    body = "identical" if p.instrs == n.instrs else f"differs ({len(p.instrs)} vs {len(n.instrs)})"
    pl, nl = p.loop_code(), n.loop_code()
    if not pl and not nl:
        loop = "-"
    else:
        sizes = "+".join(str(len(x)) for x in nl)
        loop = f"identical ({sizes})" if pl == nl else f"differs ({'+'.join(str(len(x)) for x in pl)} vs {sizes})"
    if p.instrs == n.instrs:
        outside = "-"
    else:
        po, no = p.outside(), n.outside()
        delta = collections.Counter(i.split()[0] for i in no)
        delta.subtract(collections.Counter(i.split()[0] for i in po))
        other = ", ".join(f"{op} {d:+d}" for op, d in sorted(delta.items()) if d)
        counts = f"other opcode counts ({other})" if other else "same opcode counts"
        outside = f"{counts}, {positions(po, no)} of {len(no)} positions differ"
    moved = "" if p.file == n.file else f" (from {p.file})"
    return f"| {name}{moved} | {figs} | {body} | {loop} | {outside} |"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_tree")
    ap.add_argument("new_tree")
    ap.add_argument("files", nargs="+", help=".hip file names under csrc/ (one missing from a tree is skipped there)")
    args = ap.parse_args()
    build = _build_module()
    old: dict[str, Kernel] = {}
    new: dict[str, Kernel] = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in args.files:
            for tree, tag, into in ((args.parent_tree, "p", old), (args.new_tree, "n", new)):
                asm = assembly(tree, name, build, tmp, tag)
                if asm is not None:
                    into.update(parse(asm, name))
    names = demangle(sorted(set(old) | set(new)))
    head = ("| kernel | VGPR p/n | AGPR p/n | SGPR p/n | scratch p/n | LDS p/n | body | k-loop (instrs) | outside the k-loop |\n"
            "|---|---|---|---|---|---|---|---|---|")
    for name in args.files:
        mine = sorted(m for m in set(old) | set(new) if (new[m].file if m in new else old[m].file) == name)
        if not mine:
            continue
        print(f"## {name}\n{head}")
        for m in sorted(mine, key=lambda m: names[m]):
            print(row(names[m], old.get(m), new.get(m)))
        print()
    return 0


if __name__ == "__main__":
    sys.exit(main())
