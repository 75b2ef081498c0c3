#!/usr/bin/env python3
"""Is the gfx950 device code of two source trees the same text?

    python scripts/isa_same.py PARENT_TREE [THIS_TREE] [--keep DIR] [-D MACRO ...] [--sources all|A.hip,B.hip]

Compiles each listed HIP source of both trees to device assembly with the
build's own flags (build.HIP_FLAGS) plus ``--cuda-device-only -S``, drops the
lines that name the ``__hip_cuid_<hash>`` symbol (the hash covers the source
text, so it moves with every edit, comments included) and compares what is left
line for line.  Prints ``same`` or ``differs`` per file; exits 1 on a difference.

It compares text and nothing else: no resource summary, no disassembly of an
object.  A refactor that claims to leave the kernels alone can be held to this
on a machine without a GPU.  PARENT_TREE is a checkout of the commit to compare
against (``git worktree add`` or ``git archive | tar -x``).  tgms_reduced.hip
takes about 2.5 minutes per compile on one core.
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from trajectory_generator_ros2_amd import build as B  # noqa: E402

SOURCES = ["tgms_reduced.hip", "tgms_dense.hip", "tgms_sample.hip", "tgms_band.hip"]
CSRC_REL = os.path.relpath(B.CSRC, B.ROOT)
INCLUDE_REL = os.path.relpath(B.INCLUDE, B.ROOT)


def flags(tree):
    """build.HIP_FLAGS with the two -I paths pointed at `tree`."""
    out = [f for f in B.HIP_FLAGS if not f.startswith("-I")]
    return out + ["-I" + os.path.join(tree, INCLUDE_REL), "-I" + os.path.join(tree, CSRC_REL)]


def device_asm(tree, src, out, defines):
    cmd = [B.HIPCC] + flags(tree) + defines + ["--cuda-device-only", "-S", os.path.join(tree, CSRC_REL, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("compile failed: " + " ".join(cmd))
    with open(out) as f:
        return [ln for ln in f if "__hip_cuid_" not in ln]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent", help="tree of the commit to compare against")
    ap.add_argument("tree", nargs="?", default=ROOT, help="tree under test (default: this one)")
    ap.add_argument("--keep", metavar="DIR", help="keep the assembly files here (default: a temporary folder)")
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="MACRO", help="extra -D for both sides")
    ap.add_argument("--sources", metavar="A.hip,B.hip", help="the files to compare (default: the four solve kernels' files; "
                    "'all': every HIP source of the parent tree's build)")
    a = ap.parse_args()
    global SOURCES
    if a.sources == "all":
        SOURCES = sorted(f for f in os.listdir(os.path.join(os.path.abspath(a.parent), CSRC_REL)) if f.endswith(".hip"))
    elif a.sources:
        SOURCES = a.sources.split(",")
    defines = ["-D" + d for d in a.defines]
    tmp = None if a.keep else tempfile.TemporaryDirectory()
    keep = a.keep or tmp.name
    os.makedirs(keep, exist_ok=True)
    sides = (("parent", os.path.abspath(a.parent)), ("tree", os.path.abspath(a.tree)))
    with ThreadPoolExecutor(max_workers=min(16, 2 * len(SOURCES), os.cpu_count() or 1)) as ex:
        jobs = {(s, side): ex.submit(device_asm, t, s, os.path.join(keep, side + "_" + s + ".s"), defines)
                for s in SOURCES for side, t in sides}
        bad = 0
        for s in SOURCES:
            p, t = jobs[(s, "parent")].result(), jobs[(s, "tree")].result()
            same = p == t
            bad += not same
            print(f"{s}: {'same' if same else 'differs'}  ({len(p)} lines parent, {len(t)} lines tree, "
                  f"{sum(1 for ln in t if '.amdhsa_kernel ' in ln)} kernels)", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
