"""Do the kernels a revision already had still compile to the instructions they had?

    python profiles/same_instructions.py [--rev HEAD~1] [--stems ctd_schur_cr,ctd_krylov]

For every stem, csrc/<stem>.hip of the working tree and of --rev (with the headers of that revision, taken with `git show` into a
scratch directory) are compiled for gfx950 to assembly (device side only, the flags of csrc/Makefile; no GPU needed).  Per kernel
symbol of the revision the instruction lines are compared -- comments, directives and the numbering of local labels left out.  Prints
one line per stem and exits 1 if a kernel of the revision is missing or differs.  New kernels are not compared: a new argument
struct gives a new symbol."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ctdirect.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S"]


def kernels(asm):
    out, cur = {}, None
    for line in open(asm):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and not line.strip().startswith((";", ".")):
            out[cur].append(re.sub(r"\.LBB\d+_\d+", "L", line.split(";")[0].strip()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default="HEAD~1")
    ap.add_argument("--stems", default="ctd_schur_cr,ctd_krylov")
    args = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "csrc")
        os.makedirs(old)
        names = subprocess.check_output(["git", "ls-tree", "--name-only", args.rev, "ctdirect.jl_amd/csrc/"], cwd=ROOT, text=True).split()
        for n in names:
            if n.endswith((".hpp", ".hip")):
                with open(os.path.join(old, os.path.basename(n)), "wb") as f:
                    f.write(subprocess.check_output(["git", "show", f"{args.rev}:{n}"], cwd=ROOT))
        for stem in args.stems.split(","):
            a, b = os.path.join(tmp, stem + ".old.s"), os.path.join(tmp, stem + ".new.s")
            subprocess.run([HIPCC] + FLAGS + [stem + ".hip", "-o", a], cwd=old, check=True, capture_output=True)
            subprocess.run([HIPCC] + FLAGS + [stem + ".hip", "-o", b], cwd=CSRC, check=True, capture_output=True)
            ka, kb = kernels(a), kernels(b)
            diff = [k for k in ka if ka[k] != kb.get(k)]
            bad += len(diff)
            print(f"{stem}: {len(ka)} kernels at {args.rev}, {len(kb)} now, {len(ka) - len(diff)} with the same instructions" +
                  ("".join("\n  differs: " + k for k in diff)))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
