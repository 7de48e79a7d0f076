"""Regenerates profiles/products_resource_usage.log, profiles/hprod_resource_usage.log and profiles/diag_resources.md: registers,
scratch and occupancy of every matrix-free product and KKT-diagonal kernel of the registry, from the compiler's own remarks (no GPU
needed).

    python profiles/resource_usage.py [--jobs 8]

Each csrc/ctd_pkern_<problem>.hip is compiled for the device only with -Rpass-analysis=kernel-resource-usage.  Per problem the
whole-grid kernels come first, in the order the compiler reports them (trapeze, midpoint / Euler, Gauss-Legendre s = 1, 2, 3,
then the finish kernel), followed by the shard form of the same kernels marked "shard".  The comment lines at the head of each
log are kept.  The KKT diagonals (csrc/ctd_dkern_<problem>.hip: hdiag, jsq_cols, jsq_rows; whole-grid form only) go to a table in
profiles/diag_resources.md, whose text above the table is kept.  The script fails if any kernel uses scratch."""
import argparse
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ctdirect.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("jprod_kernel", "jtprod_units_kernel", "jtprod_finish_kernel", "hprod_units_kernel", "hprod_finish_kernel")
# (file stem, name in the log): the products log names a problem by its source file, the hprod log by its problem name
PRODUCTS = [(p, p) for p in ("quadrotor", "quadrotor12", "goddard_all", "double_integrator_free_t0_tf", "goddard",
                             "double_integrator_path", "estimate_initial_condition", "estimate_rotation_rate",
                             "least_squares_constraint", "stagewise_scalar")]
HPROD = [("double_integrator_free_t0_tf", "double_integrator_freet0tf"), ("double_integrator_path", "double_integrator_path"),
         ("estimate_initial_condition", "estimate_initial_condition"), ("estimate_rotation_rate", "estimate_rotation_rate"),
         ("goddard", "goddard"), ("goddard_all", "goddard_all"), ("least_squares_constraint", "least_squares_with_constraint"),
         ("quadrotor", "quadrotor"), ("quadrotor12", "quadrotor12"), ("stagewise_scalar", "stagewise_scalar")]
DIAG_KERNELS = ("hdiag_units_kernel", "hdiag_finish_kernel", "jsq_cols_units_kernel", "jsq_cols_finish_kernel", "jsq_rows_kernel")
SCHEMES = ("trapeze", "midpoint / Euler", "Gauss-Legendre 1", "Gauss-Legendre 2", "Gauss-Legendre 3")
FIELDS = (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
          ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"))


def remarks(stem, prefix="ctd_pkern_", kernels=KERNELS):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", f"{prefix}{stem}.hip", "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(r.stderr[-4000:])
    out, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search("|".join(kernels), m.group(1))
            # the shard form is the instantiation whose LAST template argument is `true`: in the mangled name the argument
            # list and the nested name close (E, E) right behind it and the return type (v) follows, so a bool flag added
            # before SH does not match
            cur = {"kernel": k.group(0), "shard": bool(re.search(r"Lb1EE+v", m.group(1)))} if k else None
            continue
        if cur is None:
            continue
        for key, pat in FIELDS:
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
        if "LDS Size" in line:          # the last remark of a kernel
            out.append(cur)
            cur = None
    return out


def write(log, problems, table, hprod):
    path = os.path.join(ROOT, "profiles", log)
    with open(path) as f:
        head = [l for l in f if l.startswith("#")]
    lines = []
    for stem, name in problems:
        ks = [k for k in table[stem] if k["kernel"].startswith("hprod") == hprod]
        for k in sorted(ks, key=lambda k: k["shard"]):          # (stable: the compiler's order inside each form)
            assert k["scratch"] == 0, (name, k)
            ag = f" agpr={k['agpr']}" if hprod else ""
            lines.append(f"{name} {k['kernel']}{' shard' if k['shard'] else ''} vgpr={k['vgpr']}{ag} scratch=0 waves={k['waves']}\n")
    with open(path, "w") as f:
        f.writelines(head + lines)
    print(path, len(lines), "kernels")


def write_diag(table):
    """one row per problem and scheme: the three scheme-dependent kernels side by side, then the two finish kernels"""
    path = os.path.join(ROOT, "profiles", "diag_resources.md")
    with open(path) as f:
        text = f.read()
    head = text[:text.index("| problem |")] if "| problem |" in text else text
    cell = lambda k: f"{k['vgpr']} + {k['agpr']} | {k['scratch']} | {k['waves']}"      # noqa: E731
    lines = ["| problem | scheme | hdiag VGPR + AGPR | scratch B/lane | waves/SIMD | jsq_cols VGPR + AGPR | scratch B/lane | waves/SIMD "
             "| jsq_rows VGPR + AGPR | scratch B/lane | waves/SIMD |\n", "|---|---|---|---|---|---|---|---|---|---|---|\n"]
    for stem, name in HPROD:
        by = {kn: [k for k in table[stem] if k["kernel"] == kn] for kn in DIAG_KERNELS}
        for k in table[stem]:
            assert k["scratch"] == 0, (name, k)
        assert all(len(by[kn]) == 5 for kn in ("hdiag_units_kernel", "jsq_cols_units_kernel", "jsq_rows_kernel")), name
        for i, sch in enumerate(SCHEMES):
            lines.append(f"| {name} | {sch} | {cell(by['hdiag_units_kernel'][i])} | {cell(by['jsq_cols_units_kernel'][i])} | "
                         f"{cell(by['jsq_rows_kernel'][i])} |\n")
        lines.append(f"| {name} | finish | {cell(by['hdiag_finish_kernel'][0])} | {cell(by['jsq_cols_finish_kernel'][0])} | | | |\n")
    with open(path, "w") as f:
        f.write(head)
        f.writelines(lines)
    print(path, len(lines) - 2, "rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    stems = [s for s, _ in PRODUCTS]
    with ThreadPoolExecutor(args.jobs) as ex:
        table = dict(zip(stems, ex.map(remarks, stems)))
    write("products_resource_usage.log", PRODUCTS, table, False)
    write("hprod_resource_usage.log", HPROD, table, True)
    with ThreadPoolExecutor(args.jobs) as ex:
        dtable = dict(zip(stems, ex.map(lambda s: remarks(s, "ctd_dkern_", DIAG_KERNELS), stems)))
    write_diag(dtable)


if __name__ == "__main__":
    main()
