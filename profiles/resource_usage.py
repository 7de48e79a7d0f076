"""Regenerates profiles/products_resource_usage.log, profiles/hprod_resource_usage.log and profiles/diag_resources.md: registers,
scratch and occupancy of every matrix-free product and KKT-diagonal kernel of the registry, from the compiler's own remarks (no GPU
needed).

    python profiles/resource_usage.py [--jobs 8]

Each csrc/ctd_pkern_<problem>.hip is compiled for the device only with -Rpass-analysis=kernel-resource-usage.  Per problem the
whole-grid kernels come first, in the order the compiler reports them (trapeze, midpoint / Euler, Gauss-Legendre s = 1, 2, 3,
then the finish kernel), followed by the shard form of the same kernels marked "shard".  The comment lines at the head of each
log are kept.  The KKT diagonals (hdiag, jsq_cols, jsq_rows: the whole-grid form from csrc/ctd_dkern_<problem>.hip, the shard form
from csrc/ctd_dskern_<problem>.hip) go to a table in profiles/diag_resources.md, each shard row under its whole-grid twin; the text
above the table is kept.  The script fails if any kernel uses scratch.  --krylov: the vector kernels of the device-resident MINRES
solve (csrc/ctd_krylov.hip) to profiles/kkt_minres_resources.md, nothing else."""
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


def write_diag(table, shard_table):
    """per problem and scheme one row for the whole-grid form and one for the shard form: the three scheme-dependent kernels side by
    side; then the two finish kernels, both forms"""
    path = os.path.join(ROOT, "profiles", "diag_resources.md")
    with open(path) as f:
        text = f.read()
    head = text[:text.index("| problem |")] if "| problem |" in text else text
    cell = lambda k: f"{k['vgpr']} + {k['agpr']} | {k['scratch']} | {k['waves']}"      # noqa: E731
    lines = ["| problem | scheme | hdiag VGPR + AGPR | scratch B/lane | waves/SIMD | jsq_cols VGPR + AGPR | scratch B/lane | waves/SIMD "
             "| jsq_rows VGPR + AGPR | scratch B/lane | waves/SIMD |\n", "|---|---|---|---|---|---|---|---|---|---|---|\n"]
    for stem, name in HPROD:
        forms = []
        for tab, shard in ((table, False), (shard_table, True)):
            by = {kn: [k for k in tab[stem] if k["kernel"] == kn] for kn in DIAG_KERNELS}
            for k in tab[stem]:
                assert k["scratch"] == 0 and k["shard"] == shard, (name, k)
            assert all(len(by[kn]) == 5 for kn in ("hdiag_units_kernel", "jsq_cols_units_kernel", "jsq_rows_kernel")), name
            forms.append(by)
        for i, sch in enumerate(SCHEMES):
            for by, tag in zip(forms, ("", ", shard")):
                lines.append(f"| {name} | {sch}{tag} | {cell(by['hdiag_units_kernel'][i])} | {cell(by['jsq_cols_units_kernel'][i])} | "
                             f"{cell(by['jsq_rows_kernel'][i])} |\n")
        for by, tag in zip(forms, ("", ", shard")):
            lines.append(f"| {name} | finish{tag} | {cell(by['hdiag_finish_kernel'][0])} | {cell(by['jsq_cols_finish_kernel'][0])} | | | |\n")
    with open(path, "w") as f:
        f.write(head)
        f.writelines(lines)
    print(path, len(lines) - 2, "rows")


# ---- constraint / Jacobian kernel: the lean variant and its static-emit form (profiles/static_emit.md) --------------------------
# (file stem, OCP type, scheme class, stages, lanes the default rule launches) of bench/stamps.py's cfg2 / cfg3 / cfg4
CONS_JAC = (("cfg2", "goddard", "GoddardOCP", 2, 2, 320), ("cfg3", "double_integrator_path", "DoubleIntegratorPathOCP", 1, 1, 256),
            ("cfg4", "goddard", "GoddardOCP", 2, 3, 256))


def cons_jac_counts(stem):
    """{mangled kernel name: dict(resources..., code bytes, and the mnemonic-class counts of the section behind the tile's barrier)}
    Section: from the FIRST workgroup barrier of the function to the end of program or to the next pin of kernel arguments,
    whichever comes first -- the static-emit kernel places the tile's path first and the edge arm (which opens with a pin) behind
    it, so this is the tile's emit alone, ALL its store cases counted although a tile runs one of them; in the lean kernel the
    edge block's emit is inlined in the same run of code and is counted with it.  Classes: branch (s_branch / s_cbranch_*), scalar load (s_load_*), store (global_store_*)."""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", f"ctd_kern_{stem}.hip", "-o", "-"], cwd=CSRC, capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(r.stderr[-4000:])
    res, cur = {}, None
    pats = (("sgpr", r"TotalSGPRs: (\d+)"), ("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
            ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"))
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        if cur is not None:
            for key, pat in pats:
                m = re.search(pat, line)
                if m:
                    cur[key] = int(m.group(1))
    name, body = None, []
    for line in r.stdout.splitlines():
        m = re.match(r"^(_ZN3ctd\w*cons_jac\w*):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        m = re.search(r"; codeLenInByte = (\d+)", line)
        if m and name in res:
            ins = [l.split()[0] for l in body if l.startswith("\t") and (l.lstrip().startswith(";;#ASMSTART") or not l.lstrip().startswith((".", ";")))]
            b0 = next((i for i, x in enumerate(ins) if x == "s_barrier"), None)
            sec = []
            if b0 is not None:
                # (the pins of the kernel arguments are empty asm statements: the first one behind the tile's barrier opens the edge arm)
                e0 = next((i for i in range(b0, len(ins)) if ins[i] in ("s_endpgm", ";;#ASMSTART")), len(ins))
                sec = ins[b0 + 1:e0]
                if e0 < len(ins) and ins[e0] == ";;#ASMSTART":
                    # the edge arm opens with the scalar loads its pin names: the run of loads that ends within a few instructions
                    # of the pin belongs to it, not to the tile's emit
                    hi = max((i for i, x in enumerate(sec) if x.startswith("s_load")), default=-1)
                    lo, i, gap = hi, hi - 1, 0
                    while i >= 0 and gap <= 3:          # (the run may be broken by an instruction or two)
                        if sec[i].startswith("s_load"):
                            lo, gap = i, 0
                        else:
                            gap += 1
                        i -= 1
                    if hi >= 0 and len(sec) - hi <= 4:
                        sec = sec[:lo]
            ins = [x for x in ins if x != ";;#ASMSTART"]
            res[name].update(code_bytes=int(m.group(1)), instructions=len(ins), sec_instructions=len(sec),
                             sec_branches=sum(x.startswith(("s_branch", "s_cbranch")) for x in sec),
                             sec_scalar_loads=sum(x.startswith("s_load") for x in sec),
                             sec_stores=sum(x.startswith("global_store") for x in sec))
            name = None
            continue
        body.append(line)
    return res


def cons_jac_table():
    print("| workload | kernel | code bytes | instructions | behind the barrier: instructions | branches | scalar loads | stores "
          "| SGPRs | VGPRs | SGPR / VGPR spills | scratch | waves/SIMD |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    cache = {}
    for cfg, stem, ocp, sc, s, lanes in CONS_JAC:
        res = cache.setdefault(stem, cons_jac_counts(stem))
        tag = f"{len(ocp)}{ocp}ELi{sc}ELi{s}E"
        for label, suffix in (("lean", f"cons_jac_kernelINS_{tag}Lb0ELb1EEE"), (f"static, {lanes} lanes, write-through", f"cons_jac_static_kernelINS_{tag}Lb0ELi{lanes}ELb1EEE")):
            k = [v for n, v in res.items() if suffix in n]
            if not k:
                print(f"| {cfg} | {label} | not built |")
                continue
            k = k[0]
            assert k["scratch"] == 0, (cfg, label, k)
            print(f"| {cfg} | {label} | {k['code_bytes']} | {k['instructions']} | {k['sec_instructions']} | {k['sec_branches']} | {k['sec_scalar_loads']} "
                  f"| {k['sec_stores']} | {k['sgpr']} | {k['vgpr']} | {k['sgpr_spill']} / {k['vgpr_spill']} | {k['scratch']} | {k['waves']} |")


# ---- vector kernels of the device-resident MINRES solve (csrc/ctd_krylov.hip; profiles/kkt_minres_resources.md) -----------------
KRYLOV_KERNELS = ("krylov_init_kernel", "krylov_first_kernel", "krylov_alfa_kernel", "krylov_lanczos_kernel", "krylov_update_kernel",
                  # the shard form (csrc/ctd_krylov_shard_kernels.hpp)
                  "krylov_shard_init_kernel", "krylov_shard_first_kernel", "krylov_shard_alfa_kernel", "krylov_shard_lanczos_kernel",
                  "krylov_shard_update_kernel")


SCHUR_KERNELS = ("schur_assemble_kernel", "schur_factor_kernel", "schur_solve_kernel")
# the log-depth exact form (csrc/ctd_schur_cr.hip)
SCHUR_CR_KERNELS = ("schur_cr_assemble_kernel", "schur_cr_eliminate_kernel", "schur_cr_update_kernel", "schur_cr_down_kernel",
                    "schur_cr_root_kernel", "schur_cr_up_kernel", "schur_cr_dot_kernel",
                    # the joined form (csrc/ctd_schur_cr_joint_kernels.hpp; its translation unit is csrc/ctd_schur_cr_joint.hip)
                    "schur_cr_joint_interface_kernel", "schur_cr_joint_down_kernel", "schur_cr_joint_root_kernel", "schur_cr_joint_up_kernel",
                    "schur_cr_joint_contrib_kernel", "schur_cr_joint_reduce_kernel", "schur_cr_joint_record_kernel",
                    "schur_cr_joint_reduced_solve_kernel", "schur_cr_joint_correct_kernel")


def mangled(stem):
    """the mangled names of the kernels of csrc/<stem>.hip in the order of the compiler's remarks: the template arguments of an
    instantiation (remarks() keeps the kernel's plain name only)"""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", f"{stem}.hip", "-o", os.devnull], cwd=CSRC, capture_output=True, text=True)
    return re.findall(r"Function Name: (\S+)", r.stderr)


def krylov_table():
    ks = remarks("ctd_krylov", "", KRYLOV_KERNELS)
    names = [n for n in mangled("ctd_krylov") if re.search("|".join(KRYLOV_KERNELS), n)]
    assert len(names) == len(ks)
    for k, n in zip(ks, names):         # the SCHUR = true instantiation of a kernel (its only template argument); of a shard kernel:
        if re.search(r"ILb1EE", n) or "KrylovSchurShardParams" in n:      # the one for the Schur form's argument struct
            k["kernel"] += "<SCHUR>"
        if "KrylovSchurJointParams" in n:       # ... for the joined form's
            k["kernel"] += "<JOINT>"
    assert sorted({k["kernel"].replace("<SCHUR>", "").replace("<JOINT>", "") for k in ks}) == sorted(KRYLOV_KERNELS), ks
    for stem, kernels in (("ctd_schur", SCHUR_KERNELS), ("ctd_schur_cr", SCHUR_CR_KERNELS), ("ctd_schur_cr_joint", SCHUR_CR_KERNELS)):
        sch = remarks(stem, "", kernels)
        for k, n in zip(sch, [n for n in mangled(stem) if re.search("|".join(kernels), n)]):
            mb = re.search(r"ILi(\d+)E", n)
            k["kernel"] += f"<{mb.group(1)}>" if mb else ""
            if "SchurCrShard" in n:      # the instantiation for a shard's argument struct (csrc/ctd_schur_cr_kernels.hpp)
                k["kernel"] += " shard"
            if "SchurCrJoint" in n and "schur_cr_joint_" not in n:      # ... for the joined form's (csrc/ctd_schur_cr_joint_kernels.hpp)
                k["kernel"] += " joint"
        ks += sch
    path = os.path.join(ROOT, "profiles", "kkt_minres_resources.md")
    lines = ["# Resources of the MINRES vector kernels (csrc/ctd_krylov.hip)\n\n",
             "From the compiler's remarks for gfx950 (`python profiles/resource_usage.py --krylov`, no GPU needed).  The kernels do not\n"
             "depend on the OCP: one instantiation each, two (`<SCHUR>`: with the block-tridiagonal Schur preconditioner) of the four whose\n"
             "code differs with it (of the shard form: the four instantiated for the Schur form's argument struct, csrc/\n"
             "ctd_krylov_shard_kernels.hpp); below them the kernels of that preconditioner (csrc/ctd_schur.hip), the factor and the solve per\n"
             "largest block size, and those of its log-depth exact form (csrc/ctd_schur_cr.hip; `shard`: the instantiation for a\n"
             "shard's argument struct; `joint`: for the joined form's, followed by that form's own kernels).  The script fails if any of them uses\n"
             "scratch.\n\n",
             "| kernel | VGPR + AGPR | scratch B/lane | waves/SIMD |\n", "|---|---|---|---|\n"]
    # a kernel keeps the row it has in the file; new ones follow in the compiler's order (instantiating a kernel a second time
    # reorders the compiler's remarks, not the table)
    have = []
    if os.path.exists(path):
        with open(path) as f:
            have = [l.split("|")[1].strip() for l in f if l.startswith("| ") and not l.startswith("| kernel")]
    ks = [k for _, k in sorted(enumerate(ks), key=lambda ik: (have.index(ik[1]["kernel"]) if ik[1]["kernel"] in have else len(have), ik[0]))]
    for k in ks:
        assert k["scratch"] == 0, k
        lines.append(f"| {k['kernel']} | {k['vgpr']} + {k['agpr']} | {k['scratch']} | {k['waves']} |\n")
    with open(path, "w") as f:
        f.writelines(lines)
    print(path, len(ks), "kernels")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--krylov", action="store_true", help="write profiles/kkt_minres_resources.md (the MINRES vector kernels) and stop")
    ap.add_argument("--cons-jac", action="store_true", help="print the table of profiles/static_emit.md (lean and static-emit kernels of cfg2 / cfg3 / cfg4) and stop")
    args = ap.parse_args()
    if args.cons_jac:
        return cons_jac_table()
    if args.krylov:
        return krylov_table()
    stems = [s for s, _ in PRODUCTS]
    with ThreadPoolExecutor(args.jobs) as ex:
        table = dict(zip(stems, ex.map(remarks, stems)))
    write("products_resource_usage.log", PRODUCTS, table, False)
    write("hprod_resource_usage.log", HPROD, table, True)
    with ThreadPoolExecutor(args.jobs) as ex:
        dtable = dict(zip(stems, ex.map(lambda s: remarks(s, "ctd_dkern_", DIAG_KERNELS), stems)))
        stable = dict(zip(stems, ex.map(lambda s: remarks(s, "ctd_dskern_", DIAG_KERNELS), stems)))
    write_diag(dtable, stable)


if __name__ == "__main__":
    main()
