"""Regenerates profiles/kktprod_resources.md: registers, scratch and occupancy of every kktprod_units_kernel instantiation of the
registry -- whole grid and shard form -- beside the hprod_units_kernel of the same (problem, scheme), from the compiler's own
remarks (no GPU needed).

    python profiles/kktprod_resources.py [--jobs 8]

Each csrc/ctd_pkern_<problem>.hip is compiled for the device only with -Rpass-analysis=kernel-resource-usage.  The hprod kernels'
source is what it was before the fused product was added, and their figures are checked against profiles/hprod_resource_usage.log.
The script fails if a fused instantiation, of either form, uses scratch where the hprod instantiation uses none."""
import argparse
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ctdirect.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# (file stem, problem name), in the order of profiles/hprod_resource_usage.log
PROBLEMS = [("double_integrator_free_t0_tf", "double_integrator_freet0tf"), ("double_integrator_path", "double_integrator_path"),
            ("estimate_initial_condition", "estimate_initial_condition"), ("estimate_rotation_rate", "estimate_rotation_rate"),
            ("goddard", "goddard"), ("goddard_all", "goddard_all"), ("least_squares_constraint", "least_squares_with_constraint"),
            ("quadrotor", "quadrotor"), ("quadrotor12", "quadrotor12"), ("stagewise_scalar", "stagewise_scalar")]
SCHEMES = {(0, 1): "trapeze", (1, 1): "midpoint / Euler", (2, 1): "Gauss-Legendre 1", (2, 2): "Gauss-Legendre 2",
           (2, 3): "Gauss-Legendre 3"}
FIELDS = (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
          ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"))


def remarks(stem):
    """{(kernel, scheme class, stages): figures} of the unit kernels of one problem; the shard form of the fused kernel is
    "kktprod_shard", the shard form of hprod is left out"""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", f"ctd_pkern_{stem}.hip", "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(r.stderr[-4000:])
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            k = re.search(r"\d+(kktprod|hprod)_units_kernel", name)
            t = re.search(r"ELi(\d+)ELi(\d+)E", name)
            shard = bool(re.search(r"Lb1EE+v", name))
            kind = k.group(1) + ("_shard" if shard else "") if k else None
            cur = {"key": (kind, int(t.group(1)), int(t.group(2)))} if k and t and kind != "hprod_shard" else None
            continue
        if cur is None:
            continue
        for key, pat in FIELDS:
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
        if "LDS Size" in line:          # the last remark of a kernel
            out[cur.pop("key")] = cur
            cur = None
    return out


def committed_hprod():
    """the whole-grid hprod_units_kernel lines of profiles/hprod_resource_usage.log, per problem in instantiation order"""
    table = {}
    with open(os.path.join(ROOT, "profiles", "hprod_resource_usage.log")) as f:
        for line in f:
            m = re.match(r"(\S+) hprod_units_kernel vgpr=(\d+) agpr=(\d+) scratch=(\d+) waves=(\d+)", line)
            if m:
                table.setdefault(m.group(1), []).append(tuple(int(g) for g in m.groups()[1:]))
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    stems = [s for s, _ in PROBLEMS]
    with ThreadPoolExecutor(args.jobs) as ex:
        table = dict(zip(stems, ex.map(remarks, stems)))
    log = committed_hprod()
    fmt = lambda k: f"{k['vgpr']} + {k['agpr']} | {k['scratch']} | {k['waves']}"      # noqa: E731
    rows = []
    for stem, name in PROBLEMS:
        for i, (sc, s) in enumerate(sorted(SCHEMES)):
            h, k, ks = table[stem][("hprod", sc, s)], table[stem][("kktprod", sc, s)], table[stem][("kktprod_shard", sc, s)]
            assert (h["vgpr"], h["agpr"], h["scratch"], h["waves"]) == log[name][i], (name, sc, s, h, log[name][i])
            assert k["scratch"] == 0 or h["scratch"] > 0, (name, sc, s, k)
            assert ks["scratch"] == 0 or h["scratch"] > 0, (name, sc, s, "shard form", ks)
            rows.append(f"| {name} | {SCHEMES[(sc, s)]} | {fmt(k)} | {fmt(ks)} | {fmt(h)} |\n")
    path = os.path.join(ROOT, "profiles", "kktprod_resources.md")
    with open(path) as f:
        text = f.read()
    head = text[:text.index("| problem |")]
    with open(path, "w") as f:
        f.write(head)
        f.write("| problem | scheme | kktprod VGPR + AGPR | scratch B/lane | waves/SIMD | shard form VGPR + AGPR | scratch B/lane | "
                "waves/SIMD | hprod VGPR + AGPR | scratch B/lane | waves/SIMD |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
        f.writelines(rows)
    print(path, len(rows), "instantiations")


if __name__ == "__main__":
    main()
