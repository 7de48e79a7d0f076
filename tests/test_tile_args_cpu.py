"""make_tile_args (csrc/ctd_layout.hpp) against the KParams of the launch plan, on the CPU.

tests/tile_args_main.cpp is a stand-alone program (its own main, host sources only) built here with g++ and
-fsanitize=address,undefined and run directly: for Goddard on Gauss-Legendre 1 / 2 / 3 and the double integrator with free t0 and
tf on Gauss-Legendre 2, uniform and user grids, the grids of tests/test_gpu_static_tile_args.py, it builds the host-only model and
its plan, fills TileArgs and checks every field, the size (<= 192 bytes), the alignment (64), and that `valid` is cleared by
everything a static tile cannot run.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "tile_args_main.cpp")


def test_make_tile_args_against_the_plan(tmp_path):
    exe = str(tmp_path / "tile_args_main")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-o", exe, SRC, "-ldl"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("CTD_")}
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().startswith("ok: 34 cases"), r.stdout
