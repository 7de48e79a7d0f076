"""CPU tests of the launch plan of the constraint / Jacobian kernel (plan_cons_jac, csrc/ctd_host.cpp), without a GPU.

The host-only plan: tests/golden/launch_plans.json holds launch_info() of 410 host-only handles as the commit before the
planner produced them (tests/golden/gen_launch_plans.py); the planner reproduces every line.

The two rules that ask the device for its resident workgroups run here through the emulator's entry to the same function
(emu.plan) with a constant answer R on 256 compute units, and must give what their comments in ctd_host.cpp state.
"""
import importlib.util
import json
import os

import pytest

import ctdirect_jl_amd as ct
from emu import emu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("gen_launch_plans", os.path.join(HERE, "golden", "gen_launch_plans.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

GODDARD = ct.PROBLEMS["goddard"]
GL2, GL3, MIDPOINT = ct.SCHEMES["gauss_legendre_2"], ct.SCHEMES["gauss_legendre_3"], ct.SCHEMES["midpoint"]


def test_host_only_plans_are_those_of_the_commit_before_the_planner():
    with open(gen.OUT) as f:
        golden = json.load(f)
    assert tuple(golden["fields"]) == gen.FIELDS
    cases = gen.cases()
    assert [c[:-1] for c in golden["cases"]] == cases          # the file holds the whole matrix, in the generator's order
    bad = [(c[:-1], c[-1], got) for c in golden["cases"] for got in [gen.plan(c[:-1])] if got != c[-1]]
    assert not bad, f"{len(bad)} of {len(cases)} plans differ; the first (case, golden, now): {bad[:3]}"


def test_emu_plan_without_a_device_is_the_host_only_handles_plan():
    """emu.plan and ctd_create reach the same function: the same answers, shards and pinned tiles included"""
    for prob, sch, N, steps, knobs in [("goddard", "gauss_legendre_2", 10_000, None, {}), ("quadrotor12", "midpoint", 1000, (500, 1000), {}),
                                       ("double_integrator_path", "trapeze", 100_000, None, {"tile": 7}),
                                       ("goddard", "gauss_legendre_3", 1000, None, {"block": 128})]:
        env = {"CTD_" + k.upper(): str(v) for k, v in knobs.items()}
        want = dict(zip(gen.FIELDS, gen.plan([prob, sch, N, "manual", "csc", 1, steps, env])))
        a, b = steps or (0, 0)
        got = emu.plan(ct.PROBLEMS[prob], ct.SCHEMES[sch], 0, N, step_begin=a, step_end=b, **knobs)
        assert (got["grid"], got["block"], got["lds_bytes"], got["tile"]) == \
               (want["grid"], want["block"], want["lds_bytes"], want["steps_per_tile"]), (prob, sch, N, got, want)
        assert got["grid"] == got["ntiles"] + got["has_edge"] and got["wg_stride"] == 0 and got["early"] == 0


def test_knobs_are_read_from_the_environment_once(monkeypatch):
    for k in gen.KNOBS:
        monkeypatch.delenv(k, raising=False)
    dflt = emu.plan_knobs()
    assert emu.plan_knobs(from_env=True) == dflt
    assert dflt == dict(tile=0, block=0, lean=1, static_emit=1, long_grid=1, long_grid_rounds=8, wt_store=-1, early=0, multi_tile=0, debug_stop=0)
    for i, name in enumerate(dflt):
        monkeypatch.setenv("CTD_" + name.upper(), str(100 + i))
    assert emu.plan_knobs(from_env=True) == {name: 100 + i for i, name in enumerate(dflt)}


def test_even_rounds_rule():
    """Goddard, Gauss-Legendre 3, N = 80 000, R = 4 resident workgroups per CU: the 32 steps of default_tile give 2500 tiles, more
    than the 1024 resident; with tiles of up to 48 steps that is 2 rounds, and the steps spread evenly over 2 x 1024 tiles:
    ceil(80 000 / 2048) = 40 steps, 2000 tiles and the edge blocks -- the "40 steps" of the rule's comment"""
    host = emu.plan(GODDARD, GL3, 0, 80_000)
    assert host["tile"] == 32 and host["ntiles"] == 2500 and host["block"] == 256
    p = emu.plan(GODDARD, GL3, 0, 80_000, resident=4)
    assert p["tile"] == -(-80_000 // 2048) == 40 and p["ntiles"] == 2000 and p["grid"] == 2000 + p["has_edge"] and p["block"] == 256
    # only ever a larger tile, and only when the tiles do not fit one round: R = 10 holds all 2500
    assert emu.plan(GODDARD, GL3, 0, 80_000, resident=10) == host
    # not for the schemes with one point per step
    assert emu.plan(GODDARD, MIDPOINT, 0, 80_000, resident=1) == emu.plan(GODDARD, MIDPOINT, 0, 80_000)


@pytest.mark.parametrize("sch,kib,N", [(GL3, 64, 1 << 17), (MIDPOINT, 74, 1 << 19)])
def test_long_grid_rule(sch, kib, N):
    """long_grid_rounds = 1, R = 4, 2^17 steps (the midpoint scheme: 2^19, its 64-step tiles of 2^17 fit one round): 512 lanes and
    the largest tile whose records fit 64 KiB of LDS (the midpoint scheme: 74 KiB) -- the bound recomputed here from the plans of
    the pinned tiles next to it"""
    host = emu.plan(GODDARD, sch, 0, N)
    p = emu.plan(GODDARD, sch, 0, N, resident=4, long_grid_rounds=1)
    assert p["block"] == 512 and p["tile"] > host["tile"] and p["grid"] == -(-N // p["tile"]) + p["has_edge"]
    lds = lambda t: emu.plan(GODDARD, sch, 0, N, tile=t, block=512)  # noqa: E731  (a pinned tile above 80 KiB would be halved: not near here)
    assert lds(p["tile"])["tile"] == p["tile"] and lds(p["tile"] + 1)["tile"] == p["tile"] + 1
    assert lds(p["tile"] - 1)["lds_bytes"] < lds(p["tile"])["lds_bytes"] == p["lds_bytes"] <= kib * 1024 < lds(p["tile"] + 1)["lds_bytes"]
    # the default threshold is 8 rounds of 256 R tiles: 2^17 steps in 32-step tiles are 4096 = 4 rounds of R = 4, and 8 of R = 2
    M = 1 << 17
    assert emu.plan(GODDARD, GL2, 0, M)["ntiles"] == 4096
    assert emu.plan(GODDARD, GL2, 0, M, resident=4)["block"] == 256
    assert emu.plan(GODDARD, GL2, 0, M, resident=2)["block"] == 512
    assert emu.plan(GODDARD, GL2, 0, M, resident=2, long_grid=0)["block"] == 256


@pytest.mark.parametrize("N,knobs", [(80_000, {}), (1 << 17, {"long_grid_rounds": 1})])
def test_pinned_tile_pinned_block_and_failed_query(N, knobs):
    """A failed query (R = 0) and a pinned tile switch both device rules off; a pinned block switches the long-grid rule off -- which
    would set its own -- and leaves the even-rounds rule, which keeps the block, as it was before the planner"""
    host = emu.plan(GODDARD, GL3, 0, N, **knobs)
    assert emu.plan(GODDARD, GL3, 0, N, resident=4, **knobs) != host
    assert emu.plan(GODDARD, GL3, 0, N, resident=0, **knobs) == host          # R = 0: the query failed
    t, b = host["tile"], host["block"]
    assert emu.plan(GODDARD, GL3, 0, N, resident=4, tile=t, **knobs) == emu.plan(GODDARD, GL3, 0, N, tile=t, **knobs) == host
    pinned_block = emu.plan(GODDARD, GL3, 0, N, resident=4, block=b, **knobs)
    if knobs:
        assert pinned_block["block"] == b and host["tile"] <= pinned_block["tile"] <= 48
    else:
        assert pinned_block == emu.plan(GODDARD, GL3, 0, N, resident=4)


def test_write_through_threshold():
    """wt_store flips exactly where the outputs of one evaluation cross 64 MB; CTD_WT_STORE overrides it either way"""
    a, b = (ct.DOCP("goddard", N, "gauss_legendre_2", device=-1) for N in (100, 101))
    per_step = 8 * (b.dim_NLP_constraints - a.dim_NLP_constraints + b.nnzj - a.nnzj)      # bytes of c and of Jacobian values of one more step
    n_last = 64_000_000 // per_step          # the last grid whose 8 N (cb + Lseg) bytes are <= 64 MB
    assert n_last * per_step <= 64_000_000 < (n_last + 1) * per_step
    assert emu.plan(GODDARD, GL2, 0, n_last)["wt_store"] == 1
    assert emu.plan(GODDARD, GL2, 0, n_last + 1)["wt_store"] == 0
    assert emu.plan(GODDARD, GL2, 0, n_last, wt_store=0)["wt_store"] == 0
    assert emu.plan(GODDARD, GL2, 0, n_last + 1, wt_store=1)["wt_store"] == 1
    assert emu.plan(GODDARD, GL2, 0, 100)["wt_store"] == 1 and emu.plan(GODDARD, GL2, 0, 100, wt_store=0)["wt_store"] == 0
