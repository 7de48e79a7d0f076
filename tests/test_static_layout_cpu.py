"""The static layout of the kernel instantiations against the layout the model builder produces (CPU only).

The lean variant of the constraint / Jacobian kernel reads the block sizes, the counts and the Butcher tables of its registry
instantiation <problem, scheme class, stages> as compile-time constants (StaticLayout, csrc/ctd_kernel_body.hpp).  `ctd_create`
compares them with the `Layout` built for the handle -- on every handle, host-only ones included -- and refuses a mismatch with
CTD_EINVAL and the name of the field.  So: every registry problem x every scheme x the control_steps the scheme accepts gives a
host-only handle without error, and its sizes are the reference's.
"""
import pytest

import ctdirect_jl_amd as ct

PAIRS = [(p, s) for p in ct.PROBLEMS for s in ct.SCHEMES]


@pytest.mark.parametrize("prob,sch", PAIRS, ids=[f"{p}-{s}" for p, s in PAIRS])
def test_static_layout_agrees_with_built_layout(prob, sch):
    made = 0
    for cs in (1, 2, 3):
        try:
            d = ct.DOCP(prob, 7, sch, device=-1, control_steps=cs)
        except ct.CTDirectError as e:
            # control_steps > 1 is offered with the midpoint scheme only (CTD_ESCHEME); never the layout check's refusal
            assert cs > 1 and sch != "midpoint" and e.status == 3, (cs, str(e))
            assert "static layout" not in str(e)
            continue
        made += 1
        n, m, nv = d.dims.NLP_x, d.dims.NLP_u, d.dims.NLP_v
        disc = d.discretization
        s = disc.stage
        stagewise = sch in ("gauss_legendre_2", "gauss_legendre_3")
        cu = m * cs if sch == "midpoint" else (m * s if stagewise else m)
        assert disc._step_variables_block == n + cu + n * s
        assert disc._state_stage_eqs_block == n * (1 + s)
        assert d.dim_NLP_variables == 7 * disc._step_variables_block + n + nv + (m if sch == "trapeze" else 0)
        d.close()
    assert made == (3 if sch == "midpoint" else 1)
