"""CPU test of the argument handling that the 14 matrix-free methods of DOCP share (jprod, jtprod, hprod, kktprod, hdiag, jsq_rows,
jsq_cols and their *_shard forms), on host-only handles: every vector argument of wrong length raises the ValueError that names
it, a required argument left None raises, the shard forms refuse a NumPy array in any position with a TypeError, and CPU tensors of
the right lengths pass every check up to the refusal of a tensor that is not on the handle's GPU.  The values are checked on the
GPU in tests/test_gpu_products*.py, test_gpu_hprod.py, test_gpu_kktprod*.py and test_gpu_diag*.py."""
import re

import numpy as np
import pytest
import torch

import ctdirect_jl_amd as ct

# operator -> (vector arguments in call order: (name, layout, required), outputs: (name, layout)); "v": nvar, "c": ncon entries.  x is
# the first argument of every method, the arguments after it are passed by keyword, `out` as the output or the pair of them
OPS = {
    "jprod": ((("v", "v", True),), (("out", "c"),)),
    "jtprod": ((("w", "c", True),), (("out", "v"),)),
    "hprod": ((("y", "c", False), ("v", "v", True)), (("out", "v"),)),
    "kktprod": ((("y", "c", False), ("dx", "v", True), ("dy", "c", True), ("sx", "v", False), ("sc", "c", False)),
                (("out[0]", "v"), ("out[1]", "c"))),
    "hdiag": ((("y", "c", False),), (("out", "v"),)),
    "jsq_rows": ((("wx", "v", False),), (("out", "c"),)),
    "jsq_cols": ((("wc", "c", False),), (("out", "v"),)),
}
METHODS = [(op, shard) for op in OPS for shard in (False, True)]


@pytest.fixture(scope="module")
def handles():
    return {False: ct.DOCP("goddard", 10, "midpoint", device=-1), True: ct.DOCP("goddard", 10, "midpoint", device=-1, steps=(3, 7))}


def _call(d, op, shard, args):
    """args: name -> array of every vector argument and output"""
    ins, outs = OPS[op]
    out = tuple(args[name] for name, _ in outs)
    kw = {name: args[name] for name, _, _ in ins}
    return getattr(d, op + ("_shard" if shard else ""))(args["x"], out=out[0] if len(out) == 1 else out, **kw)


@pytest.mark.parametrize("op,shard", METHODS, ids=[op + ("_shard" if shard else "") for op, shard in METHODS])
def test_matrix_free_method_checks_its_arguments(handles, op, shard):
    d = handles[shard]
    size = {"v": d.dim_NLP_variables, "c": d.dim_NLP_constraints}
    ins, outs = OPS[op]
    lengths = {"x": size["v"], **{name: size[lay] for name, lay, _ in ins}, **{name: size[lay] for name, lay in outs}}
    tensor = lambda n: torch.zeros(n, dtype=torch.float64)      # noqa: E731
    kinds = (tensor,) if shard else (tensor, np.zeros)          # (the whole-grid methods have a host path too)
    for make in kinds:
        good = {name: make(n) for name, n in lengths.items()}
        # every vector of wrong length: the ValueError names it -- as "<name> has N entries, expected M" wherever the method itself
        # compares the lengths (x everywhere, every vector of a shard method, the inputs of the host path).  The device path of the
        # whole-grid methods leaves the other lengths to the per-tensor check, which on this machine refuses x first: not on a GPU
        for name, n in lengths.items():
            by_name = shard or name == "x" or (make is np.zeros and name not in dict(outs))
            named = by_name or make is np.zeros
            for wrong in (n + 1, n - 1):
                with pytest.raises(ValueError, match="^" + re.escape(name) + " " if named else "GPU") as ei:
                    _call(d, op, shard, {**good, name: make(wrong)})
                if by_name:
                    assert f"{name} has {wrong} entries, expected" in str(ei.value), ei.value
                    assert name == "x" or str(ei.value).endswith(f"expected {n}"), ei.value
        # a required argument left out
        for name in ["x"] + [name for name, _, required in ins if required]:
            with pytest.raises(ValueError, match=f"^{name} is required"):
                _call(d, op, shard, {**good, name: None})
    good = {name: tensor(n) for name, n in lengths.items()}
    if shard:
        # NumPy input: there is no host path, whichever argument it is
        for name, n in lengths.items():
            with pytest.raises(TypeError, match=re.escape(f"{name} must be a device tensor: {op}_shard has no host path")):
                _call(d, op, shard, {**good, name: np.zeros(n)})
    # tensors of the right lengths pass these checks: what stops them here is that they are not on a GPU -- with every optional
    # argument, with none of them, and with the outputs left to the method
    optional = {name: None for name, _, required in ins if not required}
    no_out = {name: None for name, _ in outs}
    for args in (good, {**good, **optional}, {**good, **no_out}):
        with pytest.raises(ValueError, match="GPU"):
            _call(d, op, shard, args)
    # ... and on the host path what stops them is the handle, which has no device
    if not shard:
        host = {name: np.zeros(n) for name, n in lengths.items()}
        for args in (host, {**host, **optional}, {**host, **no_out}):
            with pytest.raises(ct.CTDirectError) as ei:
                _call(d, op, shard, args)
            assert ei.value.status == ct._lib.CTD_ENODEVICE
