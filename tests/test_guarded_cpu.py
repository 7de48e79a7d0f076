"""tests/guarded.py fires: stray stores made by the test itself, as plain host tensor assignments, are reported with the right
offsets, and an untouched buffer passes.  Nothing of the engine runs."""
import numpy as np
import pytest
import torch

from guarded import MIN_GUARD, SENTINEL, guard_len, guarded


def raw(g):
    """the whole buffer as float64: what a stray store of a kernel would hit"""
    return g.buf.view(torch.float64)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", [1, 7, 100])
def test_layout_and_alignment(n, shift):
    g = guarded(torch, n, shift, "cpu")
    assert g.G == MIN_GUARD and g.G % 2 == 0 and g.buf.numel() == 2 * g.G + shift + n and g.buf.dtype == torch.int64
    assert g.view.dtype == torch.float64 and g.view.numel() == n and g.view.is_contiguous()
    assert g.buf.data_ptr() % 16 == 0
    assert g.view.data_ptr() - g.buf.data_ptr() == 8 * (g.G + shift)
    assert g.view.data_ptr() % 16 == (8 if shift else 0)
    assert bool(torch.isnan(g.view).all())                              # the sentinel is a NaN ...
    assert bool((g.buf == SENTINEL).all())                              # ... with its payload intact
    assert g.unwritten() == list(range(n))
    assert g.guards_intact()


def test_guards_are_as_long_as_the_output():
    assert guard_len(1) == MIN_GUARD and guard_len(MIN_GUARD + 1) == MIN_GUARD + 2 and guard_len(200001) == 200002
    g = guarded(torch, MIN_GUARD + 3, 1, "cpu")
    assert g.G == MIN_GUARD + 4 and g.G >= g.n
    assert g.view.data_ptr() % 16 == 8


def test_an_untouched_buffer_passes_and_payload_writes_are_not_guard_hits():
    like = np.arange(5.0)
    g = guarded(torch, 5, 1, "cpu", like=like).snapshot()
    assert g.guards_intact() and g.unchanged() and g.unwritten() == []
    assert np.array_equal(g.view.numpy(), like)
    out = guarded(torch, 5, 0, "cpu")
    out.view[1] = 2.0
    out.view[3] = float("nan")                                          # a NaN a kernel computed is a written entry
    assert out.guards_intact() and out.unwritten() == [0, 2, 4]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("where,offset", [("just before", -1), ("just after", 0), ("G - 1 before", None), ("G - 1 after", None)])
def test_one_stray_double_is_reported_with_its_offset(where, offset, shift):
    n = 9
    g = guarded(torch, n, shift, "cpu")
    if where == "just after":
        offset = n
    elif where == "G - 1 before":
        offset = -(g.G - 1)
    elif where == "G - 1 after":
        offset = n + g.G - 2                                            # G - 1 doubles past the last payload entry
    raw(g)[g.lo + offset] = 1.5
    assert g.touched() == [offset]
    with pytest.raises(AssertionError) as e:
        g.guards_intact("probe")
    msg = str(e.value)
    assert msg.startswith("probe: 1 guard word(s) written") and f"offsets {offset} .. {offset} " in msg
    assert g.unwritten() == list(range(n))                              # (the payload itself was not touched)


def test_first_and_last_offsets_and_the_count():
    g = guarded(torch, 4, 1, "cpu")
    for off in (-3, -1, 4, 6, 10):
        raw(g)[g.lo + off] = 0.0
    assert g.touched() == [-3, -1, 4, 6, 10]
    with pytest.raises(AssertionError, match=r"5 guard word\(s\) written, offsets -3 \.\. 10 relative to a payload of 4"):
        g.guards_intact()


def test_a_nan_written_into_a_guard_is_a_hit():
    g = guarded(torch, 4, 0, "cpu")
    raw(g)[g.lo - 2] = float("nan")                                     # compared as int64: the canonical NaN is not the sentinel
    assert g.touched() == [-2]
    with pytest.raises(AssertionError):
        g.guards_intact()


@pytest.mark.parametrize("offset", [0, 3, -1, 4])
def test_a_write_into_a_snapshotted_input_is_reported(offset):
    g = guarded(torch, 4, 1, "cpu", like=np.array([1.0, 2.0, 3.0, 4.0])).snapshot()
    assert g.unchanged()
    raw(g)[g.lo + offset] = 2.5
    with pytest.raises(AssertionError, match=rf"1 word\(s\) of an input buffer changed, offsets {offset} \.\. {offset} "):
        g.unchanged("x")
    g2 = guarded(torch, 4, 1, "cpu", like=np.array([1.0, 2.0, 3.0, 4.0])).snapshot()
    g2.view[2] = -3.0                                                   # the same magnitude, another bit
    with pytest.raises(AssertionError, match=r"offsets 2 \.\. 2 "):
        g2.unchanged()
