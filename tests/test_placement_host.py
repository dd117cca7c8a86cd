"""The placement helper proved on the CPU (tests/placement.py): five planted faults are each caught and named, a correct
op passes, the allocation proxy places a module's own tensors -- and the PLACEMENT table is complete against
sudo_rm_rf_amd.ops by introspection, so that no op can be added without a placement entry.  This is what lets
tests/test_gpu_placement.py claim that a wrong kernel would be noticed."""
import inspect
import types

import pytest
import torch

from tests import placement as pl

ROWS, COLS = 5, 37


def _arena():
    return pl.Arena("cpu", 1 << 20)


def _outside(t, first, n=1):
    """n floats of t's storage starting `first` elements relative to t's first element (may lie outside t)."""
    return t.as_strided((n,), (1,), t.storage_offset() + first)


# ---- plain torch "ops": out = 2 x + 1 on [ROWS, COLS], one correct and five wrong in one way each ---------------------
def op_correct(x, out):
    out.copy_(2 * x + 1)


def op_writes_before(x, out):
    op_correct(x, out)
    _outside(out, -1).fill_(3.0)


def op_writes_after(x, out):
    op_correct(x, out)
    _outside(out, out.numel()).fill_(3.0)


def op_writes_a_row_after(x, out):
    op_correct(x, out)
    _outside(out, out.numel() + COLS).fill_(3.0)


def op_leaves_one_unwritten(x, out):
    flat = out.view(-1)
    flat[:-1] = (2 * x + 1).view(-1)[:-1]


def op_reads_past_input(x, out):
    shifted = _outside(x, 1, x.numel()).view(x.shape)        # every element one too far: the last comes from the guard
    out.copy_(2 * shifted + 1)


def _run(op, shift_x=0, shift_out=0):
    a = _arena()
    g = torch.Generator().manual_seed(1)
    x64 = torch.randn(ROWS, COLS, generator=g, dtype=torch.float64)
    x = a.put(x64, shift_floats=shift_x, name="x")
    out = a.place((ROWS, COLS), shift_floats=shift_out, name="out")
    op(x, out)
    return a, x64, out


def _all_checks(a, x64, out):
    a.check()
    a.assert_written(out)
    a.assert_clean(out)
    assert float((out.double() - (2 * x64.float().double() + 1)).abs().max()) <= 1e-6


@pytest.mark.parametrize("shift_x,shift_out", [(0, 0), (1, 0), (0, 3), (2, 1)])
def test_a_correct_op_passes_every_check(shift_x, shift_out):
    a, x64, out = _run(op_correct, shift_x, shift_out)
    assert out.data_ptr() % 256 == 4 * shift_out and a.payloads[0].ptr % 256 == 4 * shift_x
    _all_checks(a, x64, out)


def test_a_write_before_the_output_is_caught_and_named():
    a, x64, out = _run(op_writes_before)
    with pytest.raises(pl.PlacementError, match=r"BEFORE operand 'out'.*byte offsets -4 \.\. -4"):
        a.check()


def test_a_write_after_the_output_is_caught_and_named():
    a, x64, out = _run(op_writes_after, shift_out=1)
    with pytest.raises(pl.PlacementError, match=r"AFTER operand 'out'.*byte offsets \+0 \.\. \+0"):
        a.check()


def test_a_write_one_row_after_the_output_is_caught_and_named():
    a, x64, out = _run(op_writes_a_row_after)
    with pytest.raises(pl.PlacementError, match=r"AFTER operand 'out'.*byte offsets \+%d \.\. \+%d" % (4 * COLS, 4 * COLS)):
        a.check()


def test_an_unwritten_element_is_caught_and_named():
    a, x64, out = _run(op_leaves_one_unwritten)
    a.check()                                                   # nothing outside was touched
    assert a.unwritten(out) == 1
    with pytest.raises(pl.PlacementError, match=r"operand 'out': 1 of %d word\(s\) of the output were never written" % (ROWS * COLS)):
        a.assert_written(out)
    with pytest.raises(pl.PlacementError, match="operand 'out': 1 NaN"):
        a.assert_clean(out)


def test_a_read_past_the_input_is_caught_and_named():
    a, x64, out = _run(op_reads_past_input)
    a.check()
    # (the poison may survive the arithmetic bit for bit -- a NaN's payload propagates -- so the word can also count as
    # unwritten; the NaN check is the one that must fire)
    with pytest.raises(pl.PlacementError, match=r"operand 'out': 1 NaN value\(s\), first at index \[%d, %d\]" % (ROWS - 1, COLS - 1)):
        a.assert_clean(out)


def test_guards_hold_two_rows_plus_256_floats_and_damage_goes_to_the_nearer_operand():
    a = _arena()
    first = a.place((3, 100), name="first")
    second = a.place((7,), shift_floats=2, name="second")
    p, q = a.payloads
    assert p.start >= pl.guard_bytes((3, 100)) >= (2 * 100 + 256) * 4
    assert q.start - p.end >= pl.guard_bytes((3, 100)) + pl.guard_bytes((7,))
    assert a.nbytes - q.end >= pl.guard_bytes((7,))
    first.zero_(), second.zero_()
    _outside(first, first.numel() + 200).fill_(0.0)             # two rows past `first`
    _outside(second, -2).fill_(0.0)
    with pytest.raises(pl.PlacementError) as e:
        a.check()
    assert "AFTER operand 'first'" in str(e.value) and "+800 .. +800" in str(e.value)
    assert "BEFORE operand 'second'" in str(e.value) and "-8 .. -8" in str(e.value)


def test_a_refusal_must_leave_the_output_untouched():
    a = _arena()
    out = a.place((4, 4), name="y")
    a.assert_untouched(out)
    out[1, 1] = 0.0
    with pytest.raises(pl.PlacementError, match="operand 'y': 4 byte"):
        a.assert_untouched(out)


def test_the_allocation_proxy_places_a_modules_own_tensors():
    mod = types.ModuleType("fake_ops")
    mod.torch = torch

    def wrapper(x):
        y = torch.empty_like(x)                                  # noqa: F821 (resolved through the module global below)
        acc = torch.zeros((3,), dtype=torch.float64, device=x.device)
        scratch = torch.empty(10, dtype=torch.uint8, device=x.device)
        y.copy_(x + 1)
        return y, acc, scratch, torch.float32
    mod.wrapper = types.FunctionType(wrapper.__code__, mod.__dict__)
    a = _arena()
    x = a.put(torch.ones(4, 6, dtype=torch.float64), name="x")
    with a.allocating(mod, names=("y", "acc"), shifts={"y": 3, "acc": 1}) as made:
        y, acc, scratch, f32 = mod.wrapper(x)
    assert mod.torch is torch and f32 is torch.float32
    assert [n for n, _ in made] == ["y", "acc", "alloc2"]
    assert a.owns(y) and a.owns(acc) and a.owns(scratch)
    assert y.data_ptr() % 256 == 12 and acc.data_ptr() % 256 == 8     # a double starts on an even float
    assert a.unwritten(y) == 0 and float(acc.abs().sum()) == 0.0 and a.unwritten(acc) == 0
    assert bytes(scratch.tolist()) == b"\xff" * 10                     # empty() stays poisoned
    a.check()


# ---- the declared contract ------------------------------------------------------------------------------------------
def test_placement_table_covers_every_public_op():
    ops_entries = {k for k in pl.PLACEMENT if "." not in k}
    public = pl.public_ops()
    assert not (set(pl.EXCLUDED) & ops_entries)
    assert set(pl.EXCLUDED) <= public, set(pl.EXCLUDED) - public
    assert ops_entries == public - set(pl.EXCLUDED), (sorted(public - set(pl.EXCLUDED) - ops_entries),
                                                      sorted(ops_entries - public))
    for name, why in pl.EXCLUDED.items():
        assert why


def test_placement_table_names_every_tensor_argument_of_every_op():
    """Each entry lists the wrapper's tensor parameters (everything but the integer / flag arguments below) and the tensors the
    wrapper allocates; kinds and notes are well formed."""
    from sudo_rm_rf_amd import ops
    scalars = {"L", "groups", "stride", "padding", "dilation", "T", "Cmid", "Cout2", "mix_weights_type", "want_bias", "D",
               "want_gin", "K", "hop", "pad", "rows_out", "hscale"}
    for name, entry in pl.PLACEMENT.items():
        assert entry["operands"], name
        for operand, (kind, note) in entry["operands"].items():
            assert kind in (pl.FALLBACK, pl.REFUSES, pl.NA) and note, (name, operand)
        for alloc in entry["allocs"]:
            assert alloc in entry["operands"], (name, alloc)
        if "." in name:
            continue
        params = [p for p in inspect.signature(getattr(ops, name)).parameters if p not in scalars]
        missing = [p for p in params if p not in entry["operands"]]
        assert not missing, (name, missing)
