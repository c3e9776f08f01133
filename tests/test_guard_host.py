"""The premise of tests/test_gpu_forward_bounds.py, on CPU tensors: util.guarded's check() passes on an exactly-filled interior and
names the first offending element of a stray write (front guard, back guard, pad column) or of a missing write; util.poisoned_input
surrounds an operand with NaN."""
import pytest
import torch

from util import NAN_WORD, guarded, poisoned_input

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
CPU = torch.device("cpu")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ld", [None, 13])
def test_check_passes_on_an_exactly_filled_interior(dtype, ld):
    view, check = guarded(5, 11, dtype, CPU, ld=ld, guard_rows=3)
    assert view.shape == (5, 11) and view.stride() == (ld or 11, 1)
    assert bool(torch.isnan(view.float()).all())  # the fill is a NaN in every storage type
    view.copy_(torch.arange(55, dtype=torch.float32).view(5, 11))
    check()


def test_fill_is_the_nan_word():
    v32, _ = guarded(2, 2, torch.float32, CPU, guard_rows=1)
    v16, _ = guarded(2, 2, torch.bfloat16, CPU, guard_rows=1)
    assert int(v32.contiguous().view(torch.int32)[0, 0]) == NAN_WORD
    assert int(v16.contiguous().view(torch.int16)[0, 0]) == NAN_WORD & 0xFFFF


def _filled(dtype, rows=5, cols=11, ld=13, g=3):
    view, check = guarded(rows, cols, dtype, CPU, ld=ld, guard_rows=g)
    view.fill_(1.0)
    return view, check


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_names_a_write_in_the_front_guard(dtype):
    view, check = _filled(dtype)
    view.as_strided((1,), (1,), view.storage_offset() - 2 * 13 + 4).fill_(0.0)  # two rows before the first, column 4
    with pytest.raises(AssertionError, match=r"stray write in the front guard at \(row -2, column 4\)"):
        check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_names_a_write_in_the_back_guard(dtype):
    view, check = _filled(dtype)
    view.as_strided((1,), (1,), view.storage_offset() + 6 * 13 + 12).fill_(3.0)  # one row past the last row, column 12
    with pytest.raises(AssertionError, match=r"stray write in the back guard at \(row 6, column 12\)"):
        check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_names_a_write_in_a_pad_column(dtype):
    view, check = _filled(dtype)
    view.as_strided((1,), (1,), view.storage_offset() + 2 * 13 + 11).fill_(0.0)  # row 2, the first pad column
    with pytest.raises(AssertionError, match=r"stray write in the pad columns at \(row 2, column 11\)"):
        check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_names_an_unwritten_interior_element(dtype):
    view, check = guarded(5, 11, dtype, CPU, ld=13, guard_rows=3)
    src = torch.ones(5, 11)
    view.copy_(src)
    fresh, _ = guarded(5, 11, dtype, CPU, ld=13, guard_rows=3)
    view[4, 10] = fresh[4, 10]  # the last element keeps the fill: a skipped tail
    with pytest.raises(AssertionError, match=r"missing write \(still the fill pattern\) at \(row 4, column 10\)"):
        check()


def test_check_tells_a_written_non_finite_value_from_a_missing_write():
    view, check = _filled(torch.float32)
    view[1, 3] = float("inf")
    with pytest.raises(AssertionError, match=r"non-finite value written \(inf\) at \(row 1, column 3\)"):
        check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_poisoned_input_surrounds_the_operand_with_nan(dtype):
    t = torch.arange(12, dtype=torch.float32).view(3, 4).to(dtype)
    v = poisoned_input(t, 7, tail_rows=2)
    assert v.shape == (3, 4) and v.stride() == (7, 1) and torch.equal(v, t)
    whole = v.as_strided((5, 7), (7, 1), v.storage_offset()).float()
    assert bool(torch.isnan(whole[:3, 4:]).all()) and bool(torch.isnan(whole[3:]).all())
    # what a kernel that masks by multiplication computes from the pad: 0 x NaN is NaN
    assert bool(torch.isnan(whole[0, 4] * 0.0))
