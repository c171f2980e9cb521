"""tests/compare.py same_arrays, the compare the GPU tests rest on, is itself able to fail: it accepts equal arrays and names the first
differing element, a wrong dtype and a wrong shape.  Numpy only."""
import numpy as np
import pytest

from tests.compare import same_arrays

A1 = np.arange(7, dtype=np.int32)
A2 = np.arange(12, dtype=np.int64).reshape(3, 4)


def _changed(a, at, value):
    b = a.copy()
    b[at] = value
    return b


def test_equal_arrays_pass():
    same_arrays(A1.copy(), A1, "1-D")
    same_arrays(A2.copy(), A2, "2-D")
    same_arrays([A1.copy(), A2.copy()], (A1, A2), "both", names=("traces", "edge ids"))


@pytest.mark.parametrize("got, want, says", [
    (_changed(A1, 5, -3), A1, ["1 elements differ", "first at (5,)", "got -3 want 5"]),
    (_changed(A2, (2, 1), 77), A2, ["1 elements differ", "first at (2, 1)", "got 77 want 9"]),
    (A1.astype(np.int64), A1, ["int64", "int32"]),
    (A1[:6], A1, ["(6,)", "(7,)"]),
    ([A1.copy(), _changed(A2, (0, 3), -1)], [A1, A2], ["edge ids: 1 elements differ", "first at (0, 3)", "got -1 want 3"]),
], ids=["one_element_1d", "one_element_2d", "dtype", "shape", "second_of_a_sequence"])
def test_a_difference_raises_and_is_named(got, want, says):
    with pytest.raises(AssertionError) as e:
        same_arrays(got, want, "the case", names=("traces", "edge ids") if isinstance(got, list) else None)
    assert str(e.value).startswith("the case: ") and all(s in str(e.value) for s in says), str(e.value)
