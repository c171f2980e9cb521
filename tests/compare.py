"""The bit-for-bit array compare of the GPU tests: same dtype, same shape, every element equal.  Numpy only; a device tensor is
anything with .cpu().numpy()."""
import numpy as np


def same_arrays(got, want, ctx, names=None):
    """got: a device tensor, a numpy array, or a sequence of either; want: numpy, or a sequence of as many.  names: what each array is
    called in the message, at least as many as arrays (a file's domain word goes here, or into ctx).  A failure says how many elements differ, the index of the first
    and got / want there -- or the dtypes and shapes, when those differ."""
    if not isinstance(got, (list, tuple)):
        got, want = [got], [want]
    names = names or (["array"] if len(got) == 1 else [f"array {i}" for i in range(len(got))])
    assert len(got) == len(want) <= len(names), f"{ctx}: {len(got)} arrays, want {len(want)}"
    for name, a, b in zip(names, got, want):
        a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        assert a.dtype == b.dtype and a.shape == b.shape, f"{ctx}: {name}: got {a.dtype} {a.shape} want {b.dtype} {b.shape}"
        bad = np.argwhere(a != b)
        if len(bad):
            at = tuple(int(x) for x in bad[0])
            raise AssertionError(f"{ctx}: {name}: {len(bad)} elements differ, first at {at}: got {a[at]} want {b[at]}")
