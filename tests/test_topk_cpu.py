"""What the reference of the per-row selection (tests/topk_ref.py) means, on the CPU: the k smallest E / w ARE a weighted sample
without replacement.  One row, weights [0.125, 1, 2.5, 0, 4, 0.375] at positions 1000 .. 1005, k = 2, salts 0 .. 199 999: the frequency
of each first pick against w / sum w, each inclusion frequency against the exact value of successive sampling by enumeration, both within
five binomial standard deviations (measured: every deviation below one); the zero weight is never picked; weights None equals unit
weights; LARGEST equals a plain stable argsort of -w.  No GPU."""
import numpy as np

from tests import topk_ref as ref

W = np.array([0.125, 1, 2.5, 0, 4, 0.375], dtype=np.float32)
FIRST = 1000
SALTS = 200_000
K = 2


def picks():
    """[SALTS, K] positions inside the row, best first, by the reference's keys."""
    e = np.arange(FIRST, FIRST + W.size, dtype=np.int64)
    salts = np.arange(SALTS, dtype=np.int64)
    E = ref.exp_variate(e[None, :], salts[:, None])
    with np.errstate(divide="ignore"):
        key = E / W.astype(np.float64)[None, :]
    one = ref.keys(ref.SAMPLE, e, np.zeros(W.size, np.int32), W, 12345)        # the vectorised keys are ref.keys': one salt in full
    assert np.array_equal(np.where(one[1], key[12345].view(np.uint64), ref.NO_KEY), one[0])
    key[:, W <= 0] = np.inf
    return np.argsort(key, axis=1, kind="stable")[:, :K]


def test_the_k_smallest_keys_are_a_weighted_sample_without_replacement():
    got = picks()
    p = W.astype(np.float64) / W.sum(dtype=np.float64)
    first = np.bincount(got[:, 0], minlength=W.size) / SALTS
    incl = np.bincount(got.reshape(-1), minlength=W.size) / SALTS
    want_incl = np.array([p[i] + sum(p[j] * p[i] / (1 - p[j]) for j in range(W.size) if j != i and p[j] > 0) if p[i] > 0 else 0.0
                          for i in range(W.size)])
    assert abs(want_incl.sum() - K) < 1e-12
    for name, f, q in (("first pick", first, p), ("inclusion", incl, want_incl)):
        sd = np.sqrt(q * (1 - q) / SALTS)
        dev = np.abs(f - q) / np.where(sd > 0, sd, 1)
        print(name, "deviations in standard deviations:", np.round(dev, 3))
        assert np.all(dev < 5), (name, f, q, dev)
    assert first[3] == 0 and incl[3] == 0, "the zero weight is never picked"
    assert np.all(got[:, 0] != got[:, 1])


def row_graph(w):
    indptr = np.array([0, 0, w.size], dtype=np.int64)
    col = np.arange(w.size, dtype=np.int32) + 10
    return indptr, col


def test_row_topk_takes_the_same_picks():
    """row_topk on the row placed at position 1000 (add=) is the argsort above."""
    got = picks()[:50]
    indptr, col = row_graph(W)
    for salt in range(50):
        src, eid, cnt = ref.row_topk(indptr, col, W, [1], K, ref.SAMPLE, salt, add=FIRST)
        assert cnt[0] == K and np.array_equal(eid[0] - FIRST, got[salt]) and np.array_equal(src[0], col[got[salt]])


def test_no_weights_are_unit_weights():
    indptr, col = row_graph(W)
    col = col.copy()
    col[2] = -1
    for salt in (0, 1, -7):
        for k in (1, 3, 6):
            a = ref.row_topk(indptr, col, None, [1, 0, 1, 5, -1], k, ref.SAMPLE, salt)
            b = ref.row_topk(indptr, col, np.ones(W.size, np.float32), [1, 0, 1, 5, -1], k, ref.SAMPLE, salt)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
            assert a[2].tolist() == [min(k, 5), 0, min(k, 5), 0, 0] and np.array_equal(a[0][0], a[0][2]) and -1 not in a[1][0, :min(k, 5)]


def test_largest_is_a_stable_argsort_of_minus_w():
    rng = np.random.RandomState(3)
    w = (rng.randint(-8, 9, size=300) / 8).astype(np.float32)
    w[[5, 77]] = np.inf
    w[[6, 78]] = -np.inf
    w[9] = -0.0
    indptr, col = row_graph(w)
    order = np.argsort(-w.astype(np.float64), kind="stable")
    for k in (1, 25, 64):
        src, eid, cnt = ref.row_topk(indptr, col, w, [1], k, ref.LARGEST, 0)
        assert cnt[0] == k and np.array_equal(eid[0], order[:k])
        src, eid, cnt = ref.row_topk(indptr, col, w, [1], k, ref.SMALLEST, 0)
        assert np.array_equal(eid[0], np.argsort(w.astype(np.float64), kind="stable")[:k])
    w[0] = np.nan
    assert 0 not in ref.row_topk(indptr, col, w, [1], 64, ref.LARGEST, 0)[1]
