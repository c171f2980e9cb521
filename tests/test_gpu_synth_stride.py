"""The synthetic instruments (kernels_synth.hip) past their grid caps, word for word against the numpy restatements in legion_amd/synth.py.

    rmat_kernel                   4096 x 256 = 1 048 576 edges a pass    E = 1 048 576 + 4099, scale 17 / 21 / 28 (the fifth, sixth and
                                                                         seventh hash word of an edge) and scale 1 (every edge a self loop)
    synth_features_kernel         8192 x 256 = 2 097 152 words a pass    20 000 rows of 107 words, with row * dim across 2^31 and 2^32
    synth_feature_check_kernel    2048 x 256 =   524 288 words a pass    6 000 rows of 100 words, mismatches planted in both passes
    consume_batch_kernel          (n_floats / 4 + n_edges) / 1024        2.2 M small-integer floats, 2 200 001 edges: every sum is exact.  Floats
                                  workgroups, at most 2048               with edges, and the edges alone, launch the clamped grid; the floats
                                                                         alone launch 538 workgroups (the clamp needs 8.4 M floats), whose
                                                                         threads still go round the 16-byte loop four times and the
                                                                         unaligned loop sixteen times

The generator and its checker share synth_feature_value, so the full-size property tests, which ask the checker whether gathered rows
are right, cannot see an error the two have in common.  features_numpy / feature_rows_numpy index in int64 on their own."""
import ctypes

import numpy as np
import pytest
import torch

from legion_amd import synth

DEV = "cuda:0"

RMAT_PASS = 4096 * 256
RMAT_E = RMAT_PASS + 4099
RMAT_SCALES = [1, 17, 21, 28]
RMAT_SEEDS = [20231, (1 << 63) | 0x5DEECE66D]
FEAT_PASS = 8192 * 256
FEAT_ROWS, FEAT_D, FEAT_SEED = 20_000, 107, 0xC0FFEE1234567
FEAT_FIRST = [0, (1 << 31) // FEAT_D - 9_000, (1 << 32) // FEAT_D - 11_000]
CHECK_PASS = 2048 * 256
CHECK_ROWS, CHECK_D, CHECK_SEED = 6_000, 100, 77
CONSUME_GRID_CAP = 2048
CONSUME_FLOATS = 2_200_000
CONSUME_EDGES = 2_200_001


def consume_grid(n_floats, n_edges):
    """The workgroups legion_consume_batch launches (256 threads each)."""
    return max(1, min((n_floats // 4 + n_edges + 1023) // 1024, CONSUME_GRID_CAP))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# ---- the reference side alone ------------------------------------------------------------------------------------------------
def test_inputs_cross_every_cap():
    assert RMAT_PASS < RMAT_E < 2 * RMAT_PASS
    assert [(s + 3) // 4 for s in RMAT_SCALES] == [1, 5, 6, 7], "scale 17 draws the fifth hash word of an edge, 28 the seventh"
    assert FEAT_PASS < FEAT_ROWS * FEAT_D < 2 * FEAT_PASS
    lo = [f * FEAT_D for f in FEAT_FIRST]
    hi = [(f + FEAT_ROWS) * FEAT_D for f in FEAT_FIRST]
    assert lo[0] == 0 and lo[1] < (1 << 31) < hi[1] < (1 << 32) and (1 << 31) < lo[2] < (1 << 32) < hi[2]
    # both sides of each power of two hold words of both grid passes' neighbourhood: thousands of rows before and after it
    assert min((1 << 31) - lo[1], hi[1] - (1 << 31), (1 << 32) - lo[2], hi[2] - (1 << 32)) > 5_000 * FEAT_D
    assert CHECK_PASS < CHECK_ROWS * CHECK_D < 2 * CHECK_PASS
    # the consumer's grid follows its inputs: floats with edges, and the edges alone, ask for more than the cap and launch the clamped grid;
    # the floats alone do not reach the clamp, and each of their threads still goes round both float loops more than once
    assert (CONSUME_FLOATS // 4 + CONSUME_EDGES + 1023) // 1024 > CONSUME_GRID_CAP and (CONSUME_EDGES + 1023) // 1024 > CONSUME_GRID_CAP
    assert consume_grid(CONSUME_FLOATS, CONSUME_EDGES) == consume_grid(0, CONSUME_EDGES) == CONSUME_GRID_CAP
    assert CONSUME_EDGES > CONSUME_GRID_CAP * 256 * 4, "four passes and more of the edge loop under the clamped grid"
    floats_only = consume_grid(CONSUME_FLOATS, 0)
    assert floats_only < CONSUME_GRID_CAP and CONSUME_FLOATS // 4 > 3 * floats_only * 256 and CONSUME_FLOATS > 15 * floats_only * 256


def test_a_32_bit_row_times_dim_differs_from_the_reference():
    """What a generator that formed row * dim + f in 32 bits would write: equal to the reference below 2^31, different above."""
    for first in FEAT_FIRST[1:]:
        want = synth.features_numpy(first, FEAT_ROWS, FEAT_D, FEAT_SEED)
        idx = (np.arange(first, first + FEAT_ROWS, dtype=np.int64)[:, None] * FEAT_D + np.arange(FEAT_D, dtype=np.int64)[None, :])
        narrow = idx.astype(np.int32).astype(np.int64).astype(np.uint64)           # wrapped, then sign-extended as the kernel would
        h = synth.splitmix64_np(np.uint64(FEAT_SEED) ^ narrow)
        got = ((h >> np.uint64(40)).astype(np.int64).astype(np.float32) * np.float32(1.0 / 8388608.0) - np.float32(1.0)).astype(np.float32)
        differs = (got.view(np.uint32) != want.view(np.uint32)).mean(axis=1)
        assert differs.max() > 0.99 and (differs > 0.99).sum() > 5_000


@pytest.mark.parametrize("scale", RMAT_SCALES)
def test_rmat_reference_has_no_self_loops_and_stays_in_range(scale):
    for seed in RMAT_SEEDS:
        for key in (0, synth.SCRAMBLE_KEY):
            u, v = synth.rmat_edges_numpy(scale, RMAT_E, seed, key)
            assert u.size == v.size == RMAT_E
            assert not np.any(u == v)
            assert u.min() >= 0 and v.min() >= 0 and max(int(u.max()), int(v.max())) < (1 << scale)
    if scale == 1:
        u, v = synth.rmat_edges_numpy(1, RMAT_E, RMAT_SEEDS[0])
        assert np.array_equal(v, u ^ 1) and 0 < u.sum() < RMAT_E        # both labels occur; every v is the fixed self loop


@pytest.mark.parametrize("scale", [17, 21])
def test_scramble_is_a_bijection(scale):
    x = np.arange(1 << scale)
    for key in (synth.SCRAMBLE_KEY, RMAT_SEEDS[1]):
        assert np.array_equal(np.sort(synth.scramble_labels_numpy(x, scale, key)), x)


def _checker_world():
    rng = np.random.RandomState(41)
    ids = rng.randint(0, 2**31 - 1, CHECK_ROWS).astype(np.int64)
    ids[[0, 5, 2600, CHECK_ROWS - 1]] = [0, 2**31 - 1, 2**31 - 2, 2**31 - 1]
    dead = np.array([1, 700, 2601, 5300, CHECK_ROWS - 2])
    rows = synth.feature_rows_numpy(ids, CHECK_D, CHECK_SEED)
    ids32 = ids.astype(np.int32)
    ids32[dead] = -1
    return ids32, rows, dead


def _planted():
    """(word, kind) of every planted mismatch: kind 0 flips the lowest mantissa bit, 1 the sign bit, 2 stores a NaN."""
    total = CHECK_ROWS * CHECK_D
    same_thread = 31_007                                    # this thread's second word is CHECK_PASS further on
    words = [0, total - 1, 260_211, CHECK_PASS + 40_123, same_thread, same_thread + CHECK_PASS, CHECK_PASS - 1, CHECK_PASS]
    return [(w, i % 3) for i, w in enumerate(words)]


def _plant(rows, words):
    bits = rows.reshape(-1).view(np.uint32).copy()
    for w, kind in words:
        bits[w] = [bits[w] ^ 1, bits[w] ^ 0x80000000, 0x7FC00000][kind]
    return bits.view(np.float32).reshape(rows.shape)


def test_checker_inputs_from_the_reference_side():
    ids, rows, dead = _checker_world()
    assert {-1, 0, 2**31 - 1, 2**31 - 2} <= set(ids.tolist()) and not np.isnan(rows).any()
    planted = _planted()
    words = np.array([w for w, _ in planted])
    assert np.unique(words).size == words.size and {k for _, k in planted} == {0, 1, 2}
    assert words.min() == 0 and words.max() == CHECK_ROWS * CHECK_D - 1
    assert (words < CHECK_PASS).sum() >= 2 and (words >= CHECK_PASS).sum() >= 2
    pairs = [(a, b) for a in words for b in words if b == a + CHECK_PASS]
    assert pairs, "two words of one thread, one in each pass"
    assert not np.isin(words // CHECK_D, dead).any(), "no planted word lies under an id of -1"
    assert ((ids.astype(np.int64) * CHECK_D) >= (1 << 32)).mean() > 0.9, "most ids put row * dim past 2^32"
    bad = _plant(rows, planted)
    assert int((bad.view(np.uint32) != rows.view(np.uint32)).sum()) == len(planted)


# ---- the device ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scramble", [False, True], ids=["plain", "scrambled"])
@pytest.mark.parametrize("scale", RMAT_SCALES)
def test_rmat_edges_are_the_reference(hip, scale, scramble):
    src = torch.empty(RMAT_E + 64, dtype=torch.int32, device=DEV)
    dst = torch.empty(RMAT_E + 64, dtype=torch.int32, device=DEV)
    for seed in RMAT_SEEDS:
        src.fill_(-7); dst.fill_(-7)
        if scramble:
            hip.legion_synth_rmat_edges_scrambled(_stream(), scale, RMAT_E, seed, _p(src), _p(dst), synth.SCRAMBLE_KEY)
        else:
            hip.legion_synth_rmat_edges(_stream(), scale, RMAT_E, seed, _p(src), _p(dst))
        torch.cuda.synchronize()
        u, v = synth.rmat_edges_numpy(scale, RMAT_E, seed, synth.SCRAMBLE_KEY if scramble else 0)
        gu, gv = src.cpu().numpy(), dst.cpu().numpy()
        for name, got, want in (("src", gu, u), ("dst", gv, v)):
            bad = np.nonzero(got[:RMAT_E] != want)[0]
            assert bad.size == 0, f"scale {scale} seed {seed:#x} {name}: {bad.size} edges differ, first at {bad[:5]}"
            assert np.all(got[RMAT_E:] == -7), f"{name}: written past num_edges"


@pytest.mark.gpu
@pytest.mark.parametrize("first_row", FEAT_FIRST, ids=["row0", "across-2^31", "across-2^32"])
def test_features_are_the_reference(hip, first_row):
    got = synth.features_device_rows(first_row, FEAT_ROWS, FEAT_D, FEAT_SEED, device=DEV)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = synth.features_numpy(first_row, FEAT_ROWS, FEAT_D, FEAT_SEED)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(-1))[0]
    assert bad.size == 0, f"{bad.size} words differ, first at {bad[:5]} (row {first_row + bad[:5] // FEAT_D})"
    if first_row == 0:
        assert np.array_equal(synth.features_device(FEAT_ROWS, FEAT_D, FEAT_SEED, device=DEV).cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.gpu
def test_checker_counts_exactly_what_is_planted(hip):
    ids, rows, dead = _checker_world()
    d_ids = torch.from_numpy(ids).to(DEV)
    assert synth.feature_check_device(torch.from_numpy(rows).to(DEV), d_ids, CHECK_D, CHECK_SEED) == 0
    planted = _planted()
    bad = torch.from_numpy(_plant(rows, planted)).to(DEV)
    assert synth.feature_check_device(bad, d_ids, CHECK_D, CHECK_SEED) == len(planted)
    assert synth.feature_check_device(bad, d_ids, CHECK_D, CHECK_SEED) == len(planted), "a fresh counter repeats the count"
    for i, one in enumerate(planted):                       # each of them alone, so that none can stand in for another
        assert synth.feature_check_device(torch.from_numpy(_plant(rows, [one])).to(DEV), d_ids, CHECK_D, CHECK_SEED) == 1, f"planted {i}: {one}"
    under_dead = [(int(r) * CHECK_D + 3 + j, j % 3) for j, r in enumerate(dead)]
    worse = torch.from_numpy(_plant(rows, planted + under_dead)).to(DEV)
    assert synth.feature_check_device(worse, d_ids, CHECK_D, CHECK_SEED) == len(planted), "words under an id of -1 are not counted"
    # a counter that is not zero is added to, not overwritten
    count = torch.full((1,), 1000, dtype=torch.int64, device=DEV)
    hip.legion_synth_feature_check(_stream(), _p(bad), _p(d_ids), CHECK_ROWS, CHECK_D, CHECK_SEED, _p(count))
    torch.cuda.synchronize()
    assert int(count.item()) == 1000 + len(planted)


def _consume(hip, feats, n_floats, a, b, n_edges, acc):
    hip.legion_consume_batch(_stream(), _p(feats) if feats is not None else None, n_floats, _p(a) if a is not None else None,
                             _p(b) if b is not None else None, n_edges, _p(acc) if acc is not None else None)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_consumer_reads_every_word(hip):
    rng = np.random.RandomState(3)
    f = rng.randint(-8, 9, CONSUME_FLOATS + 8).astype(np.float32)
    f[[0, 1, 2, 3, CONSUME_FLOATS - 4, CONSUME_FLOATS - 3, CONSUME_FLOATS - 2, CONSUME_FLOATS - 1, CONSUME_FLOATS]] = \
        [64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384]  # dropping a first or last word, or reading one too many, changes the sum
    a = rng.randint(-1, 1 << 20, CONSUME_EDGES).astype(np.int32)
    b = rng.randint(-1, 1 << 20, CONSUME_EDGES).astype(np.int32)
    a[-1], b[0] = 1 << 30, (1 << 30) + 1
    fsum = np.cumsum(f.astype(np.int64))
    esum = int(a.astype(np.int64).sum() + b.astype(np.int64).sum())
    d_f, d_a, d_b = (torch.from_numpy(x).to(DEV) for x in (f, a, b))
    assert d_f.data_ptr() % 16 == 0
    acc = torch.zeros(1, dtype=torch.float64, device=DEV)

    def run(feats, n_floats, n_edges, into=None):
        into = torch.zeros(1, dtype=torch.float64, device=DEV) if into is None else into
        _consume(hip, feats, n_floats, d_a, d_b, n_edges, into)
        return float(into.item())

    for n in (CONSUME_FLOATS, CONSUME_FLOATS + 1, CONSUME_FLOATS + 3):             # n % 4 = 0, 1, 3
        assert n % 4 == n - CONSUME_FLOATS
        assert run(d_f, n, CONSUME_EDGES) == float(int(fsum[n - 1]) + esum), f"{n} floats"
    for n in (CONSUME_FLOATS, CONSUME_FLOATS + 1):                                    # the pointer one float on: no 16-byte loads
        assert d_f[1:].data_ptr() % 16 == 4
        assert run(d_f[1:], n, CONSUME_EDGES) == float(int(fsum[n]) - int(f[0]) + esum), f"unaligned, {n} floats"
    assert run(d_f, 0, CONSUME_EDGES) == float(esum), "edges only"
    assert run(None, 0, CONSUME_EDGES) == float(esum), "edges only, no feature pointer"
    assert run(d_f, CONSUME_FLOATS, 0) == float(int(fsum[CONSUME_FLOATS - 1])), "floats only"
    assert run(d_f, 3, 0) == float(int(fsum[2])) and run(d_f, 5, 1) == float(int(fsum[4]) + int(a[0]) + int(b[0])), "one workgroup"
    assert run(d_f, CONSUME_FLOATS, CONSUME_EDGES, acc) == float(int(fsum[CONSUME_FLOATS - 1]) + esum)
    assert run(d_f, CONSUME_FLOATS + 3, 17, acc) == float(int(fsum[CONSUME_FLOATS - 1]) + esum + int(fsum[CONSUME_FLOATS + 2]) +
                                                         int(a[:17].astype(np.int64).sum() + b[:17].astype(np.int64).sum())), "two calls accumulate"
    before = float(acc.item())
    _consume(hip, d_f, 0, d_a, d_b, 0, acc)                                           # empty inputs
    _consume(hip, d_f, -1, d_a, d_b, -5, acc)
    _consume(hip, d_f, CONSUME_FLOATS, d_a, d_b, CONSUME_EDGES, None)                 # a null accumulator
    assert float(acc.item()) == before
