"""The C ABI's legion_row_topk and legion_topk_keys on the GPU, bit for bit against tests/topk_ref.py.

  * the keys alone: every special weight (+-0, +-denormal, +-inf, NaN, FLT_MAX, negatives, eighths) in all three modes and the SAMPLE key
    over 10^5 positions and several salts, with and without weights.  This is the test that shows that the device fused no multiply-add
    of the exponential variate and divided as IEEE does;
  * the selection on a hand-made graph: row degrees 0, 1, 2, 24, 25, 26, 63, 64, 65, 127, 128, 129, 4 095, 4 096, 4 097 (the boundary
    between the wave-per-row and the workgroup-per-row class) and 70 001 (many steps per wave); an all-dead row, an all-zero-weight row,
    rows of equal weights (the first k live entries win) short and long; dead entries and special weights sprinkled over all of them.
    k in {1, 2, 5, 25, 63, 64}, all modes, eid_out and count_out present and null, row ids -1 and node_num, rows that repeat;
  * n = 0, every refusal over sentinel-filled buffers, w = NULL against unit weights, another stream and a captured graph.
What makes a wrong kernel fail is asserted from the numpy reference alone before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from tests import topk_ref as ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A
DEGREES = [0, 1, 2, 24, 25, 26, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 70001]
ALL_DEAD, ALL_ZERO, EQUAL_SHORT, EQUAL_LONG = 16, 17, 18, 19      # rows behind those of DEGREES
EXTRA = {ALL_DEAD: 40, ALL_ZERO: 40, EQUAL_SHORT: 300, EQUAL_LONG: 20000}
KS = [1, 2, 5, 25, 63, 64]
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 3.4028234663852886e38, -3.4028234663852886e38, 1.1754942e-38],
                    dtype=np.float32)
NAMES = ("src", "eid", "count")


def hand_graph():
    """(indptr, col, w): the rows of DEGREES, then the four special rows."""
    rng = np.random.RandomState(2024)
    deg = np.array(DEGREES + [EXTRA[r] for r in sorted(EXTRA)], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E, N = int(indptr[-1]), deg.size
    col = rng.randint(0, N, E).astype(np.int32)
    col[rng.rand(E) < 0.03] = -1
    w = (rng.randint(-8, 33, E) / 8).astype(np.float32)            # eighths: ties everywhere, a fifth of them not positive
    odd = rng.rand(E) < 0.05
    w[odd] = SPECIALS[rng.randint(0, SPECIALS.size, int(odd.sum()))]
    row = lambda r: slice(int(indptr[r]), int(indptr[r + 1]))
    col[row(ALL_DEAD)] = -1
    w[row(ALL_ZERO)] = np.where(np.arange(EXTRA[ALL_ZERO]) % 2 == 0, 0.0, -0.0).astype(np.float32)
    col[row(ALL_ZERO)] = 3
    w[row(EQUAL_SHORT)] = 1.0
    w[row(EQUAL_LONG)] = 0.375
    col[indptr[EQUAL_SHORT] + 3] = col[indptr[EQUAL_LONG] + 7] = -1      # a dead entry among the first of the equal rows
    return indptr, col, w


def row_list(N):
    """Every row, -1, node_num, and rows again at other positions (the two hubs among them)."""
    return np.concatenate([np.arange(N), [-1, N, 15, 3, 14, 15, 0, -5, N + 9], np.arange(N)[::-1]]).astype(np.int32)


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    indptr, col, w = hand_graph()
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    d_w = torch.from_numpy(w).to(DEV)
    ones = torch.ones(col.size, dtype=torch.float32, device=DEV)
    yield dict(graph=graph, indptr=indptr, col=col, w=w, d_w=d_w, ones=ones, L=hip)
    torch.cuda.synchronize()
    graph.close()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def abi(L, graph, rows, k, mode, d_w, salt, with_eids=True, with_count=True, stream=None):
    """legion_row_topk over sentinel-filled buffers with 8 spare entries and a scratch with 8 spare words: (src [n, k], eid or None,
    count or None); the tails are checked untouched."""
    n = rows.size
    d_rows = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    s = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    nbytes = int(L.legion_row_topk_scratch_bytes(n))
    assert nbytes == ref.scratch_bytes(n) == 4 * (n + 1)
    scratch = torch.full((n + 1 + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    src = torch.full((n * k + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    eid = torch.full((n * k + 8,), SENTINEL, dtype=torch.int64, device=DEV) if with_eids else None
    cnt = torch.full((n + 8,), SENTINEL, dtype=torch.int32, device=DEV) if with_count else None
    assert L.legion_row_topk(s, graph.handle, P(d_rows), n, k, mode, P(d_w), salt, P(src), P(eid), P(cnt), P(scratch), nbytes) == 0
    torch.cuda.synchronize()
    assert bool((scratch[n + 1:] == SENTINEL).all()), "written past the scratch"
    out = []
    for x, size, shape in ((src, n * k, (n, k)), (eid, n * k, (n, k)), (cnt, n, (n,))):
        if x is None:
            out.append(None)
            continue
        x = x.cpu().numpy()
        assert np.all(x[size:] == SENTINEL), "written past the output"
        out.append(x[:size].reshape(shape))
    return out


def compare(got, want, ctx):
    for name, g, w in zip(NAMES, got, want):
        if g is not None:
            same_arrays(g, w, ctx, names=[name])


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
def test_the_inputs_hold_their_conditions_before_any_launch(world):
    indptr, col, w = world["indptr"], world["col"], world["w"]
    deg = np.diff(indptr)
    assert deg[:16].tolist() == DEGREES and {ref.LONG - 1, ref.LONG, ref.LONG + 1} <= set(deg.tolist()) and deg.max() > 16 * ref.LONG
    assert (deg > ref.LONG).sum() == 3, "three rows of the workgroup class"
    for x in SPECIALS:
        assert (w.view(np.uint32) == np.float32(x).view(np.uint32)).sum() >= 10, x
    assert (col < 0).sum() >= 1000
    N = deg.size
    rows = row_list(N)
    for mode in ref.MODES:
        src, eid, cnt = ref.row_topk(indptr, col, w, rows, 64, mode, 7)
        assert cnt[ALL_DEAD] == 0 and cnt[0] == 0 and cnt[N] == 0 and cnt[N + 1] == 0 and cnt[15] == 64
        assert (cnt[ALL_ZERO] == 0) == (mode == ref.SAMPLE), "zero weights: never sampled, all equal in a top-k"
        assert cnt[3] <= 24 and cnt[12] == 64
        assert np.array_equal(src[15], src[N + 2]) and np.array_equal(eid[15], eid[N + 2])
        big = eid[15] - indptr[15]
        if mode == ref.SAMPLE:
            assert big.max() > 60000 and big.min() < 10000, "the hub's picks come from all over the row"
        else:
            assert big.max() > 64 * 20, "the hub's picks come from many steps"
    for r in (EQUAL_SHORT, EQUAL_LONG):
        at = np.arange(indptr[r], indptr[r + 1])
        live = at[col[at] >= 0]
        for mode in (ref.LARGEST, ref.SMALLEST):
            assert np.array_equal(ref.row_topk(indptr, col, w, [r], 25, mode, 0)[1][0], live[:25]), "equal weights: the first k live entries"
        assert live[0] != at[0] or live[24] != at[24], "a dead entry among the first"
    # ties inside the picks: the smaller position wins
    for mode in (ref.LARGEST, ref.SMALLEST):
        eid = ref.row_topk(indptr, col, w, [15], 5, mode, 0)[1][0]
        key = ref.keys(mode, eid, col[eid], w[eid], 0)[0]
        assert (np.diff(key.astype(np.int64)) == 0).any(), "a tie inside the picks"


# ---- the keys -----------------------------------------------------------------------------------------------------------------------
def keys_abi(L, graph, eids, mode, d_w, salt):
    n = eids.size
    d_e = torch.from_numpy(eids).to(DEV)
    key = torch.full((n + 8,), SENTINEL, dtype=torch.int64, device=DEV)
    ok = torch.full((n + 8,), 0x5A, dtype=torch.uint8, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.legion_topk_keys(s, graph.handle, P(d_e), n, mode, P(d_w), salt, P(key), P(ok)) == 0
    torch.cuda.synchronize()
    assert bool((key[n:] == SENTINEL).all()) and bool((ok[n:] == 0x5A).all()), "written past the output"
    return key[:n].cpu().numpy().view(np.uint64), ok[:n].cpu().numpy()


def test_the_keys_are_the_references_to_the_last_bit(world):
    indptr, col, w, g, L = world["indptr"], world["col"], world["w"], world["graph"], world["L"]
    E = col.size
    special = np.nonzero(np.isin(w.view(np.uint32), SPECIALS.view(np.uint32)))[0]
    eids = np.concatenate([np.arange(100_000), special, [-1, E, E + 5, 2 ** 40, -2 ** 63]]).astype(np.int64)
    inside = (eids >= 0) & (eids < E)
    at = eids[inside]
    for mode in ref.MODES:
        for salt, d_w, ww in ((0, world["d_w"], w), (-3, world["d_w"], w), (2 ** 63 - 1, None, None), (12345, world["ones"], np.ones(E, np.float32))):
            if d_w is None and mode != ref.SAMPLE:
                continue
            want_key = np.full(eids.size, ref.NO_KEY, dtype=np.uint64)
            want_ok = np.zeros(eids.size, dtype=np.uint8)
            k, ok = ref.keys(mode, at, col[at], None if ww is None else ww[at], salt)
            want_key[inside], want_ok[inside] = k, ok
            assert 0 < want_ok.sum() < inside.sum()
            got_key, got_ok = keys_abi(L, g, eids, mode, d_w, salt)
            same_arrays(got_ok, want_ok, f"mode {mode} salt {salt}: eligible")
            bad = np.nonzero(got_key != want_key)[0]
            assert bad.size == 0, (f"mode {mode} salt {salt}: {bad.size} keys differ, first at e = {eids[bad[0]]}: got {got_key[bad[0]]:016x} "
                                   f"want {want_key[bad[0]]:016x} (a fused multiply-add, or a division that is not IEEE's)")


# ---- bit for bit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ref.MODES, ids=["largest", "smallest", "sample"])
@pytest.mark.parametrize("k", KS)
def test_row_topk_is_the_reference_bit_for_bit(world, k, mode):
    indptr, col, w, g = world["indptr"], world["col"], world["w"], world["graph"]
    rows = row_list(indptr.size - 1)
    for salt in (0, -1) if mode == ref.SAMPLE else (0,):
        want = ref.row_topk(indptr, col, w, rows, k, mode, salt)
        assert np.all((want[0] >= 0) == (np.arange(k)[None, :] < want[2][:, None]))
        for with_eids, with_count in ((True, True), (False, False), (True, False)):
            got = abi(world["L"], g, rows, k, mode, world["d_w"], salt, with_eids, with_count)
            compare(got, want, f"k {k} mode {mode} salt {salt} eids {with_eids} count {with_count}")


def test_no_weights_are_unit_weights(world):
    indptr, col, g = world["indptr"], world["col"], world["graph"]
    rows = row_list(indptr.size - 1)
    for k in (5, 64):
        want = ref.row_topk(indptr, col, None, rows, k, ref.SAMPLE, 11)
        assert want[2][ALL_ZERO] == min(k, EXTRA[ALL_ZERO]), "without weights the zero-weight row is sampled"
        compare(abi(world["L"], g, rows, k, ref.SAMPLE, None, 11), want, f"no weights, k {k}")
        compare(abi(world["L"], g, rows, k, ref.SAMPLE, world["ones"], 11), want, f"unit weights, k {k}")


def test_no_rows(world):
    got = abi(world["L"], world["graph"], np.zeros(0, np.int32), 5, ref.SAMPLE, None, 0)
    assert got[0].shape == (0, 5) and got[2].shape == (0,)


# ---- streams and graphs ---------------------------------------------------------------------------------------------------------------
def test_another_stream_and_a_captured_graph(world):
    indptr, col, w, g, L = world["indptr"], world["col"], world["w"], world["graph"], world["L"]
    rows = row_list(indptr.size - 1)
    n, k = rows.size, 25
    want = ref.row_topk(indptr, col, w, rows, k, ref.SAMPLE, 5)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    compare(abi(L, g, rows, k, ref.SAMPLE, world["d_w"], 5, stream=s), want, "another stream")

    d_rows = torch.from_numpy(rows).to(DEV)
    nbytes = int(L.legion_row_topk_scratch_bytes(n))
    scratch = torch.zeros(nbytes // 4, dtype=torch.int32, device=DEV)
    src = torch.zeros(n * k, dtype=torch.int32, device=DEV)
    eid = torch.zeros(n * k, dtype=torch.int64, device=DEV)
    cnt = torch.zeros(n, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cs = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = L.legion_row_topk(cs, g.handle, P(d_rows), n, k, ref.SAMPLE, P(world["d_w"]), 5, P(src), P(eid), P(cnt), P(scratch), nbytes)
    assert rc == 0
    for _ in range(2):
        for x in (scratch, src, eid, cnt):
            x.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        compare((src.reshape(n, k), eid.reshape(n, k), cnt), want, "captured")


# ---- the C ABI's refusals -----------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_leave_the_outputs_untouched(world):
    L, g = world["L"], world["graph"].handle
    n, k = 8, 4
    rows = torch.arange(n, dtype=torch.int32, device=DEV)
    scratch = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=DEV)
    src = torch.full((n * k,), SENTINEL, dtype=torch.int32, device=DEV)
    eid = torch.full((n * k,), SENTINEL, dtype=torch.int64, device=DEV)
    cnt = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    key = torch.full((n,), SENTINEL, dtype=torch.int64, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for bad_n, size in ((0, 4), (1, 8), (2 ** 20, 4 * 2 ** 20 + 4), (2 ** 20 + 1, -1), (-1, -1)):
        assert L.legion_row_topk_scratch_bytes(bad_n) == size == ref.scratch_bytes(bad_n)
    ok = dict(graph=g, rows=P(rows), n=n, k=k, mode=0, w=P(world["d_w"]), salt=0, src=P(src), eid=P(eid), cnt=P(cnt), scratch=P(scratch), bytes=36)
    for change in (dict(n=-1), dict(n=2 ** 20 + 1, bytes=1 << 40), dict(k=0), dict(k=-1), dict(k=65), dict(mode=-1), dict(mode=3), dict(w=None),
                   dict(w=None, mode=1), dict(graph=None), dict(rows=None), dict(src=None), dict(scratch=None), dict(bytes=35), dict(bytes=0),
                   dict(bytes=-1)):
        a = dict(ok, **change)
        assert None in (a["graph"], a["rows"], a["src"], a["scratch"]) or ref.refused(a["n"], a["k"], a["mode"], a["w"] is not None, a["bytes"]), change
        assert L.legion_row_topk(s, a["graph"], a["rows"], a["n"], a["k"], a["mode"], a["w"], a["salt"], a["src"], a["eid"], a["cnt"], a["scratch"],
                                 a["bytes"]) == -1, change
    eids = torch.arange(n, dtype=torch.int64, device=DEV)
    okb = torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)
    for args in ((g, P(eids), -1, 0, P(world["d_w"]), 0, P(key), P(okb)), (g, P(eids), 2 ** 31, 0, P(world["d_w"]), 0, P(key), P(okb)),
                 (g, P(eids), n, 3, P(world["d_w"]), 0, P(key), P(okb)), (g, P(eids), n, 0, None, 0, P(key), P(okb)),
                 (None, P(eids), n, 0, P(world["d_w"]), 0, P(key), P(okb)), (g, None, n, 0, P(world["d_w"]), 0, P(key), P(okb)),
                 (g, P(eids), n, 0, P(world["d_w"]), 0, None, P(okb)), (g, P(eids), n, 0, P(world["d_w"]), 0, P(key), None)):
        assert L.legion_topk_keys(s, *args) == -1, args
    assert L.legion_row_topk(s, g, P(rows), 0, k, 2, None, 0, P(src), P(eid), P(cnt), P(scratch), 4) == 0          # n == 0: nothing runs
    assert L.legion_topk_keys(s, g, P(eids), 0, 2, None, 0, P(key), P(okb)) == 0
    torch.cuda.synchronize()
    for x in (scratch, src, eid, cnt, key):
        assert bool((x == SENTINEL).all()), "a refused call wrote"
    assert bool((okb == 0x5A).all())
