"""GraphStorage.select_topk, sample_distinct and sample_distinct_block through Python, against tests/topk_ref.py followed by
link_ref.unique_ids: the symmetric graph of tests/node2vec_ref.py (6 000 vertices, hubs up to 4 097 entries, dead entries, empty rows)
with weights in eighths, rows from the host and from the device, with and without edge ids, another stream; the ValueErrors, each raised
before anything touches a device; and a block's input_nodes handed to FeatureStorage.set_ids."""
import numpy as np
import pytest
import torch

from tests import node2vec_ref
from tests import topk_ref as ref
from tests.compare import same_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = node2vec_ref.NODE_NUM


@pytest.fixture(scope="module")
def world(hip):
    from legion_amd import engine
    indptr, col, w = node2vec_ref.sym_graph()
    w = w.astype(np.float32)
    graph = engine.GraphStorage(1, torch.from_numpy(indptr).to(DEV), torch.from_numpy(col).to(DEV))
    yield dict(graph=graph, indptr=indptr, col=col, w=w, L=hip)
    torch.cuda.synchronize()
    graph.close()


def test_select_topk_and_sample_distinct(world):
    indptr, col, w, g = world["indptr"], world["col"], world["w"], world["graph"]
    rows = np.concatenate([node2vec_ref.seeds_for(257), [-1, N, 6, 6]]).astype(np.int32)
    d_rows = torch.from_numpy(rows).to(DEV)
    for k in (1, 10, 64):
        for ascending in (False, True):
            src, eid, cnt = ref.row_topk(indptr, col, w, rows, k, ref.SMALLEST if ascending else ref.LARGEST, 0)
            got = g.select_topk(rows, k, w, ascending=ascending, return_eids=True)
            torch.cuda.synchronize()
            assert len(got) == 3 and all(x.is_cuda for x in got)
            same_arrays(got, (src, cnt, eid), f"select_topk k {k} ascending {ascending}", names=("src", "counts", "eids"))
            assert len(g.select_topk(d_rows, k, torch.from_numpy(w), ascending=ascending)) == 2
        for salt, weights in ((0, w), (-7, None)):
            src, eid, cnt = ref.row_topk(indptr, col, weights, rows, k, ref.SAMPLE, salt)
            got = g.sample_distinct(d_rows, k, weights=None if weights is None else torch.from_numpy(weights).to(DEV), salt=salt, return_eids=True)
            torch.cuda.synchronize()
            same_arrays(got, (src, cnt, eid), f"sample_distinct k {k} salt {salt}", names=("src", "counts", "eids"))
    assert (cnt == 0).any() and (cnt == 64).any(), "rows without entries and a hub among them"
    s = torch.cuda.Stream()
    got = g.sample_distinct(d_rows, 64, salt=-7, stream=s)
    s.synchronize()
    same_arrays(got, (src, cnt), "another stream", names=("src", "counts"))
    none = g.sample_distinct(np.zeros(0, np.int32), 3, return_eids=True)
    assert [tuple(x.shape) for x in none] == [(0, 3), (0,), (0, 3)]


@pytest.mark.parametrize("eids", [False, True], ids=["no-eids", "eids"])
def test_sample_distinct_block(world, eids):
    from legion_amd import engine
    indptr, col, w, g = world["indptr"], world["col"], world["w"], world["graph"]
    rng = np.random.RandomState(5)
    seeds = np.concatenate([[6, 0, 1], rng.choice(np.arange(7, N), 500, replace=False)]).astype(np.int32)
    for fanout, weights, salt in ((10, w, 3), (25, None, -1)):
        want = ref.block(indptr, col, weights, seeds, fanout, salt)
        assert want["dst_local"].size > seeds.size and want["input_nodes"].size > seeds.size
        got = g.sample_distinct_block(seeds, fanout, weights=weights, salt=salt, return_eids=eids)
        torch.cuda.synchronize()
        assert len(got) == (4 if eids else 3)
        same_arrays(got, [want[key] for key in ("input_nodes", "dst_local", "src_local", "eids")][:len(got)], f"block fanout {fanout}",
                    names=("input_nodes", "dst_local", "src_local", "eids"))
    # the block's input nodes are a seed set of the feature side
    feats = torch.zeros((N, 4), dtype=torch.float32, device=DEV)
    fs = engine.FeatureStorage(1, feats)
    try:
        ids = got[0].cpu().numpy()
        assert ids.dtype == np.int32 and ids.min() >= 0 and ids.max() < N and np.unique(ids).size == ids.size
        fs.set_ids(0, engine.TRAINMODE, ids, np.zeros(ids.size, np.int32))
    finally:
        fs.close()


def test_value_errors_come_before_any_device_work(world):
    g, w = world["graph"], world["w"]
    rows = np.arange(4, dtype=np.int32)
    bad_w = [np.ones(3, np.float32), w.astype(np.float64), torch.ones((2, 2)), [1.0] * w.size, None]
    for weights in bad_w:
        with pytest.raises(ValueError):
            g.select_topk(rows, 2, weights)
    for weights in bad_w[:-1]:
        with pytest.raises(ValueError):
            g.sample_distinct(rows, 2, weights=weights)
        with pytest.raises(ValueError):
            g.sample_distinct_block(rows, 2, weights=weights)
    for k in (0, -1, 65, 2.0, True, None):
        with pytest.raises(ValueError):
            g.select_topk(rows, k, w)
        with pytest.raises(ValueError):
            g.sample_distinct(rows, k)
        with pytest.raises(ValueError):
            g.sample_distinct_block(rows, k)
    for kwargs in (dict(salt=2 ** 63), dict(salt=-2 ** 63 - 1), dict(salt=1.5), dict(return_eids=1)):
        with pytest.raises(ValueError):
            g.sample_distinct(rows, 2, **kwargs)
        with pytest.raises(ValueError):
            g.sample_distinct_block(rows, 2, **kwargs)
    for kwargs in (dict(ascending=1), dict(return_eids=None)):
        with pytest.raises(ValueError):
            g.select_topk(rows, 2, w, **kwargs)
    with pytest.raises(ValueError):
        g.select_topk(torch.zeros(3, dtype=torch.int64), 2, w)
    with pytest.raises(ValueError):
        g.sample_distinct(torch.zeros((2, 2), dtype=torch.int32), 2)
    for seeds in ([1, 1, 2], [0, N], [-1, 3]):
        with pytest.raises(ValueError):
            g.sample_distinct_block(np.array(seeds, dtype=np.int32), 2)
    with pytest.raises(ValueError):
        g.sample_distinct_block(np.arange(2 ** 14 + 1, dtype=np.int32) % N, 64)      # 2^14 + 1 seeds x 65 ids: past UNIQUE_MAX_IDS
