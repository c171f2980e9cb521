"""The per-row selection of the k smallest keys (GraphStorage.select_topk / sample_distinct / sample_distinct_block; the C ABI's
legion_row_topk and legion_topk_keys) restated in numpy on the CPU as the contract in include/legion_hip.h writes it: the hash through
synth.splitmix64_np, the exponential variate E by the contract's formula with np.frexp, one IEEE double operation per numpy operation,
the float ordering and the three keys in integers, and row_topk by np.lexsort per row.  A helper of the tests, not a test file."""
import numpy as np

from legion_amd.synth import splitmix64_np
from tests import link_ref

MAX_ROWS = 2 ** 20                                                 # LEGION_IN_EDGES_MAX_ROWS
MAX_K = 64                                                         # LEGION_TOPK_MAX_K
LARGEST, SMALLEST, SAMPLE = 0, 1, 2
MODES = (LARGEST, SMALLEST, SAMPLE)
LONG = 4096                                                        # LG_TOPK_LONG: rows above it get a workgroup
GRID_ROWS = 2048 * 4                                               # LG_TOPK_GRID workgroups of four waves: rows of one trip
LONG_GRID = 256                                                    # LG_TOPK_LONG_GRID
NO_KEY = np.uint64(2 ** 64 - 1)
SQ = 0.7071067811865476
LN2 = 0.6931471805599453
C = [np.float64(1.0) / np.float64(2 * t + 1) for t in range(11)]


def u64(x):
    return int(x) & (2 ** 64 - 1)


def salt_key(salt, raw_key=False):
    """labor_key(salt); an int64 array of salts gives a uint64 array (to broadcast against the positions)."""
    if isinstance(salt, np.ndarray):
        raw = salt.astype(np.int64).view(np.uint64)
        return raw if raw_key else splitmix64_np(raw)
    return np.uint64(u64(salt) if raw_key else int(splitmix64_np(np.uint64(u64(salt)))))


def exp_of_hash(x, fold=True, terms=11):
    """E from hashed uint64 values x: float64, the contract's operations one by one."""
    x = np.asarray(x, dtype=np.uint64)
    j = x >> np.uint64(12)
    u = (j * np.uint64(2) + np.uint64(1)).astype(np.float64) * np.float64(2.0 ** -53)
    m, ex = np.frexp(u)
    ex = ex.astype(np.int64)
    if fold:
        low = m < SQ
        m = np.where(low, 2.0 * m, m)
        ex = np.where(low, ex - 1, ex)
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = np.full(x.shape, C[terms - 1], dtype=np.float64)
    for t in range(terms - 2, -1, -1):
        p = p * z
        p = p + C[t]
    a = ex.astype(np.float64) * LN2
    b = (2.0 * s) * p
    return -(a + b)


def exp_variate(e, salt, raw_key=False):
    """E(e, salt) for an array of int64 positions e."""
    e = np.asarray(e, dtype=np.int64).astype(np.uint64)
    return exp_of_hash(splitmix64_np(salt_key(salt, raw_key) ^ e))


def float_order(w):
    """The monotone uint32 of float32 weights, -0 taken as +0, in a uint64 array."""
    b = np.ascontiguousarray(np.asarray(w, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    b = np.where(b == 0x80000000, np.uint64(0), b)
    neg = (b & np.uint64(0x80000000)) != 0
    return np.where(neg, b ^ np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))


def keys(mode, e, src, w, salt):
    """(key uint64, eligible bool) of the entries at positions e, with column entries src and weights w (None: all 1, SAMPLE only).  An
    entry that is not eligible has the key NO_KEY."""
    e = np.asarray(e, dtype=np.int64)
    src = np.asarray(src)
    assert mode in MODES and (w is not None or mode == SAMPLE)
    ww = np.ones(e.shape, dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32)
    if mode == SAMPLE:
        ok = (src >= 0) & np.isfinite(ww) & (ww > 0)
        with np.errstate(all="ignore"):
            k = (exp_variate(e, salt) / np.where(ok, ww, np.float32(1.0)).astype(np.float64)).view(np.uint64)
    else:
        ok = (src >= 0) & ~np.isnan(ww)
        o = float_order(ww)
        k = np.uint64(0xFFFFFFFF) - o if mode == LARGEST else o
    return np.where(ok, k, NO_KEY), ok


def row_topk(indptr, col, w, rows, k, mode, salt, add=0):
    """(src int32 [n, k], eid int64 [n, k], count int32 [n]) of legion_row_topk.  add: what turns a position of col here into the true
    edge id (the far-row view): the hash and eid_out take the true one."""
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    n, N = rows.size, indptr.size - 1
    src = np.full((n, k), -1, dtype=np.int32)
    eid = np.full((n, k), -1, dtype=np.int64)
    cnt = np.zeros(n, dtype=np.int32)
    done = {}
    for i, r in enumerate(rows.tolist()):
        if r < 0 or r >= N:
            continue
        if r not in done:
            pos = np.arange(indptr[r], indptr[r + 1], dtype=np.int64)
            key, ok = keys(mode, pos + add, col[pos], None if w is None else w[pos], salt)
            order = np.lexsort((pos, key))                         # by (key, position)
            order = order[ok[order]][:k]
            done[r] = pos[order]
        at = done[r]
        c = at.size
        cnt[i] = c
        src[i, :c] = col[at]
        eid[i, :c] = at + add
    return src, eid, cnt


# ---- the refusals ---------------------------------------------------------------------------------------------------------------------
def scratch_bytes(n):
    return -1 if n < 0 or n > MAX_ROWS else 4 * (n + 1)


def refused(n, k, mode, has_w, scratch=1 << 40):
    if n < 0 or n > MAX_ROWS or k < 1 or k > MAX_K or mode not in MODES or (not has_w and mode != SAMPLE):
        return True
    return scratch < scratch_bytes(n)


# ---- the block --------------------------------------------------------------------------------------------------------------------------
def block(indptr, col, w, seeds, fanout, salt):
    """dict of input_nodes, dst_local, src_local, eids: what GraphStorage.sample_distinct_block returns."""
    seeds = np.asarray(seeds, dtype=np.int32)
    src, eid, cnt = row_topk(indptr, col, w, seeds, fanout, SAMPLE, salt)
    mask = src >= 0
    dst = np.nonzero(mask)[0].astype(np.int32)
    unique, local, c = link_ref.unique_ids(np.concatenate([seeds, src[mask]]))
    n = seeds.size
    assert np.array_equal(local[:n], np.arange(n))
    return dict(input_nodes=unique[:c], dst_local=dst, src_local=local[n:], eids=eid[mask])
