"""The reverse CSR (GraphStorage.reverse / out_degrees / out_edges; the C ABI's legion_graph_build_reverse) restated in numpy on the CPU
as the contract in include/legion_hip.h writes it: a stable argsort of the live column entries, np.bincount and np.cumsum; the row of an
entry is np.searchsorted(side="right") over the row pointers.  The classes and the passes of the sort as legion_amd/csrc/reverse_rule.h
has them, graphs whose reverse rows have chosen lengths, and numpy models of wrong kernels, which must differ from the reference on the
GPU files' own inputs.  A helper of the tests, not a test file."""
import numpy as np

from tests import in_edges_ref

MAX_NODES = 2 ** 28                                                # LEGION_REVERSE_MAX_NODES
WAVE = 64                                                          # LG_REVERSE_WAVE: the longest row a wave sorts
TILE = 4096                                                        # LG_REVERSE_TILE: the longest row, and run, a workgroup sorts
CHUNK = 2048                                                       # LG_REVERSE_CHUNK: the outputs of a merge a workgroup takes
ENTRY_TILE = 1024                                                  # entries a workgroup counts and scatters at a time
ENTRY_STRIDE = 2048 * ENTRY_TILE                                   # entries of one trip of the capped grid
SCAN_ONE = 2 ** 20                                                 # the most vertices one level of the scan takes
T = TILE
CLASS_LENGTHS = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5, 5 * T - 1]


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def live_entries(indptr, col):
    col = np.asarray(col)
    N = len(indptr) - 1
    return np.nonzero((col >= 0) & (col < N))[0].astype(np.int64)


def rows_of(indptr, e):
    """row(e): the v with indptr[v] <= e < indptr[v + 1], -1 where there is none."""
    indptr = np.asarray(indptr, dtype=np.int64)
    v = np.searchsorted(indptr, e, side="right") - 1
    return np.where((v >= 0) & (v < indptr.size - 1), v, -1).astype(np.int32)


def reverse(indptr, col):
    """(rindptr int64 [N + 1], rcol int32 [E'], reid int64 [E'])."""
    indptr, col = np.asarray(indptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
    N = indptr.size - 1
    e = live_entries(indptr, col)
    reid = e[np.argsort(col[e], kind="stable")]                    # by col, then ascending e
    rindptr = np.concatenate([[0], np.cumsum(np.bincount(col[e], minlength=N))]).astype(np.int64)
    return rindptr, rows_of(indptr, reid), reid.astype(np.int64)


def live_graph(indptr, col):
    """The graph without its dead and out-of-graph entries: (indptr, col)."""
    indptr, col = np.asarray(indptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
    e = live_entries(indptr, col)
    keep = np.zeros(col.size + 1, dtype=np.int64)
    keep[e + 1] = 1
    return np.cumsum(keep)[indptr], col[e]


def out_degrees(indptr, col, nodes):
    rindptr, _, _ = reverse(indptr, col)
    return in_edges_ref.degrees(rindptr, nodes)


def out_edges(indptr, col, nodes):
    """(src int32 [M] the index into nodes, dst int32 [M], eid int64 [M] into col): what GraphStorage.out_edges returns."""
    rindptr, rcol, reid = reverse(indptr, col)
    _, i, v, at = in_edges_ref.in_edges_full(rindptr, rcol, np.asarray(nodes, dtype=np.int32))
    return i, v, reid[at]


def refused(have_graph, node_num):
    return not have_graph or node_num > MAX_NODES


# ---- the sort's classes and passes (reverse_rule.h) -----------------------------------------------------------------------------------
def sort_class(length):
    return "none" if length <= 1 else "wave" if length <= WAVE else "tile" if length <= TILE else "long"


def runs(length):
    return -(-length // TILE) if length > 0 else 0


def passes(length):
    p, r = 0, runs(length)
    while r > 1:
        p, r = p + 1, (r + 1) // 2
    return p


def scan_levels(node_num):
    return 0 if node_num <= 0 else 1 if node_num <= SCAN_ONE else 2


def classes_of(rindptr):
    """The set of sort classes among the rows, and the run counts of the long ones."""
    lengths = np.diff(np.asarray(rindptr))
    return {sort_class(int(x)) for x in np.unique(lengths)}, sorted({runs(int(x)) for x in np.unique(lengths) if x > TILE})


# ---- inputs of the tests --------------------------------------------------------------------------------------------------------------
def class_graph(lengths, seed, dead=40, outside=20):
    """(indptr, col) of len(lengths) vertices whose reverse row u has exactly lengths[u] entries.  The entries are shuffled over the
    forward rows in a way fixed by seed, so the order in which a kernel meets the entries of u is not the order of their positions
    alone; `dead` entries are -1 and `outside` ones lie at or past N.  Forward rows are of random lengths, some empty; with far more
    entries than vertex pairs there are parallel edges."""
    lengths = np.asarray(lengths, dtype=np.int64)
    N = lengths.size
    rng = np.random.RandomState(seed)
    col = np.repeat(np.arange(N, dtype=np.int32), lengths)
    extra = np.concatenate([np.full(dead, -1, np.int32), np.array([N, N + 5, 2 ** 31 - 1, N + 1], np.int32)[np.arange(outside) % 4]])
    col = np.concatenate([col, extra])
    col = col[rng.permutation(col.size)]
    row = np.sort(rng.randint(0, N, col.size))                      # the forward row of every entry, non-decreasing
    indptr = np.searchsorted(row, np.arange(N + 1), side="left").astype(np.int64)
    return indptr, col


def class_lengths(extra=27, seed=0):
    """CLASS_LENGTHS shuffled among `extra` short rows: every class boundary, and merges of 2, 3 and 5 runs with a short last run."""
    rng = np.random.RandomState(seed)
    lengths = np.concatenate([CLASS_LENGTHS, rng.randint(0, 9, extra)])
    return lengths[rng.permutation(lengths.size)]


# ---- wrong kernels --------------------------------------------------------------------------------------------------------------------
def _scatter_order(rindptr, rcol, reid, seed):
    """The reverse with every row in an order the atomics could have produced: a fixed shuffle inside each row."""
    rng = np.random.RandomState(seed)
    key = rng.rand(reid.size)
    order = np.lexsort((key, np.repeat(np.arange(rindptr.size - 1), np.diff(rindptr))))
    return rcol[order], reid[order]


def rows_in_scatter_order(indptr, col, seed=1):
    """No sort: reverse rows left as the scatter wrote them."""
    rindptr, rcol, reid = reverse(indptr, col)
    return (rindptr,) + _scatter_order(rindptr, rcol, reid, seed)


def merge_off_by_one(indptr, col, seed=1):
    """Long rows merged with the second run of every first-pass pair starting one entry late: that entry stays behind the pair."""
    rindptr, rcol, reid = reverse(indptr, col)
    rcol, reid = rcol.copy(), reid.copy()
    for u in np.nonzero(np.diff(rindptr) > TILE)[0]:
        s, L = int(rindptr[u]), int(rindptr[u + 1] - rindptr[u])
        for a in range(0, L, 2 * TILE):
            b, c = min(a + TILE, L), min(a + 2 * TILE, L)
            if c - b < 2:
                continue
            late = s + b                                            # the first entry of the second run, in the sorted row: not its largest
            pair_e = np.concatenate([reid[s + a:late], reid[late + 1:s + c], reid[late:late + 1]])
            pair_v = np.concatenate([rcol[s + a:late], rcol[late + 1:s + c], rcol[late:late + 1]])
            reid[s + a:s + c], rcol[s + a:s + c] = pair_e, pair_v
    return rindptr, rcol, reid


def dead_kept(indptr, col):
    """Dead entries counted as entries of the last vertex (an index of -1 wraps)."""
    col = np.asarray(col, dtype=np.int32)
    N = len(indptr) - 1
    return reverse(indptr, np.where(col == -1, N - 1, col).astype(np.int32))


def e32(rindptr, rcol, reid):
    """e formed in 32 bits."""
    return rindptr, rcol, ((reid + 2 ** 31) % 2 ** 32) - 2 ** 31


def stale_second_trip(indptr, col, stride=ENTRY_STRIDE):
    """A second grid trip that counts and scatters the tiles one stride earlier again: the entries past the stride never arrive, those
    of the first trip arrive twice."""
    col = np.asarray(col, dtype=np.int32)
    twice = col.copy()
    twice[stride:] = col[:col.size - stride]
    return reverse(indptr, twice)


def counts_int32(rindptr):
    """Row starts kept in int32."""
    return (((np.asarray(rindptr) + 2 ** 31) % 2 ** 32) - 2 ** 31).astype(np.int64)
