"""Host-side Python mirror of the reference's operator interface for the hot path.

Same names and argument meaning as the reference (SS = sampling_server/src):
  BatchGenerate / RandomSample / FeatureCacheLookup / IOSubmit / IOComplete
                                         SS/engine/operator_impl.cuh:11-63
  GraphStorage / FeatureStorage          SS/storage/graph_storage.cuh:7-24, feature_storage.cuh:6-34
  MemoryPool                             SS/engine/memorypool.cuh:20-221
  UnifiedCache                           SS/cache/cache.cuh:66-177
Everything computes inside liblegion_hip.so (HIP kernels for gfx950) through the C ABI in
include/legion_hip.h; PyTorch is used only to own device memory, streams and torch.distributed.
There is no CPU path: constructing any of these without a GPU-backed library raises.
"""
import ctypes

import numpy as np
import torch

from . import lib as _libmod

INTERBATCH_CON = 2
INTRABATCH_CON = 3
TRAINMODE, VALIDMODE, TESTMODE = 0, 1, 2
CACHEMISS_FLAG = -2

_TYPESTR = {torch.int32: "<i4", torch.int64: "<i8", torch.float32: "<f4", torch.int8: "|i1",
            torch.uint8: "|u1", torch.int16: "<i2"}


class _RawDevice:
    def __init__(self, ptr, shape, dtype):
        self.__cuda_array_interface__ = {
            "shape": tuple(int(s) for s in shape), "typestr": _TYPESTR[dtype],
            "data": (int(ptr), False), "version": 2, "strides": None}


def device_view(ptr, shape, dtype, device):
    """Zero-copy torch view of raw device memory owned by the library."""
    n = 1
    for s in shape:
        n *= int(s)
    if not ptr or n == 0:
        return torch.empty(tuple(shape), dtype=dtype, device=device)
    if dtype == torch.bfloat16:      # (no typestr for bfloat16 in the array interface: its bits as int16)
        return torch.as_tensor(_RawDevice(ptr, shape, torch.int16), device=device).view(torch.bfloat16)
    return torch.as_tensor(_RawDevice(ptr, shape, dtype), device=device)


def set_device_base(base):
    """One process per GPU: this process's logical GPU 0 is physical GPU `base` (LOCAL_RANK)."""
    _libmod.load().legion_set_device_base(int(base))


def set_local_device(dev):
    """A clique spread over processes: this process owns logical GPU `dev` only (dev = its rank)."""
    _libmod.load().legion_set_local_device(int(dev))


def link_counters(dev_id=0):
    """(PCIe bytes, xGMI bytes) moved by logical GPU dev_id since boot, from the driver's gpu_metrics table, or None
    when the table is not readable / has an unknown revision (legion_hip.h: legion_link_counters)."""
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    ok = _libmod.load().legion_link_counters(int(dev_id), ctypes.byref(a), ctypes.byref(b))
    return (int(a.value), int(b.value)) if ok else None


def link_counters_ex(dev_id=0, source=0):
    """The whole table as a dict (legion_hip.h: LegionLinkCounters) plus 'supported': PCIe bytes, xGMI bytes read / written
    in total and per link, the gpu_metrics revision found, the GPU's PCI bus id and which decoder produced the numbers
    (source: 0 = rocm_smi_lib's versioned decoder first, the byte-offset parser second; 1 / 2 = that one only)."""
    c = _libmod.LinkCounters()
    ok = _libmod.load().legion_link_counters_from(int(dev_id), int(source), ctypes.byref(c))
    return {"supported": bool(ok), "source": {0: None, 1: "rocm_smi_lib", 2: "sysfs gpu_metrics by offset"}.get(int(c.source)), "pcie_bytes": int(c.pcie_bytes), "xgmi_read_bytes": int(c.xgmi_read_bytes),
            "xgmi_write_bytes": int(c.xgmi_write_bytes), "xgmi_read_bytes_link": [int(x) for x in c.xgmi_read_bytes_link],
            "xgmi_write_bytes_link": [int(x) for x in c.xgmi_write_bytes_link],
            "gpu_metrics_revision": f"{int(c.format_revision)}.{int(c.content_revision)}",
            "pci_bus_id": c.pci_bus_id.decode(errors="replace")}


def tuning():
    """The library's current LegionTuning as a dict."""
    t = _libmod.Tuning()
    _libmod.load().legion_tuning_get(ctypes.byref(t))
    return {n: (list(getattr(t, n)) if n == "link_counter_values" else int(getattr(t, n))) for n, _ in t._fields_}


def set_tuning(**fields):
    """Installs programmatic tuning values (kept until tuning_from_env() is called): set_tuning(runner_lanes=4, ...)."""
    t = _libmod.Tuning()
    L = _libmod.load()
    L.legion_tuning_get(ctypes.byref(t))
    for k, v in fields.items():
        if k == "link_counter_values":
            t.link_counter_values[0], t.link_counter_values[1] = int(v[0]), int(v[1])
        else:
            if not hasattr(t, k):
                raise KeyError(k)
            setattr(t, k, int(v))
    L.legion_tuning_set(ctypes.byref(t))


def tuning_from_env():
    _libmod.load().legion_tuning_from_env()


def _torch_device(dev_id):
    base = int(_libmod.load().legion_get_device_base())
    return torch.device("cuda", (base + int(dev_id)) % max(torch.cuda.device_count(), 1))


class PinnedArray:
    """A numpy-visible array in mapped pinned host memory that the GPU reads in place over PCIe: the
    spill-over tier for tables that do not fit HBM (the reference's only tier for the full CSR/features)."""

    def __init__(self, array):
        array = np.ascontiguousarray(array)
        self._lib = _libmod.load()
        host = ctypes.c_void_p()
        self.dev_ptr = self._lib.legion_host_alloc(int(array.nbytes), ctypes.byref(host))
        self.host_ptr = host.value
        self.shape, self.dtype = array.shape, array.dtype
        ctypes.memmove(self.host_ptr, array.ctypes.data, array.nbytes)

    @classmethod
    def empty(cls, shape, dtype):
        """Uninitialised mapped pinned array (fill it through .tensor(device) or .numpy())."""
        self = cls.__new__(cls)
        self._lib = _libmod.load()
        self.shape, self.dtype = tuple(int(s) for s in shape), np.dtype(dtype)
        nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        host = ctypes.c_void_p()
        self.dev_ptr = self._lib.legion_host_alloc(nbytes, ctypes.byref(host))
        self.host_ptr = host.value
        return self

    def numpy(self):
        n = int(np.prod(self.shape, dtype=np.int64))
        buf = (ctypes.c_char * (n * self.dtype.itemsize)).from_address(self.host_ptr)
        return np.frombuffer(buf, dtype=self.dtype, count=n).reshape(self.shape)

    def tensor(self, device):
        tdt = {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.float32): torch.float32}[self.dtype]
        return device_view(self.dev_ptr, self.shape, tdt, device)

    def close(self):
        if self.host_ptr:
            self._lib.legion_host_free(ctypes.c_void_p(self.host_ptr))
            self.host_ptr = None


def _stream_handle(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _i32_array(values):
    arr = (ctypes.c_int32 * len(values))(*[int(v) for v in values])
    return arr


def _as_1d(x, dtype, name):
    """x as a one-dimensional tensor of dtype: a tensor of another dtype or shape is a ValueError, anything else goes through
    torch.as_tensor."""
    short = str(dtype).replace("torch.", "")
    if isinstance(x, torch.Tensor) and x.dtype != dtype:
        raise ValueError(f"{name} must be {short}, not {x.dtype}")
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(x, dtype=dtype)
    if x.dim() != 1:
        raise ValueError(f"{name} must be one-dimensional, not shape {tuple(x.shape)}")
    return x


def _need_bool(name, flag):
    if not isinstance(flag, bool):
        raise ValueError(f"{name} must be True or False, not {flag!r}")


def _need_int(name, value):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, not {value!r}")


def _need_prob(name, value):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.floating, np.integer)):
        raise ValueError(f"{name} must be a number in [0, 1], not {value!r}")
    if not 0.0 <= float(np.float32(value)) <= 1.0:       # (NaN fails; the library sees the float32)
        raise ValueError(f"{name} must lie in [0, 1], not {value!r}")


def _need_draw_indices(base, count, what):
    """The draw indices base .. base + count - 1 (count spelled `what`) exist: the last one is 2^31 - 2."""
    if base < 0:
        raise ValueError(f"base must not be negative, not {base}")
    if base + count > 2 ** 31 - 1:
        raise ValueError(f"base + {what} = {base + count} is past the last draw index, 2^31 - 1")


def _enqueue(lib, c_name, op, dev, stream, args, tensors):
    """The tail of every op over the graph: the C call on dev with `stream` (default: the current one) in front of args, a refusal the
    op's own checks should have caught as a RuntimeError, and the call's tensors (None: not used) recorded on a stream that is not the
    allocator's."""
    with torch.cuda.device(dev):
        rc = getattr(lib, c_name)(_stream_handle(stream), *args)
    if rc != 0:
        raise RuntimeError(f"{c_name} refused arguments that {op} had accepted")
    if stream is not None:
        for x in tensors:
            if x is not None:
                x.record_stream(stream)


UNIQUE_MAX_IDS = 2 ** 20                             # LEGION_UNIQUE_MAX_IDS


def _check_unique(m):
    if m > UNIQUE_MAX_IDS:
        raise ValueError(f"{m} ids in one call, at most {UNIQUE_MAX_IDS}")


def _read_scalar(x, stream):
    """The one-element device tensor x as an int, read under `stream` (None: the current one): it synchronises that stream."""
    if stream is None:
        return int(x.item())
    with torch.cuda.stream(stream):
        return int(x.item())


def unique_ids(ids, stream=None):
    """The distinct ids in order of first appearance, and where each id sits among them (compact_graphs' relabelling; the rule:
    legion_unique_ids in legion_hip.h).  ids: int32, a CUDA tensor (its device is used) or anything torch.as_tensor takes (the current
    device); at most UNIQUE_MAX_IDS of them.  Returns (unique, local, count): unique int32 [m], the distinct non-negative ids and -1
    from count on; local int32 [m], each id's index in unique, -1 for a negative id; count, a one-element int32 device tensor (no
    sync).  The scratch is allocated here.  Enqueued on `stream` (default: the current one)."""
    ids = _as_1d(ids, torch.int32, "ids")
    m = int(ids.numel())
    _check_unique(m)
    L = _libmod.load()
    dev = ids.device if ids.is_cuda else torch.device("cuda", torch.cuda.current_device())
    ids = ids.to(dev).contiguous()
    unique = torch.empty((m,), dtype=torch.int32, device=dev)
    local = torch.empty((m,), dtype=torch.int32, device=dev)
    if m == 0:                                       # (nothing to enqueue; an empty tensor has no address to hand over)
        return unique, local, torch.zeros((1,), dtype=torch.int32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    nbytes = int(L.legion_unique_ids_scratch_bytes(m))
    scratch = torch.empty((nbytes // 4,), dtype=torch.int32, device=dev)
    _enqueue(L, "legion_unique_ids", "unique_ids", dev, stream,
             (_ptr(ids), m, _ptr(unique), _ptr(local), _ptr(count), _ptr(scratch), nbytes), (ids, unique, local, count, scratch))
    return unique, local, count


NODE_SET_MAX_IDS = 2 ** 20                           # LEGION_NODE_SET_MAX_IDS


class NodeSet:
    """A vertex set on the device (the rule: legion_node_set_build / legion_node_set_lookup in legion_hip.h): an open-addressing table
    that answers pos(v) = the first position of v in nodes, -1 for a negative v and for one that does not occur.  nodes: int32, a CUDA
    tensor (its device is used) or anything torch.as_tensor takes (`device`, default: the current one); at most NODE_SET_MAX_IDS of
    them (ValueError before anything touches a device); they may repeat, negative entries are members of nothing, and ids past any
    graph are legal.  .nodes: the nodes on the device; .k: their number; .distinct: the number of distinct non-negative values, a
    one-element int32 device tensor (no sync).  The table is built on `stream` (default: the current one); a set is what
    GraphStorage.induced_edges and node_subgraph take, and may be used any number of times."""

    def __init__(self, nodes, device=None, stream=None):
        nodes = _as_1d(nodes, torch.int32, "nodes")
        k = int(nodes.numel())
        if k > NODE_SET_MAX_IDS:
            raise ValueError(f"{k} nodes in one set, at most {NODE_SET_MAX_IDS}")
        self._lib = _libmod.load()
        if nodes.is_cuda:
            dev = nodes.device
        else:
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.nodes = nodes.to(dev).contiguous()
        self.k = k
        self.set_bytes = int(self._lib.legion_node_set_bytes(k))
        self.table = torch.empty((self.set_bytes // 4,), dtype=torch.int32, device=dev)
        self.distinct = torch.empty((1,), dtype=torch.int32, device=dev)
        src = self.nodes if k > 0 else self.distinct          # (an empty tensor has no address to hand over; k == 0 reads nothing)
        _enqueue(self._lib, "legion_node_set_build", "NodeSet", dev, stream,
                 (_ptr(src), k, _ptr(self.table), self.set_bytes, _ptr(self.distinct)), (self.nodes, self.table, self.distinct))

    def lookup(self, ids, stream=None):
        """pos(ids[i]) for every i: int32 [m], -1 for a negative id and for a non-member.  ids: int32, a CUDA tensor or anything
        torch.as_tensor takes.  No sync.  Enqueued on `stream` (default: the current one)."""
        ids = _as_1d(ids, torch.int32, "ids")
        m = int(ids.numel())
        ids = ids.to(self.device).contiguous()
        local = torch.empty((m,), dtype=torch.int32, device=self.device)
        if m == 0:                                   # (nothing to enqueue; an empty tensor has no address to hand over)
            return local
        _enqueue(self._lib, "legion_node_set_lookup", "NodeSet.lookup", self.device, stream,
                 (_ptr(self.table), self.set_bytes, self.k, _ptr(ids), m, _ptr(local)), (self.table, ids, local))
        return local


EDGE_SET_MAX_IDS = 2 ** 21                           # LEGION_EDGE_SET_MAX_IDS
EDGE_FILTER_MAX_EDGES = 2 ** 30                      # LEGION_EDGE_FILTER_MAX_EDGES


class EdgeIdSet:
    """A set of edge ids on the device (the rule: legion_edge_set_build / legion_edge_set_contains in legion_hip.h): an
    open-addressing table of int64 keys that answers "is e a member?".  eids: int64 positions in a graph's col, a CUDA tensor (its
    device is used) or anything torch.as_tensor takes (`device`, default: the current one); at most EDGE_SET_MAX_IDS of them
    (ValueError before anything touches a device); they may repeat, and negative entries -- the -1 of an edge without a reverse -- are
    members of nothing.  .eids: the ids on the device; .k: their number.  The table is built on `stream` (default: the current one);
    a set is what exclude_edges and the block ops' exclude_eids take, and may be used any number of times."""

    def __init__(self, eids, device=None, stream=None):
        eids = _as_1d(eids, torch.int64, "eids")
        k = int(eids.numel())
        if k > EDGE_SET_MAX_IDS:
            raise ValueError(f"{k} edge ids in one set, at most {EDGE_SET_MAX_IDS}")
        self._lib = _libmod.load()
        if eids.is_cuda:
            dev = eids.device
        else:
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.eids = eids.to(dev).contiguous()
        self.k = k
        self.set_bytes = int(self._lib.legion_edge_set_bytes(k))
        self.table = torch.empty((self.set_bytes // 8,), dtype=torch.int64, device=dev)
        src = self.eids if k > 0 else self.table             # (an empty tensor has no address to hand over; k == 0 reads nothing)
        _enqueue(self._lib, "legion_edge_set_build", "EdgeIdSet", dev, stream, (_ptr(src), k, _ptr(self.table), self.set_bytes),
                 (self.eids, self.table))

    def contains(self, eids, stream=None):
        """Is eids[i] a member, for every i: int32 [m] of 0 / 1; 0 for a negative id.  eids: int64, a CUDA tensor or anything
        torch.as_tensor takes.  No sync.  Enqueued on `stream` (default: the current one)."""
        eids = _as_1d(eids, torch.int64, "eids")
        m = int(eids.numel())
        eids = eids.to(self.device).contiguous()
        member = torch.empty((m,), dtype=torch.int32, device=self.device)
        if m == 0:                                   # (nothing to enqueue; an empty tensor has no address to hand over)
            return member
        _enqueue(self._lib, "legion_edge_set_contains", "EdgeIdSet.contains", self.device, stream,
                 (_ptr(self.table), self.set_bytes, self.k, _ptr(eids), m, _ptr(member)), (self.table, eids, member))
        return member


def _need_edge_set(edge_set, name="edge_set"):
    if not isinstance(edge_set, EdgeIdSet):
        raise ValueError(f"{name} must be an EdgeIdSet, not {type(edge_set).__name__}")


def _filter_edges(dst, src, eids, edge_set, stream):
    """exclude_edges' work on checked arguments: dst, src, eids on the set's device, contiguous, of one length m <= 2^30.  Returns
    (dst, src, eids, K's device tensor or None)."""
    L, dev, m = edge_set._lib, edge_set.device, int(dst.numel())
    K, count = 0, None
    if m > 0:
        nbytes = int(L.legion_edge_filter_scratch_bytes(m))
        scratch = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
        count = torch.empty((1,), dtype=torch.int64, device=dev)
        head = (_ptr(dst), _ptr(src), _ptr(eids), m, _ptr(edge_set.table), edge_set.set_bytes, edge_set.k)
        _enqueue(L, "legion_edge_filter_count", "exclude_edges", dev, stream, head + (_ptr(count), _ptr(scratch), nbytes),
                 (dst, src, eids, edge_set.table, count, scratch))
        K = _read_scalar(count[0], stream)
    out = (torch.empty((K,), dtype=torch.int32, device=dev), torch.empty((K,), dtype=torch.int32, device=dev),
           torch.empty((K,), dtype=torch.int64, device=dev))
    if K > 0:
        _enqueue(L, "legion_edge_filter_edges", "exclude_edges", dev, stream,
                 head + (_ptr(scratch), nbytes, K, _ptr(out[0]), _ptr(out[1]), _ptr(out[2])), (dst, src, eids, edge_set.table, scratch) + out)
    return out + (count,)


def exclude_edges(dst, src, eids, edge_set, stream=None):
    """An edge list without the edges of a set (DGL's ExcludeCertainEdges after sample_neighbors; the rule: legion_edge_filter_count
    and legion_edge_filter_edges in legion_hip.h).  dst, src: int32 [m]; eids: int64 [m] -- the triples in_edges, labor_edges,
    induced_edges and the block ops return with return_eids, or a pool's agg_dst_ids, agg_src_ids and agg_edge_ids; CUDA tensors or
    anything torch.as_tensor takes; at most EDGE_FILTER_MAX_EDGES entries.  edge_set: an EdgeIdSet (GraphStorage.seed_edge_exclusion
    makes one of a batch's seed edges).  Entry p is kept iff dst[p] >= 0 and eids[p] is no member: the -1 tail of a capacity call
    drops out, a dead entry (src == -1) stays unless its id is excluded.  Returns (dst, src, eids) of the kept entries, in their
    order, sized exactly: the kept number is read back to the host once, so the call synchronises `stream` (default: the current
    one), on which everything is enqueued.  A capturing caller uses the C ABI with a capacity instead."""
    dst = _as_1d(dst, torch.int32, "dst")
    src = _as_1d(src, torch.int32, "src")
    eids = _as_1d(eids, torch.int64, "eids")
    _need_edge_set(edge_set)
    m = int(dst.numel())
    if int(src.numel()) != m or int(eids.numel()) != m:
        raise ValueError(f"dst, src and eids must have one length, not {m}, {int(src.numel())} and {int(eids.numel())}")
    if m > EDGE_FILTER_MAX_EDGES:
        raise ValueError(f"{m} edges in one call, at most {EDGE_FILTER_MAX_EDGES}")
    dev = edge_set.device
    return _filter_edges(dst.to(dev).contiguous(), src.to(dev).contiguous(), eids.to(dev).contiguous(), edge_set, stream)[:3]


class GraphStorage:
    """Full CSR (slot P of the pointer tables) from device tensors: indptr int64[N+1], col int32[E]."""

    def __init__(self, partition_count, indptr, col):
        assert indptr.dtype == torch.int64 and col.dtype == torch.int32
        assert indptr.is_cuda and col.is_cuda and indptr.is_contiguous() and col.is_contiguous()
        self._lib = _libmod.load()
        self.indptr, self.col = indptr, col          # keep alive
        self.partition_count = int(partition_count)
        self.node_num = int(indptr.numel() - 1)
        self.edge_num = int(col.numel())
        self.handle = self._lib.legion_graph_create(self.partition_count, self.node_num, self.edge_num,
                                                    _ptr(indptr), _ptr(col))

    def set_edge_weights(self, weights, stream=None):
        """Per-edge weights for weighted sampling (MemoryPool / Pipeline weighted=True; DGL's prob=): float32[E], aligned with col,
        a torch tensor (any device) or a numpy array.  Builds the graph's per-row prefix-sum table on the current device; a weight
        that is not finite and > 0 counts as 0.  May be called again until a weighted hop has been enqueued (then RuntimeError).
        The build runs on `stream` (default: the current one): synchronise before a Pipeline, which has streams of its own, samples."""
        if isinstance(weights, np.ndarray):
            if weights.dtype != np.float32:
                raise ValueError(f"edge weights must be float32, not {weights.dtype}")
            weights = torch.from_numpy(np.ascontiguousarray(weights))
        if not isinstance(weights, torch.Tensor):
            raise ValueError(f"edge weights must be a float32 tensor or array, not {type(weights).__name__}")
        if weights.dtype != torch.float32:
            raise ValueError(f"edge weights must be float32, not {weights.dtype}")
        if weights.dim() != 1 or weights.numel() != self.edge_num:
            raise ValueError(f"edge weights must have one entry per edge ({self.edge_num}), not shape {tuple(weights.shape)}")
        w = weights.to(self.col.device).contiguous()
        if self._lib.legion_graph_set_edge_weights(self.handle, _stream_handle(stream), _ptr(w)) != 0:
            raise RuntimeError("legion_graph_set_edge_weights: a weighted hop has been enqueued against this graph already")
        self._weights = w                            # (alive until the build has run; replaced by the next call)

    def edge_cdf(self):
        """The prefix-sum table, float32[E] as a device view (indexed like col), or None before set_edge_weights."""
        ptr = self._lib.legion_graph_edge_cdf(self.handle)
        if not ptr:
            return None
        return device_view(ptr, (self.edge_num,), torch.float32, self.col.device)

    @staticmethod
    def _check_walk(n, length, weighted, restart_prob, return_eids, base):
        """random_walk's arguments by the rules of legion_random_walk, before anything touches a device: ValueError with the reason."""
        _need_bool("weighted", weighted)
        _need_bool("return_eids", return_eids)
        _need_int("length", length)
        _need_int("base", base)
        if length < 1:
            raise ValueError(f"length must be at least 1, not {length}")
        _need_draw_indices(base, n * length, "num_walks * length")
        _need_prob("restart_prob", restart_prob)

    def random_walk(self, seeds, length, *, weighted=False, restart_prob=0.0, return_eids=False, base=0, stream=None):
        """Random walks over the full CSR (DGL's dgl.sampling.random_walk; the rule: legion_random_walk in legion_hip.h).  seeds: int32
        vertex ids, a CUDA tensor or anything torch.as_tensor takes; walk w starts at seeds[w] and takes `length` steps.  Returns
        traces, int32 [n, length + 1] with -1 from where a walk ended (no out-edge, a dead column entry, a restart, a seed outside
        the graph), and with return_eids also eids, int64 [n, length], each step's position in col (-1 where the trace is).
        weighted: steps pick by the edge weights (set_edge_weights must have run; the table is fixed afterwards, as after a weighted
        hop).  restart_prob: each step first ends the walk with this probability.  base: draw index of the first walk's first step;
        walks with the same seeds, flags and base are the same walks.  Enqueued on `stream` (default: the current one)."""
        seeds = _as_1d(seeds, torch.int32, "seeds")
        n = int(seeds.numel())
        self._check_walk(n, length, weighted, restart_prob, return_eids, base)
        if weighted and not self._lib.legion_graph_edge_cdf(self.handle):
            raise ValueError("a weighted walk needs the graph's edge weights (set_edge_weights)")
        dev = self.col.device
        seeds = seeds.to(dev).contiguous()
        traces = torch.empty((n, int(length) + 1), dtype=torch.int32, device=dev)
        eids = torch.empty((n, int(length)), dtype=torch.int64, device=dev) if return_eids else None
        if n == 0:                                   # (nothing to enqueue; an empty tensor has no address to hand over)
            return (traces, eids) if return_eids else traces
        _enqueue(self._lib, "legion_random_walk", "random_walk", dev, stream,
                 (self.handle, _ptr(seeds), n, int(length), int(weighted), float(restart_prob), int(base), _ptr(traces), _ptr(eids)),
                 (seeds, traces, eids))
        return (traces, eids) if return_eids else traces

    NODE2VEC_MAX_TRIES = 256                         # LEGION_NODE2VEC_MAX_TRIES
    NODE2VEC_MAX_BIAS = 16                           # LEGION_NODE2VEC_MAX_BIAS

    def rows_sorted(self, stream=None):
        """Are the column entries of every row non-decreasing (as int32: dead entries, -1, first; parallel edges are fine)?  Counted
        on the device at the first call (legion_graph_check_rows_sorted: it synchronises `stream`, default the current one) and
        remembered: node2vec_random_walk searches rows and needs True."""
        if getattr(self, "_rows_sorted", None) is None:
            with torch.cuda.device(self.col.device):
                rc = self._lib.legion_graph_check_rows_sorted(self.handle, _stream_handle(stream))
            if rc not in (0, 1):
                raise RuntimeError("legion_graph_check_rows_sorted refused the graph")
            self._rows_sorted = bool(rc)
        return self._rows_sorted

    @staticmethod
    def _check_node2vec(n, p, q, length, weighted, return_eids, max_tries, base):
        """node2vec_random_walk's arguments by the rules of legion_node2vec_walk, before anything touches a device: ValueError with the
        reason."""
        GraphStorage._check_walk(n, length, weighted, 0.0, return_eids, base)
        _need_int("max_tries", max_tries)
        if not 1 <= max_tries <= GraphStorage.NODE2VEC_MAX_TRIES:
            raise ValueError(f"max_tries must lie in [1, {GraphStorage.NODE2VEC_MAX_TRIES}], not {max_tries}")
        for name, value in (("p", p), ("q", q)):
            if isinstance(value, bool) or not isinstance(value, (int, float, np.floating, np.integer)):
                raise ValueError(f"{name} must be a finite number > 0, not {value!r}")
            with np.errstate(over="ignore"):
                f = float(np.float32(value))             # (the library sees the float32)
            if not (f > 0.0 and np.isfinite(f)):         # (NaN fails)
                raise ValueError(f"{name} must be a finite number > 0, not {value!r}")
        with np.errstate(over="ignore"):
            a, b = 1.0 / float(np.float32(p)), 1.0 / float(np.float32(q))
        if min(a, 1.0, b) * GraphStorage.NODE2VEC_MAX_BIAS < max(a, 1.0, b):
            raise ValueError(f"the bias of p = {p!r}, q = {q!r} is too strong: the largest of 1/p, 1, 1/q may be at most "
                             f"{GraphStorage.NODE2VEC_MAX_BIAS} times the smallest")

    def node2vec_random_walk(self, seeds, p, q, length, *, weighted=False, return_eids=False, max_tries=256, base=0, stream=None):
        """node2vec walks over the full CSR (DGL's dgl.sampling.node2vec_random_walk; the rule: legion_node2vec_walk in legion_hip.h).
        From v, having come from t, a candidate neighbour u is drawn as random_walk draws its step and accepted with probability
        proportional to 1/p if u == t, 1 if u is a neighbour of t, 1/q otherwise; the first step, and the max_tries-th candidate of a
        step, are taken as drawn.  p = q = 1 is random_walk's walk bit for bit.  Needs sorted rows (rows_sorted(), asked here:
        ValueError if not).  seeds, weighted, return_eids, base, stream and what is returned: as in random_walk."""
        seeds = _as_1d(seeds, torch.int32, "seeds")
        n = int(seeds.numel())
        self._check_node2vec(n, p, q, length, weighted, return_eids, max_tries, base)
        if weighted and not self._lib.legion_graph_edge_cdf(self.handle):
            raise ValueError("a weighted walk needs the graph's edge weights (set_edge_weights)")
        if not self.rows_sorted(stream):
            raise ValueError("node2vec_random_walk needs a graph whose rows are sorted (rows_sorted() is False)")
        dev = self.col.device
        seeds = seeds.to(dev).contiguous()
        traces = torch.empty((n, int(length) + 1), dtype=torch.int32, device=dev)
        eids = torch.empty((n, int(length)), dtype=torch.int64, device=dev) if return_eids else None
        if n == 0:                                   # (nothing to enqueue; an empty tensor has no address to hand over)
            return (traces, eids) if return_eids else traces
        _enqueue(self._lib, "legion_node2vec_walk", "node2vec_random_walk", dev, stream,
                 (self.handle, _ptr(seeds), n, int(length), float(p), float(q), int(weighted), int(max_tries), int(base), _ptr(traces),
                  _ptr(eids)), (seeds, traces, eids))
        return (traces, eids) if return_eids else traces

    PINSAGE_MAX_VISITS = 1024                        # LEGION_PINSAGE_MAX_VISITS

    @staticmethod
    def _check_pinsage(n, num_random_walks, walk_length, num_neighbors, termination_prob, weighted, base):
        """pinsage_neighbors' arguments by the rules of legion_pinsage_neighbors, before anything touches a device: ValueError with
        the reason."""
        cap = GraphStorage.PINSAGE_MAX_VISITS
        _need_bool("weighted", weighted)
        for name, value in (("num_random_walks", num_random_walks), ("walk_length", walk_length), ("num_neighbors", num_neighbors),
                            ("base", base)):
            _need_int(name, value)
        for name, value in (("num_random_walks", num_random_walks), ("walk_length", walk_length), ("num_neighbors", num_neighbors)):
            if value < 1:
                raise ValueError(f"{name} must be at least 1, not {value}")
        if num_random_walks * walk_length > cap:
            raise ValueError(f"num_random_walks * walk_length = {num_random_walks * walk_length} visits per seed, at most {cap}")
        if num_neighbors > cap:
            raise ValueError(f"num_neighbors must be at most {cap}, not {num_neighbors}")
        _need_draw_indices(base, n * num_random_walks * walk_length, "num_seeds * num_random_walks * walk_length")
        _need_prob("termination_prob", termination_prob)

    def pinsage_neighbors(self, seeds, num_random_walks, walk_length, num_neighbors, *, termination_prob=0.5, weighted=False, base=0,
                          stream=None):
        """PinSAGE's importance neighbourhoods (DGL's RandomWalkNeighborSampler / PinSAGESampler on a homogeneous graph; the rule:
        legion_pinsage_neighbors in legion_hip.h).  From each seed num_random_walks walks of walk_length steps over the full CSR; after
        its first step a walk ends before each step with termination_prob.  Returns (neighbors, counts), both int32
        [n, num_neighbors]: per seed the most visited vertices, by visit count descending and vertex id ascending, and their counts;
        -1 / 0 past the number of distinct visited vertices.  seeds, weighted, base and stream as in random_walk; no traces are
        written.  A DGL block: mask = neighbors >= 0, src = neighbors[mask], dst = seeds repeated per row under the mask, edge weight
        counts[mask]."""
        seeds = _as_1d(seeds, torch.int32, "seeds")
        n = int(seeds.numel())
        self._check_pinsage(n, num_random_walks, walk_length, num_neighbors, termination_prob, weighted, base)
        if weighted and not self._lib.legion_graph_edge_cdf(self.handle):
            raise ValueError("weighted walks need the graph's edge weights (set_edge_weights)")
        dev = self.col.device
        seeds = seeds.to(dev).contiguous()
        neighbors = torch.empty((n, int(num_neighbors)), dtype=torch.int32, device=dev)
        counts = torch.empty((n, int(num_neighbors)), dtype=torch.int32, device=dev)
        if n == 0:                                   # (nothing to enqueue; an empty tensor has no address to hand over)
            return neighbors, counts
        _enqueue(self._lib, "legion_pinsage_neighbors", "pinsage_neighbors", dev, stream,
                 (self.handle, _ptr(seeds), n, int(num_random_walks), int(walk_length), int(num_neighbors), int(weighted),
                  float(termination_prob), int(base), _ptr(neighbors), _ptr(counts)), (seeds, neighbors, counts))
        return neighbors, counts

    NEGATIVE_MAX_TRIES = 256                         # LEGION_NEGATIVE_MAX_TRIES

    def find_edges(self, eids, stream=None):
        """The endpoints of edges (DGL's g.find_edges; the rule: legion_find_edges in legion_hip.h).  eids: int64 positions in col, a
        CUDA tensor or anything torch.as_tensor takes.  Returns (row, col), both int32 [n]: the CSR row that holds position e -- the
        sampler's dst side -- and col[e], its src side; -1 / -1 for an e outside [0, E) and for a dead (negative) column entry.
        Enqueued on `stream` (default: the current one)."""
        eids = _as_1d(eids, torch.int64, "eids")
        n = int(eids.numel())
        dev = self.col.device
        eids = eids.to(dev).contiguous()
        row = torch.empty((n,), dtype=torch.int32, device=dev)
        col = torch.empty((n,), dtype=torch.int32, device=dev)
        if n == 0:                                   # (nothing to enqueue; an empty tensor has no address to hand over)
            return row, col
        _enqueue(self._lib, "legion_find_edges", "find_edges", dev, stream, (self.handle, _ptr(eids), n, _ptr(row), _ptr(col)),
                 (eids, row, col))
        return row, col

    @staticmethod
    def _check_negative(n, k, exclude_self, exclude_edges, max_tries, base):
        """negative_sample's arguments by the rules of legion_negative_sample, before anything touches a device: ValueError with the
        reason."""
        _need_bool("exclude_self", exclude_self)
        _need_bool("exclude_edges", exclude_edges)
        for name, value in (("k", k), ("max_tries", max_tries), ("base", base)):
            _need_int(name, value)
        if k < 1:
            raise ValueError(f"k must be at least 1, not {k}")
        if not 1 <= max_tries <= GraphStorage.NEGATIVE_MAX_TRIES:
            raise ValueError(f"max_tries must lie in [1, {GraphStorage.NEGATIVE_MAX_TRIES}], not {max_tries}")
        _need_draw_indices(base, n * k, "n * k")

    def negative_sample(self, rows, k, *, exclude_self=True, exclude_edges=True, max_tries=256, base=0, stream=None):
        """k uniform negative endpoints for each of rows (the rule: legion_negative_sample in legion_hip.h; with both exclusions off DGL's
        negative_sampler.Uniform(k), with exclude_edges PyG's structured_negative_sampling).  rows: int32 vertex ids, a CUDA tensor or
        anything torch.as_tensor takes.  Returns int32 [n, k]: vertices drawn uniformly over the graph, redrawn up to max_tries times
        while they are the row itself (exclude_self) or occur in its row of the CSR (exclude_edges: needs sorted rows, rows_sorted() is
        asked here, ValueError if not); -1 where every try was rejected and for a row outside the graph.  base: draw index of the first
        slot; the same rows, flags and base give the same negatives.  Enqueued on `stream` (default: the current one)."""
        rows = _as_1d(rows, torch.int32, "rows")
        n = int(rows.numel())
        self._check_negative(n, k, exclude_self, exclude_edges, max_tries, base)
        if exclude_edges and not self.rows_sorted(stream):
            raise ValueError("negative_sample with exclude_edges needs a graph whose rows are sorted (rows_sorted() is False)")
        dev = self.col.device
        rows = rows.to(dev).contiguous()
        neg = torch.empty((n, int(k)), dtype=torch.int32, device=dev)
        if n == 0:                                   # (nothing to enqueue; an empty tensor has no address to hand over)
            return neg
        _enqueue(self._lib, "legion_negative_sample", "negative_sample", dev, stream,
                 (self.handle, _ptr(rows), n, int(k), int(exclude_self) | int(exclude_edges) << 1, int(max_tries), int(base), _ptr(neg)),
                 (rows, neg))
        return neg

    def edge_prediction_seeds(self, eids, k, *, exclude_self=True, exclude_edges=True, max_tries=256, base=0, stream=None):
        """The seeds of a link-prediction batch from B seed edges (DGL's as_edge_prediction_sampler with a negative sampler): find_edges,
        negative_sample with k negatives per edge's row, and unique_ids over [rows | cols | negatives, row-major].  Returns (seeds,
        num_seeds, pos_row, pos_col, neg_col): seeds int32 [B (2 + k)], the distinct vertices in order of first appearance, -1 from
        num_seeds (a one-element device tensor: no sync) on; pos_row, pos_col int32 [B] and neg_col int32 [B, k], indices into seeds
        (-1 where the edge or the negative is -1).  Hand seeds[:num_seeds] to FeatureStorage.set_ids: a batch's sampled_ids start with
        them in this order, so the indices address the batch's rows.  At k = 1 the thirds of a link-prediction loss are h[pos_row],
        h[pos_col], h[neg_col[:, 0]].  Keywords and stream as in negative_sample."""
        eids = _as_1d(eids, torch.int64, "eids")
        B = int(eids.numel())
        self._check_negative(B, k, exclude_self, exclude_edges, max_tries, base)
        _check_unique(B * (2 + int(k)))
        if exclude_edges and not self.rows_sorted(stream):
            raise ValueError("edge_prediction_seeds with exclude_edges needs a graph whose rows are sorted (rows_sorted() is False)")
        row, col = self.find_edges(eids, stream=stream)
        neg = self.negative_sample(row, k, exclude_self=exclude_self, exclude_edges=exclude_edges, max_tries=max_tries, base=base,
                                   stream=stream)
        if stream is None:
            ids = torch.cat([row, col, neg.reshape(-1)])
        else:
            with torch.cuda.stream(stream):
                ids = torch.cat([row, col, neg.reshape(-1)])
        seeds, local, count = unique_ids(ids, stream=stream)
        return seeds, count, local[:B], local[B:2 * B], local[2 * B:].reshape(B, int(k))

    IN_EDGES_MAX_ROWS = 2 ** 20                      # LEGION_IN_EDGES_MAX_ROWS

    @staticmethod
    def _check_rows(rows, name="rows"):
        """The rows of row_offsets / in_edges by the rules of legion_row_offsets, before anything touches a device: ValueError with the
        reason.  Returns (rows as a tensor, n)."""
        rows = _as_1d(rows, torch.int32, name)
        n = int(rows.numel())
        if n > GraphStorage.IN_EDGES_MAX_ROWS:
            raise ValueError(f"{n} {name} in one call, at most {GraphStorage.IN_EDGES_MAX_ROWS}")
        return rows, n

    def _row_offsets(self, rows, n, stream):
        """rows: on the device, contiguous, checked."""
        dev = self.col.device
        if n == 0:                                   # (an empty tensor has no address to hand over)
            return torch.zeros((1,), dtype=torch.int64, device=dev)
        offsets = torch.empty((n + 1,), dtype=torch.int64, device=dev)
        nbytes = int(self._lib.legion_row_offsets_scratch_bytes(n))
        scratch = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
        _enqueue(self._lib, "legion_row_offsets", "row_offsets", dev, stream,
                 (self.handle, _ptr(rows), n, _ptr(offsets), _ptr(scratch), nbytes), (rows, offsets, scratch))
        return offsets

    def row_offsets(self, rows, stream=None):
        """The prefix sums of the degrees of rows (the rule: legion_row_offsets in legion_hip.h; DGL's g.in_degrees(rows) is
        offsets[1:] - offsets[:-1]).  rows: int32 vertex ids, a CUDA tensor or anything torch.as_tensor takes; at most
        IN_EDGES_MAX_ROWS of them; they may repeat, and a row outside the graph has no entries.  Returns int64 [n + 1]: offsets[i] is
        where row i's entries start in what in_edges writes, offsets[n] their number M; dead (negative) column entries count.  No sync.
        Enqueued on `stream` (default: the current one)."""
        rows, n = self._check_rows(rows)
        return self._row_offsets(rows.to(self.col.device).contiguous(), n, stream)

    def _in_edges(self, rows, n, return_eids, stream, limit=None):
        """(offsets, dst, src, eids or None) of rows (on the device, contiguous, checked); limit: the most n + M may be."""
        dev = self.col.device
        offsets = self._row_offsets(rows, n, stream)
        M = _read_scalar(offsets[n], stream)
        if M > 2 ** 31 - 1:
            raise ValueError(f"the rows hold {M} entries, at most 2^31 - 1 a call")
        if limit is not None and n + M > limit:
            raise ValueError(f"{n} seeds and their {M} entries are {n + M} ids in one call, at most {limit}")
        dst = torch.empty((M,), dtype=torch.int32, device=dev)
        src = torch.empty((M,), dtype=torch.int32, device=dev)
        eids = torch.empty((M,), dtype=torch.int64, device=dev) if return_eids else None
        if M > 0:
            _enqueue(self._lib, "legion_in_edges", "in_edges", dev, stream,
                     (self.handle, _ptr(rows), n, _ptr(offsets), M, _ptr(dst), _ptr(src), _ptr(eids)), (rows, offsets, dst, src, eids))
        return offsets, dst, src, eids

    def in_edges(self, rows, *, return_eids=False, stream=None):
        """Every entry of rows (DGL's g.in_edges(rows, form='all'); the rule: legion_in_edges in legion_hip.h).  rows as in row_offsets.
        Returns (offsets, dst, src) and with return_eids also eids: offsets int64 [n + 1] as row_offsets returns them; dst, src int32
        [M] and eids int64 [M] with M = offsets[n]: entry p of them is position p - offsets[i] of row rows[i], dst[p] = i (the index
        into rows, not the vertex: rows[dst] is the vertex), src[p] = col[eids[p]], -1 for a dead entry, and eids[p] its position in
        col.  The outputs are sized exactly, so offsets[n] is read back to the host once: the call synchronises `stream` (default: the
        current one), on which everything is enqueued.  A capturing caller uses legion_in_edges with a capacity instead."""
        _need_bool("return_eids", return_eids)
        rows, n = self._check_rows(rows)
        out = self._in_edges(rows.to(self.col.device).contiguous(), n, return_eids, stream)
        return out if return_eids else out[:3]

    def _block_tail(self, seeds, n, src, stream):
        """The end of a block: unique_ids over [seeds | src] under `stream`.  Returns (input_nodes, src_local); ValueError unless the n
        seeds are distinct vertices of the graph."""
        def chain():
            ids = torch.cat([seeds, src])
            unique, local, count = unique_ids(ids, stream=stream)
            ok = bool(torch.equal(local[:n], torch.arange(n, dtype=torch.int32, device=local.device)))      # distinct, none negative
            ok = ok and bool((seeds < self.node_num).all())
            return unique, local, int(count.item()), ok

        if stream is None:
            unique, local, U, ok = chain()
        else:
            with torch.cuda.stream(stream):
                unique, local, U, ok = chain()
        if not ok:
            raise ValueError("the seeds of a block must be distinct vertices of the graph: one repeats or lies outside it")
        return unique[:U], local[n:]

    def _check_exclude_eids(self, exclude_eids):
        """A block op's exclude_eids, before anything touches a device: None or an EdgeIdSet on the graph's device, else ValueError."""
        if exclude_eids is None:
            return
        _need_edge_set(exclude_eids, "exclude_eids")
        if exclude_eids.device != self.col.device:
            raise ValueError(f"the EdgeIdSet lives on {exclude_eids.device}, the graph on {self.col.device}")

    def _without_excluded(self, n, dst, src, eids, exclude_eids, stream):
        """What the block ops share of exclude_eids: the list (on the device, with edge ids) through the filter (_filter_edges), then
        the check the op made without a limit.  Returns (dst, src, eids, K's device tensor or None)."""
        dst, src, eids, count = _filter_edges(dst.contiguous(), src.contiguous(), eids.contiguous(), exclude_eids, stream)
        K = int(dst.numel())
        if n + K > UNIQUE_MAX_IDS:
            raise ValueError(f"{n} seeds and their {K} entries left are {n + K} ids in one call, at most {UNIQUE_MAX_IDS}")
        return dst, src, eids, count

    def full_neighbor_block(self, seeds, *, return_eids=False, exclude_eids=None, stream=None):
        """The block of all in-edges of seeds (DGL's MultiLayerFullNeighborSampler(1), or dgl.in_subgraph followed by to_block): in_edges,
        then unique_ids over [seeds | src].  seeds: distinct int32 vertices of the graph, as rows in row_offsets.  Returns (input_nodes,
        dst_local, src_local, offsets) and with return_eids also eids: input_nodes int32 [U], the distinct vertices, the seeds first
        and in their order, then the other sources in order of first appearance; dst_local, src_local int32 [M], indices into
        input_nodes (dst_local[p] is also the index into seeds; src_local[p] == -1 for a dead entry); offsets and eids as in_edges
        returns them.  input_nodes is what FeatureStorage.set_ids takes, or what a feature table is indexed with.  ValueError if the
        seeds and their entries are more than UNIQUE_MAX_IDS ids (before any device work beyond the offsets), and if a seed repeats or
        lies outside the graph: a block's dst nodes are distinct.  Reads back offsets[n], the seeds' local indices and the number of
        distinct vertices: it synchronises `stream` (default: the current one).  exclude_eids: an EdgeIdSet (seed_edge_exclusion makes
        one of a batch's seed edges) whose members are dropped from the edges before the block is made (DGL's exclude= of
        as_edge_prediction_sampler): M is then the number of edges left, offsets their rows' prefix sums, and the id limit applies to
        what is left; None: nothing is dropped."""
        _need_bool("return_eids", return_eids)
        self._check_exclude_eids(exclude_eids)
        seeds, n = self._check_rows(seeds, "seeds")
        _check_unique(n)
        seeds = seeds.to(self.col.device).contiguous()
        if exclude_eids is None:
            offsets, dst, src, eids = self._in_edges(seeds, n, return_eids, stream, limit=UNIQUE_MAX_IDS)
        else:
            _, dst, src, eids = self._in_edges(seeds, n, True, stream)
            if int(dst.numel()) > EDGE_FILTER_MAX_EDGES:
                raise ValueError(f"the seeds hold {int(dst.numel())} entries, at most 2^30 a call with exclude_eids")
            dst, src, eids, count = self._without_excluded(n, dst, src, eids, exclude_eids, stream)
            offsets = self._dst_offsets(dst, count, n, stream)
            eids = eids if return_eids else None
        input_nodes, src_local = self._block_tail(seeds, n, src, stream)
        out = (input_nodes, dst, src_local, offsets)
        return out + (eids,) if return_eids else out

    LABOR_MAX_SLOTS = 2 ** 30                        # LEGION_LABOR_MAX_SLOTS

    @staticmethod
    def _check_labor(fanout, salt, return_eids):
        """labor_edges' keywords by the rules of legion_labor_count, before anything touches a device: ValueError with the reason."""
        _need_bool("return_eids", return_eids)
        _need_int("fanout", fanout)
        _need_int("salt", salt)
        if not 1 <= fanout <= 2 ** 31 - 1:
            raise ValueError(f"fanout must lie in [1, 2^31 - 1], not {fanout}")
        if not -2 ** 63 <= salt <= 2 ** 63 - 1:
            raise ValueError(f"salt must be an int64, not {salt}")

    @staticmethod
    def _check_labor_slots(M):
        if M > GraphStorage.LABOR_MAX_SLOTS:
            raise ValueError(f"the rows hold {M} entries, at most 2^30 a call")

    def _kept_pass(self, c_name, name, stream, args, keep):
        """One pass of a kept-slot op as a call (head, tail, tensors): c_name enqueued on `stream` with `args` between the head (the
        graph, the rows, their offsets, M) and the tail, `keep` kept alive behind the first two tensors."""
        return lambda head, tail, tensors: _enqueue(self._lib, c_name, name, self.col.device, stream, head + args + tail,
                                                    tensors[:2] + keep + tensors[2:])

    def _kept_edges(self, rows, n, return_eids, stream, scratch_bytes, count_call, edges_call, limit=None):
        """(dst, src, eids or None, K's device tensor or None) of the entries of rows (on the device, contiguous, checked) that a
        predicate keeps.  scratch_bytes: the op's C function of M; count_call, edges_call: its two passes (_kept_pass); limit: the
        most n + K may be."""
        dev = self.col.device
        offsets = self._row_offsets(rows, n, stream)
        M = _read_scalar(offsets[n], stream)
        self._check_labor_slots(M)
        head = (self.handle, _ptr(rows), n, _ptr(offsets), M)
        K, count = 0, None
        if n > 0 and M > 0:
            nbytes = int(scratch_bytes(M))
            scratch = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
            count = torch.empty((1,), dtype=torch.int64, device=dev)
            count_call(head, (_ptr(count), _ptr(scratch), nbytes), (rows, offsets, count, scratch))
            K = _read_scalar(count[0], stream)
        if limit is not None and n + K > limit:
            raise ValueError(f"{n} seeds and their {K} kept entries are {n + K} ids in one call, at most {limit}")
        dst = torch.empty((K,), dtype=torch.int32, device=dev)
        src = torch.empty((K,), dtype=torch.int32, device=dev)
        eids = torch.empty((K,), dtype=torch.int64, device=dev) if return_eids else None
        if K > 0:
            edges_call(head, (_ptr(scratch), nbytes, K, _ptr(dst), _ptr(src), _ptr(eids)), (rows, offsets, scratch, dst, src, eids))
        return dst, src, eids, count

    def _labor_edges(self, rows, n, fanout, salt, return_eids, stream, limit=None):
        """(dst, src, eids or None) of rows (on the device, contiguous, checked); limit: the most n + K may be."""
        args = ("labor_edges", stream, (int(fanout), int(salt)), ())
        return self._kept_edges(rows, n, return_eids, stream, self._lib.legion_labor_scratch_bytes,
                                self._kept_pass("legion_labor_count", *args), self._kept_pass("legion_labor_edges", *args), limit)[:3]

    def labor_edges(self, rows, fanout, *, salt=0, return_eids=False, stream=None):
        """Layer-neighbour sampling of the in-edges of rows (LABOR-0; DGL's dgl.sampling.sample_labors; the rule: legion_labor_count
        and legion_labor_edges in legion_hip.h).  Every source vertex t has one random number, a hash of (t, salt); the entry t -> s is
        kept iff that number lies below fanout / deg(s), so a row keeps fanout entries in expectation, every entry when its degree is
        at most fanout, and rows with common neighbours keep the same ones.  rows as in row_offsets; fanout at least 1; salt any
        int64.  Returns (dst, src) and with return_eids also eids: int32 [K], int32 [K] and int64 [K], the kept entries in the order
        of in_edges (dst[p] is the index into rows, non-decreasing; src[p] = col[eids[p]]); dead entries are never kept.  The same
        arguments give the same result.  The same salt for every layer of a batch is LABOR's layer dependency (the same r_t in all
        layers); a new salt per batch is the caller's to choose.  The outputs are sized exactly: the number of entries M and the kept
        number K are read back to the host, so the call synchronises `stream` (default: the current one) twice.  ValueError if the
        rows hold more than 2^30 entries (a caller batches).  A capturing caller uses the C ABI with a capacity instead."""
        self._check_labor(fanout, salt, return_eids)
        rows, n = self._check_rows(rows)
        out = self._labor_edges(rows.to(self.col.device).contiguous(), n, fanout, salt, return_eids, stream)
        return out if return_eids else out[:2]

    def labor_block(self, seeds, fanout, *, salt=0, return_eids=False, exclude_eids=None, stream=None):
        """The block of a LABOR-0 layer (DGL's LaborSampler with one fan-out): labor_edges, then unique_ids over [seeds | src].  seeds:
        distinct int32 vertices of the graph.  Returns (input_nodes, dst_local, src_local) and with return_eids also eids: input_nodes
        int32 [U], the seeds first and in their order, then the other kept sources in order of first appearance; dst_local, src_local
        int32 [K], indices into input_nodes (dst_local[p] is also the index into seeds); eids as labor_edges returns them.
        input_nodes is what FeatureStorage.set_ids takes, and the seeds of the next layer out.  The same salt for every layer of a
        batch is LABOR's layer dependency (the same r_t in all layers: a vertex kept in one layer tends to be kept in the next, which
        is what keeps the input nodes few); a new salt per batch is the caller's to choose.  ValueError if the seeds and their kept
        entries are more than UNIQUE_MAX_IDS ids, and if a seed repeats or lies outside the graph, as full_neighbor_block.
        Synchronises `stream` (default: the current one).  exclude_eids: as in full_neighbor_block -- the set's members are dropped
        from the kept edges (the sampling itself does not look at the set: as DGL, which excludes after sample_neighbors)."""
        self._check_labor(fanout, salt, return_eids)
        self._check_exclude_eids(exclude_eids)
        seeds, n = self._check_rows(seeds, "seeds")
        _check_unique(n)
        seeds = seeds.to(self.col.device).contiguous()
        if exclude_eids is None:
            dst, src, eids = self._labor_edges(seeds, n, fanout, salt, return_eids, stream, limit=UNIQUE_MAX_IDS)
        else:
            dst, src, eids = self._labor_edges(seeds, n, fanout, salt, True, stream)
            dst, src, eids = self._without_excluded(n, dst, src, eids, exclude_eids, stream)[:3]
            eids = eids if return_eids else None
        input_nodes, src_local = self._block_tail(seeds, n, src, stream)
        out = (input_nodes, dst, src_local)
        return out + (eids,) if return_eids else out

    TOPK_MAX_K = 64                                  # LEGION_TOPK_MAX_K
    TOPK_LARGEST, TOPK_SMALLEST, TOPK_SAMPLE = 0, 1, 2      # LEGION_TOPK_*

    @staticmethod
    def _check_topk(k, name, salt, return_eids):
        """The keywords of select_topk / sample_distinct by the rules of legion_row_topk, before anything touches a device: ValueError
        with the reason."""
        _need_bool("return_eids", return_eids)
        _need_int(name, k)
        _need_int("salt", salt)
        if not 1 <= k <= GraphStorage.TOPK_MAX_K:
            raise ValueError(f"{name} must lie in [1, {GraphStorage.TOPK_MAX_K}], not {k}")
        if not -2 ** 63 <= salt <= 2 ** 63 - 1:
            raise ValueError(f"salt must be an int64, not {salt}")

    def _topk_weights(self, weights):
        """weights as float32 [E] on the graph's device, aligned with col: ValueError otherwise."""
        if isinstance(weights, np.ndarray):
            if weights.dtype != np.float32:
                raise ValueError(f"weights must be float32, not {weights.dtype}")
            weights = torch.from_numpy(np.ascontiguousarray(weights))
        if not isinstance(weights, torch.Tensor):
            raise ValueError(f"weights must be a float32 tensor or array, not {type(weights).__name__}")
        if weights.dtype != torch.float32:
            raise ValueError(f"weights must be float32, not {weights.dtype}")
        if weights.dim() != 1 or weights.numel() != self.edge_num:
            raise ValueError(f"weights must have one entry per edge ({self.edge_num}), not shape {tuple(weights.shape)}")
        return weights.to(self.col.device).contiguous()

    def _row_topk(self, rows, n, k, mode, w, salt, return_eids, stream):
        """(src [n, k], counts [n], eids [n, k] or None) of rows (on the device, contiguous, checked)."""
        dev = self.col.device
        src = torch.empty((n, int(k)), dtype=torch.int32, device=dev)
        counts = torch.empty((n,), dtype=torch.int32, device=dev)
        eids = torch.empty((n, int(k)), dtype=torch.int64, device=dev) if return_eids else None
        if n == 0:                                   # (nothing to enqueue; an empty tensor has no address to hand over)
            return src, counts, eids
        nbytes = int(self._lib.legion_row_topk_scratch_bytes(n))
        scratch = torch.empty((nbytes // 4,), dtype=torch.int32, device=dev)
        _enqueue(self._lib, "legion_row_topk", "select_topk / sample_distinct", dev, stream,
                 (self.handle, _ptr(rows), n, int(k), int(mode), _ptr(w), int(salt), _ptr(src), _ptr(eids), _ptr(counts), _ptr(scratch),
                  nbytes), (rows, w, src, eids, counts, scratch))
        return src, counts, eids

    def select_topk(self, rows, k, weights, *, ascending=False, return_eids=False, stream=None):
        """The k heaviest (ascending: lightest) in-edges of each of rows (DGL's dgl.sampling.select_topk; the rule: legion_row_topk in
        legion_hip.h).  rows as in row_offsets; k in [1, TOPK_MAX_K]; weights float32 [E], aligned with col, a tensor on any device or
        a numpy array.  Returns (src, counts) and with return_eids also eids: src int32 [n, k], per row the sources of its best
        entries, best first, equal weights in the order of their positions, -1 past the row's counts[i] = min(k, live entries whose
        weight is not NaN); eids int64 [n, k], their positions in col, -1 likewise.  -0 equals +0, and +-inf order as numbers.  A row
        outside the graph has no entries.  No sync.  Enqueued on `stream` (default: the current one)."""
        _need_bool("ascending", ascending)
        self._check_topk(k, "k", 0, return_eids)
        rows, n = self._check_rows(rows)
        w = self._topk_weights(weights)
        mode = self.TOPK_SMALLEST if ascending else self.TOPK_LARGEST
        out = self._row_topk(rows.to(self.col.device).contiguous(), n, k, mode, w, 0, return_eids, stream)
        return out if return_eids else out[:2]

    def sample_distinct(self, rows, fanout, *, weights=None, salt=0, return_eids=False, stream=None):
        """Weighted neighbour sampling WITHOUT replacement of the in-edges of rows (DGL's sample_neighbors(g, rows, fanout, prob=weights),
        whose replace defaults to False; the rule: legion_row_topk in legion_hip.h, mode LEGION_TOPK_SAMPLE).  Every entry e has an
        exponential variate E, a hash of (e, salt); a row keeps its fanout entries of smallest E / w, which is a weighted sample
        without replacement (Efraimidis and Spirakis).  rows as in row_offsets; fanout in [1, TOPK_MAX_K]; weights as in select_topk,
        None: every weight 1 (uniform sampling without replacement); a weight that is not finite and > 0 is never picked, nor is a
        dead entry.  Returns (src, counts) and with return_eids also eids, shaped as select_topk's: counts[i] = min(fanout, entries
        that can be picked).  The same arguments give the same result, and the same row listed twice gets the same picks: a new salt
        per batch is the caller's to choose.  The pool's sampling modes are not involved: weighted sampling inside a MemoryPool stays
        with replacement.  No sync.  Enqueued on `stream` (default: the current one)."""
        self._check_topk(fanout, "fanout", salt, return_eids)
        rows, n = self._check_rows(rows)
        w = self._topk_weights(weights) if weights is not None else None
        out = self._row_topk(rows.to(self.col.device).contiguous(), n, fanout, self.TOPK_SAMPLE, w, salt, return_eids, stream)
        return out if return_eids else out[:2]

    def sample_distinct_block(self, seeds, fanout, *, weights=None, salt=0, return_eids=False, exclude_eids=None, stream=None):
        """The block of one layer sampled by sample_distinct (DGL's NeighborSampler with one fan-out and prob=): the picks with src >= 0,
        then unique_ids over [seeds | src].  seeds: distinct int32 vertices of the graph.  Returns (input_nodes, dst_local, src_local)
        and with return_eids also eids, in labor_block's layout: input_nodes int32 [U], the seeds first and in their order, then the
        other picked sources in order of first appearance; dst_local, src_local int32 [K], indices into input_nodes (dst_local[p] is
        also the index into seeds, non-decreasing); eids int64 [K].  input_nodes is what FeatureStorage.set_ids takes, and the seeds
        of the next layer out.  A new salt per batch and per layer is the caller's to choose.  ValueError if the seeds and their picks
        could be more than UNIQUE_MAX_IDS ids, and if a seed repeats or lies outside the graph, as full_neighbor_block.  Synchronises
        `stream` (default: the current one).  exclude_eids: as in full_neighbor_block -- the set's members are dropped from the picks
        (a row then has fewer than its counts: as DGL, which excludes after sample_neighbors)."""
        self._check_topk(fanout, "fanout", salt, return_eids)
        self._check_exclude_eids(exclude_eids)
        seeds, n = self._check_rows(seeds, "seeds")
        _check_unique(n)
        if n + n * int(fanout) > UNIQUE_MAX_IDS:
            raise ValueError(f"{n} seeds and up to {n * int(fanout)} picks are {n + n * int(fanout)} ids in one call, at most {UNIQUE_MAX_IDS}")
        w = self._topk_weights(weights) if weights is not None else None
        seeds = seeds.to(self.col.device).contiguous()
        with_eids = return_eids or exclude_eids is not None
        src, _, eids = self._row_topk(seeds, n, fanout, self.TOPK_SAMPLE, w, salt, with_eids, stream)

        def mask():
            keep = src >= 0
            dst = torch.nonzero(keep)[:, 0].to(torch.int32)
            return dst, src[keep], eids[keep] if with_eids else None

        if stream is None:
            dst, picked, eids = mask()
        else:
            with torch.cuda.stream(stream):
                dst, picked, eids = mask()
        if exclude_eids is not None:
            dst, picked, eids = self._without_excluded(n, dst, picked, eids, exclude_eids, stream)[:3]
            eids = eids if return_eids else None
        input_nodes, src_local = self._block_tail(seeds, n, picked, stream)
        out = (input_nodes, dst, src_local)
        return out + (eids,) if return_eids else out

    @staticmethod
    def _check_nodes(nodes, limit=NODE_SET_MAX_IDS):
        """The nodes of induced_edges / node_subgraph by the rules of legion_node_set_build, before anything touches a device:
        ValueError with the reason.  Returns a NodeSet as it is, anything else as a tensor."""
        if not isinstance(nodes, NodeSet):
            nodes = _as_1d(nodes, torch.int32, "nodes")
        k = nodes.k if isinstance(nodes, NodeSet) else int(nodes.numel())
        if k > limit:
            raise ValueError(f"{k} nodes in one call, at most {limit}")
        return nodes

    def _node_set(self, nodes, stream):
        """nodes (checked) as a NodeSet on the graph's device: one as it is, anything else built here on `stream`."""
        if isinstance(nodes, NodeSet):
            if nodes.device != self.col.device:
                raise ValueError(f"the NodeSet lives on {nodes.device}, the graph on {self.col.device}")
            return nodes
        return NodeSet(nodes, device=self.col.device, stream=stream)

    def _induced_edges(self, rows, n, ns, return_eids, stream):
        """(dst, src_local, eids or None, K's device tensor or None) of rows (on the device, contiguous, checked) against the set ns."""
        args = ("induced_edges", stream, (_ptr(ns.table), ns.set_bytes, ns.k), (ns.table,))
        return self._kept_edges(rows, n, return_eids, stream, self._lib.legion_induced_scratch_bytes,
                                self._kept_pass("legion_induced_count", *args), self._kept_pass("legion_induced_edges", *args))

    def induced_edges(self, rows, nodes, *, return_eids=False, stream=None):
        """The in-edges of rows whose source is a member of a vertex set (the rule: legion_induced_count and legion_induced_edges in
        legion_hip.h).  rows as in row_offsets; nodes: a NodeSet, or anything NodeSet takes (the set is then built here).  rows and
        nodes are independent: the edges from a set into a frontier are a bipartite block's and ShaDow-GNN's case.  Returns (dst,
        src_local) and with return_eids also eids: int32 [K], int32 [K] and int64 [K], the kept entries in the order of in_edges:
        dst[p] is the index into rows, non-decreasing; src_local[p] the first position of the source in nodes (nodes[src_local] is the
        vertex); eids[p] the entry's position in col.  Parallel entries and self-loops are kept like any other entry, dead entries
        never.  The outputs are sized exactly: the number of entries M and the kept number K are read back to the host, so the call
        synchronises `stream` (default: the current one) twice.  ValueError if the rows hold more than 2^30 entries (a caller
        batches).  A capturing caller uses the C ABI with a capacity instead."""
        _need_bool("return_eids", return_eids)
        rows, n = self._check_rows(rows)
        ns = self._node_set(self._check_nodes(nodes), stream)
        out = self._induced_edges(rows.to(self.col.device).contiguous(), n, ns, return_eids, stream)[:3]
        return out if return_eids else out[:2]

    def node_subgraph(self, nodes, *, return_eids=False, stream=None):
        """The subgraph a vertex set induces, in this library's CSR (DGL's g.subgraph(nodes) / dgl.node_subgraph; what ClusterGCN takes
        of a partition, GraphSAINT of the vertices its walks visited, ShaDow-GNN of a sampled k-hop neighbourhood): induced_edges with
        rows = nodes, then legion_dst_offsets.  nodes: k distinct int32 vertices of the graph, a NodeSet or anything NodeSet takes.
        Returns (indptr_sub, col_sub) and with return_eids also eids: indptr_sub int64 [k + 1], col_sub int32 [K], eids int64 [K].
        Vertex j of the subgraph is nodes[j]; row j holds the positions in nodes of the live in-neighbours of nodes[j] that are
        members, in the order of the graph's row.  GraphStorage(1, indptr_sub, col_sub) is a graph this library samples and walks;
        eids are DGL's subgraph.edata[dgl.EID], the entries' positions in this graph's col.  For ascending nodes sorted rows stay
        sorted (the map is monotone), and dead entries are gone.  ValueError if a node repeats, is negative or lies at or past
        node_num: a subgraph's vertices are distinct vertices of the graph (read back after the set's build, before the expansion).
        Synchronises `stream` (default: the current one)."""
        _need_bool("return_eids", return_eids)
        ns = self._node_set(self._check_nodes(nodes, GraphStorage.IN_EDGES_MAX_ROWS), stream)
        dev, k = self.col.device, ns.k

        def legal():
            if k == 0:
                return True
            inside = (ns.nodes >= 0).all() & (ns.nodes < self.node_num).all() & (ns.distinct[0] == k)
            return bool(inside.item())

        if stream is None:
            ok = legal()
        else:
            with torch.cuda.stream(stream):
                ok = legal()
        if not ok:
            raise ValueError("the nodes of a subgraph must be distinct vertices of the graph: one repeats or lies outside it")
        dst, src, eids, count = self._induced_edges(ns.nodes, k, ns, return_eids, stream)
        K = int(dst.numel())
        if K > 0:
            indptr = torch.empty((k + 1,), dtype=torch.int64, device=dev)
            _enqueue(self._lib, "legion_dst_offsets", "node_subgraph", dev, stream, (_ptr(dst), K, _ptr(count), k, _ptr(indptr)),
                     (dst, count, indptr))
        elif stream is None:
            indptr = torch.zeros((k + 1,), dtype=torch.int64, device=dev)
        else:
            with torch.cuda.stream(stream):
                indptr = torch.zeros((k + 1,), dtype=torch.int64, device=dev)
        return (indptr, src, eids) if return_eids else (indptr, src)

    REVERSE_MAX_NODES = 2 ** 28                      # LEGION_REVERSE_MAX_NODES

    def reverse(self, stream=None):
        """The graph with every edge turned round (DGL's dgl.reverse; the rule: legion_graph_build_reverse in legion_hip.h): a
        GraphStorage whose row u holds the vertices that u's edges point to, sorted by the edges' positions in this graph's col, so
        its rows are sorted by vertex id (rows_sorted() is True) and every method of this class works on it: a walk on it follows
        the edges backwards, its in_edges are this graph's out-edges.  Dead (-1) column entries and entries outside the graph are
        dropped.  .indptr int64 [N + 1], .col int32 [E'] and .eids int64 [E'] -- entry p of the reverse is entry eids[p] of this
        graph's col -- are views of arrays the library owns; .parent is this graph, which stays alive with it.  Built on the device at
        the first call (it synchronises `stream`, default the current one, and is not to be captured) and remembered: later calls
        return the same object.  Edge weights do not travel by themselves: rev.set_edge_weights(w[rev.eids]) gives the reverse the
        weights w of this graph's edges.  ValueError for more than REVERSE_MAX_NODES vertices."""
        if getattr(self, "_reverse", None) is None:
            if self.node_num > self.REVERSE_MAX_NODES:
                raise ValueError(f"{self.node_num} vertices, at most {self.REVERSE_MAX_NODES} for a reverse")
            dev = self.col.device
            with torch.cuda.device(dev):
                rc = self._lib.legion_graph_build_reverse(self.handle, _stream_handle(stream))
            if rc != 0:
                raise RuntimeError("legion_graph_build_reverse refused the graph")
            a, b, c = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
            live = int(self._lib.legion_graph_reverse_csr(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
            rev = GraphStorage(self.partition_count, device_view(a.value, (self.node_num + 1,), torch.int64, dev),
                               device_view(b.value, (live,), torch.int32, dev))
            rev.eids = device_view(c.value, (live,), torch.int64, dev)
            rev.parent = self
            self._reverse = rev
        return self._reverse

    def out_degrees(self, nodes, stream=None):
        """The number of edges that leave each of nodes (DGL's g.out_degrees): int64 [n], by row_offsets on reverse() and a
        difference; 0 for a node outside the graph.  nodes as rows in row_offsets.  The first call builds the reverse."""
        nodes, n = self._check_rows(nodes, "nodes")
        rev = self.reverse(stream)
        offsets = rev._row_offsets(nodes.to(self.col.device).contiguous(), n, stream)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            return offsets[1:] - offsets[:-1]

    def out_edges(self, nodes, *, return_eids=False, stream=None):
        """Every edge that leaves nodes (DGL's g.out_edges(nodes, form='all')): reverse().in_edges(nodes) and one index through
        .eids.  nodes as rows in row_offsets.  Returns (src, dst) and with return_eids also eids: src, dst int32 [M] and eids int64
        [M]; src[p] = i, the index into nodes (nodes[src] is the vertex, as in_edges' dst), dst[p] the vertex the edge points to and
        eids[p] the edge's position in THIS graph's col: col[eids] == nodes[src], and find_edges(eids)'s row is dst.  The edges of
        nodes[i] are consecutive, ordered by eids.  Like in_edges it synchronises `stream` (default: the current one); the first call
        builds the reverse."""
        _need_bool("return_eids", return_eids)
        nodes, n = self._check_rows(nodes, "nodes")
        rev = self.reverse(stream)
        _, src, dst, at = rev._in_edges(nodes.to(self.col.device).contiguous(), n, return_eids, stream)
        if not return_eids:
            return src, dst
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            return src, dst, rev.eids[at]

    def _dst_offsets(self, dst, count, n, stream):
        """The row pointers int64 [n + 1] of a non-decreasing dst (on the device) whose length is count's value (a device tensor, or
        None with an empty dst): legion_dst_offsets."""
        dev, K = self.col.device, int(dst.numel())
        if K > 0:
            indptr = torch.empty((n + 1,), dtype=torch.int64, device=dev)
            _enqueue(self._lib, "legion_dst_offsets", "dst_offsets", dev, stream, (_ptr(dst), K, _ptr(count), n, _ptr(indptr)),
                     (dst, count, indptr))
            return indptr
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            return torch.zeros((n + 1,), dtype=torch.int64, device=dev)

    REVERSE_IDS_MAX = 2 ** 31 - 1                    # legion_reverse_edge_ids' n

    def reverse_edge_ids(self, eids, stream=None):
        """The reverse edge id of each edge (the pairing behind DGL's exclude="reverse_id"; the rule: legion_reverse_edge_ids in
        legion_hip.h).  eids: int64 positions in col, a CUDA tensor or anything torch.as_tensor takes.  Returns int64 [n]: for the edge
        e = eids[i] from u = col[e] into v, its row, the LEAST position e' in row u with col[e'] == v -- the first edge from v into
        u; -1 for an e outside [0, E), for a dead entry or one that points outside the graph, and where no reverse edge exists.
        Parallel edges all map to the first reverse edge (no rank-matched pairing: reverse_edge_ids of the result gives e back only
        for the least of its parallel edges); a self-loop maps to the least self-loop of its row.  The same graph gives the same
        answer, bit for bit.  With sorted rows (rows_sorted() is asked here) the graph's own rows are searched; otherwise reverse() is
        built -- set-up: it synchronises `stream` -- and its rows are.  Enqueued on `stream` (default: the current one)."""
        eids = _as_1d(eids, torch.int64, "eids")
        n = int(eids.numel())
        if n > self.REVERSE_IDS_MAX:
            raise ValueError(f"{n} edge ids in one call, at most 2^31 - 1")
        dev = self.col.device
        eids = eids.to(dev).contiguous()
        out = torch.empty((n,), dtype=torch.int64, device=dev)
        if n == 0:                                   # (nothing to enqueue; an empty tensor has no address to hand over)
            return out
        via = 0 if self.rows_sorted(stream) else 1
        if via == 1:
            self.reverse(stream)
        _enqueue(self._lib, "legion_reverse_edge_ids", "reverse_edge_ids", dev, stream, (self.handle, _ptr(eids), n, via, _ptr(out)), (eids, out))
        return out

    def seed_edge_exclusion(self, eids, exclude="self", stream=None):
        """The set of edges a link-prediction batch must not see (DGL's as_edge_prediction_sampler(exclude=...)): an EdgeIdSet to hand
        to full_neighbor_block, labor_block and sample_distinct_block as exclude_eids, or to exclude_edges.  eids: the batch's seed
        edges, int64, at most EDGE_SET_MAX_IDS with their reverses.  exclude="self": the set holds the seed edges; "reverse_id": the
        seed edges and reverse_edge_ids of them (an edge without a reverse adds nothing).  Anything else is a ValueError, before
        anything touches a device.  Enqueued on `stream` (default: the current one); no sync beyond reverse_edge_ids' set-up."""
        if not isinstance(exclude, str) or exclude not in ("self", "reverse_id"):
            raise ValueError(f'exclude must be "self" or "reverse_id", not {exclude!r}')
        eids = _as_1d(eids, torch.int64, "eids")
        k = int(eids.numel()) * (2 if exclude == "reverse_id" else 1)
        if k > EDGE_SET_MAX_IDS:
            raise ValueError(f"{k} edge ids in one set, at most {EDGE_SET_MAX_IDS}")
        dev = self.col.device
        eids = eids.to(dev).contiguous()
        if exclude == "reverse_id":
            rev = self.reverse_edge_ids(eids, stream=stream)
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
                eids = torch.cat([eids, rev])
        return EdgeIdSet(eids, device=dev, stream=stream)

    def column_slots(self, dev_id=0):
        """True when logical GPU dev_id samples from the {neighbour id, feature-cache slot} copy of the column array."""
        return bool(self._lib.legion_graph_column_slots(self.handle, int(dev_id)))

    def cached_csr(self, dev_id, capacity):
        """(index int64[capacity + 1], dst int32[index[capacity]]) of the CSR GPU dev_id caches after a fill, as device views."""
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        self._lib.legion_graph_cached_csr(self.handle, int(dev_id), ctypes.byref(a), ctypes.byref(b))
        dev = _torch_device(dev_id)
        index = device_view(a.value, (int(capacity) + 1,), torch.int64, dev)
        n = int(index[-1].item()) if capacity >= 0 and a.value else 0
        return index, device_view(b.value, (n,), torch.int32, dev)

    def close(self):
        rev = getattr(self, "_reverse", None)
        if rev is not None:                          # (its arrays are this graph's: they go with the handle below)
            rev.close()
            self._reverse = None
        if self.handle:
            self._lib.legion_graph_destroy(self.handle)
            self.handle = None


# feature_dtype of FeatureStorage -> legion_hip.h LEGION_FEATURE_*
FEATURE_DTYPES = {"float32": 0, "bfloat16": 1}


def bf16_pitch(D):
    """Elements of a stored bf16 row: D rounded up to 8 (16-byte rows, zero padded)."""
    return (int(D) + 7) // 8 * 8


def convert_f32_to_bf16(src):
    """float32[N, D] device tensor -> int16[N, round_up(D, 8)] device tensor of bf16 bit patterns (the library's conversion)."""
    assert src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 2 and src.is_cuda
    N, D = src.shape
    out = torch.empty((N, bf16_pitch(D)), dtype=torch.int16, device=src.device)
    _libmod.load().legion_convert_f32_to_bf16(None, _ptr(src), int(N), int(D), _ptr(out))
    return out


class FeatureStorage:
    """Full feature table + per-GPU seed sets.  feature_dtype="float32" (default): the device tensor float32[N, D] (HBM or mapped
    pinned) is used in place.  feature_dtype="bfloat16": the library keeps a bf16 copy of it (rows of round_up(D, 8) elements,
    round to nearest even) and every cache tier built from this storage holds bf16 rows; gathered rows are float32 as before."""

    def __init__(self, partition_count, features, total_num_nodes=None, float_feature_len=None, feature_dtype="float32"):
        self._lib = _libmod.load()
        if feature_dtype not in FEATURE_DTYPES:
            raise ValueError(f"feature_dtype must be one of {sorted(FEATURE_DTYPES)}, not {feature_dtype!r}")
        self.feature_dtype = feature_dtype
        self.features = features
        if features is not None:
            assert features.dtype == torch.float32 and features.is_contiguous()
            total_num_nodes = features.shape[0] if total_num_nodes is None else total_num_nodes
            float_feature_len = features.shape[1] if float_feature_len is None else float_feature_len
        self.total_num_nodes = int(total_num_nodes)
        self.float_feature_len = int(float_feature_len)
        self.partition_count = int(partition_count)
        if feature_dtype == "float32":
            self.handle = self._lib.legion_feature_create(self.partition_count, self.total_num_nodes,
                                                          self.float_feature_len, _ptr(features))
        else:
            self.handle = self._lib.legion_feature_create_ex(self.partition_count, self.total_num_nodes, self.float_feature_len,
                                                             FEATURE_DTYPES[feature_dtype], _ptr(features))
            if not self.handle:
                raise RuntimeError(f"legion_feature_create_ex failed for {feature_dtype}")
            self.features = None        # the library owns its converted table; the caller's float32 tensor is not referenced
        self.set_sizes = {}

    @property
    def row_bytes(self):
        return int(self._lib.legion_feature_row_bytes(self.handle))

    def set_ids(self, dev_id, mode, ids, labels=None):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32)
        self._lib.legion_feature_set_ids(self.handle, int(dev_id), int(mode),
                                         ids.ctypes.data_as(ctypes.c_void_p),
                                         lab.ctypes.data_as(ctypes.c_void_p) if lab is not None else None,
                                         int(ids.size))
        self.set_sizes[(int(dev_id), int(mode))] = int(ids.size)

    def close(self):
        if self.handle:
            self._lib.legion_feature_destroy(self.handle)
            self.handle = None


def _set_sample_mode(owner, c_name, what, value, types, refused):
    """One sampling mode of a MemoryPool or a Pipeline (owner: its _lib and handle, touched only once the value is valid) through its
    C setter, which refuses what sample_mode.h does not allow and every change after the first hop: RuntimeError."""
    if not isinstance(value, types) or int(value) not in (0, 1):
        raise ValueError(f"{what} must be True or False, not {value!r}")
    if getattr(owner._lib, c_name)(owner.handle, int(value)) != 0:
        raise RuntimeError(f"{c_name}: {refused}")


class MemoryPool:
    _BUF = {"sampled_ids": (0, torch.int32), "float_features": (1, torch.float32),
            "labels": (2, torch.int32), "agg_src_off": (3, torch.int32), "agg_dst_off": (4, torch.int32),
            "node_counter": (5, torch.int32), "edge_counter": (6, torch.int32),
            "agg_src_ids": (7, torch.int32), "agg_dst_ids": (8, torch.int32),
            "cache_search_buffer": (9, torch.int32), "tmp_part_ind": (10, torch.int8),
            "tmp_part_off": (11, torch.int32), "position_map": (12, torch.int32), "node_slot": (13, torch.int32),
            "agg_edge_ids": (14, torch.int64)}

    def __init__(self, dev_id, total_num_nodes, batch_size, fanout, float_feature_len, pipeline_depth=1, feature_out_dtype="float32",
                 replace=True, edge_ids=False, weighted=False):
        """feature_out_dtype: dtype of the rows the pool's gathers write ("float32" or "bfloat16": bf16[rows, D], the float32 row
        rounded to nearest even, or a bf16 storage's rows verbatim), independent of the FeatureStorage's dtype.
        replace: as DGL's NeighborSampler keyword -- True samples with replacement (the reference's draw), False takes min(f, D)
        distinct neighbours of each frontier entry (fan-outs up to 256).
        edge_ids: True also records, per sampled edge, its position in the graph's column array (DGL's dgl.EID): buffer("agg_edge_ids"),
        int64, indexed like agg_src_ids; read_batch returns it as "agg_edge_ids".
        weighted: as DGL's prob= -- True picks each neighbour with probability proportional to its edge's weight
        (GraphStorage.set_edge_weights, which must have run before the first batch); needs replace=True."""
        if feature_out_dtype not in FEATURE_DTYPES:
            raise ValueError(f"feature_out_dtype must be one of {sorted(FEATURE_DTYPES)}, not {feature_out_dtype!r}")
        if not isinstance(edge_ids, bool):
            raise ValueError(f"edge_ids must be True or False, not {edge_ids!r}")
        if not isinstance(weighted, bool):
            raise ValueError(f"weighted must be True or False, not {weighted!r}")
        self._lib = _libmod.load()
        self.dev_id = int(dev_id)
        self.device = _torch_device(self.dev_id)
        self.total_num_nodes = int(total_num_nodes)
        self.batch_size = int(batch_size)
        self.fanout = [int(f) for f in fanout]
        self.float_feature_len = int(float_feature_len)
        self.feature_rows = 0
        self.handle = self._lib.legion_pool_create(self.dev_id, self.total_num_nodes, self.batch_size,
                                                   _i32_array(self.fanout), len(self.fanout),
                                                   self.float_feature_len, int(pipeline_depth))
        self.num_ids = int(self._lib.legion_pool_num_ids(self.handle))
        self.set_feature_out_dtype(feature_out_dtype)
        self.set_replace(replace)
        if edge_ids:
            self.set_edge_ids(True)
        if weighted:
            self.set_weighted(True)

    @classmethod
    def _borrowed(cls, handle, dev_id, total_num_nodes, batch_size, fanout, float_feature_len, feature_rows):
        """View of a pool owned by a Pipeline lane (close() is a no-op)."""
        self = cls.__new__(cls)
        self._lib = _libmod.load()
        self.dev_id = int(dev_id)
        self.device = _torch_device(self.dev_id)
        self.total_num_nodes, self.batch_size = int(total_num_nodes), int(batch_size)
        self.fanout = [int(f) for f in fanout]
        self.float_feature_len, self.feature_rows = int(float_feature_len), int(feature_rows)
        self.handle = handle
        self.num_ids = int(self._lib.legion_pool_num_ids(handle))
        self._borrowed_handle = True
        return self

    @property
    def feature_out_dtype(self):
        return {v: k for k, v in FEATURE_DTYPES.items()}[int(self._lib.legion_pool_feature_out_dtype(self.handle))]

    def set_feature_out_dtype(self, dtype):
        """Only before alloc_features (the C ABI refuses it after: RuntimeError)."""
        if dtype not in FEATURE_DTYPES:
            raise ValueError(f"feature_out_dtype must be one of {sorted(FEATURE_DTYPES)}, not {dtype!r}")
        if self._lib.legion_pool_set_feature_out_dtype(self.handle, FEATURE_DTYPES[dtype]) != 0:
            raise RuntimeError("legion_pool_set_feature_out_dtype: the feature buffer is already allocated")

    @property
    def replace(self):
        return int(self._lib.legion_pool_sample_replace(self.handle)) == 1

    def set_replace(self, replace):
        """Only before the pool samples its first hop (the C ABI refuses it after: RuntimeError)."""
        _set_sample_mode(self, "legion_pool_set_sample_replace", "replace", replace, (bool, int),
                         "the pool has sampled already, or a fan-out is above 256 without replacement, or the pool is weighted")

    @property
    def edge_ids(self):
        return int(self._lib.legion_pool_edge_ids(self.handle)) == 1

    def set_edge_ids(self, on):
        """Only before the pool samples its first hop (the C ABI refuses it after: RuntimeError).  A Pipeline's lanes take the mode
        through Pipeline.set_edge_ids."""
        _set_sample_mode(self, "legion_pool_set_edge_ids", "edge_ids", on, bool, "the pool has sampled already")

    @property
    def weighted(self):
        return int(self._lib.legion_pool_sample_weighted(self.handle)) == 1

    def set_weighted(self, on):
        """Only before the pool samples its first hop, and only with replace=True (the C ABI refuses it otherwise: RuntimeError).  A
        Pipeline's lanes take the mode through Pipeline.set_weighted."""
        _set_sample_mode(self, "legion_pool_set_sample_weighted", "weighted", on, bool,
                         "the pool has sampled already, or it samples without replacement")

    def alloc_features(self, rows):
        self.feature_rows = int(rows)
        self._lib.legion_pool_alloc_features(self.handle, self.feature_rows)

    def set_current_pipe(self, pipe):
        self._lib.legion_pool_set_current_pipe(self.handle, int(pipe))

    def buffer(self, name):
        which, dtype = self._BUF[name]
        if name == "float_features" and self.feature_out_dtype == "bfloat16":
            dtype = torch.bfloat16
        ptr = self._lib.legion_pool_buffer(self.handle, which)
        if name == "agg_edge_ids" and not ptr:
            raise RuntimeError("agg_edge_ids: the pool's edge-id mode is off (MemoryPool(..., edge_ids=True) / set_edge_ids)")
        if name in ("node_counter", "edge_counter"):
            shape = (16,)
        elif name == "labels":
            shape = (self.batch_size,)
        elif name == "float_features":
            shape = (self.feature_rows, self.float_feature_len)
        elif name == "position_map":
            shape = (self.total_num_nodes,)
        else:
            shape = (self.num_ids,)
        return device_view(ptr, shape, dtype, self.device)

    def lds_buckets(self):
        """Hash buckets per lane of the first-touch de-duplication (8, 16, 64 or 256 by the pool's largest hop)."""
        return int(self._lib.legion_pool_lds_buckets(self.handle))

    def state_bytes(self):
        return int(self._lib.legion_pool_state_bytes(self.handle))

    def error(self):
        """Sticky LG_ERR_* bits raised on the device for this pool (0 = none)."""
        return int(self._lib.legion_pool_error(self.handle))

    def profile_begin(self, max_ops):
        self._lib.legion_pool_profile_begin(self.handle, int(max_ops))

    def profile_end(self, max_ops):
        """(ms, op_id) arrays of the gathers timed since profile_begin; synchronise the stream first."""
        ms = (ctypes.c_float * max_ops)()
        ops = (ctypes.c_int32 * max_ops)()
        n = self._lib.legion_pool_profile_end(self.handle, ms, ops, int(max_ops))
        return np.array(ms[:n], dtype=np.float64), np.array(ops[:n], dtype=np.int32)

    def close(self):
        if self.handle and not getattr(self, "_borrowed_handle", False):
            self._lib.legion_pool_destroy(self.handle)
        self.handle = None


class LaneGroup:
    """G pools served by every launch (grid.y = G); lane i produces batch counter0 + i."""

    def __init__(self, pools):
        self._lib = _libmod.load()
        self.pools = list(pools)
        arr = (ctypes.c_void_p * len(self.pools))(*[p.handle for p in self.pools])
        self.handle = self._lib.legion_group_create(arr, len(self.pools))

    def enqueue(self, strm_hdl, graph, feature, cache, batch_size, counter0, dev_id, mode, fanout):
        self._lib.legion_enqueue_group(_stream_handle(strm_hdl), graph.handle, feature.handle,
                                       cache.handle if cache else None, self.handle, int(batch_size), int(counter0),
                                       int(dev_id), int(mode), _i32_array(fanout), len(fanout))

    def close(self):
        if self.handle:
            self._lib.legion_group_destroy(self.handle)
            self.handle = None


def collective_unique_id():
    """128 bytes that rank 0 creates and every rank needs for collective_init_rank (carry them over any channel)."""
    buf = ctypes.create_string_buffer(128)
    if not _libmod.load().legion_collective_unique_id(buf):
        raise RuntimeError("ncclGetUniqueId failed")
    return buf.raw


def collective_init_rank(unique_id, world, rank, dev_id=0):
    """Joins the library's own RCCL communicator (the hotness all-reduce of a one-process-per-GPU deployment)."""
    return bool(_libmod.load().legion_collective_init_rank(ctypes.create_string_buffer(unique_id, 128), int(world), int(rank), int(dev_id)))


def collective_destroy():
    _libmod.load().legion_collective_destroy()


class Pipeline:
    """`slots` groups of `group_size` mini-batches in flight on one GPU, each group replayed as one
    hipGraph (pipeline.hip).  submit(counter0) enqueues batches counter0 .. counter0+group_size-1.
    arena: False = every lane's arrays are allocations of their own; True = all lanes' trainer-visible arrays in ONE arena built from
    shuffled physical chunks (LegionTuning.arena_scatter_mb: the gathers' rows land all over the HBM); "shared" = an arena that other GPUs and
    processes can reach (peer_gather = bulk: owners push rows into it) -- the same shuffled chunks, created exportable; other GPUs of this
    process are granted access at bulk_link, other processes map them from file descriptors at bulk_import ("plain": the old name)."""

    def __init__(self, graph, feature, cache, dev_id, batch_size, fanout, group_size, feature_rows, use_graph=True,
                 slots=2, overlap=False, split=False, weave=False, arena=False,      # (split: accepted and ignored -- removed in round 5)
                 feature_out_dtype="float32", replace=True, edge_ids=False, weighted=False):
        """replace: MemoryPool's (every lane samples with / without replacement).  edge_ids: MemoryPool's (every lane records its
        edges' ids).  weighted: MemoryPool's (every lane picks by the graph's edge weights)."""
        if feature_out_dtype not in FEATURE_DTYPES:
            raise ValueError(f"feature_out_dtype must be one of {sorted(FEATURE_DTYPES)}, not {feature_out_dtype!r}")
        if not isinstance(edge_ids, bool):
            raise ValueError(f"edge_ids must be True or False, not {edge_ids!r}")
        if not isinstance(weighted, bool):
            raise ValueError(f"weighted must be True or False, not {weighted!r}")
        self._lib = _libmod.load()
        self.group_size, self.slots = int(group_size), int(slots)
        self.fanout = [int(f) for f in fanout]
        self.handle = self._lib.legion_pipeline_create_ex(graph.handle, feature.handle, cache.handle, int(dev_id),
                                                          int(batch_size), _i32_array(self.fanout), len(self.fanout),
                                                          self.group_size, self.slots, int(feature_rows),
                                                          (1 if use_graph else 0) | (2 if overlap else 0) | (4 if split else 0) |
                                                          (16 if weave else 0) | (32 if arena else 0) | (64 if arena in ("shared", "plain") else 0),
                                                          FEATURE_DTYPES[feature_out_dtype])
        self.pools = [[MemoryPool._borrowed(self._lib.legion_pipeline_pool(self.handle, s, g), dev_id,
                                            feature.total_num_nodes, batch_size, fanout, feature.float_feature_len,
                                            feature_rows) for g in range(self.group_size)]
                      for s in range(self.slots)]
        if not replace:
            self.set_replace(False)
        if edge_ids:
            self.set_edge_ids(True)
        if weighted:
            self.set_weighted(True)

    def set_replace(self, replace):
        """Only before the first submit (the C ABI refuses it after: RuntimeError)."""
        _set_sample_mode(self, "legion_pipeline_set_sample_replace", "replace", replace, (bool, int),
                         "the pipeline has sampled already, or a fan-out is above 256 without replacement, or the pipeline is weighted")

    @property
    def edge_ids(self):
        return all(pool.edge_ids for lanes in self.pools for pool in lanes)

    def set_edge_ids(self, on):
        """Only before the first submit (the C ABI refuses it after: RuntimeError)."""
        _set_sample_mode(self, "legion_pipeline_set_edge_ids", "edge_ids", on, bool, "the pipeline has sampled already")

    @property
    def weighted(self):
        return all(pool.weighted for lanes in self.pools for pool in lanes)

    def set_weighted(self, on):
        """Only before the first submit, and only with replace=True (the C ABI refuses it otherwise: RuntimeError)."""
        _set_sample_mode(self, "legion_pipeline_set_sample_weighted", "weighted", on, bool,
                         "the pipeline has sampled already, or it samples without replacement")

    def submit(self, counter0, mode=TRAINMODE, n_active=None):
        if n_active is None or n_active >= self.group_size:
            return int(self._lib.legion_pipeline_submit(self.handle, int(counter0), int(mode)))
        return int(self._lib.legion_pipeline_submit_n(self.handle, int(counter0), int(mode), int(n_active)))

    def run_range(self, first, count, mode=TRAINMODE, wrap=None):
        """Submits batches first .. first+count-1 as full groups plus, if needed, one partial group.
        `wrap` (a number of batches): batch indices are taken modulo it -- another epoch over the same seed set, as
        the reference's schedule does with GetLocalBatchId (ipc_service.cu:213-228); a group never straddles the wrap.
        Returns (slot, first batch, lanes) of the last group submitted."""
        k, last = 0, None
        while k < count:
            b = (first + k) % wrap if wrap else first + k
            n = min(self.group_size, count - k, (wrap - b) if wrap else count)
            last = (self.submit(b, mode, n), b, n)
            k += n
        return last

    def wait(self, slot=-1):
        self._lib.legion_pipeline_wait(self.handle, int(slot))

    # ---- peer_gather = bulk (pipeline.hip): owner-bucketed transfer of the rows a striped gather needs from other members ----
    def bulk_enable(self):
        """Needs arena="shared".  Allocates this GPU's per-owner request lists (one set per slot)."""
        if not self._lib.legion_pipeline_bulk_enable(self.handle):
            raise RuntimeError("legion_pipeline_bulk_enable failed (pipeline not created with arena='plain'?)")

    def bulk_export(self):
        """Bytes the other members need (IPC handles of the lane arena and the lists)."""
        buf = ctypes.create_string_buffer(512)
        n = int(self._lib.legion_pipeline_bulk_export(self.handle, buf, 512))
        if n <= 0:
            raise RuntimeError("legion_pipeline_bulk_export failed")
        return buf.raw[:n]

    def bulk_import(self, handles):
        """A member in ANOTHER process."""
        if not self._lib.legion_pipeline_bulk_import(self.handle, ctypes.create_string_buffer(handles, len(handles))):
            raise RuntimeError("legion_pipeline_bulk_import failed")

    def bulk_link(self, other):
        """A member in THIS process (logical GPUs of a test, a thread per GPU)."""
        if not self._lib.legion_pipeline_bulk_link(self.handle, other.handle):
            raise RuntimeError("legion_pipeline_bulk_link failed")

    def bulk_phase_a(self, counter0, mode=TRAINMODE, n_active=None, batch_size=0):
        """Sampler + bucket pass + gather of everything that is not another member's stripe; returns the slot.  The caller
        barriers over the clique, calls bulk_phase_b(slot) on every member, and barriers again."""
        return int(self._lib.legion_pipeline_bulk_phase_a(self.handle, int(counter0), int(mode),
                                                          int(n_active) if n_active else self.group_size, int(batch_size)))

    def bulk_phase_b(self, slot):
        self._lib.legion_pipeline_bulk_phase_b(self.handle, int(slot))

    def bulk_listed(self, slot):
        """Rows this GPU listed for other members in `slot` (what phase B sends towards it)."""
        return int(self._lib.legion_pipeline_bulk_listed(self.handle, int(slot)))

    def profile_begin(self):
        self._lib.legion_pipeline_profile_begin(self.handle)

    def profile_end(self):
        self._lib.legion_pipeline_profile_end(self.handle)

    def regather_last(self, slot, repeats=5, n_active=0):
        """The last op's gather of the group sitting in `slot`, `repeats` more times over the lanes as they stand: ms per launch
        (HIP events on the slot's stream).  legion_hip.h: legion_pipeline_regather_last."""
        ms = (ctypes.c_double * int(repeats))()
        n = self._lib.legion_pipeline_regather_last(self.handle, int(slot), int(n_active), int(repeats), ms)
        return [float(ms[i]) for i in range(n)]

    def profile_read(self):
        """{gather op id: (summed ms, launches)} for every batch waited for since profile_begin()."""
        ops = (ctypes.c_int32 * 16)()
        ms = (ctypes.c_double * 16)()
        cnt = (ctypes.c_int64 * 16)()
        n = self._lib.legion_pipeline_profile_read(self.handle, ops, ms, cnt, 16)
        return {int(ops[i]): (float(ms[i]), int(cnt[i])) for i in range(n)}

    def close(self):
        if self.handle:
            self._lib.legion_pipeline_destroy(self.handle)
            self.handle = None


class UnifiedCache:
    _ARR = {"QF": (0, torch.int32), "QT": (1, torch.int32), "AF": (2, torch.int64), "AT": (3, torch.int64),
            "node_access_time": (4, torch.int64), "edge_access_time": (5, torch.int64),
            "node_map": (6, torch.int32), "edge_index_map": (7, torch.int8), "edge_offset_map": (8, torch.int32)}

    def __init__(self, cache_memory, float_feature_len, train_step, device_count, total_num_nodes):
        self._lib = _libmod.load()
        self.device_count = int(device_count)
        self.total_num_nodes = int(total_num_nodes)
        self.handle = self._lib.legion_cache_create(int(cache_memory), int(float_feature_len), int(train_step),
                                                    self.device_count, self.total_num_nodes)

    def init_controller(self, dev_id):
        self._lib.legion_cache_init_controller(self.handle, int(dev_id))

    def candidate_selection(self, cache_agg_mode, graph, world_reduced=False):
        self._lib.legion_cache_candidate_selection(self.handle, int(cache_agg_mode), graph.handle,
                                                   1 if world_reduced else 0)

    def allreduce_hotness(self, dev_id=0):
        """One process per GPU: RCCL all-reduce (issued by the library, collective_init_rank's communicator) of this GPU's two
        access-counter arrays in place.  Returns (world size the collective ran over -- 0 on failure --, milliseconds)."""
        ms = ctypes.c_double(0)
        world = int(self._lib.legion_cache_allreduce_hotness(self.handle, int(dev_id), ctypes.byref(ms)))
        return world, float(ms.value)

    def hotness_reduce_path(self, dev_id=0):
        """How the last candidate_selection summed the clique's counters: 'none', 'p2p' (leader loop) or 'rccl'."""
        return ("none", "p2p", "rccl")[int(self._lib.legion_cache_hotness_reduce_path(self.handle, int(dev_id)))]

    def cost_model(self, feature, graph, counters=(0, 0), train_step=0):
        cnt = (ctypes.c_uint64 * 2)(int(counters[0]), int(counters[1]))
        self._lib.legion_cache_cost_model(self.handle, feature.handle, graph.handle, cnt, int(train_step))

    def set_replica_memory(self, nbytes):
        """Every member of a striped clique also keeps the clique's hottest rows locally, as many as nbytes hold."""
        self._lib.legion_cache_set_replica_memory(self.handle, int(nbytes))

    def replica_rows(self, dev_id=0):
        return int(self._lib.legion_cache_replica_rows(self.handle, int(dev_id)))

    def gather_stats(self, dev_id=0):
        """(rows read through a stripe pointer, rows read from the local replica) so far; the first call enables counting."""
        out = (ctypes.c_uint64 * 2)()
        self._lib.legion_cache_gather_stats(self.handle, int(dev_id), out)
        return int(out[0]), int(out[1])

    def gather_stats3(self, dev_id=0):
        """(rows through a stripe pointer, rows from the local replica, rows from a PEER's stripe) so far."""
        out = (ctypes.c_uint64 * 3)()
        self._lib.legion_cache_gather_stats3(self.handle, int(dev_id), out)
        return int(out[0]), int(out[1]), int(out[2])

    def gather_stats_enable(self, on):
        self._lib.legion_cache_gather_stats_enable(self.handle, 1 if on else 0)

    def peer_transactions(self, dev_id=0):
        """64-byte transactions read from other members' stripes so far (the computed stand-in for the xGMI counter)."""
        return int(self._lib.legion_cache_peer_transactions(self.handle, int(dev_id)))

    def set_capacity(self, node_capacity, edge_capacity):
        self._lib.legion_cache_set_capacity(self.handle, int(node_capacity), int(edge_capacity))

    def fill_up(self, feature, graph):
        self._lib.legion_cache_fill_up(self.handle, feature.handle, graph.handle)

    def hybrid_init(self, feature, graph, cpu_cache_capacity, gpu_cache_capacity, miss_from_table=True):
        """The hybrid CPU-cache / GPU-cache tier instead of candidate_selection + cost_model + fill_up
        (UnifiedCache::HybridInit, SS/cache/cache.cu:614-670)."""
        self._hybrid = (int(cpu_cache_capacity), int(gpu_cache_capacity), int(feature.float_feature_len))
        self._lib.legion_cache_hybrid_init(self.handle, feature.handle, graph.handle, int(cpu_cache_capacity),
                                           int(gpu_cache_capacity), 1 if miss_from_table else 0)

    def hybrid_caches(self, dev_id=0):
        """(CPU cache, GPU cache) of dev_id after hybrid_init as float32 tensors [capacity, D] (device views)."""
        cpu_cap, gpu_cap, dim = self._hybrid
        dev = _torch_device(dev_id)
        cpu = device_view(self._lib.legion_cache_hybrid_cpu_cache(self.handle, int(dev_id)), (cpu_cap, dim), torch.float32, dev)
        gpu = device_view(self._lib.legion_cache_feature_cache(self.handle, int(dev_id)), (gpu_cap, dim), torch.float32, dev)
        return cpu, gpu

    def fill_up_distributed(self, feature, graph, rank, world, max_ids_all, all_gather_bytes):
        """FillUp of a clique spread over `world` processes (this process owns member `rank`):
        local stripe -> export 3 IPC handles -> all-gather -> open the peers' -> link.
        `all_gather_bytes(b: bytes) -> list[bytes]` is the caller's collective (torch.distributed)."""
        self._lib.legion_cache_fill_up_local(self.handle, feature.handle, graph.handle)
        mine = ctypes.create_string_buffer(192)
        self._lib.legion_cache_export(self.handle, graph.handle, int(rank), mine)
        everyone = all_gather_bytes(mine.raw)
        self._peer_handles = [ctypes.create_string_buffer(b, 192) for b in everyone]
        for peer in range(world):
            if peer != rank:
                self._lib.legion_cache_import_peer(self.handle, graph.handle, int(rank), peer, self._peer_handles[peer])
        self._lib.legion_cache_fill_up_link(self.handle, feature.handle, graph.handle)

    def set_peer_max_ids(self, max_ids_all):
        arr = _i32_array(max_ids_all)
        self._lib.legion_cache_set_peer_max_ids(self.handle, arr, len(max_ids_all))

    def node_capacity(self, dev_id=0):
        return int(self._lib.legion_cache_node_capacity(self.handle, int(dev_id)))

    def edge_capacity(self, dev_id=0):
        return int(self._lib.legion_cache_edge_capacity(self.handle, int(dev_id)))

    def max_id_num(self, dev_id=0):
        return int(self._lib.legion_cache_max_id_num(self.handle, int(dev_id)))

    def topo_transactions(self, dev_id):
        """64-byte transactions of GPU dev_id's PreSC topology reads (the PCM counter of the paper; see legion_hip.h)."""
        return int(self._lib.legion_cache_topo_transactions(self.handle, int(dev_id)))

    def find_topo(self, dev_id, input_ids):
        """(partition_index int8, partition_offset int32) for a device int32 tensor of vertex ids."""
        n = int(input_ids.numel())
        ind = torch.empty(n, dtype=torch.int8, device=input_ids.device)
        off = torch.empty(n, dtype=torch.int32, device=input_ids.device)
        self._lib.legion_cache_find_topo(self.handle, int(dev_id), _stream_handle(None), _ptr(input_ids), n,
                                         _ptr(ind), _ptr(off))
        return ind, off

    def array(self, name, dev_id=0):
        which, dtype = self._ARR[name]
        ptr = self._lib.legion_cache_array(self.handle, int(dev_id), which)
        return device_view(ptr, (self.total_num_nodes,), dtype, _torch_device(dev_id))

    def close(self):
        if self.handle:
            self._lib.legion_cache_destroy(self.handle)
            self.handle = None


# ---- the five operators, reference names and argument order ------------------------------------
def BatchGenerate(strm_hdl, feature, cache, memorypool, batch_size, counter, part_id, dev_id, mode,
                  is_presc, hop_num):
    _libmod.load().BatchGenerate(_stream_handle(strm_hdl), feature.handle, cache.handle if cache else None,
                                 memorypool.handle, int(batch_size), int(counter), int(part_id), int(dev_id),
                                 int(mode), bool(is_presc), int(hop_num))


def RandomSample(strm_hdl, graph, cache, memorypool, count, dev_id, op_id, is_presc):
    _libmod.load().RandomSample(_stream_handle(strm_hdl), graph.handle, cache.handle if cache else None,
                                memorypool.handle, int(count), int(dev_id), int(op_id), bool(is_presc))


def FeatureCacheLookup(strm_hdl, cache, memorypool, op_id, dev_id):
    _libmod.load().FeatureCacheLookup(_stream_handle(strm_hdl), cache.handle, memorypool.handle, int(op_id),
                                      int(dev_id))


def IOSubmit(strm_hdl, feature, memorypool, op_id, dev_id):
    _libmod.load().IOSubmit(_stream_handle(strm_hdl), feature.handle, memorypool.handle, int(op_id), int(dev_id))


def IOComplete(strm_hdl, cache, memorypool, dev_id, mode):
    _libmod.load().IOComplete(_stream_handle(strm_hdl), cache.handle if cache else None, memorypool.handle,
                              int(dev_id), int(mode))


def enqueue_batch(strm_hdl, graph, feature, cache, memorypool, batch_size, counter, dev_id, mode, is_presc,
                  fanout):
    """All ops of one mini-batch in GPURunner::RunOnce order (SS/engine/server.cu:302-332)."""
    _libmod.load().legion_enqueue_batch(_stream_handle(strm_hdl), graph.handle, feature.handle,
                                        cache.handle if cache else None, memorypool.handle, int(batch_size),
                                        int(counter), int(dev_id), int(mode), bool(is_presc),
                                        _i32_array(fanout), len(fanout))


def read_batch(memorypool):
    """Host copy of everything a trainer (and the parity tests) can observe about the current batch."""
    nc = memorypool.buffer("node_counter").cpu().numpy().copy()
    ec = memorypool.buffer("edge_counter").cpu().numpy().copy()
    hop_num = int(nc[INTRABATCH_CON * 3 - 1])
    n_nodes = int(nc[INTRABATCH_CON * 3 + hop_num])
    n_edges = int(ec[INTRABATCH_CON * 3 + hop_num])
    out = {"node_counter": nc, "edge_counter": ec, "hop_num": hop_num,
           "sampled_ids": memorypool.buffer("sampled_ids")[:max(n_nodes, 0)].cpu().numpy().copy(),
           "labels": memorypool.buffer("labels")[:max(int(nc[INTRABATCH_CON * 3]), 0)].cpu().numpy().copy(),
           "agg_src_off": memorypool.buffer("agg_src_off")[:n_edges].cpu().numpy().copy(),
           "agg_dst_off": memorypool.buffer("agg_dst_off")[:n_edges].cpu().numpy().copy(),
           "agg_src_ids": memorypool.buffer("agg_src_ids")[:n_edges].cpu().numpy().copy(),
           "agg_dst_ids": memorypool.buffer("agg_dst_ids")[:n_edges].cpu().numpy().copy()}
    if memorypool.edge_ids:
        out["agg_edge_ids"] = memorypool.buffer("agg_edge_ids")[:n_edges].cpu().numpy().copy()
    if memorypool.feature_rows > 0:
        rows = memorypool.buffer("float_features")[:max(n_nodes, 0)]     # (the batch past the end counts a negative size)
        if rows.dtype == torch.bfloat16:     # (numpy has no bfloat16: the rows' bits, as uint16)
            rows = rows.view(torch.int16)
        out["float_features"] = rows.cpu().numpy().copy()
        if out["float_features"].dtype == np.int16:
            out["float_features"] = out["float_features"].view(np.uint16)
    return out
