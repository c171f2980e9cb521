"""The feature gather (legion_amd/csrc/kernels_gather.hip, legion_gather_rows_fmt) stated in numpy on bit patterns: float32 values
are uint32, bf16 values uint16, so that NaN payloads, signed zeros and subnormals compare like any other value.

    rows = min(cnt, max_rows, dst_rows - off)
    for r in 0 .. rows-1:
        id = ids[off + r]
        g  = node_slot[off + r]                  where slots are carried (and there is a node_map) and the value is not UNKNOWN
             node_map[id]                        else, where there is a node_map and id >= 0
             MISS                                else
        cache_index[r] = g
        g >= 0          : dst[off + r] = convert(caches[g // cap][g % cap])
        g < 0, id >= 0  : dst[off + r] = convert(table[id % N])          (where a table is given)
        g < 0, id < 0   : the row is left as it is
Source rows of bf16 tables are pitch(D) elements long; only their first D elements are ever stored.  dst rows are D elements."""
import numpy as np

F32, BF16 = 0, 1                 # LEGION_FEATURE_*
MISS, UNKNOWN = -2, -3           # CACHEMISS_FLAG, LG_FS_UNKNOWN
FORMATS = ("F32", "F32Tail", "F32Scalar", "Bf16x8", "Bf16Copy", "F32Narrow")     # GatherFormat, in plan_out's numbering
BITS = {F32: np.uint32, BF16: np.uint16}


def pitch(dtype, D):
    """Elements between two stored rows: bf16 rows are padded to 8 elements (16 bytes)."""
    return (D + 7) // 8 * 8 if dtype == BF16 else D


def widen(b16):
    """bf16 -> float32: exact."""
    return np.asarray(b16, dtype=np.uint16).astype(np.uint32) << np.uint32(16)


def narrow(b32):
    """float32 -> bf16, the rule of kernels_cache.hip: round to nearest even on the bit pattern (subnormals like any other value,
    finite values past the largest bf16 become +-inf); NaNs keep sign and top payload bits and get the quiet bit."""
    u = np.asarray(b32, dtype=np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    rne = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, rne).astype(np.uint16)


def convert(src, dtype, out_dtype):
    if dtype == out_dtype:
        return src
    return widen(src) if dtype == BF16 else narrow(src)


def expected_format(dtype, out_dtype, D):
    """The row format gather_plan.h gives a launch (an index into FORMATS)."""
    if out_dtype == BF16:
        return FORMATS.index("Bf16Copy" if dtype == BF16 else "F32Narrow")
    if dtype == BF16:
        return FORMATS.index("Bf16x8")
    return FORMATS.index("F32" if D % 4 == 0 else "F32Tail" if D > 4 else "F32Scalar")


def lookup(node_map, ids, node_slot, off, rows):
    """g of rows off .. off + rows - 1."""
    i = ids[off:off + rows].astype(np.int64)
    if node_map is None:
        return np.full(rows, MISS, dtype=np.int32)
    g = np.where(i >= 0, node_map[np.maximum(i, 0)], MISS).astype(np.int32)
    if node_slot is not None:
        c = node_slot[off:off + rows]
        g = np.where(c != UNKNOWN, c, g).astype(np.int32)
    return g


def gather(dtype, out_dtype, D, table, caches, node_map, cap, ids, node_slot, off, cnt, max_rows, dst_rows, dst, cache_index):
    """Returns (dst, cache_index) after the gather; the arguments are left as they are.  table: [N, pitch] bits or None; caches: a
    list of [cap, pitch] bits; dst: [any, D] bits of out_dtype; cache_index: int32."""
    dst, cache_index = dst.copy(), cache_index.copy()
    assert dst.dtype == BITS[out_dtype] and dst.shape[1] == D and all(c.shape == (cap, pitch(dtype, D)) for c in caches)
    rows = min(cnt, max_rows, dst_rows - off)
    if rows <= 0 or D <= 0:
        return dst, cache_index
    i = ids[off:off + rows].astype(np.int64)
    g = lookup(node_map, ids, node_slot, off, rows)
    cache_index[:rows] = g
    out = dst[off:off + rows]
    hit = g >= 0
    if hit.any():
        stripes = np.concatenate(caches)               # row (g // cap) * cap + g % cap = g
        out[hit] = convert(stripes[g[hit]][:, :D], dtype, out_dtype)
    miss = (g < 0) & (i >= 0)
    if table is not None and miss.any():
        out[miss] = convert(table[i[miss] % table.shape[0]][:, :D], dtype, out_dtype)
    return dst, cache_index


def gather_loop(dtype, out_dtype, D, table, caches, node_map, cap, ids, node_slot, off, cnt, max_rows, dst_rows, dst, cache_index):
    """The same, one row and one element at a time (tests/test_gather_ref_cpu.py holds gather() against it)."""
    dst, cache_index = dst.copy(), cache_index.copy()
    rows = cnt
    if rows > max_rows:
        rows = max_rows
    if rows > dst_rows - off:
        rows = dst_rows - off
    for r in range(rows):
        v = int(ids[off + r])
        g = UNKNOWN
        if node_slot is not None and node_map is not None:
            g = int(node_slot[off + r])
        if g == UNKNOWN:
            g = int(node_map[v]) if node_map is not None and v >= 0 else MISS
        cache_index[r] = g
        if g >= 0:
            src = caches[g // cap][g % cap]
        elif v >= 0 and table is not None:
            src = table[v % table.shape[0]]
        else:
            continue
        for k in range(D):
            b = int(src[k])
            if dtype == BF16 and out_dtype == F32:
                b = b << 16
            elif dtype == F32 and out_dtype == BF16:
                if (b & 0x7FFFFFFF) > 0x7F800000:
                    b = (b >> 16) | 0x40
                else:
                    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
            dst[off + r, k] = b
    return dst, cache_index


# float32 bit patterns a conversion gets wrong first (those of tests/test_gpu_feature_bf16.py, and NaNs)
SPECIAL = np.array([0x00000000, 0x80000000,                                                             # +-0
                    0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00018000, 0x00007FFF,   # subnormals
                    0x3F808000, 0x3F818000, 0x3F80C000, 0x3F817FFF, 0xBF808000,                          # ties / near ties
                    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000,                                      # FLT_MAX, past the bf16 maximum
                    0x7F800000, 0xFF800000], dtype=np.uint32)                                            # +-inf
NANS = np.array([0x7F800001, 0xFF800001, 0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F807FFF, 0x7FBFFFFF, 0x7F80FFFF,
                 0xFF808000], dtype=np.uint32)
AWKWARD = np.concatenate([SPECIAL, NANS])
POISON = np.uint16(0x7FA5)       # a NaN: what the pad elements of the tests' bf16 tables hold


def awkward_rows(n, D):
    """n rows of D float32 bit patterns that walk through AWKWARD, each row starting one value further."""
    k = (np.arange(n)[:, None] + np.arange(D)[None, :]) % AWKWARD.size
    return AWKWARD[k]


def stored(bits32, dtype):
    """A float32 table (bits) as it is stored in `dtype`: itself, or narrowed rows of pitch elements whose pad holds POISON."""
    if dtype == F32:
        return bits32
    n, D = bits32.shape
    out = np.full((n, pitch(BF16, D)), POISON, dtype=np.uint16)
    out[:, :D] = narrow(bits32)
    return out
