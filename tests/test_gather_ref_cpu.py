"""tests/gather_ref.py is what tests/test_gpu_gather_formats.py holds every gather instance against, so it is pinned here without a
GPU: the vectorised gather against a row-by-row loop at tiny sizes, the narrowing against torch's float32 -> bfloat16."""
import numpy as np
import pytest
import torch

from tests import gather_ref as ref


def torch_bf16_bits(bits32):
    return torch.from_numpy(bits32.view(np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_narrow_is_torchs_rounding_on_random_bit_patterns():
    rng = np.random.RandomState(11)
    bits = rng.randint(0, 2 ** 32, size=1 << 21, dtype=np.uint64).astype(np.uint32)
    bits = bits[(bits & 0x7FFFFFFF) <= 0x7F800000]              # NaNs: by class, below
    # every exponent with the mantissa patterns around a tie
    exps = (np.arange(256, dtype=np.uint32) << 23)[:, None]
    ties = np.array([0x7FFF, 0x8000, 0x8001, 0x17FFF, 0x18000, 0x18001, 0x7F7FFF, 0x7F8000, 0x7FFFFF, 0], dtype=np.uint32)[None, :]
    around = (exps | ties).ravel()
    around = np.concatenate([around, around | np.uint32(0x80000000)])
    around = around[(around & 0x7FFFFFFF) <= 0x7F800000]
    for x in (bits, around, ref.SPECIAL):
        assert np.array_equal(ref.narrow(x), torch_bf16_bits(x))


def test_narrow_special_values_stated():
    want = {0x00000000: 0x0000, 0x80000000: 0x8000, 0x00000001: 0x0000, 0x007FFFFF: 0x0080, 0x00008000: 0x0000, 0x00018000: 0x0002,
            0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3F80C000: 0x3F81, 0x3F817FFF: 0x3F81, 0x7F7FFFFF: 0x7F80, 0xFF7FFFFF: 0xFF80,
            0x7F7F7FFF: 0x7F7F, 0x7F7F8000: 0x7F80, 0x7F800000: 0x7F80, 0xFF800000: 0xFF80}
    for x, y in want.items():
        assert int(ref.narrow(np.array([x], dtype=np.uint32))[0]) == y, hex(x)


def test_narrow_keeps_nans_quiet_with_sign_and_top_payload():
    got = ref.narrow(ref.NANS)
    t = torch_bf16_bits(ref.NANS)
    assert np.all((got & 0x7FFF) > 0x7F80) and np.all((t & 0x7FFF) > 0x7F80)          # NaN in, NaN out: both
    assert np.array_equal(got & 0x8000, (ref.NANS >> 16) & 0x8000)                    # sign
    assert np.array_equal(got, ((ref.NANS >> 16) | 0x40).astype(np.uint16))           # top payload bits, quiet bit
    rng = np.random.RandomState(12)
    nans = (rng.randint(1, 1 << 23, size=100000).astype(np.uint32) | np.uint32(0x7F800000) |
            (rng.randint(0, 2, size=100000).astype(np.uint32) << 31))
    assert np.all((ref.narrow(nans) & 0x7FFF) > 0x7F80) and np.all((torch_bf16_bits(nans) & 0x7FFF) > 0x7F80)


def test_widen_is_exact_and_inverts_narrow_on_bf16_values():
    b = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    w = ref.widen(b)
    assert w.dtype == np.uint32 and np.array_equal(w >> 16, b) and not np.any(w & 0xFFFF)
    t = torch.from_numpy(b.view(np.int16)).view(torch.bfloat16).to(torch.float32).numpy().view(np.uint32)
    num = (b & 0x7FFF) <= 0x7F80
    assert np.array_equal(w[num], t[num])
    assert np.array_equal(ref.narrow(w)[num], b[num])


def test_stored_tables_poison_their_pad():
    bits = ref.awkward_rows(5, 11)
    s = ref.stored(bits, ref.BF16)
    assert s.shape == (5, 16) and np.all(s[:, 11:] == ref.POISON) and np.array_equal(s[:, :11], ref.narrow(bits))
    assert ref.stored(bits, ref.F32) is bits
    assert (ref.POISON & 0x7FFF) > 0x7F80 and [ref.pitch(ref.BF16, d) for d in (1, 8, 9)] == [8, 8, 16] and ref.pitch(ref.F32, 9) == 9


PAIRS = [(ref.F32, ref.F32), (ref.BF16, ref.F32), (ref.BF16, ref.BF16), (ref.F32, ref.BF16)]


def tiny_case(rng, dtype, out_dtype, D, with_map=True, carried=False):
    N, cap, total = 37, 6, 60
    bits = rng.randint(0, 2 ** 32, size=(N, D), dtype=np.uint64).astype(np.uint32)
    bits[:4] = ref.awkward_rows(4, D)
    table = ref.stored(bits, dtype)
    caches = [ref.stored(rng.randint(0, 2 ** 32, size=(cap, D), dtype=np.uint64).astype(np.uint32), dtype) for _ in range(2)]
    node_map = np.full(N, ref.MISS, dtype=np.int32)
    node_map[rng.permutation(N)[:2 * cap]] = rng.permutation(2 * cap)
    ids = rng.randint(0, N, size=total).astype(np.int32)
    ids[::7] = -1
    ids[3:7] = [0, 1, 2, 3]
    slots = None
    if carried:
        slots = np.where(ids >= 0, node_map[np.maximum(ids, 0)], ref.MISS).astype(np.int32)
        slots[::3] = ref.UNKNOWN
        slots[1::9] = rng.randint(0, 2 * cap, size=slots[1::9].size)        # not what node_map says
        slots[4::11] = ref.MISS
    dst = np.full((total, D), 0xBEEF if out_dtype == ref.BF16 else 0xFFC0DEAD, dtype=ref.BITS[out_dtype])
    cidx = np.full(total, 99, dtype=np.int32)
    return (dtype, out_dtype, D, table, caches, node_map if with_map else None, cap, ids, slots), dst, cidx


@pytest.mark.parametrize("dtype,out_dtype", PAIRS)
def test_gather_matches_the_row_loop(dtype, out_dtype):
    rng = np.random.RandomState(100 + 2 * dtype + out_dtype)
    for D in (1, 3, 8, 9, 17):
        for with_map, carried in ((True, False), (True, True), (False, False), (False, True)):
            args, dst, cidx = tiny_case(rng, dtype, out_dtype, D, with_map, carried)
            # off, cnt, max_rows, dst_rows: plain, both clamps, nothing to do, a buffer that ends before the range starts
            for off, cnt, max_rows, dst_rows in ((5, 40, 1000, 1000), (5, 40, 23, 1000), (5, 40, 1000, 31), (5, 0, 9, 60), (5, 40, 50, 3)):
                a = ref.gather(*args, off, cnt, max_rows, dst_rows, dst, cidx)
                b = ref.gather_loop(*args, off, cnt, max_rows, dst_rows, dst, cidx)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (D, with_map, carried, off, cnt, max_rows, dst_rows)
                rows = max(0, min(cnt, max_rows, dst_rows - off))
                sent = dst[0, 0]
                assert np.all(a[0][:off] == sent) and np.all(a[0][off + rows:] == sent) and np.all(a[1][rows:] == 99)
                assert np.all(dst == sent) and np.all(cidx == 99)                   # the arguments are left alone
                if rows:
                    skipped = (args[7][off:off + rows] < 0) & (a[1][:rows] < 0)
                    assert np.all(a[0][off:off + rows][skipped] == sent)
                    if not carried:
                        assert skipped.any() and (with_map is False or (a[1][:rows] >= 0).any())


def test_gather_serves_the_carried_slot_not_the_maps():
    rng = np.random.RandomState(3)
    args, dst, cidx = tiny_case(rng, ref.BF16, ref.F32, 5, True, True)
    _, _, D, table, caches, node_map, cap, ids, slots = args
    out, idx = ref.gather(*args, 0, 60, 60, 60, dst, cidx)
    differ = [r for r in range(60) if slots[r] >= 0 and (ids[r] < 0 or node_map[ids[r]] != slots[r])]
    assert differ
    for r in differ:
        assert idx[r] == slots[r] and np.array_equal(out[r], ref.widen(caches[slots[r] // cap][slots[r] % cap][:D]))
    assert not np.any(out == (np.uint32(ref.POISON) << 16))              # no pad element reaches a row


def test_expected_format():
    f = ref.FORMATS
    assert [f[ref.expected_format(ref.F32, ref.F32, D)] for D in (1, 3, 4, 5, 8, 602)] == \
        ["F32Scalar", "F32Scalar", "F32", "F32Tail", "F32", "F32Tail"]
    assert f[ref.expected_format(ref.BF16, ref.F32, 3)] == "Bf16x8" and f[ref.expected_format(ref.BF16, ref.BF16, 3)] == "Bf16Copy"
    assert f[ref.expected_format(ref.F32, ref.BF16, 4)] == "F32Narrow"
