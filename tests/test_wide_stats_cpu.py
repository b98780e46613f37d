"""nbxReduceMultiWideStats / nbxReduceMultiWideBatchStats without a GPU: the
record's layout, the argument checks (every one before any device call: fake
pointers, as tests/test_wide_batch_cpu.py), and the numpy reference of
tests/widestats on hand-computed vectors."""
import ctypes

import numpy as np
import pytest

E = 4   # ncclInvalidArgument
F32, BF16, E4M3 = 7, 9, 10
PROD, PREMULSUM = 1, 3
FAKE = 0x100000
GOOD = ([FAKE], [FAKE + 4096, FAKE + 8192], 64)
STATS = FAKE + 16384


def single(nbx, stats, dsts=GOOD[0], srcs=GOOD[1], count=64, st=BF16, dt=BF16, op=None):
    return nbx.reduce_multi_wide_stats_raw(dsts, srcs, count, st, dt, op or nbx.DevRedOpFull(), stats)


def batch(nbx, stats, buckets=(GOOD, GOOD), st=BF16, dt=BF16, op=None):
    return nbx.reduce_multi_wide_batch_stats_raw(list(buckets), st, dt, op or nbx.DevRedOpFull(), stats)


def test_record_layout_and_symbols(nbx):
    assert ctypes.sizeof(nbx.WideStats) == 16 and ctypes.alignment(nbx.WideStats) == 8
    assert (nbx.WideStats.sumSq.offset, nbx.WideStats.amax.offset, nbx.WideStats.reserved.offset) == (0, 8, 12)
    lib = nbx.load_library()
    assert hasattr(lib, "nbxReduceMultiWideStats") and hasattr(lib, "nbxReduceMultiWideBatchStats")
    assert lib.nbxAbiVersion() == 1 and lib.nbxKernelCount() == 6 * 5 + 6 * 4   # additive; a table of their own
    assert nbx.LAUNCH_STATS == 8 and nbx.WIDE_STATS_L == 32


@pytest.mark.parametrize("call", [single, batch])
def test_stats_pointer_checks(nbx, call):
    assert call(nbx, 0) == E            # NULL
    assert call(nbx, STATS + 4) == E    # not 8-byte aligned
    assert call(nbx, STATS + 1) == E


def test_inherited_checks_come_before_any_device_call(nbx):
    bad_op = nbx.DevRedOpFull()
    bad_op.op = PROD
    null_scalar = nbx.DevRedOpFull()
    null_scalar.op, null_scalar.scalarArgIsPtr = PREMULSUM, 1
    for call in (single, batch):
        assert call(nbx, STATS, st=F32, dt=F32) == E
        assert call(nbx, STATS, st=BF16, dt=E4M3) == E
        assert call(nbx, STATS, op=bad_op) == E
        assert call(nbx, STATS, op=null_scalar) == E
    assert single(nbx, STATS, srcs=[]) == E
    assert single(nbx, STATS, srcs=[FAKE + 4096] * 65) == E
    assert single(nbx, STATS, srcs=[FAKE + 4097]) == E                       # odd bf16 source
    assert single(nbx, STATS, dsts=[FAKE + 4096], dt=F32) == E               # fp32 destination on its source
    assert batch(nbx, STATS, [GOOD, ([FAKE + 1], [FAKE + 4096], 16)]) == E   # a bad bucket behind a good one
    assert batch(nbx, 0, []) == 0                                            # no buckets: nothing to write
    lib = nbx.load_library()
    assert lib.nbxReduceMultiWideBatchStats(None, 1, BF16, BF16, nbx.DevRedOpFull(), 0, STATS, None) == E


def test_reference_on_hand_computed_vectors():
    from tests.widestats.test_reduce_gpu import check_stats

    def record(sq, amax):
        return np.frombuffer(np.float64(sq).tobytes() + np.float32(amax).tobytes() + bytes(4), np.uint8)

    f = np.float32
    check_stats(record(25.0, 4.0), np.array([3, -4], f))
    check_stats(record(0.0, 0.0), np.array([0.0, -0.0], f))
    check_stats(record(0.0, 0.0), np.zeros(0, f))
    check_stats(record(np.inf, np.inf), np.array([1, -np.inf, 1e30], f))     # inf > every finite value
    check_stats(record(np.nan, np.nan), np.array([1, np.inf, np.nan], f))    # NaN > inf
    check_stats(record(3 * 4.9e9, 70000.0), np.full(3, 70000.0, f))          # beyond fp16's range
    for wrong in (record(25.0, 3.0), record(25.0 * (1 + 2.0 ** -18), 4.0), record(25.0, np.nan)):
        with pytest.raises(AssertionError):
            check_stats(wrong, np.array([3, -4], f))
    with pytest.raises(AssertionError):
        check_stats(record(np.inf, np.inf), np.array([1, np.inf, np.nan], f))
