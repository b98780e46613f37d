"""nbxReduceMultiWideMxBatch without a GPU: the symbol, the wrapper, the tile
constant, and every argument check before any device call (fake pointers, as
tests/test_wide_mx_cpu.py)."""
import pytest

E = 4   # ncclInvalidArgument
F32, BF16, E4M3, E5M2, FP4 = 7, 9, 10, 11, 32
FAKE = 0x100000


def bucket(k, scaled=False, out32=False, count=64, **over):
    """Bucket k's own 64 KiB of fake address space: (dsts, dst_scales, srcs, src_scales, count)."""
    b = FAKE + k * 0x10000
    f = dict(dsts=[b], dscales=None if out32 else [b + 0x1000], srcs=[b + 0x2000, b + 0x3000],
             sscales=[b + 0x4000, b + 0x5000] if scaled else None)
    f.update(over)
    return f["dsts"], f["dscales"], f["srcs"], f["sscales"], count


def call(nbx, buckets, st=BF16, dt=E4M3, op=None):
    return nbx.reduce_multi_wide_mx_batch_raw(buckets, st, dt, op or nbx.DevRedOpFull())


def test_symbol_wrapper_and_constants(nbx):
    lib = nbx.load_library()
    assert hasattr(lib, "nbxReduceMultiWideMxBatch") and callable(nbx.reduce_multi_wide_mx_batch)
    assert nbx.mx_batch_tile_elts() == lib.nbxDebugMxBatchTileElts() == 4096
    assert nbx.LaunchFamily.MxBatchList == 21
    assert lib.nbxAbiVersion() == 1 and lib.nbxKernelCount() == 6 * 5 + 6 * 4   # tables of its own


def test_no_ops_after_the_type_checks(nbx):
    assert call(nbx, []) == 0 and call(nbx, [], st=E4M3, dt=F32) == 0
    assert call(nbx, [bucket(k, count=0) for k in range(3)]) == 0
    assert call(nbx, [bucket(0, count=0, srcs=[0, 1], dsts=[3])]) == 0        # an empty bucket's entries: unexamined
    assert call(nbx, [], st=F32) == E and call(nbx, [], dt=BF16) == E and call(nbx, [], dt=F32) == E


@pytest.mark.parametrize("case", ["mixed", "mixed-empty", "fp4-src", "fp4-dst", "negative", "null-tasks", "bad-op",
                                  "null-scalar", "null-scale", "null-dst-scale", "overlap", "in-place-scales",
                                  "misaligned", "no-dst-scales", "plain-to-fp32"])
def test_checks_come_before_any_device_call(nbx, case):
    lib, op = nbx.load_library(), nbx.DevRedOpFull()
    good, mx = [bucket(0), bucket(1)], [bucket(0, True), bucket(1, True)]
    if case == "mixed":
        rc = call(nbx, [bucket(0, True), bucket(1)], st=E4M3)
    elif case == "mixed-empty":
        rc = call(nbx, [bucket(0), bucket(1, True, count=0)], st=E4M3)
    elif case in ("fp4-src", "fp4-dst"):
        rc = call(nbx, good, **({"st": FP4} if case == "fp4-src" else {"dt": FP4}))
    elif case == "negative":
        rc = lib.nbxReduceMultiWideMxBatch(nbx._reduce_mx_tasks(good)[0], -1, BF16, E4M3, op, 0, None)
    elif case == "null-tasks":
        rc = lib.nbxReduceMultiWideMxBatch(None, 2, BF16, E4M3, op, 0, None)
    elif case == "bad-op":
        op.op = 1   # Prod
        rc = call(nbx, good, op=op)
    elif case == "null-scalar":
        op.op, op.scalarArgIsPtr = 3, 1
        rc = call(nbx, good, op=op)
    elif case == "null-scale":        # in bucket 1, behind a good one
        rc = call(nbx, [mx[0], bucket(1, True, sscales=[FAKE + 0x14000, 0])], st=E4M3)
    elif case == "null-dst-scale":
        rc = call(nbx, [good[0], bucket(1, dscales=[0])])
    elif case == "overlap":           # bucket 1's destination partly on its second source
        rc = call(nbx, [good[0], bucket(1, dsts=[FAKE + 0x13000 + 16])], st=E4M3)
    elif case == "in-place-scales":   # in place, but not on the source's own scale array
        rc = call(nbx, [mx[0], bucket(1, True, dsts=[FAKE + 0x12000])], st=E4M3)
    elif case == "misaligned":        # an odd bf16 source
        rc = call(nbx, [good[0], bucket(1, srcs=[FAKE + 0x12001, FAKE + 0x13000])])
    elif case == "no-dst-scales":     # an MX output without scale arrays
        rc = call(nbx, [good[0], bucket(1, dscales=None)])
    else:                             # fp32 output is for scaled sources only
        rc = call(nbx, [bucket(0, out32=True), bucket(1, out32=True)], st=E4M3, dt=F32)
    assert rc == E
