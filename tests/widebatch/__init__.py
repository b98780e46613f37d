"""What the nbxReduceMultiWideBatch tests share: tests/widebatch/test_reduce_gpu.py
and its CPU companion tests/test_wide_batch_cpu.py.

The buckets are those of tests/batch/cases.py (the table, list_walk,
record_width, small_set through place) over tests/matrix/inputs.py's uploads;
here are only the launch record of kWideBatchList<W, NSRC, OUT32> and the
host's rule for which bucket may enter a batch, restated from
include/nbx_reduce.h so that the tests can say which record a layout leaves.
"""
from tests.batch import cases as bc

FAM_WIDE_PACKS, FAM_WIDE_ELTS, FAM_WIDE_LIST = 6, 7, 15   # include/nbx_debug.h nbxDebugLaunchLog
OUT32, PART_FIRST = 2, 4                                   # flag bits 1 and 2


def records(nsrc, launches, out32):
    """Family-15 records of work-list launches of `launches` buckets each."""
    return [(FAM_WIDE_LIST, nsrc, 1, (OUT32 if out32 else 0) | n << bc.SEGS_SHIFT) for n in launches]


def wide_unroll(nsrc):
    """wideUnroll (nbx_kargs.h): packs per lane per source of kWidePacks."""
    return 4 if nsrc >= 4 else 1


def single_pack_record(nsrc, out32):
    """The record of one bucket of <= 8 sources through nbxReduceMultiWide's pack kernel."""
    return (FAM_WIDE_PACKS, nsrc, wide_unroll(nsrc), OUT32 if out32 else 0)


def eligible(src_addrs, dst_addrs, eb, out32):
    """nbxReduceMultiWide's pack-kernel condition, which is the batch's: all
    sources on one misalignment modulo 16, every destination 16-byte aligned
    behind the head elements (an fp32 one: (dst + 4 * head) % 16 == 0)."""
    mis = src_addrs[0] % 16
    head = (16 - mis) // eb if mis else 0
    deb = 4 if out32 else eb
    return all(a % 16 == mis for a in src_addrs) and all((a + head * deb) % 16 == 0 for a in dst_addrs)


def bucket_eligible(b, eb, out32):
    """`eligible` for a cases.py bucket whose uploads and destination rows
    start on 16-byte boundaries."""
    return eligible([b.start * eb], [b.dstart * (4 if out32 else eb)], eb, out32)
