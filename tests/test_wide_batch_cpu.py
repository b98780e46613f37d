"""nbxReduceMultiWideBatch without a GPU: the symbol is declared, exported and
bound, every argument check returns before any device call (fake pointers, as
tests/test_wide_cpu.py), bucket by bucket, and the case tables of
tests/widebatch/test_reduce_gpu.py are what that file takes them for."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import widebatch as wb
from tests.batch import cases as bc
from tests.matrix import inputs as mi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = 4   # ncclInvalidArgument
F16, F32, F64, BF16, E4M3, E5M2 = 6, 7, 8, 9, 10, 11
SUM, PROD, MINMAX, PREMULSUM, SUMPOSTDIV = range(5)
FAKE = 0x100000
GOOD = ([FAKE], [FAKE + 4096, FAKE + 8192], 64)   # a bucket nothing is wrong with


def batch(nbx, buckets, st=BF16, dt=BF16, op=None, npre=0):
    return nbx.reduce_multi_wide_batch_raw(buckets, st, dt, op if op is not None else nbx.DevRedOpFull(), npre)


def devop(nbx, code, arg=0, is_ptr=0):
    op = nbx.DevRedOpFull()
    op.op, op.scalarArg, op.scalarArgIsPtr = code, arg, is_ptr
    return op


def test_symbol_declared_exported_and_bound(nbx):
    header = open(os.path.join(ROOT, "include", "nbx_reduce.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"ncclResult_t\s+nbxReduceMultiWideBatch\s*\(", code)
    assert "nbxReduceMultiWideBatch" in nbx.PUBLIC_SYMBOLS
    lib = nbx.load_library()
    assert hasattr(lib, "nbxReduceMultiWideBatch")
    out = subprocess.run(["nm", "-D", "--defined-only", nbx.library_path()], capture_output=True, text=True,
                         check=True).stdout
    assert any(l.split()[-1] == "nbxReduceMultiWideBatch" and " T " in l for l in out.splitlines())
    assert callable(nbx.reduce_multi_wide_batch) and callable(nbx.reduce_multi_wide_batch_raw)
    assert nbx.LaunchFamily.WideBatchList == wb.FAM_WIDE_LIST == 15
    assert lib.nbxAbiVersion() == 1   # additive: the ABI version stays
    assert lib.nbxKernelCount() == 6 * 5 + 6 * 4   # the batch kernels live in the wide launch table


def test_no_tasks_is_a_noop_after_the_type_and_op_checks(nbx):
    lib = nbx.load_library()
    for st in (F16, BF16, E4M3, E5M2):
        for dt in (st, F32):
            assert batch(nbx, [], st, dt) == 0
            assert lib.nbxReduceMultiWideBatch(None, 0, st, dt, nbx.DevRedOpFull(), 0, None) == 0
    assert batch(nbx, [], op=devop(nbx, PREMULSUM, 0x3f000000), npre=2) == 0
    for st, dt in ((F32, F32), (2, F32), (F64, F64), (-1, F32), (12, 12), (BF16, F16), (BF16, F64), (E4M3, E5M2)):
        assert batch(nbx, [], st, dt) == E
    for code in (PROD, MINMAX, SUMPOSTDIV, 5, -1):
        assert batch(nbx, [], op=devop(nbx, code, 3)) == E
    assert batch(nbx, [], op=devop(nbx, PREMULSUM, 0, 1)) == E


def test_bad_task_list(nbx):
    lib = nbx.load_library()
    op = nbx.DevRedOpFull()
    tasks, _keep = nbx._reduce_tasks([GOOD])
    assert lib.nbxReduceMultiWideBatch(tasks, -1, BF16, BF16, op, 0, None) == E
    assert lib.nbxReduceMultiWideBatch(None, 1, BF16, BF16, op, 0, None) == E
    assert lib.nbxReduceMultiWideBatch(None, -1, BF16, BF16, op, 0, None) == E


BAD_BUCKETS = {
    "no source": (([FAKE + 16384], [], 16), BF16, BF16),
    "no destination": (([], [FAKE + 16384], 16), BF16, BF16),
    "65 sources": (([FAKE + 16384], [FAKE + 20480] * 65, 16), BF16, BF16),
    "9 destinations": (([FAKE + 16384] * 9, [FAKE + 20480], 16), BF16, BF16),
    "NULL source": (([FAKE + 16384], [FAKE + 20480, 0], 16), BF16, BF16),
    "NULL destination": (([FAKE + 16384, 0], [FAKE + 20480], 16), BF16, BF16),
    "odd bf16 source": (([FAKE + 16384], [FAKE + 20481], 16), BF16, BF16),
    "odd bf16 destination": (([FAKE + 16385], [FAKE + 20480], 16), BF16, BF16),
    "fp32 destination at +2": (([FAKE + 16386], [FAKE + 20480], 16), BF16, F32),
    "fp32 destination at +1 of fp8 sources": (([FAKE + 16385], [FAKE + 20483], 16), E4M3, F32),
    "fp32 destination on its own source": (([FAKE + 16384], [FAKE + 20480, FAKE + 16384 + 4 * 64 - 4], 64), BF16, F32),
    "fp32 destination ending on its own source": (([FAKE + 20480 - 4 * 64 + 4], [FAKE + 20480], 64), BF16, F32),
}


@pytest.mark.parametrize("name", list(BAD_BUCKETS))
def test_every_bucket_is_checked(nbx, name):
    """A bad bucket behind a good one (and behind empty ones): the call is
    refused before anything is enqueued."""
    bad, st, dt = BAD_BUCKETS[name]
    assert batch(nbx, [bad], st, dt) == E
    assert batch(nbx, [GOOD, bad], st, dt) == E
    assert batch(nbx, [GOOD, (GOOD[0], GOOD[1], 0), ([1], [3], 0), bad, GOOD], st, dt) == E


@pytest.mark.parametrize("code", [PROD, MINMAX, SUMPOSTDIV])
def test_bad_op_with_buckets(nbx, code):
    assert batch(nbx, [GOOD, GOOD], op=devop(nbx, code, 3)) == E


def test_device_scalar_checks(nbx):
    two = [GOOD, GOOD]
    assert batch(nbx, two, op=devop(nbx, PREMULSUM, 0, 1), npre=1) == E                    # NULL device scalar
    assert batch(nbx, two, op=devop(nbx, PREMULSUM, FAKE + 12288 + 2, 1), npre=1) == E     # not 4-byte aligned
    assert batch(nbx, two, E4M3, E4M3, op=devop(nbx, PREMULSUM, FAKE + 12288 + 1, 1), npre=1) == E
    empty = [(GOOD[0], GOOD[1], 0)] * 2
    assert batch(nbx, empty, op=devop(nbx, PREMULSUM, FAKE + 12288, 1), npre=1) == 0


def test_empty_buckets_are_skipped_unexamined(nbx):
    """Buckets of count 0: NULL and odd pointers are accepted, as in the single
    call, and nothing is launched (no device is needed)."""
    buckets = [([0], [1], 0), ([3], [0, 5], 0), ([FAKE + 1] * 8, [FAKE + 3] * 64, 0)]
    for st in (F16, BF16, E4M3, E5M2):
        for dt in (st, F32):
            assert batch(nbx, buckets, st, dt) == 0
    # the arrays themselves are still looked at, as in the single call
    lib = nbx.load_library()
    tasks, _keep = nbx._reduce_tasks([GOOD])
    tasks[0].count = 0
    tasks[0].srcs = None
    assert lib.nbxReduceMultiWideBatch(tasks, 1, BF16, BF16, nbx.DevRedOpFull(), 0, None) == E
    assert batch(nbx, [([FAKE], [], 0)]) == E


# ---------------------------------------------------------------------------
# the GPU test's case tables

def all_case_buckets(eb):
    yield "table", bc.table_buckets(eb, [1 + j % 8 for j in range(7)])
    yield "list_walk", bc.list_walk(eb)
    yield "record_width", bc.record_width(eb)
    yield "small_set", bc.place(bc.small_set(eb, 20), eb)


@pytest.mark.parametrize("eb", [1, 2])
def test_case_tables_fit_the_uploads_and_are_eligible(eb):
    """Every bucket reads inside mi.matrix_inputs' arrays; its destination
    stretch starts where its source window does modulo 4 elements (the table:
    dstart = start; place: modulo a pack), which is what makes an fp32
    destination 16-byte aligned behind the head, so every bucket may enter a
    batch for either output kind."""
    epp = 16 // eb
    for name, buckets in all_case_buckets(eb):
        for b in buckets:
            assert b.start + b.count <= mi.max_count(eb), (name, b.name)
            assert (b.dstart - b.start) % 4 == 0 and (b.dstart - b.start) % epp == 0, (name, b.name)
            if b.count:
                assert wb.bucket_eligible(b, eb, False) and wb.bucket_eligible(b, eb, True), (name, b.name)
            head = bc.packer_geometry(b.start, b.count, eb)[0]
            assert head <= 15   # the record's four bits
    assert [bc.packer_geometry(s, c, eb)[0] for _, s, c in bc.table(eb)][5] == epp - 3   # fp8: 13 head elements


def test_eligibility_rule():
    assert wb.eligible([0x1006, 0x2006], [0x3006], 2, False)
    assert not wb.eligible([0x1006, 0x2004], [0x3006], 2, False)       # sources on two misalignments
    assert not wb.eligible([0x1006, 0x2006], [0x3004], 2, False)       # narrow destination off the sources'
    assert wb.eligible([0x1006, 0x2006], [0x300c], 2, True)            # head 5: 0xc + 20 = 32
    assert not wb.eligible([0x1006, 0x2006], [0x3000], 2, True)
    assert wb.eligible([0x1003], [0x300c], 1, True)                    # fp8 head 13: 0xc + 52 = 64
    assert not wb.eligible([0x1003], [0x3008], 1, True)


@pytest.mark.parametrize("st", mi.WIDE_TYPES)
def test_nan_cap_per_call(oracle, st):
    """NaN is compared only as NaN: over every (output, source count, op) the
    NaN share of one table call's expected outputs taken together stays under
    mi.NAN_CAP (measured: f16 0.032, bf16 0.005, e4m3 0.007, e5m2 0.023)."""
    srcs = mi.matrix_inputs(oracle, st)
    eb = srcs[0].itemsize
    n = 1216 * (16 // eb)   # the table ends below 1,200 packs
    wide = [mi.widen(oracle, s[:n], st) for s in srcs[:mi.MAX_SRCS]]
    worst = 0.0
    for nsrc in range(1, mi.MAX_SRCS + 1):
        for code, arg, npre in mi.wide_cases(oracle, st, nsrc):
            fold = oracle.reduce_multi(wide[:nsrc], F32, code, arg, npre, threads=8)[0]
            for out32 in (True, False):
                exp = fold if out32 else mi.narrow(oracle, fold, st)
                share = bc.nan_share_of_call(exp, eb, F32 if out32 else st)
                large = max(mi.nan_share(exp[s:s + c], F32 if out32 else st) for name, s, c in bc.table(eb)
                            if name in bc.LARGE)
                assert share <= mi.NAN_CAP and large <= mi.NAN_CAP, (nsrc, code, out32, share, large)
                worst = max(worst, share)
    assert worst > 0.0   # the inputs do carry NaN through the fold
    assert np.isfinite(worst)
