"""nbxReduceMultiWide without a GPU: the symbol is declared, exported and
bound, and every argument check returns before any device call (fake
pointers, as tests/test_abi.py::test_reduce_multi_argument_checks_before_device)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = 4   # ncclInvalidArgument
F16, F32, F64, BF16, E4M3, E5M2 = 6, 7, 8, 9, 10, 11
SUM, PROD, MINMAX, PREMULSUM, SUMPOSTDIV = range(5)
FAKE = 0x100000


def test_symbol_declared_exported_and_bound(nbx):
    header = open(os.path.join(ROOT, "include", "nbx_reduce.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"ncclResult_t\s+nbxReduceMultiWide\s*\(", code)
    assert "nbxReduceMultiWide" in nbx.PUBLIC_SYMBOLS
    lib = nbx.load_library()
    assert hasattr(lib, "nbxReduceMultiWide")
    out = subprocess.run(["nm", "-D", "--defined-only", nbx.library_path()], capture_output=True, text=True,
                         check=True).stdout
    assert any(l.split()[-1] == "nbxReduceMultiWide" and " T " in l for l in out.splitlines())
    assert callable(nbx.reduce_multi_wide) and callable(nbx.reduce_multi_wide_raw)
    assert lib.nbxAbiVersion() == 1   # additive: the ABI version stays


def test_kernel_count_unchanged(nbx):
    """The wide kernels have their own launch table: nbxKernelCount still
    counts the (datatype, op) kernel sets of nbxReduceMulti."""
    assert nbx.load_library().nbxKernelCount() == 6 * 5 + 6 * 4   # integer types x 5 ops, float types x 4


def wide(nbx, dsts, srcs, count=16, st=BF16, dt=BF16, op=None, npre=0):
    return nbx.reduce_multi_wide_raw(dsts, srcs, count, st, dt, op if op is not None else nbx.DevRedOpFull(), npre)


def test_good_arguments_count_zero_is_noop(nbx):
    for st in (F16, BF16, E4M3, E5M2):
        for dt in (st, F32):
            assert wide(nbx, [FAKE], [FAKE + 4096], 0, st, dt) == 0
    op = nbx.DevRedOpFull()
    op.op = PREMULSUM
    assert wide(nbx, [FAKE], [FAKE + 4096], 0, op=op, npre=1) == 0
    # NULL pointers and odd addresses are only looked at when there is something to do
    assert wide(nbx, [0], [1], 0) == 0


@pytest.mark.parametrize("st", [2, F32, F64, 0, 5, -1, 12])
def test_bad_source_type(nbx, st):
    assert wide(nbx, [FAKE], [FAKE + 4096], 16, st, st) == E
    assert wide(nbx, [FAKE], [FAKE + 4096], 16, st, F32) == E
    assert wide(nbx, [FAKE], [FAKE + 4096], 0, st, F32) == E   # type checks come before the count == 0 return


def test_bad_destination_type(nbx):
    assert wide(nbx, [FAKE], [FAKE + 4096], 16, BF16, F64) == E
    assert wide(nbx, [FAKE], [FAKE + 4096], 16, BF16, F16) == E
    assert wide(nbx, [FAKE], [FAKE + 4096], 16, E4M3, E5M2) == E
    assert wide(nbx, [FAKE], [FAKE + 4096], 0, BF16, F16) == E


@pytest.mark.parametrize("devop", [PROD, MINMAX, SUMPOSTDIV, 5, -1])
def test_bad_op(nbx, devop):
    op = nbx.DevRedOpFull()
    op.op = devop
    op.scalarArg = 3
    assert wide(nbx, [FAKE], [FAKE + 4096], 16, op=op) == E
    assert wide(nbx, [FAKE], [FAKE + 4096], 0, op=op) == E


def test_source_and_destination_counts(nbx):
    assert wide(nbx, [FAKE], []) == E
    assert wide(nbx, [FAKE], [FAKE + 4096] * 65) == E
    assert wide(nbx, [], [FAKE + 4096]) == E
    assert wide(nbx, [FAKE] * 9, [FAKE + 4096]) == E


def test_null_pointers(nbx):
    lib = nbx.load_library()
    op = nbx.DevRedOpFull()
    one = (ctypes.c_void_p * 1)(ctypes.c_void_p(FAKE))
    assert lib.nbxReduceMultiWide(None, 1, one, 1, 16, BF16, BF16, op, 0, None) == E
    assert lib.nbxReduceMultiWide(one, 1, None, 1, 16, BF16, BF16, op, 0, None) == E
    assert lib.nbxReduceMultiWide(None, 1, one, 1, 0, BF16, BF16, op, 0, None) == E   # NULL arrays even for count 0
    assert wide(nbx, [0], [FAKE]) == E
    assert wide(nbx, [FAKE], [FAKE + 4096, 0]) == E


def test_pointer_alignment(nbx):
    assert wide(nbx, [FAKE], [FAKE + 4097]) == E                       # bf16 source at an odd address
    assert wide(nbx, [FAKE + 1], [FAKE + 4096]) == E                   # bf16 destination at an odd address
    assert wide(nbx, [FAKE + 2], [FAKE + 4096], dt=F32) == E           # fp32 destination at +2
    assert wide(nbx, [FAKE + 1], [FAKE + 4099], 16, E4M3, F32) == E    # fp8 sources take any address, the fp32 output does not


def test_device_scalar_checks(nbx):
    op = nbx.DevRedOpFull()
    op.op = PREMULSUM
    op.scalarArgIsPtr = 1
    op.scalarArg = 0
    assert wide(nbx, [FAKE], [FAKE + 4096], op=op, npre=1) == E        # NULL device scalar
    op.scalarArg = FAKE + 8192 + 2
    assert wide(nbx, [FAKE], [FAKE + 4096], op=op, npre=1) == E        # not 4-byte aligned
    op.scalarArg = FAKE + 8192 + 1
    assert wide(nbx, [FAKE], [FAKE + 4096], 16, E4M3, E4M3, op=op, npre=1) == E   # an fp32 scalar whatever the source type


def test_fp32_destination_must_not_overlap_a_source(nbx):
    n = 64
    src = [FAKE, FAKE + 4096]
    assert wide(nbx, [FAKE], src, n, BF16, F32) == E                   # the same address
    assert wide(nbx, [FAKE + 4096 + 2 * n - 4], src, n, BF16, F32) == E   # its first element on the source's last two
    assert wide(nbx, [FAKE + 4096 - 4 * n + 4], src, n, BF16, F32) == E   # its last element on the source's first two
    assert wide(nbx, [FAKE + 8192, FAKE + 4100], src, n, BF16, F32) == E  # any destination
    assert wide(nbx, [FAKE + 64], [FAKE + 60], 8, E5M2, F32) == E
