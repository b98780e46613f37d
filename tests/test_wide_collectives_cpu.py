"""The wide (fp32-accumulating) collectives without a GPU: the case table of
tests/widecoll/cases.py and its slice arithmetic, that the wide expectation is
not the per-step one, nbxRedOpCreateWide's argument checks, the unchanged
kernel count and ABI version, and the NBX_WIDE_ACCUM setting.

A communicator cannot be created without a device (ncclCommInitRank asks HIP
for the current one first), so the checks that need a live handle — create /
destroy / reuse of a slot, the datatype mismatch at the call — run in
tests/widecoll/test_clique_transport_gpu.py on a one-rank communicator; the argument
checks here are the ones nbxRedOpCreateWide makes before it looks at the
communicator."""
import ctypes

import numpy as np
import pytest

from tests.widecoll import cases


def test_case_table():
    assert cases.TYPES == (6, 9, 10, 11) and cases.OPS == (0, 4) and cases.NS == (2, 3, 5)
    assert cases.PATHS == ("ll", "ll128", "ll128x2", "simple", "simple_elts", "ring_direct")
    total = 0
    for path in cases.PATHS:
        pc = cases.path_cases(path)
        assert len(pc) == len(set(pc)) == len(cases.PATH_KINDS[path]) * 8
        kinds = [cases.input_kind(path, *c) for c in pc]
        assert kinds.count("edge") == kinds.count("uniform") == len(pc) // 2
        for dt in cases.TYPES:       # every (type, op) meets both kinds of input on the path
            for op in cases.OPS:
                assert {cases.input_kind(path, k, dt, op) for k in cases.PATH_KINDS[path]} == {"edge", "uniform"}
        total += len(pc)
    assert cases.PATH_KINDS["ll128x2"] == ("ar", "red")
    assert total == 136 and total * 5 < 756   # under a fifth of tests/edges' cases per n
    # the families: ring_direct is the direct Simple kernel on the ring communicator
    assert cases.PATH_COMM["ring_direct"] == "ring" and cases.COMM_ENV["ring"]["NCCL_ALGO"] == "Ring"
    for n in cases.NS:
        for kind in ("ar", "rs", "red"):
            assert cases.family_of("ring_direct", kind, n) == 11
            assert cases.family_of("simple", kind, n) == cases.family_of("simple_elts", kind, n) == 11
            assert cases.family_of("ll", kind, n) == 8 and cases.family_of("ll128", kind, n) == 9
        assert cases.family_of("ll128x2", "ar", n) == (10 if n > 2 else 9)


def test_sizes_and_inputs(oracle):
    for dt in cases.TYPES:
        eb = cases.itemsize(oracle, dt)
        assert cases.count_of(oracle, "ll", dt) == 20011 // eb
        assert cases.count_of(oracle, "ll128", dt) == 12011 // eb
        assert cases.count_of(oracle, "ll128x2", dt) == 50021 // eb
        assert cases.count_of(oracle, "simple", dt) == cases.count_of(oracle, "ring_direct", dt) == 300011 // eb
        assert cases.count_of(oracle, "simple_elts", dt) == 5003 and cases.shift_of(oracle, "simple_elts", dt) == eb
        assert cases.shift_of(oracle, "ring_direct", dt) == 0
    # rank r's input does not depend on n (but for a ReduceScatter's length)
    for which_op in cases.OPS:
        a = cases.rank_inputs(oracle, "ll", "ar", 9, which_op, 5)
        b = cases.rank_inputs(oracle, "ll", "ar", 9, which_op, 2)
        assert len(a) == 5 and len(b) == 2 and all(np.array_equal(a[r], b[r]) for r in range(2))
        assert all(x.dtype == np.uint16 and x.size == 20011 // 2 for x in a)


@pytest.mark.parametrize("n", cases.NS)
def test_wide_simple_iterations(n):
    """The slice arithmetic of cases.py's docstring for the wide unrolls 8 / 4 / 4: at every n some
    workgroup folds a full iteration and a ragged one (in one slice, or in successive rounds)."""
    u = cases.wide_unroll(n)
    assert u == {2: 8, 3: 4, 5: 4}[n]
    it = u * 256 * 16
    spans = cases.fold_spans("ar", 300011, 1, n, False)
    by_wg = {}
    for b, k, w, nbytes in spans:
        if b == 0:
            by_wg.setdefault(w, []).append(nbytes)
    full = {w: any(x >= it for x in v) for w, v in by_wg.items()}
    ragged = {w: any(x % it != 0 for x in v) for w, v in by_wg.items()}
    assert any(full[w] and ragged[w] for w in by_wg), (by_wg, it)
    want = {2: {0: [65536, 18944], 1: [65536]}, 3: {0: [50016], 1: [50000]}, 5: {0: [30016], 1: [30000]}}[n]
    assert by_wg == want
    # the last block ends in a tail below one pack
    last = [nbytes for b, k, w, nbytes in spans if b == n - 1]
    assert sum(last) % 16 == 11


@pytest.mark.parametrize("n", (3, 5))
@pytest.mark.parametrize("op", cases.OPS)
@pytest.mark.parametrize("dt", (6, 9))
def test_wide_expectation_is_not_the_per_step_one(oracle, dt, op, n):
    """Uniform inputs, 16-bit types: in EVERY block of every kind the wide result differs from
    the per-step operator's in at least one element, so a library that ignored the handle cannot
    pass the GPU test. (At n = 2 a wide Sum is the per-step Sum: one add, one rounding.)"""
    seen = 0
    for path in ("ll", "ll128", "simple_elts"):
        for kind in cases.PATH_KINDS[path]:
            if cases.input_kind(path, kind, dt, op) != "uniform":
                continue
            xs = cases.rank_inputs(oracle, path, kind, dt, op, n)
            count = cases.count_of(oracle, path, dt)
            root = 1
            wide = cases.expected_with(cases.wide_fold_of, oracle, xs, kind, dt, op, n, root, count)
            step = cases.expected_with(cases.per_step_fold_of, oracle, xs, kind, dt, op, n, root, count)
            if kind == "ar":
                for b, lo, hi in cases.blocks_of(kind, count, 2, n):
                    assert hi > lo and (wide[0][lo:hi] != step[0][lo:hi]).any(), (path, kind, b)
                share = float((wide[0] != step[0]).mean())
            else:
                for r in wide:
                    assert (wide[r] != step[r]).any(), (path, kind, r)
                share = float(np.mean([(wide[r] != step[r]).mean() for r in wide]))
            assert 0.05 < share < 0.9, share
            seen += 1
    assert seen >= 3


def test_two_rank_wide_sum_is_the_per_step_sum(oracle):
    for dt in (6, 9):
        xs = cases._sources(oracle, "uniform", dt, 20011, 20011 // 2)[:2]
        assert np.array_equal(cases.wide_fold_of(oracle, xs, dt, cases.SUM, 2),
                              cases.per_step_fold_of(oracle, xs, dt, cases.SUM, 2))


def test_create_wide_argument_checks(nbx):
    """NULL op or comm, a base other than Sum / Avg (a user handle's value included), a datatype
    outside the four: ncclInvalidArgument, decided before the communicator is looked at."""
    lib = nbx.load_library()
    assert "nbxRedOpCreateWide" in nbx.PUBLIC_SYMBOLS and hasattr(nbx.Communicator, "redop_create_wide")
    assert not hasattr(lib, "pnbxRedOpCreateWide")
    f = lib.nbxRedOpCreateWide
    f.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    f.restype = ctypes.c_int
    op = ctypes.c_int(-7)
    fake = ctypes.c_void_p(1)   # never dereferenced: every call below fails an earlier check
    assert f(ctypes.byref(op), 0, 9, None) == 4
    assert f(None, 0, 9, fake) == 4
    for base in (1, 2, 3, 5, 6, 1000, -1):   # Prod, Max, Min, ncclNumOps, user handles, garbage
        assert f(ctypes.byref(op), base, 9, fake) == 4
    for dt in (0, 1, 2, 3, 4, 5, 7, 8, 12, -1):
        for base in (0, 4):
            assert f(ctypes.byref(op), base, dt, fake) == 4
    assert op.value == -7


def test_kernel_count_and_abi_unchanged(nbx):
    lib = nbx.load_library()
    assert lib.nbxKernelCount() == 6 * 5 + 6 * 4
    assert lib.nbxAbiVersion() == 1


def test_wide_accum_setting(nbx, monkeypatch):
    lib = nbx.load_library()
    lib.nbxDebugTransportSettings.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
    lib.nbxDebugTransportSettings.restype = ctypes.c_int
    undef = -2147483648

    def settings(n_out=17):
        out = (ctypes.c_int64 * 17)(*([-1] * 17))
        got = lib.nbxDebugTransportSettings(2, 256, 1, 0, undef, undef, 0, out, n_out)
        return got, list(out)

    monkeypatch.delenv("NBX_WIDE_ACCUM", raising=False)
    got, off = settings()
    assert got == 17 and off[16] == 0
    monkeypatch.setenv("NBX_WIDE_ACCUM", "0")
    assert settings()[1][16] == 0
    monkeypatch.setenv("NBX_WIDE_ACCUM", "1")
    got, on = settings()
    assert got == 17 and on[16] == 1
    assert on[:16] == off[:16]            # nothing else moves
    got, short = settings(16)             # existing callers: 16 values, the 17th untouched
    assert got == 16 and short[16] == -1 and short[:16] == off[:16]
