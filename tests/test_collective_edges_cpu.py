"""The collective edge-value tests' case table (tests/edges/cases.py), without
a GPU:

  * the table and its inputs are deterministic, and rank r's input does not
    depend on how many ranks there are;
  * NaN — compared only as NaN on the GPU — stays under the 10 % cap in every
    float case's expected result;
  * the edge classes reach the outputs: sums, products and averages of the
    50,021-byte case land in the denormal range;
  * every (path, kind, size, n) maps to the protocol it is meant for through
    the library's own choice (nbxDebugChooseProto), under the masks and limits
    the path's environment sets, so a threshold change fails here before it
    silently reroutes a GPU case;
  * the Simple size gives the full / ragged / tail iterations cases.py's
    docstring works out;
  * for Sum / Prod / Avg the ring chain and the direct fold give the same
    non-NaN bits — these ops commute bit for bit and the chain associates like
    the left fold, so only Max / Min (ties return the second operand) can tell
    the two operand orders apart; the ring cases use ring_chain all the same."""
import ctypes

import numpy as np
import pytest

from tests import mp_diag
from tests.conftest import gpu_order_key
from tests.edges import cases
from tests.matrix import inputs as mi

F32, F64 = mi.F32, mi.F64
K, M = 1 << 10, 1 << 20
LL_MAX, LL128_MAX, ONESHOT_MAX = 64 * K, 1 * M, 256 * K   # the defaults (comm_mp_settings.cc mpSettings)
ITER_BYTES = {16: 65536, 8: 32768, 4: 16384}              # one simpleFoldU iteration: U x 256 packs x 16 B


@pytest.fixture(scope="module", autouse=True)
def _release_inputs():
    yield
    cases._sources.cache_clear()


def bits(a):
    return a.view(mi.UINT_OF[a.itemsize])


def each_case(paths=cases.PATHS):
    for path in paths:
        for i, (kind, dt, op) in enumerate(cases.path_cases(path)):
            yield path, i, kind, dt, op


# ---------------------------------------------------------------------------
# the table

def test_case_table_shape():
    per_path = {p: len(cases.path_cases(p)) for p in cases.PATHS}
    # 12 types x (5 AllReduce + 3 ReduceScatter + 3 Reduce ops); the two-shot path has no ReduceScatter
    assert per_path == {"ll": 132, "ll128": 132, "ll128x2": 96, "simple": 132, "simple_elts": 132, "ring": 132}
    for p in cases.PATHS:
        cs = cases.path_cases(p)
        assert cs == cases.path_cases(p) and len(set(cs)) == len(cs)
        assert {(k, op) for k, _, op in cs if k == "ar"} == {("ar", op) for op in range(5)}
        assert {dt for _, dt, _ in cs} == set(range(12))
    assert set(cases.PATH_COMM.values()) == set(cases.COMMS)
    for env in cases.COMM_ENV.values():
        assert set(env) <= set(cases.ENV_KEYS) | set(cases.PROCESS_ENV)


def test_sizes_and_alignment(oracle):
    for p in cases.PATHS:
        for dt in cases.ALL_TYPES:
            eb = cases.itemsize(oracle, dt)
            c = cases.count_of(oracle, p, dt)
            if p == "simple_elts":
                assert c == 5003 and cases.shift_of(oracle, p, dt) == eb and (16 + eb) % 16 != 0
            else:
                assert c == cases.PATH_BYTES[p] // eb and cases.shift_of(oracle, p, dt) == 0
                assert cases.PATH_BYTES[p] % 16 not in (0, 8) and cases.PATH_BYTES[p] % 48 != 0   # partial last unit


@pytest.mark.parametrize("dtype", [1, 4, 6, 7, 8, 9, 10, 11])
def test_inputs_are_deterministic_and_rank_stable(oracle, dtype):
    """Rank r's input is source r of edge_inputs(oracle, dtype, 8, total, seed)
    however many sources are asked for, and a second call gives the same bits."""
    nb = cases.nbytes_of(oracle, "ll", dtype)
    total = cases.total_of(oracle, "ll", "ar", dtype, 5)
    ref = mi.edge_inputs(oracle, dtype, 8, total, cases.seed_of(dtype, nb))
    for n in cases.NS:
        xs = cases.rank_inputs(oracle, "ll", "ar", dtype, n)
        assert len(xs) == n
        for r in range(n):
            assert np.array_equal(bits(xs[r]), bits(ref[r]))
            assert np.array_equal(bits(cases.rank_input(oracle, "ll", "ar", dtype, n, r)), bits(ref[r]))
    cases._sources.cache_clear()
    again = cases.rank_inputs(oracle, "ll", "ar", dtype, 5)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(again, ref))
    # another size, another type: other values
    other = cases.rank_inputs(oracle, "ll128", "ar", dtype, 2)[0]
    assert not np.array_equal(bits(other[:1000]), bits(ref[0][:1000]))
    # a ReduceScatter's input is n blocks long
    assert cases.rank_inputs(oracle, "ll", "rs", dtype, 3)[0].size == 3 * cases.count_of(oracle, "ll", dtype)


def test_roots_rotate():
    for n in cases.NS:
        roots = {cases.root_of(i, n) for i, (kind, _, _) in enumerate(cases.path_cases("ll")) if kind == "red"}
        assert roots == ({1} if n == 3 else set(range(n)))   # (3 i + 1) mod n


# ---------------------------------------------------------------------------
# expected results

@pytest.mark.parametrize("n", cases.NS)
def test_expected_results(oracle, n):
    """Every case's expected result, on every rank that has one, folded once.

    NaN cap: every float result holds <= 10 % NaN. e4m3fn has no infinity: its
    one code 0x7f / 0xff is what is_nan counts, so an overflow that saturates
    to it is counted as NaN here, as the fp32 folds' inf is in
    test_matrix_inputs_cpu.py::test_nan_cap_wide. No result is all zero either
    (the GPU test's outputs start as 0xA5 and must become these).

    Ring against direct (same 300,011-byte inputs). Sum / Prod / Avg:
    Fn(local, received) and Fn(received, local) give the same bits (NaN
    payloads aside), and the chain b+1 -> ... -> b associates like the left
    fold b+1, ..., b, so the ring's expected values equal the direct
    schedule's. Max / Min return the second operand of a tie (+0 / -0), so
    there the order shows — which these inputs do exercise."""
    worst, direct, differ = {}, {}, 0
    assert cases.PATHS.index("simple") < cases.PATHS.index("ring")
    assert cases.path_cases("simple") == cases.path_cases("ring")
    for path, i, kind, dt, op in each_case():
        exp = cases.expected(oracle, path, kind, dt, op, n, cases.root_of(i, n))
        for r, e in exp.items():
            assert e.size == cases.count_of(oracle, path, dt)
            assert np.count_nonzero(bits(e)) > e.size // 4, (path, kind, dt, op, r)
            if dt in mi.FLOAT_TYPES:
                share = mi.nan_share(e, dt)
                worst[dt] = max(worst.get(dt, 0.0), share)
                assert share <= mi.NAN_CAP, (path, kind, dt, op, n, r, share)
        if dt in mi.FLOAT_TYPES and path == "simple":
            direct[i] = exp
        if dt in mi.FLOAT_TYPES and path == "ring":
            for r, e in exp.items():
                if op in (cases.MAX, cases.MIN):
                    differ += int(not np.array_equal(bits(e), bits(direct[i][r])))
                else:
                    mi.assert_same(e, direct[i][r], dt)
            del direct[i]
    assert differ > 0
    print(f"n = {n}: largest NaN share per type", {oracle.TYPE_NAMES[d]: f"{s:.2%}" for d, s in worst.items()})


@pytest.mark.parametrize("n", cases.NS)
@pytest.mark.parametrize("dtype", [F32, F64])
def test_denormals_reach_the_outputs(oracle, dtype, n):
    """A kernel that flushed denormals would differ from the oracle in more
    than 20 outputs of each of these cases."""
    for op in (cases.SUM, cases.PROD, cases.AVG):
        e = cases.expected(oracle, "ll128x2", "ar", dtype, op, n, 0)[0]
        d = mi.denormal_count(e, dtype)
        print(f"{oracle.TYPE_NAMES[dtype]} op {op} x{n}: {d} denormal outputs of {e.size}")
        assert d > 20, (dtype, op, n, d)


# ---------------------------------------------------------------------------
# protocol and geometry

@pytest.fixture(scope="module")
def lib(nbx):
    lib = nbx.load_library()
    lib.nbxDebugProtoMask.argtypes = [ctypes.c_char_p]
    lib.nbxDebugProtoMask.restype = ctypes.c_int
    lib.nbxDebugChooseProto.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                        ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    lib.nbxDebugChooseProto.restype = ctypes.c_int
    return lib


@pytest.mark.parametrize("n", cases.NS)
def test_every_case_maps_to_its_protocol(lib, oracle, n):
    for path in cases.PATHS:
        env = cases.COMM_ENV[cases.PATH_COMM[path]]
        mask = lib.nbxDebugProtoMask(env["NCCL_PROTO"].encode())
        oneshot = int(env.get("NBX_LL128_ONESHOT_MAX", ONESHOT_MAX))
        for kind in cases.PATH_KINDS[path]:
            for dt in cases.ALL_TYPES:
                eb = cases.itemsize(oracle, dt)
                count = cases.count_of(oracle, path, dt)
                lo, hi = mp_diag.block_range(count, eb, n, 0)
                got = lib.nbxDebugChooseProto(mask, int(kind != "rs"), count * eb, (hi - lo) * eb, n, LL_MAX, LL128_MAX,
                                              oneshot)
                want = cases.PROTO_OF_FAMILY[cases.family_of(path, kind, n)]
                assert got == want, (path, kind, dt, n, got, want)
    # the ring is an algorithm of the Simple protocol, chosen by NCCL_ALGO at creation
    assert cases.COMM_ENV["ring"]["NCCL_ALGO"] == "Ring" and "NCCL_ALGO" not in cases.COMM_ENV["simple"]


def _by_workgroup(spans, block):
    out = {}
    for b, k, w, nb in spans:
        if b == block:
            out.setdefault(w, []).append(nb)
    return out


@pytest.mark.parametrize("eb", [1, 2, 4, 8])
def test_simple_size_reaches_every_iteration_shape(eb):
    """cases.py's arithmetic for SIMPLE_BYTES, at every element size."""
    count = cases.SIMPLE_BYTES // eb
    for n in (3, 5):
        it = ITER_BYTES[cases.fold_unroll("simple", n)]
        spans = cases.fold_spans("ar", count, eb, n, ring=False)
        assert {w for _, _, w, _ in spans} == {0, 1} and {k for _, k, _, _ in spans} == {0}
        for b, k, w, nb in spans:
            assert it < nb < 2 * it and nb // 16 % (it // 16) != 0, (n, b, w, nb)   # a full iteration, then a ragged one
        tails = [(b, w) for b, _, w, nb in spans if nb % 16]
        assert tails == [(n - 1, 1)]                                                # then a tail below one pack
    it = ITER_BYTES[cases.fold_unroll("simple", 2)]
    spans = cases.fold_spans("ar", count, eb, 2, ring=False)
    for b in (0, 1):
        wg = _by_workgroup(spans, b)
        assert wg[1] == [it]                       # workgroup 1: one whole iteration
        assert wg[0][0] == it and 16 <= wg[0][1] < it and len(wg[0]) == 2   # workgroup 0: whole, then ragged
    assert [nb % 16 != 0 for b, _, _, nb in spans if b == 1][-1] and not any(nb % 16 for b, _, _, nb in spans if b == 0)
    # U = 16 and the 64 KiB slice: no slice can hold more than one iteration
    assert mp_diag.simple_geometry("ar", 64 * M, 1, 2, cases.SIMPLE_GRID, 64 * K).slice_elts == it
    # the ring (U = 16 on every hop): full + ragged rounds at 2 ranks and in every Reduce
    it = ITER_BYTES[cases.fold_unroll("ring", 5)]
    assert it == 65536
    for n in cases.NS:
        red = [nb for _, _, _, nb in cases.fold_spans("red", count, eb, n, ring=True)]
        assert red.count(it) == 4 and len(red) == 5 and red[-1] % 16 != 0 and red[-1] > 16
    wg = _by_workgroup(cases.fold_spans("ar", count, eb, 2, ring=True), 1)
    assert wg[0][0] == it and wg[0][1] % 16 != 0
    # the element path: one workgroup or two, more than one pass of 256 lanes
    for n in cases.NS:
        for kind in ("ar", "rs", "red"):
            spans = cases.fold_spans(kind, cases.ELTS_COUNT, eb, n, ring=False)
            assert max(nb for _, _, _, nb in spans) // eb > 256


def test_gpu_file_sorts_with_the_multiprocess_tests():
    assert gpu_order_key("tests/edges/test_multiprocess_gpu.py") == gpu_order_key("tests/test_multiprocess_gpu.py")
    assert gpu_order_key("tests/edges/test_multiprocess_gpu.py", "test_collective_edges[3]") == \
        gpu_order_key("tests/test_multiprocess_gpu.py")
