"""The clique transport tests' tables (tests/clique/cases.py), without a GPU:

  * the stream budget: at every rank count used, the streams the worker
    creates plus the default stream fit the hardware queues it asks for;
  * the byte-bound arithmetic of the routing cases, and which protocol the
    library's own choice (nbxDebugChooseProto) gives every routing size under
    the protocol set its communicator is created with — and under the default
    set, where they are LL128-sized and the bound would not apply;
  * every table of parts 2-4 is non-empty, its expected records well formed,
    and the eight-rank sizes map to the kernels they are meant for;
  * part 1 is tests/edges/cases.py's table itself, not a copy that can drift;
  * the chain's values stay exactly representable at every step for n <= 3;
  * the scenario model (simulate) is the plain sum for the exact inputs, and
    match_records accepts what it should and nothing else."""
import ctypes

import numpy as np
import pytest

from tests import mp_diag
from tests.clique import cases
from tests.conftest import gpu_order_key
from tests.edges import cases as edges

K, M = 1 << 10, 1 << 20
LL_MAX, LL128_MAX, ONESHOT_MAX = 64 * K, 1 * M, 256 * K   # the defaults (comm_mp_settings.cc mpSettings)


@pytest.fixture(scope="module")
def lib(nbx):
    lib = nbx.load_library()
    lib.nbxDebugProtoMask.argtypes = [ctypes.c_char_p]
    lib.nbxDebugProtoMask.restype = ctypes.c_int
    lib.nbxDebugChooseProto.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                        ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    lib.nbxDebugChooseProto.restype = ctypes.c_int
    return lib


def _proto(lib, mask, kind, count, eb, n, oneshot=ONESHOT_MAX):
    lo, hi = mp_diag.block_range(count, eb, n, 0)
    return lib.nbxDebugChooseProto(mask, int(kind != "rs"), count * eb, (hi - lo) * eb, n, LL_MAX, LL128_MAX, oneshot)


def test_stream_budget():
    default_stream = 1
    for n in cases.NS + (cases.EIGHT_N, cases.ROUTE_N):
        assert cases.streams_needed(n) == n + 1
        assert cases.streams_needed(n) <= cases.HW_QUEUES - default_stream
    assert cases.streams_needed(cases.EIGHT_N) == 9
    for n in range(2, cases.TWO_STREAM_MAX_N + 1):   # the chain: two streams per rank
        assert cases.streams_needed(n, True) == 2 * n + 1 <= cases.HW_QUEUES - default_stream
    assert cases.ROUTE_N <= cases.TWO_STREAM_MAX_N
    assert cases.HW_QUEUES == 24 <= 32 and cases.CHILD_ENV["GPU_MAX_HW_QUEUES"] == "24"
    assert cases.CHILD_ENV["NBX_CLIQUE_LL"] == "1" and cases.CHILD_ENV["NBX_TIMEOUT_SEC"] == "5"
    assert cases.CHILD_ENV["NBX_LL128_MAX_GRID"] == edges.PROCESS_ENV["NBX_LL128_MAX_GRID"]


def test_part_one_is_the_edge_table():
    for name in ("PATHS", "PATH_COMM", "PATH_KINDS", "COMM_ENV", "COMMS", "NS", "path_cases", "root_of", "rank_input",
                 "expected", "family_of", "host_unroll", "count_of", "shift_of", "itemsize", "nbytes_of"):
        assert getattr(cases, name) is getattr(edges, name), name
    assert cases.edges is edges and cases.GUARD == 16
    assert sum(len(cases.path_cases(p)) for p in cases.PATHS) == 756
    assert set(edges.ENV_KEYS) <= set(cases.ENV_KEYS) <= set(cases.SCRUB_ENV)
    # the file's name places it in the transport group of the GPU suite
    key = gpu_order_key("tests/clique/test_clique_transport_gpu.py")
    assert key == gpu_order_key("tests/test_clique_transport_gpu.py") != gpu_order_key("tests/clique/other_gpu.py")


def test_eight_rank_table(lib, oracle):
    n = cases.EIGHT_N
    total = 0
    for path in cases.EIGHT_PATHS:
        cs = cases.eight_cases(path)
        total += len(cs)
        assert cs and {k for k, _, _ in cs} == set(cases.PATH_KINDS[path])
        assert {d for _, d, _ in cs} == {cases.F32, cases.BF16} and {o for _, _, o in cs} == {cases.SUM, cases.AVG}
        env = cases.COMM_ENV[cases.PATH_COMM[path]]
        mask = lib.nbxDebugProtoMask(env["NCCL_PROTO"].encode())
        oneshot = int(env.get("NBX_LL128_ONESHOT_MAX", ONESHOT_MAX))
        for kind, dt, _ in cs:
            got = _proto(lib, mask, kind, cases.count_of(oracle, path, dt), cases.itemsize(oracle, dt), n, oneshot)
            assert got == edges.PROTO_OF_FAMILY[cases.family_of(path, kind, n)], (path, kind, dt)
        assert {cases.root_of(i, n) for i, (k, _, _) in enumerate(cs) if k == "red"} <= set(range(n))
    assert total == 2 * 2 * (4 * 3 + 2)
    assert cases.family_of("ll128x2", "ar", n) == edges.FAM_LL128X2
    assert edges.fold_unroll("simple", n) == 4 and edges.fold_unroll("ring", n) == 16   # the U = 4 fold
    # every rank's input exists at eight ranks: edge_inputs draws eight sources
    assert len(edges.rank_inputs(oracle, "ll", "ar", cases.F32, n)) == n


def test_byte_bound_arithmetic(lib):
    n, eb = cases.ROUTE_N, 4
    assert int(cases.SCENARIO_COMM_ENV["bound"]["NBX_CLIQUE_SIMPLE_MAX_BYTES"]) == cases.BOUND_BYTES == 262144
    assert [(k, c) for k, c, _, _ in cases.BOUND_CASES] == [("ar", 65536), ("ar", 65537), ("rs", 21845), ("rs", 21846)]
    for kind, count, sent, inside in cases.BOUND_CASES:
        assert sent == count * eb * (n if kind == "rs" else 1)    # cliqueInKernel's sendBytes
        assert inside == (sent <= cases.BOUND_BYTES)
    assert [s for _, _, s, _ in cases.BOUND_CASES] == [262144, 262148, 262140, 262152]
    # under the default protocol set these sizes are LL128-sized, and the bound is only asked of a
    # Simple-sized call: the communicator is created with NCCL_PROTO=Simple
    default_mask = lib.nbxDebugProtoMask(None)
    bound_mask = lib.nbxDebugProtoMask(cases.SCENARIO_COMM_ENV["bound"]["NCCL_PROTO"].encode())
    for kind, count, _, _ in cases.BOUND_CASES:
        assert _proto(lib, default_mask, kind, count, eb, n) in (edges.P_LL128, edges.P_LL128X2)
        assert _proto(lib, bound_mask, kind, count, eb, n) == edges.P_SIMPLE


def test_routing_sizes_and_protocols(lib, oracle):
    n = cases.ROUTE_N
    scenarios = cases.routing_scenarios()
    assert {sc.name for sc in scenarios} == {"shared_stream", "count_zero", "simple_byte_bound", "clique_simple_off",
                                             "clique_ll_off", "mismatched_collective"}
    default_mask = lib.nbxDebugProtoMask(None)
    for sc in scenarios:
        env = cases.SCENARIO_COMM_ENV[sc.comm]
        mask = lib.nbxDebugProtoMask(env["NCCL_PROTO"].encode()) if "NCCL_PROTO" in env else default_mask
        for gi, (g, phases) in enumerate(zip(sc.groups, sc.expect)):
            for ci, c in enumerate(g):
                if c.count == 0:
                    continue
                p = _proto(lib, mask, c.kind, c.count, cases.itemsize(oracle, c.dtype), n)
                if sc.protos is not None:
                    assert p == sc.protos[gi][ci], (sc.name, gi, p)
                # an in-kernel expectation names the family of the protocol the size gets
                kernels = [ph for ph in phases if ph[0] == "kernel"]
                if kernels and len(g) == 1:
                    assert edges.PROTO_OF_FAMILY[kernels[0][1]] == p, (sc.name, gi, p)
    off = next(sc for sc in scenarios if sc.name == "clique_simple_off")
    assert [g[0].count for g in off.groups] == [300011, 20011] and all(g[0].dtype == cases.INT8 for g in off.groups)
    # 300,011 B is LL128 two-shot under the default set: NBX_CLIQUE_SIMPLE=0 only shows with LL128 out
    assert _proto(lib, default_mask, "ar", 300011, 1, n) == edges.P_LL128X2
    shared = next(sc for sc in scenarios if sc.name == "shared_stream")
    assert all(c.stream == "shared" for g in shared.groups for c in g)
    bad = next(sc for sc in scenarios if sc.name == "mismatched_collective")
    assert bad.groups[0][0].bad_rank == 1 and bad.expect[0] == [("error", 5)] and bad.groups[0][0].count > 1


def test_group_scenarios(lib, oracle):
    n = cases.ROUTE_N
    scenarios = cases.group_scenarios()
    assert [sc.name for sc in scenarios] == ["segment_table", "buffer_dependency", "mixed_group", "chain"]
    mask = lib.nbxDebugProtoMask(None)
    assert _proto(lib, mask, "ar", cases.LL_COUNT, 4, n) == edges.P_LL
    assert _proto(lib, mask, "ar", cases.BIG_COUNT, 4, n) == edges.P_SIMPLE
    assert all(_proto(lib, mask, "ar", c, 4, n) == edges.P_LL for c in cases.SEGMENT_COUNTS)
    by = {sc.name: sc for sc in scenarios}
    # the mirror of runMpGroup's cut: six segments in one launch; the dependent call alone
    plan = cases.group_plan(oracle, by["segment_table"].groups[0], n, {"llMax": LL_MAX, "l128Max": LL128_MAX,
                                                                       "groupBatch": 1})
    assert plan.records == [(8, n, 1, 6 << 8)] and len(cases.SEGMENT_COUNTS) == 6
    dep = by["buffer_dependency"].groups[0]
    assert dep[2].send == dep[1].recv
    plan = cases.group_plan(oracle, dep, n, {"llMax": LL_MAX, "l128Max": LL128_MAX, "groupBatch": 1})
    assert plan.runs == [(0, 2), (2, 3)] and plan.reasons == ["conflict"]
    assert [("kernel", r[0], r[2], r[3]) for r in plan.records] == by["buffer_dependency"].expect[0]
    mixed = by["mixed_group"].groups[0]
    assert [c.stream for c in mixed] == ["own", "shared", "own"]
    assert len({c.send for c in mixed} | {c.recv for c in mixed}) == 6   # independent buffers
    chain = by["chain"]
    assert not chain.sync and [g[0].stream for g in chain.groups] == ["own", "shared", "own2", "own"]
    for a, b in zip(chain.groups, chain.groups[1:]):
        assert b[0].send == a[0].recv
    # the last link is Simple-sized and above the communicator's bound: a fold on distinct streams
    assert chain.groups[3][0].count * 4 > int(cases.SCENARIO_COMM_ENV["chain"]["NBX_CLIQUE_SIMPLE_MAX_BYTES"])


def test_expected_records_are_well_formed():
    for sc in cases.routing_scenarios() + cases.group_scenarios():
        assert sc.groups and len(sc.groups) == len(sc.expect) and sc.comm in cases.SCENARIO_COMM_ENV
        assert sc.protos is None or [len(p) for p in sc.protos] == [len(g) for g in sc.groups]
        for g, phases in zip(sc.groups, sc.expect):
            assert g and cases.well_formed(phases)
            assert phases or all(c.count == 0 for c in g)   # only a count of 0 leaves no record
    assert cases.inplace_cases() and len(cases.inplace_cases()) == 2 * len(cases.PATHS) - 1
    assert {p for p, _ in cases.inplace_cases()} == set(cases.PATHS)
    pm = cases.premul_cases()
    assert len(pm) == 3 * 3 * 3 * 2 and {d for *_, d in pm} == {False, True}
    assert {dt for _, _, dt, _ in pm} == {cases.F16, cases.F32, cases.INT32}
    assert cases.well_formed([("premul", 9, 1)])


def test_match_records():
    n = 3
    ll = (8, n, 1, 0)
    assert cases.match_records([ll] * n, [("kernel", 8, 1, 0)], n) is None
    assert cases.match_records([ll] * (n - 1), [("kernel", 8, 1, 0)], n)
    assert cases.match_records([ll] * (n + 1), [("kernel", 8, 1, 0)], n)
    assert cases.match_records([(1, n, 4, 0)] * n, [("kernel", 8, 1, 0)], n)        # the fold path instead
    assert cases.match_records([(8, n, 1, 2 << 8)] * n, [("kernel", 8, 1, 0)], n)   # a grouped launch instead
    assert cases.match_records([(2, n, 4, 0), (3, n, 1, 4)], [("fold",)], n) is None
    assert cases.match_records([], [("fold",)], n) and cases.match_records([ll] * n, [("fold",)], n)
    mixed = [("kernel", 8, 1, 0), ("fold",), ("kernel", 8, 1, 0)]
    assert cases.match_records([ll] * n + [(2, n, 4, 0)] + [ll] * n, mixed, n) is None
    assert cases.match_records([], [], n) is None and cases.match_records([ll], [], n)
    assert cases.match_records([], [("error", 5)], n) is None and cases.match_records([ll], [("error", 5)], n)
    pre = (3, 1, 1, 0)
    assert cases.match_records([pre, ll] * n, [("premul", 8, 1)], n) is None
    assert cases.match_records([ll] * n, [("premul", 8, 1)], n) and cases.match_records([pre] * n + [ll] * n,
                                                                                         [("premul", 8, 1)], n)


def test_chain_stays_exact(oracle):
    """Every value of the chain is a whole number below 2^24 in magnitude: fp32 holds it exactly,
    so every order of summation gives the same bits."""
    for n in range(2, cases.TWO_STREAM_MAX_N + 1):
        assert cases.chain_bound(n) == 8 * n ** 4 < 2 ** 24
    n = cases.ROUTE_N
    scenarios = cases.group_scenarios()
    si = next(i for i, sc in enumerate(scenarios) if sc.name == "chain")
    sc = scenarios[si]
    first = cases.initial_buffers(oracle, si, sc, n)
    for r in range(n):
        for name, (elts, dt, is_input) in cases.buffer_specs(sc, n).items():
            assert dt == cases.F32
            if is_input:
                x = first[r][name].view(np.float32)
                assert x.size == elts and np.all(x == np.round(x)) and np.abs(x).max() <= cases.F32_INPUT_MAX
    final = cases.simulate(oracle, si, sc, n)
    x = np.stack([first[r]["x"].view(np.float32).astype(np.float64) for r in range(n)]).sum(0)
    m = cases.LL_COUNT
    for r in range(n):
        assert np.array_equal(final[r]["y1"].view(np.float32), x)
        assert np.array_equal(final[r]["y2"].view(np.float32), n * x)
        assert np.array_equal(final[r]["y3"].view(np.float32)[:m], n * n * x)
        y4 = final[r]["y4"].view(np.float32)
        assert np.array_equal(y4[:m], n ** 3 * x) and np.abs(y4).max() <= cases.chain_bound(n)
        tail = np.stack([first[q]["y3"].view(np.float32)[m:].astype(np.float64) for q in range(n)]).sum(0)
        assert np.array_equal(y4[m:], tail)   # past the chain's head y3 still holds its first contents


def test_simulate_models_every_kind(oracle):
    n = 3
    sc = cases.Scenario("kinds", "default",
                        [[cases.Call("rs", cases.F32, cases.SUM, 7, "a", "b")],
                         [cases.Call("red", cases.F32, cases.SUM, 7, "a", "c", root=2)],
                         [cases.Call("ar", cases.F32, cases.SUM, 5, "a", "d", bad_rank=1)],
                         [cases.Call("ar", cases.INT8, cases.SUM, 33, "e", "f")]], [[("fold",)]] * 4)
    first = cases.initial_buffers(oracle, 9, sc, n)
    final = cases.simulate(oracle, 9, sc, n)
    a = np.stack([first[r]["a"].view(np.float32) for r in range(n)]).sum(0)
    e = np.stack([first[r]["e"].view(np.int8) for r in range(n)]).astype(np.int64).sum(0).astype(np.int8)
    for r in range(n):
        assert np.array_equal(final[r]["b"].view(np.float32), a[7 * r:7 * r + 7])
        c = final[r]["c"]
        assert np.array_equal(c.view(np.float32), a[:7]) if r == 2 else (c == 0xA5).all()
        assert (final[r]["d"] == 0xA5).all()                       # the mismatched call writes nothing
        assert np.array_equal(final[r]["f"].view(np.int8), e)    # integer sums wrap
        assert np.array_equal(final[r]["a"], first[r]["a"])
