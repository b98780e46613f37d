"""The in-process clique's in-kernel transport, case by case: the
deterministic half of its tests (tests/test_clique_transport_gpu.py is the
randomized half). ncclCommInitAll's ranks share the one GPU, NBX_CLIQUE_LL=1
forces the transport on, and every stream has a hardware queue of its own, so
each test starts one fresh process (tests/clique/worker.py, through
subprocess.run with a time limit) whose environment carries
tests/clique/cases.CHILD_ENV before HIP loads, and reads the results that
process wrote under tmp_path.

  1. every (type, op) of tests/edges/cases.py through kLLColl, kLL128Coll,
     kLL128AllReduce2, kSimpleColl (packs and elements) and kSimpleRing at 2, 3
     and 5 ranks, bit for bit against the oracle in the schedule's operand order;
  2. a short table at 8 ranks (the U = 4 fold; the grid caps at maxShare = 8);
  3. one scenario per routing rule of cliqueInKernel;
  4. groups, the hand-over between the in-kernel and the fold path across
     streams, in-place calls, and a user PreMulSum with per-rank scalars.

Every case is checked on its output, its guard bytes and the calling thread's
launch record: one thread launches all n ranks, so an in-kernel case leaves
exactly n records of its kernel's family, and a record of families 1-5 means
the call took the fold path. tests/clique/cases.py holds the tables and why
they are what they are; tests/test_clique_cases_cpu.py checks them without a
GPU.

The file carries the name of tests/test_clique_transport_gpu.py on purpose:
the GPU suite orders files by name (tests/conftest.py GPU_FILE_ORDER).

Time limits of the child processes: three times the wall time of
tests/edges/test_multiprocess_gpu.py::test_collective_edges at the same rank
count (the same kernels on the same table; the clique adds one thread
launching n ranks in turn) — EDGES_SECONDS, measured on an MI355X."""
import os
import pickle
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import mp_diag
from tests.clique import cases
from tests.matrix import inputs as mi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WORKER = os.path.join(ROOT, "tests", "clique", "worker.py")
GUARD = cases.GUARD

# wall seconds of test_collective_edges[n], measured on an MI355X in the session that set these limits
EDGES_SECONDS = {2: 4.94, 3: 3.55, 5: 4.65}
LIMIT = {n: 3 * s for n, s in EDGES_SECONDS.items()}
SHORT_LIMIT = LIMIT[3]        # parts 3 and 4 run at 3 ranks
EIGHT_LIMIT = LIMIT[5]        # no edge test runs at 8 ranks: the limit of the largest rank count that has one


def _run_worker(tmp_path, mode, n, limit, paths=None):
    out_file = tmp_path / f"{mode}_{n}.pkl"
    env = {k: v for k, v in os.environ.items() if k not in cases.SCRUB_ENV}
    env.update(cases.CHILD_ENV)
    cmd = [sys.executable, WORKER, mode, str(n), str(out_file)] + ([",".join(paths)] if paths else [])
    t0 = time.perf_counter()
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=ROOT, env=env)
    print(f"worker {mode} at {n} ranks: {time.perf_counter() - t0:.2f} s of a limit of {limit:.2f} s")
    res = None
    if out_file.exists():
        with open(out_file, "rb") as f:
            res = pickle.load(f)
    if res is not None and "async_error" in res:
        done = sorted(str(k) for k in res if isinstance(k, tuple))
        pytest.fail(f"a device wait gave up: {res['async_error']}\n  settings: {res.get('info')}\n"
                    f"  {len(done)} results before it, the last: {done[-3:]}\n{proc.stderr[-1500:]}")
    assert proc.returncode == 0 and res is not None, f"worker exit {proc.returncode}:\n{proc.stderr[-3000:]}"
    return res


def _check_settings(info, names, n):
    for name in names:
        assert all(m >= 0 for m in info[name]["masks"]) and len(info[name]["masks"]) == n, (name, info[name])
        for st in info[name]["settings"]:
            assert st and st["checkPlans"] == 0 and st["checkSlices"] == 0, (name, st)
            if name in ("simple", "ring"):   # cases.py's iteration arithmetic holds here too
                assert st["simpleGrid"] == cases.edges.SIMPLE_GRID and st["sliceBytes"] == 64 << 10, (name, st)


def _compare(oracle, failures, ctx, buf, shift, exp, dt, geom=None, base=0):
    """One output with its guards against the expectation (mi.assert_same's rule: NaN only as NaN)."""
    e = np.ascontiguousarray(exp)
    lo = GUARD + shift
    assert buf.size == lo + e.nbytes + GUARD, ctx
    if not ((buf[:lo] == 0xA5).all() and (buf[lo + e.nbytes:] == 0xA5).all()):
        failures.append(f"{ctx}: guard bytes overwritten: front {np.flatnonzero(buf[:lo] != 0xA5)[:8]}, "
                        f"back {np.flatnonzero(buf[lo + e.nbytes:] != 0xA5)[:8]}")
    got = buf[lo:lo + e.nbytes].copy().view(oracle.NP_STORAGE[dt])
    if np.array_equal(got.view(np.uint8), e.view(np.uint8)):
        return
    try:
        mi.assert_same(got, e, dt)
    except AssertionError as err:
        d = mp_diag.describe_mismatch(got, e, geom, base)
        failures.append(f"{ctx}: {err}\n    all differing bytes (NaN payloads included): {mp_diag.format_mismatch(d)}")


def _raise(failures, checked, what):
    if failures:
        head = f"{len(failures)} failure(s) in {checked} outputs, {what}"
        raise AssertionError(head + ":\n" + "\n".join(failures[:8]) + "\n" +
                             mp_diag.emit_summary([head] + [f.splitlines()[0][:160] for f in failures[:4]]))


def _run_table(oracle, tmp_path, mode, n, table, limit, paths=None):
    """table: [(path, index, kind, dtype, op)]. Outputs: mi.assert_same against cases.expected on every
    rank (a Reduce: its root), guards intact. Launch record: exactly n entries of (the path's family,
    n, the host's unroll field, 0). The count of checked outputs is the table's."""
    def fold_all():   # on a host thread while the ranks run
        return {(p, i): cases.expected(oracle, p, kind, dt, op, n, cases.root_of(i, n)) for p, i, kind, dt, op in table}
    with ThreadPoolExecutor(1) as pool:
        folding = pool.submit(fold_all)
        res = _run_worker(tmp_path, mode, n, limit, paths)
        expected = folding.result()
    info = res["info"]
    _check_settings(info, sorted({cases.PATH_COMM[p] for p, *_ in table}), n)
    failures, checked = [], 0
    for p, i, kind, dt, op in table:
        bufs, recs = res[(mode, p, i)]
        root = cases.root_of(i, n)
        ctx = f"{p} {kind} {oracle.TYPE_NAMES[dt]} op {op} root {root} at {n} ranks"
        want = [(cases.family_of(p, kind, n), n, cases.host_unroll(p), 0)] * n
        if [tuple(x) for x in recs] != want:
            failures.append(f"{ctx}: launch record {recs}, expected {want}")
        geom = None
        if cases.PATH_COMM[p] in ("simple", "ring"):
            st = info[cases.PATH_COMM[p]]["settings"][0]
            geom = mp_diag.simple_geometry(kind, cases.count_of(oracle, p, dt), cases.itemsize(oracle, dt), n,
                                           st["simpleGrid"], st["sliceBytes"], ring=p == "ring")
        for r in range(n):
            if r not in expected[(p, i)]:
                assert bufs[r] is None and kind == "red"
                continue
            checked += 1
            _compare(oracle, failures, f"{ctx} rank {r}", bufs[r], cases.shift_of(oracle, p, dt), expected[(p, i)][r],
                     dt, geom, r * cases.count_of(oracle, p, dt) if kind == "rs" else 0)
    assert checked == sum(n if kind != "red" else 1 for _, _, kind, _, _ in table)   # nothing is skipped
    _raise(failures, checked, f"{mode} at {n} ranks")


@pytest.mark.parametrize("n", cases.NS)
def test_clique_collective_edges(oracle, tmp_path, n):
    """Part 1: the 756 cases of tests/edges/cases.py, one at a time (group_start, the n ranks' calls
    on their own streams, group_end), through the four cliques LL, LL128, Simple direct and Simple
    ring, each created under its own environment by Communicator.init_all([0] * n)."""
    table = [(p, i, *c) for p in cases.PATHS for i, c in enumerate(cases.path_cases(p))]
    assert len(table) == 756
    _run_table(oracle, tmp_path, "edges", n, table, LIMIT[n])


def test_clique_eight_ranks(oracle, tmp_path):
    """Part 2: fp32 and bf16, Sum and Avg, AllReduce / ReduceScatter / Reduce through ll, ll128,
    ll128x2, simple and ring at 8 ranks (nine streams): the U = 4 fold of kSimpleColl and the LL /
    LL128 grid caps at maxShare = 8. Same assertions as part 1."""
    table = [(p, i, *c) for p in cases.EIGHT_PATHS for i, c in enumerate(cases.eight_cases(p))]
    _run_table(oracle, tmp_path, "eight", cases.EIGHT_N, table, EIGHT_LIMIT)


def _check_scenarios(oracle, res, scenarios, n):
    info = res["info"]
    failures, checked = [], 0
    for si, sc in enumerate(scenarios):
        got = res[("scenario", sc.name)]
        masks = info[sc.comm]["masks"]
        if sc.comm in cases.IN_KERNEL_COMMS:
            assert all(m >= 0 for m in masks) and all(info[sc.comm]["settings"]), (sc.comm, info[sc.comm])
        else:
            assert all(m == -1 for m in masks), (sc.comm, masks)   # no transport: every size goes to the fold
        for gi, (phases, recs, code) in enumerate(zip(sc.expect, got["records"], got["codes"])):
            ctx = f"{sc.name} group {gi}"
            want_code = phases[0][1] if phases and phases[0][0] == "error" else 0
            if code != want_code:
                failures.append(f"{ctx}: ncclGroupEnd returned {code}, expected {want_code}")
            why = cases.match_records(recs, phases, n)
            if why:
                failures.append(f"{ctx}: {why}")
            if sc.protos is not None and got["protos"][gi] != sc.protos[gi]:
                failures.append(f"{ctx}: nbxDebugChooseProto says {got['protos'][gi]}, expected {sc.protos[gi]}")
        assert len(got["records"]) == len(sc.groups) == len(sc.expect)
        final = cases.simulate(oracle, si, sc, n)
        for r in range(n):
            for name, (elts, dt, _) in cases.buffer_specs(sc, n).items():
                checked += 1
                _compare(oracle, failures, f"{sc.name} buffer {name} rank {r}", got["buffers"][r][name], 0,
                         final[r][name].view(oracle.NP_STORAGE[dt]), dt)
    return failures, checked


def test_clique_routing(oracle, tmp_path):
    """Part 3, at 3 ranks: a call whose ranks share a stream leaves fold records only; a count of 0
    leaves none and no error; NBX_CLIQUE_SIMPLE_MAX_BYTES=262144 keeps 262,144 B (AllReduce) and
    3 x 87,380 = 262,140 B (ReduceScatter: the bound is on the bytes sent, n x count) in-kernel and
    sends 262,148 B and 262,152 B to the fold; NBX_CLIQUE_SIMPLE=0 sends the Simple-sized 300,011 B
    to the fold and keeps 20,011 B on kLLColl; NBX_CLIQUE_LL=0 leaves no transport
    (nbxDebugCommProtoMask == -1) and every size on the fold; a collective whose count differs on
    one rank fails ncclGroupEnd with ncclInvalidUsage, launches nothing and leaves nothing queued
    (the next call is exact). Every buffer is exact against the oracle, guards included."""
    n = cases.ROUTE_N
    scenarios = cases.routing_scenarios()
    res = _run_worker(tmp_path, "routing", n, SHORT_LIMIT)
    failures, checked = _check_scenarios(oracle, res, scenarios, n)
    _raise(failures, checked, "routing")


def test_clique_groups_and_handover(oracle, tmp_path):
    """Part 4, at 3 ranks. Six independent LL-sized AllReduces of one group are one launch per rank
    with a six-entry segment table (what mp_diag.group_runs, the mirror of runMpGroup's cut, says
    under the communicator's settings). A group whose third call reads the second's output is cut
    there: two launches per rank, the third output the oracle applied to the second. A group of
    [LL-sized, Simple-sized on the shared stream, LL-sized] leaves in-kernel, fold, in-kernel
    records. In place: AllReduce with recv == send and ReduceScatter with recv == send + r x count,
    once per path, fp16.

    The chain y1 = AR(x) in-kernel on streams A, y2 = AR(y1) by fold on the shared stream, y3 =
    AR(y2) in-kernel on streams B, y4 = AR(y3 ...) by fold on streams A (y3 is the head of a
    buffer long enough to pass the communicator's Simple byte bound, the only way to the fold on
    distinct streams: tests/clique/cases.py) runs with no host synchronisation in between;
    its inputs are small whole numbers in fp32, so every order of
    summation is exact and only a missed ordering can change a value. A race need not show on every
    run: this pins the ordering the host code sets up (cliqueOrderBefore / cliqueOrderAfter, extDone
    / extStream against lastSeq), not the absence of races."""
    n = cases.ROUTE_N
    scenarios = cases.group_scenarios()
    res = _run_worker(tmp_path, "groups", n, SHORT_LIMIT)
    _check_settings(res["info"], cases.COMMS, n)
    failures, checked = _check_scenarios(oracle, res, scenarios, n)
    # the segment table is what the mirror of runMpGroup's cut says under the default NBX_GROUP_BATCH
    seg = next(sc for sc in scenarios if sc.name == "segment_table")
    st = res["info"][seg.comm]["settings"][0]
    assert st["groupBatch"] == 1
    plan = cases.group_plan(oracle, seg.groups[0], n, st)
    assert plan.records == [(cases.FAM_LL, n, 1, len(cases.SEGMENT_COUNTS) << cases.SEGS_SHIFT)], plan
    assert [("kernel", *rec[:1], *rec[2:]) for rec in plan.records] == list(seg.expect[0])

    for path, kind in cases.inplace_cases():
        dt = cases.F16
        bufs, recs = res[("inplace", path, kind)]
        ctx = f"in place {path} {kind}"
        want = [(cases.family_of(path, kind, n), n, cases.host_unroll(path), 0)] * n
        if [tuple(x) for x in recs] != want:
            failures.append(f"{ctx}: launch record {recs}, expected {want}")
        exp = cases.expected(oracle, path, kind, dt, cases.SUM, n, 0)
        count = cases.count_of(oracle, path, dt)
        for r in range(n):
            if kind == "rs":   # only the rank's own block of its send buffer changes
                image = np.ascontiguousarray(cases.rank_input(oracle, path, kind, dt, n, r)).copy()
                image[r * count:(r + 1) * count] = exp[r]
            else:
                image = exp[r]
            checked += 1
            _compare(oracle, failures, f"{ctx} rank {r}", bufs[r], cases.shift_of(oracle, path, dt), image, dt)

    _raise(failures, checked, "groups and hand-over")


def test_clique_user_premulsum(oracle, tmp_path):
    """Part 4, at 3 ranks: a user PreMulSum with another scalar on every rank, host-immediate and
    device-resident, AllReduce / ReduceScatter / Reduce at the ll, ll128 and simple sizes for fp16,
    fp32 and int32, against tests/test_multiprocess_gpu.py's _premul_expected with its root
    convention (1 % n). The record is one pre-pass of the fold families per rank (nbxReduceMulti
    into the communicator's scratch), then the collective's kernel."""
    n = cases.ROUTE_N
    res = _run_worker(tmp_path, "premul", n, SHORT_LIMIT)
    _check_settings(res["info"], sorted({cases.PATH_COMM[p] for p in cases.PREMUL_PATHS}), n)
    failures, checked = [], 0
    for path, kind, dt, dev in cases.premul_cases():
        bufs, recs = res[("premul", path, kind, dt, dev)]
        ctx = f"PreMulSum {path} {kind} {oracle.TYPE_NAMES[dt]} {'device' if dev else 'host'} scalar"
        why = cases.match_records(recs, [("premul", cases.family_of(path, kind, n), cases.host_unroll(path))], n)
        if why:
            failures.append(f"{ctx}: {why}")
        exp = cases.premul_expected(oracle, path, kind, dt, n)
        for r in range(n):
            if r not in exp:
                assert bufs[r] is None and kind == "red"
                continue
            checked += 1
            _compare(oracle, failures, f"{ctx} rank {r}", bufs[r], 0, exp[r], dt)
    assert checked == sum(n if kind != "red" else 1 for _, kind, _, _ in cases.premul_cases())
    _raise(failures, checked, "user PreMulSum")
