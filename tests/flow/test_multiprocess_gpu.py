"""The Simple transport's flow control (kSimpleColl, kSimpleRing) at every slot
depth NBX_SIMPLE_SLOTS accepts and with the next-round prefetch on and off,
and its first use at 8 ranks on default settings — outputs bit for bit against
the oracle, and the protocol state itself (per-cell counters and flag words,
read through nbxDebugSimpleState once every rank is idle) word for word
against tests/simple_model.py and against the pairwise invariants that hold
with or without a model.

tests/flow/cases.py holds the call table and why it is what it is;
tests/test_simple_flow_cpu.py checks the table and the state checker without
a GPU. One spawn of n ranks per test: every rank creates the communicators one
after another, each under its own environment, and only one is alive at a
time: create, run both passes back to back with no host synchronisation, meet,
read the state, run the grouped launch, meet, read it again, destroy.

The file carries the name of tests/test_multiprocess_gpu.py on purpose: the
GPU suite orders files by name (tests/conftest.py GPU_FILE_ORDER)."""
import multiprocessing as mp
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import mp_diag
from tests.flow import cases
from tests.test_multiprocess_gpu import _run_ranks

pytestmark = pytest.mark.gpu

# Every communicator's send and receive buffers are allocated after it was
# created and released after it was destroyed, as an application's are: from
# the second communicator on they are device memory allocated after
# communicators came and went in the process, next to the connection buffers
# the library keeps for the next communicator (comm_mp_connect.cc allocSyncMem;
# DESIGN §6.4). Every rank compares its send buffers with what it uploaded at
# the end, so a report can tell a wrong output from a changed input.
GUARD = 16          # bytes of 0xA5 either side of every output
MEET_SEC = 120      # the ranks meet on the host before the state is read (NBX_TIMEOUT_SEC is 60)


def _plan(which, n):
    """[(config, environment, calls, grouped calls)] of one test."""
    if which == "first_use":
        return [(cfg, cases.FIRST_USE_ENV[cfg.name], list(cases.FIRST_USE), []) for cfg in cases.FIRST_USE_CONFIGS]
    return [(cfg, cases.comm_env(cfg), cases.sequence(n, cfg), cases.group_calls(n, cfg)) for cfg in cases.CONFIGS]


def _child_flow(uid0, rank, n, q, uids, barrier, which):
    try:
        import os

        import torch
        from tests.conftest import load_package
        nbx = load_package()
        lib = nbx.load_library()
        torch.cuda.set_device(0)
        st = torch.cuda.current_stream().cuda_stream
        out = {}
        for (cfg, env, calls, grouped), uid in zip(_plan(which, n), (uid0,) + tuple(uids)):
            for k in cases.ENV_KEYS:   # each communicator under its own environment
                os.environ.pop(k, None)
            os.environ.update(env)
            comm = nbx.Communicator.init_rank(n, nbx.ncclUniqueId.from_buffer_copy(uid), rank)
            settings = mp_diag.comm_settings(nbx, comm)
            words = 4 * n * settings["simpleGrid"]
            # every buffer before the first call: nothing between the calls touches the host or the stream
            bufs = []
            for call in calls + grouped:
                x = cases.rank_input(call, n, rank).view(np.uint8)
                host = np.full(GUARD + x.size + GUARD, 0xA5, dtype=np.uint8)
                host[GUARD:GUARD + x.size] = x
                tx = torch.from_numpy(host).cuda()
                ty = torch.full((GUARD + call.count * call.eb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
                assert tx.data_ptr() % 16 == 0 and ty.data_ptr() % 16 == 0
                bufs.append((tx, ty))
            torch.cuda.synchronize()

            def issue(call, tx, ty):
                sp, rp = tx.data_ptr() + GUARD, ty.data_ptr() + GUARD
                if call.kind == "ar":
                    comm.all_reduce(sp, rp, call.count, call.dtype, call.op, st)
                elif call.kind == "rs":
                    comm.reduce_scatter(sp, rp, call.count, call.dtype, call.op, st)
                else:
                    comm.reduce(sp, rp if rank == call.root else 0, call.count, call.dtype, call.op, call.root, st)

            def at_rest():
                """Every rank idle, then the state; the peers post into this rank's flag words."""
                torch.cuda.synchronize()
                err = comm.async_error()
                if err:
                    barrier.abort()
                    raise RuntimeError(f"{cfg.name}: asynchronous error {err}: "
                                       f"{(lib.ncclGetLastError(None) or b'').decode(errors='replace')}")
                barrier.wait(MEET_SEC)
                state = nbx.simple_state(comm, words)
                too_small = nbx.simple_state(comm, words - 1)
                barrier.wait(MEET_SEC)   # nobody launches again before everyone has read
                return state, too_small

            nbx.launch_log_reset()
            for call, (tx, ty) in zip(calls, bufs):
                issue(call, tx, ty)
            n_recs, recs = nbx.launch_log()
            state, too_small = at_rest()
            res = {"settings": settings, "records": (n_recs, recs), "state": state, "too_small": too_small,
                   "ptrs": [(tx.data_ptr(), ty.data_ptr()) for tx, ty in bufs]}
            if grouped:
                nbx.launch_log_reset()
                nbx.group_start()
                for call, (tx, ty) in zip(grouped, bufs[len(calls):]):
                    issue(call, tx, ty)
                nbx.group_end()
                res["group_records"] = nbx.launch_log()
                res["group_state"], _ = at_rest()
            res["outputs"] = [ty.cpu().numpy() if call.kind != "red" or rank == call.root else None
                              for call, (_tx, ty) in zip(calls + grouped, bufs)]
            res["inputs_changed"] = []
            for ci, (call, (tx, _ty)) in enumerate(zip(calls + grouped, bufs)):
                x = cases.rank_input(call, n, rank).view(np.uint8)
                back = tx.cpu().numpy()
                image = np.full(back.size, 0xA5, dtype=np.uint8)
                image[GUARD:GUARD + x.size] = x
                if not np.array_equal(back, image):
                    bad = np.flatnonzero(back != image)
                    res["inputs_changed"].append((ci, int(bad.size), int(bad[0]), bytes(back[bad[:16]]).hex()))
            comm.destroy()
            del bufs
            out[cfg.name] = res
        q.put((rank, "ok", out))
    except Exception:
        import traceback
        try:
            barrier.abort()   # the peers fail at once instead of waiting out the meeting
        except Exception:
            pass
        q.put((rank, "error", traceback.format_exc()))


def _reference(oracle, which, n, grid, slice_bytes):
    """{config name: (expected outputs per call, model run)}: the oracle for the
    outputs, the model with the communicator's settings for the state."""
    ref, folded = {}, {}
    for cfg, _env, calls, grouped in _plan(which, n):
        key = (cfg.slots, cfg.ring)   # the prefetch changes neither the calls nor the fold order
        if key not in folded:
            folded[key] = [cases.expected(oracle, c, [cases.rank_input(c, n, r) for r in range(n)], n, cfg.ring)
                           for c in calls + grouped]
        model = cases.run_model(n, cfg, calls, grid, slice_bytes)
        ref[cfg.name] = (folded[key], model, cases.run_model_group(model, n, cfg, grouped, grid, slice_bytes)
                         if grouped else None)
    return ref


def _check_outputs(cfg, n, calls, first_grouped, exp, res, model, gmodel, grid, slice_bytes, failures):
    checked = 0
    for ci, call in enumerate(calls):
        part = "grouped " if ci >= first_grouped else ""
        for r in range(n):
            buf = res[r][cfg.name]["outputs"][ci]
            ctx = (f"{cfg.name} {part}call {ci} ({call.kind} {call.count} x {call.eb} B, root {call.root}) "
                   f"rank {r} of {n}")
            if r not in exp[ci]:
                assert buf is None and call.kind == "red"
                continue
            e = np.ascontiguousarray(exp[ci][r])
            assert buf.size == GUARD + e.nbytes + GUARD
            if not ((buf[:GUARD] == 0xA5).all() and (buf[GUARD + e.nbytes:] == 0xA5).all()):
                failures.append(f"{ctx}: guard bytes overwritten: front {np.flatnonzero(buf[:GUARD] != 0xA5)[:8]}, "
                                f"back {np.flatnonzero(buf[GUARD + e.nbytes:] != 0xA5)[:8]}")
            got = buf[GUARD:GUARD + e.nbytes].copy().view(e.dtype)
            checked += 1
            if np.array_equal(got, e):
                continue
            base = r * e.size if call.kind == "rs" else 0
            cand = {f"raw_input_rank{j}": cases.rank_input(call, n, j)[base:base + e.size] for j in range(n)}
            cand["guard_fill"] = np.full(e.nbytes, 0xA5, np.uint8).view(e.dtype)
            if ci >= first_grouped:   # a segment of the grouped launch: the launch's own cut
                d = mp_diag.describe_mismatch(got, e, None, base, cand)
                bad = np.flatnonzero(got != e)
                loc = gmodel[1].locate(ci - first_grouped, bad + base)
                failures.append(f"{ctx}: {mp_diag.format_mismatch(d)}; first at {loc[0].tolist()} last at "
                                f"{loc[-1].tolist()} (segment, block, round, workgroup, slice offset) of the grouped "
                                f"launch, sliceOff {gmodel[1].slice_off}")
                continue
            d = mp_diag.describe_mismatch(got, e, cases.geometry(call, n, grid, slice_bytes, cfg.ring), base, cand)
            where = ""
            if d.get("cells"):
                c = d["cells"][0]
                where = "; top cell " + cases.slot_report(call, cfg, n, r, (c["block"], c["round"], c["workgroup"]),
                                                          model.starts[ci])
            failures.append(f"{ctx}: {mp_diag.format_mismatch(d)}{where}")
    return checked


def _run_and_check(nbx, oracle, which, n, monkeypatch, grid_guess, slice_bytes):
    monkeypatch.setenv("NBX_BOOTSTRAP_TIMEOUT", "60")
    monkeypatch.setenv("NBX_TIMEOUT_SEC", "60")
    for k in cases.ENV_KEYS + ("NBX_CHECK_PLANS", "NCCL_CHECK_POINTERS", "NBX_CHECK_SLICES", "NCCL_BUFFSIZE",
                               "NCCL_MAX_NCHANNELS", "NCCL_MIN_NCHANNELS", "NBX_GROUP_BATCH"):
        monkeypatch.delenv(k, raising=False)
    plan = _plan(which, n)
    barrier = mp.get_context("spawn").Barrier(n)
    # the references are worked out on a host thread while the ranks run
    with ThreadPoolExecutor(1) as pool:
        working = pool.submit(_reference, oracle, which, n, grid_guess, slice_bytes)
        res = _run_ranks(nbx, n, _child_flow, [bytes(nbx.get_unique_id()) for _ in plan[1:]], barrier, which)
        ref = working.result()

    failures, outputs, state_words = [], 0, 0
    for cfg, _env, calls, grouped in plan:
        s = res[0][cfg.name]["settings"]
        grid = s["simpleGrid"]
        exp, model, gmodel = ref[cfg.name]
        if grid != grid_guess:   # the first-use test takes the grid from the communicator
            model = cases.run_model(n, cfg, calls, grid, slice_bytes)
            gmodel = cases.run_model_group(model, n, cfg, grouped, grid, slice_bytes) if grouped else None
        for r in range(n):
            got = res[r][cfg.name]
            # the settings the communicator was asked for took effect, on every rank
            assert got["settings"] == s, (cfg.name, r, got["settings"], s)
            assert s["sliceBytes"] == slice_bytes and s["slots"] == cfg.slots, (cfg.name, s)
            assert s["checkPlans"] == 0 and s["checkSlices"] == 0 and s["groupBatch"] == 1, (cfg.name, s)
            assert got["state"] is not None and got["state"][2] == cfg.prefetch, (cfg.name, r, got["state"] and got["state"][2])
            assert len(got["state"][0]) == len(got["state"][1]) == 4 * n * grid
            assert got["too_small"] is None, (cfg.name, r, "nWords one short of the arrays was accepted")
            for ci, nbad, first, sample in got["inputs_changed"]:
                failures.append(f"{cfg.name} call {ci} rank {r}: the send buffer no longer holds its input "
                                f"({nbad} bytes of the guarded buffer, first at {first}: {sample})")
            # every call ran the intended kernel, once, unchecked and on its own
            total, recs = got["records"]
            want = [(cases.family_of(cfg), n, 0, 0)] * len(calls)
            if total != len(calls) or [tuple(x) for x in recs] != want:
                failures.append(f"{cfg.name} rank {r}: launch record {total} {recs}, expected {len(calls)} x {want[0]}")
            if grouped:
                total, recs = got["group_records"]
                want = [(cases.family_of(cfg), n, 0, len(grouped) << nbx.LAUNCH_SEGS_SHIFT)]
                if total != 1 or [tuple(x) for x in recs] != want:
                    failures.append(f"{cfg.name} rank {r}: grouped launch record {total} {recs}, expected {want}")
        if which == "matrix":
            assert grid == cases.GRID, (cfg.name, s)
        outputs += _check_outputs(cfg, n, calls + grouped, len(calls), exp, res, model, gmodel, grid, slice_bytes,
                                  failures)
        # the state against the model, then the invariants that need no model (again after the group)
        states = [res[r][cfg.name]["state"][:2] for r in range(n)]
        failures += [f"{cfg.name} state vs model: {x}" for x in cases.check_model(states, model.comm, n, grid)]
        failures += [f"{cfg.name} at rest: {x}" for x in cases.check_pairs(states, n, grid)]
        state_words += sum(len(a) + len(b) for a, b in states)
        if grouped:
            after = [res[r][cfg.name]["group_state"][:2] for r in range(n)]
            # the grouped launch against the grouped model, word for word: the slot uses it should have consumed
            failures += [f"{cfg.name} state after the grouped launch vs model: {x}"
                         for x in cases.check_model(after, gmodel[0].comm, n, grid)]
            failures += [f"{cfg.name} after the grouped launch: {x}" for x in cases.check_pairs(after, n, grid)]
            if all(np.array_equal(a[0], b[0]) for a, b in zip(states, after)):
                failures.append(f"{cfg.name}: the grouped launch left every counter where it was")
    # AllReduce and ReduceScatter on every rank, Reduce on its root
    assert outputs == sum(sum(n if c.kind != "red" else 1 for c in calls + grouped) for _c, _e, calls, grouped in plan)
    print(f"flow {which} at {n} ranks: {len(plan)} communicators, {outputs} outputs and {state_words} state words "
          f"compared, {len(failures)} failure(s)", file=sys.stderr)
    if failures:
        head = f"{len(failures)} failure(s) in {outputs} outputs and {state_words} state words at {n} ranks"
        raise AssertionError(head + ":\n" + "\n".join(failures[:12]) + "\n" +
                             mp_diag.emit_summary([head] + [f.splitlines()[0][:160] for f in failures[:4]]))
    return outputs, state_words


@pytest.mark.parametrize("n", cases.NS)
def test_simple_flow_matrix(nbx, oracle, n, monkeypatch):
    """Twelve communicators (direct: slots 2, 3, 4, 8 x prefetch 0, 1; ring:
    slots 2, 3, 4, 8), grid 3, 4 KiB slices; on each the 24-call table as
    uint32 Sum and as uint64 Sum, 48 calls back to back, then four AllReduces
    in one group. Per communicator: the settings and the hook say grid, slice,
    slots and prefetch took effect; the launch record says every call ran
    kSimpleColl (11) or kSimpleRing (12), unchecked and alone, and the group
    ran as one launch of four segments; every output equals the oracle in the
    schedule's order with its guard bytes intact; every rank's counters and
    flag words equal the model's, word for word; the pairwise invariants hold
    at rest; after the grouped launch the counters and flag words equal the
    grouped model's (simple_model.run_group), word for word, and the pairwise
    invariants hold again. Every rank and call is checked before the test fails; a wrong
    output is reported with its (block, round, workgroup) cells and the slot
    and use of the top one."""
    outputs, words = _run_and_check(nbx, oracle, "matrix", n, monkeypatch, cases.GRID, cases.SLICE)
    assert outputs == 12 * (2 * (16 * n + 8) + 4 * n) and words == 12 * n * 2 * 4 * n * cases.GRID


def test_simple_first_use_8_ranks(nbx, oracle, monkeypatch):
    """A fresh default communicator's first Simple calls at 8 ranks (direct,
    then NCCL_ALGO=Ring): three int32 ncclMax AllReduces of 1,000,003
    elements, three ReduceScatters of 125,004, three Reduces to root 5 — one
    round on every workgroup, so each kind's calls are the first use of slot
    0, the first use of slot 1 and the first reuse of slot 0 of every cell.
    The same checks as the matrix; the grid comes from the communicator's
    settings and goes into the model."""
    _run_and_check(nbx, oracle, "first_use", cases.FIRST_USE_N, monkeypatch, 32, 64 << 10)
