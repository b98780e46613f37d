"""Grouped collective launches, segment by segment on every protocol: the
segment lookup every thread of a grouped kernel starts with (llMsg over
LLSeg.packOff in kLLColl / kLL128Coll, simpleSlice over SimpleSeg.sliceOff in
kSimpleColl / kSimpleRing), the host arithmetic that fills the tables
(mpLaunchLL, mpLaunchSimple) and the cut of a group into launches (runMpGroup).

test_group_segments: four communicators (ll, ll128, simple, ring) in one spawn
per n; on each, for AllReduce and ReduceScatter, ONE ncclGroupStart/End of 8
(type, op) pairs x 8 segments whose sizes, placements and in-place member
tests/groups/cases.py tabulates. The launch record read after ncclGroupEnd must
be eight launches of eight segments; every output must equal the oracle in the
schedule's own operand order, with every other byte of both arenas (guards,
padding, the send buffers) as it was uploaded; and the Simple communicators'
counters and flag words at rest must equal the grouped model's
(tests/simple_model.py run_group), word for word.

test_group_cut_rules: one group per cut rule on a default communicator, the
launch record against mp_diag.group_runs and every byte of the group's arena
against the calls folded in call order on the host.

tests/test_group_segments_cpu.py checks the tables, the mirror and the model
without a GPU. The file carries the name of tests/test_multiprocess_gpu.py on
purpose: the GPU suite orders files by name (tests/conftest.py GPU_FILE_ORDER)."""
import multiprocessing as mp
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import mp_diag
from tests import simple_model as sm
from tests.flow import cases as flow
from tests.groups import cases
from tests.matrix import inputs as mi
from tests.test_multiprocess_gpu import _run_ranks

pytestmark = pytest.mark.gpu

MEET_SEC = 120      # the ranks meet on the host before the state is read (NBX_TIMEOUT_SEC is 60)
COLLECTIVE_FAMILIES = (cases.FAM_LL, cases.FAM_LL128, cases.FAM_LL128X2, cases.FAM_SIMPLE, cases.FAM_RING)


def _child_segments(uid_ll, rank, n, q, uid_ll128, uid_simple, uid_ring, barrier):
    try:
        import os

        import torch
        from oracle import oracle
        from tests.conftest import load_package
        nbx = load_package()
        lib = nbx.load_library()
        torch.cuda.set_device(0)
        uids = dict(zip(cases.PATHS, (uid_ll, uid_ll128, uid_simple, uid_ring)))
        os.environ.update(cases.PROCESS_ENV)
        comms, settings = {}, {}
        for name in cases.PATHS:   # each communicator under its own environment
            for k in cases.ENV_KEYS:
                os.environ.pop(k, None)
            os.environ.update(cases.COMM_ENV[name])
            comms[name] = nbx.Communicator.init_rank(n, nbx.ncclUniqueId.from_buffer_copy(uids[name]), rank)
            settings[name] = mp_diag.comm_settings(nbx, comms[name])
        st = torch.cuda.current_stream().cuda_stream
        out = {"settings": settings}
        for path in cases.PATHS:
            comm = comms[path]
            for kind in cases.KINDS:
                slots, send_bytes, recv_bytes = cases.layout(oracle, path, kind, n, rank)
                tx = torch.from_numpy(cases.send_image(oracle, path, kind, n, rank)).cuda()
                ty = torch.full((recv_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
                assert tx.numel() == send_bytes and tx.data_ptr() % 16 == 0 and ty.data_ptr() % 16 == 0
                torch.cuda.synchronize()
                nbx.launch_log_reset()
                nbx.group_start()
                for sl in slots:
                    sp = tx.data_ptr() + sl.send_off
                    rp = (tx.data_ptr() if sl.in_place else ty.data_ptr()) + sl.recv_off
                    if kind == "ar":
                        comm.all_reduce(sp, rp, sl.count, sl.dtype, sl.op, st)
                    else:
                        comm.reduce_scatter(sp, rp, sl.count, sl.dtype, sl.op, st)
                nbx.group_end()
                records = nbx.launch_log()
                torch.cuda.synchronize()
                err = comm.async_error()
                if err:
                    raise RuntimeError(f"{path} {kind}: asynchronous error {err}: "
                                       f"{(lib.ncclGetLastError(None) or b'').decode(errors='replace')}")
                out[(path, kind)] = (records, tx.cpu().numpy(), ty.cpu().numpy())
            if cases.is_simple(path):
                # every rank idle, then the state: the peers post into this rank's flag words
                barrier.wait(MEET_SEC)
                out[(path, "state")] = nbx.simple_state(comm, 4 * n * settings[path]["simpleGrid"])
                barrier.wait(MEET_SEC)
        for comm in comms.values():
            comm.destroy()
        q.put((rank, "ok", out))
    except Exception:
        import traceback
        try:
            barrier.abort()   # the peers fail at once instead of waiting out the meeting
        except Exception:
            pass
        q.put((rank, "error", traceback.format_exc()))


def _expected_images(oracle, path, kind, n):
    """Per rank: (send arena, recv arena, output mask of each) as the group must
    leave them, and the slots' expected outputs."""
    exps = {(pi, s): cases.expected(oracle, path, kind, pi, s, n)
            for pi in range(len(cases.TYPE_OPS)) for s in range(cases.N_SEGS)}
    images = []
    for r in range(n):
        slots, _, recv_bytes = cases.layout(oracle, path, kind, n, r)
        simg = cases.send_image(oracle, path, kind, n, r).copy()
        rimg = np.full(recv_bytes, 0xA5, dtype=np.uint8)
        smask, rmask = np.zeros(simg.size, dtype=bool), np.zeros(rimg.size, dtype=bool)
        for sl in slots:
            e = np.ascontiguousarray(exps[(sl.pair, sl.seg)][r]).view(np.uint8)
            img, mask = (simg, smask) if sl.in_place else (rimg, rmask)
            img[sl.recv_off:sl.recv_off + e.size] = e
            mask[sl.recv_off:sl.recv_off + e.size] = True
        images.append((simg, rimg, smask, rmask))
    return exps, images


def _nearest_slot(slots, arena_is_send, off):
    """The call whose buffer lies closest to byte `off` of an arena, for a report."""
    def dist(sl):
        if arena_is_send:
            lo, hi = sl.send_off, sl.send_off + sl.send_elts * sl.eb
        elif sl.in_place:
            return 1 << 60
        else:
            lo, hi = sl.recv_off, sl.recv_off + sl.count * sl.eb
        return 0 if lo <= off < hi else min(abs(off - lo), abs(off - hi + 1))
    sl = min(slots, key=dist)
    return f"pair {sl.pair} segment {sl.seg} ({dist(sl)} B away)"


def _where(path, kind, sl, n, rank, bad, settings):
    """Which part of the launch the wrong elements of one output belong to."""
    base = rank * sl.count if kind == "rs" else 0
    if cases.is_simple(path):
        s = settings[path]
        g = cases.launch_geometry(path, kind, sl.eb, n, s["simpleGrid"], s["sliceBytes"])
        loc = g.locate(sl.seg, bad + base)
        cells, counts = np.unique(loc[:, :4], axis=0, return_counts=True)
        top = cells[np.argsort(-counts, kind="stable")[:4]].tolist()
        return (f"{len(cells)} (segment, block, round, workgroup) cells, top {top}; first at {loc[0].tolist()} "
                f"last at {loc[-1].tolist()}; sliceOff {g.slice_off} slice {g.slice_elts} elts grid {g.grid}")
    offs, total = cases.launch_units(path, kind, sl.eb, n)
    unit = cases.UNIT[path]
    u = bad * sl.eb // unit
    return (f"segment {sl.seg} units {int(u[0])}..{int(u[-1])} of its own, launch units {offs[sl.seg] + int(u[0])}.."
            f"{offs[sl.seg] + int(u[-1])} of {total} ({unit}-byte units; packOff {offs})")


@pytest.mark.parametrize("n", cases.NS)
def test_group_segments(nbx, oracle, n, monkeypatch):
    """Per communicator and kind, one group of 64 calls. Launch record: exactly
    8 entries of the path's family, nSrcs == n, unroll 1 (LL family) or 0
    (Simple), flags 8 << 8 — and the same from mp_diag.group_runs. Outputs:
    mi.assert_same against cases.expected (blocks from each segment's own
    count; ring: ring_chain, float Sum included), NaN compared only as NaN and
    at most NAN_CAP of a launch's pooled results; every byte outside the
    outputs — 16 guard bytes either side of every buffer, padding, every send
    buffer but the in-place segment's output — as uploaded. Simple and ring:
    nbxDebugSimpleState at rest equals the grouped model's end state word for
    word (so grid, slice, rounds and sliceOff of the mirror are the library's),
    and flow.cases.check_pairs holds. A mismatch names its (segment, block,
    round, workgroup) cells, or its segment and units."""
    monkeypatch.setenv("NBX_BOOTSTRAP_TIMEOUT", "60")
    monkeypatch.setenv("NBX_TIMEOUT_SEC", "60")
    for k, v in cases.PROCESS_ENV.items():
        monkeypatch.setenv(k, v)
    for k in ("NBX_CHECK_PLANS", "NCCL_CHECK_POINTERS", "NBX_CHECK_SLICES", "NCCL_BUFFSIZE", "NBX_LL_MAX_BYTES",
              "NCCL_LL_BUFFSIZE", "NBX_LL128_MAX_BYTES", "NCCL_LL128_BUFFSIZE", "NBX_SIMPLE_SLOTS",
              "NBX_SIMPLE_PREFETCH", "NCCL_MAX_NCHANNELS", "NCCL_MIN_NCHANNELS"):
        monkeypatch.delenv(k, raising=False)
    t0 = time.perf_counter()
    barrier = mp.get_context("spawn").Barrier(n)

    def references():   # worked out on a host thread while the ranks run
        ref = {(path, kind): _expected_images(oracle, path, kind, n) for path in cases.PATHS for kind in cases.KINDS}
        widths = [cases.itemsize(oracle, dt) for dt, _ in cases.TYPE_OPS]
        with np.errstate(over="ignore"):
            models = {path: cases.run_model_groups(sm, n, path, widths=widths)[0] for path in ("simple", "ring")}
        return ref, models
    with ThreadPoolExecutor(1) as pool:
        working = pool.submit(references)
        res = _run_ranks(nbx, n, _child_segments, *(bytes(nbx.get_unique_id()) for _ in range(3)), barrier)
        ref, models = working.result()
    t_run = time.perf_counter() - t0

    settings = res[0]["settings"]
    for name in ("simple", "ring"):
        s = settings[name]
        assert (s["simpleGrid"], s["sliceBytes"], s["slots"]) == (cases.SIMPLE_GRID, cases.SIMPLE_SLICE,
                                                                  cases.SIMPLE_SLOTS), (name, s)
    for name in cases.PATHS:
        assert all(res[r]["settings"][name] == settings[name] for r in range(n))
        assert settings[name]["checkPlans"] == 0 and settings[name]["checkSlices"] == 0

    failures, checked, worst_nan = [], 0, 0.0
    # NBX_GROUP_BATCH is not among the communicators' keys: were it 0 in the environment, every output
    # below would still match and the launch records would not
    failures += [f"{name}: groupBatch is {settings[name]['groupBatch']}" for name in cases.PATHS
                 if settings[name]["groupBatch"] != 1]
    for path in cases.PATHS:
        oneshot = int(cases.COMM_ENV[path].get("NBX_LL128_ONESHOT_MAX", 256 << 10))
        want_rec = [(cases.FAMILY[path], n, 0 if cases.is_simple(path) else 1, 8 << nbx.LAUNCH_SEGS_SHIFT)] * 8
        for kind in cases.KINDS:
            exps, images = ref[(path, kind)]
            # NaN is compared only as NaN: its share of every launch's pooled results stays small
            for pi, (dt, _op) in enumerate(cases.TYPE_OPS):
                if dt in mi.FLOAT_TYPES:
                    pooled = np.concatenate([exps[(pi, s)][r] for s in range(cases.N_SEGS) for r in range(n)])
                    worst_nan = max(worst_nan, mi.nan_share(pooled, dt))
                    assert mi.nan_share(pooled, dt) <= mi.NAN_CAP, (path, kind, dt)
            for r in range(n):
                (total, recs), got_send, got_recv = res[r][(path, kind)]
                ctx = f"{path} {kind} rank {r} of {n}"
                slots, _, _ = cases.layout(oracle, path, kind, n, r)
                plan = mp_diag.group_runs(cases.group_calls(oracle, path, kind, n, r), n,
                                          dict(settings[path], groupBatch=1), cases.PROTO_MASK[path], path == "ring",
                                          oneshot)
                assert plan.records == want_rec, (ctx, plan.records)
                if total != 8 or [tuple(x) for x in recs] != want_rec:
                    failures.append(f"{ctx}: launch record {total} {recs}, expected 8 x {want_rec[0]}")
                simg, rimg, smask, rmask = images[r]
                for is_send, got, img, mask in ((True, got_send, simg, smask), (False, got_recv, rimg, rmask)):
                    assert got.size == img.size
                    bad = np.flatnonzero((got != img) & ~mask)
                    if bad.size:
                        failures.append(f"{ctx}: {bad.size} bytes outside the outputs of the "
                                        f"{'send' if is_send else 'recv'} arena changed, first at {int(bad[0])} near "
                                        f"{_nearest_slot(slots, is_send, int(bad[0]))}: "
                                        f"{bytes(got[bad[:16]]).hex()} (runs {mp_diag._runs(bad)})")
                for sl in slots:
                    e = np.ascontiguousarray(exps[(sl.pair, sl.seg)][r])
                    arena = got_send if sl.in_place else got_recv
                    got = arena[sl.recv_off:sl.recv_off + e.nbytes].copy().view(e.dtype)
                    checked += 1
                    if np.array_equal(got.view(np.uint8), e.view(np.uint8)):
                        continue   # equal bytes: mi.assert_same's rule holds
                    try:
                        mi.assert_same(got, e, sl.dtype)
                    except AssertionError as err:
                        d = mp_diag.describe_mismatch(got, e)
                        gu, eu = got.view(np.uint8).reshape(e.size, -1), e.view(np.uint8).reshape(e.size, -1)
                        bad = np.flatnonzero((gu != eu).any(axis=1))
                        failures.append(f"{ctx} pair {sl.pair} ({oracle.TYPE_NAMES[sl.dtype]} op {sl.op}) segment "
                                        f"{sl.seg} ({sl.count} elements{', in place' if sl.in_place else ''}): {err}\n"
                                        f"    all differing bytes (NaN payloads included): "
                                        f"{mp_diag.format_mismatch(d)}; {_where(path, kind, sl, n, r, bad, settings)}")
        if cases.is_simple(path):
            states = [res[r][(path, "state")] for r in range(n)]
            assert all(s is not None and len(s[0]) == len(s[1]) == 4 * n * cases.SIMPLE_GRID for s in states)
            states = [s[:2] for s in states]
            failures += [f"{path} state vs the grouped model: {x}"
                         for x in flow.check_model(states, models[path], n, cases.SIMPLE_GRID)]
            failures += [f"{path} at rest: {x}" for x in flow.check_pairs(states, n, cases.SIMPLE_GRID)]
    assert checked == len(cases.PATHS) * len(cases.KINDS) * 64 * n
    print(f"group segments at {n} ranks: {checked} outputs, largest pooled NaN share {worst_nan:.2%}, "
          f"{len(failures)} failure(s); ranks ran {t_run:.1f} s, test {time.perf_counter() - t0:.1f} s", file=sys.stderr)
    if failures:
        head = f"{len(failures)} failure(s) in {checked} outputs at {n} ranks"
        raise AssertionError(head + ":\n" + "\n".join(failures[:10]) + "\n" +
                             mp_diag.emit_summary([head] + [f.splitlines()[0][:160] for f in failures[:4]]))


# ---------------------------------------------------------------------------
# the cut rules

def _child_cut(uid, rank, n, q, uid_off):
    try:
        import os

        import torch
        from tests.conftest import load_package
        nbx = load_package()
        lib = nbx.load_library()
        torch.cuda.set_device(0)
        comm = nbx.Communicator.init_rank(n, nbx.ncclUniqueId.from_buffer_copy(uid), rank)
        os.environ["NBX_GROUP_BATCH"] = "0"
        comm_off = nbx.Communicator.init_rank(n, nbx.ncclUniqueId.from_buffer_copy(uid_off), rank)
        os.environ.pop("NBX_GROUP_BATCH")
        settings = mp_diag.comm_settings(nbx, comm)
        out = {"settings": settings, "settings_off": mp_diag.comm_settings(nbx, comm_off)}
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        groups = cases.cut_groups(n, settings)
        scalar = np.array([cases.PREMUL_INTS[rank]], dtype=np.int32)

        def run(which, gi, name, calls):
            lay, size = cases.buffer_layout(calls, n)
            t = torch.from_numpy(cases.arena_image(gi, calls, n, rank)).cuda()
            assert t.numel() == size
            premul = which.redop_create_premulsum(scalar.ctypes.data, cases.INT32) if any(c.premul for c in calls) else None
            torch.cuda.synchronize()
            nbx.launch_log_reset()
            nbx.group_start()
            for c in calls:
                s = streams[c.stream].cuda_stream
                sp = t.data_ptr() + lay[c.send[0]][0] + 4 * c.send[1]
                rp = t.data_ptr() + lay[c.recv[0]][0] + 4 * c.recv[1]
                assert sp + 4 * c.count * (n if c.kind == "rs" else 1) <= t.data_ptr() + size
                assert rp + 4 * c.count <= t.data_ptr() + size
                op = premul if c.premul else c.op
                if c.kind == "ar":
                    which.all_reduce(sp, rp, c.count, c.dtype, op, s)
                elif c.kind == "rs":
                    which.reduce_scatter(sp, rp, c.count, c.dtype, op, s)
                else:
                    which.reduce(sp, 0 if (c.null_recv and rank != c.root) else rp, c.count, c.dtype, op, c.root, s)
            nbx.group_end()
            records = nbx.launch_log()
            later = None
            if any(c.stream for c in calls):   # later work on the other stream sees the results
                with torch.cuda.stream(streams[1]):
                    later = t.clone()
            torch.cuda.synchronize()
            if premul is not None:
                which.redop_destroy(premul)
            err = which.async_error()
            if err:
                raise RuntimeError(f"{name}: asynchronous error {err}: "
                                   f"{(lib.ncclGetLastError(None) or b'').decode(errors='replace')}")
            return records, t.cpu().numpy(), None if later is None else later.cpu().numpy()

        for gi, (name, calls) in enumerate(groups.items()):
            out[name] = run(comm, gi, name, calls)
        gi = list(groups).index(cases.BATCH_OFF_GROUP)
        out["batch_off"] = run(comm_off, gi, "batch_off", groups[cases.BATCH_OFF_GROUP])
        comm_off.destroy()
        comm.destroy()
        q.put((rank, "ok", out))
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc()))


@pytest.mark.parametrize("n", cases.CUT_NS)
def test_group_cut_rules(nbx, n, monkeypatch):
    """One group per cut rule of runMpGroup (tests/groups/cases.py cut_groups)
    on a default communicator: all protocols, default thresholds, batching on.
    After every ncclGroupEnd the launch record (its collective families; a user
    PreMulSum's pre-pass is a reduce launch of its own) equals
    mp_diag.group_runs' answer on that rank — computed from the communicator's
    own settings, cut for the reason the rule is there for — and every byte of
    the group's arena equals the calls folded in call order on the host
    (int32 sums wrap, the f32 values are small whole numbers: exact in any
    order). Two streams inside one run: one launch, and a copy enqueued on the
    second stream after the group holds the results. A second communicator
    created under NBX_GROUP_BATCH=0 runs the 17-call group as 17 launches with
    segment count 0."""
    monkeypatch.setenv("NBX_BOOTSTRAP_TIMEOUT", "60")
    monkeypatch.setenv("NBX_TIMEOUT_SEC", "60")
    for k in cases.ENV_KEYS + ("NBX_GROUP_BATCH", "NBX_CHECK_PLANS", "NCCL_CHECK_POINTERS", "NBX_CHECK_SLICES", "NCCL_BUFFSIZE",
                               "NBX_LL_MAX_BYTES", "NCCL_LL_BUFFSIZE", "NBX_LL128_MAX_BYTES", "NCCL_LL128_BUFFSIZE",
                               "NBX_LL128_MAX_GRID", "NBX_LL_MAX_GRID", "NCCL_MAX_NCHANNELS", "NCCL_MIN_NCHANNELS"):
        monkeypatch.delenv(k, raising=False)
    t0 = time.perf_counter()
    res = _run_ranks(nbx, n, _child_cut, bytes(nbx.get_unique_id()))
    t_run = time.perf_counter() - t0
    settings = res[0]["settings"]
    assert all(res[r]["settings"] == settings for r in range(n)) and settings["groupBatch"] == 1
    assert all(res[r]["settings_off"]["groupBatch"] == 0 for r in range(n))
    groups = cases.cut_groups(n, settings)
    defaults = all(settings[k] == v for k, v in cases.DEFAULT_SETTINGS.items())
    failures, seen = [], set()
    for gi, (name, calls) in enumerate(list(groups.items()) + [("batch_off", groups[cases.BATCH_OFF_GROUP])]):
        off = name == "batch_off"
        gidx = list(groups).index(cases.BATCH_OFF_GROUP) if off else gi
        want_arenas = cases.simulate(gidx, calls, n)
        for r in range(n):
            (total, recs), arena, later = res[r][name]
            plan = mp_diag.group_runs(cases.cut_group_calls(calls, n, r), n, dict(settings, groupBatch=0 if off else 1))
            if r == 0:
                seen |= set(plan.reasons)
                if not off and name in cases.CUT_REASON and not (name == "ll128_two_shot" and n == 2):
                    assert cases.CUT_REASON[name] in plan.reasons, (name, plan.reasons)   # two ranks have no two-shot
                if not off and defaults and n == 3 and name in cases.CUT_EXPECT_3:
                    assert [x[3] >> 8 for x in plan.records] == cases.CUT_EXPECT_3[name], (name, plan.records)
                if off:
                    assert plan.records == [(cases.FAM_LL, n, 1, 0)] * len(calls)
            assert total <= nbx.LAUNCH_LOG_CAP
            coll = [tuple(x) for x in recs if x[0] in COLLECTIVE_FAMILIES]
            if not any(c.premul for c in calls):   # a user PreMulSum's pre-pass may leave a reduce record of its own
                assert len(coll) == len(recs) == total, (name, recs)
            if coll != plan.records:
                failures.append(f"{name} rank {r} of {n}: launch record {coll}, expected {plan.records} "
                                f"(runs {plan.runs}, cut for {plan.reasons})")
            for what, got in (("arena", arena), ("copy on the second stream", later)):
                if got is None:
                    continue
                try:
                    mp_diag.check_equal(got, want_arenas[r], f"{name} rank {r} of {n} {what}")
                except AssertionError as err:
                    lay, _ = cases.buffer_layout(calls, n)
                    bad = np.flatnonzero(got != want_arenas[r])
                    names = sorted({nm for nm, (o, ne, _) in lay.items() if ((bad >= o) & (bad < o + 4 * ne)).any()})
                    failures.append(f"{str(err).splitlines()[0]}; buffers touched: {names or 'none (guard bytes)'}")
    assert seen == set(mp_diag.CUT_REASONS), seen
    assert sum(1 for c in groups["two_streams"] if c.stream) == 2 and res[0]["two_streams"][2] is not None
    print(f"group cut rules at {n} ranks: {len(groups) + 1} groups, {len(failures)} failure(s); ranks ran {t_run:.1f} s, "
          f"test {time.perf_counter() - t0:.1f} s", file=sys.stderr)
    if failures:
        head = f"{len(failures)} failure(s) in {len(groups) + 1} groups at {n} ranks"
        raise AssertionError(head + ":\n" + "\n".join(failures[:10]) + "\n" +
                             mp_diag.emit_summary([head] + [f[:160] for f in failures[:4]]))
