"""Wide (fp32-accumulating) sums through every direct-schedule collective kernel
of a multi-process communicator: an operator of nbxRedOpCreateWide on
ncclAllReduce / ncclReduceScatter / ncclReduce, bit for bit against
nbxReduceMultiWide's arithmetic folded in the schedule's own operand order
(tests/widecoll/cases.py; NaN compared only as NaN), with the launch record
saying which kernel and which instantiation each call took.

One spawn of n ranks per n for the case table, as tests/edges/; one spawn of 3
ranks for the checking instantiations, groups and NBX_WIDE_ACCUM; one of 2
ranks for graph capture.

The file carries the name of tests/test_multiprocess_gpu.py on purpose: the
GPU suite orders files by name (tests/conftest.py GPU_FILE_ORDER)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import mp_diag
from tests.matrix import inputs as mi
from tests.test_multiprocess_gpu import _run_ranks
from tests.widecoll import cases

pytestmark = pytest.mark.gpu

GUARD = 16   # bytes of 0xA5 either side of every output
BF16, F32, I32 = 9, 7, 2
ENV_CLEAR = ("NBX_CHECK_PLANS", "NCCL_CHECK_POINTERS", "NBX_CHECK_SLICES", "NBX_SIMPLE_SLICE_BYTES", "NCCL_BUFFSIZE",
             "NBX_LL_MAX_BYTES", "NCCL_LL_BUFFSIZE", "NBX_LL128_MAX_BYTES", "NCCL_LL128_BUFFSIZE", "NBX_WIDE_ACCUM",
             "NCCL_PROTO", "NCCL_ALGO", "NBX_SIMPLE_MAX_GRID", "NBX_GROUP_BATCH")


def _env(monkeypatch):
    monkeypatch.setenv("NBX_BOOTSTRAP_TIMEOUT", "60")
    monkeypatch.setenv("NBX_TIMEOUT_SEC", "60")
    for k, v in cases.PROCESS_ENV.items():
        monkeypatch.setenv(k, v)
    for k in ENV_CLEAR:
        monkeypatch.delenv(k, raising=False)


def _child_cases(uid_ll, rank, n, q, uid_ll128, uid_simple, uid_ring):
    try:
        import os

        import torch
        from oracle import oracle
        from tests.conftest import load_package
        nbx = load_package()
        lib = nbx.load_library()
        torch.cuda.set_device(0)
        uids = dict(zip(cases.COMMS, (uid_ll, uid_ll128, uid_simple, uid_ring)))
        os.environ.update(cases.PROCESS_ENV)
        comms, settings, ops = {}, {}, {}
        for name in cases.COMMS:   # each communicator under its own environment
            for k in cases.ENV_KEYS:
                os.environ.pop(k, None)
            os.environ.update(cases.COMM_ENV[name])
            comms[name] = nbx.Communicator.init_rank(n, nbx.ncclUniqueId.from_buffer_copy(uids[name]), rank)
            settings[name] = mp_diag.comm_settings(nbx, comms[name])
            ops[name] = {(dt, op): comms[name].redop_create_wide(op, dt) for dt in cases.TYPES for op in cases.OPS}
        st = torch.cuda.current_stream().cuda_stream
        out = {"settings": settings}
        uploads = {}
        for path in cases.PATHS:
            comm = comms[cases.PATH_COMM[path]]
            for i, (kind, dt, op) in enumerate(cases.path_cases(path)):
                count = cases.count_of(oracle, path, dt)
                shift = cases.shift_of(oracle, path, dt)
                key = (cases.input_kind(path, kind, dt, op), dt, cases.nbytes_of(oracle, path, dt), kind == "rs", shift)
                if key not in uploads:
                    x = np.ascontiguousarray(cases.rank_inputs(oracle, path, kind, dt, op, n)[rank]).view(np.uint8)
                    host = np.full(GUARD + shift + x.size + GUARD, 0xA5, dtype=np.uint8)
                    host[GUARD + shift:GUARD + shift + x.size] = x
                    uploads[key] = torch.from_numpy(host).cuda()
                tx = uploads[key]
                nb = count * cases.itemsize(oracle, dt)
                ty = torch.full((GUARD + shift + nb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
                assert tx.data_ptr() % 16 == 0 and ty.data_ptr() % 16 == 0
                sp, rp = tx.data_ptr() + GUARD + shift, ty.data_ptr() + GUARD + shift
                root = cases.root_of(i, n)
                handle = ops[cases.PATH_COMM[path]][(dt, op)]
                torch.cuda.synchronize()
                nbx.launch_log_reset()
                if kind == "ar":
                    comm.all_reduce(sp, rp, count, dt, handle, st)
                elif kind == "rs":
                    comm.reduce_scatter(sp, rp, count, dt, handle, st)
                else:
                    comm.reduce(sp, rp if rank == root else 0, count, dt, handle, root, st)
                total, recs = nbx.launch_log()
                torch.cuda.synchronize()
                assert total == len(recs)
                out[(path, i)] = (ty.cpu().numpy() if kind != "red" or rank == root else None, recs)
            err = comm.async_error()
            assert err == 0, (path, err, (lib.ncclGetLastError(None) or b"").decode(errors="replace"))
        for name, comm in comms.items():
            for h in ops[name].values():
                comm.redop_destroy(h)
            comm.destroy()
        q.put((rank, "ok", out))
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc()))


@pytest.mark.parametrize("n", cases.NS)
def test_wide_collective_cases(nbx, oracle, n, monkeypatch):
    """Every case of tests/widecoll/cases.py: outputs on every rank (a Reduce: its root)
    mi.assert_same against cases.expected, 16 guard bytes of 0xA5 either side untouched, and
    exactly one launch record per call: the path's family (ring_direct: 11, not 12), nSrcs == n,
    the host's unroll field, flags == 2 (bit 1 the fp32-accumulating instantiation, bit 0 clear)."""
    _env(monkeypatch)

    def fold_all():
        return {(path, i): cases.expected(oracle, path, kind, dt, op, n, cases.root_of(i, n))
                for path in cases.PATHS for i, (kind, dt, op) in enumerate(cases.path_cases(path))}
    with ThreadPoolExecutor(1) as pool:
        folding = pool.submit(fold_all)
        res = _run_ranks(nbx, n, _child_cases, *(bytes(nbx.get_unique_id()) for _ in range(3)))
        expected = folding.result()

    settings = res[0]["settings"]
    for name in ("simple", "ring"):
        assert settings[name]["simpleGrid"] == 2 and settings[name]["sliceBytes"] == 64 << 10
    failures, checked = [], 0
    for path in cases.PATHS:
        for i, (kind, dt, op) in enumerate(cases.path_cases(path)):
            root = cases.root_of(i, n)
            exp = expected[(path, i)]
            stt = oracle.NP_STORAGE[dt]
            shift = cases.shift_of(oracle, path, dt)
            want_rec = [(cases.family_of(path, kind, n), n, cases.host_unroll(path), cases.FLAG_WIDE)]
            for r in range(n):
                buf, recs = res[r][(path, i)]
                ctx = f"{path} {kind} {oracle.TYPE_NAMES[dt]} wide op {op} root {root} rank {r} of {n}"
                if [tuple(x) for x in recs] != want_rec:
                    failures.append(f"{ctx}: launch record {recs}, expected {want_rec}")
                if r not in exp:
                    assert buf is None and kind == "red"
                    continue
                e = np.ascontiguousarray(exp[r])
                lo = GUARD + shift
                assert buf.size == lo + e.nbytes + GUARD
                if not ((buf[:lo] == 0xA5).all() and (buf[lo + e.nbytes:] == 0xA5).all()):
                    failures.append(f"{ctx}: guard bytes overwritten")
                got = buf[lo:lo + e.nbytes].copy().view(stt)
                checked += 1
                if np.array_equal(got.view(np.uint8), e.view(np.uint8)):
                    continue
                try:
                    mi.assert_same(got, e, dt)
                except AssertionError as err:
                    failures.append(f"{ctx} ({cases.input_kind(path, kind, dt, op)} inputs): {err}")
    assert checked == sum(n if k != "red" else 1 for p in cases.PATHS for k, _, _ in cases.path_cases(p))
    assert not failures, f"{len(failures)} failure(s) in {checked} outputs at {n} ranks:\n" + "\n".join(failures[:8])


# ---------------------------------------------------------------------------
# checking instantiations, groups, NBX_WIDE_ACCUM: one spawn of 3 ranks

LL_COUNT, SIMPLE_COUNT = 4001, 150011      # bf16 elements: 8,002 B (LL) and 300,022 B (Simple)
EXTRA_COMMS = ("plain", "slices", "plans", "accum")
EXTRA_ENV = {"plain": {}, "slices": {"NBX_CHECK_SLICES": "1"}, "plans": {"NBX_CHECK_PLANS": "1"},
             "accum": {"NBX_WIDE_ACCUM": "1"}}
EXTRA_KEYS = ("NBX_CHECK_SLICES", "NBX_CHECK_PLANS", "NBX_WIDE_ACCUM")


def _extra_input(oracle, dt, count, rank):
    from tests.wide.test_reduce_gpu import many_inputs
    if dt == BF16:
        return np.ascontiguousarray(many_inputs(oracle, BF16, 3, count, 4242)[rank])
    return np.ascontiguousarray(oracle.random_inputs(dt, 3, count, seed=4242)[rank])


def _child_extras(uid0, rank, n, q, uid1, uid2, uid3):
    try:
        import ctypes
        import os

        import torch
        from oracle import oracle
        from tests.conftest import load_package
        nbx = load_package()
        lib = nbx.load_library()
        torch.cuda.set_device(0)
        os.environ.update(cases.PROCESS_ENV)
        os.environ["NCCL_PROTO"] = "LL,Simple"
        comms = {}
        out = {}
        for name, uid in zip(EXTRA_COMMS, (uid0, uid1, uid2, uid3)):
            for k in EXTRA_KEYS:
                os.environ.pop(k, None)
            os.environ.update(EXTRA_ENV[name])
            comms[name] = nbx.Communicator.init_rank(n, nbx.ncclUniqueId.from_buffer_copy(uid), rank)
            vals = (ctypes.c_int64 * 12)()
            got = lib.nbxDebugCommSettings(comms[name].handle, vals, 12)
            out[("settings", name)] = (got, list(vals))
        st = torch.cuda.current_stream().cuda_stream
        keep = []

        def dev(x):
            t = torch.from_numpy(x.view(np.uint8).copy()).cuda()
            keep.append(t)
            return t

        def run(comm, dt, count, op, tx):
            ty = torch.zeros(tx.numel(), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            nbx.launch_log_reset()
            comm.all_reduce(tx.data_ptr(), ty.data_ptr(), count, dt, op, st)
            _, recs = nbx.launch_log()
            torch.cuda.synchronize()
            return ty.cpu().numpy(), recs

        x_ll, x_simple = dev(_extra_input(oracle, BF16, LL_COUNT, rank)), dev(_extra_input(oracle, BF16, SIMPLE_COUNT, rank))
        # the checking instantiations: one wide AllReduce each (Simple size / LL size)
        for name, tx, count in (("slices", x_simple, SIMPLE_COUNT), ("plans", x_ll, LL_COUNT), ("plans", x_simple, SIMPLE_COUNT)):
            h = comms[name].redop_create_wide(0, BF16)
            out[("check", name, count)] = run(comms[name], BF16, count, h, tx)
            comms[name].redop_destroy(h)
        # a group of four wide AllReduces (two LL sizes, two Simple sizes), then wide and per-step alternating
        plain = comms["plain"]
        h = plain.redop_create_wide(0, BF16)
        outs = [torch.zeros(x.numel(), dtype=torch.uint8, device="cuda") for x in (x_ll, x_ll, x_simple, x_simple)]
        torch.cuda.synchronize()
        nbx.launch_log_reset()
        lib.ncclGroupStart()
        for x, y, c in zip((x_ll, x_ll, x_simple, x_simple), outs, (LL_COUNT, LL_COUNT, SIMPLE_COUNT, SIMPLE_COUNT)):
            plain.all_reduce(x.data_ptr(), y.data_ptr(), c, BF16, h, st)
        assert lib.ncclGroupEnd() == 0
        _, recs = nbx.launch_log()
        torch.cuda.synchronize()
        out["group"] = ([y.cpu().numpy() for y in outs], recs)
        outs = [torch.zeros(x_ll.numel(), dtype=torch.uint8, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        nbx.launch_log_reset()
        lib.ncclGroupStart()
        for k, y in enumerate(outs):
            plain.all_reduce(x_ll.data_ptr(), y.data_ptr(), LL_COUNT, BF16, h if k % 2 == 0 else 0, st)
        assert lib.ncclGroupEnd() == 0
        _, recs = nbx.launch_log()
        torch.cuda.synchronize()
        out["alternating"] = ([y.cpu().numpy() for y in outs], recs)
        plain.redop_destroy(h)
        # NBX_WIDE_ACCUM=1: plain ncclSum / ncclAvg; and the communicator without it
        for dt, count in ((BF16, LL_COUNT), (F32, 2003), (I32, 2003)):
            tx = dev(_extra_input(oracle, dt, count, rank))
            for op in (0, 4):
                out[("accum", dt, op)] = run(comms["accum"], dt, count, op, tx)
                if dt == BF16:
                    out[("plain", dt, op)] = run(plain, dt, count, op, tx)
        for name, comm in comms.items():
            err = comm.async_error()
            assert err == 0, (name, err, (lib.ncclGetLastError(None) or b"").decode(errors="replace"))
            comm.destroy()
        q.put((rank, "ok", out))
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc()))


@pytest.fixture(scope="module")
def extras(nbx):
    import os
    saved = {k: os.environ.get(k) for k in ENV_CLEAR + tuple(cases.PROCESS_ENV) + ("NBX_BOOTSTRAP_TIMEOUT", "NBX_TIMEOUT_SEC")}
    try:
        for k in ENV_CLEAR:
            os.environ.pop(k, None)
        os.environ.update(cases.PROCESS_ENV)
        os.environ.update({"NBX_BOOTSTRAP_TIMEOUT": "60", "NBX_TIMEOUT_SEC": "60"})
        return _run_ranks(nbx, 3, _child_extras, *(bytes(nbx.get_unique_id()) for _ in range(3)))
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _allreduce_expected(oracle, fold, dt, op, count, n=3):
    xs = [_extra_input(oracle, dt, count, r) for r in range(n)]
    return cases.expected_with(fold, oracle, xs, "ar", dt, op, n, 0, count)[0]


def _same(oracle, got_u8, exp, dt):
    mi.assert_same(got_u8.view(oracle.NP_STORAGE[dt]), exp, dt)


def test_checking_instantiations(oracle, extras):
    """NBX_CHECK_SLICES=1 and NBX_CHECK_PLANS=1 communicators, one wide AllReduce each at 3
    ranks: flags bits 0 and 1 set where the protocol has a checking kernel (slices: Simple;
    plans: the LL family), equal outputs, no async error (the child asserts it)."""
    want = {LL_COUNT: _allreduce_expected(oracle, cases.wide_fold_of, BF16, 0, LL_COUNT),
            SIMPLE_COUNT: _allreduce_expected(oracle, cases.wide_fold_of, BF16, 0, SIMPLE_COUNT)}
    for r in range(3):
        got, recs = extras[r][("check", "slices", SIMPLE_COUNT)]
        assert [tuple(x) for x in recs] == [(11, 3, 0, 3)]
        _same(oracle, got, want[SIMPLE_COUNT], BF16)
        got, recs = extras[r][("check", "plans", LL_COUNT)]
        assert [tuple(x) for x in recs] == [(8, 3, 1, 3)]
        _same(oracle, got, want[LL_COUNT], BF16)
        # plan headers of the Simple kernel are a run-time switch of the plain instantiation
        got, recs = extras[r][("check", "plans", SIMPLE_COUNT)]
        assert [tuple(x) for x in recs] == [(11, 3, 0, 2)]
        _same(oracle, got, want[SIMPLE_COUNT], BF16)


def test_groups(oracle, extras):
    """Four wide AllReduces in a group: one launch per run (LL, then Simple) with the segment
    count in the flags. Wide and per-step calls of one type alternating: cut apart, four launches."""
    wide = {c: _allreduce_expected(oracle, cases.wide_fold_of, BF16, 0, c) for c in (LL_COUNT, SIMPLE_COUNT)}
    step = _allreduce_expected(oracle, cases.per_step_fold_of, BF16, 0, LL_COUNT)
    assert (wide[LL_COUNT] != step).any()
    for r in range(3):
        outs, recs = extras[r]["group"]
        assert [tuple(x) for x in recs] == [(8, 3, 1, 2 | (2 << 8)), (11, 3, 0, 2 | (2 << 8))]
        for y, c in zip(outs, (LL_COUNT, LL_COUNT, SIMPLE_COUNT, SIMPLE_COUNT)):
            _same(oracle, y, wide[c], BF16)
        outs, recs = extras[r]["alternating"]
        assert [tuple(x) for x in recs] == [(8, 3, 1, 2), (8, 3, 1, 0), (8, 3, 1, 2), (8, 3, 1, 0)]
        for k, y in enumerate(outs):
            _same(oracle, y, wide[LL_COUNT] if k % 2 == 0 else step, BF16)


def test_wide_accum_env(oracle, extras):
    """NBX_WIDE_ACCUM=1 at creation: built-in ncclSum / ncclAvg on bf16 give the wide bits and
    the flag; on fp32 and int32 the per-step record with flags 0. nbxDebugCommSettings[11]
    reports it. A communicator without it gives today's bits for bf16."""
    for r in range(3):
        got, vals = extras[r][("settings", "accum")]
        assert got == 12 and vals[11] == 1
        got, vals = extras[r][("settings", "plain")]
        assert got == 12 and vals[11] == 0
        for op in (0, 4):
            y, recs = extras[r][("accum", BF16, op)]
            assert [tuple(x) for x in recs] == [(8, 3, 1, 2)]
            _same(oracle, y, _allreduce_expected(oracle, cases.wide_fold_of, BF16, op, LL_COUNT), BF16)
            for dt in (F32, I32):
                y, recs = extras[r][("accum", dt, op)]
                assert [tuple(x) for x in recs] == [(8, 3, 1, 0)]
                _same(oracle, y, _allreduce_expected(oracle, cases.per_step_fold_of, dt, op, 2003), dt)


def test_without_wide_accum_bf16_is_per_step(oracle, extras):
    """Unset, nothing changes: plain ncclSum / ncclAvg on bf16 are the per-step bits and record."""
    for r in range(3):
        for op in (0, 4):
            y, recs = extras[r][("plain", BF16, op)]
            assert [tuple(x) for x in recs] == [(8, 3, 1, 0)]
            _same(oracle, y, _allreduce_expected(oracle, cases.per_step_fold_of, BF16, op, LL_COUNT), BF16)


# ---------------------------------------------------------------------------
# graph capture

def _child_graph(uid, rank, n, q):
    try:
        import os

        import torch
        from oracle import oracle
        from tests.conftest import load_package
        nbx = load_package()
        torch.cuda.set_device(0)
        os.environ["NCCL_PROTO"] = "Simple"
        comm = nbx.Communicator.init_rank(n, nbx.ncclUniqueId.from_buffer_copy(uid), rank)
        h = comm.redop_create_wide(4, BF16)
        xs = [torch.from_numpy(_extra_input(oracle, BF16, SIMPLE_COUNT, (rank + k) % 3).view(np.uint8).copy()).cuda()
              for k in range(2)]
        tx = torch.empty_like(xs[0])
        ty = torch.zeros_like(tx)
        s = torch.cuda.Stream()
        outs = []
        with torch.cuda.stream(s):
            tx.copy_(xs[0])
            comm.all_reduce(tx.data_ptr(), ty.data_ptr(), SIMPLE_COUNT, BF16, h, s.cuda_stream)   # eager first
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                comm.all_reduce(tx.data_ptr(), ty.data_ptr(), SIMPLE_COUNT, BF16, h, s.cuda_stream)
            for k in range(2):
                tx.copy_(xs[k])
                ty.zero_()
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                outs.append(ty.cpu().numpy())
        assert comm.async_error() == 0
        comm.redop_destroy(h)
        comm.destroy()
        q.put((rank, "ok", outs))
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc()))


def test_graph_capture(nbx, oracle, monkeypatch):
    """One wide Simple AllReduce (wide Avg, bf16) captured at 2 ranks and replayed twice with
    different inputs: the operator's state was copied at enqueue, the sequencing is on the device."""
    _env(monkeypatch)
    res = _run_ranks(nbx, 2, _child_graph)
    for k in range(2):
        xs = [_extra_input(oracle, BF16, SIMPLE_COUNT, (r + k) % 3) for r in range(2)]
        exp = cases.expected_with(cases.wide_fold_of, oracle, xs, "ar", BF16, 4, 2, 0, SIMPLE_COUNT)[0]
        for r in range(2):
            _same(oracle, res[r][k], exp, BF16)
