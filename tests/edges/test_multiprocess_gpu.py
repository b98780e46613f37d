"""Every (type, op) through every collective kernel's own fold loop — kLLColl,
kLL128Coll, kLL128AllReduce2, kSimpleColl (pack and element paths, at the
unroll of 2, 3 and 5 ranks) and kSimpleRing — with edge-rich inputs (random
bit patterns, denormals, +-0, inf, NaN), bit for bit against the oracle in each
schedule's own operand order (NaN compared only as NaN), and with the
library's launch record saying which kernel each call took.

tests/edges/cases.py holds the case table, the sizes and why they are what
they are; tests/test_collective_edges_cpu.py checks the table without a GPU.
One spawn of n ranks per n: every rank creates the four communicators (LL,
LL128, Simple direct, Simple ring — they coexist in one process), runs the
756 cases one at a time with a synchronisation after each, and returns every
output with its guard bytes and the launch-record entries the call produced.

The file carries the name of tests/test_multiprocess_gpu.py on purpose: the
GPU suite orders files by name (tests/conftest.py GPU_FILE_ORDER)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import mp_diag
from tests.edges import cases
from tests.matrix import inputs as mi
from tests.test_multiprocess_gpu import _run_ranks

pytestmark = pytest.mark.gpu

GUARD = 16   # bytes of 0xA5 either side of every output


def _child_edges(uid_ll, rank, n, q, uid_ll128, uid_simple, uid_ring):
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
        comms, settings = {}, {}
        for name in cases.COMMS:   # each communicator under its own environment
            for k in cases.ENV_KEYS:
                os.environ.pop(k, None)
            os.environ.update(cases.COMM_ENV[name])
            comms[name] = nbx.Communicator.init_rank(n, nbx.ncclUniqueId.from_buffer_copy(uids[name]), rank)
            settings[name] = mp_diag.comm_settings(nbx, comms[name])
        st = torch.cuda.current_stream().cuda_stream
        out = {"settings": settings}
        uploads = {}   # one upload per (input, placement): the ops of a type share it
        for path in cases.PATHS:
            comm = comms[cases.PATH_COMM[path]]
            for i, (kind, dt, op) in enumerate(cases.path_cases(path)):
                count = cases.count_of(oracle, path, dt)
                shift = cases.shift_of(oracle, path, dt)
                key = (dt, cases.nbytes_of(oracle, path, dt), kind == "rs", shift)
                if key not in uploads:
                    x = np.ascontiguousarray(cases.rank_input(oracle, path, kind, dt, n, rank)).view(np.uint8)
                    host = np.full(GUARD + shift + x.size + GUARD, 0xA5, dtype=np.uint8)
                    host[GUARD + shift:GUARD + shift + x.size] = x
                    uploads[key] = torch.from_numpy(host).cuda()
                tx = uploads[key]
                nb = count * cases.itemsize(oracle, dt)
                ty = torch.full((GUARD + shift + nb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
                assert tx.data_ptr() % 16 == 0 and ty.data_ptr() % 16 == 0
                sp, rp = tx.data_ptr() + GUARD + shift, ty.data_ptr() + GUARD + shift
                root = cases.root_of(i, n)
                torch.cuda.synchronize()
                nbx.launch_log_reset()
                if kind == "ar":
                    comm.all_reduce(sp, rp, count, dt, op, st)
                elif kind == "rs":
                    comm.reduce_scatter(sp, rp, count, dt, op, st)
                else:
                    comm.reduce(sp, rp if rank == root else 0, count, dt, op, root, st)
                total, recs = nbx.launch_log()
                torch.cuda.synchronize()
                assert total == len(recs)
                out[(path, i)] = (ty.cpu().numpy() if kind != "red" or rank == root else None, recs)
            err = comm.async_error()
            assert err == 0, (path, err, (lib.ncclGetLastError(None) or b"").decode(errors="replace"))
        for comm in comms.values():
            comm.destroy()
        q.put((rank, "ok", out))
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc()))


def _geometry(oracle, path, kind, dt, n, settings):
    """The Simple cut of a case, for the description of a mismatch."""
    if cases.PATH_COMM[path] not in ("simple", "ring"):
        return None
    s = settings[cases.PATH_COMM[path]]
    return mp_diag.simple_geometry(kind, cases.count_of(oracle, path, dt), cases.itemsize(oracle, dt), n,
                                   s["simpleGrid"], s["sliceBytes"], ring=path == "ring")


@pytest.mark.parametrize("n", cases.NS)
def test_collective_edges(nbx, oracle, n, monkeypatch):
    """Outputs: mi.assert_same against cases.expected (direct: left fold b+1,
    ..., b per block; ring: ring_chain), 16 guard bytes of 0xA5 either side
    untouched. Launch record: exactly one entry per call — the family the path
    means, nSrcs == n, the host's unroll field (1 for LL / LL128, 0 for Simple),
    flags 0 (no checking instantiation, no group).

    The unroll a Simple case runs is picked on the device (simpleFold, from the
    sources of each fold): the direct schedule folds the n sources of a block
    in one call, so 16 packs per lane at 2 ranks, 8 at 3, 4 at 5; a ring hop
    folds the local input with one received slice, so 16 at any n
    (cases.fold_unroll). The host cannot record it; what is asserted here is
    what decides it — family and nSrcs — and that under the communicator's own
    settings the call's slices are as long as cases.py's arithmetic for that
    unroll assumes (a grid of 2, the 64 KiB slice; a full iteration of that
    unroll in some slice wherever the docstring claims one)."""
    monkeypatch.setenv("NBX_BOOTSTRAP_TIMEOUT", "60")
    monkeypatch.setenv("NBX_TIMEOUT_SEC", "60")
    for k, v in cases.PROCESS_ENV.items():
        monkeypatch.setenv(k, v)
    for k in ("NBX_CHECK_PLANS", "NCCL_CHECK_POINTERS", "NBX_CHECK_SLICES", "NBX_SIMPLE_SLICE_BYTES", "NCCL_BUFFSIZE",
              "NBX_LL_MAX_BYTES", "NCCL_LL_BUFFSIZE", "NBX_LL128_MAX_BYTES", "NCCL_LL128_BUFFSIZE"):
        monkeypatch.delenv(k, raising=False)
    # the expected values are folded on a host thread while the ranks run
    def fold_all():
        return {(path, i): cases.expected(oracle, path, kind, dt, op, n, cases.root_of(i, n))
                for path in cases.PATHS for i, (kind, dt, op) in enumerate(cases.path_cases(path))}
    with ThreadPoolExecutor(1) as pool:
        folding = pool.submit(fold_all)
        res = _run_ranks(nbx, n, _child_edges, *(bytes(nbx.get_unique_id()) for _ in range(3)))
        expected = folding.result()

    settings = res[0]["settings"]
    for name in ("simple", "ring"):
        assert settings[name]["simpleGrid"] == cases.SIMPLE_GRID and settings[name]["sliceBytes"] == 64 << 10
    for name in cases.COMMS:
        assert settings[name]["checkPlans"] == 0 and settings[name]["checkSlices"] == 0
    # the unroll each Simple path runs at this n, and a full iteration of it where cases.py works one out
    iter_bytes = {p: cases.fold_unroll(p, n) * 256 * 16 for p in ("simple", "ring")}
    assert iter_bytes["simple"] == {2: 65536, 3: 32768, 5: 16384}[n] and iter_bytes["ring"] == 65536
    eb1 = dict(grid=settings["simple"]["simpleGrid"], slice_bytes=settings["simple"]["sliceBytes"])
    assert max(b for *_, b in cases.fold_spans("ar", cases.SIMPLE_BYTES, 1, n, False, **eb1)) >= iter_bytes["simple"]
    assert max(b for *_, b in cases.fold_spans("red", cases.SIMPLE_BYTES, 1, n, True, **eb1)) >= iter_bytes["ring"]

    failures, checked = [], 0
    for path in cases.PATHS:
        for i, (kind, dt, op) in enumerate(cases.path_cases(path)):
            root = cases.root_of(i, n)
            exp = expected[(path, i)]
            stt = oracle.NP_STORAGE[dt]
            shift = cases.shift_of(oracle, path, dt)
            want_rec = [(cases.family_of(path, kind, n), n, cases.host_unroll(path), 0)]
            for r in range(n):
                buf, recs = res[r][(path, i)]
                ctx = f"{path} {kind} {oracle.TYPE_NAMES[dt]} op {op} root {root} rank {r} of {n}"
                if [tuple(x) for x in recs] != want_rec:
                    failures.append(f"{ctx}: launch record {recs}, expected {want_rec}")
                if r not in exp:
                    assert buf is None and kind == "red"
                    continue
                e = np.ascontiguousarray(exp[r])
                lo = GUARD + shift
                assert buf.size == lo + e.nbytes + GUARD
                if not ((buf[:lo] == 0xA5).all() and (buf[lo + e.nbytes:] == 0xA5).all()):
                    failures.append(f"{ctx}: guard bytes overwritten: front {np.flatnonzero(buf[:lo] != 0xA5)[:8]}, "
                                    f"back {np.flatnonzero(buf[lo + e.nbytes:] != 0xA5)[:8]}")
                got = buf[lo:lo + e.nbytes].copy().view(stt)
                checked += 1
                if np.array_equal(got.view(np.uint8), e.view(np.uint8)):
                    continue   # equal bytes: mi.assert_same's rule holds
                try:
                    mi.assert_same(got, e, dt)
                except AssertionError as err:
                    d = mp_diag.describe_mismatch(got, e, _geometry(oracle, path, kind, dt, n, settings),
                                                  r * e.size if kind == "rs" else 0)
                    failures.append(f"{ctx}: {err}\n    all differing bytes (NaN payloads included): "
                                    f"{mp_diag.format_mismatch(d)}")
    # AllReduce and ReduceScatter on every rank, Reduce on its root
    per_path = {p: sum(n if k != "red" else 1 for k, _, _ in cases.path_cases(p)) for p in cases.PATHS}
    assert checked == sum(per_path.values())
    if failures:
        head = f"{len(failures)} failure(s) in {checked} outputs at {n} ranks"
        raise AssertionError(head + ":\n" + "\n".join(failures[:8]) + "\n" +
                             mp_diag.emit_summary([head] + [f.splitlines()[0][:160] for f in failures[:4]]))
