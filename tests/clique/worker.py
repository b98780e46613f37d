"""The child process of tests/clique/test_clique_transport_gpu.py: one thread
drives every rank of in-process cliques whose ranks share GPU 0, with the
in-kernel transport forced on. The parent puts tests/clique/cases.CHILD_ENV into
this process's environment before it starts (GPU_MAX_HW_QUEUES has to be there
before HIP loads: every stream needs a hardware queue of its own, or one rank's
kernel queues behind a peer's waiting one).

usage: worker.py MODE N OUT [PATHS]
  MODE edges    part 1: the edge table at N ranks (PATHS: comma-separated subset)
       eight    part 2: the short table at 8 ranks
       routing  part 3: cases.routing_scenarios()
       groups   part 4: cases.group_scenarios() and the in-place cases
       premul   part 4: the user PreMulSum cases
Results are pickled to OUT. After every call (every scenario of the chain) the
worker synchronises and reads every rank's asynchronous error; at the first
one it issues no more GPU work, writes what it has plus ncclGetLastError under
"async_error", and exits with status 3."""
import ctypes
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests.clique import cases  # noqa: E402

GUARD = cases.GUARD


class AsyncFailure(Exception):
    pass


class Rig:
    def __init__(self, n, two_streams=False):
        import torch
        from oracle import oracle
        from tests.conftest import load_package
        self.torch, self.oracle, self.n = torch, oracle, n
        self.nbx = load_package()
        self.lib = self.nbx.load_library()
        self.lib.nbxDebugCommProtoMask.argtypes = [ctypes.c_void_p]
        self.lib.nbxDebugCommProtoMask.restype = ctypes.c_int
        self.lib.nbxDebugChooseProto.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
                                                 ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
        self.lib.nbxDebugChooseProto.restype = ctypes.c_int
        torch.cuda.set_device(0)
        assert two_streams is False or n <= cases.TWO_STREAM_MAX_N
        assert cases.streams_needed(n, two_streams) + 1 <= int(os.environ["GPU_MAX_HW_QUEUES"]) <= 32
        self.own = [torch.cuda.Stream() for _ in range(n)]
        self.own2 = [torch.cuda.Stream() for _ in range(n)] if two_streams else None
        self.shared = torch.cuda.Stream()
        self.comms, self.info = {}, {}

    def make_comms(self, name, env):
        """One clique under its own environment (as tests/edges' child creates its communicators)."""
        from tests import mp_diag
        for k in cases.ENV_KEYS:
            os.environ.pop(k, None)
        os.environ["NBX_CLIQUE_LL"] = "1"
        os.environ.update(env)
        self.comms[name] = self.nbx.Communicator.init_all([0] * self.n)
        os.environ["NBX_CLIQUE_LL"] = "1"
        self.info[name] = {"masks": [int(self.lib.nbxDebugCommProtoMask(c.handle)) for c in self.comms[name]],
                           "settings": [mp_diag.comm_settings(self.nbx, c) for c in self.comms[name]]}

    def stream(self, which, r):
        s = {"own": self.own, "own2": self.own2}.get(which)
        return (self.shared if s is None else s[r]).cuda_stream

    def check(self):
        self.torch.cuda.synchronize()
        for name, comms in self.comms.items():
            errs = [c.async_error() for c in comms]
            if any(errs):
                raise AsyncFailure(f"communicator {name}: async errors {errs}: "
                                   f"{(self.lib.ncclGetLastError(None) or b'').decode(errors='replace')}")

    def proto(self, name, kind, count, eb):
        """nbxDebugChooseProto under the communicator's own mask and thresholds (None: no transport)."""
        from tests import mp_diag
        mask, st = self.info[name]["masks"][0], self.info[name]["settings"][0]
        if mask < 0 or count == 0:
            return None
        lo, hi = mp_diag.block_range(count, eb, self.n, 0)
        return int(self.lib.nbxDebugChooseProto(mask, int(kind != "rs"), count * eb, (hi - lo) * eb, self.n,
                                                st["llMax"], st["l128Max"], 256 << 10))

    def upload(self, data_u8, shift=0):
        host = np.full(GUARD + shift + data_u8.size + GUARD, 0xA5, dtype=np.uint8)
        host[GUARD + shift:GUARD + shift + data_u8.size] = data_u8
        t = self.torch.from_numpy(host).cuda()
        assert t.data_ptr() % 16 == 0
        return t

    def destroy(self):
        for comms in self.comms.values():
            for c in comms:
                c.destroy()


def run_one(rig, comms, kind, dt, ops, count, root, sends, recvs):
    """One case: group_start, the n ranks' calls on their own streams, group_end; the calling
    thread's launch record of exactly that. ops: the op of every rank."""
    nbx = rig.nbx
    rig.torch.cuda.synchronize()
    nbx.launch_log_reset()
    nbx.group_start()
    for r in range(rig.n):
        st = rig.stream("own", r)
        if kind == "ar":
            comms[r].all_reduce(sends[r], recvs[r], count, dt, ops[r], st)
        elif kind == "rs":
            comms[r].reduce_scatter(sends[r], recvs[r], count, dt, ops[r], st)
        else:
            comms[r].reduce(sends[r], recvs[r] if r == root else 0, count, dt, ops[r], root, st)
    nbx.group_end()
    total, recs = nbx.launch_log()
    assert total == len(recs)
    rig.check()
    return recs


def run_table(rig, out, tag, table):
    """table: [(path, index, kind, dtype, op)], the edge inputs; results under (tag, path, index):
    ([every rank's output with its guard bytes, None on a Reduce's non-roots], records)."""
    oracle, n, torch = rig.oracle, rig.n, rig.torch
    uploads = {}   # one upload per (input, placement, rank): the ops of a type share it
    for path, i, kind, dt, op in table:
        comms = rig.comms[cases.PATH_COMM[path]]
        count, shift = cases.count_of(oracle, path, dt), cases.shift_of(oracle, path, dt)
        key = (dt, cases.nbytes_of(oracle, path, dt), kind == "rs", shift)
        if key not in uploads:
            uploads[key] = [rig.upload(np.ascontiguousarray(cases.rank_input(oracle, path, kind, dt, n, r))
                                       .view(np.uint8), shift) for r in range(n)]
        nb = count * cases.itemsize(oracle, dt)
        tys = [torch.full((GUARD + shift + nb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(n)]
        assert all(t.data_ptr() % 16 == 0 for t in tys)
        root = cases.root_of(i, n)
        recs = run_one(rig, comms, kind, dt, [op] * n, count, root,
                       [t.data_ptr() + GUARD + shift for t in uploads[key]],
                       [t.data_ptr() + GUARD + shift for t in tys])
        out[(tag, path, i)] = ([tys[r].cpu().numpy() if kind != "red" or r == root else None for r in range(n)], recs)


def run_inplace(rig, out):
    """AllReduce with recv == send, ReduceScatter with recv == send + rank x count: every rank's
    whole send buffer afterwards."""
    oracle, n = rig.oracle, rig.n
    for path, kind in cases.inplace_cases():
        dt = cases.F16
        comms = rig.comms[cases.PATH_COMM[path]]
        count, shift = cases.count_of(oracle, path, dt), cases.shift_of(oracle, path, dt)
        eb = cases.itemsize(oracle, dt)
        txs = [rig.upload(np.ascontiguousarray(cases.rank_input(oracle, path, kind, dt, n, r)).view(np.uint8), shift)
               for r in range(n)]
        sends = [t.data_ptr() + GUARD + shift for t in txs]
        recvs = [s + (r * count * eb if kind == "rs" else 0) for r, s in enumerate(sends)]
        recs = run_one(rig, comms, kind, dt, [cases.SUM] * n, count, 0, sends, recvs)
        out[("inplace", path, kind)] = ([t.cpu().numpy() for t in txs], recs)


def run_premul(rig, out):
    """A user PreMulSum whose scalar differs on every rank, host-immediate or device-resident."""
    oracle, n, torch, nbx = rig.oracle, rig.n, rig.torch, rig.nbx
    for path, kind, dt, device_scalar in cases.premul_cases():
        comms = rig.comms[cases.PATH_COMM[path]]
        count = cases.count_of(oracle, path, dt)
        nb = count * cases.itemsize(oracle, dt)
        xs = cases.premul_inputs(oracle, path, kind, dt, n)
        txs = [rig.upload(np.ascontiguousarray(x).view(np.uint8)) for x in xs]
        tys = [torch.full((GUARD + nb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(n)]
        ops, keep = [], []
        for r in range(n):
            sc = cases._premul_scalar(np, dt, r)
            if device_scalar:
                dsc = torch.from_numpy(sc.view(np.uint8).copy()).cuda()
                keep.append(dsc)
                ops.append(comms[r].redop_create_premulsum(dsc.data_ptr(), dt,
                                                           nbx.ncclScalarResidence.ncclScalarDevice))
            else:
                keep.append(sc)
                ops.append(comms[r].redop_create_premulsum(sc.ctypes.data, dt))
        root = 1 % n
        recs = run_one(rig, comms, kind, dt, ops, count, root, [t.data_ptr() + GUARD for t in txs],
                       [t.data_ptr() + GUARD for t in tys])
        for r in range(n):
            comms[r].redop_destroy(ops[r])
        out[("premul", path, kind, dt, device_scalar)] = (
            [tys[r].cpu().numpy() if kind != "red" or r == root else None for r in range(n)], recs)


def run_scenario(rig, out, si, sc):
    """A scenario's groups in order; results under ("scenario", name): every buffer of every rank
    with its guard bytes, the records and the result code of every group, the protocol of every call."""
    oracle, n, nbx = rig.oracle, rig.n, rig.nbx
    comms = rig.comms[sc.comm]
    first = cases.initial_buffers(oracle, si, sc, n)
    bufs = [{name: rig.upload(data) for name, data in first[r].items()} for r in range(n)]
    res = {"records": [], "codes": [], "protos": []}
    out[("scenario", sc.name)] = res
    rig.torch.cuda.synchronize()
    for g in sc.groups:
        res["protos"].append([rig.proto(sc.comm, c.kind, c.count, cases.itemsize(oracle, c.dtype)) for c in g])
        nbx.launch_log_reset()
        nbx.group_start()
        for c in g:
            for r in range(n):
                send, recv = bufs[r][c.send].data_ptr() + GUARD, bufs[r][c.recv].data_ptr() + GUARD
                count = c.count - 1 if c.bad_rank == r else c.count
                st = rig.stream(c.stream, r)
                if c.kind == "ar":
                    comms[r].all_reduce(send, recv, count, c.dtype, c.op, st)
                elif c.kind == "rs":
                    comms[r].reduce_scatter(send, recv, count, c.dtype, c.op, st)
                else:
                    comms[r].reduce(send, recv if r == c.root else 0, count, c.dtype, c.op, c.root, st)
        code = 0
        try:
            nbx.group_end()
        except nbx.NcclError as e:
            code = int(e.code)
        total, recs = nbx.launch_log()
        assert total == len(recs)
        res["records"].append(recs)
        res["codes"].append(code)
        if sc.sync:
            rig.check()
    rig.check()
    res["buffers"] = [{name: t.cpu().numpy() for name, t in bufs[r].items()} for r in range(n)]


def main():
    mode, n, out_path = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    paths = sys.argv[4].split(",") if len(sys.argv) > 4 else list(cases.PATHS)
    out = {}
    rig = Rig(n, two_streams=mode == "groups")
    status = 0
    try:
        if mode == "premul":
            paths = list(cases.PREMUL_PATHS)
        if mode in ("edges", "eight", "groups", "premul"):
            for name in cases.COMMS:
                if any(cases.PATH_COMM[p] == name for p in paths):
                    rig.make_comms(name, cases.COMM_ENV[name])
        if mode == "edges":
            run_table(rig, out, "edges", [(p, i, *c) for p in paths for i, c in enumerate(cases.path_cases(p))])
        elif mode == "eight":
            run_table(rig, out, "eight", [(p, i, *c) for p in cases.EIGHT_PATHS
                                          for i, c in enumerate(cases.eight_cases(p))])
        elif mode == "premul":
            run_premul(rig, out)
        else:
            scenarios = cases.routing_scenarios() if mode == "routing" else cases.group_scenarios()
            for name in dict.fromkeys(sc.comm for sc in scenarios):
                rig.make_comms(name, cases.SCENARIO_COMM_ENV[name])
            for si, sc in enumerate(scenarios):
                run_scenario(rig, out, si, sc)
            if mode == "groups":
                run_inplace(rig, out)
        rig.check()
        rig.destroy()
    except AsyncFailure as e:   # a device wait gave up: every later call would wait out the timeout too
        out["async_error"] = str(e)
        status = 3
    out["info"] = rig.info
    with open(out_path, "wb") as f:
        pickle.dump(out, f, protocol=4)
    sys.exit(status)


if __name__ == "__main__":
    main()
