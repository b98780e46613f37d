"""The child process of tests/widecoll/test_clique_transport_gpu.py: one thread drives
the 3 ranks of in-process cliques that share GPU 0 (tests/clique/worker.py's
rig: the parent puts tests/clique/cases.CHILD_ENV into the environment before
HIP loads), or a one-rank communicator.

usage: worker.py MODE OUT
  MODE fold     the event-ordered fold path (NBX_CLIQUE_LL=0): the wide core
       kernel   the in-kernel transport (NBX_CLIQUE_LL=1): an LL clique and a Simple one
       onerank  a one-rank communicator: handle checks, wide Avg as a copy
Results are pickled to OUT."""
import ctypes
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests.clique import worker as cw  # noqa: E402
from tests.widecoll import cases  # noqa: E402

N, COUNT, GUARD = 3, 5003, 16
TYPES = (cases.BF16, cases.E4M3)
KINDS = ("ar", "rs", "red")
ROOT_RANK = 1


def clique_cases():
    return [(kind, dt, op) for kind in KINDS for dt in TYPES for op in cases.OPS]


def inputs(oracle, kind, dt, op):
    """Rank inputs of one case: uniform for Sum, edge-rich for Avg."""
    total = COUNT * N if kind == "rs" else COUNT
    return cases._sources(oracle, "uniform" if op == cases.SUM else "edge", dt, COUNT, total)[:N]


def run_cases(rig, name, out):
    oracle, torch = rig.oracle, rig.torch
    comms = rig.comms[name]
    handles = {(dt, op): [c.redop_create_wide(op, dt) for c in comms] for dt in TYPES for op in cases.OPS}
    for i, (kind, dt, op) in enumerate(clique_cases()):
        xs = inputs(oracle, kind, dt, op)
        ups = [rig.upload(np.ascontiguousarray(x).view(np.uint8)) for x in xs]
        nb = COUNT * xs[0].itemsize
        tys = [torch.full((GUARD + nb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(N)]
        recs = cw.run_one(rig, comms, kind, dt, handles[(dt, op)], COUNT, ROOT_RANK,
                          [t.data_ptr() + GUARD for t in ups], [t.data_ptr() + GUARD for t in tys])
        out[(name, i)] = ([tys[r].cpu().numpy() if kind != "red" or r == ROOT_RANK else None for r in range(N)], recs)
    for (dt, op), hs in handles.items():
        for c, h in zip(comms, hs):
            c.redop_destroy(h)


def one_rank(out):
    import torch
    from oracle import oracle
    from tests.conftest import load_package
    nbx = load_package()
    lib = nbx.load_library()
    torch.cuda.set_device(0)
    comm = nbx.Communicator.init_all([0])[0]
    st = torch.cuda.current_stream().cuda_stream
    f = lib.nbxRedOpCreateWide
    f.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    f.restype = ctypes.c_int
    op = ctypes.c_int(-7)
    # argument checks on a live communicator
    user = comm.redop_create_wide(0, cases.BF16)
    out["bad"] = [f(None, 0, 9, comm.handle), f(ctypes.byref(op), 1, 9, comm.handle), f(ctypes.byref(op), user, 9, comm.handle),
                  f(ctypes.byref(op), 0, 7, comm.handle), f(ctypes.byref(op), 4, 2, comm.handle), op.value]
    # create / destroy / reuse of a slot
    second = comm.redop_create_wide(4, cases.E4M3)
    comm.redop_destroy(user)
    again = comm.redop_create_wide(4, cases.F16)
    out["slots"] = (user, second, again, lib.ncclRedOpDestroy(user + 1000, comm.handle))
    x = np.ascontiguousarray(cases._sources(oracle, "edge", cases.F16, COUNT, COUNT)[0])
    tx = torch.from_numpy(x.view(np.uint8).copy()).cuda()
    ty = torch.full((x.nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    # the datatype given at the call must be the handle's
    out["mismatch"] = lib.ncclAllReduce(ctypes.c_void_p(tx.data_ptr()), ctypes.c_void_p(ty.data_ptr()), COUNT, cases.BF16,
                                        again, comm.handle, ctypes.c_void_p(st))
    # wide Avg at one rank: a copy out of place, nothing in place; no kernel of the reduction core
    nbx.launch_log_reset()
    comm.all_reduce(tx.data_ptr(), ty.data_ptr(), COUNT, cases.F16, again, st)
    comm.reduce_scatter(tx.data_ptr(), tx.data_ptr(), COUNT, cases.F16, again, st)
    comm.reduce(tx.data_ptr(), tx.data_ptr(), COUNT, cases.F16, again, 0, st)
    torch.cuda.synchronize()
    out["copy"] = (x, ty.cpu().numpy().view(np.uint16), tx.cpu().numpy().view(np.uint16), nbx.launch_log()[1])
    out["async"] = comm.async_error()
    comm.redop_destroy(again)
    comm.redop_destroy(second)
    comm.destroy()


def main():
    mode, out_file = sys.argv[1], sys.argv[2]
    out = {}
    if mode == "onerank":
        one_rank(out)
    else:
        rig = cw.Rig(N)
        try:
            if mode == "fold":
                for k in cw.cases.ENV_KEYS:
                    os.environ.pop(k, None)
                os.environ["NBX_CLIQUE_LL"] = "0"
                rig.comms["fold"] = rig.nbx.Communicator.init_all([0] * N)
                run_cases(rig, "fold", out)
            else:
                rig.make_comms("ll", cases.COMM_ENV["ll"])
                rig.make_comms("simple", cases.COMM_ENV["simple"])
                run_cases(rig, "ll", out)
                run_cases(rig, "simple", out)
            rig.destroy()
        except cw.AsyncFailure as e:
            out["async_error"] = str(e)
            with open(out_file, "wb") as fh:
                pickle.dump(out, fh)
            sys.exit(3)
    with open(out_file, "wb") as fh:
        pickle.dump(out, fh)


if __name__ == "__main__":
    main()
