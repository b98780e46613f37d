#!/usr/bin/env python3
"""mp_creation_records.py — what communicator creation decides, case by case, as text.

For every case of a fixed list this creates a communicator under the case's environment in fresh
processes (one per rank, all on device 0; the two clique cases: one process, ncclCommInitAll) and
prints per rank: the creation's return code, the eleven nbxDebugCommSettings values,
nbxDebugCommProtoMask, and for one LL-, one LL128- and one Simple-sized AllReduce (8 KiB, 512 KiB,
4 MiB of fp32, the sizes of tests/test_multiprocess_gpu.py _child_knobs) the launch records and
whether the result is exact; for a creation that fails, ncclGetLastError's text. No pointer, pid
or time enters the output, so two builds of the library that decide alike print the same bytes:

    NBX_LIB=<parent's libnbxccl.so> python scripts/mp_creation_records.py --out records_parent.txt
    NBX_LIB=<head's libnbxccl.so>   python scripts/mp_creation_records.py --out records_head.txt
    cmp records_parent.txt records_head.txt          (profiles/r13)

At most three processes use the GPU at a time (the driver itself never touches it), every case
runs under one deadline for all its processes, and the run stops at the first child that times out
or fails. LIMIT: three times the 4.94 s that tests/edges/test_multiprocess_gpu.py's 2-rank child
takes on an MI355X (tests/clique/test_clique_transport_gpu.py EDGES_SECONDS) — that child imports
the same modules, creates communicators the same way and runs far more calls than a case here.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 3 * 4.94
COUNTS = (2048, 131072, 1 << 20)   # 8 KiB (LL), 512 KiB (LL128), 4 MiB (Simple) of fp32

# every variable a case sets, removed from the children's environment first
KNOBS = ("NCCL_BUFFSIZE", "NCCL_LL_BUFFSIZE", "NCCL_LL128_BUFFSIZE", "NCCL_MAX_NCHANNELS", "NCCL_MIN_NCHANNELS",
         "NCCL_MAX_CTAS", "NCCL_MIN_CTAS", "NCCL_CHECK_POINTERS", "NCCL_ALGO", "NCCL_PROTO", "NCCL_NTHREADS",
         "NBX_SIMPLE_SLICE_BYTES", "NBX_SIMPLE_MAX_GRID", "NBX_SIMPLE_SLOTS", "NBX_SIMPLE_PREFETCH",
         "NBX_LL_MAX_BYTES", "NBX_LL128_MAX_BYTES", "NBX_LL128_ONESHOT_MAX", "NBX_LL128_ACROSS_GPUS",
         "NBX_DEBUG_ASSUME_MULTI_GPU", "NBX_CHECK_PLANS", "NBX_CHECK_SLICES", "NBX_GROUP_BATCH", "NBX_IPC_VERIFY_FAIL",
         "NBX_CLIQUE_LL", "NBX_CLIQUE_SIMPLE", "NBX_MP_STREAM_ORDER", "NBX_LL128_SELFTEST_ITERS",
         "NBX_LL128_SELFTEST_FAIL", "NBX_DEBUG_SLICE_FAULT", "NBX_SYNC_MEM")


def _same(n, **env):
    return {k: [v] * n for k, v in env.items()}


REF = dict(NCCL_LL_BUFFSIZE="65536", NCCL_LL128_BUFFSIZE="1048576", NCCL_MAX_NCHANNELS="16")
# (name, ranks, {variable: [value of rank 0, ...]} (None: unset), ncclConfig_t fields or None, clique)
CASES = [
    ("defaults-2", 2, {}, None, False),
    ("defaults-3", 3, {}, None, False),
    ("buffsize-64k", 2, _same(2, NCCL_BUFFSIZE="65536", **REF), None, False),
    ("buffsize-4m", 2, _same(2, NCCL_BUFFSIZE="4194304", **REF), None, False),
    ("ctas-max8", 2, {}, {"maxCTAs": 8}, False),
    ("ctas-min16-max64", 2, {}, {"minCTAs": 16, "maxCTAs": 64}, False),
    ("ctas-max64-env4", 2, _same(2, NCCL_MAX_CTAS="4"), {"maxCTAs": 64}, False),
    ("ctas-max100-nchannels12", 2, _same(2, NCCL_MAX_NCHANNELS="12"), {"maxCTAs": 100}, False),
    ("nbx-override", 2, _same(2, NCCL_BUFFSIZE="262144", NBX_SIMPLE_SLICE_BYTES="16384", NCCL_MIN_NCHANNELS="8",
                              NCCL_MAX_NCHANNELS="4", NBX_SIMPLE_MAX_GRID="6"), None, False),
    ("plans-NCCL_CHECK_POINTERS", 2, _same(2, NCCL_CHECK_POINTERS="1"), None, False),
    ("plans-NBX_CHECK_PLANS", 2, _same(2, NBX_CHECK_PLANS="1"), None, False),
    ("check-slices", 2, _same(2, NBX_CHECK_SLICES="1"), None, False),
    ("algo-ring", 2, _same(2, NCCL_ALGO="Ring"), None, False),
    ("proto-not-ll128", 2, _same(2, NCCL_PROTO="^LL128"), None, False),
    ("assume-multi-gpu-proto-ll128", 2, _same(2, NCCL_PROTO="LL128", NBX_DEBUG_ASSUME_MULTI_GPU="1"), None, False),
    ("assume-multi-gpu", 2, _same(2, NBX_DEBUG_ASSUME_MULTI_GPU="1"), None, False),
    ("ll128-max-0", 2, _same(2, NBX_LL128_MAX_BYTES="0"), None, False),
    ("simple-slots-4", 2, _same(2, NBX_SIMPLE_SLOTS="4"), None, False),
] + [(f"ipc-verify-fail-1:{b}", 3, _same(3, NBX_IPC_VERIFY_FAIL=f"1:{b}"), None, False) for b in range(4)] + [
    (f"differ-{k}", 2, {k: v}, None, False) for k, v in (
        ("NCCL_BUFFSIZE", ["65536", "32768"]), ("NBX_GROUP_BATCH", ["1", "0"]),
        ("NCCL_LL_BUFFSIZE", ["65536", "32768"]), ("NBX_CHECK_PLANS", ["1", "0"]), ("NCCL_ALGO", ["Ring", None]),
        ("NBX_CHECK_SLICES", ["1", "0"]), ("NCCL_PROTO", ["LL", "Simple"]))
] + [
    ("clique-simple-on", 2, _same(2, NBX_CLIQUE_LL="1", GPU_MAX_HW_QUEUES="24", NBX_CLIQUE_SIMPLE="1"), None, True),
    ("clique-simple-off", 2, _same(2, NBX_CLIQUE_LL="1", GPU_MAX_HW_QUEUES="24", NBX_CLIQUE_SIMPLE="0"), None, True),
]


def _load():
    sys.path.insert(0, ROOT)
    from tests.conftest import load_package
    nbx = load_package()
    return nbx, nbx.load_library()


def _settings(nbx, lib, comm):
    import ctypes
    vals = (ctypes.c_int64 * 11)()
    got = lib.nbxDebugCommSettings(comm.handle, vals, 11)
    return {"settings": list(vals)[:max(got, 0)], "mask": int(lib.nbxDebugCommProtoMask(comm.handle))}


def _inputs(torch, cnt, r):
    return torch.remainder(torch.arange(cnt, device="cuda", dtype=torch.float32) * 3 + r, 101)


def child_rank(case, rank, uid_hex):
    """One rank of a multi-process case: prints its record as one JSON line."""
    import torch
    nbx, lib = _load()
    _, n, _, cfg, _ = case
    torch.cuda.set_device(0)
    uid = nbx.ncclUniqueId.from_buffer_copy(bytes.fromhex(uid_hex))
    try:
        if cfg is None:
            comm = nbx.Communicator.init_rank(n, uid, rank)
        else:
            comm, _ = nbx.Communicator.init_rank_config(n, uid, rank, **cfg)
    except nbx.NcclError as e:
        print(json.dumps({"rc": int(e.code), "detail": (lib.ncclGetLastError(None) or b"").decode(errors="replace")}))
        return
    out = {"rc": 0, **_settings(nbx, lib, comm)}
    st = torch.cuda.current_stream().cuda_stream
    for cnt in COUNTS:
        x, y = _inputs(torch, cnt, rank), torch.full((cnt,), -1.0, device="cuda")
        torch.cuda.synchronize()
        nbx.launch_log_reset()
        comm.all_reduce(x.data_ptr(), y.data_ptr(), cnt, 7, 0, st)
        total, recs = nbx.launch_log()
        torch.cuda.synchronize()
        want = sum(_inputs(torch, cnt, r) for r in range(n))
        out[str(cnt)] = {"launches": [total] + [list(r) for r in recs], "exact": bool(torch.equal(y, want))}
    out["async"] = comm.async_error()
    comm.destroy()
    print(json.dumps(out))


def child_clique(case):
    """A clique case: every rank of ncclCommInitAll on device 0 in this process, own streams."""
    import torch
    nbx, lib = _load()
    _, n, _, _, _ = case
    torch.cuda.set_device(0)
    comms = nbx.Communicator.init_all([0] * n)
    out = {"rc": 0, "ranks": [_settings(nbx, lib, c) for c in comms]}
    streams = [torch.cuda.Stream() for _ in range(n)]
    for cnt in COUNTS:
        xs = [_inputs(torch, cnt, r) for r in range(n)]
        ys = [torch.full((cnt,), -1.0, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        nbx.launch_log_reset()
        nbx.group_start()
        for r in range(n):
            comms[r].all_reduce(xs[r].data_ptr(), ys[r].data_ptr(), cnt, 7, 0, streams[r].cuda_stream)
        nbx.group_end()
        total, recs = nbx.launch_log()
        torch.cuda.synchronize()
        want = sum(xs)
        out[str(cnt)] = {"launches": [total] + [list(r) for r in recs],
                         "exact": [bool(torch.equal(y, want)) for y in ys]}
    out["async"] = [c.async_error() for c in comms]
    for c in comms:
        c.destroy()
    print(json.dumps(out))


def run_case(nbx, idx, case, out):
    """Starts the case's processes, waits for all of them under one deadline of LIMIT, writes their records.
    Returns False when the run has to stop (a child timed out or did not end with exit code 0)."""
    name, n, env, _, clique = case
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    base.update(NBX_BOOTSTRAP_TIMEOUT="10", NBX_TIMEOUT_SEC="5")   # a stuck wait gives up well inside LIMIT
    procs = []
    if clique:
        e = dict(base, **{k: v[0] for k, v in env.items()})
        procs.append(subprocess.Popen([sys.executable, __file__, "--clique", str(idx)], env=e, cwd=ROOT,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    else:
        uid_hex = bytes(nbx.get_unique_id()).hex()   # the bootstrap root listens in this process; no GPU
        for r in range(n):
            e = dict(base, **{k: v[r] for k, v in env.items() if v[r] is not None})
            procs.append(subprocess.Popen([sys.executable, __file__, "--rank", str(idx), str(r), uid_hex], env=e,
                                          cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    ok, deadline = True, time.monotonic() + LIMIT
    for r, p in enumerate(procs):
        try:
            so, se = p.communicate(timeout=max(0.0, deadline - time.monotonic()))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            out.write(f"{name} rank {r}: TIMEOUT, the case's {LIMIT:.1f} s are over\n")
            return False
        line = so.strip().splitlines()[-1] if so.strip() else ""
        if p.returncode != 0 or not line:
            out.write(f"{name} rank {r}: exit {p.returncode}\n")
            sys.stderr.write(se[-2000:])
            ok = False
        else:
            out.write(f"{name} rank {r}: {json.dumps(json.loads(line), sort_keys=True)}\n")
    out.flush()
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="the record file (default: stdout)")
    ap.add_argument("--rank", nargs=3, metavar=("CASE", "RANK", "UID"), help=argparse.SUPPRESS)
    ap.add_argument("--clique", metavar="CASE", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rank:
        return child_rank(CASES[int(a.rank[0])], int(a.rank[1]), a.rank[2])
    if a.clique:
        return child_clique(CASES[int(a.clique)])
    out = open(a.out, "w") if a.out else sys.stdout
    nbx, _ = _load()   # the driver: ncclGetUniqueId only, no GPU
    for idx, case in enumerate(CASES):
        if not run_case(nbx, idx, case, out):
            out.write("stopped: a child timed out or failed\n")
            out.flush()
            sys.exit(1)
    out.flush()


if __name__ == "__main__":
    main()
