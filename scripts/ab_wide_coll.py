#!/usr/bin/env python3
"""Per-step against wide (fp32-accumulating) AllReduce on a multi-process
communicator whose ranks share GPU 0: bf16 and fp8 e4m3 at 2 and 4 ranks, at
16 KiB (LL), 512 KiB (LL128) and 16 MiB (Simple) per rank.

The two operators are interleaved call by call in the same run (per-step,
wide, per-step, ...), each call timed on its rank's stream with a pair of
events; the warm-up calls are discarded and the median of ITERS calls per
operator is reported, with the per-step calls' own spread (25th / 75th
percentile) beside it: a wide figure inside that spread is no difference.
The times are rank 0's; every rank waits for its peers inside the kernel, so
the ranks' medians agree to the spread.

usage: python scripts/ab_wide_coll.py [OUT.txt]       (needs one MI355X)
The table in profiles/r10/ab_wide_coll_mi355x.txt is this script's output."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

WARMUP, ITERS = 10, 30
BF16, E4M3 = 9, 10
SIZES = ((16 << 10, "LL"), (512 << 10, "LL128"), (16 << 20, "Simple"))
FAMILY = {8: "LL", 9: "LL128", 10: "LL128x2", 11: "Simple", 12: "SimpleRing"}


def child(uid, rank, n, q):
    try:
        import torch
        from tests.conftest import load_package
        nbx = load_package()
        torch.cuda.set_device(0)
        comm = nbx.Communicator.init_rank(n, nbx.ncclUniqueId.from_buffer_copy(uid), rank)
        s = torch.cuda.Stream()
        rows = []
        with torch.cuda.stream(s):
            for dt, name, eb in ((BF16, "bf16", 2), (E4M3, "e4m3", 1)):
                wide = comm.redop_create_wide(0, dt)
                for nbytes, _ in SIZES:
                    count = nbytes // eb
                    gen = torch.Generator(device="cuda").manual_seed(17 + rank)
                    tx = torch.randint(0, 120, (nbytes,), dtype=torch.uint8, device="cuda", generator=gen)
                    ty = torch.empty_like(tx)
                    times = {0: [], wide: []}
                    fam = {}
                    for it in range(WARMUP + ITERS):
                        for op in (0, wide):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            nbx.launch_log_reset()
                            e0.record(s)
                            comm.all_reduce(tx.data_ptr(), ty.data_ptr(), count, dt, op, s.cuda_stream)
                            e1.record(s)
                            fam[op] = nbx.launch_log()[1][-1]
                            e1.synchronize()
                            if it >= WARMUP:
                                times[op].append(e0.elapsed_time(e1) * 1e3)
                    rows.append((n, name, nbytes, tuple(fam[0]), tuple(fam[wide]), times[0], times[wide]))
                comm.redop_destroy(wide)
        assert comm.async_error() == 0
        comm.destroy()
        q.put((rank, "ok", rows))
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc()))


def main():
    from tests.conftest import load_package
    from tests.test_multiprocess_gpu import _run_ranks
    os.environ.setdefault("NBX_BOOTSTRAP_TIMEOUT", "60")
    os.environ.setdefault("NBX_TIMEOUT_SEC", "60")
    os.environ.setdefault("NBX_LL128_MAX_GRID", "16")   # every rank's grid resident on the shared GPU, as the tests
    nbx = load_package()
    lines = [f"# scripts/ab_wide_coll.py: AllReduce, ranks sharing one GPU, {WARMUP} warm-up + {ITERS} timed calls per "
             "operator, interleaved; microseconds, rank 0",
             f"# {'ranks':>5} {'type':>5} {'bytes':>9} {'kernel':>8} {'per-step med':>13} {'p25':>8} {'p75':>8} "
             f"{'wide med':>9} {'wide/step':>9}  verdict"]
    for n in (2, 4):
        res = _run_ranks(nbx, n, child)
        for (nr, name, nbytes, f0, f1, t0, t1) in res[0]:
            assert f0[0] == f1[0] and f0[3] & 2 == 0 and f1[3] & 2 == 2, (f0, f1)
            m0, m1 = float(np.median(t0)), float(np.median(t1))
            p25, p75 = float(np.percentile(t0, 25)), float(np.percentile(t0, 75))
            verdict = "within the per-step spread" if p25 <= m1 <= p75 else ("slower" if m1 > p75 else "faster")
            lines.append(f"  {nr:>5} {name:>5} {nbytes:>9} {FAMILY[f0[0]]:>8} {m0:>13.1f} {p25:>8.1f} {p75:>8.1f} {m1:>9.1f} "
                         f"{m1 / m0:>9.3f}  {verdict}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
