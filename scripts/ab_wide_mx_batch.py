#!/usr/bin/env python3
"""A/B of the batched MXFP8 block-scaled sum (nbxReduceMultiWideMxBatch) on one GPU.

Three ways to reduce a set of buckets, interleaved round by round in one
process (the method of scripts/ab_wide_mx.py: device events around `inner`
back-to-back passes over the set, `inner` sized per row and leg from a first
timing so that a round's passes last about --window seconds, the batched legs
in bursts of 48 so that no call runs out of table slots; medians with the 25th / 75th percentiles over the rounds):
  (a) one nbxReduceMultiWideMx call per bucket, the only path before the batch,
  (b) one nbxReduceMultiWideMxBatch call,
  (c) one nbxReduceMultiWideBatch call into fp32 on the same buckets (for MX
      sources: their codes as plain e4m3), the 4 B / element store, for the
      byte context.
Every call goes through prebuilt ctypes arguments, so a leg's host cost is the
library's and one foreign call per launch. Each leg's launch record is checked
once (17 per bucket / 21 / 15).
Rows: bf16 x 8 and x 2 sources into MX e4m3, MX e4m3 x 8 sources into MX e4m3.
Bucket sets: 128 x 32 Ki elements, 384 x 8 Ki, 16 x 1 Mi.

  python scripts/ab_wide_mx_batch.py [--rounds 15] [--out profiles/r16/ab_wide_mx_batch_mi355x.txt]
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32, BF16, E4M3 = 7, 9, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--window", type=float, default=0.05, help="seconds of timed passes per leg and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "ab_wide_mx_batch_mi355x.txt"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import _load_package
    if not torch.cuda.is_available():
        sys.exit("ab_wide_mx_batch: no GPU; this script measures, it has no CPU form")
    nbx = _load_package()
    lib = nbx.load_library()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    op = nbx.DevRedOpFull()

    def timed(fn, inner, burst):
        """us per pass over `inner` passes, in event-timed bursts with a synchronise (untimed) between them."""
        ms, left = 0.0, inner
        while left > 0:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(min(burst, left)):
                fn()
            e1.record()
            e1.synchronize()
            ms += e0.elapsed_time(e1)
            left -= burst
        return ms * 1000.0 / inner

    def families(fn):
        nbx.launch_log_reset()
        fn()
        total, recs = nbx.launch_log()
        return total, sorted({r[0] for r in recs})

    lines = [f"# {torch.cuda.get_device_name(0)}; us per bucket set, median [p25, p75] over {args.rounds} interleaved "
             f"rounds", f"# {'row':28s}{'inner a/b/c':>14s} {'(a) MX call per bucket':>26s} {'(b) MX batch':>24s} "
                        f"{'(c) wide batch fp32':>24s}  b/a   b/c"]
    gen = torch.Generator(device="cuda").manual_seed(1)

    for st, tname, eb, scaled, nsrc in ((BF16, "bf16", 2, False, 8), (BF16, "bf16", 2, False, 2),
                                        (E4M3, "mx-e4m3", 1, True, 8)):
        for nb, count in ((128, 32 << 10), (384, 8 << 10), (16, 1 << 20)):
            n = nb * count
            hi = 0x4000 if eb == 2 else 0x70   # finite codes
            srcs = [torch.randint(0, hi, (n,), dtype=torch.int16 if eb == 2 else torch.uint8, device="cuda",
                                  generator=gen) for _ in range(nsrc)]
            sscales = [torch.randint(120, 134, (n // 32,), dtype=torch.uint8, device="cuda", generator=gen)
                       for _ in range(nsrc)] if scaled else None
            codes = torch.empty(n, dtype=torch.uint8, device="cuda")
            dscales = torch.empty(n // 32, dtype=torch.uint8, device="cuda")
            acc = torch.empty(n, dtype=torch.float32, device="cuda")
            at = lambda t, k, per: t.data_ptr() + k * per
            mx = [([at(codes, k, count)], [at(dscales, k, count // 32)], [at(s, k, count * eb) for s in srcs],
                   [at(e, k, count // 32) for e in sscales] if scaled else None, count) for k in range(nb)]
            wide = [([at(acc, k, count * 4)], [at(s, k, count * eb) for s in srcs], count) for k in range(nb)]
            mx_tasks, keep_mx = nbx._reduce_mx_tasks(mx)
            wide_tasks, keep_wide = nbx._reduce_tasks(wide)

            single = [(t.dsts, t.dstScales, t.srcs, t.srcScales) for t in mx_tasks]

            def a():
                for d, dsc, s, ssc in single:
                    lib.nbxReduceMultiWideMx(d, dsc, 1, s, ssc, nsrc, count, st, E4M3, op, 0, stream)

            b = lambda: lib.nbxReduceMultiWideMxBatch(mx_tasks, nb, st, E4M3, op, 0, stream)
            c = lambda: lib.nbxReduceMultiWideBatch(wide_tasks, nb, st, F32, op, 0, stream)
            assert families(a) == (nb, [17]) and families(b)[1] == [21] and families(c)[1] == [15]
            torch.cuda.synchronize()
            # a batched call holds one or two of the arena's 128 table slots until it completes, and a call
            # that finds none runs one launch per bucket: bursts of 48 keep the queue inside the arena
            burst = {"a": 1 << 30, "b": 48, "c": 48}
            inner = {k: int(min(5000, max(5, args.window * 1e6 / timed(fn, 3, 3)))) for k, fn in zip("abc", (a, b, c))}
            fb0 = lib.nbxDebugBatchListSlots(torch.cuda.current_device(), 3)
            t = {k: [] for k in "abc"}
            for _ in range(args.rounds):
                for k, fn in zip("abc", (a, b, c)):
                    t[k].append(timed(fn, inner[k], burst[k]))
            assert lib.nbxDebugBatchListSlots(torch.cuda.current_device(), 3) == fb0, "a timed call found no table slot"
            q = {k: np.percentile(v, [50, 25, 75]) for k, v in t.items()}
            cell = lambda k, w: f"{q[k][0]:9.1f} [{q[k][1]:.1f}, {q[k][2]:.1f}]".rjust(w)
            row = f"{tname} {nsrc} src {nb} x {count >> 10} Ki"
            lines.append(f"{row:30s}{'/'.join(str(inner[k]) for k in 'abc'):>14s} {cell('a', 26)} {cell('b', 24)} {cell('c', 24)}  "
                         f"{q['b'][0] / q['a'][0]:.3f} {q['b'][0] / q['c'][0]:.3f}")
            print(lines[-1], flush=True)
            del srcs, sscales, codes, dscales, acc, keep_mx, keep_wide
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
