#!/usr/bin/env python3
"""A/B of the fused bucket statistics (nbxReduceMultiWideStats) on one GPU.

Three ways to get a reduced bucket and its amax / sum of squares, interleaved
round by round in one process so that drift and neighbours hit all alike:
  (a) nbxReduceMultiWide alone (no statistics: the floor),
  (b) nbxReduceMultiWideStats,
  (c) (a), then the second pass a caller writes today over the fp32 output:
      torch.amax(abs) and torch.linalg.vector_norm (for a narrow output the
      caller has no fp32 master to read: (c) reads the narrow result).
Rows: bf16 / e4m3, 2 / 8 sources, fp32 / narrow output, 1 Mi / 16 Mi / 128 Mi
elements, and the batch at 128 buckets of 64 KiB with 8 sources. Every timing is
device events around `inner` back-to-back calls, `inner` sized per row from a
first timing of (a) so that its window lasts about --window seconds (0.05 s:
several thousand calls at 1 Mi elements, 100 to 700 at 128 Mi; (b) and (c) run the same
count, so their windows are longer); medians with the 25th / 75th percentiles
over the rounds, in microseconds per call.

  python scripts/ab_wide_stats.py [--rounds 15] [--out profiles/r11/ab_wide_stats_mi355x.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32, BF16, E4M3 = 7, 9, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--window", type=float, default=0.05, help="seconds of (a) per timed window")
    ap.add_argument("--max-elts", type=int, default=128 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "ab_wide_stats_mi355x.txt"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import _load_package
    if not torch.cuda.is_available():
        sys.exit("ab_wide_stats: no GPU; this script measures, it has no CPU form")
    nbx = _load_package()
    nbx.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    op = nbx.DevRedOpFull()
    stats = torch.zeros(16 * 128, dtype=torch.uint8, device="cuda")

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / inner

    def two_pass(outs, out32):
        for o in outs:
            v = o if out32 else o.view(torch.bfloat16 if o.element_size() == 2 else torch.float8_e4m3fn).float()
            torch.amax(v.abs())
            torch.linalg.vector_norm(v)

    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median [p25, p75] over {args.rounds} interleaved rounds",
             f"# {'row':38s}{'inner':>6s} {'(a) wide':>22s} {'(b) wide+stats':>22s} {'(c) wide, two-pass':>22s}  b/a   b/c"]

    def row(name, a, b, c):
        for fn in (a, b, c):   # warm every shape
            fn()
        torch.cuda.synchronize()
        inner = int(min(10000, max(10, args.window * 1e6 / timed(a, 10))))
        t = {k: [] for k in "abc"}
        for _ in range(args.rounds):
            for k, fn in zip("abc", (a, b, c)):
                t[k].append(timed(fn, inner))
        q = {k: np.percentile(v, [50, 25, 75]) for k, v in t.items()}
        cell = lambda k: f"{q[k][0]:9.1f} [{q[k][1]:.1f}, {q[k][2]:.1f}]".rjust(22)
        lines.append(f"{name:40s}{inner:6d} {cell('a')} {cell('b')} {cell('c')}  {q['b'][0] / q['a'][0]:.3f} {q['b'][0] / q['c'][0]:.3f}")
        print(lines[-1], flush=True)

    gen = torch.Generator(device="cuda").manual_seed(1)

    def codes(n, eb):   # finite, |x| < 2 (bf16) or <= 60 (e4m3): the square-sum stays far below 2^120
        if eb == 2:
            return torch.randint(0, 0x4000, (n,), dtype=torch.int16, device="cuda", generator=gen).view(torch.uint8)
        return torch.randint(0, 0x70, (n,), dtype=torch.uint8, device="cuda", generator=gen)

    for st, tname, eb in ((BF16, "bf16", 2), (E4M3, "e4m3", 1)):
        for n in (1 << 20, 16 << 20, 128 << 20):
            if n > args.max_elts:
                continue
            for nsrc in (2, 8):
                srcs = [codes(n, eb) for _ in range(nsrc)]
                sp = [s.data_ptr() for s in srcs]
                for out32 in (True, False):
                    out = torch.empty(n * (4 if out32 else eb), dtype=torch.uint8, device="cuda")
                    view = out.view(torch.float32) if out32 else out.view(torch.int16 if eb == 2 else torch.uint8)
                    dt = F32 if out32 else st
                    a = lambda: nbx.reduce_multi_wide([out.data_ptr()], sp, n, st, dt, op, 0, stream)
                    b = lambda: nbx.reduce_multi_wide_stats([out.data_ptr()], sp, n, st, dt, op, stats.data_ptr(), 0, stream)
                    c = lambda: (a(), two_pass([view], out32))
                    row(f"{tname} {nsrc} src -> {'fp32' if out32 else tname} {n >> 20} Mi", a, b, c)
                    del out, view
                del srcs
    # the batch: 128 buckets of 64 KiB bf16, 8 sources, fp32 output
    nb, n = 128, 32768
    srcs = [[codes(n, 2) for _ in range(8)] for _ in range(nb)]
    outs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(nb)]
    tasks = [([o.data_ptr()], [s.data_ptr() for s in ss], n) for o, ss in zip(outs, srcs)]
    a = lambda: nbx.reduce_multi_wide_batch(tasks, BF16, F32, op, 0, stream)
    b = lambda: nbx.reduce_multi_wide_batch_stats(tasks, BF16, F32, op, stats.data_ptr(), 0, stream)
    c = lambda: (a(), two_pass(outs, True))
    row("batch 128 x 64 KiB bf16 8 src -> fp32", a, b, c)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
