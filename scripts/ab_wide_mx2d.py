#!/usr/bin/env python3
"""A/B of the 2-D MXFP8 block-scaled sum (nbxReduceMultiWideMx2d) on one GPU.

Four legs on one rows x cols bucket, interleaved round by round in one process
(the method of scripts/ab_wide_mx_batch.py: device events around `inner`
back-to-back calls, `inner` sized per leg from a first timing so that a round's
calls last about --window seconds; medians with the 25th / 75th percentiles
over the rounds):
  (a) nbxReduceMultiWideMx2d with both copies,
  (b) nbxReduceMultiWideMx2d with the column-wise copy only,
  (c) what gave the same result before: nbxReduceMultiWideMx for the row-wise
      copy plus an fp32-output pass over the same sources (nbxReduceMultiWide,
      or nbxReduceMultiWideMx into fp32 for MX sources) — the least an outside
      column quantiser must have re-read,
  (d) nbxReduceMultiWideMx alone: (b)'s yardstick, the same bytes without the
      per-tile barrier.
Each leg's rate is the bytes that leg must move (sources, their scales, codes
and scales stored; for (c) the fp32 sum once) over its time. Every call goes
through prebuilt ctypes arguments. Each leg's launch record is checked once.
Rows: bf16 and MX e4m3 sources, 2 and 8 of them, into MX e4m3.

  python scripts/ab_wide_mx2d.py [--rows 8192 --cols 8192] [--rounds 15] [--out profiles/r19/ab_wide_mx2d_mi355x.txt]
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
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--cols", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of timed calls per leg and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "ab_wide_mx2d_mi355x.txt"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import _load_package
    if not torch.cuda.is_available():
        sys.exit("ab_wide_mx2d: no GPU; this script measures, it has no CPU form")
    nbx = _load_package()
    lib = nbx.load_library()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    op = nbx.DevRedOpFull()
    rows, cols = args.rows, args.cols
    assert rows % 32 == 0 and cols % 128 == 0, "whole tiles: the rates are the tile kernel's"
    n = rows * cols

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / inner

    def families(fn):
        nbx.launch_log_reset()
        fn()
        return [r[0] for r in nbx.launch_log()[1]]

    lines = [f"# {torch.cuda.get_device_name(0)}; {rows} x {cols} into MX e4m3; us per call, median [p25, p75] over "
             f"{args.rounds} interleaved rounds, and GB/s of the bytes the leg must move",
             f"# {'row':16s}{'inner a/b/c/d':>16s} {'(a) 2-D both':>30s} {'(b) 2-D columns':>30s} "
             f"{'(c) 1-D rows + fp32 pass':>30s} {'(d) 1-D rows':>30s}  a/c   b/d  rate b/d"]
    gen = torch.Generator(device="cuda").manual_seed(1)
    arr = lambda ts: nbx._ptr_array([t.data_ptr() for t in ts]) if ts else None

    for st, tname, eb, scaled in ((BF16, "bf16", 2, False), (E4M3, "mx-e4m3", 1, True)):
        for nsrc in (2, 8):
            hi = 0x4000 if eb == 2 else 0x70   # finite codes
            srcs = [torch.randint(0, hi, (n,), dtype=torch.int16 if eb == 2 else torch.uint8, device="cuda",
                                  generator=gen) for _ in range(nsrc)]
            sscales = [torch.randint(120, 134, (n // 32,), dtype=torch.uint8, device="cuda", generator=gen)
                       for _ in range(nsrc)] if scaled else None
            new = lambda k, dt=torch.uint8: torch.empty(k, dtype=dt, device="cuda")
            rc, rs, cc, cs, acc = new(n), new(n // 32), new(n), new(n // 32), new(n, torch.float32)
            S, SS = arr(srcs), arr(sscales)
            RC, RS, CC, CS, ACC = arr([rc]), arr([rs]), arr([cc]), arr([cs]), arr([acc])

            a = lambda: lib.nbxReduceMultiWideMx2d(RC, RS, CC, CS, 1, S, SS, nsrc, rows, cols, st, E4M3, op, 0, stream)
            b = lambda: lib.nbxReduceMultiWideMx2d(None, None, CC, CS, 1, S, SS, nsrc, rows, cols, st, E4M3, op, 0, stream)
            d = lambda: lib.nbxReduceMultiWideMx(RC, RS, 1, S, SS, nsrc, n, st, E4M3, op, 0, stream)

            def c():
                d()
                if scaled:
                    lib.nbxReduceMultiWideMx(ACC, None, 1, S, SS, nsrc, n, st, F32, op, 0, stream)
                else:
                    lib.nbxReduceMultiWide(ACC, 1, S, nsrc, n, st, F32, op, 0, stream)

            assert families(a) == [24] and families(b) == [24] and families(d) == [17] and families(c) == [17, 17 if scaled else 6]
            torch.cuda.synchronize()
            src_bytes = n * eb * nsrc + (n // 32 * nsrc if scaled else 0)
            copy = n + n // 32
            moved = {"a": src_bytes + 2 * copy, "b": src_bytes + copy, "c": 2 * src_bytes + copy + 4 * n, "d": src_bytes + copy}
            legs = dict(a=a, b=b, c=c, d=d)
            inner = {k: int(min(5000, max(3, args.window * 1e6 / timed(fn, 3)))) for k, fn in legs.items()}
            t = {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, fn in legs.items():
                    t[k].append(timed(fn, inner[k]))
            q = {k: np.percentile(v, [50, 25, 75]) for k, v in t.items()}
            rate = {k: moved[k] / q[k][0] / 1e3 for k in legs}
            cell = lambda k: f"{q[k][0]:9.1f} [{q[k][1]:.1f}, {q[k][2]:.1f}] {rate[k]:6.0f}".rjust(30)
            lines.append(f"{tname + ' x ' + str(nsrc):18s}{'/'.join(str(inner[k]) for k in 'abcd'):>16s} "
                         f"{cell('a')} {cell('b')} {cell('c')} {cell('d')}  {q['a'][0] / q['c'][0]:.3f} "
                         f"{q['b'][0] / q['d'][0]:.3f} {rate['b'] / rate['d']:.3f}")
            print(lines[-1], flush=True)
            del srcs, sscales, rc, rs, cc, cs, acc
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
