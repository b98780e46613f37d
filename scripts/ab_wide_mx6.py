#!/usr/bin/env python3
"""A/B of the MXFP6 block-scaled sum (nbxReduceMultiWideMx, NBX_FLOAT6_E2M3 / _E3M2) on one GPU.

The ways to a reduced bucket are interleaved round by round in one process so
that drift and neighbours hit all alike (the method of scripts/ab_wide_mx4.py:
device events around `inner` back-to-back calls, `inner` sized per row from a
first timing of (a8); medians with the 25th / 75th percentiles over the rounds):
  (a8) nbxReduceMultiWideMx into MX e4m3, (a4) into MXFP4 — the kernels the
       library had before MXFP6, untouched by it,
  (b2) the same call into E2M3, (b3) into E3M2,
  (c)  what a caller writes without it: nbxReduceMultiWide into fp32, then a
       torch quantise-and-pack pass over the fp32 buffer: per-block amax of the
       magnitude bits, the scale from its exponent field, multiply, round half
       to even on the type's grid, saturate, the code by table, the sign, four
       codes into three bytes, and the scale bytes (E2M3).
Rows: 8 bf16 sources at 1 Mi / 16 Mi / 128 Mi elements; then 8 MXFP6 sources
into the same type, (b2) and (b3) alone.

  python scripts/ab_wide_mx6.py [--rounds 15] [--out profiles/r17/ab_wide_mx6_mi355x.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32, BF16, E4M3, FP4, E2M3, E3M2 = 7, 9, 10, 32, 33, 34


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--window", type=float, default=0.05, help="seconds of (a8) per timed window")
    ap.add_argument("--max-elts", type=int, default=128 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "ab_wide_mx6_mi355x.txt"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import _load_package
    if not torch.cuda.is_available():
        sys.exit("ab_wide_mx6: no GPU; this script measures, it has no CPU form")
    nbx = _load_package()
    nbx.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    op = nbx.DevRedOpFull()
    grid = torch.tensor([m / 8 for m in range(8)] + [(1 + m / 8) * 2.0 ** (e - 1) for e in (1, 2, 3) for m in range(8)],
                        dtype=torch.float32, device="cuda")   # E2M3's 32 magnitudes

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / inner

    def torch_quantise(acc, packed, scales):
        v = acc.view(-1, 32)
        s = (((v.view(torch.int32) & 0x7FFFFFFF).amax(dim=1) >> 23) - 2).clamp_(min=0)
        x = v * ((254 - s) << 23).view(torch.float32)[:, None]
        a = x.abs()
        e = ((a.view(torch.int32) >> 23) - 127).clamp_(min=0)            # the grid's exponent: subnormals share e = 0
        step = ((e - 3 + 127) << 23).view(torch.float32)
        q = (torch.round(a / step) * step).clamp_(max=7.5)               # torch.round: half to even
        c = torch.bucketize(q, grid).to(torch.int32) | (torch.signbit(x).to(torch.int32) << 5)
        c = c.view(-1, 4)
        packed.view(-1, 3).copy_(torch.stack([c[:, 0] | c[:, 1] << 6, c[:, 1] >> 2 | c[:, 2] << 4,
                                              c[:, 2] >> 4 | c[:, 3] << 2], dim=1).to(torch.uint8))
        scales.copy_(s.to(torch.uint8))

    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median [p25, p75] over {args.rounds} interleaved rounds",
             f"# {'row':24s}{'inner':>6s} {'(a8) MX e4m3':>22s} {'(a4) MXFP4':>22s} {'(b2) E2M3':>22s} {'(b3) E3M2':>22s} "
             f"{'(c) fp32 + torch E2M3':>24s}  b2/a8 b2/a4 b2/c"]
    gen = torch.Generator(device="cuda").manual_seed(1)
    rand8 = lambda n, hi: torch.randint(0, hi, (n,), dtype=torch.uint8, device="cuda", generator=gen)

    for tname in ("bf16", "mxfp6"):
        for n in (1 << 20, 16 << 20, 128 << 20):
            if n > args.max_elts:
                continue
            nsrc, nb = 8, n // 32
            out8 = torch.empty(n, dtype=torch.uint8, device="cuda")      # every destination fits in n bytes
            scales = torch.empty(nb, dtype=torch.uint8, device="cuda")
            dp, sp = [out8.data_ptr()], [scales.data_ptr()]
            if tname == "bf16":
                acc = torch.empty(n, dtype=torch.float32, device="cuda")
                packed = torch.empty(n // 4 * 3, dtype=torch.uint8, device="cuda")
                srcs = [torch.randint(0, 0x4000, (n,), dtype=torch.int16, device="cuda", generator=gen)
                        for _ in range(nsrc)]   # finite codes
                ptrs = [s.data_ptr() for s in srcs]
                mx = lambda dt: (lambda: nbx.reduce_multi_wide_mx(dp, sp, ptrs, None, n, BF16, dt, op, 0, stream))
                fns = {"a8": mx(E4M3), "a4": mx(FP4), "b2": mx(E2M3), "b3": mx(E3M2),
                       "c": lambda: (nbx.reduce_multi_wide([acc.data_ptr()], ptrs, n, BF16, F32, op, 0, stream),
                                     torch_quantise(acc, packed, scales))}
            else:
                srcs = [rand8(n // 4 * 3, 256) for _ in range(nsrc)]
                sscales = [rand8(nb, 4) + 125 for _ in range(nsrc)]      # 2^-2 .. 2^1
                ptrs, ssp = [s.data_ptr() for s in srcs], [e.data_ptr() for e in sscales]
                mx = lambda t: (lambda: nbx.reduce_multi_wide_mx(dp, sp, ptrs, ssp, n, t, t, op, 0, stream))
                fns = {"b2": mx(E2M3), "b3": mx(E3M2)}
            for fn in fns.values():   # warm every shape
                fn()
            torch.cuda.synchronize()
            inner = int(min(10000, max(3, args.window * 1e6 / timed(next(iter(fns.values())), 10))))
            t = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k, fn in fns.items():
                    t[k].append(timed(fn, inner if k != "c" else max(1, inner // 8)))
            q = {k: np.percentile(v, [50, 25, 75]) for k, v in t.items()}
            cell = lambda k: (f"{q[k][0]:9.1f} [{q[k][1]:.1f}, {q[k][2]:.1f}]" if k in q else "-").rjust(22)
            ratio = lambda k: f"{q['b2'][0] / q[k][0]:.3f}" if k in q else "  -  "
            lines.append(f"{tname + ' ' + str(nsrc) + ' src ' + str(n >> 20) + ' Mi':26s}{inner:6d} {cell('a8')} {cell('a4')} "
                         f"{cell('b2')} {cell('b3')} {cell('c')}    {ratio('a8')} {ratio('a4')} {ratio('c')}")
            print(lines[-1], flush=True)
            del srcs, out8, scales
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
