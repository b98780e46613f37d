#!/usr/bin/env python3
"""A/B of the MXFP4 block-scaled sum (nbxReduceMultiWideMx, NBX_FLOAT4_E2M1) on one GPU.

Three ways to a reduced bucket, interleaved round by round in one process so
that drift and neighbours hit all alike (the method of scripts/ab_wide_mx.py:
device events around `inner` back-to-back calls, `inner` sized per row from a
first timing of (a); medians with the 25th / 75th percentiles over the rounds):
  (a) nbxReduceMultiWideMx into MX e4m3 — the path the library had before
      MXFP4; for the MXFP4 rows its sources are MX e4m3 (1 B / element), the
      nearest it could read,
  (b) the same call into MXFP4 (for the MXFP4 rows: MXFP4 into MXFP4),
  (c) what a caller writes without it: nbxReduceMultiWide into fp32 (MXFP4
      rows: a torch decode-scale-add of the packed sources into fp32), then a
      torch quantise-to-MXFP4 pass over the fp32 buffer: per-block amax of the
      magnitude bits, the scale from its exponent field, multiply, seven
      compares, sign, pack two codes per byte, and the scale bytes.
Rows: bf16 / MXFP4 sources, 2 / 8 sources, 1 Mi / 16 Mi / 128 Mi elements.

  python scripts/ab_wide_mx4.py [--rounds 15] [--out profiles/r15/ab_wide_mx4_mi355x.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32, BF16, E4M3, FP4 = 7, 9, 10, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--window", type=float, default=0.05, help="seconds of (a) per timed window")
    ap.add_argument("--max-elts", type=int, default=128 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "ab_wide_mx4_mi355x.txt"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import _load_package
    if not torch.cuda.is_available():
        sys.exit("ab_wide_mx4: no GPU; this script measures, it has no CPU form")
    nbx = _load_package()
    nbx.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    op = nbx.DevRedOpFull()
    lut = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float32, device="cuda")

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / inner

    def torch_decode_sum(acc, srcs, sscales):
        for k, (b, e) in enumerate(zip(srcs, sscales)):
            codes = torch.stack([b & 15, b >> 4], dim=1).view(-1, 32).long()
            v = lut[codes] * (e.to(torch.int32) << 23).view(torch.float32)[:, None]   # scale bytes in [1, 254] here
            acc.view(-1, 32).copy_(v) if k == 0 else acc.view(-1, 32).add_(v)

    def torch_quantise(acc, packed, scales):
        v = acc.view(-1, 32)
        s = (((v.view(torch.int32) & 0x7FFFFFFF).amax(dim=1) >> 23) - 2).clamp_(min=0)
        x = v * ((254 - s) << 23).view(torch.float32)[:, None]
        a = x.abs()
        code = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
        code |= torch.signbit(x).to(torch.uint8) << 3
        packed.copy_((code[:, 0::2] | (code[:, 1::2] << 4)).view(-1))
        scales.copy_(s.to(torch.uint8))

    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median [p25, p75] over {args.rounds} interleaved rounds",
             f"# {'row':26s}{'inner':>6s} {'(a) into MX e4m3':>22s} {'(b) into MXFP4':>22s} {'(c) fp32 + torch MXFP4':>24s}  b/a   b/c"]
    gen = torch.Generator(device="cuda").manual_seed(1)
    rand8 = lambda n, hi: torch.randint(0, hi, (n,), dtype=torch.uint8, device="cuda", generator=gen)

    for tname in ("bf16", "mxfp4"):
        for n in (1 << 20, 16 << 20, 128 << 20):
            if n > args.max_elts:
                continue
            for nsrc in (2, 8):
                nb = n // 32
                codes8 = torch.empty(n, dtype=torch.uint8, device="cuda")
                packed = torch.empty(n // 2, dtype=torch.uint8, device="cuda")
                scales = torch.empty(nb, dtype=torch.uint8, device="cuda")
                acc = torch.empty(n, dtype=torch.float32, device="cuda")
                dp, pp, sp = [codes8.data_ptr()], [packed.data_ptr()], [scales.data_ptr()]
                if tname == "bf16":
                    srcs = [torch.randint(0, 0x4000, (n,), dtype=torch.int16, device="cuda", generator=gen)
                            for _ in range(nsrc)]   # finite codes
                    ptrs = [s.data_ptr() for s in srcs]
                    a = lambda: nbx.reduce_multi_wide_mx(dp, sp, ptrs, None, n, BF16, E4M3, op, 0, stream)
                    b = lambda: nbx.reduce_multi_wide_mx(pp, sp, ptrs, None, n, BF16, FP4, op, 0, stream)
                    c = lambda: (nbx.reduce_multi_wide([acc.data_ptr()], ptrs, n, BF16, F32, op, 0, stream),
                                 torch_quantise(acc, packed, scales))
                else:
                    srcs = [rand8(n // 2, 256) for _ in range(nsrc)]
                    srcs8 = [rand8(n, 0x70) for _ in range(nsrc)]          # finite e4m3 codes for (a)
                    sscales = [rand8(nb, 4) + 125 for _ in range(nsrc)]    # 2^-2 .. 2^1
                    ptrs, ptrs8 = [s.data_ptr() for s in srcs], [s.data_ptr() for s in srcs8]
                    ssp = [e.data_ptr() for e in sscales]
                    a = lambda: nbx.reduce_multi_wide_mx(dp, sp, ptrs8, ssp, n, E4M3, E4M3, op, 0, stream)
                    b = lambda: nbx.reduce_multi_wide_mx(pp, sp, ptrs, ssp, n, FP4, FP4, op, 0, stream)
                    c = lambda: (torch_decode_sum(acc, srcs, sscales), torch_quantise(acc, packed, scales))
                for fn in (a, b, c):   # warm every shape
                    fn()
                torch.cuda.synchronize()
                inner = int(min(10000, max(3, args.window * 1e6 / timed(a, 10))))
                t = {k: [] for k in "abc"}
                for _ in range(args.rounds):
                    for k, fn in zip("abc", (a, b, c)):
                        t[k].append(timed(fn, inner if k != "c" else max(1, inner // 8)))
                q = {k: np.percentile(v, [50, 25, 75]) for k, v in t.items()}
                cell = lambda k: f"{q[k][0]:9.1f} [{q[k][1]:.1f}, {q[k][2]:.1f}]".rjust(22)
                lines.append(f"{tname + ' ' + str(nsrc) + ' src ' + str(n >> 20) + ' Mi':28s}{inner:6d} {cell('a')} "
                             f"{cell('b')} {cell('c')}    {q['b'][0] / q['a'][0]:.3f} {q['b'][0] / q['c'][0]:.3f}")
                print(lines[-1], flush=True)
                del srcs, acc, codes8, packed, scales
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
