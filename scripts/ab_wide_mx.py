#!/usr/bin/env python3
"""A/B of the MXFP8 block-scaled sum (nbxReduceMultiWideMx) on one GPU.

Three ways to a reduced bucket, interleaved round by round in one process so
that drift and neighbours hit all alike (the method of scripts/ab_wide_stats.py:
device events around `inner` back-to-back calls, `inner` sized per row from a
first timing of (a); medians with the 25th / 75th percentiles over the rounds):
  (a) nbxReduceMultiWide into fp32 (no quantisation: the 4 B / element store),
  (b) nbxReduceMultiWideMx into MX e4m3,
  (c) (a), then the quantise pass a caller writes today in torch over the fp32
      buffer: per-block amax, the scale from its exponent field, multiply,
      clamp, cast to float8_e4m3fn, and the scale bytes.
Rows: bf16 / e4m3 sources, 2 / 8 sources, 1 Mi / 16 Mi / 128 Mi elements.

  python scripts/ab_wide_mx.py [--rounds 15] [--out profiles/r14/ab_wide_mx_mi355x.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "ab_wide_mx_mi355x.txt"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import _load_package
    if not torch.cuda.is_available():
        sys.exit("ab_wide_mx: no GPU; this script measures, it has no CPU form")
    nbx = _load_package()
    nbx.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    op = nbx.DevRedOpFull()

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / inner

    def torch_quantise(acc, codes, scales):
        v = acc.view(-1, 32)
        s = ((v.abs().amax(dim=1).view(torch.int32) >> 23) - 8).clamp_(min=0)
        r = ((254 - s) << 23).view(torch.float32)
        codes.copy_((v * r[:, None]).clamp_(-448.0, 448.0).to(torch.float8_e4m3fn).view(-1))
        scales.copy_(s.to(torch.uint8))

    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median [p25, p75] over {args.rounds} interleaved rounds",
             f"# {'row':26s}{'inner':>6s} {'(a) wide fp32':>22s} {'(b) wide MX':>22s} {'(c) wide + torch MX':>22s}  b/a   b/c"]
    gen = torch.Generator(device="cuda").manual_seed(1)

    def codes_of(n, eb):   # finite codes
        if eb == 2:
            return torch.randint(0, 0x4000, (n,), dtype=torch.int16, device="cuda", generator=gen).view(torch.uint8)
        return torch.randint(0, 0x70, (n,), dtype=torch.uint8, device="cuda", generator=gen)

    for st, tname, eb in ((BF16, "bf16", 2), (E4M3, "e4m3", 1)):
        for n in (1 << 20, 16 << 20, 128 << 20):
            if n > args.max_elts:
                continue
            for nsrc in (2, 8):
                srcs = [codes_of(n, eb) for _ in range(nsrc)]
                sp = [s.data_ptr() for s in srcs]
                acc = torch.empty(n, dtype=torch.float32, device="cuda")
                codes = torch.empty(n, dtype=torch.float8_e4m3fn, device="cuda")
                scales = torch.empty(n // 32, dtype=torch.uint8, device="cuda")
                a = lambda: nbx.reduce_multi_wide([acc.data_ptr()], sp, n, st, F32, op, 0, stream)
                b = lambda: nbx.reduce_multi_wide_mx([codes.data_ptr()], [scales.data_ptr()], sp, None, n, st, E4M3,
                                                     op, 0, stream)
                c = lambda: (a(), torch_quantise(acc, codes, scales))
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
                lines.append(f"{tname + ' ' + str(nsrc) + ' src ' + str(n >> 20) + ' Mi':28s}{inner:6d} {cell('a')} "
                             f"{cell('b')} {cell('c')}  {q['b'][0] / q['a'][0]:.3f} {q['b'][0] / q['c'][0]:.3f}")
                print(lines[-1], flush=True)
                del srcs, acc, codes, scales
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
