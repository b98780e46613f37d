#!/usr/bin/env python3
"""ab_elts.py — time the per-step element kernel (kReduceElts): nbxReduceMulti
Sum with two destinations on different offsets modulo 16 (the second one
element past a 256-byte boundary) and source k at ((3k + 1) * eb) % 16 past
one, 8 Mi elements, f32 / f16 / fp8 e4m3 / int32, 2 and 8 sources. One process,
one stream; per case a launch record, three warm-up calls, then 7 timings of 10
back-to-back calls between HIP events; prints and writes one JSON line per
case with the median in us. It times the library NBX_LIB names (the built one
otherwise): to compare two builds run it once per build and process,
alternating, and compare the medians over the rounds (profiles/r12).
usage: [NBX_LIB=path/libnbxccl.so] ab_elts.py OUT.jsonl"""
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ESZ = {7: 4, 6: 2, 10: 1, 2: 4}   # f32, f16, e4m3, int32
NAME = {7: "f32", 6: "f16", 10: "e4m3", 2: "int32"}


def load_package():
    pkg = os.path.join(ROOT, "neuronabox-nccl_amd")
    spec = importlib.util.spec_from_file_location("neuronabox_nccl_amd", os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["neuronabox_nccl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    out_path = sys.argv[1]
    nbx = load_package()
    nbx.load_library()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    n = 8 << 20
    lines = []
    for dt in (7, 6, 10, 2):
        eb = ESZ[dt]
        bufs = [torch.randint(0, 120, (n * eb + 512,), dtype=torch.uint8, device="cuda") for _ in range(8)]
        outs = [torch.empty(n * eb + 512, dtype=torch.uint8, device="cuda") for _ in range(2)]
        op = nbx.host_to_dev_redop(nbx.ncclRedOp.ncclSum, dt, 1)
        for nsrc in (2, 8):
            srcs = [b.data_ptr() + 256 + ((3 * k + 1) * eb) % 16 for k, b in enumerate(bufs[:nsrc])]
            dsts = [outs[0].data_ptr() + 256, outs[1].data_ptr() + 256 + eb]

            def run():
                nbx.reduce_multi(dsts, srcs, n, dt, op, 0, False, stream.cuda_stream)
            nbx.launch_log_reset()
            run()
            recs = nbx.launch_log()[1]
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            ts = []
            for _ in range(7):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(10):
                    run()
                e1.record(stream)
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) / 10 * 1e3)
            ts.sort()
            line = json.dumps({"type": NAME[dt], "nsrc": nsrc, "elements": n, "family": [r[0] for r in recs],
                               "elts": {"us": round(ts[len(ts) // 2], 2)}})
            print(line, flush=True)
            lines.append(line)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
