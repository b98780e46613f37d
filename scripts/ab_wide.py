#!/usr/bin/env python3
"""ab_wide.py — in-process A/B of the fp32-accumulating sum (nbxReduceMultiWide)
against the per-step sum (nbxReduceMulti) on the configs' single-bucket
shapes: f16 / bf16 at 256 MiB per input, fp8 e4m3 / e5m2 at 128 MiB, 8 and 2
sources. One process, same source buffers, one output buffer and one stream;
the contestants
    step    nbxReduceMulti Sum (rounds to the element type after every source)
    wide    nbxReduceMultiWide, output of the source type
    wide32  nbxReduceMultiWide, fp32 output
alternate per round; HIP events around 10 back-to-back calls after a warm-up
of every shape; the median over the rounds is reported as algorithmic GB/s
(source bytes + destination bytes actually written), with the per-step
contestant's round-to-round spread (max - min rate). Every contestant's output
is compared bit for bit against the CPU oracle's fold on a sample (the first
and last 32 Ki elements), so a fast wrong kernel shows.
Acceptance (8-source shapes): the wide rate may not fall below the step rate
by more than the step contestant's own spread.
--bpc 1,3 adds the wide contestant at those workgroups-per-CU knobs
(nbxSetLaunchConfig) as "wide@bpcN"; --mib M overrides the size per input.
usage: ab_wide.py [--rounds R] [--cases bf16,f16,fp8e4m3,fp8e5m2] [--nsrc 8,2] [--bpc 1,3] [--mib M]
                  [--out FILE.jsonl]"""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402  (checker only)

CASES = {"f16": (6, 2, 256), "bf16": (9, 2, 256), "fp8e4m3": (10, 1, 128), "fp8e5m2": (11, 1, 128)}
SAMPLE = 32768


def load_package():
    pkg = os.path.join(ROOT, "neuronabox-nccl_amd")
    spec = importlib.util.spec_from_file_location("neuronabox_nccl_amd", os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["neuronabox_nccl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def widen_table(dt):
    dec = {6: oracle.f16_to_f32, 9: oracle.bf16_to_f32, 10: oracle.e4m3_to_f32, 11: oracle.e5m2_to_f32}[dt]
    return np.array([dec(c) for c in range(256 if dt >= 10 else 65536)], dtype=np.float32)


def narrow(f, dt):
    enc = {6: oracle.f32_to_f16, 9: oracle.f32_to_bf16, 10: oracle.f32_to_e4m3, 11: oracle.f32_to_e5m2}[dt]
    bits, inv = np.unique(f.view(np.uint32), return_inverse=True)
    return np.array([enc(float(v)) for v in bits.view(np.float32)], dtype=oracle.NP_STORAGE[dt])[inv.reshape(-1)]


def sample_of(t, esz, n):
    """First and last SAMPLE elements of a device byte buffer holding n elements."""
    k = min(SAMPLE, n // 2)
    return torch.cat([t[:k * esz], t[(n - k) * esz:n * esz]]).cpu().numpy()


def main():
    argv = sys.argv[1:]
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 5
    names = argv[argv.index("--cases") + 1].split(",") if "--cases" in argv else list(CASES)
    nsrcs = [int(x) for x in argv[argv.index("--nsrc") + 1].split(",")] if "--nsrc" in argv else [8, 2]
    bpcs = [int(x) for x in argv[argv.index("--bpc") + 1].split(",")] if "--bpc" in argv else []
    mib_override = int(argv[argv.index("--mib") + 1]) if "--mib" in argv else 0
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    nbx = load_package()
    nbx.load_library()
    oracle.build()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    op = nbx.DevRedOpFull()
    lines = []
    for name in names:
        dt, esz, mib = CASES[name]
        mib = mib_override or mib
        nbytes = mib << 20
        n = nbytes // esz
        g = torch.Generator(device="cuda").manual_seed(5)
        npst = oracle.NP_STORAGE[dt]
        srcs = []
        for _ in range(max(nsrcs)):
            if dt in (6, 9):
                b = torch.rand(n, device="cuda", generator=g).to({6: torch.float16, 9: torch.bfloat16}[dt]).view(
                    torch.uint8)
            else:
                b = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g)
                b &= 0x77   # finite codes
            srcs.append(b)
        # one output buffer for every contestant (its placement alone moves rates), sized for fp32
        out = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
        tab = widen_table(dt)
        for nsrc in nsrcs:
            sp = [t.data_ptr() for t in srcs[:nsrc]]
            host = [sample_of(t, esz, n).view(npst) for t in srcs[:nsrc]]
            fold = oracle.reduce_multi([tab[h] for h in host], 7, 0, threads=8)[0]
            want = {"step": oracle.reduce_multi(host, dt, 0, threads=8)[0], "wide": narrow(fold, dt), "wide32": fold}
            calls = {
                "step": lambda: nbx.reduce_multi_raw([out.data_ptr()], sp, n, dt, op, 0, False, sh),
                "wide": lambda: nbx.reduce_multi_wide_raw([out.data_ptr()], sp, n, dt, dt, op, 0, sh),
                "wide32": lambda: nbx.reduce_multi_wide_raw([out.data_ptr()], sp, n, dt, 7, op, 0, sh),
            }
            out_esz = {"step": esz, "wide": esz, "wide32": 4}

            def at_bpc(b, f=calls["wide"]):
                nbx.set_launch_config(b, 0)
                try:
                    return f()
                finally:
                    nbx.set_launch_config(0, 0)

            for b in bpcs:
                calls[f"wide@bpc{b}"] = (lambda b=b: at_bpc(b))
                want[f"wide@bpc{b}"] = want["wide"]
                out_esz[f"wide@bpc{b}"] = esz
            times = {k: [] for k in calls}
            ok = {}
            for k, f in calls.items():   # warm-up of every shape, and the correctness sample
                out.fill_(0xA5)
                for _ in range(3):
                    assert f() == 0
                torch.cuda.synchronize()
                got = sample_of(out, out_esz[k], n)
                ok[k] = bool(np.array_equal(got, want[k].view(np.uint8)))
            for _ in range(rounds):
                for k, f in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(10):
                        f()
                    e1.record(stream)
                    torch.cuda.synchronize()
                    times[k].append(e0.elapsed_time(e1) / 10)
            row = {"case": name, "MiB_per_input": mib, "nsrc": nsrc, "rounds": rounds,
                   "device": torch.cuda.get_device_name(0)}
            for k in calls:
                alg = nsrc * nbytes + n * out_esz[k]
                rates = sorted(alg / (ms * 1e-3) / 1e9 for ms in times[k])
                ms = sorted(times[k])[len(times[k]) // 2]
                row[k] = {"ms": round(ms, 4), "GBps": round(rates[len(rates) // 2], 1),
                          "spread_GBps": round(rates[-1] - rates[0], 1), "sample_exact": ok[k]}
            if nsrc == 8:
                row["accept"] = bool(row["wide"]["GBps"] >= row["step"]["GBps"] - row["step"]["spread_GBps"])
            line = json.dumps(row)
            print(line, flush=True)
            lines.append(line)
        del srcs, out
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
