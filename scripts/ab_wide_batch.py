#!/usr/bin/env python3
"""ab_wide_batch.py — in-process A/B of nbxReduceMultiWideBatch against one
nbxReduceMultiWide call per bucket, on config C's bucket sets:
128 x 64 KiB and 64 x 256 KiB per input, 8 sources, bf16 -> bf16, bf16 -> fp32
and fp8 e4m3 -> fp32, and a sweep of eight 4-source bf16 buckets across the
size at which the batched call hands a bucket to the single-bucket kernel
(wideUnroll(4) x 256 x CUs packs). One process, one stream, the contestants
    single  one nbxReduceMultiWide call per bucket (ctypes arguments prebuilt)
    batch   one nbxReduceMultiWideBatch call
    step    one nbxReduceMultiBatch call on fp16 buckets of the same bytes:
            the rate a per-step work-list launch reaches on the same traffic
alternate per round; HIP events around enough back-to-back repetitions for
0.5 s of work, after a warm-up of every shape; the median over the rounds is
reported as algorithmic GB/s (source bytes + destination bytes written) with
the round-to-round spread (max - min); `host_us` is the host's time to enqueue
one repetition into an empty queue (five after a synchronize): a contestant
whose host_us reaches its us is bound by the host, not the kernel. The outputs of single and batch are compared byte for
byte. In the sweep the batch contestant runs under launch
variant 1, which keeps every bucket in the batch, so the crossover against the
single-bucket kernel shows; `policy` says what the default rule would do.
usage: ab_wide_batch.py [--rounds R] [--seconds S] [--out FILE.txt]"""
import ctypes
import importlib.util
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, F32, BF16, E4M3 = 6, 7, 9, 10
ESZ = {F16: 2, F32: 4, BF16: 2, E4M3: 1}
NAME = {F16: "f16", F32: "fp32", BF16: "bf16", E4M3: "e4m3"}


def load_package():
    pkg = os.path.join(ROOT, "neuronabox-nccl_amd")
    spec = importlib.util.spec_from_file_location("neuronabox_nccl_amd", os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["neuronabox_nccl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def finite_codes(nbytes, st, gen):
    if st == E4M3:
        return torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=gen) & 0x77
    t = torch.rand(nbytes // 2, device="cuda", generator=gen)
    return t.to({F16: torch.float16, BF16: torch.bfloat16}[st]).view(torch.uint8)


def main():
    argv = sys.argv[1:]
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 5
    seconds = float(argv[argv.index("--seconds") + 1]) if "--seconds" in argv else 0.5
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    nbx = load_package()
    lib = nbx.load_library()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    op = nbx.DevRedOpFull()
    gen = torch.Generator(device="cuda").manual_seed(11)
    threshold = 4 * 256 * cus * 16   # bytes per source of a 4-source bucket that runs alone
    shapes = []
    for st, dt in ((BF16, BF16), (BF16, F32), (E4M3, F32)):
        for nb, kib in ((128, 64), (64, 256)):
            shapes.append((f"{nb} x {kib} KiB", st, dt, 8, nb, kib << 10, 0))
    for num, den in ((1, 8), (1, 4), (1, 2), (1, 1), (2, 1)):
        shapes.append((f"sweep 8 x {num}/{den} threshold", BF16, BF16, 4, 8, threshold * num // den, 1))
    lines = [f"# {torch.cuda.get_device_name(0)}, {cus} CUs, rounds {rounds}, >= {seconds} s per timing; "
             f"4-source single-bucket threshold {threshold >> 10} KiB per source"]
    print(lines[0], flush=True)
    for label, st, dt, nsrc, nb, nbytes, variant in shapes:
        n = nbytes // ESZ[st]
        srcs = [[finite_codes(nbytes, st, gen) for _ in range(nsrc)] for _ in range(nb)]
        outs = {k: [torch.empty(n * ESZ[dt], dtype=torch.uint8, device="cuda") for _ in range(nb)]
                for k in ("single", "batch", "step")}
        def buckets(k):
            return [([o.data_ptr()], [t.data_ptr() for t in ss], n) for ss, o in zip(srcs, outs[k])]
        single_args = []
        for d, s, c in buckets("single"):
            da = (ctypes.c_void_p * 1)(ctypes.c_void_p(d[0]))
            sa = (ctypes.c_void_p * nsrc)(*[ctypes.c_void_p(x) for x in s])
            single_args.append((da, sa))
        btasks, _keep_b = nbx._reduce_tasks(buckets("batch"))
        n16 = nbytes // 2   # fp16 elements of the same bytes
        stasks, _keep_s = nbx._reduce_tasks([(d, s, n16) for d, s, _ in buckets("step")])
        shp = ctypes.c_void_p(sh)

        def run_single():
            for da, sa in single_args:
                lib.nbxReduceMultiWide(da, 1, sa, nsrc, n, st, dt, op, 0, shp)

        def run_batch():
            if variant:
                nbx.set_launch_config(0, variant)
            lib.nbxReduceMultiWideBatch(btasks, nb, st, dt, op, 0, shp)
            if variant:
                nbx.set_launch_config(0, 0)

        def run_step():
            lib.nbxReduceMultiBatch(stasks, nb, F16, op, 0, 0, shp)

        calls = {"single": run_single, "batch": run_batch, "step": run_step}
        reps, host = {}, {}
        for k, f in calls.items():   # warm-up of every shape, and the repetition count for `seconds` of work
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            for _ in range(5):
                f()
            host[k] = (time.perf_counter() - t0) / 5   # into an empty queue: the host's own cost per repetition
            e1.record(stream)
            torch.cuda.synchronize()
            reps[k] = max(5, int(seconds / (e0.elapsed_time(e1) * 1e-3 / 5)) + 1)
        nbx.launch_log_reset()
        run_batch()
        records = nbx.launch_log()[1]
        torch.cuda.synchronize()
        equal = all(torch.equal(a, b) for a, b in zip(outs["single"], outs["batch"]))
        times = {k: [] for k in calls}
        for _ in range(rounds):
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(reps[k]):
                    f()
                e1.record(stream)
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / reps[k])
        row = {"shape": label, "types": f"{NAME[st]} -> {NAME[dt]}", "nsrc": nsrc, "KiB_per_input": nbytes >> 10,
               "outputs_equal": equal, "batch_launches": [list(r) for r in records]}
        if variant:
            row["policy"] = "runs alone" if nbytes >= threshold else "batched"
        for k in calls:
            dst_bytes = nbytes if k == "step" else n * ESZ[dt]
            alg = nb * (nsrc * nbytes + dst_bytes)
            rates = sorted(alg / (ms * 1e-3) / 1e9 for ms in times[k])
            row[k] = {"us": round(sorted(times[k])[len(times[k]) // 2] * 1e3, 1), "GBps": round(rates[len(rates) // 2], 1),
                      "spread_GBps": round(rates[-1] - rates[0], 1), "reps": reps[k],
                      "host_us": round(host[k] * 1e6, 1)}
        row["batch_over_single"] = round(row["batch"]["GBps"] / row["single"]["GBps"], 2)
        line = json.dumps(row)
        print(line, flush=True)
        lines.append(line)
        del srcs, outs
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
