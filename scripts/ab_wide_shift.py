#!/usr/bin/env python3
"""ab_wide_shift.py — in-process A/B of nbxReduceMultiWide's realigning kernel
(kWideShiftedLds, launch family 16) against the element kernel it replaces and
the pack kernel it cannot reach. For each source type, both
outputs and 2 / 4 / 8 sources, three contestants on the same bytes:
    elts    the realigning layout (source k at ((3k + 1) * eb) % 16 past a
            256-byte boundary, the destination aligned: a reduce-scatter block
            of a count that is no multiple of a pack) with the threshold out of
            reach: the element kernel, what every such call ran before
    shift   the same call with the threshold at 1: kWideShiftedLds
    packs   the same buffers read from their aligned start: kWidePacks, the ceiling
Sizes: 256 MiB and 4 MiB per input, and a sweep of 4 Ki .. 4 Mi elements (every
power of two) for the crossover between elts and shift. One process, one
stream; the contestants alternate per round; HIP events around enough
back-to-back calls for `--seconds` of work (`--sweep-seconds` in the sweep),
after a warm-up of every shape; reported are the median over the rounds in us
and as algorithmic GB/s (source bytes + destination bytes written) and the
round-to-round spread (max - min). Each contestant's launch record is checked
(families 7, 16, 6) and the outputs of elts and shift are compared byte for
byte. The last lines derive the default threshold: the smallest swept count
from which shift beats elts for every type, output and source count, rounded up
to a power of two and not below 4,096.
usage: ab_wide_shift.py [--part big|mid|sweep|all] [--types f16,bf16,e4m3,e5m2] [--rounds R] [--seconds S]
                        [--sweep-seconds S] [--out FILE.txt]"""
import ctypes
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, F32, BF16, E4M3, E5M2 = 6, 7, 9, 10, 11
ESZ = {F16: 2, F32: 4, BF16: 2, E4M3: 1, E5M2: 1}
NAME = {F16: "f16", F32: "fp32", BF16: "bf16", E4M3: "e4m3", E5M2: "e5m2"}
FAMILY = {"elts": 7, "shift": 16, "packs": 6}
NSRCS = (2, 4, 8)
BIG, MID = 256 << 20, 4 << 20
SWEEP = [1 << k for k in range(12, 23)]   # elements
OUT_OF_REACH = 1 << 62


def load_package():
    pkg = os.path.join(ROOT, "neuronabox-nccl_amd")
    spec = importlib.util.spec_from_file_location("neuronabox_nccl_amd", os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["neuronabox_nccl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def finite_codes(nbytes, st, gen):
    """Random codes without inf / NaN (a cleared exponent bit), so that no contestant's time depends on them."""
    t = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=gen)
    if ESZ[st] == 1:
        return t & 0x77
    t[1::2] &= 0xBF   # the high byte of a little-endian 16-bit code
    return t


def arg(argv, name, default, conv=str):
    return conv(argv[argv.index(name) + 1]) if name in argv else default


def main():
    argv = sys.argv[1:]
    part = arg(argv, "--part", "all")
    types = [{v: k for k, v in NAME.items()}[t] for t in arg(argv, "--types", "f16,bf16,e4m3,e5m2").split(",")]
    rounds = arg(argv, "--rounds", 5, int)
    seconds = arg(argv, "--seconds", 0.25, float)
    sweep_seconds = arg(argv, "--sweep-seconds", 0.05, float)
    out_path = arg(argv, "--out", None)
    nbx = load_package()
    lib = nbx.load_library()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    shp = ctypes.c_void_p(stream.cuda_stream)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    op = nbx.DevRedOpFull()
    gen = torch.Generator(device="cuda").manual_seed(17)
    saved = nbx.set_wide_shift_min_elts(0)
    lines = [f"# {torch.cuda.get_device_name(0)}, {cus} CUs, rounds {rounds}, >= {seconds} s per timing "
             f"({sweep_seconds} s in the sweep), part {part}, library default threshold {saved}"]
    print(lines[0], flush=True)
    sizes = []   # (label, elements or None, bytes per input or None, seconds)
    if part in ("big", "all"):
        sizes.append(("256 MiB", None, BIG, seconds))
    if part in ("mid", "all"):
        sizes.append(("4 MiB", None, MID, seconds))
    if part in ("sweep", "all"):
        sizes += [(f"sweep {n >> 10} Ki", n, None, sweep_seconds) for n in SWEEP]
    wins = {}   # swept count -> [shift beats elts, per configuration]
    for st in types:
        eb = ESZ[st]
        cap = max(b if b else n * eb for _, n, b, _ in sizes)   # bytes per input
        bufs = [finite_codes(cap + 512, st, gen) for _ in range(max(NSRCS))]
        assert all(b.data_ptr() % 256 == 0 for b in bufs)
        outs = {k: torch.empty(cap // eb * 4 + 512, dtype=torch.uint8, device="cuda") for k in ("elts", "other")}
        for dt in (st, F32):
            deb = ESZ[dt]
            for nsrc in NSRCS:
                offs = [((3 * k + 1) * eb) % 16 for k in range(nsrc)]
                ptrs = {"elts": [b.data_ptr() + 256 + o for b, o in zip(bufs, offs)],
                        "packs": [b.data_ptr() + 256 for b in bufs[:nsrc]]}
                ptrs["shift"] = ptrs["elts"]
                sa = {k: (ctypes.c_void_p * nsrc)(*[ctypes.c_void_p(x) for x in v]) for k, v in ptrs.items()}
                da = {k: (ctypes.c_void_p * 1)(ctypes.c_void_p(outs["elts" if k == "elts" else "other"].data_ptr()))
                      for k in FAMILY}
                for label, n, nbytes, secs in sizes:
                    if n is None:
                        n = nbytes // eb
                    calls = {}
                    for k in FAMILY:
                        def run(k=k):
                            if k != "packs":
                                lib.nbxDebugSetWideShiftMinElts(OUT_OF_REACH if k == "elts" else 1)
                            rc = lib.nbxReduceMultiWide(da[k], 1, sa[k], nsrc, n, st, dt, op, 0, shp)
                            assert rc == 0, rc
                        calls[k] = run
                    reps = {}
                    for k, f in calls.items():   # warm-up, the launch record, the repetition count
                        nbx.launch_log_reset()
                        f()
                        recs = nbx.launch_log()[1]
                        assert [r[0] for r in recs] == [FAMILY[k]], (k, recs)
                        f()
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        for _ in range(3):
                            f()
                        e1.record(stream)
                        torch.cuda.synchronize()
                        reps[k] = max(5, int(secs / (e0.elapsed_time(e1) * 1e-3 / 3)) + 1)
                    calls["elts"]()
                    calls["shift"]()   # "other" now holds shift's output
                    torch.cuda.synchronize()
                    equal = torch.equal(outs["elts"][:n * deb], outs["other"][:n * deb])
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
                    alg = nsrc * n * eb + n * deb
                    row = {"size": label, "types": f"{NAME[st]} -> {NAME[dt]}", "nsrc": nsrc, "elements": n,
                           "outputs_equal": equal}
                    for k in calls:
                        rates = sorted(alg / (ms * 1e-3) / 1e9 for ms in times[k])
                        row[k] = {"us": round(sorted(times[k])[len(times[k]) // 2] * 1e3, 2),
                                  "GBps": round(rates[len(rates) // 2], 1), "spread_GBps": round(rates[-1] - rates[0], 1),
                                  "reps": reps[k]}
                    row["shift_over_elts"] = round(row["elts"]["us"] / row["shift"]["us"], 2)
                    row["shift_over_packs"] = round(row["packs"]["us"] / row["shift"]["us"], 2)
                    if label.startswith("sweep"):
                        wins.setdefault(n, []).append(row["shift"]["us"] < row["elts"]["us"])
                    line = json.dumps(row)
                    print(line, flush=True)
                    lines.append(line)
        del bufs, outs
        torch.cuda.empty_cache()
    nbx.set_wide_shift_min_elts(saved)
    if wins:
        counts = sorted(wins)
        crossover = None
        for n in reversed(counts):
            if not all(wins[n]):
                break
            crossover = n
        lines.append("# shift beats elts in every configuration at: " + ", ".join(str(n) for n in counts if all(wins[n])))
        if crossover is None:
            lines.append("# no swept count from which shift beats elts everywhere")
        else:
            default = max(4096, 1 << (crossover - 1).bit_length())
            note = " (the smallest swept count: the crossover lies at or below it)" if crossover == counts[0] else ""
            lines.append(f"# crossover {crossover} elements{note}; default threshold {default}")
        for l in lines[-2:]:
            print(l, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
