"""nbxReduceMultiWideStats / nbxReduceMultiWideBatchStats on the GPU: the
destinations are nbxReduceMultiWide's bits, amax is numpy's max |acc| bit for
bit, sumSq is numpy's fp64 sum of squares within L * 2^-24 (L = 32,
include/nbx_reduce.h), over acc = the oracle's ordered fp32 fold of the exactly
widened sources (tests/wide's route), before any narrowing.

The file carries the parity core's name on purpose, as tests/wide/ does: the
GPU suite orders files by name (tests/conftest.py)."""

import numpy as np
import pytest

from tests.conftest import load_package
from tests.wide.test_reduce_gpu import BF16, E4M3, E5M2, F16, F32, PREMULSUM, SUM, Dev, avg3_bits, make_op, many_inputs, \
    widen

pytestmark = pytest.mark.gpu

PACKS, ELTS, BATCH, SHIFT = 6, 7, 15, 16
OUT32, STATS = 2, 8
BOUND = load_package().WIDE_STATS_L * 2.0 ** -24   # L as include/nbx_reduce.h states it, through the mirror
_INPUTS = {}


def inputs(oracle, st, nsrc, count):
    """The first `count` elements of `nsrc` seeded finite sources of type st (made once per type)."""
    if st not in _INPUTS:
        _INPUTS[st] = many_inputs(oracle, st, 8, 40000, seed=7000 + st)
    return [s[:count].copy() for s in _INPUTS[st][:nsrc]]


def check_stats(raw, acc, what=""):
    """16 bytes of an nbxWideStats against the accumulators `acc`."""
    got_sq, got_max, reserved = raw[:8].view(np.float64)[0], raw[8:12].view(np.float32)[0], raw[12:].view(np.uint32)[0]
    with np.errstate(all="ignore"):
        ref_max = np.max(np.abs(acc)) if acc.size else np.float32(0)
        ref_sq = np.sum(acc.astype(np.float64) ** 2)
    print(f"{what} amax {got_max!r} / {ref_max!r}  sumSq {got_sq!r} / {ref_sq!r}")
    assert reserved == 0
    if np.isnan(ref_max):
        assert np.isnan(got_max) and np.isnan(got_sq), what
        return
    assert got_max.view(np.uint32) == np.float32(ref_max).view(np.uint32), what
    if np.isinf(ref_sq):
        assert got_sq == np.inf, what
    else:
        assert abs(got_sq - ref_sq) <= BOUND * ref_sq, what


def run(nbx, oracle, torch, srcs, st, out32, family, unroll, devop=SUM, arg=0, npre=0, src_off=None, dst_off=(0,),
        arg_on_device=False):
    """One call of each entry point over the same uploads: equal destinations,
    the launch record's last pass on `family` with the stats flag, the record
    against the reference. Returns (the 16 bytes, acc)."""
    dev = Dev(torch)
    count, nsrc = srcs[0].size, len(srcs)
    deb = 4 if out32 else srcs[0].itemsize
    sb = [dev.buf(s.nbytes, o, s) for s, o in zip(srcs, src_off or [0] * nsrc)]
    plain, fused = ([dev.buf(count * deb, o) for o in dst_off] for _ in range(2))
    stats = dev.buf(16)
    op = make_op(nbx, dev, devop, arg, arg_on_device)
    stream = torch.cuda.current_stream().cuda_stream
    sp, dt = [Dev.ptr(b) for b in sb], F32 if out32 else st
    nbx.reduce_multi_wide([Dev.ptr(b) for b in plain], sp, count, st, dt, op, npre, stream)
    nbx.launch_log_reset()
    nbx.reduce_multi_wide_stats([Dev.ptr(b) for b in fused], sp, count, st, dt, op, Dev.ptr(stats), npre, stream)
    torch.cuda.synchronize()
    last = nbx.launch_log()[1][-1]
    slots = nsrc if nsrc <= 8 else 1 + ((nsrc - 9) % 7 + 1)   # the last pass: the partial and 1 .. 7 sources
    assert last[:3] == (family, slots, unroll) and last[3] & STATS, last
    assert bool(last[3] & OUT32) == out32
    for a, b in zip(plain, fused):
        assert np.array_equal(Dev.read(a, np.uint8), Dev.read(b, np.uint8)) and Dev.guards_intact(b)
    assert Dev.guards_intact(stats)
    acc = oracle.reduce_multi([widen(oracle, s, st) for s in srcs], F32, devop, arg, npre, threads=8)[0]
    raw = Dev.read(stats, np.uint8)
    check_stats(raw, acc, f"type {st} nsrc {nsrc} count {count}")
    return raw.copy(), acc


def geometry(st, nsrc):
    """(elements per pack, packs per lane per tile, byte offsets that peel a head of 3)."""
    epp = 16 if st in (E4M3, E5M2) else 8
    return epp, 4 if nsrc >= 4 else 1, (epp - 3) * (16 // epp)


def full_count(st, nsrc):
    epp, unroll, _ = geometry(st, nsrc)
    return 3 + 2 * unroll * 256 * epp + epp + 5   # head, two full tiles, a one-pack ragged tile, tail


@pytest.mark.parametrize("nsrc", [1, 2, 4, 8])
@pytest.mark.parametrize("out32", [False, True], ids=["same", "fp32"])
@pytest.mark.parametrize("st", [F16, BF16, E4M3, E5M2])
def test_pack_kernel_shapes(nbx, oracle, torch_gpu, st, out32, nsrc):
    epp, unroll, off = geometry(st, nsrc)
    for count in (full_count(st, nsrc), 1, 3, 3 + epp):
        run(nbx, oracle, torch_gpu, inputs(oracle, st, nsrc, count), st, out32, PACKS, unroll, src_off=[off] * nsrc,
            dst_off=[4 if out32 else off])


@pytest.mark.parametrize("where", ["head", "last lane of tile 0", "ragged pack", "last tail"])
def test_planted_extremum(nbx, oracle, torch_gpu, where):
    nsrc, count = 4, full_count(BF16, 4)
    pos = {"head": 0, "last lane of tile 0": 3 + 1023 * 8 + 7, "ragged pack": 3 + 2048 * 8 + 2, "last tail": count - 1}[where]
    srcs = inputs(oracle, BF16, nsrc, count)
    for s in srcs:
        s[pos] = 0
    srcs[1][pos] = 0xC2C8   # -100.0
    raw, _ = run(nbx, oracle, torch_gpu, srcs, BF16, False, PACKS, 4, src_off=[10] * nsrc, dst_off=[10])
    assert raw[8:12].view(np.float32)[0] == 100.0


@pytest.mark.parametrize("where", ["body", "tail"])
@pytest.mark.parametrize("kind", ["inf", "nan", "nan and inf"])
def test_non_finite(nbx, oracle, torch_gpu, kind, where):
    count = full_count(BF16, 2)
    srcs = inputs(oracle, BF16, 2, count)
    pos = 777 if where == "body" else count - 2
    srcs[0][pos] = 0xFF80 if kind == "inf" else 0x7FC0
    if kind == "nan and inf":
        srcs[1][pos - 100] = 0x7F80
    raw, _ = run(nbx, oracle, torch_gpu, srcs, BF16, True, PACKS, 1, src_off=[10, 10], dst_off=[4])   # head 3, tail 5
    sq, amax = raw[:8].view(np.float64)[0], raw[8:12].view(np.float32)[0]
    assert (sq == np.inf and amax == np.inf) if kind == "inf" else (np.isnan(sq) and np.isnan(amax))


def test_statistics_are_pre_narrowing(nbx, oracle, torch_gpu):
    """60000 + 10000 in fp16: the destination overflows to inf, the statistics do not."""
    srcs = [np.full(4097, v, np.float16).view(np.uint16) for v in (60000.0, 10000.0)]
    raw, acc = run(nbx, oracle, torch_gpu, srcs, F16, False, PACKS, 1)
    assert (acc == 70000.0).all() and raw[8:12].view(np.float32)[0] == 70000.0 and np.isfinite(raw[:8].view(np.float64)[0])


@pytest.mark.parametrize("out32", [False, True], ids=["same", "fp32"])
@pytest.mark.parametrize("nsrc", [9, 17])
def test_only_the_last_pass_contributes(nbx, oracle, torch_gpu, nsrc, out32):
    """Eight sources of 1024 give a partial of 8192 everywhere; the later sources bring it down to
    32 .. 128 (9 sources) or to a value below 1 (17)."""
    count = full_count(BF16, 8)
    rng = np.random.default_rng(nsrc)
    srcs = [np.full(count, 0x4480, np.uint16) for _ in range(8)]
    if nsrc == 9:
        srcs.append(rng.choice(np.array([0xC5FF, 0xC5FE, 0xC5FC], np.uint16), count))   # -8160, -8128, -8064
    else:
        srcs += [np.full(count, 0xC480, np.uint16) for _ in range(8)] + inputs(oracle, BF16, 1, count)
    raw, acc = run(nbx, oracle, torch_gpu, srcs, BF16, out32, PACKS, 1)
    assert 0 < raw[8:12].view(np.float32)[0] <= 128.0 and np.abs(acc).max() <= 128.0


@pytest.mark.parametrize("family", ["elements", "realigning", "device scalar"])
def test_every_kernel_family(nbx, oracle, torch_gpu, family):
    arg = avg3_bits(oracle)
    if family == "elements":      # destinations on two alignments; two 2048-element tiles and a ragged one
        run(nbx, oracle, torch_gpu, inputs(oracle, BF16, 3, 2 * 2048 + 100), BF16, False, ELTS, 1, dst_off=[0, 2])
    elif family == "realigning":  # 3 sources: 128-pack wave tiles; two of them, a ragged one and a tail
        saved = nbx.set_wide_shift_min_elts(1)
        try:
            run(nbx, oracle, torch_gpu, inputs(oracle, E4M3, 3, (2 * 128 + 1) * 16 + 5), E4M3, True, SHIFT, 2,
                src_off=[0, 3, 7])
        finally:
            nbx.set_wide_shift_min_elts(saved)
    else:
        run(nbx, oracle, torch_gpu, inputs(oracle, F16, 4, full_count(F16, 4)), F16, False, PACKS, 4, PREMULSUM, arg, npre=2,
            arg_on_device=True)


def test_reproducible_across_grids_and_schedules(nbx, oracle, torch_gpu):
    torch, lib = torch_gpu, nbx.load_library()
    n = 3_000_001
    dev = Dev(torch)
    sb = [dev.buf(s.nbytes, 0, s) for s in many_inputs(oracle, BF16, 8, n, seed=99)]
    out, stats = dev.buf(n * 4), dev.buf(16)
    stream = torch.cuda.current_stream().cuda_stream
    saved, dyn_saved = nbx.get_launch_config(), lib.nbxDebugSetDynMinTiles(1)
    seen, schedules = set(), set()
    try:
        for per_cu in (1, 5):
            for dyn_min in (1, 1 << 20):
                nbx.set_launch_config(per_cu, 0)
                lib.nbxDebugSetDynMinTiles(dyn_min)
                nbx.launch_log_reset()
                nbx.reduce_multi_wide_stats([Dev.ptr(out)], [Dev.ptr(b) for b in sb], n, BF16, F32, nbx.DevRedOpFull(),
                                            Dev.ptr(stats), 0, stream)
                torch.cuda.synchronize()
                schedules.add(nbx.launch_log()[1][-1][3] & nbx.LAUNCH_DYNAMIC)
                seen.add(Dev.read(stats, np.uint8).tobytes())
    finally:
        nbx.set_launch_config(*saved)
        lib.nbxDebugSetDynMinTiles(dyn_saved)
    assert schedules == {0, 1} and len(seen) == 1
    check_stats(np.frombuffer(seen.pop(), np.uint8), Dev.read(out, np.float32))   # acc is the fp32 output itself


def test_batch(nbx, oracle, torch_gpu):
    """One table: empty, one element, a bucket across a chunk boundary (tiles 1-5 of chunks of 4), two
    in one chunk, a mixed layout and a 9-source bucket (own launches), a head-and-tail bucket."""
    torch = torch_gpu
    dev = Dev(torch)
    spec = [(2, 0, None), (2, 1, None), (2, 10000, None), (2, 100, None), (2, 300, None), (2, 777, [0, 2]),
            (9, 5000, None), (2, 3 + 2 * 2048 + 5, [10, 10])]
    tasks, plain, accs = [], [], []
    for k, (nsrc, count, offs) in enumerate(spec):
        srcs = many_inputs(oracle, BF16, nsrc, count, seed=300 + 20 * k)
        sb = [dev.buf(s.nbytes, o, s) for s, o in zip(srcs, offs or [0] * nsrc)]
        d, p = (dev.buf(count * 2, offs[0] if offs else 0) for _ in range(2))
        tasks.append(([Dev.ptr(d)], [Dev.ptr(b) for b in sb], count))
        plain.append((d, p))
        accs.append(oracle.reduce_multi([widen(oracle, s, BF16) for s in srcs], F32, SUM, 0, 0)[0] if count else
                    np.zeros(0, np.float32))
    stats = dev.buf(16 * len(spec))
    op, stream = nbx.DevRedOpFull(), torch.cuda.current_stream().cuda_stream
    nbx.reduce_multi_wide_batch([([Dev.ptr(p)], s, c) for (_, p), (_, s, c) in zip(plain, tasks)], BF16, BF16, op, 0, stream)
    nbx.launch_log_reset()
    nbx.reduce_multi_wide_batch_stats(tasks, BF16, BF16, op, Dev.ptr(stats), 0, stream)
    torch.cuda.synchronize()
    recs = nbx.launch_log()[1]
    assert [r[0] for r in recs] == [ELTS, PACKS, PACKS, BATCH], recs
    assert [bool(r[3] & STATS) for r in recs] == [True, False, True, True]   # the 9-source bucket's first pass is plain
    assert recs[3][3] >> nbx.LAUNCH_SEGS_SHIFT == 5
    first = Dev.read(stats, np.uint8).copy()
    for k, ((d, p), acc) in enumerate(zip(plain, accs)):
        assert np.array_equal(Dev.read(d, np.uint8), Dev.read(p, np.uint8)) and Dev.guards_intact(d)
        check_stats(first[16 * k:16 * k + 16], acc, f"bucket {k}")
    assert not first[:16].any() and Dev.guards_intact(stats)
    # a second run, and the call captured in a graph and replayed twice: the same bytes
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        nbx.reduce_multi_wide_batch_stats(tasks, BF16, BF16, op, Dev.ptr(stats), 0, torch.cuda.current_stream().cuda_stream)
    for again in (None, g, g):
        stats[0][:16 * len(spec)].fill_(0xA5)
        if again is None:
            nbx.reduce_multi_wide_batch_stats(tasks, BF16, BF16, op, Dev.ptr(stats), 0, stream)
        else:
            again.replay()
        torch.cuda.synchronize()
        assert np.array_equal(Dev.read(stats, np.uint8), first)
