"""GPU parity of nbxReduceMultiWideMx (MXFP8 block-scaled sums) against numpy
and the oracle's codecs, bit for bit (NaN codes compared as NaN): the fp32 fold
by oracle.reduce_multi over the widened (and, for MX sources, scaled) inputs,
per-block m / S / R by integer operations on the fp32 bits, one narrowing per
distinct scaled value. The file name places it with the single-GPU parity core
(tests/conftest.py GPU_FILE_ORDER), as tests/wide's."""
import functools

import numpy as np
import pytest

from tests.wide.test_reduce_gpu import (BF16, E4M3, E5M2, F16, F32, PREMULSUM, SUM, Dev, assert_same, avg3_bits,
                                        make_op, many_inputs, narrow, widen)

pytestmark = pytest.mark.gpu

KINDS = [(F16, False), (BF16, False), (E4M3, False), (E5M2, False), (E4M3, True), (E5M2, True)]
KIND_IDS = ["f16", "bf16", "e4m3", "e5m2", "mx-e4m3", "mx-e5m2"]
SCALE_BYTES = np.array([0, 1, 126, 127, 128, 254, 255], np.uint8)
SCALE_P = [0.02, 0.04, 0.3, 0.3, 0.3, 0.02, 0.02]   # mostly ordinary blocks; the ends and MX's NaN block now and then
FAM_BLOCKS, FAM_GENERIC, PART_FIRST, MX_SCALED = 17, 18, 4, 16


# ---------------------------------------------------------------------------
# reference

def scale_in(e):
    """Scale bytes -> X = 2^(e - 127) as fp32 (e = 0: a denormal); e = 0xFF is MX's NaN block."""
    x = np.ldexp(np.float32(1), np.minimum(e, 254).astype(np.int32) - 127).astype(np.float32)
    return np.where(e == 255, np.float32(np.nan), x)


def mx_quantise(oracle, acc, dt):
    """fp32 accumulators -> (fp8 codes, scale bytes) as include/nbx_reduce.h defines them."""
    emax = 8 if dt == E4M3 else 15
    n, nb = acc.size, (acc.size + 31) // 32
    pad = np.zeros(nb * 32, np.float32)
    pad[:n] = acc
    mb = (pad.view(np.uint32) & 0x7FFFFFFF).reshape(nb, 32).max(axis=1)   # unsigned: NaN > inf > finite
    fin = mb < 0x7F800000
    s = np.where(fin, np.maximum((mb >> 23).astype(np.int64) - emax, 0), 255)
    r = np.where(fin, (254 - s) << 23, 0x3F800000).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        scaled = (pad.reshape(nb, 32) * r[:, None]).astype(np.float32).reshape(-1)[:n]
    return narrow(oracle, scaled, dt), s.astype(np.uint8)


def reference(oracle, srcs, scales, st, dt, devop=SUM, arg=0, npre=0):
    n = srcs[0].size
    wide = [widen(oracle, s, st) for s in srcs]
    if scales is not None:
        with np.errstate(all="ignore"):
            wide = [(w * np.repeat(scale_in(e), 32)[:n]).astype(np.float32) for w, e in zip(wide, scales)]
    fold = oracle.reduce_multi(wide, F32, devop, arg, npre, threads=8)[0]
    return (fold, None) if dt == F32 else mx_quantise(oracle, fold, dt)


def planted(st):
    """Edge blocks as (source 0, source 1) fp32 values; further sources hold zeros there."""
    tiny = {F16: 2.0 ** -24, BF16: 2.0 ** -133, E4M3: 2.0 ** -9, E5M2: 2.0 ** -16}[st]
    base = np.zeros(32, np.float32)
    base[:5] = [7.0, 1.0, -0.5, tiny, -tiny]       # 7 = 448 * 2^-6 = 57344 * 2^-13
    z = np.zeros(32, np.float32)
    blocks = [(np.where(np.arange(32) == 3, np.float32(-0.0), z), z), (base, z)]
    for extra in (0.25, 0.5):                      # 464 and 480 (59392 and 61440) after scaling
        b = z.copy()
        b[0] = extra
        blocks.append((base, b))
    for special in (np.nan, np.inf):
        a = np.ones(32, np.float32)
        a[5] = special
        blocks.append((a, z))
    if st == BF16:                                 # S at both ends
        for vals in ([2.0 ** 127, -2.0 ** 126, 2.0 ** 100], [2.0 ** -130, -2.0 ** -133, 0.0]):
            a = z.copy()
            a[:3] = vals
            blocks.append((a, z))
    return blocks


@functools.lru_cache(maxsize=None)
def inputs(oracle, st, scaled, count, seed=0):
    """8 seeded sources of `count` codes (and their scale bytes): uniform, the first blocks planted."""
    srcs = many_inputs(oracle, st, 8, count, seed=1000 * st + count + seed)
    nb = (count + 31) // 32
    scales = None
    if scaled:
        rng = np.random.default_rng(count + st + seed)
        shared = rng.choice(SCALE_BYTES, nb, p=SCALE_P)
        scales = [np.where(rng.random(nb) < 0.8, shared, rng.choice(SCALE_BYTES, nb, p=SCALE_P)) for _ in range(8)]
    for j, (a, b) in enumerate(planted(st)[:count // 32]):
        for k, s in enumerate(srcs):
            s[32 * j:32 * j + 32] = narrow(oracle, a if k == 0 else b if k == 1 else np.zeros(32, np.float32), st)
            if scaled:
                scales[k][j] = 127
    return srcs, scales


def tile_elts(nbx):
    """T: the largest tile of the block kernel, from the launch code."""
    return max(nbx.mx_tile_elts(st, n) for st in (BF16, E4M3) for n in range(1, 9))


# ---------------------------------------------------------------------------
# one call, checked

def run_mx(nbx, oracle, torch, srcs, scales, st, dt, exp, devop=SUM, arg=0, npre=0, ndst=1, src_off=None, dst_off=0,
           arg_on_device=False, inplace=None, family=FAM_BLOCKS):
    dev = Dev(torch)
    n, nb = srcs[0].size, (srcs[0].size + 31) // 32
    src_off = src_off or [0] * len(srcs)
    sb = [dev.buf(s.nbytes, o, s) for s, o in zip(srcs, src_off)]
    ssb = [dev.buf(nb, 0, e) for e in scales] if scales is not None else None
    if inplace is not None:
        outs, osc = [sb[inplace]], [ssb[inplace] if ssb else dev.buf(nb)]
    else:
        outs = [dev.buf(n * (4 if dt == F32 else 1), dst_off) for _ in range(ndst)]
        osc = [dev.buf(nb) for _ in range(ndst)] if dt != F32 else None
    op = make_op(nbx, dev, devop, arg, arg_on_device)
    nbx.launch_log_reset()
    nbx.reduce_multi_wide_mx([Dev.ptr(b) for b in outs], [Dev.ptr(b) for b in osc] if osc else None,
                             [Dev.ptr(b) for b in sb], [Dev.ptr(b) for b in ssb] if ssb else None, n, st, dt, op, npre,
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k, b in enumerate(outs):
        assert_same(Dev.read(b, np.float32 if dt == F32 else np.uint8), exp[0], dt)
        if osc:
            got = Dev.read(osc[k], np.uint8)
            assert np.array_equal(got, exp[1]), f"scale bytes differ at blocks {np.flatnonzero(got != exp[1])[:8]}"
    for b in outs + (osc or []) + sb + (ssb or []):
        assert Dev.guards_intact(b), "bytes around a buffer were written"
    last = nbx.launch_log()[1][-1]
    assert last[0] == family and bool(last[3] & MX_SCALED) == (scales is not None), last
    return last


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("dt", [E4M3, E5M2])
@pytest.mark.parametrize("nsrc", [1, 2, 3, 8])
def test_parity(nbx, oracle, torch_gpu, kind, dt, nsrc):
    st, scaled = kind
    t = tile_elts(nbx)
    for count in (1, 31, 32, 33, t + 32 + 5, 2 * t + 17):
        srcs, scales = inputs(oracle, st, scaled, count)
        srcs, scales = srcs[:nsrc], scales[:nsrc] if scaled else None
        run_mx(nbx, oracle, torch_gpu, srcs, scales, st, dt, reference(oracle, srcs, scales, st, dt))


@pytest.mark.parametrize("k,kind", list(enumerate(KINDS)), ids=KIND_IDS)
def test_generic_kernel_gives_the_same_bits(nbx, oracle, torch_gpu, k, kind):
    st, scaled = kind
    srcs, scales = inputs(oracle, st, scaled, 2 * tile_elts(nbx) + 17)
    srcs, scales = srcs[:3], scales[:3] if scaled else None
    exp = reference(oracle, srcs, scales, st, E4M3)
    run_mx(nbx, oracle, torch_gpu, srcs, scales, st, E4M3, exp)
    off = dict(dst_off=1) if k % 2 == 0 else dict(src_off=[0, srcs[0].itemsize, 0])   # +1 byte / one element off
    run_mx(nbx, oracle, torch_gpu, srcs, scales, st, E4M3, exp, family=FAM_GENERIC, **off)


@pytest.mark.parametrize("kind", [(BF16, False), (E4M3, True)], ids=["bf16", "mx-e4m3"])
@pytest.mark.parametrize("nsrc", [9, 17])
def test_more_than_eight_sources(nbx, oracle, torch_gpu, kind, nsrc):
    st, scaled = kind
    count = tile_elts(nbx) + 32 + 5
    parts = [inputs(oracle, st, scaled, count, seed=s) for s in range(3)]
    srcs = [x for p in parts for x in p[0]][:nsrc]
    scales = [x for p in parts for x in p[1]][:nsrc] if scaled else None
    arg = avg3_bits(oracle)
    exp = reference(oracle, srcs, scales, st, E5M2, PREMULSUM, arg, nsrc - 4)
    last = run_mx(nbx, oracle, torch_gpu, srcs, scales, st, E5M2, exp, PREMULSUM, arg, npre=nsrc - 4)
    assert last[3] & PART_FIRST and nbx.launch_log()[0] >= 2


@pytest.mark.parametrize("st", [E4M3, E5M2])
@pytest.mark.parametrize("nsrc,dst_off,family", [(3, 0, FAM_BLOCKS), (8, 0, FAM_BLOCKS), (3, 4, FAM_GENERIC),
                                                 (10, 0, FAM_BLOCKS)])
def test_mx_sources_into_fp32(nbx, oracle, torch_gpu, st, nsrc, dst_off, family):
    count = 2 * tile_elts(nbx) + 17
    a, b = inputs(oracle, st, True, count), inputs(oracle, st, True, count, seed=1)
    srcs, scales = (a[0] + b[0])[:nsrc], (a[1] + b[1])[:nsrc]
    run_mx(nbx, oracle, torch_gpu, srcs, scales, st, F32, reference(oracle, srcs, scales, st, F32), dst_off=dst_off,
           family=family)


@pytest.mark.parametrize("case", ["premul-value", "premul-device", "avg", "two-dsts", "in-place", "in-place-plain"])
def test_other_cases(nbx, oracle, torch_gpu, case):
    st, scaled = (BF16, False) if case in ("premul-value", "avg") else (E4M3, case != "in-place-plain")
    srcs, scales = inputs(oracle, st, scaled, tile_elts(nbx) + 32 + 5)
    srcs, scales = srcs[:5], scales[:5] if scaled else None
    kw = {}
    if case.startswith("premul"):
        kw = dict(devop=PREMULSUM, arg=avg3_bits(oracle), npre=3, arg_on_device=case == "premul-device")
    elif case == "avg":
        op = nbx.host_to_dev_redop(nbx.ncclRedOp.ncclAvg, F32, 5)   # the fp32 Avg scalar: every source pre-multiplied
        kw = dict(devop=op.op, arg=op.scalarArg, npre=5)
    elif case == "two-dsts":
        kw = dict(ndst=2)
    elif case.startswith("in-place"):
        kw = dict(inplace=2)
    exp = reference(oracle, srcs, scales, st, E4M3, kw.get("devop", SUM), kw.get("arg", 0), kw.get("npre", 0))
    run_mx(nbx, oracle, torch_gpu, [s.copy() for s in srcs], scales, st, E4M3, exp, **kw)


def test_graph_capture_and_replay(nbx, oracle, torch_gpu):
    """9 MX sources -> MX e5m2: two passes and the scratch partial in one graph, replayed on new inputs."""
    torch = torch_gpu
    n = tile_elts(nbx) + 32 + 5
    nb = (n + 31) // 32
    sets = []
    for seed in (0, 2):
        a, b = inputs(oracle, E4M3, True, n, seed=seed), inputs(oracle, E4M3, True, n, seed=seed + 1)
        sets.append(((a[0] + b[0])[:9], (a[1] + b[1])[:9]))
    dev = Dev(torch)
    sb = [dev.buf(n, 0, s) for s in sets[0][0]]
    ssb = [dev.buf(nb, 0, e) for e in sets[0][1]]
    out, osc = dev.buf(n), dev.buf(nb)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        nbx.reduce_multi_wide_mx([Dev.ptr(out)], [Dev.ptr(osc)], [Dev.ptr(b) for b in sb], [Dev.ptr(b) for b in ssb], n,
                                 E4M3, E5M2, nbx.DevRedOpFull(), 0, torch.cuda.current_stream().cuda_stream)
    for srcs, scales in (sets[0], sets[1], sets[1]):
        for b, s in zip(sb + ssb, srcs + scales):
            b[0][:s.nbytes].copy_(torch.from_numpy(s.view(np.uint8).copy()))
        out[0][:n].fill_(0xA5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        exp = reference(oracle, srcs, scales, E4M3, E5M2)
        assert_same(Dev.read(out, np.uint8), exp[0], E5M2)
        assert np.array_equal(Dev.read(osc, np.uint8), exp[1])
    assert Dev.guards_intact(out) and Dev.guards_intact(osc)
