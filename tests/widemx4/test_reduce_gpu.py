"""GPU parity of nbxReduceMultiWideMx with MXFP4 (NBX_FLOAT4_E2M1) elements
against numpy, bit for bit: destination bytes, scale bytes and the guard bytes
around every buffer. The fp32 fold is oracle.reduce_multi over the widened (for
MXFP4 sources: decoded and scaled) inputs; the quantiser is written out below:
a 16-entry decode table and the seven tie thresholds. The file name places it
with the single-GPU parity core (tests/conftest.py GPU_FILE_ORDER)."""
import functools

import numpy as np
import pytest

from tests.wide.test_reduce_gpu import (BF16, F16, F32, PREMULSUM, SUM, Dev, assert_same, avg3_bits, make_op,
                                        many_inputs, narrow, widen)
from tests.widemx.test_reduce_gpu import MX_SCALED, PART_FIRST, SCALE_BYTES, SCALE_P, scale_in

pytestmark = pytest.mark.gpu

FP4 = 32
FAM_BLOCKS, FAM_GENERIC = 19, 20
MAGS = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
DECODE = np.array(MAGS + [-m for m in MAGS], np.float32)           # code -> value; bit 3 is the sign
CODE = {float(v): c for c, v in enumerate(DECODE) if c != 8}       # value -> code (0.0 -> 0)
PAIRS = [(F16, FP4), (BF16, FP4), (FP4, FP4), (FP4, F32)]
PAIR_IDS = ["f16-fp4", "bf16-fp4", "fp4-fp4", "fp4-f32"]


# ---------------------------------------------------------------------------
# reference

def unpack(b, n):
    """FP4 bytes -> n codes: element 2 j the low nibble of byte j."""
    return np.stack([b & 15, b >> 4], axis=1).reshape(-1)[:n]


def pack(codes):
    """Codes -> FP4 bytes; an odd count's last high nibble is 0."""
    c = np.concatenate([codes, np.zeros(codes.size & 1, np.uint8)]).astype(np.uint8)
    return c[0::2] | (c[1::2] << 4)


def mx4_quantise(acc):
    """fp32 accumulators -> (codes, one per element; scale bytes) as include/nbx_reduce.h defines MXFP4 output."""
    n, nb = acc.size, (acc.size + 31) // 32
    pad = np.zeros(nb * 32, np.float32)
    pad[:n] = acc
    mb = (pad.view(np.uint32) & 0x7FFFFFFF).reshape(nb, 32).max(axis=1)   # unsigned: NaN > inf > finite
    fin = mb < 0x7F800000
    s = np.where(fin, np.maximum((mb >> 23).astype(np.int64) - 2, 0), 255)
    r = np.where(fin, (254 - s) << 23, 0x3F800000).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        v = (pad.reshape(nb, 32) * r[:, None]).astype(np.float32)
        a = np.abs(v)
        code = ((a > 0.25).astype(np.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
    code = np.where(fin[:, None], code | (np.signbit(v) << 3), 0).astype(np.uint8)   # a 0xFF block: all codes 0
    return code.reshape(-1)[:n], s.astype(np.uint8)


def reference(oracle, srcs, scales, n, st, dt, devop=SUM, arg=0, npre=0):
    """-> (destination array: FP4 bytes or fp32, scale bytes or None)."""
    if st == FP4:
        with np.errstate(all="ignore"):
            wide = [(DECODE[unpack(s, n)] * np.repeat(scale_in(e), 32)[:n]).astype(np.float32)
                    for s, e in zip(srcs, scales)]
    else:
        wide = [widen(oracle, s, st) for s in srcs]
    fold = oracle.reduce_multi(wide, F32, devop, arg, npre, threads=8)[0]
    if dt == F32:
        return fold, None
    codes, s = mx4_quantise(fold)
    return pack(codes), s


TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5]   # and 5, in the blocks whose maximum lies above it


def planted16(st):
    """Edge blocks of three 16-bit sources as fp32 values (further sources hold zeros). Every block's
    maximum lies in [4, 8), so R = 1 and the accumulators are narrowed as they are."""
    ulp = lambda t: 2.0 ** (int(np.floor(np.log2(t))) - (10 if st == F16 else 7))
    z = np.zeros(32, np.float32)
    a = z.copy()                                    # every tie and its neighbours at the type's spacing
    a[:19] = [4.0] + [s * (t + d * ulp(t)) for k, t in enumerate(TIES) for s in [1 - 2 * (k & 1)] for d in (-1, 0, 1)]
    b = z.copy()                                    # the tie 5 and the saturation band (6, 8)
    b[:9] = [5 - ulp(5), 5, 5 + ulp(5), 6, 6 + ulp(6), 7, -7.5, 8 - ulp(4), -5]
    c, d = z.copy(), z.copy()                       # ties met from fp32 neighbours: t +- 2^-14 in the accumulator
    c[:15] = [4.0] + [t for t in TIES + [5.0] for _ in (0, 1)]
    d[1:15] = [s * 2.0 ** -14 for _ in range(7) for s in (1, -1)]
    blocks = [(a, z, z), (b, z, z), (c, d, z), (-c, z, d), (np.where(np.arange(32) == 3, np.float32(-0.0), z), z, z)]
    for special in (np.nan, np.inf):
        e = np.ones(32, np.float32)
        e[5] = special
        blocks.append((e, z, z))
    if st == BF16:                                  # S at both ends
        for vals in ([2.0 ** 127, -2.0 ** 126, 2.0 ** 100], [2.0 ** -130, -2.0 ** -133, 0.0]):
            e = z.copy()
            e[:3] = vals
            blocks.append((e, z, z))
    return blocks


def planted4():
    """Edge blocks of three MXFP4 sources as ((codes, scale byte),) * 3: sums of scaled codes that land on
    every tie (c + 0.25, c + 0.5, 4 + 1), beside it (a third source adds +-2^-18) and in (6, 8)."""
    i = np.arange(32)
    allc, z = (i & 15).astype(np.uint8), np.zeros(32, np.uint8)
    quarter = np.where(i < 16, CODE[0.5], CODE[1.0]).astype(np.uint8)        # at scale 126: + 0.25, + 0.5
    big = np.array([CODE[4.0], CODE[6.0], CODE[-4.0], CODE[-6.0]], np.uint8)[i & 3]
    step = np.array([CODE[0.0], CODE[0.5], CODE[1.0], CODE[1.5]], np.uint8)[(i >> 2) & 3]   # 4 + 1 = 5, 6 + 1 = 7, ...
    blocks = []
    for s0, s1 in (((allc, 127), (quarter, 126)), ((big, 127), (step, 127))):
        for tiny in (CODE[0.0], CODE[0.5], CODE[-0.5]):
            blocks.append((s0, s1, (np.full(32, tiny, np.uint8), 110)))
    blocks.append(((((i == 3) * 8).astype(np.uint8), 127), (z, 127), (z, 127)))   # -0 among zeros
    blocks.append(((allc, 255), (z, 127), (z, 127)))                              # a NaN block
    blocks.append(((big, 254), (z, 127), (z, 127)))                               # 4 * 2^127 overflows: an inf block
    return blocks


@functools.lru_cache(maxsize=None)
def inputs(oracle, st, count, seed=0):
    """8 seeded sources of `count` elements (FP4: bytes and scale bytes), the first blocks planted."""
    nb = (count + 31) // 32
    if st != FP4:
        srcs = many_inputs(oracle, st, 8, count, seed=1000 * st + count + seed)
        for j, blk in enumerate(planted16(st)[:count // 32]):
            for k, s in enumerate(srcs):
                s[32 * j:32 * j + 32] = narrow(oracle, blk[k] if k < 3 else np.zeros(32, np.float32), st)
        return srcs, None
    rng = np.random.default_rng(count + seed)
    srcs = [rng.integers(0, 256, (count + 1) // 2, dtype=np.uint8) for _ in range(8)]
    shared = rng.choice(SCALE_BYTES, nb, p=SCALE_P)
    scales = [np.where(rng.random(nb) < 0.8, shared, rng.choice(SCALE_BYTES, nb, p=SCALE_P)) for _ in range(8)]
    for j, blk in enumerate(planted4()[:count // 32]):
        for k in range(8):
            codes, e = blk[k] if k < 3 else (np.zeros(32, np.uint8), 127)
            srcs[k][16 * j:16 * j + 16] = pack(codes)
            scales[k][j] = e
    return srcs, scales


def tile_elts(nbx):
    """T: the largest tile of the block kernel, from the launch code."""
    return max(nbx.mx4_tile_elts(st, n) for st in (BF16, FP4) for n in range(1, 9))


# ---------------------------------------------------------------------------
# one call, checked

def run_mx4(nbx, torch, srcs, scales, n, st, dt, exp, devop=SUM, arg=0, npre=0, ndst=1, src_off=None, dst_off=0,
            inplace=None, family=FAM_BLOCKS):
    dev = Dev(torch)
    nb = (n + 31) // 32
    src_off = src_off or [0] * len(srcs)
    sb = [dev.buf(s.nbytes, o, s) for s, o in zip(srcs, src_off)]
    ssb = [dev.buf(nb, 0, e) for e in scales] if scales is not None else None
    if inplace is not None:
        outs, osc = [sb[inplace]], [ssb[inplace]]
    else:
        outs = [dev.buf(n * 4 if dt == F32 else (n + 1) // 2, dst_off) for _ in range(ndst)]
        osc = [dev.buf(nb) for _ in range(ndst)] if dt != F32 else None
    nbx.launch_log_reset()
    nbx.reduce_multi_wide_mx([Dev.ptr(b) for b in outs], [Dev.ptr(b) for b in osc] if osc else None,
                             [Dev.ptr(b) for b in sb], [Dev.ptr(b) for b in ssb] if ssb else None, n, st, dt,
                             make_op(nbx, dev, devop, arg, False), npre, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k, b in enumerate(outs):
        if dt == F32:
            assert_same(Dev.read(b, np.float32), exp[0], F32)
            continue
        got, gs = Dev.read(b, np.uint8), Dev.read(osc[k], np.uint8)
        assert np.array_equal(gs, exp[1]), f"scale bytes differ at blocks {np.flatnonzero(gs != exp[1])[:8]}"
        bad = np.flatnonzero(got != exp[0])
        assert bad.size == 0, f"{bad.size} bytes differ, first {bad[:8]}: got {got[bad[:4]]} exp {exp[0][bad[:4]]}"
    for b in outs + (osc or []) + sb + (ssb or []):
        assert Dev.guards_intact(b), "bytes around a buffer were written"
    last = nbx.launch_log()[1][-1]
    assert last[0] == family and bool(last[3] & MX_SCALED) == (st == FP4), last
    return last


def take(oracle, st, count, nsrc, seeds=(0,)):
    parts = [inputs(oracle, st, count, seed=s) for s in seeds]
    srcs = [x for p in parts for x in p[0]][:nsrc]
    return srcs, [x for p in parts for x in p[1]][:nsrc] if st == FP4 else None


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("nsrc", [1, 2, 3, 8])
def test_parity(nbx, oracle, torch_gpu, pair, nsrc):
    st, dt = pair
    t = tile_elts(nbx)
    for count in (1, 2, 31, 32, 33, 63, t + 32 + 5, 2 * t + 17):
        srcs, scales = take(oracle, st, count, nsrc)
        run_mx4(nbx, torch_gpu, srcs, scales, count, st, dt, reference(oracle, srcs, scales, count, st, dt))


@pytest.mark.parametrize("pair,off", [((F16, FP4), "dst"), ((BF16, FP4), "src"), ((FP4, FP4), "src"),
                                      ((FP4, FP4), "dst"), ((FP4, F32), "src")])
def test_generic_kernel_gives_the_same_bits(nbx, oracle, torch_gpu, pair, off):
    """A destination one byte off, a 16-bit source one element off, an FP4 source one byte off."""
    st, dt = pair
    count = 2 * tile_elts(nbx) + 17
    srcs, scales = take(oracle, st, count, 3)
    exp = reference(oracle, srcs, scales, count, st, dt)
    run_mx4(nbx, torch_gpu, srcs, scales, count, st, dt, exp)
    kw = dict(dst_off=1) if off == "dst" else dict(src_off=[0, srcs[0].itemsize, 0])
    run_mx4(nbx, torch_gpu, srcs, scales, count, st, dt, exp, family=FAM_GENERIC, **kw)


@pytest.mark.parametrize("pair", [(BF16, FP4), (FP4, FP4), (FP4, F32)], ids=["bf16-fp4", "fp4-fp4", "fp4-f32"])
@pytest.mark.parametrize("nsrc", [9, 17])
def test_more_than_eight_sources(nbx, oracle, torch_gpu, pair, nsrc):
    st, dt = pair
    count = tile_elts(nbx) + 32 + 5
    srcs, scales = take(oracle, st, count, nsrc, seeds=(0, 1, 2))
    arg = avg3_bits(oracle)
    exp = reference(oracle, srcs, scales, count, st, dt, PREMULSUM, arg, nsrc - 4)
    last = run_mx4(nbx, torch_gpu, srcs, scales, count, st, dt, exp, PREMULSUM, arg, npre=nsrc - 4)
    assert last[3] & PART_FIRST and nbx.launch_log()[0] >= 2


@pytest.mark.parametrize("case", ["two-dsts", "in-place"])
def test_other_cases(nbx, oracle, torch_gpu, case):
    count = tile_elts(nbx) + 32 + 5
    srcs, scales = take(oracle, FP4, count, 5)
    exp = reference(oracle, srcs, scales, count, FP4, FP4)
    kw = dict(ndst=2) if case == "two-dsts" else dict(inplace=2)
    run_mx4(nbx, torch_gpu, [s.copy() for s in srcs], scales, count, FP4, FP4, exp, **kw)


def test_graph_capture_and_replay(nbx, oracle, torch_gpu):
    """9 bf16 sources -> MXFP4: the fp32 fold, the scratch partial and the PART pass in one graph, on new inputs."""
    torch = torch_gpu
    n = tile_elts(nbx) + 32 + 5
    sets = [take(oracle, BF16, n, 9, seeds=(s, s + 1))[0] for s in (0, 2)]
    dev = Dev(torch)
    sb = [dev.buf(2 * n, 0, s) for s in sets[0]]
    out, osc = dev.buf((n + 1) // 2), dev.buf((n + 31) // 32)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        nbx.reduce_multi_wide_mx([Dev.ptr(out)], [Dev.ptr(osc)], [Dev.ptr(b) for b in sb], None, n, BF16, FP4,
                                 nbx.DevRedOpFull(), 0, torch.cuda.current_stream().cuda_stream)
    for srcs in (sets[0], sets[1], sets[1]):
        for b, s in zip(sb, srcs):
            b[0][:s.nbytes].copy_(torch.from_numpy(s.view(np.uint8).copy()))
        out[0][:out[2]].fill_(0xA5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        exp = reference(oracle, srcs, None, n, BF16, FP4)
        assert np.array_equal(Dev.read(out, np.uint8), exp[0]) and np.array_equal(Dev.read(osc, np.uint8), exp[1])
    assert Dev.guards_intact(out) and Dev.guards_intact(osc)
