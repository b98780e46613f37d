"""GPU parity of nbxReduceMultiWideMx with MXFP6 (NBX_FLOAT6_E2M3 / NBX_FLOAT6_E3M2)
elements against numpy, bit for bit: destination bytes, scale bytes and the guard
bytes around every buffer. The fp32 fold is oracle.reduce_multi over the widened
(for MXFP6 sources: decoded and scaled) inputs; the quantiser and the packer are
include/nbx_reduce.h's definitions written out below: the 32 magnitudes of each
type, their 31 midpoints, and the three byte formulas. No tolerance anywhere."""
import functools

import numpy as np
import pytest

from tests.wide.test_reduce_gpu import (BF16, F16, F32, PREMULSUM, SUM, Dev, assert_same, avg3_bits, make_op,
                                        many_inputs, narrow, widen)
from tests.widemx.test_reduce_gpu import MX_SCALED, PART_FIRST, SCALE_BYTES, SCALE_P, scale_in

pytestmark = pytest.mark.gpu

E2M3, E3M2 = 33, 34
FAM_BLOCKS, FAM_GENERIC = 22, 23
MBITS, BIAS, EMAX = {E2M3: 3, E3M2: 2}, {E2M3: 1, E3M2: 3}, {E2M3: 2, E3M2: 4}


def magnitude(t, c):
    e, m, one = (c & 31) >> MBITS[t], c & ((1 << MBITS[t]) - 1), 1 << MBITS[t]
    return m / one * 2.0 ** (1 - BIAS[t]) if e == 0 else (1 + m / one) * 2.0 ** (e - BIAS[t])


GRID = {t: np.array([magnitude(t, c) for c in range(32)]) for t in (E2M3, E3M2)}      # float64, exact
MIDS = {t: (g[:-1] + g[1:]) / 2 for t, g in GRID.items()}
DECODE = {t: np.concatenate([g, -g]).astype(np.float32) for t, g in GRID.items()}     # code -> value; bit 5 the sign
PAIRS = [(F16, E2M3), (BF16, E3M2), (BF16, E2M3), (E2M3, E2M3), (E3M2, E3M2), (E2M3, F32), (E3M2, F32)]
PAIR_IDS = ["f16-e2m3", "bf16-e3m2", "bf16-e2m3", "e2m3-e2m3", "e3m2-e3m2", "e2m3-f32", "e3m2-f32"]


# ---------------------------------------------------------------------------
# reference

def pack6(codes):
    """Codes -> the dense bit stream: ceil(3 n / 4) bytes, the last byte's spare bits 0."""
    n = codes.size
    c = np.concatenate([codes, np.zeros(-n % 4, np.uint8)]).astype(np.uint32).reshape(-1, 4).T
    b = np.stack([c[0] | c[1] << 6, c[1] >> 2 | c[2] << 4, c[2] >> 4 | c[3] << 2], axis=1) & 0xFF
    return b.astype(np.uint8).reshape(-1)[:(3 * n + 3) // 4]


def unpack6(b, n):
    b = np.concatenate([b, np.zeros(-b.size % 3, np.uint8)]).astype(np.uint32).reshape(-1, 3).T
    c = np.stack([b[0], b[0] >> 6 | b[1] << 2, b[1] >> 4 | b[2] << 4, b[2] >> 2], axis=1) & 63
    return c.astype(np.uint8).reshape(-1)[:n]


def mx6_quantise(acc, t):
    """fp32 accumulators -> (codes, one per element; scale bytes) as include/nbx_reduce.h defines MXFP6 output."""
    n, nb = acc.size, (acc.size + 31) // 32
    pad = np.zeros(nb * 32, np.float32)
    pad[:n] = acc
    mb = (pad.view(np.uint32) & 0x7FFFFFFF).reshape(nb, 32).max(axis=1)   # unsigned: NaN > inf > finite
    fin = mb < 0x7F800000
    s = np.where(fin, np.maximum((mb >> 23).astype(np.int64) - EMAX[t], 0), 255)
    r = np.where(fin, (254 - s) << 23, 0x3F800000).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        v = (pad.reshape(nb, 32) * r[:, None]).astype(np.float32)
        a = np.abs(v).astype(np.float64)[..., None]
        # nearest, a tie to the even code; nothing lies above code 31, so everything beyond it stays there
        code = np.where(np.arange(31) & 1, a >= MIDS[t], a > MIDS[t]).sum(axis=-1).astype(np.uint8)
    code = np.where(fin[:, None], code | (np.signbit(v) << 5), 0).astype(np.uint8)   # a 0xFF block: all codes 0
    return code.reshape(-1)[:n], s.astype(np.uint8)


def reference(oracle, srcs, scales, n, st, dt, devop=SUM, arg=0, npre=0):
    """-> (destination array: FP6 bytes or fp32, scale bytes or None)."""
    if st in DECODE:
        with np.errstate(all="ignore"):
            wide = [(DECODE[st][unpack6(s, n)] * np.repeat(scale_in(e), 32)[:n]).astype(np.float32)
                    for s, e in zip(srcs, scales)]
    else:
        wide = [widen(oracle, s, st) for s in srcs]
    fold = oracle.reduce_multi(wide, F32, devop, arg, npre, threads=8)[0]
    if dt == F32:
        return fold, None
    codes, s = mx6_quantise(fold, dt)
    return pack6(codes), s


def planted16(st, dt):
    """Edge blocks of three 16-bit sources as fp32 values (further sources hold zeros). The first blocks'
    maximum lies in [2^emax, 2^(emax + 1)), so R = 1 and the accumulators are narrowed as they are."""
    z, top = np.zeros(32, np.float32), GRID[dt][31]
    sign = np.where(np.arange(32) & 1, -1.0, 1.0).astype(np.float32)
    a = np.append(MIDS[dt], top + (top - GRID[dt][30]) / 2).astype(np.float32) * sign   # every tie; (7.5, 8) / (28, 32)
    tiny = np.full(32, 2.0 ** -14, np.float32)                  # ties met from fp32 neighbours on either side
    ulp = 2.0 ** (EMAX[dt] - (10 if st == F16 else 7))
    b = z.copy()
    b[:5] = [2 * 2.0 ** EMAX[dt] - ulp, -top, top + ulp, -(top + ulp), GRID[dt][1] / 2]
    blocks = [(a, z, z), (a, tiny, z), (a, z, -tiny), (b, z, z), (np.where(np.arange(32) == 3, np.float32(-0.0), z), z, z)]
    for special in (np.nan, np.inf, -np.inf):
        e = np.ones(32, np.float32)
        e[5] = special
        blocks.append((e, z, z))
    if st == BF16:                                  # S at both ends: a denormal maximum is S = 0
        for vals in ([2.0 ** 127, -2.0 ** 126, 2.0 ** 100], [2.0 ** -130, -2.0 ** -133, 2.0 ** -131]):
            e = z.copy()
            e[:3] = vals
            blocks.append((e, z, z))
    return blocks


def planted6(t):
    """Edge blocks of three MXFP6 sources as ((codes, scale byte),) * 3: every code at scale 127 plus half the
    step above it at scale 124 (every tie, and the saturating range above the largest), a third source
    stepping off the tie by a tiny amount; -0, a 0xFF block, an overflowing block, scale 0."""
    code_of = {float(v): c for c, v in enumerate(GRID[t])}
    half = np.append(np.diff(GRID[t]), GRID[t][31] - GRID[t][30]) / 2
    up = np.array([code_of[float(h * 8)] for h in half], np.uint8)             # at scale 124: h = value * 2^-3
    z, blocks = np.zeros(32, np.uint8), []
    for sgn in (0, 32):
        for tiny in (0, 8, 40):                                                # code 8 / -8 at scale 105
            blocks.append(((np.arange(32, dtype=np.uint8) | sgn, 127), (up | sgn, 124), (np.full(32, tiny, np.uint8), 105)))
    allc = np.arange(32, dtype=np.uint8) * 2 + 1
    blocks.append(((((np.arange(32) == 3) * 32).astype(np.uint8), 127), (z, 127), (z, 127)))   # -0 among zeros
    blocks.append(((allc, 255), (z, 127), (z, 127)))                                           # a NaN block
    blocks.append(((allc, 254), (z, 127), (z, 127)))                                           # 2^127 * > 2: inf
    blocks.append(((allc, 0), (z, 127), (z, 127)))                                             # scale 0: S = 0
    return blocks


@functools.lru_cache(maxsize=None)
def inputs(oracle, st, dt, count, seed=0):
    """8 seeded sources of `count` elements (FP6: bytes and scale bytes), the first blocks planted."""
    nb = (count + 31) // 32
    if st not in DECODE:
        srcs = many_inputs(oracle, st, 8, count, seed=1000 * st + count + seed)
        for j, blk in enumerate(planted16(st, dt)[:count // 32]):
            for k, s in enumerate(srcs):
                s[32 * j:32 * j + 32] = narrow(oracle, blk[k] if k < 3 else np.zeros(32, np.float32), st)
        return srcs, None
    rng = np.random.default_rng(count + seed)
    srcs = [rng.integers(0, 256, (3 * count + 3) // 4, dtype=np.uint8) for _ in range(8)]
    shared = rng.choice(SCALE_BYTES, nb, p=SCALE_P)
    scales = [np.where(rng.random(nb) < 0.8, shared, rng.choice(SCALE_BYTES, nb, p=SCALE_P)) for _ in range(8)]
    for j, blk in enumerate(planted6(st)[:count // 32]):
        for k in range(8):
            codes, e = blk[k] if k < 3 else (np.zeros(32, np.uint8), 127)
            srcs[k][24 * j:24 * j + 24] = pack6(codes)
            scales[k][j] = e
    return srcs, scales


def take(oracle, st, dt, count, nsrc, seeds=(0,)):
    parts = [inputs(oracle, st, dt, count, seed=s) for s in seeds]
    srcs = [x for p in parts for x in p[0]][:nsrc]
    return srcs, [x for p in parts for x in p[1]][:nsrc] if st in DECODE else None


def nbytes(t, n):
    return (3 * n + 3) // 4 if t in DECODE else n * (4 if t == F32 else 2)


# ---------------------------------------------------------------------------
# one call, checked

def run_mx6(nbx, torch, srcs, scales, n, st, dt, exp, devop=SUM, arg=0, npre=0, src_off=None, dst_off=0, inplace=None,
            family=FAM_BLOCKS, arg_on_device=False):
    dev = Dev(torch)
    nb = (n + 31) // 32
    src_off = src_off or [0] * len(srcs)
    sb = [dev.buf(s.nbytes, o, s) for s, o in zip(srcs, src_off)]
    ssb = [dev.buf(nb, 0, e) for e in scales] if scales is not None else None
    if inplace is not None:
        outs, osc = [sb[inplace]], [ssb[inplace]]
    else:
        outs = [dev.buf(nbytes(dt, n), dst_off)]
        osc = [dev.buf(nb)] if dt != F32 else None
    nbx.launch_log_reset()
    nbx.reduce_multi_wide_mx([Dev.ptr(b) for b in outs], [Dev.ptr(b) for b in osc] if osc else None,
                             [Dev.ptr(b) for b in sb], [Dev.ptr(b) for b in ssb] if ssb else None, n, st, dt,
                             make_op(nbx, dev, devop, arg, arg_on_device), npre, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if dt == F32:
        assert_same(Dev.read(outs[0], np.float32), exp[0], F32)
    else:
        got, gs = Dev.read(outs[0], np.uint8), Dev.read(osc[0], np.uint8)
        assert np.array_equal(gs, exp[1]), f"scale bytes differ at blocks {np.flatnonzero(gs != exp[1])[:8]}"
        bad = np.flatnonzero(got != exp[0])
        assert bad.size == 0, f"{bad.size} bytes differ, first {bad[:8]}: got {got[bad[:4]]} exp {exp[0][bad[:4]]}"
    for b in outs + (osc or []) + sb + (ssb or []):
        assert Dev.guards_intact(b), "bytes around a buffer were written"
    last = nbx.launch_log()[1][-1]
    assert last[0] == family and bool(last[3] & MX_SCALED) == (st in DECODE), last
    return last


def body_count(nbx, st, nsrc):
    """One full tile of the block kernel, three blocks of a partial one, a 7-element tail."""
    return nbx.mx6_tile_elts(st, nsrc) + 3 * 32 + 7


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("nsrc", [1, 2, 3, 8])
def test_block_kernel(nbx, oracle, torch_gpu, pair, nsrc):
    st, dt = pair
    for count in (1, 3, 5, 31, 33, body_count(nbx, st, nsrc)):
        srcs, scales = take(oracle, st, dt, count, nsrc)
        run_mx6(nbx, torch_gpu, srcs, scales, count, st, dt, reference(oracle, srcs, scales, count, st, dt))


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("off", ["dst", "src"])
def test_any_alignment_gives_the_same_bits(nbx, oracle, torch_gpu, pair, off):
    """A destination one byte off (fp32: one element); a 16-bit source one element off, an FP6 source one byte."""
    st, dt = pair
    count = body_count(nbx, st, 3)
    srcs, scales = take(oracle, st, dt, count, 3)
    exp = reference(oracle, srcs, scales, count, st, dt)
    kw = dict(dst_off=4 if dt == F32 else 1) if off == "dst" else dict(src_off=[0, srcs[0].itemsize, 0])
    run_mx6(nbx, torch_gpu, srcs, scales, count, st, dt, exp, family=FAM_GENERIC, **kw)


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_premulsum_scalar_by_device_pointer(nbx, oracle, torch_gpu, pair):
    st, dt = pair
    count = body_count(nbx, st, 3)
    srcs, scales = take(oracle, st, dt, count, 3)
    arg = avg3_bits(oracle)
    exp = reference(oracle, srcs, scales, count, st, dt, PREMULSUM, arg, 2)
    run_mx6(nbx, torch_gpu, srcs, scales, count, st, dt, exp, PREMULSUM, arg, npre=2, arg_on_device=True)


@pytest.mark.parametrize("t", [E2M3, E3M2], ids=["e2m3", "e3m2"])
def test_in_place_on_the_sources_own_scale_array(nbx, oracle, torch_gpu, t):
    count = body_count(nbx, t, 5)
    srcs, scales = take(oracle, t, t, count, 5)
    exp = reference(oracle, srcs, scales, count, t, t)
    run_mx6(nbx, torch_gpu, [s.copy() for s in srcs], scales, count, t, t, exp, inplace=2)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_nine_bf16_sources(nbx, oracle, torch_gpu, graph):
    """The fp32 fold, the scratch partial and the PART pass; captured, three replays on changing inputs."""
    torch = torch_gpu
    n = body_count(nbx, BF16, 8)
    sets = [take(oracle, BF16, E2M3, n, 9, seeds=(s, s + 1))[0] for s in (0, 2)]
    if not graph:
        last = run_mx6(nbx, torch, sets[0], None, n, BF16, E2M3, reference(oracle, sets[0], None, n, BF16, E2M3))
        assert last[3] & PART_FIRST and nbx.launch_log()[0] >= 2
        return
    dev = Dev(torch)
    sb = [dev.buf(2 * n, 0, s) for s in sets[0]]
    out, osc = dev.buf(nbytes(E2M3, n)), dev.buf((n + 31) // 32)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        nbx.reduce_multi_wide_mx([Dev.ptr(out)], [Dev.ptr(osc)], [Dev.ptr(b) for b in sb], None, n, BF16, E2M3,
                                 nbx.DevRedOpFull(), 0, torch.cuda.current_stream().cuda_stream)
    for srcs in (sets[0], sets[1], sets[1]):
        for b, s in zip(sb, srcs):
            b[0][:s.nbytes].copy_(torch.from_numpy(s.view(np.uint8).copy()))
        out[0][:out[2]].fill_(0xA5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        exp = reference(oracle, srcs, None, n, BF16, E2M3)
        assert np.array_equal(Dev.read(out, np.uint8), exp[0]) and np.array_equal(Dev.read(osc, np.uint8), exp[1])
    assert Dev.guards_intact(out) and Dev.guards_intact(osc)
