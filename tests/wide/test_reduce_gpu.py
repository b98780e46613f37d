"""GPU parity of nbxReduceMultiWide (fp32 accumulator, one rounding) against
the CPU oracle, bit for bit (NaN compared as NaN).

The expected result needs nothing new in the oracle: the inputs are widened
with the oracle's scalar codecs through a 256- / 65,536-entry table, folded
by the oracle's ordered fp32 Sum / PreMulSum (which the fp32 kernels already
match bit for bit), and for a narrow output narrowed once with the oracle's
codec applied to the distinct values of the fold.

The file carries the name of the parity core's file on purpose: the GPU suite
orders files by name (tests/conftest.py GPU_FILE_ORDER), and under this name
the wide parity checks run with the single-GPU core, ahead of the transports,
instead of splitting test_configs_gpu.py's two groups."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F16, F32, BF16, E4M3, E5M2 = 6, 7, 9, 10, 11
WIDE_TYPES = [F16, BF16, E4M3, E5M2]
SUM, PREMULSUM = 0, 3
FLOAT_TYPES = {6, 7, 8, 9, 10, 11}


def _dec16(a):
    return ((a & 0x7C00) == 0x7C00) & ((a & 0x3FF) != 0)


def _decbf16(a):
    return ((a & 0x7F80) == 0x7F80) & ((a & 0x7F) != 0)


def _dec_e4m3(a):
    return (a & 0x7F) == 0x7F


def _dec_e5m2(a):
    return ((a & 0x7C) == 0x7C) & ((a & 0x03) != 0)


def assert_same(got, exp, dtype):
    assert got.shape == exp.shape
    if dtype in FLOAT_TYPES:
        if dtype in (7, 8):
            gn, en = np.isnan(got), np.isnan(exp)
        else:
            dec = {6: _dec16, 9: _decbf16, 10: _dec_e4m3, 11: _dec_e5m2}[dtype]
            gn, en = dec(got), dec(exp)
        assert np.array_equal(gn, en), f"NaN mismatch at {np.flatnonzero(gn != en)[:8]}"
        keep = ~en
        ut = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.itemsize]
        bad = np.flatnonzero(got.view(ut)[keep] != exp.view(ut)[keep])
        assert bad.size == 0, f"{bad.size} mismatches, first at {np.flatnonzero(keep)[bad[:8]]}: " \
                              f"got {got.view(ut)[keep][bad[:4]]} exp {exp.view(ut)[keep][bad[:4]]}"
    else:
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, f"{bad.size} mismatches, first at {bad[:8]}: got {got[bad[:4]]} exp {exp[bad[:4]]}"


# ---------------------------------------------------------------------------
# reference

_TABLES = {}


def widen(oracle, a, dtype):
    """Raw codes -> fp32, through the oracle's scalar decoder of every code."""
    if dtype not in _TABLES:
        dec = {F16: oracle.f16_to_f32, BF16: oracle.bf16_to_f32, E4M3: oracle.e4m3_to_f32,
               E5M2: oracle.e5m2_to_f32}[dtype]
        n = 256 if dtype in (E4M3, E5M2) else 65536
        _TABLES[dtype] = np.array([dec(c) for c in range(n)], dtype=np.float32)
    return _TABLES[dtype][a]


def narrow(oracle, f, dtype):
    """fp32 -> raw codes with the oracle's scalar encoder, once per distinct value."""
    enc = {F16: oracle.f32_to_f16, BF16: oracle.f32_to_bf16, E4M3: oracle.f32_to_e4m3, E5M2: oracle.f32_to_e5m2}[dtype]
    bits, inv = np.unique(f.view(np.uint32), return_inverse=True)
    codes = np.array([enc(float(v)) for v in bits.view(np.float32)], dtype=oracle.NP_STORAGE[dtype])
    return codes[inv.reshape(-1)]


def f32_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def avg3_bits(oracle):
    """The 3-rank Avg scalar in fp32 (hostToDevRedOp for ncclFloat32)."""
    devop, arg = oracle.host_to_dev_redop(4, F32, 3)
    assert devop == PREMULSUM
    return arg


def many_inputs(oracle, st, nsrc, count, seed):
    """Seeded uniform[-1, 1) inputs like oracle.random_inputs, narrowed with
    numpy instead of one codec call per element (64 sources stay quick)."""
    if st in (E4M3, E5M2):
        return oracle.random_inputs(st, nsrc, count, seed=seed)
    out = []
    for s in range(nsrc):
        f = np.random.default_rng(seed + s).uniform(-1.0, 1.0, count).astype(np.float32)
        if st == F16:
            out.append(f.astype(np.float16).view(np.uint16))
        else:
            u = f.view(np.uint32).astype(np.uint64)
            out.append(((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16))   # RNE, finite inputs
    return out


def expected(oracle, srcs, st, out32, devop=SUM, arg=0, npre=0):
    fold = oracle.reduce_multi([widen(oracle, s, st) for s in srcs], F32, devop, arg, npre, threads=8)[0]
    return fold if out32 else narrow(oracle, fold, st)


# ---------------------------------------------------------------------------
# device staging: every buffer is 0xA5 around its payload

class Dev:
    PAD = 64

    def __init__(self, torch):
        self.torch = torch
        self.keep = []

    def buf(self, nbytes, offset=0, data=None):
        t = self.torch.full((nbytes + offset + self.PAD,), 0xA5, dtype=self.torch.uint8, device="cuda")
        if data is not None and data.nbytes:
            t[offset:offset + data.nbytes].copy_(self.torch.from_numpy(data.view(np.uint8).copy()))
        self.keep.append(t)
        return t, offset, nbytes

    @staticmethod
    def ptr(b):
        return b[0].data_ptr() + b[1]

    @staticmethod
    def read(b, dtype):
        t, o, n = b
        return t[o:o + n].cpu().numpy().view(dtype)

    @staticmethod
    def guards_intact(b):
        t, o, n = b
        return bool((t[:o] == 0xA5).all()) and bool((t[o + n:] == 0xA5).all())


def make_op(nbx, dev, devop, arg, arg_on_device):
    op = nbx.DevRedOpFull()
    op.op = devop
    if devop == PREMULSUM and arg_on_device:
        scal = dev.buf(4, 0, np.array([arg], dtype=np.uint32))
        op.scalarArgIsPtr = 1
        op.scalarArg = Dev.ptr(scal)
    else:
        op.scalarArg = arg
    return op


def run_wide(nbx, oracle, torch, srcs, st, out32, devop=SUM, arg=0, npre=0, ndst=1, src_off=None, dst_off=None,
             arg_on_device=False, inplace=None, exp=None):
    """One call checked against the oracle. inplace = k: the (single,
    source-type) destination is source k's buffer."""
    dev = Dev(torch)
    count = srcs[0].size
    nsrc = len(srcs)
    dt = F32 if out32 else st
    dst_np = np.float32 if out32 else oracle.NP_STORAGE[st]
    deb = np.dtype(dst_np).itemsize
    src_off = src_off or [0] * nsrc
    dst_off = dst_off or [0] * ndst
    sb = [dev.buf(s.nbytes, o, s) for s, o in zip(srcs, src_off)]
    if inplace is not None:
        assert not out32 and ndst == 1
        outs = [sb[inplace]]
    else:
        outs = [dev.buf(count * deb, o) for o in dst_off]
    op = make_op(nbx, dev, devop, arg, arg_on_device)
    if exp is None:
        exp = expected(oracle, srcs, st, out32, devop, arg, npre)
    stream = torch.cuda.current_stream().cuda_stream
    nbx.reduce_multi_wide([Dev.ptr(b) for b in outs], [Dev.ptr(b) for b in sb], count, st, dt, op, npre, stream)
    torch.cuda.synchronize()
    for b in outs:
        assert_same(Dev.read(b, dst_np), exp, dt)
    for k, b in enumerate(outs + sb):
        assert Dev.guards_intact(b), f"bytes around buffer {k} were written"
    for k, (b, s) in enumerate(zip(sb, srcs)):   # sources are read-only (but for the in-place one)
        if k != inplace:
            assert np.array_equal(Dev.read(b, s.dtype), s)
    return exp


def per_step_sum(nbx, torch, srcs, st):
    """nbxReduceMulti Sum of the same inputs (the per-step rule)."""
    dev = Dev(torch)
    sb = [dev.buf(s.nbytes, 0, s) for s in srcs]
    out = dev.buf(srcs[0].nbytes)
    nbx.reduce_multi([Dev.ptr(out)], [Dev.ptr(b) for b in sb], srcs[0].size, st, nbx.DevRedOpFull(), 0, False,
                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return Dev.read(out, srcs[0].dtype)


# ---------------------------------------------------------------------------
# 1. known answers

KNOWN_N = 4097


@pytest.mark.parametrize("st,small,wide_code,step_code,wide_f32", [
    (BF16, 0x3B00, 0x3F82, 0x3F80, 1.013671875),
    (F16, 0x0C00, 0x3C02, 0x3C00, 1.001708984375),
    (E4M3, 0x08, 0x39, 0x38, 1.109375),
    (E5M2, 0x2C, 0x3E, 0x3C, 1.4375),
])
def test_known_answers_one_plus_seven_small(nbx, oracle, torch_gpu, st, small, wide_code, step_code, wide_f32):
    npst = oracle.NP_STORAGE[st]
    one = {BF16: 0x3F80, F16: 0x3C00, E4M3: 0x38, E5M2: 0x3C}[st]
    srcs = [np.full(KNOWN_N, one, npst)] + [np.full(KNOWN_N, small, npst) for _ in range(7)]
    known = run_wide(nbx, oracle, torch_gpu, srcs, st, False, exp=np.full(KNOWN_N, wide_code, npst))
    assert_same(expected(oracle, srcs, st, False), known, st)         # the oracle route gives the same codes
    run_wide(nbx, oracle, torch_gpu, srcs, st, True, exp=np.full(KNOWN_N, wide_f32, np.float32))
    # what the per-step rule makes of the same inputs (documents the difference)
    assert (per_step_sum(nbx, torch_gpu, srcs, st) == step_code).all()


@pytest.mark.parametrize("st,pmax,nmax,step_code", [
    (E4M3, 0x7E, 0xFE, 0xFE), (E5M2, 0x7B, 0xFB, 0xFB), (F16, 0x7BFF, 0xFBFF, 0x7C00)])
def test_known_answers_intermediate_overflow(nbx, oracle, torch_gpu, st, pmax, nmax, step_code):
    """[+max, +max, -max, -max]: the fp32 accumulator passes through 2 x max
    and comes back to zero; the per-step rule saturates (fp8) or overflows (f16)."""
    npst = oracle.NP_STORAGE[st]
    srcs = [np.full(KNOWN_N, c, npst) for c in (pmax, pmax, nmax, nmax)]
    run_wide(nbx, oracle, torch_gpu, srcs, st, False, exp=np.zeros(KNOWN_N, npst))
    run_wide(nbx, oracle, torch_gpu, srcs, st, True, exp=np.zeros(KNOWN_N, np.float32))
    assert (per_step_sum(nbx, torch_gpu, srcs, st) == step_code).all()


@pytest.mark.parametrize("st,pmax,out_code,out_f32", [
    (E4M3, 0x7E, 0x7E, 3584.0), (E5M2, 0x7B, 0x7B, 458752.0), (F16, 0x7BFF, 0x7C00, 524032.0)])
def test_known_answers_final_overflow(nbx, oracle, torch_gpu, st, pmax, out_code, out_f32):
    """Eight +max: fp8 saturates to the largest finite code, f16 goes to inf."""
    npst = oracle.NP_STORAGE[st]
    srcs = [np.full(KNOWN_N, pmax, npst) for _ in range(8)]
    run_wide(nbx, oracle, torch_gpu, srcs, st, False, exp=np.full(KNOWN_N, out_code, npst))
    run_wide(nbx, oracle, torch_gpu, srcs, st, True, exp=np.full(KNOWN_N, out_f32, np.float32))


# ---------------------------------------------------------------------------
# 2. type x output x op x source count

@pytest.mark.parametrize("st", WIDE_TYPES)
@pytest.mark.parametrize("out32", [False, True])
@pytest.mark.parametrize("nsrc", [1, 2, 3, 8])
def test_types_outputs_ops(nbx, oracle, torch_gpu, st, out32, nsrc):
    rng = np.random.default_rng(500 + st * 16 + nsrc * 2 + out32)
    srcs = oracle.random_inputs(st, nsrc, 70001, seed=int(rng.integers(1 << 30)), specials=True)
    run_wide(nbx, oracle, torch_gpu, srcs, st, out32)
    arg = avg3_bits(oracle)
    for on_device in (False, True):
        npre = int(rng.integers(0, nsrc + 1))
        run_wide(nbx, oracle, torch_gpu, srcs, st, out32, PREMULSUM, arg, npre=npre, arg_on_device=on_device)


# ---------------------------------------------------------------------------
# 3. edge sizes, at every launch configuration

@pytest.mark.parametrize("count", [0, 1, 7, 8, 15, 16, 17, 255, 4095, 4096, 65537, (1 << 20) + 13])
@pytest.mark.parametrize("st", [BF16, E4M3])
@pytest.mark.parametrize("out32", [False, True])
def test_edge_sizes(nbx, oracle, torch_gpu, st, out32, count):
    if count == 0:
        dev = Dev(torch_gpu)
        b = dev.buf(16)
        rc = nbx.reduce_multi_wide_raw([Dev.ptr(b)], [Dev.ptr(dev.buf(16))] * 8, 0, st, F32 if out32 else st,
                                       nbx.DevRedOpFull())
        torch_gpu.cuda.synchronize()
        assert rc == 0 and Dev.guards_intact(b) and (Dev.read(b, np.uint8) == 0xA5).all()
        return
    srcs = oracle.random_inputs(st, 8, count, seed=11 + count)
    exp = expected(oracle, srcs, st, out32)
    saved = nbx.get_launch_config()
    try:
        for cfg in ((0, 0), (0, 1), (0, 2)):
            nbx.set_launch_config(*cfg)
            run_wide(nbx, oracle, torch_gpu, srcs, st, out32, exp=exp)
    finally:
        nbx.set_launch_config(*saved)


# ---------------------------------------------------------------------------
# 4. dynamic tile schedule

def test_dynamic_tiles_back_to_back(nbx, oracle, torch_gpu):
    """The unrolled wide kernels take tiles from the stream's counter under the
    per-step kernels' rule; forced here for every launch. Two calls back to
    back on one stream: the second starts from the base the first left."""
    torch = torch_gpu
    lib = nbx.load_library()
    n = 3_000_001
    srcs = oracle.random_inputs(BF16, 8, n, seed=4242)
    exp = expected(oracle, srcs, BF16, True)
    dev = Dev(torch)
    sb = [dev.buf(s.nbytes, 0, s) for s in srcs]
    outs = [dev.buf(n * 4), dev.buf(n * 4)]
    stream = torch.cuda.current_stream().cuda_stream
    prev = lib.nbxDebugSetDynMinTiles(1)
    try:
        for o in outs:
            nbx.reduce_multi_wide([Dev.ptr(o)], [Dev.ptr(b) for b in sb], n, BF16, F32, nbx.DevRedOpFull(), 0, stream)
        torch.cuda.synchronize()
    finally:
        lib.nbxDebugSetDynMinTiles(prev)
    for o in outs:
        assert_same(Dev.read(o, np.float32), exp, F32)
        assert Dev.guards_intact(o)


# ---------------------------------------------------------------------------
# 5. alignment

@pytest.mark.parametrize("st,offs", [(BF16, [2, 6, 14]), (E4M3, [1, 5, 15])])
@pytest.mark.parametrize("count", [100, 70001])
def test_shared_misalignment_same_type(nbx, oracle, torch_gpu, st, offs, count):
    srcs = oracle.random_inputs(st, 3, count, seed=count + st)
    exp = expected(oracle, srcs, st, False)
    for off in offs:
        run_wide(nbx, oracle, torch_gpu, srcs, st, False, src_off=[off] * 3, dst_off=[off], exp=exp)


@pytest.mark.parametrize("st", [BF16, E4M3])
@pytest.mark.parametrize("count", [100, 70001])
def test_fp32_destination_alignment(nbx, oracle, torch_gpu, st, count):
    """Sources `off` bytes past a 16-byte boundary peel head = (16 - off) / eb
    elements; the pack kernel needs (dst + 4 * head) % 16 == 0, any other
    destination offset takes the element kernel."""
    eb = np.dtype(oracle.NP_STORAGE[st]).itemsize
    srcs = oracle.random_inputs(st, 5, count, seed=count + 3 * st)
    exp = expected(oracle, srcs, st, True)
    for off in ([2, 6, 14] if st == BF16 else [1, 5, 15]):
        head = (16 - off) // eb
        good = (-4 * head) % 16
        for dst_off in (good, (good + 4) % 16, (good + 8) % 16):
            run_wide(nbx, oracle, torch_gpu, srcs, st, True, src_off=[off] * 5, dst_off=[dst_off], exp=exp)
    # aligned sources, destination 4 past a boundary: element kernel
    run_wide(nbx, oracle, torch_gpu, srcs, st, True, dst_off=[4], exp=exp)
    # two destinations, only one of them aligned: element kernel
    run_wide(nbx, oracle, torch_gpu, srcs, st, True, ndst=2, dst_off=[0, 12], exp=exp)


@pytest.mark.parametrize("st", [BF16, E4M3])
@pytest.mark.parametrize("out32", [False, True])
@pytest.mark.parametrize("count", [100, 70001])
def test_mixed_source_misalignment(nbx, oracle, torch_gpu, st, out32, count):
    eb = np.dtype(oracle.NP_STORAGE[st]).itemsize
    srcs = oracle.random_inputs(st, 4, count, seed=count + 5 * st, specials=True)
    run_wide(nbx, oracle, torch_gpu, srcs, st, out32, PREMULSUM, avg3_bits(oracle), npre=3,
             src_off=[0, eb, 3 * eb, 0], dst_off=[0 if out32 else 2 * eb])
    # sources aligned alike, a source-type destination elsewhere: element kernel too
    if not out32:
        run_wide(nbx, oracle, torch_gpu, srcs, st, False, src_off=[eb] * 4, dst_off=[0])


# ---------------------------------------------------------------------------
# 6. destinations, 7. in place

@pytest.mark.parametrize("st", [F16, E5M2])
@pytest.mark.parametrize("out32", [False, True])
@pytest.mark.parametrize("ndst,nsrc", [(2, 3), (8, 8), (2, 8), (8, 3)])
def test_several_destinations(nbx, oracle, torch_gpu, st, out32, ndst, nsrc):
    srcs = oracle.random_inputs(st, nsrc, 20011, seed=ndst * 10 + nsrc + st)
    run_wide(nbx, oracle, torch_gpu, srcs, st, out32, ndst=ndst)


@pytest.mark.parametrize("st", WIDE_TYPES)
@pytest.mark.parametrize("nsrc", [1, 3, 8])
def test_in_place(nbx, oracle, torch_gpu, st, nsrc):
    srcs = oracle.random_inputs(st, nsrc, 70001, seed=nsrc + 7 * st, specials=True)
    exp = expected(oracle, srcs, st, False)
    for k in sorted({0, nsrc - 1}):
        run_wide(nbx, oracle, torch_gpu, srcs, st, False, inplace=k, exp=exp)


# ---------------------------------------------------------------------------
# 8. more than 8 sources

@pytest.mark.parametrize("st", [BF16, E5M2])
@pytest.mark.parametrize("out32", [False, True])
@pytest.mark.parametrize("nsrc", [9, 16, 20, 64])
def test_more_than_eight_sources(nbx, oracle, torch_gpu, st, out32, nsrc):
    """Ordered passes through an fp32 partial: the single fp32 left fold over
    all sources, with the pre-multiplied sources ending inside a later pass."""
    srcs = oracle.random_inputs(st, 9, 70001, seed=27 + st, specials=True) if nsrc == 9 else \
        many_inputs(oracle, st, nsrc, 70001, seed=nsrc * 3 + st)
    arg = avg3_bits(oracle)
    npre = {9: 9, 16: 11, 20: 16, 64: 37}[nsrc]
    exp_sum = run_wide(nbx, oracle, torch_gpu, srcs, st, out32)
    exp_pre = run_wide(nbx, oracle, torch_gpu, srcs, st, out32, PREMULSUM, arg, npre=npre, arg_on_device=(nsrc == 16))
    if not out32:
        run_wide(nbx, oracle, torch_gpu, srcs, st, False, inplace=nsrc - 1, exp=exp_sum)
        run_wide(nbx, oracle, torch_gpu, srcs, st, False, PREMULSUM, arg, npre=npre, inplace=nsrc - 1, exp=exp_pre)


@pytest.mark.parametrize("out32", [False, True])
def test_more_than_eight_sources_misaligned(nbx, oracle, torch_gpu, out32):
    """The partial follows the sources' head: shared misalignment (pack kernel,
    scratch partial placed to match) and mixed (element kernel)."""
    srcs = oracle.random_inputs(BF16, 11, 20011, seed=77)
    exp = expected(oracle, srcs, BF16, out32)
    run_wide(nbx, oracle, torch_gpu, srcs, BF16, out32, src_off=[6] * 11, dst_off=[4 if out32 else 6], exp=exp)
    run_wide(nbx, oracle, torch_gpu, srcs, BF16, out32, src_off=[2 * (k % 3) for k in range(11)], dst_off=[0], exp=exp)


# ---------------------------------------------------------------------------
# 9. graph capture

def test_graph_capture_with_scratch_partial(nbx, oracle, torch_gpu):
    """bf16 -> bf16 with 20 sources: three passes and the stream-ordered
    scratch partial inside one captured graph, replayed on new inputs."""
    torch = torch_gpu
    n, nsrc = 70001, 20
    dev = Dev(torch)
    first = oracle.random_inputs(BF16, nsrc, n, seed=900)
    second = oracle.random_inputs(BF16, nsrc, n, seed=901)
    sb = [dev.buf(s.nbytes, 0, s) for s in first]
    out = dev.buf(n * 2)
    op = nbx.DevRedOpFull()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        nbx.reduce_multi_wide([Dev.ptr(out)], [Dev.ptr(b) for b in sb], n, BF16, BF16, op, 0,
                              torch.cuda.current_stream().cuda_stream)
    g.replay()
    torch.cuda.synchronize()
    assert_same(Dev.read(out, np.uint16), expected(oracle, first, BF16, False), BF16)
    for b, s in zip(sb, second):
        b[0][:s.nbytes].copy_(torch.from_numpy(s.view(np.uint8).copy()))
    out[0][:n * 2].fill_(0xA5)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert_same(Dev.read(out, np.uint16), expected(oracle, second, BF16, False), BF16)
    assert Dev.guards_intact(out)


# ---------------------------------------------------------------------------
# 10. the per-step path is untouched

@pytest.mark.parametrize("st", [BF16, E4M3])
def test_per_step_path_untouched(nbx, oracle, torch_gpu, st):
    torch = torch_gpu
    n = 70001
    srcs = oracle.random_inputs(st, 8, n, seed=31 + st)
    dev = Dev(torch)
    sb = [dev.buf(s.nbytes, 0, s) for s in srcs]
    wide_out, step_out = dev.buf(n * 4), dev.buf(srcs[0].nbytes)
    stream = torch.cuda.current_stream().cuda_stream
    sp = [Dev.ptr(b) for b in sb]
    nbx.reduce_multi_wide([Dev.ptr(wide_out)], sp, n, st, F32, nbx.DevRedOpFull(), 0, stream)
    nbx.reduce_multi([Dev.ptr(step_out)], sp, n, st, nbx.DevRedOpFull(), 0, False, stream)
    torch.cuda.synchronize()
    assert_same(Dev.read(step_out, srcs[0].dtype), oracle.reduce_multi(srcs, st, SUM, threads=8)[0], st)
    assert_same(Dev.read(wide_out, np.float32), expected(oracle, srcs, st, True), F32)
    assert Dev.guards_intact(step_out) and Dev.guards_intact(wide_out)
