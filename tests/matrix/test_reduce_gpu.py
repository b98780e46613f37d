"""Every reduce-kernel instantiation — type x op x source count x kernel shape
— against the CPU oracle, bit for bit (NaN compared as NaN), at the smallest
sizes that reach every branch of each kernel's tile loop.

makeKernelSet compiles one kernel per (functor, shape, source count); the
sized-up tests elsewhere reach the big-tile, LDS and wide shapes only along a
few diagonals. Here each case is one nbxReduceMulti / nbxReduceMultiWide call
of a forced shape, and the library's launch record (nbxDebugLaunchLog) has to
say that the intended family, source count and unroll ran: a forced variant
that was silently ignored would still give the right answer from another
kernel.

Sizes: 9,037 packs = 2 x 4,096 + 3 x 256 + 77, which for every unroll in
{1, 4, 8, 16} is several full tiles, a last tile where some lanes hold one
pack fewer, then tail elements; 1,301 packs does the same for the LDS
kernel's 256- / 512-pack tiles. Inputs are tests/matrix/inputs.py's edge-rich
values (random bit patterns, denormals); every case asserts that NaN (compared
only as NaN) stays under 10 % of the oracle's result.

The file carries the parity core's name on purpose, as tests/wide/ does: the
GPU suite orders files by name (tests/conftest.py GPU_FILE_ORDER)."""
import numpy as np
import pytest

from tests.matrix import inputs as mi

pytestmark = pytest.mark.gpu

ALL_TYPES = list(range(12))
F32 = mi.F32
WIDE_TYPES = mi.WIDE_TYPES
SUM, PREMULSUM = mi.SUM, mi.PREMULSUM

# nbxDebugLaunchLog families and flags (include/nbx_debug.h)
SMALL, BIG, ELTS, LDS, RUNTIME, WIDE_PACKS, WIDE_ELTS = range(1, 8)
OUT32, PART_FIRST = 2, 4
FAMILY_NAMES = {SMALL: "small_packs", BIG: "big_packs", ELTS: "elements", LDS: "realign_lds",
                RUNTIME: "realign_runtime"}
VARIANT = {SMALL: 1, BIG: 2, ELTS: 0, LDS: 0, RUNTIME: 1}   # nbxSetLaunchConfig's variant that forces the family

PACKS, LDS_PACKS, ELT_COUNT = mi.PACKS, mi.LDS_PACKS, mi.ELT_COUNT
FRONT = 256          # guard bytes in front of every buffer (keeps the payload's offset modulo 128)
MAX_SRCS, MAX_WIDE_SRCS, MAX_DSTS = mi.MAX_SRCS, mi.MAX_WIDE_SRCS, 8


def unroll_cap(dtype, devop):
    """Fn::kUnrollCap (nbx_functors.h): fp8 functors 4; byte integers 4 but for Sum; 16 otherwise."""
    if dtype in (mi.E4M3, mi.E5M2):
        return 4
    if dtype in (0, 1):
        return 16 if devop == SUM else 4
    return 16


def big_unroll(nsrc, dtype, devop):
    return min(4 if nsrc >= 5 else 8 if nsrc >= 3 else 16, unroll_cap(dtype, devop))


def expected_unroll(family, nsrc, dtype, devop):
    if family == BIG:
        return big_unroll(nsrc, dtype, devop)
    if family == LDS:
        return 2 if nsrc >= 3 else 1
    if family == WIDE_PACKS:
        return 4 if nsrc >= 4 else 1
    return 1


def shared_misalignment(eb):
    return (3 * eb) % 16 or eb


# ---------------------------------------------------------------------------
# per-type state: host inputs, device uploads per layout, expected results

class TypeState:
    """Everything the cases of one datatype share. Sources are generated once at
    the longest count and used by prefix (the fold is element-wise, so the
    expected result of a prefix is the prefix of the expected result)."""

    def __init__(self, torch, oracle, dtype):
        self.torch, self.oracle, self.dtype = torch, oracle, dtype
        self.st = np.dtype(oracle.NP_STORAGE[dtype])
        self.eb = self.st.itemsize
        self.epp = 16 // self.eb
        self.n_max = mi.max_count(self.eb)
        self.srcs = mi.matrix_inputs(oracle, dtype)
        self.wide_srcs = None
        self.uploads = {}
        self.expected = {}
        deb = 4 if dtype in WIDE_TYPES else self.eb
        self.dst_row = (FRONT + self.n_max * deb + 16 + 256 + 255) // 256 * 256
        self.dst = torch.full((MAX_DSTS, self.dst_row), 0xA5, dtype=torch.uint8, device="cuda")
        self.scalar = torch.zeros(16, dtype=torch.uint8, device="cuda")
        assert self.dst.data_ptr() % 256 == 0 and self.scalar.data_ptr() % 16 == 0

    def src_ptrs(self, offs):
        """Device pointers of the sources placed `offs[k]` bytes past a 256-byte boundary."""
        offs = tuple(offs)
        if offs not in self.uploads:
            row = (FRONT + self.n_max * self.eb + 16 + 256 + 255) // 256 * 256
            host = np.full((len(offs), row), 0xA5, dtype=np.uint8)
            for k, o in enumerate(offs):
                host[k, FRONT + o:FRONT + o + self.n_max * self.eb] = self.srcs[k].view(np.uint8)
            t = self.torch.from_numpy(host).cuda()
            assert t.data_ptr() % 256 == 0
            self.uploads[offs] = (t, [t.data_ptr() + k * row + FRONT + o for k, o in enumerate(offs)])
        return self.uploads[offs][1]

    def expect(self, nsrc, devop, arg, npre, post):
        key = (nsrc, devop, arg, npre, post)
        if key not in self.expected:
            self.expected[key] = self.oracle.reduce_multi(self.srcs[:nsrc], self.dtype, devop, arg, npre, post,
                                                          threads=8)[0]
        return self.expected[key]

    def expect_wide(self, nsrc, out32, devop, arg, npre):
        key = ("wide", nsrc, out32, devop, arg, npre)
        if key not in self.expected:
            if self.wide_srcs is None:
                self.wide_srcs = [mi.widen(self.oracle, s, self.dtype) for s in self.srcs]
            fkey = ("fold", nsrc, devop, arg, npre)
            if fkey not in self.expected:
                self.expected[fkey] = self.oracle.reduce_multi(self.wide_srcs[:nsrc], F32, devop, arg, npre,
                                                               threads=8)[0]
            fold = self.expected[fkey]
            self.expected[key] = fold if out32 else mi.narrow(self.oracle, fold, self.dtype)
        return self.expected[key]

    def set_scalar(self, value, nbytes):
        raw = np.array([value], dtype=np.uint64).view(np.uint8)[:nbytes].copy()
        self.scalar[:nbytes].copy_(self.torch.from_numpy(raw))
        return self.scalar.data_ptr()


_STATE = {}


def state_for(torch, oracle, dtype):
    """The datatype's TypeState, kept for the module: every family reuses the
    uploads and the expected results (some 15 MB of host memory per type)."""
    if dtype not in _STATE:
        _STATE[dtype] = TypeState(torch, oracle, dtype)
    return _STATE[dtype]


@pytest.fixture(scope="module", autouse=True)
def _release_state():
    yield
    _STATE.clear()


@pytest.fixture
def launch_variant(nbx):
    saved = nbx.get_launch_config()

    def force(variant):
        nbx.set_launch_config(0, variant)
    yield force
    nbx.set_launch_config(*saved)


# ---------------------------------------------------------------------------
# one call, checked

def check_call(nbx, ts, call, dst_offs, count, deb, out_np, exp, exp_dtype, records, what):
    """Refills the destinations with 0xA5, runs `call(dst_ptrs)`, then checks
    every destination against `exp`, the guard bytes around it, and the launch
    record against `records`."""
    exp = exp[:count]
    share = mi.nan_share(exp, exp_dtype)
    assert share <= mi.NAN_CAP, f"{what}: {share:.1%} of the oracle's result is NaN"
    ndst = len(dst_offs)
    ts.dst.fill_(0xA5)
    base = ts.dst.data_ptr()
    ptrs = [base + d * ts.dst_row + FRONT + o for d, o in enumerate(dst_offs)]
    nbx.launch_log_reset()
    call(ptrs)
    total, recs = nbx.launch_log()
    rows = ts.dst[:ndst].cpu().numpy()   # synchronizes with the stream
    assert (total, recs) == (len(records), records), f"{what}: launch record {recs} (of {total}), wanted {records}"
    nbytes = count * deb
    for d, o in enumerate(dst_offs):
        lo = FRONT + o
        try:
            mi.assert_same(rows[d, lo:lo + nbytes].view(out_np), exp, exp_dtype)
        except AssertionError as e:
            raise AssertionError(f"{what}, destination {d}: {e}") from None
        assert (rows[d, :lo] == 0xA5).all() and (rows[d, lo + nbytes:] == 0xA5).all(), \
            f"{what}: bytes around destination {d} were written"
    if ndst < MAX_DSTS:
        assert bool((ts.dst[ndst:] == 0xA5).all()), f"{what}: an unused destination buffer was written"


def run_per_step(nbx, ts, family, nsrc, case, ndst, src_offs, dst_offs, count):
    label, devop, arg, npre, post, on_device = case
    dtype = ts.dtype
    op = nbx.DevRedOpFull()
    op.op = devop
    if on_device:
        op.scalarArgIsPtr = 1
        op.scalarArg = ts.set_scalar(arg, ts.eb)
    else:
        op.scalarArg = arg
    sp = ts.src_ptrs(src_offs)[:nsrc]
    stream = ts.torch.cuda.current_stream().cuda_stream
    exp = ts.expect(nsrc, devop, arg, npre, post)
    records = [(family, nsrc, expected_unroll(family, nsrc, dtype, devop), 0)]
    what = f"{FAMILY_NAMES[family]} {ts.oracle.TYPE_NAMES[dtype]} {label} nsrc={nsrc} ndst={ndst} count={count}"
    check_call(nbx, ts, lambda dp: nbx.reduce_multi(dp, sp, count, dtype, op, npre, post, stream), dst_offs, count,
               ts.eb, ts.st, exp, dtype, records, what)


class DstCycle:
    """1, 2, 3, 1, ... destinations (from `first`), and 8 once."""

    def __init__(self, first=1):
        self.i, self.first, self.eight_done = 0, first, False

    def next(self, want_eight=False):
        if want_eight and not self.eight_done:
            self.eight_done = True
            return 8
        n = self.first + self.i % 3
        self.i += 1
        return n


# ---------------------------------------------------------------------------
# nbxReduceMulti: family x type, every op and source count inside

@pytest.mark.parametrize("dtype", ALL_TYPES)
@pytest.mark.parametrize("family", [SMALL, BIG], ids=lambda f: FAMILY_NAMES[f])
def test_pack_kernels(nbx, oracle, torch_gpu, launch_variant, family, dtype):
    """kReducePacks<Fn, NSRC, U>: U = 1 (variant 1) and the functor's big-tile
    unroll (variant 2), all pointers on one misalignment: 0 for every op, and
    (3 * eb) % 16 for every source count with the ops taking turns."""
    ts = state_for(torch_gpu, oracle, dtype)
    launch_variant(VARIANT[family])
    eb, epp = ts.eb, ts.epp
    dsts = DstCycle()
    count = PACKS * epp + epp - 1   # aligned: no head
    for nsrc in range(1, MAX_SRCS + 1):
        for case in mi.op_cases(oracle, dtype, nsrc):
            ndst = dsts.next(want_eight=(nsrc == 8 and case[1] == SUM))
            run_per_step(nbx, ts, family, nsrc, case, ndst, [0] * MAX_SRCS, [0] * ndst, count)
    mis = shared_misalignment(eb)
    head = (128 - mis) // eb            # the library peels to the destination's 128-byte line
    count = head + PACKS * epp + epp - 1
    for nsrc in range(1, MAX_SRCS + 1):
        cases = mi.op_cases(oracle, dtype, nsrc)
        ndst = dsts.next()
        run_per_step(nbx, ts, family, nsrc, cases[(nsrc + dtype) % len(cases)], ndst, [mis] * MAX_SRCS, [mis] * ndst,
                     count)


@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_element_kernel(nbx, oracle, torch_gpu, launch_variant, dtype):
    """kReduceElts<Fn>: destinations at offsets 0 and eb (no shared alignment
    on the destination side), sources aligned."""
    ts = state_for(torch_gpu, oracle, dtype)
    launch_variant(VARIANT[ELTS])
    dsts = DstCycle(first=2)
    for nsrc in range(1, MAX_SRCS + 1):
        for case in mi.op_cases(oracle, dtype, nsrc):
            ndst = dsts.next(want_eight=(nsrc == 8 and case[1] == SUM))
            run_per_step(nbx, ts, ELTS, nsrc, case, ndst, [0] * MAX_SRCS, [(d % 2) * ts.eb for d in range(ndst)],
                         ELT_COUNT)


@pytest.mark.parametrize("dtype", ALL_TYPES)
@pytest.mark.parametrize("family", [LDS, RUNTIME], ids=lambda f: FAMILY_NAMES[f])
def test_realigning_kernels(nbx, oracle, torch_gpu, launch_variant, family, dtype):
    """kReduceShiftedLds<Fn, NSRC> (variant 0) and kReduceShifted<Fn> (variant
    1): source k at ((3k + 1) * eb) % 16, the destinations together at 0 (odd
    source counts) or (2 * eb) % 16 (even)."""
    ts = state_for(torch_gpu, oracle, dtype)
    launch_variant(VARIANT[family])
    eb, epp = ts.eb, ts.epp
    src_offs = [((3 * k + 1) * eb) % 16 for k in range(MAX_SRCS)]
    count = LDS_PACKS * epp + epp - 1
    dsts = DstCycle()
    for nsrc in range(1, MAX_SRCS + 1):
        dst_off = 0 if nsrc % 2 else (2 * eb) % 16
        for case in mi.op_cases(oracle, dtype, nsrc):
            ndst = dsts.next(want_eight=(nsrc == 8 and case[1] == SUM))
            run_per_step(nbx, ts, family, nsrc, case, ndst, src_offs, [dst_off] * ndst, count)


# ---------------------------------------------------------------------------
# nbxReduceMultiWide

def run_wide(nbx, ts, nsrc, out32, case, on_device, ndst, src_off, dst_offs, count, family):
    oracle, st = ts.oracle, ts.dtype
    devop, arg, npre = case
    op = nbx.DevRedOpFull()
    op.op = devop
    if devop == PREMULSUM and on_device:
        op.scalarArgIsPtr = 1
        op.scalarArg = ts.set_scalar(arg, 4)
    else:
        op.scalarArg = arg
    dt = F32 if out32 else st
    out_np = np.dtype(np.float32) if out32 else ts.st
    sp = ts.src_ptrs([src_off] * MAX_WIDE_SRCS)[:nsrc]
    stream = ts.torch.cuda.current_stream().cuda_stream
    exp = ts.expect_wide(nsrc, out32, devop, arg, npre)
    o32 = OUT32 if out32 else 0
    un = (lambda n: expected_unroll(family, n, st, devop))
    if nsrc <= 8:
        records = [(family, nsrc, un(nsrc), o32)]
    else:   # a first pass of 8 into the fp32 partial, then the partial and the other sources
        records = [(family, 8, un(8), OUT32), (family, nsrc - 7, un(nsrc - 7), o32 | PART_FIRST)]
    what = (f"wide {'packs' if family == WIDE_PACKS else 'elements'} {oracle.TYPE_NAMES[st]} -> "
            f"{'fp32' if out32 else 'same'} {'premulsum npre=%d' % npre if devop == PREMULSUM else 'sum'} "
            f"nsrc={nsrc} ndst={ndst} count={count}")
    check_call(nbx, ts, lambda dp: nbx.reduce_multi_wide(dp, sp, count, st, dt, op, npre, stream), dst_offs, count,
               out_np.itemsize, out_np, exp, dt, records, what)


@pytest.mark.parametrize("out32", [False, True], ids=["same", "fp32"])
@pytest.mark.parametrize("st", WIDE_TYPES)
def test_wide_pack_kernels(nbx, oracle, torch_gpu, st, out32):
    """kWidePacks<W, NSRC, U, OUT32, PART>: 1..8 sources first-pass, and 9..15
    sources as a first pass of 8 and a partial-first pass of 2..8 slots."""
    ts = state_for(torch_gpu, oracle, st)
    eb, epp = ts.eb, ts.epp
    dsts = DstCycle()
    count = PACKS * epp + epp - 1
    for nsrc in range(1, MAX_WIDE_SRCS + 1):
        for case in mi.wide_cases(oracle, st, nsrc):
            ndst = dsts.next(want_eight=(nsrc == 8 and case[0] == SUM))
            run_wide(nbx, ts, nsrc, out32, case, nsrc % 2 == 1, ndst, 0, [0] * ndst, count, WIDE_PACKS)
    # one shared misalignment: the head elements bring the sources to a 16-byte
    # boundary, and the destination has to be on one behind them
    mis = shared_misalignment(eb)
    head = (16 - mis) // eb
    dst_off = (-4 * head) % 16 if out32 else mis
    count = head + PACKS * epp + epp - 1
    for nsrc in range(1, MAX_WIDE_SRCS + 1):
        case = mi.wide_cases(oracle, st, nsrc)[(nsrc + st) % 2]
        ndst = dsts.next()
        run_wide(nbx, ts, nsrc, out32, case, nsrc % 2 == 0, ndst, mis, [dst_off] * ndst, count, WIDE_PACKS)


@pytest.mark.parametrize("st", WIDE_TYPES)
def test_wide_element_kernels(nbx, oracle, torch_gpu, st):
    """kWideElts<W, OUT32, PART>: aligned sources and a destination that is not
    16-byte aligned, 3 sources (one pass) and 11 (8, then partial + 3)."""
    ts = state_for(torch_gpu, oracle, st)
    for out32 in (False, True):
        off = 4 if out32 else ts.eb
        for nsrc in (3, 11):
            for k, case in enumerate(mi.wide_cases(oracle, st, nsrc)):
                ndst = 1 + (nsrc + k) % 2
                run_wide(nbx, ts, nsrc, out32, case, nsrc == 11, ndst, 0, [off, 0][:ndst], ELT_COUNT, WIDE_ELTS)
