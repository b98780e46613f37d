"""nbxReduceMultiWide's realigning kernel — every kWideShiftedLds<W, NSRC,
OUT32, PART> instantiation (4 source types x {source-type, fp32} output x 1..8
first-pass and 2..8 partial-first sources), its edge shapes, its two-stage
pipeline, graph capture, the dispatch policy and the batch — against the oracle
route of the wide tests: widen through the oracle's codecs, the oracle's
ordered fp32 fold, one narrowing; bit for bit, NaN compared as NaN.

Sources sit on misalignments of their own (tests/wideshift/__init__.py), the
destinations together on one; the expected value does not depend on either.
Every case sets the realigning threshold to 1 through
nbxDebugSetWideShiftMinElts unless it says otherwise and restores it, asserts
its exact launch record (family 16), and checks the 0xA5 guards around every
destination and in the unused destination rows.

The file carries the parity core's name on purpose, as tests/wide/ and
tests/widebatch/ do: the GPU suite orders files by name (tests/conftest.py)."""
import numpy as np
import pytest

from tests import widebatch as wb
from tests import wideshift as ws
from tests.batch import cases as bc
from tests.matrix import inputs as mi
from tests.matrix.test_reduce_gpu import FRONT, MAX_DSTS, DstCycle, TypeState, check_call

pytestmark = pytest.mark.gpu

F32, BF16, E4M3, E5M2 = mi.F32, mi.BF16, mi.E4M3, mi.E5M2
SUM, PREMULSUM = mi.SUM, mi.PREMULSUM
SHIFT, ELTS, PACKS = ws.FAM_WIDE_SHIFT, ws.FAM_WIDE_ELTS, ws.FAM_WIDE_PACKS

_STATE = {}
_PIPE = {}


def state_for(torch, oracle, st):
    if st not in _STATE:
        _STATE[st] = TypeState(torch, oracle, st)
    return _STATE[st]


@pytest.fixture(scope="module", autouse=True)
def _release_state():
    yield
    _STATE.clear()
    _PIPE.clear()


@pytest.fixture
def shift_min(nbx):
    """Threshold 1 for the test; yields (setter, the threshold found), restores it."""
    saved = nbx.set_wide_shift_min_elts(0)
    nbx.set_wide_shift_min_elts(1)
    yield nbx.set_wide_shift_min_elts, saved
    nbx.set_wide_shift_min_elts(saved)


@pytest.fixture
def launch_config(nbx):
    saved = nbx.get_launch_config()
    nbx.set_launch_config(0, 0)
    yield nbx.set_launch_config
    nbx.set_launch_config(*saved)


def make_op(nbx, ts, case, on_device):
    devop, arg, _ = case
    op = nbx.DevRedOpFull()
    op.op = devop
    if devop == PREMULSUM and on_device:
        op.scalarArgIsPtr = 1
        op.scalarArg = ts.set_scalar(arg, 4)
    else:
        op.scalarArg = arg
    return op


def describe(ts, out32, case, nsrc, ndst, count):
    op = "premulsum npre=%d" % case[2] if case[0] == PREMULSUM else "sum"
    return f"{ts.oracle.TYPE_NAMES[ts.dtype]} -> {'fp32' if out32 else 'same'} {op} nsrc={nsrc} ndst={ndst} count={count}"


def run_shift(nbx, ts, nsrc, out32, case, on_device, src_offs, dst_offs, count, family=SHIFT, label="wide realign"):
    """One nbxReduceMultiWide call over the matrix inputs placed at `src_offs`,
    checked by tests/matrix's check_call (result, guards, exact record)."""
    st = ts.dtype
    op = make_op(nbx, ts, case, on_device)
    dt = F32 if out32 else st
    out_np = np.dtype(np.float32) if out32 else ts.st
    sp = ts.src_ptrs(src_offs)[:nsrc]
    stream = ts.torch.cuda.current_stream().cuda_stream
    exp = ts.expect_wide(nsrc, out32, *case)
    eb = ts.eb
    if family != PACKS:   # the policy the record is expected from, restated
        addrs = [256 + FRONT + o for o in src_offs[:nsrc]], [256 + FRONT + o for o in dst_offs]
        want = ws.REALIGN if family == SHIFT else ws.ELEMENTS
        assert ws.layout(*addrs, count, eb, out32, nbx.set_wide_shift_min_elts(0))[0] == want
    check_call(nbx, ts, lambda dp: nbx.reduce_multi_wide(dp, sp, count, st, dt, op, case[2], stream), dst_offs, count,
               out_np.itemsize, out_np, exp, dt, ws.records(family, nsrc, out32),
               f"{label} {describe(ts, out32, case, nsrc, len(dst_offs), count)}")


# ---------------------------------------------------------------------------
# 1. the instantiation matrix

@pytest.mark.parametrize("out32", [False, True], ids=["same", "fp32"])
@pytest.mark.parametrize("st", mi.WIDE_TYPES)
def test_wide_realigning_kernels(nbx, oracle, torch_gpu, shift_min, launch_config, st, out32):
    """kWideShiftedLds<W, NSRC, OUT32, PART>: 1..8 sources first-pass, 9..15 as
    a first pass of 8 and a partial-first pass of 2..8 slots; Sum and
    PreMulSum, the scalar by value (even counts) or on the device (odd)."""
    ts = state_for(torch_gpu, oracle, st)
    eb, epp = ts.eb, ts.epp
    src_offs = ws.src_offsets(eb)
    count = ws.matrix_count(epp)
    dsts = DstCycle()
    for nsrc in range(1, mi.MAX_WIDE_SRCS + 1):
        dst_off = ws.matrix_dst_offset(nsrc, eb, out32)
        for case in mi.wide_cases(oracle, st, nsrc):
            ndst = dsts.next(want_eight=(nsrc == 8 and case[0] == SUM))
            run_shift(nbx, ts, nsrc, out32, case, nsrc % 2 == 1, src_offs, [dst_off] * ndst, count)


# ---------------------------------------------------------------------------
# 2. edge shapes

@pytest.mark.parametrize("out32", [False, True], ids=["same", "fp32"])
@pytest.mark.parametrize("st", ws.EDGE_TYPES)
def test_wide_realigning_edge_shapes(nbx, oracle, torch_gpu, shift_min, launch_config, st, out32):
    """One element, less than the head, the head alone, a body of 0 packs (no
    DMA may be issued), one pack, exactly one wave tile, a workgroup tile and a
    pack, and sources of which some need no shift."""
    ts = state_for(torch_gpu, oracle, st)
    eb = ts.eb
    dst_off = ws.shared_dst_offset(eb, out32)
    dsts = DstCycle()
    for nsrc in ws.EDGE_SRCS:
        cases = mi.wide_cases(oracle, st, nsrc)
        for k, (name, count, src_offs) in enumerate(ws.edge_shapes(eb, out32, nsrc)):
            ndst = dsts.next()
            run_shift(nbx, ts, nsrc, out32, cases[k % 2], k % 4 < 2, src_offs, [dst_off] * ndst, count,
                      label=f"wide realign, {name},")


def test_wide_realigning_in_place(nbx, oracle, torch_gpu, shift_min, launch_config):
    """Source-type output on source 1 of 3 (bf16): that source needs no shift,
    the others do; the other sources and every guard byte stay what they were."""
    torch = torch_gpu
    ts = state_for(torch, oracle, BF16)
    eb, epp, nsrc = ts.eb, ts.epp, 3
    count = ws.matrix_count(epp)
    offs = ws.src_offsets(eb)[:nsrc]
    row = (FRONT + count * eb + 16 + 256 + 255) // 256 * 256
    host = np.full((nsrc, row), 0xA5, dtype=np.uint8)
    for k, o in enumerate(offs):
        host[k, FRONT + o:FRONT + o + count * eb] = ts.srcs[k][:count].view(np.uint8)
    dev = torch.from_numpy(host).cuda()
    sp = [dev.data_ptr() + k * row + FRONT + o for k, o in enumerate(offs)]
    assert ws.layout(sp, [sp[1]], count, eb, False, 1) == (ws.REALIGN, ws.head_of(offs[1], eb, False))
    case = mi.wide_cases(oracle, BF16, nsrc)[1]
    exp = ts.expect_wide(nsrc, False, *case)[:count]
    op = make_op(nbx, ts, case, False)
    nbx.launch_log_reset()
    nbx.reduce_multi_wide([sp[1]], sp, count, BF16, BF16, op, case[2], torch.cuda.current_stream().cuda_stream)
    total, recs = nbx.launch_log()
    got = dev.cpu().numpy()
    assert (total, recs) == (1, ws.records(SHIFT, nsrc, False))
    lo = FRONT + offs[1]
    mi.assert_same(got[1, lo:lo + count * eb].view(ts.st), exp, BF16)
    want = host.copy()
    want[1, lo:lo + count * eb] = got[1, lo:lo + count * eb]
    assert np.array_equal(got, want), "a byte outside the destination was written"


# ---------------------------------------------------------------------------
# 3. the pipeline: more than one tile per wave

def pipe_state(torch, oracle, st, cus):
    """Inputs of the pipeline shape for one type: 11 sources of the matrix
    generator at the longest count (three or more sources: 128-pack wave
    tiles), uploaded at the matrix's source offsets; folds cached per call."""
    if st not in _PIPE:
        eb = np.dtype(oracle.NP_STORAGE[st]).itemsize
        n = ws.pipe_count(cus, 8, 16 // eb)
        srcs = mi.edge_inputs(oracle, st, max(ws.PIPE_SRCS), n, ws.PIPE_SEED + st)
        ups, ptrs = [], []
        for k, o in enumerate(ws.src_offsets(eb, len(srcs))):
            host = np.full(FRONT + n * eb + 256, 0xA5, dtype=np.uint8)
            host[FRONT + o:FRONT + o + n * eb] = srcs[k].view(np.uint8)
            t = torch.from_numpy(host).cuda()
            assert t.data_ptr() % 256 == 0
            ups.append(t)
            ptrs.append(t.data_ptr() + FRONT + o)
        _PIPE[st] = {"srcs": srcs, "ups": ups, "ptrs": ptrs, "fold": {}}
    return _PIPE[st]


def call_on_own_arena(nbx, torch, oracle, st, out32, sp, count, exp, ndst, op, npre, family, what):
    """One nbxReduceMultiWide call of the sources at `sp` into `ndst` aligned
    rows of a fresh 0xA5 arena with one more row: the NaN share of `exp`, the
    mirror's layout, the exact record, every destination bit for bit, the
    guards around them and the unused row."""
    eb = np.dtype(oracle.NP_STORAGE[st]).itemsize
    dt = F32 if out32 else st
    out_np = np.dtype(np.float32) if out32 else np.dtype(oracle.NP_STORAGE[st])
    exp = exp[:count]
    share = mi.nan_share(exp, dt)
    assert share <= mi.NAN_CAP, f"{what}: {share:.1%} of the oracle's result is NaN"
    nbytes = count * out_np.itemsize
    arena = torch.full((ndst + 1, (FRONT + nbytes + 256 + 255) // 256 * 256), 0xA5, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 256 == 0
    dp = [arena.data_ptr() + d * arena.shape[1] + FRONT for d in range(ndst)]
    want_layout = (ws.REALIGN, 0) if family == SHIFT else (ws.ELEMENTS, 0)
    assert ws.layout(sp, dp, count, eb, out32, nbx.set_wide_shift_min_elts(0)) == want_layout
    nbx.launch_log_reset()
    nbx.reduce_multi_wide(dp, sp, count, st, dt, op, npre, torch.cuda.current_stream().cuda_stream)
    total, recs = nbx.launch_log()
    rows = arena.cpu().numpy()
    want = ws.records(family, len(sp), out32)
    assert (total, recs) == (len(want), want), f"{what}: launch record {recs} (of {total}), wanted {want}"
    for d in range(ndst):
        try:
            mi.assert_same(rows[d, FRONT:FRONT + nbytes].view(out_np), exp, dt)
        except AssertionError as e:
            raise AssertionError(f"{what}, destination {d}: {e}") from None
        assert (rows[d, :FRONT] == 0xA5).all() and (rows[d, FRONT + nbytes:] == 0xA5).all(), \
            f"{what}: bytes around destination {d} were written"
    assert (rows[ndst] == 0xA5).all(), f"{what}: the unused destination row was written"


@pytest.mark.parametrize("out32", [False, True], ids=["same", "fp32"])
@pytest.mark.parametrize("nsrc", ws.PIPE_SRCS)
@pytest.mark.parametrize("st", ws.PIPE_TYPES)
def test_wide_realigning_pipeline(nbx, oracle, torch_gpu, shift_min, launch_config, st, nsrc, out32):
    """One workgroup per CU, so waves = 4 x CUs; 3 x waves + 5 wave tiles: five
    waves run four tiles, the rest three (prologue, steady state, drain), the
    last tile ragged at 37 packs, then EPP - 1 tail elements."""
    torch = torch_gpu
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    launch_config(1, 0)
    ps = pipe_state(torch, oracle, st, cus)
    eb = ps["srcs"][0].itemsize
    epp = 16 // eb
    count = ws.pipe_count(cus, nsrc, epp)
    packs = ws.pipe_packs(cus, nsrc)
    wave_tile = ws.shift_unroll(min(nsrc, 8)) * ws.WAVE
    assert -(-packs // (ws.WAVES * wave_tile)) >= cus          # the grid is one workgroup per CU
    assert -(-packs // wave_tile) == 3 * ws.WAVES * cus + 5 and packs % wave_tile == 37
    case = mi.wide_cases(oracle, st, nsrc)[nsrc % 2]
    if (nsrc, case) not in ps["fold"]:
        ps["fold"].clear()   # one fold at a time: they are the size of four sources
        wide = [mi.widen(oracle, s[:count], st) for s in ps["srcs"][:nsrc]]
        ps["fold"][(nsrc, case)] = oracle.reduce_multi(wide, F32, case[0], case[1], case[2], threads=8)[0]
    fold = ps["fold"][(nsrc, case)]
    exp = fold if out32 else mi.narrow(oracle, fold, st)
    what = f"pipeline {oracle.TYPE_NAMES[st]} -> {'fp32' if out32 else 'same'} nsrc={nsrc} count={count}"
    ts = state_for(torch, oracle, st)   # the device scalar lives there
    op = make_op(nbx, ts, case, nsrc == 8)
    call_on_own_arena(nbx, torch, oracle, st, out32, ps["ptrs"][:nsrc], count, exp, 2 if nsrc == 3 else 1, op, case[2],
                      SHIFT, what)


# ---------------------------------------------------------------------------
# 4. graph capture

def fold_of(oracle, st, windows, out32, case=(SUM, 0, 0)):
    """The oracle route for sources given as arrays of raw codes."""
    fold = oracle.reduce_multi([mi.widen(oracle, w, st) for w in windows], F32, case[0], case[1], case[2], threads=8)[0]
    return fold if out32 else mi.narrow(oracle, fold, st)


def test_wide_realigning_graph_capture(nbx, oracle, torch_gpu, shift_min, launch_config):
    """One captured call (bf16, 3 sources, source-type output), replayed twice
    with the inputs changed between the replays."""
    torch = torch_gpu
    ts = state_for(torch, oracle, BF16)
    eb, epp, nsrc = ts.eb, ts.epp, 3
    count = ws.matrix_count(epp)
    offs = ws.src_offsets(eb)[:nsrc]
    bufs = [torch.full((FRONT + count * eb + 256,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(nsrc)]
    sp = [b.data_ptr() + FRONT + o for b, o in zip(bufs, offs)]
    dst_off = ws.shared_dst_offset(eb, False)
    out = torch.full((2, (FRONT + count * eb + 256 + 255) // 256 * 256), 0xA5, dtype=torch.uint8, device="cuda")
    assert all(b.data_ptr() % 256 == 0 for b in bufs) and out.data_ptr() % 256 == 0 and out.shape[1] % 256 == 0
    dp = [out.data_ptr() + FRONT + dst_off]
    assert ws.layout(sp, dp, count, eb, False, 1)[0] == ws.REALIGN
    op = nbx.DevRedOpFull()
    op.op = SUM
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    nbx.launch_log_reset()
    with torch.cuda.graph(g, stream=s):
        nbx.reduce_multi_wide(dp, sp, count, BF16, BF16, op, 0, torch.cuda.current_stream().cuda_stream)
    assert nbx.launch_log() == (1, ws.records(SHIFT, nsrc, False))
    for first in (0, 5):
        windows = [ts.srcs[first + k][:count] for k in range(nsrc)]
        for b, o, w in zip(bufs, offs, windows):
            b[FRONT + o:FRONT + o + count * eb].copy_(torch.from_numpy(w.view(np.uint8).copy()))
        out.fill_(0xA5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        rows = out.cpu().numpy()
        lo = FRONT + dst_off
        mi.assert_same(rows[0, lo:lo + count * eb].view(ts.st), fold_of(oracle, BF16, windows, False), BF16)
        assert (rows[0, :lo] == 0xA5).all() and (rows[0, lo + count * eb:] == 0xA5).all() and (rows[1] == 0xA5).all()


# ---------------------------------------------------------------------------
# 5. policy

def test_wide_realigning_policy(nbx, oracle, torch_gpu, shift_min, launch_config):
    """With the default threshold: a realigning layout one element below it
    runs the element kernel, at it the realigning kernel. Destinations on two
    alignments run the element kernel at any size, a pack layout the pack
    kernel whatever the threshold is; the launch variant changes nothing."""
    torch = torch_gpu
    set_min, default = shift_min
    sum_case = (SUM, 0, 0)
    assert default >= 4096 and default & (default - 1) == 0
    set_min(default)
    # two sources of `default` elements of their own (e5m2: 1 byte each), at the matrix's offsets
    st = ws.POLICY_TYPE
    srcs = mi.edge_inputs(oracle, st, 2, default, ws.POLICY_SEED)
    ups, sp = [], []
    for s, o in zip(srcs, ws.src_offsets(1)):
        host = np.full(FRONT + default + 256, 0xA5, dtype=np.uint8)
        host[FRONT + o:FRONT + o + default] = s.view(np.uint8)
        ups.append(torch.from_numpy(host).cuda())
        assert ups[-1].data_ptr() % 256 == 0
        sp.append(ups[-1].data_ptr() + FRONT + o)
    op = nbx.DevRedOpFull()
    op.op = SUM
    for out32 in (False, True):
        exp = fold_of(oracle, st, srcs, out32)
        for count, family in ((default - 1, ELTS), (default, SHIFT)):
            call_on_own_arena(nbx, torch, oracle, st, out32, sp, count, exp, 1, op, 0, family,
                              f"default threshold {default}, {count} elements, fp32={out32}")
    del ups
    ts = state_for(torch, oracle, BF16)
    eb, epp = ts.eb, ts.epp
    offs = ws.src_offsets(eb)
    count = ws.matrix_count(epp)
    for threshold in (1, default):
        set_min(threshold)
        for variant in (0, 1, 2):
            launch_config(0, variant)
            for out32 in (False, True):
                off = 4 if out32 else eb
                run_shift(nbx, ts, 3, out32, sum_case, False, offs, [0, off], count, family=ELTS,
                          label=f"destinations on two alignments, threshold {threshold}, variant {variant}")
                run_shift(nbx, ts, 3, out32, sum_case, False, [0] * mi.MAX_WIDE_SRCS, [0, 0], count, family=PACKS,
                          label=f"pack layout, threshold {threshold}, variant {variant}")
                if threshold == 1:
                    run_shift(nbx, ts, 3, out32, sum_case, False, offs, [0, 0], count,
                              label=f"realigning layout, variant {variant}")
        launch_config(0, 0)


# ---------------------------------------------------------------------------
# 6. the batch

@pytest.mark.parametrize("out32", [True, False], ids=["fp32", "same"])
def test_wide_batch_takes_the_realigning_kernel(nbx, oracle, torch_gpu, shift_min, launch_config, out32):
    """One nbxReduceMultiWideBatch call: a bucket whose sources lie on two
    misalignments and one whose destination is off its pack offset, each once
    above and once below the threshold (families 16 and 7, single buckets
    first, in bucket order), among pack-layout buckets (one family-15 launch
    behind them). Every bucket equals the oracle and its own nbxReduceMultiWide
    call, byte for byte."""
    torch = torch_gpu
    set_min, _ = shift_min
    lib = nbx.load_library()
    mode = lib.nbxDebugSetBatchMode(-1)
    lib.nbxDebugSetBatchMode(bc.MODE_DEFAULT)
    try:
        ts = state_for(torch, oracle, E4M3)
        st, eb, epp = ts.dtype, ts.eb, ts.epp
        deb = 4 if out32 else eb
        threshold = 1024
        set_min(threshold)
        big, small = 150 * epp + 5, 50 * epp + 3
        assert small < threshold <= big
        sp = ts.src_ptrs([0] * mi.MAX_WIDE_SRCS)
        off = 4 if out32 else eb
        # (name, sources, window starts in elements, destination offset in bytes past a 16-byte slot, count, family)
        specs = [("packs a", 2, [0, 0], 0, 40 * epp + 1, None),
                 ("mixed sources, above", 3, [0, 1, 0], 0, big, SHIFT),
                 ("mixed sources, below", 3, [16, 17, 16], 0, small, ELTS),
                 ("packs b", 2, [32, 32], 0, 1, None),
                 ("destination off, above", 2, [48, 48], off, big, SHIFT),
                 ("destination off, below", 2, [64, 64], off, small, ELTS)]
        slot = (big * deb + 64 + 15) // 16 * 16
        arena = torch.full((2, (FRONT + slot * len(specs) + 256 + 255) // 256 * 256), 0xA5, dtype=torch.uint8,
                           device="cuda")
        assert arena.data_ptr() % 256 == 0
        row = arena.shape[1]
        tasks, checks, singles = [], [], []
        for i, (name, nsrc, starts, doff, count, family) in enumerate(specs):
            srcs = [sp[k] + s * eb for k, s in enumerate(starts)]
            byte = FRONT + i * slot + doff
            dst = arena.data_ptr() + byte
            want = {None: ws.PACKS, SHIFT: ws.REALIGN, ELTS: ws.ELEMENTS}[family]
            assert ws.layout(srcs, [dst], count, eb, out32, threshold)[0] == want, name
            tasks.append(([dst], srcs, count))
            windows = [ts.srcs[k][s:s + count] for k, s in enumerate(starts)]
            checks.append((name, byte, fold_of(oracle, st, windows, out32)))
            if family is not None:
                singles += ws.records(family, nsrc, out32)
        want = singles + wb.records(2, [2], out32)
        dt = F32 if out32 else st
        op = nbx.DevRedOpFull()
        op.op = SUM
        stream = torch.cuda.current_stream().cuda_stream
        nbx.launch_log_reset()
        nbx.reduce_multi_wide_batch(tasks, st, dt, op, 0, stream)
        total, recs = nbx.launch_log()
        assert (total, recs) == (len(want), want), f"launch record {recs} (of {total}), wanted {want}"
        for dsts, srcs, count in tasks:
            nbx.reduce_multi_wide([p + row for p in dsts], srcs, count, st, dt, op, 0, stream)
        rows = arena.cpu().numpy()
        out_np = np.dtype(np.float32) if out32 else ts.st
        untouched = np.ones(row, dtype=bool)
        for name, byte, exp in checks:
            try:
                mi.assert_same(rows[0, byte:byte + exp.size * deb].view(out_np), exp, dt)
            except AssertionError as e:
                raise AssertionError(f"bucket '{name}': {e}") from None
            untouched[byte:byte + exp.size * deb] = False
        assert (rows[0, untouched] == 0xA5).all(), "bytes outside every bucket's destination were written"
        assert np.array_equal(rows[0], rows[1]), "the batched call and the per-bucket calls differ"
    finally:
        lib.nbxDebugSetBatchMode(mode)
