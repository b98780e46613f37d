"""nbxReduceMultiWideBatch — every kWideBatchList<W, NSRC, OUT32> instantiation
(4 source types x {source-type, fp32} output x 1..8 sources) and the call's
launch policy — against the oracle route of the wide tests: widen through the
oracle's codecs, the oracle's ordered fp32 fold, one narrowing; bit for bit,
NaN compared as NaN.

The buckets are tests/batch/cases.py's (one element, below a pack, head only,
clipped head, exact tile, tile + pack, ragged three tiles, empty; the
scheduler shapes list_walk and record_width), the inputs tests/matrix/inputs.py's
edge-rich values through tests/matrix/test_reduce_gpu.py's TypeState. An fp32
destination stretch starts at its bucket's `dstart` counted in floats, which
keeps it 16-byte aligned behind the head (tests/test_wide_batch_cpu.py).

Every call is checked three ways: the launch record (nbxDebugLaunchLog, family
15 for a work-list launch, 6 / 7 for a bucket that ran alone) matches exactly,
every destination stretch matches its expected value, and every other byte of
the 0xA5-filled destination arena is untouched.

The file carries the parity core's name on purpose, as tests/wide/ and
tests/batch/ do: the GPU suite orders files by name (tests/conftest.py)."""
import ctypes
import os

import numpy as np
import pytest

from tests import widebatch as wb
from tests.batch import cases as bc
from tests.matrix import inputs as mi
from tests.matrix.test_reduce_gpu import FRONT, TypeState

pytestmark = pytest.mark.gpu

F16, F32, BF16, E4M3, E5M2 = mi.F16, mi.F32, mi.BF16, mi.E4M3, mi.E5M2
SUM, PREMULSUM = mi.SUM, mi.PREMULSUM
SUM_CASE = (SUM, 0, 0)

_STATE = {}


def state_for(torch, oracle, st):
    if st not in _STATE:
        _STATE[st] = TypeState(torch, oracle, st)
    return _STATE[st]


@pytest.fixture(scope="module", autouse=True)
def _release_state():
    yield
    _STATE.clear()


@pytest.fixture
def batch_mode(nbx):
    lib = nbx.load_library()
    saved = lib.nbxDebugSetBatchMode(-1)
    yield lib.nbxDebugSetBatchMode
    lib.nbxDebugSetBatchMode(saved)


@pytest.fixture
def launch_config(nbx):
    saved = nbx.get_launch_config()
    yield nbx.set_launch_config
    nbx.set_launch_config(*saved)


# ---------------------------------------------------------------------------
# one call, checked

def new_arena(torch, rows, payload_bytes):
    """`rows` destination rows: FRONT guard bytes, the payload, a guard behind it."""
    row = (FRONT + payload_bytes + 256 + 255) // 256 * 256
    t = torch.empty((rows, row), dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    return t


def row_ptr(arena, row, byte):
    return arena.data_ptr() + row * arena.shape[1] + FRONT + byte


def from_buckets(ts, arena, sp, buckets, nsrc, exp, out32):
    """(tasks, checks) of buckets that read windows of the sources at `sp` and
    write `arena`, stretches counted in destination elements; `exp` is the
    expected result over the whole sources."""
    deb = 4 if out32 else ts.eb
    tasks, checks = [], []
    for b in buckets:
        tasks.append(([row_ptr(arena, r, b.dstart * deb) for r in b.rows],
                      [p + b.start * ts.eb for p in sp[:nsrc]], b.count))
        checks.append((b.name, b.rows, b.dstart * deb, exp[b.start:b.start + b.count]))
    return tasks, checks


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


def check_arena(ts, arena, checks, out32, what, background=None):
    """Every (name, rows, byte offset, expected) of `checks` bit for bit, every
    other byte of the arena what it was; returns the arena's host image."""
    out_np = np.dtype(np.float32) if out32 else ts.st
    out_t = F32 if out32 else ts.dtype
    rows = arena.cpu().numpy()   # synchronizes with the stream
    untouched = np.ones(rows.shape, dtype=bool)
    for name, drows, off, exp in checks:
        lo = FRONT + off
        hi = lo + exp.size * out_np.itemsize
        for d, r in enumerate(drows):
            try:
                mi.assert_same(rows[r, lo:hi].view(out_np), exp, out_t)
            except AssertionError as e:
                raise AssertionError(f"{what}, bucket '{name}', destination {d}: {e}") from None
            untouched[r, lo:hi] = False
    was = 0xA5 if background is None else background[untouched]
    bad = np.flatnonzero(rows[untouched] != was)
    if bad.size:
        r, c = (a[bad[0]] for a in np.nonzero(untouched))
        raise AssertionError(f"{what}: {bad.size} bytes outside every bucket's destinations were written, the first "
                             f"in row {r} at byte {c - FRONT} of the payload")
    return rows


def run_call(nbx, ts, arena, tasks, checks, out32, case, on_device, want, what, background=None):
    """Refills `arena` (0xA5, or `background`: a host image and its device
    copy), makes one nbxReduceMultiWideBatch call of `tasks`, then checks the
    launch record against `want` and the arena (check_arena)."""
    if background is None:
        arena.fill_(0xA5)
    else:
        arena.copy_(background[1])
    op = make_op(nbx, ts, case, on_device)
    stream = ts.torch.cuda.current_stream().cuda_stream
    nbx.launch_log_reset()
    nbx.reduce_multi_wide_batch(tasks, ts.dtype, F32 if out32 else ts.dtype, op, case[2], stream)
    total, recs = nbx.launch_log()
    rows = check_arena(ts, arena, checks, out32, what, None if background is None else background[0])
    assert (total, recs) == (len(want), want), f"{what}: launch record {recs} (of {total}), wanted {want}"
    return rows


def what_of(ts, out32, case, nsrc):
    op = "premulsum npre=%d" % case[2] if case[0] == PREMULSUM else "sum"
    return f"wide batch {ts.oracle.TYPE_NAMES[ts.dtype]} -> {'fp32' if out32 else 'same'} {op} nsrc={nsrc}"


def table_arena(ts, out32, rows=bc.MAX_DSTS):
    return new_arena(ts.torch, rows, 1216 * ts.epp * (4 if out32 else ts.eb))   # the table ends below 1,200 packs


# ---------------------------------------------------------------------------
# 1. the instantiation matrix

@pytest.mark.parametrize("out32", [False, True], ids=["same", "fp32"])
@pytest.mark.parametrize("st", mi.WIDE_TYPES)
def test_wide_batch_kernels(nbx, oracle, torch_gpu, batch_mode, launch_config, st, out32):
    """One call of cases.py's table per (source count, op): all seven non-empty
    buckets in one launch of kWideBatchList<W, nsrc, out32>, destination counts
    cycling 1..8 across the buckets, the PreMulSum scalar by value (even source
    counts) or in device memory (odd)."""
    ts = state_for(torch_gpu, oracle, st)
    batch_mode(bc.MODE_DEFAULT)
    launch_config(0, 0)
    arena = table_arena(ts, out32)
    sp = ts.src_ptrs([0] * mi.MAX_WIDE_SRCS)
    call = 0
    for nsrc in range(1, mi.MAX_SRCS + 1):
        for case in mi.wide_cases(oracle, st, nsrc):
            ndsts = [1 + (7 * call + j) % 8 for j in range(7)]
            call += 1
            exp = ts.expect_wide(nsrc, out32, *case)
            what = what_of(ts, out32, case, nsrc)
            share = bc.nan_share_of_call(exp, ts.eb, F32 if out32 else st)
            assert share <= mi.NAN_CAP, f"{what}: {share:.1%} of the oracle's results is NaN"
            tasks, checks = from_buckets(ts, arena, sp, bc.table_buckets(ts.eb, ndsts), nsrc, exp, out32)
            run_call(nbx, ts, arena, tasks, checks, out32, case, nsrc % 2 == 1, wb.records(nsrc, [7], out32), what)


# ---------------------------------------------------------------------------
# 2, 3. scheduler shapes: one workgroup per CU (set_launch_config(1, 0))

def run_shape(nbx, oracle, torch, st, out32, case, buckets_of, nsrc, launches, rows=1):
    ts = state_for(torch, oracle, st)
    buckets = buckets_of(ts.eb)
    arena = new_arena(torch, rows, bc.arena_elts(buckets, ts.eb) * (4 if out32 else ts.eb))
    exp = ts.expect_wide(nsrc, out32, *case)
    tasks, checks = from_buckets(ts, arena, ts.src_ptrs([0] * mi.MAX_WIDE_SRCS), buckets, nsrc, exp, out32)
    run_call(nbx, ts, arena, tasks, checks, out32, case, True, wb.records(nsrc, launches, out32),
             what_of(ts, out32, case, nsrc))


def test_wide_batch_record_search(nbx, oracle, torch_gpu, batch_mode, launch_config):
    """list_walk's 400 two-source buckets in launches of 384 and 16: the
    search past the first 64 running totals, chunks crossing bucket boundaries
    and a second workgroup turn (the arithmetic of
    tests/batch/test_reduce_gpu.py::test_batch_list_record_search)."""
    cus = torch_gpu.cuda.get_device_properties(0).multi_processor_count
    chunk = max(1, int(os.environ.get("NBX_BATCH_CHUNK", "4") or 4))
    batch_mode(bc.MODE_DEFAULT)
    launch_config(1, 0)
    for eb in (2, 1):
        buckets = bc.list_walk(eb)
        assert bc.list_launches(len(buckets)) == [384, 16]
        tiles = bc.tiles_of(buckets[:384], eb)
        first = sum(tiles)
        assert first > chunk * cus, f"{first} tiles in the first launch: no workgroup takes a second turn"
        grid = min(-(-first // chunk), cus)
        assert chunk * (grid - 1) >= sum(tiles[:64]), "every workgroup's first tile lies in the first 64 records"
        assert chunk > 1 and tiles[0] < chunk
    premul = mi.wide_cases(oracle, E4M3, 2)[1]
    run_shape(nbx, oracle, torch_gpu, BF16, True, SUM_CASE, bc.list_walk, 2, [384, 16])
    run_shape(nbx, oracle, torch_gpu, E4M3, False, (premul[0], premul[1], 1), bc.list_walk, 2, [384, 16])


def test_wide_batch_record_width(nbx, oracle, torch_gpu, batch_mode, launch_config):
    """Records of 19 words: eight sources, destination counts alternating 1
    and 8, f16 -> fp32; the one-destination buckets' windows in rows 1..7 stay
    untouched."""
    batch_mode(bc.MODE_DEFAULT)
    launch_config(1, 0)
    assert 3 + 8 + max(len(b.rows) for b in bc.record_width(2)) == 19 <= bc.LIST_REC_WORDS_MAX
    case = mi.wide_cases(oracle, F16, 8)[1]
    run_shape(nbx, oracle, torch_gpu, F16, True, (case[0], case[1], 3), bc.record_width, 8, [20], rows=8)


# ---------------------------------------------------------------------------
# 4. in place

@pytest.mark.parametrize("st", mi.WIDE_TYPES)
def test_wide_batch_in_place(nbx, oracle, torch_gpu, batch_mode, launch_config, st):
    """Source-type output, every bucket's destination its own source 0 or its
    last source: the table at 3 and 8 sources on private copies of the
    sources. Every other source, and the written one outside the windows,
    stays what it was."""
    torch = torch_gpu
    ts = state_for(torch, oracle, st)
    batch_mode(bc.MODE_DEFAULT)
    launch_config(0, 0)
    n = 1216 * ts.epp
    for nsrc in (3, 8):
        arena = table_arena(ts, False, rows=nsrc)
        host = np.full(tuple(arena.shape), 0xA5, dtype=np.uint8)
        for k in range(nsrc):
            host[k, FRONT:FRONT + n * ts.eb] = ts.srcs[k][:n].view(np.uint8)
        background = (host, torch.from_numpy(host).cuda())
        sp = [row_ptr(arena, k, 0) for k in range(nsrc)]
        for which, case in zip((0, nsrc - 1), mi.wide_cases(oracle, st, nsrc)):
            exp = ts.expect_wide(nsrc, False, *case)
            buckets = [b._replace(rows=(which,)) for b in bc.table_buckets(ts.eb, [1] * 7)]
            tasks, checks = from_buckets(ts, arena, sp, buckets, nsrc, exp, False)
            assert all(t[0][0] == t[1][which] for t in tasks)
            run_call(nbx, ts, arena, tasks, checks, False, case, which == 0, wb.records(nsrc, [7], False),
                     what_of(ts, False, case, nsrc) + f" in place on source {which}", background=background)


# ---------------------------------------------------------------------------
# 5. policy and record order

def fold_of(oracle, ts, windows, out32, case=SUM_CASE):
    """The oracle route for sources given as arrays of raw codes."""
    fold = oracle.reduce_multi([mi.widen(oracle, w, ts.dtype) for w in windows], F32, case[0], case[1], case[2],
                               threads=8)[0]
    return fold if out32 else mi.narrow(oracle, fold, ts.dtype)


def mixed_call(ts, oracle, arena_of, out32):
    """One call, interleaved: small eligible buckets of 2, 5 and 8 sources, an
    11-source bucket, a bucket whose sources lie on two misalignments, one
    whose destination is 4 bytes off its eligible offset, and an empty one.
    Returns (arena, [(task, check, nsrc, kind)]) in call order; kind: 'list',
    'eleven', 'elements' or 'empty'."""
    eb, epp = ts.eb, ts.epp
    deb = 4 if out32 else eb
    specs = bc.small_set(eb, 8) + [("11 sources", 24 * epp, 300 * epp + 5), ("mixed sources", 40 * epp, 200 * epp + 3),
                                   ("destination off", 48 * epp, 100 * epp + 1), ("empty", 64 * epp, 0)]
    buckets = bc.place(specs, eb)
    arena = arena_of(bc.arena_elts(buckets, eb) * deb + 16)
    sp = ts.src_ptrs([0] * mi.MAX_WIDE_SRCS)
    nsrcs = [2, 5, 8, 2, 5, 8, 2, 5]
    out = []
    for b, ns in zip(buckets[:8], nsrcs):
        exp = ts.expect_wide(ns, out32, *SUM_CASE)
        t, c = from_buckets(ts, arena, sp, [b], ns, exp, out32)
        out.append((t[0], c[0], ns, "list"))
    eleven, mixed, off, empty = buckets[8:]
    t, c = from_buckets(ts, arena, sp, [eleven], 11, ts.expect_wide(11, out32, *SUM_CASE), out32)
    out.insert(2, (t[0], c[0], 11, "eleven"))
    # source 1 one element further on: two misalignments, the fold of shifted windows
    win = [ts.srcs[k][mixed.start + (k == 1):mixed.start + (k == 1) + mixed.count] for k in range(3)]
    task = ([row_ptr(arena, 0, mixed.dstart * deb)], [sp[k] + (mixed.start + (k == 1)) * eb for k in range(3)],
            mixed.count)
    out.insert(5, (task, (mixed.name, (0,), mixed.dstart * deb, fold_of(oracle, ts, win, out32)), 3, "elements"))
    # 4 bytes (fp32) or one element (source type) past the offset the pack kernel needs
    shift = 4 if out32 else eb
    t, c = from_buckets(ts, arena, sp, [off], 2, ts.expect_wide(2, out32, *SUM_CASE), out32)
    task = ([t[0][0][0] + shift], t[0][1], t[0][2])
    out.insert(7, (task, (off.name, (0,), off.dstart * deb + shift, c[0][3]), 2, "elements"))
    t, c = from_buckets(ts, arena, sp, [empty], 2, ts.expect_wide(2, out32, *SUM_CASE), out32)
    out.insert(9, (t[0], c[0], 2, "empty"))
    for task, _, ns, kind in out:
        if kind != "empty":
            assert wb.eligible(task[1], task[0], eb, out32) == (kind in ("list", "eleven"))
    return arena, out


def single_records(items, out32):
    o32 = wb.OUT32 if out32 else 0
    recs = []
    for _, _, ns, kind in items:
        if kind == "eleven":   # a first pass of 8 into the fp32 partial, then the partial and three sources
            recs += [(wb.FAM_WIDE_PACKS, 8, 4, wb.OUT32), (wb.FAM_WIDE_PACKS, 4, 4, o32 | wb.PART_FIRST)]
        elif kind == "elements":
            recs.append((wb.FAM_WIDE_ELTS, ns, 1, o32))
        elif kind == "list":
            recs.append(wb.single_pack_record(ns, out32))
    return recs


@pytest.mark.parametrize("out32", [True, False], ids=["fp32", "same"])
def test_wide_batch_policy_record(nbx, oracle, torch_gpu, batch_mode, launch_config, out32):
    """The documented order (include/nbx_debug.h): the buckets that run alone
    first, in bucket order; then one work-list launch per source count,
    ascending. Launch variant 2 batches nothing; batch mode 0 runs every
    eligible bucket as its own launch behind the single ones, per source
    count. The results are the same every time."""
    ts = state_for(torch_gpu, oracle, BF16)
    arena, items = mixed_call(ts, oracle, lambda nbytes: new_arena(torch_gpu, 1, nbytes), out32)
    tasks = [it[0] for it in items]
    checks = [it[1] for it in items]
    alone = [it for it in items if it[3] in ("eleven", "elements")]
    listed = [it for it in items if it[3] == "list"]
    per_count = {ns: [it for it in listed if it[2] == ns] for ns in (2, 5, 8)}
    assert [len(v) for v in per_count.values()] == [3, 3, 2]
    batched = single_records(alone, out32) + [r for ns, v in per_count.items() for r in wb.records(ns, [len(v)], out32)]
    unbatched = single_records(alone, out32) + [r for v in per_count.values() for r in single_records(v, out32)]
    in_order = single_records(items, out32)
    for mode, variant, want, label in ((bc.MODE_DEFAULT, 0, batched, "default"), (bc.MODE_LIST, 1, batched, "mode 2"),
                                       (bc.MODE_DEFAULT, 2, in_order, "variant 2"),
                                       (bc.MODE_KERNARG, 0, unbatched, "mode 0")):
        batch_mode(mode)
        launch_config(0, variant)
        run_call(nbx, ts, arena, tasks, checks, out32, SUM_CASE, False, want, f"policy, {label}, fp32={out32}")


def test_wide_batch_policy_big_bucket_threshold(nbx, oracle, torch_gpu, batch_mode, launch_config):
    """At four sources a bucket of wideUnroll(4) x 256 x CUs packs (one unrolled
    tile per CU) runs alone; one 256-pack tile fewer it is batched. Variant 1
    batches both."""
    torch = torch_gpu
    ts = state_for(torch, oracle, BF16)
    eb, epp = ts.eb, ts.epp
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nsrc, out32 = 4, True
    packs = wb.wide_unroll(nsrc) * 256 * cus
    batch_mode(bc.MODE_DEFAULT)
    srcs = mi.edge_inputs(oracle, BF16, nsrc, packs * epp, seed=mi.seed_for(BF16) + 1)
    exp = fold_of(oracle, ts, srcs, out32)
    up = [torch.from_numpy(s).cuda() for s in srcs]
    sp = [t.data_ptr() for t in up]
    assert all(p % 16 == 0 for p in sp)
    buckets = bc.place([("one unrolled tile per CU", 0, packs * epp), ("one tile fewer", 0, (packs - 256) * epp)], eb)
    arena = new_arena(torch, 1, bc.arena_elts(buckets, eb) * 4)
    tasks, checks = from_buckets(ts, arena, sp, buckets, nsrc, exp, out32)
    for variant, want in ((0, [wb.single_pack_record(nsrc, out32)] + wb.records(nsrc, [1], out32)),
                          (1, wb.records(nsrc, [2], out32))):
        launch_config(0, variant)
        run_call(nbx, ts, arena, tasks, checks, out32, SUM_CASE, False, want,
                 f"variant {variant}, buckets of {packs} and {packs - 256} packs")


# ---------------------------------------------------------------------------
# 6. slot exhaustion and capture

def test_wide_batch_slots_and_graph_ownership(nbx, oracle, torch_gpu):
    """More calls in flight than the arena has slots: the rest run one
    nbxReduceMultiWide launch per bucket, never wait, and come out right. A
    call captured into a graph keeps its slot while eager calls recycle the
    others, and every replay reads it in place."""
    torch = torch_gpu
    lib = nbx.load_library()
    dev_id = torch.cuda.current_device()
    prev = lib.nbxDebugSetBatchMode(1)
    saved = nbx.get_launch_config()
    nbx.set_launch_config(0, 0)
    try:
        nsrc = 3
        counts = [3000, 20000, 5, 4001] * 5   # 20 buckets, one work-list launch per call
        srcs = [[torch.empty(c, dtype=torch.int16, device="cuda") for _ in range(nsrc)] for c in counts]
        outs = [torch.empty(c, dtype=torch.float32, device="cuda") for c in counts]
        buckets = [([o.data_ptr()], [t.data_ptr() for t in ss], c) for ss, o, c in zip(srcs, outs, counts)]
        other_in = [torch.zeros(1000, dtype=torch.int16, device="cuda") for _ in range(2)]
        other_out = [torch.empty(1000, dtype=torch.float32, device="cuda") for _ in range(20)]
        other = [([o.data_ptr()], [t.data_ptr() for t in other_in], 1000) for o in other_out]
        op = nbx.DevRedOpFull()
        s = torch.cuda.Stream()

        def fill(it):
            host = []
            for k, (ss, c) in enumerate(zip(srcs, counts)):
                xs = oracle.random_inputs(BF16, nsrc, c, seed=500 * it + k)
                for t, x in zip(ss, xs):
                    t.copy_(torch.from_numpy(x.view(np.int16)))
                host.append(xs)
            return host

        def check(host):
            for xs, o in zip(host, outs):
                exp = oracle.reduce_multi([mi.widen(oracle, x, BF16) for x in xs], F32, SUM)[0]
                mi.assert_same(o.cpu().numpy(), exp, F32)

        def call():
            nbx.reduce_multi_wide_batch(buckets, BF16, F32, op, 0, s.cuda_stream)

        host = fill(0)
        torch.cuda.synchronize()
        fb0 = lib.nbxDebugBatchListSlots(dev_id, 3)
        hold = lib.nbxDebugHoldStream(ctypes.c_void_p(s.cuda_stream), 60_000)
        assert hold >= 0
        nbx.launch_log_reset()
        try:
            with torch.cuda.stream(s):
                for _ in range(140):   # > 128 slots in flight
                    call()
        finally:
            assert lib.nbxDebugReleaseStream(hold) == 0
        total, recs = nbx.launch_log()
        s.synchronize()
        check(host)
        assert lib.nbxDebugBatchListSlots(dev_id, 3) > fb0
        listed, single = wb.records(nsrc, [20], True)[0], wb.single_pack_record(nsrc, True)
        assert set(recs) <= {listed, single} and recs[-1] == single
        assert total > 140   # some calls found no slot and took 20 launches each
        with torch.cuda.stream(s):
            for _ in range(20):   # each eager call returns a few completed slots to the free pool
                call()
                s.synchronize()
        assert lib.nbxDebugBatchListSlots(dev_id, 0) > 0
        owned0 = lib.nbxDebugBatchListSlots(dev_id, 2)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        assert lib.nbxDebugBatchListSlots(dev_id, 2) == owned0 + 1
        for it in (1, 2):
            host = fill(it)
            with torch.cuda.stream(s):
                for _ in range(100):   # recycles every other slot, never the graph's
                    nbx.reduce_multi_wide_batch(other, BF16, F32, op, 0, s.cuda_stream)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            check(host)
        del g
        torch.cuda.synchronize()
        assert lib.nbxDebugBatchListSlots(dev_id, 2) in (owned0, owned0 + 1)
    finally:
        lib.nbxDebugSetBatchMode(prev)
        nbx.set_launch_config(*saved)


# ---------------------------------------------------------------------------
# 7. equal to the per-bucket call

@pytest.mark.parametrize("out32", [True, False], ids=["fp32", "same"])
def test_wide_batch_equals_per_bucket_calls(nbx, oracle, torch_gpu, batch_mode, launch_config, out32):
    """The mixed call of the policy test, and the same buckets as one
    nbxReduceMultiWide call each into a second arena on the same offsets: the
    two arenas are byte-identical."""
    torch = torch_gpu
    batch_mode(bc.MODE_DEFAULT)
    launch_config(0, 0)
    for st, case in ((BF16, SUM_CASE), (E5M2, mi.wide_cases(oracle, E5M2, 2)[1][:2] + (1,))):
        ts = state_for(torch, oracle, st)
        arenas = []
        arena, items = mixed_call(ts, oracle, lambda nbytes: arenas.append(new_arena(torch, 2, nbytes)) or arenas[-1],
                                  out32)
        stream = torch.cuda.current_stream().cuda_stream
        dt = F32 if out32 else st
        op = make_op(nbx, ts, case, True)
        arena.fill_(0xA5)
        nbx.reduce_multi_wide_batch([it[0] for it in items], st, dt, op, case[2], stream)
        row = arena.shape[1]
        for task, _, _, _ in items:
            nbx.reduce_multi_wide([p + row for p in task[0]], task[1], task[2], st, dt, op, case[2], stream)
        rows = arena.cpu().numpy()
        assert (rows[0] != 0xA5).any()
        assert np.array_equal(rows[0], rows[1]), f"{oracle.TYPE_NAMES[st]} fp32={out32}: the batched call and the " \
                                                 f"per-bucket calls differ at bytes {np.flatnonzero(rows[0] != rows[1])[:8]}"
