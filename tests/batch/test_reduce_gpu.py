"""Every batched-reduce kernel instantiation — kReduceBatch<Fn, NSRC> and
kReduceBatchList<Fn, NSRC>, type x op x source count x launch form — against
the CPU oracle, bit for bit (NaN compared as NaN), on tests/batch/cases.py's
bucket table: buckets below one pack, head-only and clipped-head buckets, an
exact tile, a head with a one-pack last tile and a tail, a ragged three-tile
bucket and an empty one, all in one nbxReduceMultiBatch call per (type, op,
source count, form). Inputs are tests/matrix/inputs.py's edge-rich values, so
NaN, inf, +-0 and denormals go through batchElt's scalar pre / red / post as
well as through the pack path.

After every call the library's launch record (nbxDebugLaunchLog, families 13
kernel-argument batch and 14 work-list batch) has to name the form, the source
count and the number of buckets that ran: nbxReduceMultiBatch can fall back to
kernel-argument tables, keep a small set in kernel arguments, send a big
bucket to the big-tile kernel or run a bucket alone, and every one of those
still gives the right answer.

The scheduler shapes pin the kernels' record walks to sizes that must take
them (cases.py), with every threshold derived from the device's CU count; the
policy test pins nbxReduceMultiBatch's choice of form and its fallbacks.

The file carries the parity core's name on purpose, as tests/matrix/ does: the
GPU suite orders files by name (tests/conftest.py GPU_FILE_ORDER)."""
import os

import numpy as np
import pytest

from tests.batch import cases as bc
from tests.matrix import inputs as mi
from tests.matrix.test_reduce_gpu import FRONT, DstCycle, TypeState, big_unroll

pytestmark = pytest.mark.gpu

ALL_TYPES = list(range(12))
F32, BF16 = mi.F32, mi.BF16
SUM, PREMULSUM = mi.SUM, mi.PREMULSUM
SMALL, BIG, LDS = 1, 2, 4                # nbxDebugLaunchLog families of the single-bucket paths
DYNAMIC = 1                              # flag bit 0 of the per-step families
FORMS = {bc.MODE_KERNARG: ("kernel arguments", bc.FAM_KERNARG), bc.MODE_LIST: ("work list", bc.FAM_LIST)}
SUM_CASE = ("sum", SUM, 0, 0, False, False)

_STATE = {}


def state_for(torch, oracle, dtype):
    if dtype not in _STATE:
        _STATE[dtype] = TypeState(torch, oracle, dtype)
    return _STATE[dtype]


@pytest.fixture(scope="module", autouse=True)
def _release_state():
    yield
    _STATE.clear()


@pytest.fixture
def batch_mode(nbx):
    lib = nbx.load_library()
    saved = lib.nbxDebugSetBatchMode(-1)

    def force(mode):
        lib.nbxDebugSetBatchMode(mode)
    yield force
    lib.nbxDebugSetBatchMode(saved)


@pytest.fixture
def launch_config(nbx):
    saved = nbx.get_launch_config()
    yield nbx.set_launch_config
    nbx.set_launch_config(*saved)


def premulsum_case(oracle, dtype, nsrc):
    """PreMulSum with the 3-rank Avg scalar in device memory and the pre-op on
    an interior number of sources (0 < npre < nsrc)."""
    devop, scalar = oracle.host_to_dev_redop(mi.NCCL_AVG, dtype, 3)
    assert devop == PREMULSUM
    npre = (nsrc + 1) // 2
    assert 0 < npre < nsrc
    return (f"premulsum npre={npre}", PREMULSUM, scalar, npre, False, True)


def sched_cases(oracle, nsrc):
    return [(F32, SUM_CASE), (BF16, premulsum_case(oracle, BF16, nsrc))]


# ---------------------------------------------------------------------------
# one call, checked

def new_arena(torch, rows, payload_bytes):
    """`rows` destination rows: FRONT guard bytes, the payload, a guard behind it."""
    row = (FRONT + payload_bytes + 256 + 255) // 256 * 256
    t = torch.empty((rows, row), dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    return t


def dst_ptr(arena, eb, row, dstart):
    return arena.data_ptr() + row * arena.shape[1] + FRONT + dstart * eb


def from_buckets(ts, arena, sp, buckets, nsrc, exp):
    """(tasks, checks) of buckets that read windows of the sources at `sp` and
    write `arena`; `exp` is the expected fold of the whole sources."""
    tasks, checks = [], []
    for b in buckets:
        tasks.append(([dst_ptr(arena, ts.eb, r, b.dstart) for r in b.rows],
                      [p + b.start * ts.eb for p in sp[:nsrc]], b.count))
        checks.append((b.name, b.rows, b.dstart, exp[b.start:b.start + b.count]))
    return tasks, checks


def make_op(nbx, ts, case):
    _, devop, arg, _, _, on_device = case
    op = nbx.DevRedOpFull()
    op.op = devop
    if on_device:
        op.scalarArgIsPtr = 1
        op.scalarArg = ts.set_scalar(arg, ts.eb)
    else:
        op.scalarArg = arg
    return op


def run_call(nbx, ts, arena, tasks, checks, case, want, what, background=None, ignore_dynamic=False):
    """Refills `arena` (0xA5, or `background`: a host image and its device
    copy), makes one nbxReduceMultiBatch call of `tasks`, then checks the launch
    record against `want`, every (name, rows, dstart, expected) of `checks` bit
    for bit, and that every other byte of the arena is what it was."""
    if background is None:
        arena.fill_(0xA5)
    else:
        arena.copy_(background[1])
    op = make_op(nbx, ts, case)
    stream = ts.torch.cuda.current_stream().cuda_stream
    nbx.launch_log_reset()
    nbx.reduce_multi_batch(tasks, ts.dtype, op, case[3], case[4], stream)
    total, recs = nbx.launch_log()
    rows = arena.cpu().numpy()   # synchronizes with the stream
    if ignore_dynamic:
        recs = [(f, n, u, fl & ~DYNAMIC if f <= 7 else fl) for f, n, u, fl in recs]
    assert (total, recs) == (len(want), want), f"{what}: launch record {recs} (of {total}), wanted {want}"
    untouched = np.ones(rows.shape, dtype=bool)
    for name, drows, dstart, exp in checks:
        lo = FRONT + dstart * ts.eb
        hi = lo + exp.size * ts.eb
        for d, r in enumerate(drows):
            try:
                mi.assert_same(rows[r, lo:hi].view(ts.st), exp, ts.dtype)
            except AssertionError as e:
                raise AssertionError(f"{what}, bucket '{name}', destination {d}: {e}") from None
            untouched[r, lo:hi] = False
    was = 0xA5 if background is None else background[0][untouched]
    bad = np.flatnonzero(rows[untouched] != was)
    if bad.size:
        r, c = (a[bad[0]] for a in np.nonzero(untouched))
        raise AssertionError(f"{what}: {bad.size} bytes outside every bucket's destinations were written, the first "
                             f"in row {r} at byte {c - FRONT} of the payload")


def what_of(ts, form, case, nsrc):
    return f"{FORMS[form][0] if form in FORMS else 'mode %d' % form} {ts.oracle.TYPE_NAMES[ts.dtype]} {case[0]} nsrc={nsrc}"


def table_arena(ts, rows=bc.MAX_DSTS):
    return new_arena(ts.torch, rows, 1216 * 16)   # the table ends below 1,200 packs


# ---------------------------------------------------------------------------
# the instantiation matrix

@pytest.mark.parametrize("dtype", ALL_TYPES)
@pytest.mark.parametrize("form", list(FORMS), ids=["kernarg", "list"])
def test_batch_kernels(nbx, oracle, torch_gpu, batch_mode, launch_config, form, dtype):
    """One call of cases.py's table per (op, source count): all seven non-empty
    buckets in one launch of the form's kernel for that source count."""
    ts = state_for(torch_gpu, oracle, dtype)
    batch_mode(form)
    launch_config(0, 0)
    arena = table_arena(ts)
    sp = ts.src_ptrs([0] * mi.MAX_SRCS)
    dsts = DstCycle()
    for nsrc in range(1, mi.MAX_SRCS + 1):
        for case in mi.op_cases(oracle, dtype, nsrc):
            ndsts = [dsts.next() for _ in range(7)]
            if nsrc == 8 and case[1] == SUM:
                ndsts[bc.NAMES.index("tile + pack")] = 8
            exp = ts.expect(nsrc, *case[1:5])
            share = bc.nan_share_of_call(exp, ts.eb, dtype)
            what = what_of(ts, form, case, nsrc)
            assert share <= mi.NAN_CAP, f"{what}: {share:.1%} of the oracle's results is NaN"
            tasks, checks = from_buckets(ts, arena, sp, bc.table_buckets(ts.eb, ndsts), nsrc, exp)
            run_call(nbx, ts, arena, tasks, checks, case, bc.records(FORMS[form][1], nsrc, [7]), what)


# ---------------------------------------------------------------------------
# scheduler shapes: one workgroup per CU (set_launch_config(1, 0))

def device_shape(torch):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    chunk = max(1, int(os.environ.get("NBX_BATCH_CHUNK", "4") or 4))
    return cus, chunk


def run_shape(nbx, oracle, torch, form, buckets_of, nsrc, launches, rows=1):
    for dtype, case in sched_cases(oracle, nsrc):
        ts = state_for(torch, oracle, dtype)
        buckets = buckets_of(ts.eb)
        arena = new_arena(torch, rows, bc.arena_elts(buckets, ts.eb) * ts.eb)
        exp = ts.expect(nsrc, *case[1:5])
        tasks, checks = from_buckets(ts, arena, ts.src_ptrs([0] * mi.MAX_SRCS), buckets, nsrc, exp)
        run_call(nbx, ts, arena, tasks, checks, case, bc.records(FORMS[form][1], nsrc, launches),
                 what_of(ts, form, case, nsrc))


def test_batch_kernarg_cursor_walk(nbx, oracle, torch_gpu, batch_mode, launch_config):
    """kReduceBatch's `do ... while (tile >= tEnd)`: 120 two-source buckets in
    tables of 101 and 19, the first holding more than 1.5 tiles per workgroup,
    so workgroups come back for a second tile whose record lies dozens of
    records past the cursor."""
    cus, _ = device_shape(torch_gpu)
    batch_mode(bc.MODE_KERNARG)
    launch_config(1, 0)
    for eb in (4, 2):
        buckets = bc.kernarg_walk(eb)
        assert bc.kernarg_launches(buckets, 2) == [101, 19]
        first = sum(bc.tiles_of(buckets[:101], eb))
        assert first > 1.5 * cus, f"{first} tiles in the first launch do not give {cus} workgroups a second tile"
        assert cus // 4 >= 24   # records between a workgroup's first and second tile (16 tiles per 4 records)
    run_shape(nbx, oracle, torch_gpu, bc.MODE_KERNARG, bc.kernarg_walk, 2, [101, 19])


def test_batch_list_record_search(nbx, oracle, torch_gpu, batch_mode, launch_config):
    """kReduceBatchList's `for (base = k + 1;; base += 64)`: 400 two-source
    buckets in launches of 384 and 16. The first launch holds more tiles than
    one turn of every workgroup takes, so workgroups take a second turn with
    the cursor already advanced; the last workgroup's first chunk lies past the
    tiles of the first 64 records, so its first search finds no match in the
    first 64 running totals; chunks cross bucket boundaries."""
    cus, chunk = device_shape(torch_gpu)
    batch_mode(bc.MODE_LIST)
    launch_config(1, 0)
    for eb in (4, 2):
        buckets = bc.list_walk(eb)
        assert bc.list_launches(len(buckets)) == [384, 16]
        tiles = bc.tiles_of(buckets[:384], eb)
        first = sum(tiles)
        assert first > chunk * cus, f"{first} tiles in the first launch: no workgroup takes a second turn"
        grid = min(-(-first // chunk), cus)
        assert chunk * (grid - 1) >= sum(tiles[:64]), "every workgroup's first tile lies in the first 64 records"
        assert chunk > 1 and tiles[0] < chunk   # the first chunk already crosses a bucket boundary
    run_shape(nbx, oracle, torch_gpu, bc.MODE_LIST, bc.list_walk, 2, [384, 16])


def test_batch_list_record_width(nbx, oracle, torch_gpu, batch_mode, launch_config):
    """Work-list records of 19 words: eight sources, destination counts
    alternating 1 and 8, so every other record's last seven destination slots
    are padding; the one-destination buckets' windows in rows 1..7 stay
    untouched."""
    batch_mode(bc.MODE_LIST)
    launch_config(1, 0)
    for eb in (4, 2):
        assert 3 + 8 + max(len(b.rows) for b in bc.record_width(eb)) == 19 <= bc.LIST_REC_WORDS_MAX
    run_shape(nbx, oracle, torch_gpu, bc.MODE_LIST, bc.record_width, 8, [20], rows=8)


@pytest.mark.parametrize("form", list(FORMS), ids=["kernarg", "list"])
def test_batch_in_place(nbx, oracle, torch_gpu, batch_mode, launch_config, form):
    """Every bucket's dsts[0] is its srcs[0]: the table's buckets at three
    sources, on private copies of the sources. Source 0 outside the windows and
    sources 1 and 2 everywhere stay what they were."""
    torch = torch_gpu
    batch_mode(form)
    launch_config(1, 0)
    nsrc = 3
    for dtype, case in sched_cases(oracle, nsrc):
        ts = state_for(torch, oracle, dtype)
        arena = table_arena(ts, rows=nsrc)
        host = np.full(tuple(arena.shape), 0xA5, dtype=np.uint8)
        n = 1216 * ts.epp
        for k in range(nsrc):
            host[k, FRONT:FRONT + n * ts.eb] = ts.srcs[k][:n].view(np.uint8)
        background = (host, torch.from_numpy(host).cuda())
        sp = [dst_ptr(arena, ts.eb, k, 0) for k in range(nsrc)]
        exp = ts.expect(nsrc, *case[1:5])
        tasks, checks = from_buckets(ts, arena, sp, bc.table_buckets(ts.eb, [1] * 7), nsrc, exp)
        assert all(t[0][0] == t[1][0] for t in tasks)
        run_call(nbx, ts, arena, tasks, checks, case, bc.records(FORMS[form][1], nsrc, [7]),
                 what_of(ts, form, case, nsrc) + " in place", background=background)


# ---------------------------------------------------------------------------
# launch policy

def test_batch_policy_record(nbx, oracle, torch_gpu, batch_mode, launch_config):
    """nbxReduceMultiBatch's choice of form and its fallbacks, in the default
    mode: up to 16 buckets of a source count stay in kernel arguments, 17 take
    the work list; a bucket of mixed alignment and one of 12 sources run alone,
    ahead of the batch, which does not count them; a bucket of 4+ sources that
    gives every CU a big tile leaves the batch unless the launch variant says
    otherwise."""
    torch = torch_gpu
    ts = state_for(torch, oracle, F32)
    eb, epp = ts.eb, ts.epp
    cus, _ = device_shape(torch)
    batch_mode(bc.MODE_DEFAULT)
    launch_config(0, 0)
    sp = ts.src_ptrs([0] * mi.MAX_SRCS)
    exp3 = ts.expect(3, *SUM_CASE[1:5])
    for n, want in ((16, bc.records(bc.FAM_KERNARG, 3, [16])), (17, bc.records(bc.FAM_LIST, 3, [17]))):
        buckets = bc.place(bc.small_set(eb, n), eb)
        arena = new_arena(torch, 1, bc.arena_elts(buckets, eb) * eb)
        tasks, checks = from_buckets(ts, arena, sp, buckets, 3, exp3)
        run_call(nbx, ts, arena, tasks, checks, SUM_CASE, want, f"default mode, {n} three-source buckets")

    # the 17 again, with a bucket whose destination is one element off its
    # sources in front and a 12-source bucket in the middle
    buckets = bc.place(bc.small_set(eb, 17) + [("mixed alignment", 40 * epp, 300 * epp + 1),
                                               ("12 sources", 48 * epp, 200 * epp + 3)], eb)
    arena = new_arena(torch, 1, (bc.arena_elts(buckets, eb) + 1) * eb)
    tasks, checks = from_buckets(ts, arena, sp, buckets[:17], 3, exp3)
    mixed, twelve = buckets[17], buckets[18]
    order = list(range(8)) + list(range(4))   # the 12 sources: uploads 0..7, then 0..3 again
    exp12 = oracle.reduce_multi([ts.srcs[k][twelve.start:twelve.start + twelve.count] for k in order], F32, SUM,
                                threads=8)[0]
    t_mixed = ([dst_ptr(arena, eb, 0, mixed.dstart + 1)], [p + mixed.start * eb for p in sp[:3]], mixed.count)
    t_twelve = ([dst_ptr(arena, eb, 0, twelve.dstart)], [sp[k] + twelve.start * eb for k in order], twelve.count)
    assert (t_mixed[0][0] - t_mixed[1][0]) % 16 == eb
    tasks = [t_mixed] + tasks[:8] + [t_twelve] + tasks[8:]
    checks = checks + [(mixed.name, (0,), mixed.dstart + 1, exp3[mixed.start:mixed.start + mixed.count]),
                       (twelve.name, (0,), twelve.dstart, exp12)]
    want = [(LDS, 3, 2, 0), (SMALL, 8, 1, 0), (SMALL, 5, 1, 0)] + bc.records(bc.FAM_LIST, 3, [17])
    run_call(nbx, ts, arena, tasks, checks, SUM_CASE, want, "default mode, 17 buckets and two fallbacks")


def test_batch_policy_big_bucket_threshold(nbx, oracle, torch_gpu, batch_mode, launch_config):
    """At five sources a bucket of unroll x 256 x CUs packs (one big tile per
    CU) leaves the batch for the big-tile kernel; one pack shorter it stays.
    Launch variant 1 keeps both in the batch, variant 2 batches nothing."""
    torch = torch_gpu
    ts = state_for(torch, oracle, F32)
    eb, epp = ts.eb, ts.epp
    cus, _ = device_shape(torch)
    nsrc = 5
    unroll = big_unroll(nsrc, F32, SUM)
    packs = unroll * 256 * cus
    batch_mode(bc.MODE_DEFAULT)
    srcs = mi.edge_inputs(oracle, F32, nsrc, packs * epp, seed=mi.seed_for(F32) + 1)
    exp = oracle.reduce_multi(srcs, F32, SUM, threads=8)[0]
    up = [torch.from_numpy(s).cuda() for s in srcs]
    sp = [t.data_ptr() for t in up]
    assert all(p % 16 == 0 for p in sp)
    buckets = bc.place([("one big tile per CU", 0, packs * epp), ("one pack shorter", 0, (packs - 1) * epp),
                        ("small", 16 * epp, 300 * epp + 3)], eb)
    arena = new_arena(torch, 1, bc.arena_elts(buckets, eb) * eb)
    tasks, checks = from_buckets(ts, arena, sp, buckets, nsrc, exp)
    big = (BIG, nsrc, unroll, 0)
    for variant, want in ((0, [big] + bc.records(bc.FAM_KERNARG, nsrc, [2])),
                          (1, bc.records(bc.FAM_KERNARG, nsrc, [3])),
                          (2, [big, big, big])):
        launch_config(0, variant)
        run_call(nbx, ts, arena, tasks, checks, SUM_CASE, want,
                 f"default mode, variant {variant}, buckets of {packs}, {packs - 1} and 300 packs", ignore_dynamic=True)
