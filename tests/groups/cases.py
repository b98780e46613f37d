"""Case tables of the grouped-launch tests, shared by the GPU tests
(tests/groups/test_multiprocess_gpu.py) and their CPU companion
(tests/test_group_segments_cpu.py).

ncclGroupStart ... ncclGroupEnd on a multi-process communicator is cut into
runs (comm_mp_launch.cc runMpGroup) and every run is ONE kernel that carries a
segment table: LLSeg (packOff, in 8-byte packs for kLLColl and 48-byte lines
for kLL128Coll) or SimpleSeg (sliceOff, in virtual slices of a block, for
kSimpleColl and kSimpleRing; slice, grid and rounds come from the sum of the
segments' block bytes). Every thread first looks up which message its unit
belongs to (llMsg, simpleSlice). None of that runs for a single call.

Section 1 of this file is the segment table of test_group_segments: four
communicators (ll, ll128, simple, ring), AllReduce and ReduceScatter, eight
(type, op) pairs x eight segments in one group of 64 calls, which the library
has to cut into exactly eight launches of eight segments at the type / op
changes. Sizes are bytes per message for LL / LL128 and bytes per block for
Simple; counts are max(1, B // eb) elements; a Simple AllReduce counts n blocks
minus s % 4 elements, so its last block is ragged. Segment s puts its send
(s eb) % 16 and its recv ((s + 3) eb) % 16 bytes past a 16-byte boundary; the
last segment is in place. tests/test_group_segments_cpu.py asserts what these
shapes reach (a segment boundary inside a round and on one, slot reuse by
another segment, partial units, a pass spanning two segments, ...) at every
element width and n, from mp_diag's mirror of the host arithmetic.

Section 2 is the table of test_group_cut_rules: one group per cut rule of
runMpGroup on a default communicator, int32 / f32 Sum with exact arithmetic,
whose launch record must equal mp_diag.group_runs' answer."""
import functools
from collections import namedtuple

import numpy as np

from tests import mp_diag
from tests.matrix import inputs as mi
from tests.test_multiprocess_gpu import _blocks, ring_chain

NS = (2, 3, 5)
SUM, PROD, MAX, MIN, AVG = range(5)                              # ncclRedOp_t
INT8, INT32, INT64, F16, F32, F64, BF16, E4M3 = 0, 2, 4, 6, 7, 8, 9, 10   # ncclDataType_t
FAM_LL, FAM_LL128, FAM_LL128X2, FAM_SIMPLE, FAM_RING = 8, 9, 10, 11, 12   # include/nbx_debug.h
GUARD = 16          # bytes of 0xA5 either side of every buffer

# one pair per element width and functor kind (the folds themselves are tests/edges' subject)
TYPE_OPS = ((E4M3, SUM), (INT8, MAX), (F16, AVG), (BF16, SUM), (F32, SUM), (INT32, AVG), (F64, PROD), (INT64, MIN))
KINDS = ("ar", "rs")
N_SEGS, IN_PLACE = 8, 7
ONE = None          # "one element"
SEG_BYTES = {
    "ll": (ONE, 5, 8, 13, 2048, 2051, 4099, 1000),         # 2,048 B: 256 packs, exactly one workgroup pass
    "ll128": (ONE, 47, 48, 49, 96, 3072, 5003, 1000),      # 3,072 B: 64 lines, one workgroup pass
    "simple": (ONE, 8, 3000, 4096, 4104, 12288, 20000, 6000),   # 12,288 B: one full round of 3 x 4,096
    "ring": (ONE, 8, 3000, 4096, 4104, 12288, 20000, 6000),
}
PATHS = tuple(SEG_BYTES)          # a path is a communicator here
UNIT = {"ll": 8, "ll128": 48}     # bytes per LLSeg unit
PASS_UNITS = {"ll": 256, "ll128": 64}   # units one workgroup moves per pass
FAMILY = {"ll": FAM_LL, "ll128": FAM_LL128, "simple": FAM_SIMPLE, "ring": FAM_RING}
LL128_ONESHOT_MAX, LL128_MAX_GRID, SIMPLE_GRID, SIMPLE_SLICE, SIMPLE_SLOTS = 16384, 16, 3, 4096, 2

# the environment a communicator is created under; every key of ENV_KEYS that a
# communicator does not name is unset while it is created. NBX_LL128_MAX_GRID is
# read once per process (tests/edges/cases.py), so it is set for the process too.
ENV_KEYS = ("NCCL_PROTO", "NCCL_ALGO", "NBX_LL128_ONESHOT_MAX", "NBX_SIMPLE_MAX_GRID", "NBX_SIMPLE_SLICE_BYTES")
PROCESS_ENV = {"NBX_LL128_MAX_GRID": str(LL128_MAX_GRID)}
COMM_ENV = {
    "ll": {"NCCL_PROTO": "LL"},
    "ll128": {"NCCL_PROTO": "LL128", "NBX_LL128_ONESHOT_MAX": str(LL128_ONESHOT_MAX),
              "NBX_LL128_MAX_GRID": str(LL128_MAX_GRID)},
    "simple": {"NCCL_PROTO": "Simple", "NBX_SIMPLE_MAX_GRID": str(SIMPLE_GRID),
               "NBX_SIMPLE_SLICE_BYTES": str(SIMPLE_SLICE)},
    "ring": {"NCCL_PROTO": "Simple", "NCCL_ALGO": "Ring", "NBX_SIMPLE_MAX_GRID": str(SIMPLE_GRID),
             "NBX_SIMPLE_SLICE_BYTES": str(SIMPLE_SLICE)},
}
PROTO_MASK = {"ll": 1, "ll128": 2, "simple": 4, "ring": 4}   # nbxDebugProtoMask of NCCL_PROTO
DEFAULT_SETTINGS = {"llMax": 64 << 10, "l128Max": 1 << 20, "groupBatch": 1}


def itemsize(oracle, dtype):
    return np.dtype(oracle.NP_STORAGE[dtype]).itemsize


def is_simple(path):
    return path in ("simple", "ring")


def seg_count(path, kind, s, eb, n):
    """Elements of segment s: the message (LL / LL128, AllReduce count or
    ReduceScatter recvcount), or for Simple the block (ReduceScatter recvcount)
    and n blocks minus s % 4 elements (AllReduce count)."""
    b = SEG_BYTES[path][s]
    be = 1 if b is ONE else max(1, b // eb)
    if is_simple(path) and kind == "ar":
        return n * be - s % 4
    return be


def seg_counts(path, kind, eb, n):
    return [seg_count(path, kind, s, eb, n) for s in range(N_SEGS)]


def send_shift(s, eb):
    return (s * eb) % 16


def recv_shift(s, eb):
    return ((s + 3) * eb) % 16


Slot = namedtuple("Slot", "pair seg dtype op eb count send_elts send_off recv_off in_place")


def _take(cursor, shift, nbytes):
    """A region [guard][shift][data][guard] from a 16-byte boundary: (data offset, next cursor)."""
    data = cursor + GUARD + shift
    return data, (data + nbytes + GUARD + 15) & ~15


@functools.lru_cache(maxsize=None)
def layout(oracle, path, kind, n, rank):
    """Where every call of one group lives: (slots, send arena bytes, recv arena
    bytes). Offsets are bytes inside the rank's send and recv arenas (two
    16-byte-aligned allocations filled with 0xA5); the in-place segment's recv
    offset lies in the SEND arena: its send (AllReduce), or the rank's own block
    of its send (ReduceScatter)."""
    slots, cs, cr = [], 0, 0
    for pi, (dt, op) in enumerate(TYPE_OPS):
        eb = itemsize(oracle, dt)
        for s in range(N_SEGS):
            count = seg_count(path, kind, s, eb, n)
            total = count * n if kind == "rs" else count
            so, cs = _take(cs, send_shift(s, eb), total * eb)
            if s == IN_PLACE:
                ro = so + (rank * count * eb if kind == "rs" else 0)
            else:
                ro, cr = _take(cr, recv_shift(s, eb), count * eb)
            slots.append(Slot(pi, s, dt, op, eb, count, total, so, ro, s == IN_PLACE))
    return tuple(slots), cs, cr


RECV_BASE = 1 << 40   # the recv arena's origin for the cut's mirror: far from the send arena


def group_calls(oracle, path, kind, n, rank):
    """The 64 calls as mp_diag.group_runs takes them."""
    slots, _, _ = layout(oracle, path, kind, n, rank)
    return [mp_diag.GroupCall(kind, sl.dtype, sl.eb, sl.op, sl.count, sl.send_off,
                              sl.recv_off if sl.in_place else RECV_BASE + sl.recv_off) for sl in slots]


def seed_of(dtype, path, s):
    return 7_000_003 * dtype + 1_009 * PATHS.index(path) + s


@functools.lru_cache(maxsize=None)
def _sources(oracle, dtype, path, s, total, n_srcs):
    xs = mi.edge_inputs(oracle, dtype, n_srcs, total, seed_of(dtype, path, s))
    for x in xs:
        x.setflags(write=False)
    return xs


def rank_inputs(oracle, path, kind, pi, s, n, n_srcs=None):
    """Sources 0 .. n_srcs-1 of mi.edge_inputs: rank r is source r, seeded per (type, path, segment)."""
    dt = TYPE_OPS[pi][0]
    count = seg_count(path, kind, s, itemsize(oracle, dt), n)
    return _sources(oracle, dt, path, s, count * n if kind == "rs" else count, n if n_srcs is None else n_srcs)


def send_image(oracle, path, kind, n, rank):
    """The rank's send arena as uploaded."""
    slots, nbytes, _ = layout(oracle, path, kind, n, rank)
    img = np.full(nbytes, 0xA5, dtype=np.uint8)
    for sl in slots:
        x = np.ascontiguousarray(rank_inputs(oracle, path, kind, sl.pair, sl.seg, n, rank + 1)[rank]).view(np.uint8)
        img[sl.send_off:sl.send_off + x.size] = x
    return img


def expected(oracle, path, kind, pi, s, n):
    """{rank: expected output} of one segment (tests/edges/cases.expected's
    pattern): the oracle in the schedule's own operand order — direct (LL,
    LL128, Simple): left fold b+1, ..., b of every block, the blocks taken from
    this segment's own count; ring: ring_chain along the same order."""
    dt, op = TYPE_OPS[pi]
    xs = rank_inputs(oracle, path, kind, pi, s, n)
    count = seg_count(path, kind, s, xs[0].itemsize, n)
    devop, arg = oracle.host_to_dev_redop(op, dt, n)

    def fold(parts):
        if path == "ring":
            return ring_chain(oracle, parts, dt, devop, arg, n)
        return oracle.reduce_multi(parts, dt, devop, arg, n_pre_op_srcs=n, post_op=devop == 4)[0]

    if kind == "rs":
        return {b: fold([xs[(b + 1 + k) % n][b * count:(b + 1) * count] for k in range(n)]) for b in range(n)}
    full = np.empty(count, dtype=xs[0].dtype)
    for b, (lo, hi) in enumerate(_blocks(count, xs[0].itemsize, n)):
        if hi > lo:
            full[lo:hi] = fold([xs[(b + 1 + k) % n][lo:hi] for k in range(n)])
    return {r: full for r in range(n)}


def launch_geometry(path, kind, eb, n, grid=SIMPLE_GRID, slice_bytes=SIMPLE_SLICE):
    """mp_diag.simple_group_geometry of one launch of the Simple tables (every launch of a width is alike)."""
    assert is_simple(path)
    return mp_diag.simple_group_geometry([(kind, c) for c in seg_counts(path, kind, eb, n)], eb, n, grid, slice_bytes,
                                         ring=path == "ring")


def launch_units(path, kind, eb, n):
    """mp_diag.ll_group_units of one launch of the LL / LL128 tables."""
    return mp_diag.ll_group_units(seg_counts(path, kind, eb, n), eb, UNIT[path])


# ---------------------------------------------------------------------------
# the grouped model (tests/simple_model.py) over the Simple tables

def model_fold(dtype_np):
    """Wrapping integer sums stand in for the folds: the protocol state does not depend on the values."""
    def fold(srcs, pre_mask=None, post=True):
        acc = srcs[0].view(dtype_np)
        for x in srcs[1:]:
            acc = acc + x.view(dtype_np)
        return np.ascontiguousarray(acc).view(np.uint8)
    return fold


def run_model_groups(sm, n, path, kinds=KINDS, grid=SIMPLE_GRID, slice_bytes=SIMPLE_SLICE, slots=SIMPLE_SLOTS,
                     widths=None, mutate=None, comm=None, seed=0):
    """The Simple communicator's life in test_group_segments on the model: for
    every kind, one grouped launch per (type, op) pair, segment data random
    bytes folded as wrapping unsigned sums. widths: the element width of every
    launch, in order (default: TYPE_OPS'). mutate: geometry -> geometry (a
    deliberately wrong cut). Returns (model communicator, outputs[kind][launch]
    [segment][rank])."""
    comm = comm or sm.Comm(n, grid, slice_bytes, slots)
    widths = widths or [1, 1, 2, 2, 4, 4, 8, 8]
    outputs = {}
    for kind in kinds:
        outputs[kind] = []
        for li, eb in enumerate(widths):
            counts = seg_counts(path, kind, eb, n)
            geom = mp_diag.simple_group_geometry([(kind, c) for c in counts], eb, n, grid, slice_bytes,
                                                 ring=path == "ring")
            if mutate:
                geom = mutate(geom)
            rng = np.random.default_rng([seed, li, eb, n])
            sends = [[rng.integers(0, 256, (c * n if kind == "rs" else c) * eb, dtype=np.uint8) for _r in range(n)]
                     for c in counts]
            recvs = [[np.full(c * eb, 0xA5, np.uint8) for _r in range(n)] for c in counts]
            sm.run_group(comm, kind, geom, sends, recvs, eb, model_fold(mi.UINT_OF[eb]), ring=path == "ring")
            outputs[kind].append(recvs)
    return comm, outputs


# ---------------------------------------------------------------------------
# Section 2: one group per cut rule (test_group_cut_rules), n in 2, 3

CUT_NS = (2, 3)
LL_COUNT, LL128_COUNT, SIMPLE_COUNT, TWO_SHOT_COUNT = 1000, 30000, 300000, 100000   # 4-byte elements, default limits
PREMUL_INTS = (3, -2, 5)   # the user PreMulSum's scalar on rank 0, 1, 2

# kind, dtype, op, count, root, send / recv as (buffer name, element offset), stream index, flags
Call = namedtuple("Call", "kind dtype op count root send recv stream premul null_recv", defaults=(0, False, False))


def _ar(count, send, recv, dtype=INT32, op=SUM, **kw):
    return Call("ar", dtype, op, count, 0, (send, 0), (recv, 0), **kw)


def _rs(count, send, recv, dtype=INT32, op=SUM):
    return Call("rs", dtype, op, count, 0, (send, 0), (recv, 0))


def _red(count, send, recv, root, null_recv=False):
    return Call("red", INT32, SUM, count, root, (send, 0), (recv, 0), null_recv=null_recv)


def _fresh(k, count, **kw):
    return _ar(count, f"s{k}", f"r{k}", **kw)


def cut_groups(n, settings=None):
    """{name: [Call]}: one group per rule, in run order. Counts that depend on
    the LL / LL128 limits come from the communicator's settings."""
    st = dict(DEFAULT_SETTINGS, **(settings or {}))
    root = 1 % n
    ll_cap_count = st["llMax"] * 3 // 8 // 4          # 3/8 of the LL slot: two fit, a third does not
    l128_lines = mp_diag.l128_slot_lines(st["l128Max"])
    l128_count = 50000                                # 200,000 B: LL128 one-shot at any n
    l128_fit = l128_lines // -(-l128_count * 4 // 48)
    g = {}
    g["max_segs_17"] = [_fresh(k, 10) for k in range(17)]
    g["max_segs_40"] = [_fresh(k, 10, dtype=F32) for k in range(40)]
    g["ll_capacity"] = [_ar(ll_cap_count, "s", f"r{k}") for k in range(5)]
    g["ll128_capacity"] = [_ar(l128_count, "s", f"r{k}") for k in range(l128_fit + 2)]
    g["proto_change"] = [_ar(c, f"s{c}", f"r{k}") for k, c in
                         enumerate((LL_COUNT, LL_COUNT, LL128_COUNT, LL128_COUNT, SIMPLE_COUNT, SIMPLE_COUNT, LL_COUNT))]
    g["ll128_two_shot"] = [_ar(c, f"s{c}", f"r{k}") for k, c in
                           enumerate((TWO_SHOT_COUNT, TWO_SHOT_COUNT, LL128_COUNT, LL128_COUNT))]
    g["kind_change"] = [_ar(100, "s0", "r0"), _ar(100, "s1", "r1"), _rs(100, "s2", "r2"), _rs(100, "s3", "r3"),
                        _ar(100, "s4", "r4"), _ar(100, "s5", "r5")]
    g["op_change"] = [_fresh(0, 100), _fresh(1, 100), _fresh(2, 100, op=MAX), _fresh(3, 100, op=MAX)]
    g["type_change"] = [_fresh(0, 100, dtype=F32), _fresh(1, 100, dtype=F32), _fresh(2, 100), _fresh(3, 100)]
    g["reduce_between"] = [_fresh(0, 100), _fresh(1, 100), _red(100, "s2", "r2", root), _fresh(3, 100), _fresh(4, 100)]
    g["two_reduces"] = [_red(100, "s0", "r0", root), _red(100, "s1", "r1", root)]
    g["null_recv"] = [_fresh(0, 100), _fresh(1, 100), _red(100, "s2", "r2", root, null_recv=True), _fresh(3, 100),
                      _fresh(4, 100)]
    g["zero_inside"] = [_fresh(0, 100), _fresh(1, 100), _fresh(2, 0), _fresh(3, 100), _fresh(4, 100)]
    g["zero_first"] = [_fresh(0, 0), _fresh(1, 100), _fresh(2, 100), _fresh(3, 100)]
    g["user_premul"] = [_fresh(0, 100), _fresh(1, 100), _fresh(2, 100, premul=True), _fresh(3, 100), _fresh(4, 100)]
    # the read / write conflict cut
    g["chain"] = [_ar(100, "a", "b"), _ar(100, "b", "c")]
    g["same_recv"] = [_ar(100, "a", "c"), _ar(100, "b", "c")]
    g["writes_earlier_send"] = [_ar(100, "a", "b"), _ar(100, "c", "a")]
    g["shared_send"] = [_ar(100, "a", "b"), _ar(100, "a", "c")]
    g["in_place_among"] = [_ar(100, "a", "b"), _ar(100, "c", "c"), _ar(100, "d", "e")]
    # two streams inside one run: one launch, on the first call's stream
    g["two_streams"] = [_fresh(k, 100, stream=k % 2) for k in range(4)]
    return g


BATCH_OFF_GROUP = "max_segs_17"      # what the NBX_GROUP_BATCH=0 communicator runs
# the launches each rule must leave at 3 ranks on default settings, as segment counts (0: a call alone)
CUT_EXPECT_3 = {
    "max_segs_17": [16, 0], "max_segs_40": [16, 16, 8], "ll_capacity": [2, 2, 0], "proto_change": [2, 2, 2, 0],
    "ll128_two_shot": [0, 0, 2], "kind_change": [2, 2, 2], "op_change": [2, 2], "type_change": [2, 2],
    "reduce_between": [2, 0, 2], "two_reduces": [0, 0], "null_recv": [2, 0, 2], "zero_inside": [2, 2],
    "zero_first": [3], "user_premul": [2, 0, 2], "chain": [0, 0], "same_recv": [0, 0],
    "writes_earlier_send": [0, 0], "shared_send": [2], "in_place_among": [3], "two_streams": [4],
}
# the cut reason each rule is there for
CUT_REASON = {
    "max_segs_17": "max_segs", "max_segs_40": "max_segs", "ll_capacity": "capacity", "ll128_capacity": "capacity",
    "proto_change": "proto", "ll128_two_shot": "proto", "kind_change": "op", "op_change": "op", "type_change": "op",
    "reduce_between": "reduce", "two_reduces": "reduce", "null_recv": "reduce", "zero_inside": "zero_count",
    "zero_first": "zero_count", "user_premul": "user_premul", "chain": "conflict", "same_recv": "conflict",
    "writes_earlier_send": "conflict",
}


def buffer_layout(calls, n):
    """{buffer name: (byte offset, elements, dtype)} and the arena's size: every
    named buffer of a group, 256-byte aligned with 64 guard bytes between, as
    long as its longest use; its dtype is its first use's."""
    need, dts = {}, {}
    for c in calls:
        for (name, off), elts in ((c.send, c.count * (n if c.kind == "rs" else 1)), (c.recv, c.count)):
            need[name] = max(need.get(name, 1), off + elts)
            dts.setdefault(name, c.dtype)
    out, cur = {}, 64
    for name in need:
        cur = (cur + 255) & ~255
        out[name] = (cur, need[name], dts[name])
        cur += need[name] * 4 + 64
    return out, (cur + 255) & ~255


def buffer_image(name_index, gi, nelts, dtype, n, rank):
    """A buffer's first contents: full-range int32, or small whole numbers as f32 (sums stay exact)."""
    rng = np.random.default_rng([20261021, gi, name_index, n, rank])
    if dtype == F32:
        return rng.integers(-100, 100, nelts).astype(np.float32)
    return rng.integers(-2**31, 2**31 - 1, nelts, dtype=np.int32, endpoint=True)


def arena_image(gi, calls, n, rank):
    lay, size = buffer_layout(calls, n)
    img = np.full(size, 0xA5, dtype=np.uint8)
    for k, (name, (off, nelts, dt)) in enumerate(lay.items()):
        img[off:off + 4 * nelts] = buffer_image(k, gi, nelts, dt, n, rank).view(np.uint8)
    return img


def cut_group_calls(calls, n, rank):
    """A group as mp_diag.group_runs takes it on one rank (a user PreMulSum's
    scalar is the rank's own; every rank still passes a PreMulSum)."""
    lay, _ = buffer_layout(calls, n)
    out = []
    for c in calls:
        send = lay[c.send[0]][0] + 4 * c.send[1]
        recv = None if (c.null_recv and rank != c.root) else lay[c.recv[0]][0] + 4 * c.recv[1]
        out.append(mp_diag.GroupCall(c.kind, c.dtype, 4, ("premul",) if c.premul else c.op, c.count, send, recv, c.root,
                                     c.premul))
    return out


def simulate(gi, calls, n):
    """Every rank's arena after the group, the calls folded in call order on the
    host. Integer sums wrap, the f32 values are small whole numbers and Max is
    exact, so the operand order does not show."""
    lay, _ = buffer_layout(calls, n)
    arenas = [arena_image(gi, calls, n, r) for r in range(n)]

    def view(r, ref, elts, dt):
        off = lay[ref[0]][0] + 4 * ref[1]
        return arenas[r][off:off + 4 * elts].view(np.float32 if dt == F32 else np.int32)

    for c in calls:
        if c.count == 0:
            continue
        total = c.count * (n if c.kind == "rs" else 1)
        xs = [view(r, c.send, total, c.dtype).copy() for r in range(n)]
        if c.premul:
            xs = [x * np.int32(PREMUL_INTS[r]) for r, x in enumerate(xs)]
        acc = xs[0]
        for x in xs[1:]:
            acc = np.maximum(acc, x) if c.op == MAX else acc + x
        for r in range(n):
            if c.kind == "red" and r != c.root:
                continue
            view(r, c.recv, c.count, c.dtype)[:] = acc[r * c.count:(r + 1) * c.count] if c.kind == "rs" else acc
    return arenas
