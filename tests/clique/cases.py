"""Case tables of the in-process clique's in-kernel transport tests, shared by
the worker (tests/clique/worker.py), the GPU tests
(tests/clique/test_clique_transport_gpu.py) and their CPU companion
(tests/test_clique_cases_cpu.py).

ncclCommInitAll runs a collective in one of two ways (comm_clique.cc): the
event-ordered fold (runCliqueColl / runCliqueBatch: nbxReduceMulti between
event exchanges, launch families 1-5) or the in-kernel transport
(cliqueInKernel -> cliqueRunLL -> runMpGroup: one kLLColl / kLL128Coll /
kLL128AllReduce2 / kSimpleColl / kSimpleRing launch per rank, families 8-12).
One thread drives every rank, so the calling thread's launch record holds the
launches of all n ranks of a case, rank after rank.

Operand order. cliqueRunLL hands every rank's calls to runMpGroup, which builds
the same LLArgs / SimpleArgs as on a multi-process communicator (mpLaunchLL,
mpLaunchSimple: rank, nRanks, blockRange blocks, the ring flag from NCCL_ALGO)
— only the peer tables differ (direct pointers instead of IPC maps). Block b
is therefore folded b+1, ..., b (a Reduce: root+1, ..., root) and ring_chain
applies along the ring: tests/edges/cases.expected is the expectation, unchanged.
The fold path (cliqueBlock) folds block r in the same order r+1, ..., r and a
Reduce root+1, ..., root for every block, so `simulate` below serves both.

Part 1 is tests/edges/cases.py's table itself (imported, never copied), at 2, 3
and 5 ranks; part 2 a short table at 8 ranks; part 3 one scenario per routing
rule of cliqueInKernel; part 4 groups, the hand-over between the two paths, in
place calls and the user PreMulSum.

Two things the default protocol set decides differently from what a size
alone suggests, both checked against nbxDebugChooseProto by the worker and by
the CPU companion:
  * the byte-bound sizes (262,140 .. 262,152 B) and the 300,011 B call are
    LL128-sized under the default thresholds (LL up to 64 KiB, LL128 up to
    1 MiB), and an LL128-sized call runs in-kernel whatever
    NBX_CLIQUE_SIMPLE / NBX_CLIQUE_SIMPLE_MAX_BYTES say. The byte-bound
    communicator is therefore created with NCCL_PROTO=Simple, and the
    NBX_CLIQUE_SIMPLE=0 one with NCCL_PROTO=^LL128 (20,011 B stays LL,
    300,011 B becomes Simple-sized);
  * a fold on distinct streams happens only to a Simple-sized call above
    NBX_CLIQUE_SIMPLE_MAX_BYTES, so the chain's last link (the fold on
    streams A) reads y3 as the head of a 300,000-element buffer whose first
    1,000 elements the in-kernel links wrote, on a communicator whose bound is
    262,144 B.
"""
import functools
from collections import namedtuple

import numpy as np

from tests import mp_diag
from tests.edges import cases as edges
from tests.test_multiprocess_gpu import _blocks, _ll_input, _premul_expected, _premul_scalar  # noqa: F401

# part 1 runs the edge table itself
PATHS, PATH_COMM, PATH_KINDS, COMM_ENV, COMMS, NS = (edges.PATHS, edges.PATH_COMM, edges.PATH_KINDS, edges.COMM_ENV,
                                                     edges.COMMS, edges.NS)
path_cases, root_of, rank_input, expected, family_of, host_unroll = (edges.path_cases, edges.root_of,
                                                                     edges.rank_input, edges.expected,
                                                                     edges.family_of, edges.host_unroll)
count_of, shift_of, itemsize, nbytes_of = edges.count_of, edges.shift_of, edges.itemsize, edges.nbytes_of

SUM, PROD, MAX, MIN, AVG = range(5)
INT8, INT32, F16, F32, BF16 = 0, 2, 6, 7, 9
FOLD_FAMILIES = (1, 2, 3, 4, 5)          # nbxReduceMulti's kernels: the fold path, and a user PreMulSum's pre-pass
GUARD = 16                               # bytes of 0xA5 either side of every buffer
SEGS_SHIFT = 8                           # launch record flags: group segments from bit 8

# ---------------------------------------------------------------------------
# the rig: one fresh process per test, every stream on its own hardware queue

HW_QUEUES = 24                           # scripts/clique_stress.py's value; never above 32
CHILD_ENV = dict({"GPU_MAX_HW_QUEUES": str(HW_QUEUES), "NBX_CLIQUE_LL": "1", "NBX_TIMEOUT_SEC": "5"},
                 **edges.PROCESS_ENV)
# unset while a communicator is created unless it names them; NBX_CLIQUE_LL goes back to 1
ENV_KEYS = edges.ENV_KEYS + ("NBX_CLIQUE_SIMPLE", "NBX_CLIQUE_SIMPLE_MAX_BYTES")
# never inherited from the caller: they change a size's protocol, a grid or a check
SCRUB_ENV = ENV_KEYS + ("NBX_CHECK_PLANS", "NCCL_CHECK_POINTERS", "NBX_CHECK_SLICES", "NBX_SIMPLE_SLICE_BYTES",
                        "NCCL_BUFFSIZE", "NBX_LL_MAX_BYTES", "NCCL_LL_BUFFSIZE", "NBX_LL128_MAX_BYTES",
                        "NCCL_LL128_BUFFSIZE", "NBX_GROUP_BATCH", "NBX_LL_MAX_GRID", "NCCL_MAX_NCHANNELS",
                        "NCCL_MIN_NCHANNELS", "NBX_SIMPLE_SLOTS", "NBX_STREAM_ORDER")
TWO_STREAM_MAX_N = 3                     # the chain gives every rank two streams


def streams_needed(n, two_per_rank=False):
    """Streams the worker creates for n ranks: one per rank (two for the chain)
    plus the shared one. The default stream comes on top."""
    return n * (2 if two_per_rank else 1) + 1


# ---------------------------------------------------------------------------
# part 2: eight ranks, briefly

EIGHT_N = 8
EIGHT_PATHS = ("ll", "ll128", "ll128x2", "simple", "ring")
EIGHT_TYPES, EIGHT_OPS = (F32, BF16), (SUM, AVG)


def eight_cases(path):
    """[(kind, dtype, op)] of one path at eight ranks; a Reduce's root is root_of(index, 8)."""
    return [(kind, dt, op) for kind in PATH_KINDS[path] for dt in EIGHT_TYPES for op in EIGHT_OPS]


# ---------------------------------------------------------------------------
# parts 3 and 4 as scenarios: named buffers, groups of calls, expected records

ROUTE_N = 3
# kind, dtype, op, count, send / recv buffer names, stream ("own": the rank's stream A, "own2": its stream B,
# "shared"), root, bad_rank: that rank passes count - 1 (the mismatched collective)
Call = namedtuple("Call", "kind dtype op count send recv stream root bad_rank", defaults=("own", 0, None))
# expect: per group a list of phases, in record order —
#   ("kernel", family, unroll, flags): exactly n records (family, n, unroll, flags), one per rank
#   ("fold",): one or more records of families 1-5, nothing else
#   ("error", code): ncclGroupEnd returns that code and records nothing
# and [] for a group that must leave no record at all.
# sync: the worker synchronises and reads every rank's async error after each group (False: only at the end)
Scenario = namedtuple("Scenario", "name comm groups expect sync protos", defaults=(True, None))

SCENARIO_COMM_ENV = {
    "default": {},
    "bound": {"NCCL_PROTO": "Simple", "NBX_CLIQUE_SIMPLE_MAX_BYTES": "262144"},
    "nosimple": {"NCCL_PROTO": "^LL128", "NBX_CLIQUE_SIMPLE": "0"},
    "off": {"NBX_CLIQUE_LL": "0"},
    "chain": {"NBX_CLIQUE_SIMPLE_MAX_BYTES": "262144"},
}
IN_KERNEL_COMMS = ("default", "bound", "nosimple", "chain")   # nbxDebugCommProtoMask >= 0; "off": == -1
BOUND_BYTES = 262144
# (kind, count, bytes sent, in-kernel) of the byte-bound cases, fp32
BOUND_CASES = (("ar", 65536, 262144, True), ("ar", 65537, 262148, False),
               ("rs", 21845, 262140, True), ("rs", 21846, 262152, False))
FAM_LL, FAM_SIMPLE = edges.FAM_LL, edges.FAM_SIMPLE
P_SIMPLE, P_LL = edges.P_SIMPLE, edges.P_LL
LL_COUNT = 1000                          # fp32: 4,000 B, LL under the default thresholds
BIG_COUNT = 300000                       # fp32: 1,200,000 B, Simple-sized under the default thresholds


def _ar(count, send, recv, stream="own", dtype=F32, **kw):
    return Call("ar", dtype, SUM, count, send, recv, stream, **kw)


def _k(family, unroll, segs=0):
    return ("kernel", family, unroll, segs << SEGS_SHIFT)


def routing_scenarios():
    """Part 3: one deterministic case per rule of cliqueInKernel, n = ROUTE_N."""
    bound_groups, bound_expect = [], []
    for i, (kind, count, _, inside) in enumerate(BOUND_CASES):
        bound_groups.append([Call(kind, F32, SUM, count, f"s{i}", f"r{i}")])
        bound_expect.append([_k(FAM_SIMPLE, 0)] if inside else [("fold",)])
    return [
        Scenario("shared_stream", "default", [[_ar(LL_COUNT, "s", "r", "shared")]], [[("fold",)]]),
        Scenario("count_zero", "default", [[_ar(0, "s", "r")]], [[]]),
        Scenario("simple_byte_bound", "bound", bound_groups, bound_expect, protos=[[P_SIMPLE]] * 4),
        Scenario("clique_simple_off", "nosimple",
                 [[_ar(edges.SIMPLE_BYTES, "s0", "r0", dtype=INT8)], [_ar(edges.LL_BYTES, "s1", "r1", dtype=INT8)]],
                 [[("fold",)], [_k(FAM_LL, 1)]], protos=[[P_SIMPLE], [P_LL]]),
        Scenario("clique_ll_off", "off",
                 [[_ar(edges.LL_BYTES, "s0", "r0", dtype=INT8)], [_ar(edges.SIMPLE_BYTES, "s1", "r1", dtype=INT8)],
                  [_ar(BIG_COUNT, "s2", "r2")]],
                 [[("fold",)], [("fold",)], [("fold",)]]),
        # runCliqueColl returns ncclInvalidUsage before anything is launched, and flushPendingImpl has
        # already taken the round off every rank's queue: the next call runs as if nothing had happened
        Scenario("mismatched_collective", "default",
                 [[_ar(LL_COUNT, "s0", "r0", bad_rank=1)], [_ar(LL_COUNT, "s1", "r1")]],
                 [[("error", 5)], [_k(FAM_LL, 1)]]),
    ]


SEGMENT_COUNTS = (1, 5, 250, 1000, 2051, 4099)   # six LL-sized fp32 AllReduces: 29,624 B, one LL slot


def group_scenarios():
    """Part 4's groups and the hand-over between the two paths, n = ROUTE_N."""
    return [
        # one launch per rank that carries all six segments
        Scenario("segment_table", "default", [[_ar(c, f"s{k}", f"r{k}") for k, c in enumerate(SEGMENT_COUNTS)]],
                 [[_k(FAM_LL, 1, len(SEGMENT_COUNTS))]]),
        # the third call reads what the second writes: the in-kernel run is cut there (spansConflict)
        Scenario("buffer_dependency", "default",
                 [[_ar(LL_COUNT, "a", "b"), _ar(LL_COUNT, "c", "d"), _ar(LL_COUNT, "d", "e")]],
                 [[_k(FAM_LL, 1, 2), _k(FAM_LL, 1)]]),
        Scenario("mixed_group", "default",
                 [[_ar(LL_COUNT, "a", "b"), _ar(BIG_COUNT, "c", "d", "shared"), _ar(LL_COUNT, "e", "f")]],
                 [[_k(FAM_LL, 1), ("fold",), _k(FAM_LL, 1)]]),
        # in-kernel on A -> fold on the shared stream -> in-kernel on B -> fold on A, no host synchronisation
        Scenario("chain", "chain",
                 [[_ar(LL_COUNT, "x", "y1")], [_ar(LL_COUNT, "y1", "y2", "shared")],
                  [_ar(LL_COUNT, "y2", "y3", "own2")], [_ar(BIG_COUNT, "y3", "y4")]],
                 [[_k(FAM_LL, 1)], [("fold",)], [_k(FAM_LL, 1)], [("fold",)]], sync=False),
    ]


F32_INPUT_MAX = 8   # |x| of every fp32 scenario input: small whole numbers, every order of summation is exact


def chain_bound(n, links=4):
    """Largest magnitude the chain can reach: every link multiplies by at most n."""
    return F32_INPUT_MAX * n ** links


def buffer_specs(sc, n):
    """{name: (elements, dtype, is_input)} of a scenario's buffers, in first-use order: as long as
    the longest use (at least one element), an input when any call reads it."""
    need, dts, read = {}, {}, set()
    for g in sc.groups:
        for c in g:
            for name, elts in ((c.send, c.count * (n if c.kind == "rs" else 1)), (c.recv, c.count)):
                need[name] = max(need.get(name, 1), elts)
                dts.setdefault(name, c.dtype)
            read.add(c.send)
    return {name: (need[name], dts[name], name in read) for name in need}


def buffer_image(oracle, sc_index, name_index, elts, dtype, rank):
    """A buffer's first contents: small whole numbers as fp32, full-range integers otherwise."""
    rng = np.random.default_rng([20261021, sc_index, name_index, rank])
    if dtype == F32:
        return rng.integers(-F32_INPUT_MAX, F32_INPUT_MAX, elts, endpoint=True).astype(np.float32)
    st = np.dtype(oracle.NP_STORAGE[dtype])
    return rng.integers(np.iinfo(st).min, np.iinfo(st).max, elts, dtype=st, endpoint=True)


def initial_buffers(oracle, sc_index, sc, n):
    """[rank][name] -> the data bytes (np.uint8) every buffer starts with: inputs by buffer_image,
    pure outputs 0xA5."""
    out = []
    for r in range(n):
        bufs = {}
        for k, (name, (elts, dt, is_input)) in enumerate(buffer_specs(sc, n).items()):
            eb = itemsize(oracle, dt)
            bufs[name] = (np.ascontiguousarray(buffer_image(oracle, sc_index, k, elts, dt, r)).view(np.uint8).copy()
                          if is_input else np.full(elts * eb, 0xA5, np.uint8))
        out.append(bufs)
    return out


def simulate(oracle, sc_index, sc, n):
    """[rank][name] -> data bytes after the scenario: the calls folded in call order by the oracle,
    block b in the order b+1, ..., b (a Reduce root+1, ..., root) — the order of both paths. A call
    with a bad_rank changes nothing (it must fail before anything is launched)."""
    bufs = initial_buffers(oracle, sc_index, sc, n)
    for g in sc.groups:
        for c in g:
            if c.count == 0 or c.bad_rank is not None:
                continue
            st = oracle.NP_STORAGE[c.dtype]
            eb = itemsize(oracle, c.dtype)
            total = c.count * (n if c.kind == "rs" else 1)
            xs = [bufs[r][c.send][:total * eb].view(st).copy() for r in range(n)]
            devop, arg = oracle.host_to_dev_redop(c.op, c.dtype, n)

            def fold(first, lo, hi):
                return oracle.reduce_multi([xs[(first + k) % n][lo:hi] for k in range(n)], c.dtype, devop, arg,
                                           n_pre_op_srcs=n, post_op=devop == 4)[0]
            if c.kind == "rs":
                outs = {r: fold(r + 1, r * c.count, (r + 1) * c.count) for r in range(n)}
            elif c.kind == "red":
                outs = {c.root: fold(c.root + 1, 0, c.count)}
            else:
                full = np.empty(c.count, dtype=st)
                for b, (lo, hi) in enumerate(_blocks(c.count, eb, n)):
                    if hi > lo:
                        full[lo:hi] = fold(b + 1, lo, hi)
                outs = {r: full for r in range(n)}
            for r, y in outs.items():
                bufs[r][c.recv][:c.count * eb] = np.ascontiguousarray(y).view(np.uint8)
    return bufs


def group_plan(oracle, group, n, settings):
    """mp_diag.group_runs (the mirror of runMpGroup's cut) over one group whose calls all run in-kernel
    in one cliqueRunLL run; every buffer at its own address."""
    names = {}
    for c in group:
        for name in (c.send, c.recv):
            names.setdefault(name, (len(names) + 1) << 32)
    calls = [mp_diag.GroupCall(c.kind, c.dtype, itemsize(oracle, c.dtype), c.op, c.count, names[c.send], names[c.recv],
                               c.root) for c in group]
    return mp_diag.group_runs(calls, n, settings)


def match_records(recs, phases, n):
    """None when the launch record `recs` is exactly what `phases` describe, else a description."""
    recs = [tuple(r) for r in recs]
    at = 0
    for ph in phases:
        if ph[0] == "kernel":
            want = [(ph[1], n, ph[2], ph[3])] * n
            if recs[at:at + n] != want:
                return f"records {recs}: expected {want} at index {at} (phases {phases})"
            at += n
        elif ph[0] == "fold":
            k = at
            while k < len(recs) and recs[k][0] in FOLD_FAMILIES:
                k += 1
            if k == at:
                return f"records {recs}: expected fold-path records (families 1-5) at index {at} (phases {phases})"
            at = k
        elif ph[0] == "premul":   # per rank: one pre-pass of the fold families, then the collective's kernel
            for _ in range(n):
                if not (at + 1 < len(recs) and recs[at][0] in FOLD_FAMILIES and recs[at + 1] == (ph[1], n, ph[2], 0)):
                    return f"records {recs}: expected a pre-pass and {(ph[1], n, ph[2], 0)} at index {at}"
                at += 2
        elif ph[0] != "error":
            raise ValueError(ph)
    if at != len(recs):
        return f"records {recs}: {len(recs) - at} more than the phases {phases} describe"
    return None


def well_formed(phases):
    for ph in phases:
        if ph[0] == "kernel":
            assert len(ph) == 4 and ph[1] in (8, 9, 10, 11, 12) and ph[2] in (0, 1) and ph[3] >= 0 and ph[3] % 256 == 0
            assert ph[2] == (0 if ph[1] in (11, 12) else 1)
        elif ph[0] == "premul":
            assert len(ph) == 3 and ph[1] in (8, 9, 10, 11, 12) and ph[2] == (0 if ph[1] in (11, 12) else 1)
        elif ph[0] == "error":
            assert len(ph) == 2 and ph[1] > 0 and len(phases) == 1
        else:
            assert ph == ("fold",)
    return True


# ---------------------------------------------------------------------------
# part 4: in place, and the user PreMulSum — one call per case, on the edge communicators

def inplace_cases():
    """[(path, kind)]: AllReduce with recv == send and ReduceScatter with recv == send + rank x count,
    once per path, fp16 Sum with the edge inputs."""
    return [(path, kind) for path in PATHS for kind in ("ar", "rs") if kind in PATH_KINDS[path]]


PREMUL_PATHS, PREMUL_TYPES, PREMUL_KINDS = ("ll", "ll128", "simple"), (F16, F32, INT32), ("ar", "rs", "red")


def premul_cases():
    """[(path, kind, dtype, device_scalar)]; the root of a Reduce is 1 % n (_premul_expected's)."""
    return [(path, kind, dt, dev) for path in PREMUL_PATHS for kind in PREMUL_KINDS for dt in PREMUL_TYPES
            for dev in (False, True)]


@functools.lru_cache(maxsize=None)
def premul_inputs(oracle, path, kind, dt, n):
    count = count_of(oracle, path, dt)
    return tuple(_ll_input(kind, dt, count, n, r) for r in range(n))


def premul_expected(oracle, path, kind, dt, n):
    xs = list(premul_inputs(oracle, path, kind, dt, n))
    return _premul_expected(oracle, kind, dt, count_of(oracle, path, dt), n, xs)
