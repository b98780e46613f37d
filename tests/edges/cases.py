"""Case table of the collective edge-value tests, shared by the GPU test
(tests/edges/test_multiprocess_gpu.py) and its CPU companion
(tests/test_collective_edges_cpu.py).

kLLColl, kLL128Coll (l128FoldLine), kLL128AllReduce2, kSimpleColl and
kSimpleRing each carry their own fold loop over the functors, one compiled
instance per (type, op): the LL kernels call the scalar pre / red / post on
8-byte words, simpleFoldU the pack forms at three unrolls picked by source
count (16 for <= 2 sources, 8 for <= 4, 4 above) and the scalar forms on
unaligned buffers and tails. Every (type, op) goes through each of them here
with tests/matrix/inputs.py's edge-rich inputs (random bit patterns, denormals,
+-0, inf, NaN), against the oracle folded in the schedule's own operand order.

A path is one communicator (its environment at creation) and one message size:

  path         communicator  bytes per rank input     kernel meant (launch family)
  ll           ll            20,011                   kLLColl (8)
  ll128        ll128         12,011                   kLL128Coll (9)
  ll128x2      ll128         50,021 (ar, red only)    kLL128AllReduce2 (10); one-shot (9) at 2 ranks
  simple       simple        300,011                  kSimpleColl, pack path (11)
  simple_elts  simple        5,003 elements, send and recv one element past a
                             16-byte boundary         kSimpleColl, element path (11)
  ring         ring          300,011                  kSimpleRing (12)

count = max(1, bytes // itemsize); a ReduceScatter's count is its per-rank
block, so its inputs are n times as long.

Sizes. Odd byte counts leave the last 8-byte LL pack, 48-byte LL128 line and
16-byte Simple pack partial, over more than one workgroup: 20,011 B = 2,502
packs (256 per workgroup pass); 12,011 B = 251 lines, 50,021 B = 1,043 lines
(two-shot: 348 / 209 lines per block at 3 / 5 ranks; 64 lines per workgroup
pass, at most 16 workgroups, so the 2-rank one-shot call of 1,043 lines runs a
second pass).

SIMPLE_BYTES = 300,011 against simpleCollBody's cut (comm_mp_launch.cc
mpLaunchSimple; mp_diag.simple_geometry is the same arithmetic), with a grid of
2 and the default 64 KiB staging slice. One iteration of simpleFoldU is U x 256
packs x 16 B: 65,536 B at U = 16, 32,768 B at U = 8, 16,384 B at U = 4. For
one-byte elements (wider types differ only in the rounding of the block):

  n = 3 (U = 8): block = ceil16(ceil(300,011 / 3)) = 100,016 B; slice =
    ceil16(100,016 / 2) = 50,016 B <= 64 KiB, one round. Workgroup 0 folds
    50,016 B = 3,126 packs = one iteration of 2,048 + a ragged one of 1,078;
    workgroup 1 folds 50,000 B = 3,125 packs = 2,048 + 1,077. The last block
    is 300,011 - 200,032 = 99,979 B: its workgroup 1 folds 49,963 B = 3,122
    packs + 11 B below one pack.
  n = 5 (U = 4): block = 60,016 B; slice = 30,016 B. Workgroup 0: 1,876 packs
    = 1,024 + 852; workgroup 1: 30,000 B = 1,875 packs = 1,024 + 851. Last
    block 59,947 B: workgroup 1 folds 29,931 B = 1,870 packs + 11 B.
  n = 2 (U = 16): block = 150,016 B; ceil16(150,016 / 2) = 75,008 B is above
    the 64 KiB slice, so slice = 65,536 B and there are 2 rounds. Round 0:
    both workgroups fold 65,536 B = exactly one iteration of 4,096 packs.
    Round 1: workgroup 0 folds 150,016 - 131,072 = 18,944 B = 1,184 packs (a
    ragged iteration), workgroup 1 nothing. Last block 149,995 B: round 1 of
    workgroup 0 is 18,923 B = 1,182 packs + 11 B.

So at 3 and 5 ranks every workgroup runs a full iteration, then a ragged one,
and the rank that folds the last block a tail below one pack (only the end of
the message can be a partial pack: blocks are whole packs). At U = 16 a slice
is at most 64 KiB = one iteration, so a full and a ragged iteration can never
share a slice whatever the size: at 2 ranks workgroup 0 runs them in
successive rounds (any block of 128 KiB < B < 192 KiB per rank does this;
above 192 KiB workgroup 1 gets the ragged round and workgroup 0 none) and
workgroup 1 runs whole iterations only. 300,011 B is kept: no size gives more.
The ring folds two sources per hop (U = 16) over the same blocks: one full
and one ragged round of workgroup 0 at 2 ranks, ragged iterations only at 3
and 5 ranks (50,016 B and 30,016 B slices), and its Reduce — the whole
message as one block — four full slices and a ragged one at every n.
A ReduceScatter block starts at b x count elements of the send buffer, which
for these odd counts is a 16-byte boundary only for some b: those ranks fold
by packs, the others by elements (simpleCollBody's `aligned`).
tests/test_collective_edges_cpu.py asserts this arithmetic.
"""
import functools

import numpy as np

from tests import mp_diag
from tests.matrix import inputs as mi
from tests.test_multiprocess_gpu import _blocks, _ll_root, ring_chain

ALL_TYPES = tuple(range(12))
NS = (2, 3, 5)
SUM, PROD, MAX, MIN, AVG = range(5)                       # ncclRedOp_t
OPS = {"ar": (SUM, PROD, MAX, MIN, AVG), "rs": (SUM, MAX, AVG), "red": (SUM, MAX, AVG)}

# launch families (include/nbx_debug.h nbxDebugLaunchLog)
FAM_LL, FAM_LL128, FAM_LL128X2, FAM_SIMPLE, FAM_RING = 8, 9, 10, 11, 12
# nbxDebugChooseProto's answers
P_LL, P_LL128, P_SIMPLE, P_LL128X2 = 0, 1, 2, 3

LL_BYTES, LL128_BYTES, LL128X2_BYTES, SIMPLE_BYTES, ELTS_COUNT = 20011, 12011, 50021, 300011, 5003
LL128_ONESHOT_MAX, LL128_MAX_GRID, SIMPLE_GRID = 16384, 16, 2

# the environment a communicator is created under; every key of ENV_KEYS that
# a communicator does not name is unset while it is created. NBX_LL128_MAX_GRID
# is read once per process, at its first LL128 launch (the ranks share one GPU
# and every rank's grid has to stay resident), so the test sets it for the
# whole process as well.
ENV_KEYS = ("NCCL_PROTO", "NCCL_ALGO", "NBX_LL128_ONESHOT_MAX", "NBX_SIMPLE_MAX_GRID")
PROCESS_ENV = {"NBX_LL128_MAX_GRID": "16"}
COMM_ENV = {
    "ll": {"NCCL_PROTO": "LL"},
    "ll128": {"NCCL_PROTO": "LL128", "NBX_LL128_ONESHOT_MAX": str(LL128_ONESHOT_MAX),
              "NBX_LL128_MAX_GRID": str(LL128_MAX_GRID)},
    "simple": {"NCCL_PROTO": "Simple", "NBX_SIMPLE_MAX_GRID": str(SIMPLE_GRID)},
    "ring": {"NCCL_PROTO": "Simple", "NCCL_ALGO": "Ring", "NBX_SIMPLE_MAX_GRID": str(SIMPLE_GRID)},
}
COMMS = tuple(COMM_ENV)
PATHS = ("ll", "ll128", "ll128x2", "simple", "simple_elts", "ring")
PATH_COMM = {"ll": "ll", "ll128": "ll128", "ll128x2": "ll128", "simple": "simple", "simple_elts": "simple",
             "ring": "ring"}
PATH_BYTES = {"ll": LL_BYTES, "ll128": LL128_BYTES, "ll128x2": LL128X2_BYTES, "simple": SIMPLE_BYTES,
              "ring": SIMPLE_BYTES}
PATH_KINDS = {p: ("ar", "red") if p == "ll128x2" else ("ar", "rs", "red") for p in PATHS}


def itemsize(oracle, dtype):
    return np.dtype(oracle.NP_STORAGE[dtype]).itemsize


def nbytes_of(oracle, path, dtype):
    """Bytes per rank input (the figure the seed is drawn from)."""
    return ELTS_COUNT * itemsize(oracle, dtype) if path == "simple_elts" else PATH_BYTES[path]


def count_of(oracle, path, dtype):
    return max(1, nbytes_of(oracle, path, dtype) // itemsize(oracle, dtype))


def shift_of(oracle, path, dtype):
    """Bytes the send and recv pointers lie past a 16-byte boundary."""
    return itemsize(oracle, dtype) if path == "simple_elts" else 0


def path_cases(path):
    """[(kind, dtype, op)] of one path, in run order; a Reduce's root is root_of(index, n)."""
    return [(kind, dt, op) for kind in PATH_KINDS[path] for dt in ALL_TYPES for op in OPS[kind]]


def root_of(i, n):
    """The root of the Reduce at index i of a path's cases, rotated as
    tests/test_multiprocess_gpu.py rotates its LL cases': (3 i + 1) mod n, which
    visits every rank at 2 and 5 ranks and stays at rank 1 at 3 ranks."""
    return _ll_root(i, n)


def family_of(path, kind, n):
    """The kernel a case is meant to take."""
    if path == "ll128x2":
        return FAM_LL128X2 if n > 2 else FAM_LL128   # two ranks: one hop is the whole exchange
    return {"ll": FAM_LL, "ll128": FAM_LL128, "simple": FAM_SIMPLE, "simple_elts": FAM_SIMPLE, "ring": FAM_RING}[path]


PROTO_OF_FAMILY = {FAM_LL: P_LL, FAM_LL128: P_LL128, FAM_LL128X2: P_LL128X2, FAM_SIMPLE: P_SIMPLE,
                   FAM_RING: P_SIMPLE}


def host_unroll(path):
    """The record's unroll field: 1 for the LL family, 0 for Simple (picked on the device)."""
    return 0 if PATH_COMM[path] in ("simple", "ring") else 1


def fold_unroll(path, n):
    """The simpleFoldU instance a Simple case runs (nbx_simple.h simpleFold): the
    direct schedule folds all n sources of a block in one call — 16 packs per
    lane for <= 2 sources, 8 for <= 4, 4 above; every ring hop folds the local
    input with the one received slice, two sources, so 16 at any n."""
    assert PATH_COMM[path] in ("simple", "ring")
    return 16 if path == "ring" or n <= 2 else 8 if n <= 4 else 4


def seed_of(dtype, nbytes):
    return 1_000_003 * dtype + nbytes


@functools.lru_cache(maxsize=None)
def _sources(oracle, dtype, nbytes, total, n_srcs):
    xs = mi.edge_inputs(oracle, dtype, n_srcs, total, seed_of(dtype, nbytes))
    for x in xs:
        x.setflags(write=False)
    return xs


def total_of(oracle, path, kind, dtype, n):
    c = count_of(oracle, path, dtype)
    return c * n if kind == "rs" else c


def rank_inputs(oracle, path, kind, dtype, n, n_srcs=None):
    """Sources 0 .. n_srcs-1 (default n) of mi.edge_inputs(oracle, dtype, 8,
    total, seed): each source is drawn from its own generators, so a shorter
    call gives the same arrays (asserted by the CPU test) and rank r's input
    is the same at any n — but for a ReduceScatter, whose total is n x count."""
    return _sources(oracle, dtype, nbytes_of(oracle, path, dtype), total_of(oracle, path, kind, dtype, n),
                    n if n_srcs is None else n_srcs)


def rank_input(oracle, path, kind, dtype, n, r):
    return rank_inputs(oracle, path, kind, dtype, n, r + 1)[r]


def expected(oracle, path, kind, dtype, op, n, root):
    """{rank: expected output} of one case: the oracle in the schedule's own
    operand order — direct (LL, LL128, Simple): left fold b+1, ..., b of every
    block; ring: ring_chain along the same order."""
    xs = rank_inputs(oracle, path, kind, dtype, n)
    count = count_of(oracle, path, dtype)
    devop, arg = oracle.host_to_dev_redop(op, dtype, n)

    def fold(parts):
        if path == "ring":
            return ring_chain(oracle, parts, dtype, devop, arg, n)
        return oracle.reduce_multi(parts, dtype, devop, arg, n_pre_op_srcs=n, post_op=devop == 4, threads=4)[0]

    if kind == "rs":
        return {b: fold([xs[(b + 1 + k) % n][b * count:(b + 1) * count] for k in range(n)]) for b in range(n)}
    if kind == "red":
        return {root: fold([xs[(root + 1 + k) % n] for k in range(n)])}
    full = np.empty(count, dtype=xs[0].dtype)
    for b, (lo, hi) in enumerate(_blocks(count, xs[0].itemsize, n)):
        if hi > lo:
            full[lo:hi] = fold([xs[(b + 1 + k) % n][lo:hi] for k in range(n)])
    return {r: full for r in range(n)}


def fold_spans(kind, count, eb, n, ring, grid=SIMPLE_GRID, slice_bytes=64 << 10):
    """[(block, round, workgroup, bytes)] of every non-empty slice a Simple call
    folds (rank b folds block b on the direct schedule; every rank folds a slice
    of every block along the ring), from mp_diag.simple_geometry."""
    g = mp_diag.simple_geometry(kind, count, eb, n, grid, slice_bytes, ring=ring)
    if kind == "rs":
        blocks = [(b * count, (b + 1) * count) for b in range(n)]
    elif kind == "red" and ring:
        blocks = [(0, count)]
    else:
        blocks = [mp_diag.block_range(count, eb, n, b) for b in range(n)]
    out = []
    for b, (lo, hi) in enumerate(blocks):
        for k in range(g.n_rounds):
            for w in range(g.grid):
                s0 = (k * g.grid + w) * g.slice_elts
                cnt = min(g.slice_elts, hi - lo - s0)
                if cnt > 0:
                    out.append((b, k, w, cnt * eb))
    return out
