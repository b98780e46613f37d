"""Case table of the wide (fp32-accumulating) collective tests, shared by the
GPU tests (tests/widecoll/test_multiprocess_gpu.py, test_clique_transport_gpu.py) and
their CPU companion (tests/test_wide_collectives_cpu.py).

An operator of nbxRedOpCreateWide sums the ranks' inputs in fp32 in the direct
schedule's operand order and narrows once. Each direct-schedule kernel has its
own wide fold (kLLColl's 8-byte packs, l128FoldLine for kLL128Coll and
kLL128AllReduce2, simpleFoldU's pack and element paths), one compiled instance
per type; every (type, op) goes through each of them here.

Paths, communicators, environments and sizes are tests/edges/cases.py's own
(chosen there to leave ragged packs, lines and iterations):

  path         communicator  bytes per rank input     kernel meant (launch family)
  ll           ll            20,011                   kLLColl (8)
  ll128        ll128         12,011                   kLL128Coll (9)
  ll128x2      ll128         50,021 (ar, red only)    kLL128AllReduce2 (10); one-shot (9) at 2 ranks
  simple       simple        300,011                  kSimpleColl, pack path (11)
  simple_elts  simple        5,003 elements one element past a 16-byte
                             boundary                 kSimpleColl, element path (11)
  ring_direct  ring          300,011                  kSimpleColl (11), NOT kSimpleRing (12): the ring
                                                      moves partials of the element type, so a wide
                                                      call on an NCCL_ALGO=Ring communicator runs the
                                                      direct schedule, with the direct shapes (a
                                                      Reduce in n blocks, not one)

Types 6 (f16), 9 (bf16), 10 (e4m3), 11 (e5m2); ops wide Sum and wide Avg; n in
(2, 3, 5). Every record carries flags bit 1 (the fp32-accumulating
instantiation) and bit 0 clear.

At n = 2 wide and per-step Sum are the same bits: one add, one rounding (the
per-step add is computed in fp32 and rounded once as well). Only the launch
record distinguishes them there; the outputs are still checked. Wide Avg
differs from per-step Avg at any n (the per-step form rounds each product).

Inputs: tests/matrix/inputs.py's edge-rich inputs (denormals, +-0, inf, NaN,
random bits) for one half of the cases, tests/wide's many_inputs (uniform
[-1, 1)) for the other: input_kind alternates with the parity of kind index +
type index + op index, so every (type, op) meets both over a path's kinds.

Expected values as tests/wide/test_reduce_gpu.py builds them: every source
widened with the oracle's decoders, the oracle's fp32 left fold (Sum; for Avg
PreMulSum with oracle.host_to_dev_redop(4, F32, n)'s scalar on all n sources),
narrowed once with the oracle's encoder; per block, in the direct order
b+1, ..., b (a Reduce: root+1, ..., root).

Slice arithmetic of the wide Simple fold. The wide simpleFoldU runs 8 / 4 / 4
packs per lane at <= 2 / <= 4 / more sources (per-step: 16 / 8 / 4), so one
iteration is 8 x 256 x 16 B = 32,768 B at n = 2 and 4 x 256 x 16 B = 16,384 B
at n = 3 and n = 5. With the grid of 2 and the 64 KiB staging slice, for
SIMPLE_BYTES = 300,011 one-byte elements (edges/cases.py has the cut):

  n = 2 (U = 8): block 150,016 B, slice 65,536 B, 2 rounds. Round 0: both
    workgroups fold 65,536 B = 4,096 packs = two full iterations of 2,048.
    Round 1: workgroup 0 folds 18,944 B = 1,184 packs, one ragged iteration.
    So workgroup 0 runs full iterations and a ragged one (in successive
    rounds), workgroup 1 full ones only.
  n = 3 (U = 4): block 100,016 B, slice 50,016 B, one round. Workgroup 0 folds
    3,126 packs = 3 full iterations of 1,024 + a ragged one of 54; workgroup 1
    3,125 packs = 3 x 1,024 + 53.
  n = 5 (U = 4): block 60,016 B, slice 30,016 B. Workgroup 0: 1,876 packs =
    1,024 + 852; workgroup 1: 1,875 = 1,024 + 851.

So at every n some workgroup runs a full iteration and a ragged one
(tests/test_wide_collectives_cpu.py asserts it from fold_spans), and the rank
folding the last block a tail below one pack.
"""
import functools

import numpy as np

from tests.edges import cases as ec
from tests.test_multiprocess_gpu import _blocks
from tests.wide.test_reduce_gpu import expected as wide_fold
from tests.wide.test_reduce_gpu import many_inputs
from tests.matrix import inputs as mi

F16, F32, BF16, E4M3, E5M2 = 6, 7, 9, 10, 11
TYPES = (F16, BF16, E4M3, E5M2)
NS = ec.NS
SUM, AVG = 0, 4                       # ncclRedOp_t bases of the wide operator
OPS = (SUM, AVG)
DEV_SUM, DEV_PREMULSUM = 0, 3

FAM_WIDE_PACKS, FAM_WIDE_ELTS = 6, 7   # the wide core's records (a clique's fold path)
FLAG_CHECKED, FLAG_WIDE = 1, 2         # launch-record flags bits 0 and 1

COMMS = ec.COMMS
COMM_ENV, ENV_KEYS, PROCESS_ENV = ec.COMM_ENV, ec.ENV_KEYS, ec.PROCESS_ENV
PATHS = ("ll", "ll128", "ll128x2", "simple", "simple_elts", "ring_direct")
PATH_COMM = {**{p: ec.PATH_COMM[p] for p in PATHS if p != "ring_direct"}, "ring_direct": "ring"}
PATH_KINDS = {p: ec.PATH_KINDS["ring" if p == "ring_direct" else p] for p in PATHS}
_EDGE_PATH = {p: ("simple" if p == "ring_direct" else p) for p in PATHS}   # same size as the direct Simple path

MAX_SRCS = 8   # inputs are drawn for 8 sources, rank r takes source r: the same array at any n


def wide_unroll(n):
    """Packs per lane of the wide simpleFoldU at n sources (nbx_simple.h simpleFold)."""
    return 8 if n <= 2 else 4


def itemsize(oracle, dtype):
    return ec.itemsize(oracle, dtype)


def count_of(oracle, path, dtype):
    return ec.count_of(oracle, _EDGE_PATH[path], dtype)


def nbytes_of(oracle, path, dtype):
    return ec.nbytes_of(oracle, _EDGE_PATH[path], dtype)


def shift_of(oracle, path, dtype):
    return ec.shift_of(oracle, _EDGE_PATH[path], dtype)


def path_cases(path):
    """[(kind, dtype, op)] of one path, in run order; a Reduce's root is root_of(index, n)."""
    return [(kind, dt, op) for kind in PATH_KINDS[path] for dt in TYPES for op in OPS]


def root_of(i, n):
    return ec.root_of(i, n)


def family_of(path, kind, n):
    """The kernel a case is meant to take: ring_direct is the direct Simple kernel."""
    return ec.FAM_SIMPLE if path == "ring_direct" else ec.family_of(path, kind, n)


def host_unroll(path):
    return 0 if PATH_COMM[path] in ("simple", "ring") else 1


def input_kind(path, kind, dtype, op):
    k = PATH_KINDS[path].index(kind) + TYPES.index(dtype) + OPS.index(op)
    return "edge" if k % 2 == 0 else "uniform"


def total_of(oracle, path, kind, dtype, n):
    c = count_of(oracle, path, dtype)
    return c * n if kind == "rs" else c


@functools.lru_cache(maxsize=None)
def _sources(oracle, which, dtype, nbytes, total):
    seed = ec.seed_of(dtype, nbytes)
    if which == "edge":
        xs = mi.edge_inputs(oracle, dtype, MAX_SRCS, total, seed)
    else:
        xs = [np.ascontiguousarray(x) for x in many_inputs(oracle, dtype, MAX_SRCS, total, seed)]
    for x in xs:
        x.setflags(write=False)
    return xs


def rank_inputs(oracle, path, kind, dtype, op, n):
    """The n ranks' inputs of one case (sources 0 .. n-1 of 8 drawn)."""
    xs = _sources(oracle, input_kind(path, kind, dtype, op), dtype, nbytes_of(oracle, path, dtype),
                  total_of(oracle, path, kind, dtype, n))
    return xs[:n]


def wide_fold_of(oracle, parts, dtype, op, n):
    """nbxReduceMultiWide's arithmetic over `parts` in order: wide Sum the Sum
    device op, wide Avg PreMulSum by the fp32 scalar of an fp32 ncclAvg on every source."""
    if op == SUM:
        return wide_fold(oracle, parts, dtype, False, DEV_SUM, 0, 0)
    devop, arg = oracle.host_to_dev_redop(AVG, F32, n)
    assert devop == DEV_PREMULSUM
    return wide_fold(oracle, parts, dtype, False, devop, arg, n)


def per_step_fold_of(oracle, parts, dtype, op, n):
    """The per-step operator over the same parts (what the library computes without the handle)."""
    devop, arg = oracle.host_to_dev_redop(op, dtype, n)
    return oracle.reduce_multi(parts, dtype, devop, arg, n_pre_op_srcs=n, post_op=devop == 4, threads=4)[0]


def blocks_of(kind, count, eb, n):
    """[(first rank of the fold order's base, lo, hi)] in the rank inputs' element indices."""
    if kind == "rs":
        return [(b, b * count, (b + 1) * count) for b in range(n)]
    return [(b, lo, hi) for b, (lo, hi) in enumerate(_blocks(count, eb, n))]


def expected_with(fold, oracle, xs, kind, dtype, op, n, root, count):
    """{rank: expected output}: `fold` over every block in the direct order."""
    if kind == "red":
        return {root: fold(oracle, [xs[(root + 1 + k) % n] for k in range(n)], dtype, op, n)}
    eb = xs[0].itemsize
    if kind == "rs":
        return {b: fold(oracle, [xs[(b + 1 + k) % n][lo:hi] for k in range(n)], dtype, op, n)
                for b, lo, hi in blocks_of(kind, count, eb, n)}
    full = np.empty(count, dtype=xs[0].dtype)
    for b, lo, hi in blocks_of(kind, count, eb, n):
        if hi > lo:
            full[lo:hi] = fold(oracle, [xs[(b + 1 + k) % n][lo:hi] for k in range(n)], dtype, op, n)
    return {r: full for r in range(n)}


def expected(oracle, path, kind, dtype, op, n, root):
    xs = rank_inputs(oracle, path, kind, dtype, op, n)
    return expected_with(wide_fold_of, oracle, xs, kind, dtype, op, n, root, count_of(oracle, path, dtype))


fold_spans = ec.fold_spans
