"""Call table of the Simple transport's flow-control tests, shared by the GPU
tests (tests/flow/test_multiprocess_gpu.py) and their CPU companion
(tests/test_simple_flow_cpu.py).

What is under test is the hand-off of kSimpleColl and kSimpleRing
(csrc/nbx_simple.h), not their arithmetic: staging slots reused modulo the
communicator's slot count S, ready flags and credits, the per-cell counters a
workgroup carries from one call to the next, and the next-round prefetch of the
direct schedule. The knobs that shape it are NBX_SIMPLE_SLOTS (2..8) and
NBX_SIMPLE_PREFETCH (0 / 1); the matrix is

  direct schedule   S in {2, 3, 4, 8} x prefetch in {0, 1}
  NCCL_ALGO=Ring    S in {2, 3, 4, 8}          (the ring has no prefetch path)

twelve communicators, each with NCCL_PROTO=Simple, NBX_SIMPLE_MAX_GRID=3 and
NBX_SIMPLE_SLICE_BYTES=4096 (the smallest slice the library accepts), so one
round moves R = 3 x 4096 = 12,288 B of a block and S rounds fill the slot ring
of a (region, source, workgroup) cell once.

One pass is 24 calls, back to back on one stream. Seven block sizes (bytes),
each as AllReduce, ReduceScatter and Reduce (index i = 3 x size + kind):

  3,000            one workgroup, one round
  6,000            two workgroups, one ragged round
  2 R              two full rounds
  S R              exactly fills the slot ring: the call after it starts where
                   this one started (modulo S)
  S R + 4,100      S + 1 rounds; in the last one workgroup 0 moves a full
                   slice, workgroup 1 four bytes (eight in the uint64 pass,
                   sixteen for the pack-rounded AllReduce / Reduce block) and
                   workgroup 2 nothing — and its counters advance all the same
  (S + 1) R + 100  the first wrap: the last rounds reuse slots of this call
  (2S + 1) R + 8,200   wraps twice

then a 1-element AllReduce, a 1-element ReduceScatter and a 2-element Reduce to
root n - 1, which leave most blocks empty. A block of B bytes is ceil(B / eb)
elements. ReduceScatter: recvcount = that block. AllReduce and Reduce: count =
n blocks minus (i mod 4) elements, so the last block is ragged (the library
rounds their blocks up to whole 16-byte packs; where B is a multiple of 16 the
block stays B). The ring's Reduce is a chain over the whole message, so the
same count runs n times the rounds there: up to 89 in one call at 5 ranks and
S = 8. A Reduce's root is (3 i + 1) mod n.

The table runs twice on each communicator: pass 0 is uint32 Sum, pass 1 uint64
Sum at the same byte sizes — other element counts, the same rounds. Because
the sizes are not multiples of S R, successive calls begin on different slots
(start counter mod S): on the direct schedule in every (pair, workgroup) cell;
along the ring on every workgroup but not in every cell — a ring AllReduce or
ReduceScatter moves n - 1 hops per round through a cell, only a Reduce (one
hop per round, none into the rank after its root) shifts a cell's phase, and
the roots (3 i + 1) mod n are always 1 at 3 ranks, so there pair 1->2 of
workgroups 1 and 2 begins every call on slot 0 at S = 2.
tests/test_simple_flow_cpu.py asserts that, and every other claim made here,
from the model instead of trusting this text. Inputs are
full-range random integers: any stale, missing or misplaced slice changes the
sum.

The reference for the outputs is the oracle folded in the schedule's own order
(direct: left fold b+1, ..., b per block; ring: ring_chain). The reference for
the protocol state is tests/simple_model.py run over the same sequence with the
communicator's own grid, slice, slots and prefetch: counters and flag words at
rest do not depend on how the workgroups interleaved, so the model's end state
is what every rank's nbxDebugSimpleState must return, word for word.

FIRST_USE is the 8-rank sequence on default settings (grid 32 where 8 ranks
share 256 CUs, 64 KiB slices, 2 slots): three int32 ncclMax AllReduces of
1,000,003 elements, three ReduceScatters of 125,004 and three Reduces of
1,000,003 to root 5 — 125,004-element blocks on all 32 workgroups in one
round. On the direct schedule the first AllReduce is therefore the first use
of slot 0 of every (region, pair, workgroup) cell, the second the first use of
slot 1 and the third the first reuse of slot 0, in both regions. The calls
that follow go on from there: every call advances each cell it uses by one, so
the three calls of a kind always begin on alternating slots (the
ReduceScatters on 1, 0, 1 of the RS cells, the Reduces on 0, 1, 0). Along the
ring an AllReduce or ReduceScatter moves 7 hops through each cell per region,
so its calls alternate too (uses 0, 7, 14), but the first call alone already
fills both slots; the ring's Reduce is a chain over the whole message, two
rounds of 64 KiB slices, so each of its calls begins on slot 0.
"""
import copy
from collections import namedtuple

import numpy as np

from tests import mp_diag
from tests import simple_model as sm
from tests.test_multiprocess_gpu import _blocks, _ll_root, ring_chain

NS = (2, 3, 5)
SLOTS = (2, 3, 4, 8)
GRID, SLICE = 3, 4096
R = GRID * SLICE
SUM, MAX = 0, 2                      # ncclRedOp_t
INT32, UINT32, UINT64 = 2, 3, 5      # ncclDataType_t
PASSES = ((UINT32, 4), (UINT64, 8))
FAM_SIMPLE, FAM_RING = 11, 12        # include/nbx_debug.h nbxDebugLaunchLog
KINDS = ("ar", "rs", "red")
REGIONS = ("RS", "AG")
COUNTER_NAMES = ("RsSent", "RsRecv", "AgSent", "AgRecv")
FLAG_NAMES = ("RS_READY", "RS_CREDIT", "AG_READY", "AG_CREDIT")

Config = namedtuple("Config", "name slots prefetch ring")
Call = namedtuple("Call", "kind count root dtype eb op seed")

CONFIGS = tuple([Config(f"direct-s{s}-p{p}", s, p, False) for s in SLOTS for p in (0, 1)] +
                [Config(f"ring-s{s}", s, 1, True) for s in SLOTS])

# every key is unset, then the communicator's own are set, while it is created
ENV_KEYS = ("NCCL_PROTO", "NCCL_ALGO", "NBX_SIMPLE_MAX_GRID", "NBX_SIMPLE_SLICE_BYTES", "NBX_SIMPLE_SLOTS",
            "NBX_SIMPLE_PREFETCH")


def comm_env(cfg):
    env = {"NCCL_PROTO": "Simple", "NBX_SIMPLE_MAX_GRID": str(GRID), "NBX_SIMPLE_SLICE_BYTES": str(SLICE),
           "NBX_SIMPLE_SLOTS": str(cfg.slots)}
    if cfg.ring:
        env["NCCL_ALGO"] = "Ring"
    else:
        env["NBX_SIMPLE_PREFETCH"] = str(cfg.prefetch)
    return env


def block_bytes(slots):
    return (3000, 6000, 2 * R, slots * R, slots * R + 4100, (slots + 1) * R + 100, (2 * slots + 1) * R + 8200)


def root_of(i, n):
    return _ll_root(i, n)   # (3 i + 1) mod n


def pass_calls(n, slots, pass_index):
    """The 24 calls of one pass on a communicator of `slots` slots."""
    dtype, eb = PASSES[pass_index]
    out = []
    for bb in block_bytes(slots):
        be = -(-bb // eb)
        for kind in KINDS:
            i = len(out)
            count = be if kind == "rs" else n * be - i % 4
            out.append(Call(kind, count, root_of(i, n) if kind == "red" else 0, dtype, eb, SUM, (pass_index, i)))
    out.append(Call("ar", 1, 0, dtype, eb, SUM, (pass_index, 21)))
    out.append(Call("rs", 1, 0, dtype, eb, SUM, (pass_index, 22)))
    out.append(Call("red", 2, n - 1, dtype, eb, SUM, (pass_index, 23)))
    return out


def sequence(n, cfg):
    """Both passes: what one communicator runs before its state is read."""
    return pass_calls(n, cfg.slots, 0) + pass_calls(n, cfg.slots, 1)


def group_calls(n, cfg):
    """The four AllReduces of the grouped launch: blocks of (S + 1) R bytes plus the call's index."""
    be = (cfg.slots + 1) * R // 4
    return [Call("ar", n * be + k, 0, UINT32, 4, SUM, (2, k)) for k in range(4)]


FIRST_USE_N, FIRST_USE_ROOT = 8, 5
FIRST_USE = tuple([Call("ar", 1_000_003, 0, INT32, 4, MAX, (3, k)) for k in range(3)] +
                  [Call("rs", 125_004, 0, INT32, 4, MAX, (3, 3 + k)) for k in range(3)] +
                  [Call("red", 1_000_003, FIRST_USE_ROOT, INT32, 4, MAX, (3, 6 + k)) for k in range(3)])
FIRST_USE_CONFIGS = (Config("direct-default", 2, 1, False), Config("ring-default", 2, 1, True))
FIRST_USE_ENV_KEYS = ENV_KEYS
FIRST_USE_ENV = {"direct-default": {"NCCL_PROTO": "Simple"}, "ring-default": {"NCCL_PROTO": "Simple", "NCCL_ALGO": "Ring"}}

_NP = {INT32: np.int32, UINT32: np.uint32, UINT64: np.uint64}


def np_type(call):
    return _NP[call.dtype]


def total_of(call, n):
    return call.count * n if call.kind == "rs" else call.count


def rank_input(call, n, r):
    """Rank r's send buffer: full-range random integers, the same wherever it is asked for."""
    t = np.dtype(np_type(call))
    info = np.iinfo(t)
    rng = np.random.default_rng([20261020, n, call.seed[0], call.seed[1], r])
    return rng.integers(info.min, info.max, total_of(call, n), dtype=t, endpoint=True)


def expected(oracle, call, xs, n, ring):
    """{rank: expected output}: the oracle in the schedule's own operand order
    (tests/edges/cases.expected's pattern)."""
    devop, arg = oracle.host_to_dev_redop(call.op, call.dtype, n)

    def fold(parts):
        if ring:
            return ring_chain(oracle, parts, call.dtype, devop, arg, n)
        return oracle.reduce_multi(parts, call.dtype, devop, arg, n_pre_op_srcs=n, post_op=devop == 4, threads=4)[0]

    c = call.count
    if call.kind == "rs":
        return {b: fold([xs[(b + 1 + k) % n][b * c:(b + 1) * c] for k in range(n)]) for b in range(n)}
    if call.kind == "red":   # both schedules fold a Reduce in the order root+1, ..., root
        return {call.root: fold([xs[(call.root + 1 + k) % n] for k in range(n)])}
    full = np.empty(c, dtype=xs[0].dtype)
    for b, (lo, hi) in enumerate(_blocks(c, call.eb, n)):
        if hi > lo:
            full[lo:hi] = fold([xs[(b + 1 + k) % n][lo:hi] for k in range(n)])
    return {r: full for r in range(n)}


def geometry(call, n, grid, slice_bytes, ring):
    return mp_diag.simple_geometry(call.kind, call.count, call.eb, n, grid, slice_bytes, ring=ring)


def family_of(cfg):
    return FAM_RING if cfg.ring else FAM_SIMPLE


# ---------------------------------------------------------------------------
# the model over a sequence

def _model_fold(call):
    t = np_type(call)
    red = np.add if call.op == SUM else np.maximum

    def fold(srcs, pre_mask=None, post=True):
        acc = srcs[0].view(t)
        for s in srcs[1:]:
            acc = red(acc, s.view(t))
        return np.ascontiguousarray(acc).view(np.uint8)
    return fold


ModelRun = namedtuple("ModelRun", "comm starts outputs")


def run_model(n, cfg, calls, grid=GRID, slice_bytes=SLICE, order="rr", seed=0):
    """tests/simple_model.py over `calls` on one communicator. starts[c][rank]:
    the counter words at the start of call c (a last entry holds the end
    state); outputs[c][rank]: the recv buffer as the element type, or None."""
    comm = sm.Comm(n, grid, slice_bytes, cfg.slots)
    starts, outputs = [], []
    for ci, call in enumerate(calls):
        starts.append([c.copy() for c in comm.counters])
        t = np_type(call)
        sends = [rank_input(call, n, r).view(np.uint8) for r in range(n)]
        recvs = [np.full(call.count * call.eb, 0xA5, np.uint8) if call.kind != "red" or r == call.root else None
                 for r in range(n)]
        sm.run_call(comm, call.kind, sends, recvs, call.count, call.eb, _model_fold(call), root=call.root,
                    ring=cfg.ring, prefetch=bool(cfg.prefetch), order=order, seed=seed + ci)
        outputs.append([None if x is None else x.view(t) for x in recvs])
    starts.append([c.copy() for c in comm.counters])
    return ModelRun(comm, starts, outputs)


def run_model_group(run, n, cfg, grouped, grid=GRID, slice_bytes=SLICE):
    """The grouped launch on the model (tests/simple_model.py run_group, cut by
    mp_diag.simple_group_geometry), going on from a copy of `run`'s end state:
    what every rank's nbxDebugSimpleState must return after the group."""
    comm = copy.deepcopy(run.comm)
    first = grouped[0]
    assert all((c.kind, c.dtype, c.op) == (first.kind, first.dtype, first.op) for c in grouped)
    geom = mp_diag.simple_group_geometry([(c.kind, c.count) for c in grouped], first.eb, n, grid, slice_bytes,
                                         ring=cfg.ring)
    sends = [[rank_input(c, n, r).view(np.uint8) for r in range(n)] for c in grouped]
    recvs = [[np.full(c.count * c.eb, 0xA5, np.uint8) for _r in range(n)] for c in grouped]
    sm.run_group(comm, first.kind, geom, sends, recvs, first.eb, _model_fold(first), ring=cfg.ring,
                 prefetch=bool(cfg.prefetch))
    return ModelRun(comm, [run.starts[-1]], [[x.view(np_type(first)) for x in seg] for seg in recvs]), geom


def idx(n, grid, kind, who, g):
    return (kind * n + who) * grid + g


# ---------------------------------------------------------------------------
# the state checker

def check_pairs(states, n, grid):
    """Pairwise invariants of the protocol state at rest. states[rank] =
    (counters, flags) as nbxDebugSimpleState returns them. For every ordered
    pair a -> b, region and workgroup: what a sent is what b received, what b's
    ready flag from a says, and what a's credit flag from b says. Returns one
    line per broken cell, naming the pair, the region and the workgroup."""
    out = []
    for a in range(n):
        for b in range(n):
            if a == b:
                continue
            for region in range(2):
                sent_k, recv_k, ready_k, credit_k = 2 * region, 2 * region + 1, 2 * region, 2 * region + 1
                for g in range(grid):
                    sent = int(states[a][0][idx(n, grid, sent_k, b, g)])
                    recv = int(states[b][0][idx(n, grid, recv_k, a, g)])
                    ready = int(states[b][1][idx(n, grid, ready_k, a, g)])
                    credit = int(states[a][1][idx(n, grid, credit_k, b, g)])
                    if sent == recv == ready == credit:
                        continue
                    what = []
                    if sent > recv:
                        what.append("receive counter lags the sender")
                    if sent < recv:
                        what.append("receive counter ahead of the sender")
                    if ready != sent:
                        what.append(f"{FLAG_NAMES[ready_k]} flag {'behind' if ready < sent else 'ahead of'} the sender")
                    if credit != recv:
                        what.append(f"{FLAG_NAMES[credit_k]} flag {'behind' if credit < recv else 'ahead of'} "
                                    "the receiver")
                    out.append(f"pair {a}->{b} region {REGIONS[region]} workgroup {g}: "
                               f"{a}.{COUNTER_NAMES[sent_k]}[{b}]={sent} {b}.{COUNTER_NAMES[recv_k]}[{a}]={recv} "
                               f"{b}.flags[{FLAG_NAMES[ready_k]}][{a}]={ready} "
                               f"{a}.flags[{FLAG_NAMES[credit_k]}][{b}]={credit} ({'; '.join(what)})")
    return out


def check_model(states, model_comm, n, grid):
    """Every rank's counters and flags against the model's, word for word."""
    out = []
    for r in range(n):
        for which, names, want in ((0, COUNTER_NAMES, model_comm.counters[r]), (1, FLAG_NAMES, model_comm.flags[r])):
            got = np.asarray(states[r][which], dtype=np.uint64)
            if got.shape != want.shape:
                out.append(f"rank {r}: {len(got)} {'flag' if which else 'counter'} words, the model has {len(want)}")
                continue
            for w in np.flatnonzero(got != want):
                kind, rest = divmod(int(w), n * grid)
                who, g = divmod(rest, grid)
                # a sent counter and a credit flag belong to the data r sends to `who`; a receive
                # counter and a ready flag to the data `who` sends to r
                outgoing = (kind % 2 == 0) if which == 0 else (kind % 2 == 1)
                pair = f"{r}->{who}" if outgoing else f"{who}->{r}"
                out.append(f"rank {r} {'flags' if which else 'counters'}[{names[kind]}][{who}] workgroup {g} "
                           f"(pair {pair} region {REGIONS[kind // 2]}): device {int(got[w])}, model {int(want[w])}")
    return out


def slot_report(call, cfg, n, rank, cell, start):
    """Which staging slot, at which use, fed (block, round, workgroup) = cell of
    rank `rank`'s output in this call; start[r] are the model's counter words at
    the start of the call (grid = len / 4n)."""
    b, k, g = cell
    grid = len(start[rank]) // (4 * n)
    s = cfg.slots

    def cnt(kind, who):
        return int(start[rank][idx(n, grid, kind, who, g)])

    def say(region, use, src):
        return f"{region} slot {use % s} (use {use}) from rank {src}"

    if not cfg.ring:
        if b == rank:   # folded here from every peer's RS slot
            return "folded from " + ", ".join(say("RS", cnt(sm.RS_RECV, j) + k, j) for j in range(n) if j != rank)
        return "copied from " + say("AG", cnt(sm.AG_RECV, b) + k, b)
    left = (rank + n - 1) % n
    if call.kind == "red":
        return "last hop " + say("RS", cnt(sm.RS_RECV, left) + k, left)
    if b == rank or call.kind == "rs":
        u0 = cnt(sm.RS_RECV, left) + k * (n - 1)
        return f"folded along the ring; last hop {say('RS', u0 + n - 2, left)} (this round's uses {u0}..{u0 + n - 2})"
    st = (rank - 1 - b) % n
    return "copied from " + say("AG", cnt(sm.AG_RECV, left) + k * (n - 1) + st, left)
