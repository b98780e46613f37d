"""The flow-control call table (tests/flow/cases.py) without a GPU: the model
(tests/simple_model.py) runs every configuration of the GPU tests in round
robin order and in one seeded random order — outputs exact against the
oracle, no deadlock — and the claims the table's docstring makes are asserted
from the model's counters instead of trusted. The state checker checks itself:
the pairwise invariants hold on the model's end state, and a lagging receive
counter or a flag word left behind is named with its pair, region and
workgroup. The hook's argument checks need no device."""
import ctypes
import os

import numpy as np
import pytest

from tests import simple_model as sm
from tests.conftest import load_package
from tests.flow import cases


def _assert_outputs(oracle, n, cfg, calls, run, label):
    for ci, call in enumerate(calls):
        exp = cases.expected(oracle, call, [cases.rank_input(call, n, r) for r in range(n)], n, cfg.ring)
        for r in range(n):
            got = run.outputs[ci][r]
            if r not in exp:
                assert got is None and call.kind == "red"
                continue
            assert got is not None and np.array_equal(got, exp[r]), (label, ci, call, r)


def _states(run, n):
    return [(run.comm.counters[r].copy(), run.comm.flags[r].copy()) for r in range(n)]


@pytest.mark.parametrize("cfg", [cases.CONFIGS[0], cases.CONFIGS[5], cases.CONFIGS[8], cases.CONFIGS[11]],
                         ids=lambda c: c.name)
@pytest.mark.parametrize("n", cases.NS)
def test_grouped_launch_on_the_model(oracle, n, cfg):
    """The four AllReduces of the GPU test's grouped launch as ONE launch on the
    model, going on from the state a sequence left: every segment exact against
    the oracle, the invariants hold, and every cell advanced by the launch's
    rounds: segment 0 is 3 (S + 1) whole slices, the others one 16-byte slice
    more, 12 (S + 1) + 3 virtual slices in 4 (S + 1) + 1 rounds of 3 — more
    than the S slots, and every segment boundary but the first inside a round."""
    before = cases.run_model(n, cfg, cases.sequence(n, cfg)[:6])
    grouped = cases.group_calls(n, cfg)
    run, geom = cases.run_model_group(before, n, cfg, grouped)
    full = 3 * (cfg.slots + 1)
    assert geom.slices == [full, full + 1, full + 1, full + 1] and (geom.grid, geom.slice_bytes) == (cases.GRID, cases.SLICE)
    assert geom.n_rounds == 4 * (cfg.slots + 1) + 1 > cfg.slots
    assert [o % cases.GRID for o in geom.slice_off] == [0, 0, 1, 2]
    for s, call in enumerate(grouped):
        exp = cases.expected(oracle, call, [cases.rank_input(call, n, r) for r in range(n)], n, cfg.ring)
        for r in range(n):
            assert np.array_equal(run.outputs[s][r], exp[r]), (s, r)
    assert cases.check_pairs(_states(run, n), n, cases.GRID) == []
    hops = (n - 1) if cfg.ring else 1
    for r in range(n):
        d = run.comm.counters[r].astype(np.int64) - before.comm.counters[r].astype(np.int64)
        to = (r + 1) % n
        for g in range(cases.GRID):
            assert d[cases.idx(n, cases.GRID, sm.RS_SENT, to, g)] == geom.n_rounds * hops
            assert d[cases.idx(n, cases.GRID, sm.AG_SENT, to, g)] == geom.n_rounds * hops
    assert all(np.array_equal(a, b) for a, b in zip(before.comm.counters, before.starts[-1]))   # a copy went on


def _uses(run, n, grid, ci, kind):
    """{(a, b, g): uses} of counter `kind` (a's count toward b) during call ci."""
    out = {}
    for a in range(n):
        d = run.starts[ci + 1][a].astype(np.int64) - run.starts[ci][a].astype(np.int64)
        for b in range(n):
            for g in range(grid):
                if d[cases.idx(n, grid, kind, b, g)]:
                    out[(a, b, g)] = int(d[cases.idx(n, grid, kind, b, g)])
    return out


@pytest.mark.parametrize("cfg", cases.CONFIGS, ids=lambda c: c.name)
@pytest.mark.parametrize("n", cases.NS)
def test_flow_table_on_the_model(oracle, n, cfg):
    calls = cases.sequence(n, cfg)
    assert len(calls) == 48 and len(cases.CONFIGS) == 12
    rr = cases.run_model(n, cfg, calls)                              # a deadlock fails inside run_call
    rnd = cases.run_model(n, cfg, calls, order="random", seed=1000 * n + cfg.slots)
    _assert_outputs(oracle, n, cfg, calls, rr, "rr")
    _assert_outputs(oracle, n, cfg, calls, rnd, "random")
    # the end state does not depend on the interleaving: it is a prediction of the device's
    for r in range(n):
        assert np.array_equal(rr.comm.counters[r], rnd.comm.counters[r])
        assert np.array_equal(rr.comm.flags[r], rnd.comm.flags[r])
    assert cases.check_pairs(_states(rr, n), n, cases.GRID) == []
    assert cases.check_model(_states(rnd, n), rr.comm, n, cases.GRID) == []

    s, grid = cfg.slots, cases.GRID
    end = rr.starts[-1]
    # the cells the schedule uses: every pair on the direct schedule, a -> a + 1 along the ring,
    # on every workgroup, in both regions — and every slot index 0 .. S-1 of each was written
    pairs = {(a, b) for a in range(n) for b in range(n) if a != b and (not cfg.ring or b == (a + 1) % n)}
    for kind in (sm.RS_SENT, sm.AG_SENT):
        used = {(a, b, g): int(end[a][cases.idx(n, grid, kind, b, g)])
                for a in range(n) for b in range(n) for g in range(grid) if end[a][cases.idx(n, grid, kind, b, g)]}
        assert set(used) == {(a, b, g) for a, b in pairs for g in range(grid)}, (kind, sorted(used))
        assert min(used.values()) >= s   # uses are consecutive, slot = use mod S
    # some call wraps a cell's slot ring twice
    most = max(max(_uses(rr, n, grid, ci, sm.RS_SENT).values()) for ci in range(len(calls)))
    assert most >= 2 * s + 1
    if cfg.ring and n == 5 and s == 8:
        assert most == 89 * (n - 1) or most == 89   # the chain Reduce: 89 rounds in one call
    # some call's last round leaves a workgroup of its grid without a byte, and its counters advance all the same
    idle = 0
    for ci, call in enumerate(calls):
        block, total, g_, sl, rounds = sm.call_shape(rr.comm, call.kind, call.count, call.eb, cfg.ring)
        blocks = 1 if cfg.ring and call.kind == "red" else n
        for w in range(g_):
            if all(sm._slice(block, total, sl // call.eb, g_, b, rounds - 1, w)[1] == 0 for b in range(blocks)):
                idle += 1
                per = _uses(rr, n, grid, ci, sm.RS_SENT)
                assert all(per[(a, b, w)] == per[(a, b, 0)] for a, b in pairs if (a, b, 0) in per), (ci, call, w)
    assert idle >= 2
    # calls begin on more than one slot phase: in every cell on the direct schedule; along the
    # ring on every workgroup, though not in every cell — a ring call moves n - 1 hops per round
    # through a cell and only a Reduce (one hop, none into the rank after the root) shifts the
    # phase, so at 3 ranks, where the table's roots are always 1, pair 1->2 stays in phase at S = 2
    per_call = [_uses(rr, n, grid, ci, sm.RS_SENT) for ci in range(len(calls))]
    for w in range(grid):
        varied = 0
        for a, b in pairs:
            phases = {int(rr.starts[ci][a][cases.idx(n, grid, sm.RS_SENT, b, w)]) % s
                      for ci in range(len(calls)) if (a, b, w) in per_call[ci]}
            assert len(phases) > 1 or cfg.ring, (a, b, w, phases)
            varied += len(phases) > 1
        assert varied >= 1, (w, "every cell of this workgroup always begins on one slot")


def test_flow_table_sizes():
    """The block sizes the docstring lists, as rounds of the communicator's cut."""
    for s in cases.SLOTS:
        for n in cases.NS:
            comm = sm.Comm(n, cases.GRID, cases.SLICE, s)
            calls = cases.pass_calls(n, s, 0)
            rounds = [sm.call_shape(comm, c.kind, c.count, c.eb, False)[4] for c in calls]
            grids = [sm.call_shape(comm, c.kind, c.count, c.eb, False)[2] for c in calls]
            rs = [i for i, c in enumerate(calls) if c.kind == "rs"]
            assert [rounds[i] for i in rs] == [1, 1, 2, s, s + 1, s + 2, 2 * s + 2, 1]
            assert [grids[i] for i in rs] == [1, 2, 3, 3, 3, 3, 3, 1]
            # the AllReduce and Reduce blocks round up to whole packs, never to another round
            for i in range(0, 21, 3):
                assert rounds[i] == rounds[i + 1] == rounds[i + 2], (s, n, i, rounds)
            assert [c.root for c in calls if c.kind == "red"][:7] == [(3 * i + 1) % n for i in range(2, 21, 3)]
            assert calls[23].root == n - 1 and [c.count for c in calls[21:]] == [1, 1, 2]
            # both passes: the same bytes but for the rounding of a block to whole elements
            for a, b in zip(calls, cases.pass_calls(n, s, 1)):
                assert a.kind == b.kind and a.root == b.root and b.eb == 8
                if a.kind == "rs" and a.count > 1:
                    assert 0 <= b.count * 8 - a.count * 4 < 8


@pytest.mark.parametrize("cfg", cases.FIRST_USE_CONFIGS, ids=lambda c: c.name)
def test_first_use_sequence_on_the_model(oracle, cfg):
    n, grid, calls = cases.FIRST_USE_N, 32, list(cases.FIRST_USE)
    rr = cases.run_model(n, cfg, calls, grid, 64 << 10)
    rnd = cases.run_model(n, cfg, calls, grid, 64 << 10, order="random", seed=8)
    _assert_outputs(oracle, n, cfg, calls, rr, "rr")
    _assert_outputs(oracle, n, cfg, calls, rnd, "random")
    assert cases.check_pairs(_states(rr, n), n, grid) == []
    assert cases.check_model(_states(rnd, n), rr.comm, n, grid) == []
    # the round-5 record's shape: 125,004-element blocks on all 32 workgroups in one round
    for call in calls:
        block, _total, g_, sl, rounds = sm.call_shape(rr.comm, call.kind, call.count, call.eb, cfg.ring)
        if not (cfg.ring and call.kind == "red"):
            assert (block, g_, sl // 4, rounds) == (125_004, 32, 3908, 1)
    for kind_i, kind in enumerate(cases.KINDS):
        three = [kind_i * 3 + k for k in range(3)]
        for counter in (sm.RS_SENT, sm.RS_RECV, sm.AG_SENT, sm.AG_RECV):
            cells = set.intersection(*[set(_uses(rr, n, grid, ci, counter)) for ci in three]) if kind != "rs" or \
                counter < 2 else set()
            if kind == "ar":   # every cell of both regions, all 32 workgroups
                assert len(cells) == (n if cfg.ring else n * (n - 1)) * grid
            for a, b, g in cells:
                start = [int(rr.starts[ci][a][cases.idx(n, grid, counter, b, g)]) for ci in three]
                slots = [x % cfg.slots for x in start]
                if cfg.ring and kind == "red":   # the chain cuts the whole message: two rounds, so every call on slot 0
                    assert start[1] - start[0] == start[2] - start[1] == 2 and slots == [0, 0, 0]
                    continue
                assert slots[0] != slots[1] and slots[2] == slots[0], (kind, counter, a, b, g, start)
                if kind == "ar" and not cfg.ring:   # first use of slot 0, first use of slot 1, first reuse
                    assert start == [0, 1, 2]
                if kind == "ar" and cfg.ring:
                    assert start == [0, 7, 14]


def test_state_checker_names_a_lagging_counter_and_a_flag_left_behind():
    n, cfg = 3, cases.CONFIGS[2]   # direct, 3 slots
    run = cases.run_model(n, cfg, cases.pass_calls(n, cfg.slots, 0))
    good = _states(run, n)
    assert cases.check_pairs(good, n, cases.GRID) == [] and cases.check_model(good, run.comm, n, cases.GRID) == []
    # rank 2's receive counter for what rank 0 sends, AG region, workgroup 1, one behind
    bad = _states(run, n)
    bad[2][0][cases.idx(n, cases.GRID, sm.AG_RECV, 0, 1)] -= 1
    lines = cases.check_pairs(bad, n, cases.GRID)
    assert len(lines) == 1 and lines[0].startswith("pair 0->2 region AG workgroup 1:")
    assert "receive counter lags the sender" in lines[0]
    lines = cases.check_model(bad, run.comm, n, cases.GRID)
    assert len(lines) == 1 and "rank 2 counters[AgRecv][0] workgroup 1 (pair 0->2 region AG)" in lines[0]
    # rank 1's ready flag from rank 2, RS region, workgroup 2, one behind
    bad = _states(run, n)
    bad[1][1][cases.idx(n, cases.GRID, sm.RS_READY, 2, 2)] -= 1
    lines = cases.check_pairs(bad, n, cases.GRID)
    assert len(lines) == 1 and lines[0].startswith("pair 2->1 region RS workgroup 2:")
    assert "RS_READY flag behind the sender" in lines[0] and "counter" not in lines[0].split("(")[-1]
    lines = cases.check_model(bad, run.comm, n, cases.GRID)
    assert len(lines) == 1 and "rank 1 flags[RS_READY][2] workgroup 2 (pair 2->1 region RS)" in lines[0]
    # a credit flag: rank 0's credit from rank 1 (for what 0 sends to 1)
    bad = _states(run, n)
    bad[0][1][cases.idx(n, cases.GRID, sm.AG_CREDIT, 1, 0)] -= 1
    lines = cases.check_pairs(bad, n, cases.GRID)
    assert len(lines) == 1 and lines[0].startswith("pair 0->1 region AG workgroup 0:")
    assert "AG_CREDIT flag behind the receiver" in lines[0]


def test_slot_report_names_slot_and_use():
    n, cfg = 3, cases.CONFIGS[2]
    calls = cases.pass_calls(n, cfg.slots, 0)
    run = cases.run_model(n, cfg, calls)
    ci = 18   # the AllReduce that wraps twice
    start = int(run.starts[ci][1][cases.idx(n, cases.GRID, sm.AG_RECV, 2, 1)])
    text = cases.slot_report(calls[ci], cfg, n, 1, (2, 4, 1), run.starts[ci])
    assert text == f"copied from AG slot {(start + 4) % 3} (use {start + 4}) from rank 2"
    assert cases.slot_report(calls[ci], cfg, n, 1, (1, 0, 0), run.starts[ci]).startswith("folded from RS slot")


def test_simple_state_hook_refuses_bad_arguments():
    nbx = load_package()
    if not os.path.exists(nbx.library_path()):
        pytest.fail("libnbxccl.so is not built")
    lib = nbx.load_library()
    assert nbx.simple_state(None, 64) is None                 # a NULL handle
    words = (ctypes.c_uint64 * 8)()
    pre = ctypes.c_int(7)
    assert lib.nbxDebugSimpleState(None, words, words, 8, ctypes.byref(pre)) == -1 and pre.value == 7
    junk = ctypes.create_string_buffer(4096)                  # no communicator: the magic is missing
    assert lib.nbxDebugSimpleState(ctypes.cast(junk, ctypes.c_void_p), words, words, 8, ctypes.byref(pre)) == -1
