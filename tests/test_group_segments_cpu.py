"""The grouped-launch tests' tables (tests/groups/cases.py) and the Python
mirror of the grouped launch (mp_diag.group_runs, ll_group_units,
simple_group_geometry; simple_model.run_group), without a GPU. Everything
tests/groups/cases.py and DESIGN §3 claim for the tables is asserted here from
the mirror, not from prose:

  * the mirror's protocol choice is the library's own (nbxDebugChooseProto) on
    every call of both tables;
  * the 64-call group of every (communicator, kind, n) is cut into exactly
    eight launches of eight segments, at the type / op changes;
  * the Simple tables reach, at every element width and n: a segment boundary
    inside a round and one on a round boundary, more rounds than slots with a
    slot reused by another segment than the one that filled it, a segment
    shorter than a slice and one an exact multiple, the one-element segment
    leaving blocks empty at some n;
  * the LL / LL128 tables: a packOff off a workgroup pass, a partial last unit,
    the total inside one slot; ReduceScatter blocks on and off a 16-byte
    boundary; pack-aligned and misaligned pointers in one launch;
  * the oracle's expected results pooled over each launch hold at most NAN_CAP
    NaN;
  * the grouped model computes what a plain sum computes and leaves the
    counters of `rounds` rounds; with a deliberately wrong sliceOff it yields
    different outputs and different counters (model only — nothing of the kind
    runs on a GPU);
  * every cut rule's group is cut as the issue's table says, for the reason it
    is there for, alike on every rank."""
import ctypes

import numpy as np
import pytest

from tests import mp_diag
from tests import simple_model as sm
from tests.conftest import gpu_order_key
from tests.flow import cases as flow
from tests.groups import cases
from tests.matrix import inputs as mi

WIDTHS = (1, 2, 4, 8)
PROTO_CODE = {"LL": 0, "LL128": 1, "Simple": 2, "LL128x2": 3}   # nbxDebugChooseProto's answers
DEF = cases.DEFAULT_SETTINGS


@pytest.fixture(scope="module", autouse=True)
def _release_inputs():
    yield
    cases._sources.cache_clear()


@pytest.fixture(scope="module")
def lib(nbx):
    lib = nbx.load_library()
    lib.nbxDebugProtoMask.argtypes = [ctypes.c_char_p]
    lib.nbxDebugProtoMask.restype = ctypes.c_int
    lib.nbxDebugChooseProto.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                        ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    lib.nbxDebugChooseProto.restype = ctypes.c_int
    return lib


def _lib_proto(lib, mask, kind, count, eb, n, oneshot):
    lo, hi = mp_diag.block_range(count, eb, n, 0)
    return lib.nbxDebugChooseProto(mask, int(kind != "rs"), count * eb, (hi - lo) * eb, n, DEF["llMax"], DEF["l128Max"],
                                   oneshot)


# ---------------------------------------------------------------------------
# the mirror's protocol choice

def test_table_covers_every_width_and_functor(oracle):
    assert sorted(cases.itemsize(oracle, dt) for dt, _ in cases.TYPE_OPS) == [1, 1, 2, 2, 4, 4, 8, 8]
    devops = {(cases.itemsize(oracle, dt), oracle.host_to_dev_redop(op, dt, 3)[0]) for dt, op in cases.TYPE_OPS}
    # Sum, MinMax, PreMulSum (float Avg), Prod, SumPostDiv (integer Avg)
    assert {d for _, d in devops} == {0, 1, 2, 3, 4} and len(devops) == 8
    assert cases.E4M3 in dict(cases.TYPE_OPS) and cases.INT64 in dict(cases.TYPE_OPS)
    for path in cases.PATHS:
        assert len(cases.SEG_BYTES[path]) == cases.N_SEGS and set(cases.COMM_ENV[path]) <= set(cases.ENV_KEYS) | \
            set(cases.PROCESS_ENV)


@pytest.mark.parametrize("n", cases.NS)
def test_protocol_choice_is_the_librarys(lib, oracle, n):
    for path in cases.PATHS:
        env = cases.COMM_ENV[path]
        mask = lib.nbxDebugProtoMask(env["NCCL_PROTO"].encode())
        assert mask == cases.PROTO_MASK[path]
        oneshot = int(env.get("NBX_LL128_ONESHOT_MAX", 256 << 10))
        want = {"ll": "LL", "ll128": "LL128", "simple": "Simple", "ring": "Simple"}[path]
        for kind in cases.KINDS:
            for c in cases.group_calls(oracle, path, kind, n, 0):
                got = mp_diag.proto_of(kind, c.count, c.eb, n, DEF, mask, oneshot)
                assert got == want and PROTO_CODE[got] == _lib_proto(lib, mask, kind, c.count, c.eb, n, oneshot), \
                    (path, kind, c)
    if n in cases.CUT_NS:
        for name, calls in cases.cut_groups(n).items():
            for c in calls:
                if c.count:
                    got = mp_diag.proto_of(c.kind, c.count, 4, n, DEF)
                    assert PROTO_CODE[got] == _lib_proto(lib, 7, c.kind, c.count, 4, n, 256 << 10), (name, c)


# ---------------------------------------------------------------------------
# section 2's table

@pytest.mark.parametrize("n", cases.NS)
def test_the_64_calls_cut_into_eight_launches_of_eight(oracle, n):
    for path in cases.PATHS:
        oneshot = int(cases.COMM_ENV[path].get("NBX_LL128_ONESHOT_MAX", 256 << 10))
        for kind in cases.KINDS:
            for rank in range(n):
                calls = cases.group_calls(oracle, path, kind, n, rank)
                assert len(calls) == 64
                plan = mp_diag.group_runs(calls, n, DEF, cases.PROTO_MASK[path], path == "ring", oneshot)
                assert plan.runs == [(8 * k, 8 * k + 8) for k in range(8)] and plan.reasons == ["op"] * 7
                assert plan.records == [(cases.FAMILY[path], n, 0 if cases.is_simple(path) else 1, 8 << 8)] * 8
            # with batching off every call runs alone
            off = mp_diag.group_runs(calls, n, dict(DEF, groupBatch=0), cases.PROTO_MASK[path], path == "ring", oneshot)
            assert len(off.runs) == 64 and set(off.reasons) == {"batch_off"} and all(r[3] == 0 for r in off.records)


def test_layout_places_every_segment(oracle):
    for path in cases.PATHS:
        for kind in cases.KINDS:
            for n in cases.NS:
                for rank in (0, n - 1):
                    slots, sb, rb = cases.layout(oracle, path, kind, n, rank)
                    spans = []
                    for sl in slots:
                        assert sl.send_off % 16 == cases.send_shift(sl.seg, sl.eb) and sl.send_off % sl.eb == 0
                        spans.append((0, sl.send_off - cases.GUARD, sl.send_off + sl.send_elts * sl.eb + cases.GUARD))
                        if sl.in_place:
                            assert sl.seg == cases.IN_PLACE
                            assert sl.recv_off == sl.send_off + (rank * sl.count * sl.eb if kind == "rs" else 0)
                        else:
                            assert sl.recv_off % 16 == cases.recv_shift(sl.seg, sl.eb) and sl.recv_off % sl.eb == 0
                            spans.append((1, sl.recv_off - cases.GUARD, sl.recv_off + sl.count * sl.eb + cases.GUARD))
                    for arena, size in ((0, sb), (1, rb)):
                        own = sorted((lo, hi) for a, lo, hi in spans if a == arena)
                        assert own[0][0] >= 0 and own[-1][1] <= size
                        assert all(a[1] <= b[0] for a, b in zip(own, own[1:]))   # guards included, nothing overlaps


@pytest.mark.parametrize("eb", WIDTHS)
def test_pointer_alignments_in_one_launch(eb):
    send = [cases.send_shift(s, eb) for s in range(cases.N_SEGS)]
    recv = [cases.recv_shift(s, eb) for s in range(cases.N_SEGS) if s != cases.IN_PLACE]
    assert 0 in send and any(send) and any(recv)                                  # pack-aligned and not, in one launch
    assert (0 in recv) == (eb > 1)               # one-byte elements: recv shifts 3 .. 9, never on a boundary
    if eb < 8:
        assert any(a and b and a != b for a, b in zip(send, recv))                # two different misalignments
    else:
        assert all(a != b for a, b in zip(send, recv))           # 8-byte elements: on a boundary or 8 past it
    if eb < 8:
        assert any(x % 8 for x in send) and any(x % 8 for x in recv)              # a byte-shifted 8-byte LL load
    assert cases.send_shift(cases.IN_PLACE, eb) != 0      # the in-place segment is off a 16-byte boundary too


@pytest.mark.parametrize("n", cases.NS)
@pytest.mark.parametrize("eb", WIDTHS)
@pytest.mark.parametrize("path", ["simple", "ring"])
def test_simple_table_reaches_every_shape(path, eb, n):
    for kind in cases.KINDS:
        g = cases.launch_geometry(path, kind, eb, n)
        # the flow tests' settings: a round moves 3 x 4,096 B of a block; the sum of the blocks decides
        assert (g.grid, g.slice_bytes, g.n_rounds) == (3, 4096, 6)
        assert g.slices == [1, 1, 1, 1, 2, 3, 5, 2] and g.slice_off == [0, 1, 2, 3, 4, 6, 9, 14]
        inner = [q for q in range(1, 8) if g.slice_off[q] % g.grid]
        on_round = [q for q in range(1, 8) if g.slice_off[q] % g.grid == 0]
        assert inner and on_round
        # two workgroups of one round serve different segments
        assert any(g.segment_of(k * g.grid) != g.segment_of(k * g.grid + g.grid - 1) for k in range(g.n_rounds))
        # more rounds than slots: a slot is reused inside the launch, by another segment than filled it
        assert g.n_rounds > cases.SIMPLE_SLOTS
        assert any(g.segment_of(k * g.grid + w) != g.segment_of((k - cases.SIMPLE_SLOTS) * g.grid + w)
                   for k in range(cases.SIMPLE_SLOTS, g.n_rounds) for w in range(g.grid))
        seg_bytes = [min(b, t) * eb for b, t in zip(g.block_elts, g.totals)]
        assert any(0 < sb < g.slice_bytes for sb in seg_bytes) and any(sb % g.slice_bytes == 0 for sb in seg_bytes)
        assert seg_bytes[5] == 3 * 4096                     # one full round
        assert any(sb % g.slice_bytes and sb > g.slice_bytes for sb in seg_bytes)   # a ragged last slice
        # every element of every segment is moved exactly once, by the workgroup locate() names
        for s in range(8):
            seen = np.zeros(g.totals[s], dtype=np.int32)
            for b in range(n):
                for k in range(g.n_rounds):
                    for w in range(g.grid):
                        sg, off, cnt = g.span(b, k, w)
                        if sg == s and cnt:
                            seen[off:off + cnt] += 1
                            loc = g.locate(s, np.array([off, off + cnt - 1]))
                            assert [list(r[:4]) for r in loc] == [[s, b, k, w]] * 2 and loc[0][4] == 0
            assert (seen == 1).all(), (kind, s)
        if kind == "ar":
            # the last block of every AllReduce segment with s % 4 != 0 is ragged
            for s, (c, blk) in enumerate(zip(cases.seg_counts(path, kind, eb, n), g.block_elts)):
                assert c == n * (1 if cases.SEG_BYTES[path][s] is None else max(1, cases.SEG_BYTES[path][s] // eb)) - s % 4
                assert blk * eb % 16 == 0 or blk == c      # whole packs, unless the message ends inside block 0
    # at 2 ranks the one-element AllReduce (count n = 2) is block 0 alone: blocks 1 .. n-1 are empty
    g2 = cases.launch_geometry(path, "ar", eb, 2)
    assert g2.totals[0] == 2 and g2.block_elts[0] >= 2
    assert g2.span(0, 0, 0) == (0, 0, 2) and g2.span(1, 0, 0) == (0, 2, 0)


@pytest.mark.parametrize("n", cases.NS)
@pytest.mark.parametrize("eb", WIDTHS)
@pytest.mark.parametrize("path", ["ll", "ll128"])
def test_ll_tables_reach_every_shape(path, eb, n):
    unit, per_pass = cases.UNIT[path], cases.PASS_UNITS[path]
    cap = DEF["llMax"] // 8 if path == "ll" else mp_diag.l128_slot_lines(DEF["l128Max"])
    for kind in cases.KINDS:
        counts = cases.seg_counts(path, kind, eb, n)
        offs, total = cases.launch_units(path, kind, eb, n)
        assert offs == sorted(offs) and offs[0] == 0 and len(offs) == 8
        assert total <= cap                                         # no capacity cut in this table
        assert total > per_pass                                     # more than one workgroup pass
        assert any(o % per_pass for o in offs[1:])                  # one pass spans two segments
        units = [-(-c * eb // unit) for c in counts]
        assert per_pass in units                                    # a segment of exactly one pass
        partial = [c * eb % unit for c in counts]
        if eb < 8 or unit == 48:
            assert any(partial)                                     # a segment ends in a partial unit
        else:
            assert not any(partial)                                 # an 8-byte element is a whole LL pack: none can
        assert counts[0] == 1 and units[0] == 1                     # the one-element message


@pytest.mark.parametrize("eb", WIDTHS)
def test_reduce_scatter_blocks_on_and_off_a_pack_boundary(oracle, eb):
    dt = next(d for d, _ in cases.TYPE_OPS if cases.itemsize(oracle, d) == eb)
    for path in cases.PATHS:
        for n in cases.NS:
            slots, _, _ = cases.layout(oracle, path, "rs", n, 0)
            starts = {(sl.send_off + r * sl.count * eb) % 16 == 0 for sl in slots if sl.dtype == dt for r in range(n)}
            assert starts == {True, False}, (path, n)
            one = [sl for sl in slots if sl.dtype == dt and len({(sl.send_off + r * sl.count * eb) % 16 == 0
                                                                 for r in range(n)}) == 2]
            assert one, (path, n)   # within ONE segment some ranks' blocks are aligned, others are not


# ---------------------------------------------------------------------------
# expected results

@pytest.mark.parametrize("n", cases.NS)
def test_pooled_nan_share_per_launch(oracle, n):
    """A one-element segment alone may be all NaN, so the cap holds per launch:
    the expected results of a launch's eight segments, every rank's, pooled."""
    worst = {}
    for path in cases.PATHS:
        for kind in cases.KINDS:
            for pi, (dt, op) in enumerate(cases.TYPE_OPS):
                exps = [cases.expected(oracle, path, kind, pi, s, n) for s in range(cases.N_SEGS)]
                assert all(sorted(e) == list(range(n)) for e in exps)
                pooled = np.concatenate([e[r] for e in exps for r in range(n)])
                assert np.count_nonzero(pooled.view(np.uint8)) > pooled.size // 4
                if dt in mi.FLOAT_TYPES:
                    share = mi.nan_share(pooled, dt)
                    worst[dt] = max(worst.get(dt, 0.0), share)
                    assert share <= mi.NAN_CAP, (path, kind, dt, op, n, share)
    print(f"n = {n}: largest pooled NaN share per type", {oracle.TYPE_NAMES[d]: f"{s:.2%}" for d, s in worst.items()})


def test_inputs_are_per_type_path_and_segment(oracle):
    a = cases.rank_inputs(oracle, "simple", "ar", 4, 6, 3)
    assert len(a) == 3 and a[0].size == cases.seg_count("simple", "ar", 6, 4, 3)
    assert a[1].tobytes() == cases.rank_inputs(oracle, "simple", "ar", 4, 6, 3, 2)[1].tobytes()   # rank r is source r
    assert a[0][:100].tobytes() != cases.rank_inputs(oracle, "ring", "ar", 4, 6, 3)[0][:100].tobytes()
    assert a[0][:100].tobytes() != cases.rank_inputs(oracle, "simple", "ar", 4, 5, 3)[0][:100].tobytes()
    img = cases.send_image(oracle, "simple", "rs", 3, 1)
    slots, size, _ = cases.layout(oracle, "simple", "rs", 3, 1)
    assert img.size == size and (img[:cases.GUARD] == 0xA5).all()


# ---------------------------------------------------------------------------
# the grouped model

def _plain_sums(outputs_kind, n, path, kind, seed=0):
    """What run_model_groups' launches must compute: wrapping sums of the same random bytes."""
    for li, eb in enumerate([1, 1, 2, 2, 4, 4, 8, 8]):
        counts = cases.seg_counts(path, kind, eb, n)
        rng = np.random.default_rng([seed, li, eb, n])
        ut = mi.UINT_OF[eb]
        for s, c in enumerate(counts):
            sends = [rng.integers(0, 256, (c * n if kind == "rs" else c) * eb, dtype=np.uint8) for _r in range(n)]
            acc = sends[0].view(ut).copy()
            for x in sends[1:]:
                acc = acc + x.view(ut)
            for r in range(n):
                want = acc[r * c:(r + 1) * c] if kind == "rs" else acc
                yield li, s, r, np.array_equal(outputs_kind[li][s][r].view(ut), want)


@pytest.mark.parametrize("n", cases.NS)
@pytest.mark.parametrize("path", ["simple", "ring"])
def test_grouped_model_computes_the_sums_and_counts_the_rounds(path, n):
    with np.errstate(over="ignore"):
        comm, outputs = cases.run_model_groups(sm, n, path)
        for kind in cases.KINDS:
            wrong = [(li, s, r) for li, s, r, ok in _plain_sums(outputs[kind], n, path, kind) if not ok]
            assert not wrong, (kind, wrong[:8])
    states = [(comm.counters[r], comm.flags[r]) for r in range(n)]
    assert flow.check_pairs(states, n, cases.SIMPLE_GRID) == []
    # 16 launches of 6 rounds: the direct schedule advances a pair's RS cell once per round (the AG cell
    # too in an AllReduce), the ring n - 1 hops per round through the cell towards the right neighbour
    rounds = 6 * 8
    for r in range(n):
        for w in range(cases.SIMPLE_GRID):
            to = (r + 1) % n
            rs_sent = int(comm.counters[r][comm.flag_idx(sm.RS_SENT, to, w)])
            ag_sent = int(comm.counters[r][comm.flag_idx(sm.AG_SENT, to, w)])
            if path == "ring":
                assert (rs_sent, ag_sent) == (2 * rounds * (n - 1), rounds * (n - 1))
            else:
                assert (rs_sent, ag_sent) == (2 * rounds, rounds)


@pytest.mark.parametrize("n", cases.NS)
@pytest.mark.parametrize("path", ["simple", "ring"])
def test_a_wrong_slice_off_changes_outputs_and_counters(path, n):
    """The checks of test_group_segments would see a wrong sliceOff: the model
    run with segment q (and what follows it) starting one slice early — as a
    host that counted the segment before it one slice short would cut it, so
    the launch has 15 virtual slices and 5 rounds — yields different outputs
    and different counters, for every q. A lone segment starting one slice late
    hides its last slice behind its successor: other outputs, the same
    counters, which is why both are compared."""
    kinds = ("ar",)
    with np.errstate(over="ignore"):
        good, good_out = cases.run_model_groups(sm, n, path, kinds=kinds, widths=[4])
        for q in range(1, cases.N_SEGS):
            bad, bad_out = cases.run_model_groups(sm, n, path, kinds=kinds, widths=[4], mutate=lambda g: g.shifted(q, -1))
            assert any(not np.array_equal(a, b) for sa, sb in zip(good_out["ar"][0], bad_out["ar"][0])
                       for a, b in zip(sa, sb)), q
            assert any(not np.array_equal(good.counters[r], bad.counters[r]) for r in range(n)), q
            assert any(not np.array_equal(good.flags[r], bad.flags[r]) for r in range(n)), q

        def late(g, q=4):
            off = list(g.slice_off)
            off[q] += 1
            return mp_diag.SimpleGroupGeometry(g.kind, g.eb, g.n, g.block_elts, g.totals, g.slices, off, g.grid,
                                               g.slice_bytes, g.n_rounds)
        bad, bad_out = cases.run_model_groups(sm, n, path, kinds=kinds, widths=[4], mutate=late)
        assert not np.array_equal(good_out["ar"][0][4][0], bad_out["ar"][0][4][0])
        assert all(np.array_equal(good.counters[r], bad.counters[r]) for r in range(n))


def test_single_calls_are_unchanged_by_the_segment_lookup():
    """run_call goes through the same workgroup code with no segment table: a
    group of ONE segment and the plain call leave the same outputs and state."""
    n, eb, count = 3, 4, 3 * 5000 - 3
    rng = np.random.default_rng(5)
    sends = [rng.integers(0, 256, count * eb, dtype=np.uint8) for _ in range(n)]
    fold = cases.model_fold(np.uint32)
    with np.errstate(over="ignore"):
        for ring in (False, True):
            a, b = sm.Comm(n, 3, 4096, 2), sm.Comm(n, 3, 4096, 2)
            ra = [np.zeros(count * eb, np.uint8) for _ in range(n)]
            rb = [np.zeros(count * eb, np.uint8) for _ in range(n)]
            sm.run_call(a, "ar", sends, ra, count, eb, fold, ring=ring)
            geom = mp_diag.simple_group_geometry([("ar", count)], eb, n, 3, 4096, ring=ring)
            single = mp_diag.simple_geometry("ar", count, eb, n, 3, 4096, ring=ring)
            assert (geom.grid, geom.slice_elts, geom.n_rounds) == (single.grid, single.slice_elts, single.n_rounds)
            sm.run_group(b, "ar", geom, [sends], [rb], eb, fold, ring=ring)
            assert all(np.array_equal(x, y) for x, y in zip(ra, rb))
            assert all(np.array_equal(a.counters[r], b.counters[r]) and np.array_equal(a.flags[r], b.flags[r])
                       for r in range(n))


# ---------------------------------------------------------------------------
# section 3's table: the cut rules

def _plan(calls, n, rank, settings=DEF):
    return mp_diag.group_runs(cases.cut_group_calls(calls, n, rank), n, settings)


def test_every_cut_rule_cuts_where_the_table_says():
    groups = cases.cut_groups(3)
    assert set(cases.CUT_EXPECT_3) | {"ll128_capacity"} == set(groups)
    seen = set()
    for name, calls in groups.items():
        plan = _plan(calls, 3, 0)
        segs = [r[3] >> 8 for r in plan.records]
        if name in cases.CUT_EXPECT_3:
            assert segs == cases.CUT_EXPECT_3[name], (name, segs)
        if name in cases.CUT_REASON:
            assert cases.CUT_REASON[name] in plan.reasons, (name, plan.reasons)
        seen |= set(plan.reasons)
        assert all(fam in (8, 9, 10, 11) and nn == 3 for fam, nn, _, _ in plan.records)
    assert seen == set(mp_diag.CUT_REASONS) - {"batch_off"}
    off = _plan(groups[cases.BATCH_OFF_GROUP], 3, 0, dict(DEF, groupBatch=0))
    assert set(off.reasons) == {"batch_off"} and [r[3] for r in off.records] == [0] * 17
    # the rules by name
    assert _plan(groups["max_segs_40"], 3, 0).reasons == ["max_segs"] * 2
    assert _plan(groups["ll_capacity"], 3, 0).reasons == ["capacity"] * 2
    cap = _plan(groups["ll128_capacity"], 3, 0)
    assert cap.reasons == ["capacity"] and cap.protos == ["LL128"] * 2 and 1 < cap.records[0][3] >> 8 < 16
    assert _plan(groups["proto_change"], 3, 0).protos == ["LL", "LL128", "Simple", "LL"]
    assert _plan(groups["ll128_two_shot"], 3, 0).protos == ["LL128x2", "LL128x2", "LL128"]
    assert _plan(groups["ll128_two_shot"], 2, 0).protos == ["LL128"]    # two ranks: one hop is the whole exchange
    assert _plan(groups["zero_inside"], 3, 0).runs == [(0, 2), (2, 3), (3, 5)]
    assert _plan(groups["zero_first"], 3, 0).runs == [(0, 1), (1, 4)]
    assert _plan(groups["shared_send"], 3, 0).reasons == [] and _plan(groups["in_place_among"], 3, 0).reasons == []


@pytest.mark.parametrize("n", cases.CUT_NS)
def test_every_rank_cuts_alike(n):
    for name, calls in cases.cut_groups(n).items():
        plans = [_plan(calls, n, r) for r in range(n)]
        assert all(p.runs == plans[0].runs and p.records == plans[0].records for p in plans), name
    # the NULL recv of a Reduce's non-roots is the one place the ranks' own buffers differ
    calls = cases.cut_groups(n)["null_recv"]
    assert [c.recv is None for c in cases.cut_group_calls(calls, n, (1 % n + 1) % n)].count(True) == 1
    assert not any(c.recv is None for c in cases.cut_group_calls(calls, n, 1 % n))


@pytest.mark.parametrize("n", cases.CUT_NS)
def test_simulated_results(n):
    """simulate() folds a chain in call order: a -> b, then b -> c gives the sum of sums."""
    groups = cases.cut_groups(n)
    gi = list(groups).index("chain")
    calls = groups["chain"]
    lay, _ = cases.buffer_layout(calls, n)
    before = [cases.arena_image(gi, calls, n, r) for r in range(n)]
    after = cases.simulate(gi, calls, n)

    def buf(img, name):
        off, nelts, _ = lay[name]
        return img[off:off + 4 * nelts].view(np.int32)
    with np.errstate(over="ignore"):
        s = sum(buf(b, "a")[:100].astype(np.int64) for b in before).astype(np.int32)
    for r in range(n):
        assert np.array_equal(buf(after[r], "b")[:100], s)
        assert np.array_equal(buf(after[r], "c")[:100], (s.astype(np.int64) * n).astype(np.int32))
        assert np.array_equal(buf(after[r], "a"), buf(before[r], "a"))
    # a user PreMulSum weighs every rank's input with the rank's own scalar
    gi = list(groups).index("user_premul")
    calls = groups["user_premul"]
    lay, _ = cases.buffer_layout(calls, n)
    before = [cases.arena_image(gi, calls, n, r) for r in range(n)]
    after = cases.simulate(gi, calls, n)
    want = sum(buf(b, "s2")[:100].astype(np.int64) * cases.PREMUL_INTS[r] for r, b in enumerate(before))
    assert np.array_equal(buf(after[0], "r2")[:100], want.astype(np.int32))
    assert len(cases.PREMUL_INTS) >= max(cases.CUT_NS)


def test_mismatch_reports_name_the_cell(oracle):
    """What the GPU test says about a wrong output, on made-up wrong elements."""
    from tests.groups import test_multiprocess_gpu as gpu
    settings = {p: {"simpleGrid": cases.SIMPLE_GRID, "sliceBytes": cases.SIMPLE_SLICE} for p in ("simple", "ring")}
    slots, _, _ = cases.layout(oracle, "simple", "rs", 3, 1)
    sl = next(s for s in slots if s.eb == 4 and s.seg == 6)          # 20,000 B blocks: slices 9 .. 13 of every block
    text = gpu._where("simple", "rs", sl, 3, 1, np.array([0, 1024, sl.count - 1]), settings)
    # rank 1's output is block 1: slice 9 is round 3 workgroup 0, slice 10 workgroup 1, slice 13 round 4 workgroup 1
    assert text.startswith("3 (segment, block, round, workgroup) cells")
    assert "first at [6, 1, 3, 0, 0]" in text and "last at [6, 1, 4, 1, 903]" in text and "[6, 1, 3, 1]" in text
    lslots, _, _ = cases.layout(oracle, "ll", "ar", 3, 0)
    ll = next(s for s in lslots if s.eb == 2 and s.seg == 5)         # 2,051 B: 1,025 f16, 257 packs from pack 261
    text = gpu._where("ll", "ar", ll, 3, 0, np.array([4, 1024]), settings)
    assert text.startswith("segment 5 units 1..256 of its own, launch units 262..517 of 1156 (8-byte units")
    assert gpu._nearest_slot(slots, False, slots[9].recv_off) == "pair 1 segment 1 (0 B away)"
    assert gpu._nearest_slot(slots, True, slots[9].send_off - 3) == "pair 1 segment 1 (3 B away)"
    assert gpu._nearest_slot(slots, False, slots[9].recv_off + slots[9].count * slots[9].eb + 2) == \
        "pair 1 segment 1 (3 B away)"


def test_gpu_file_sorts_with_the_multiprocess_tests():
    assert gpu_order_key("tests/groups/test_multiprocess_gpu.py") == gpu_order_key("tests/test_multiprocess_gpu.py")
    assert gpu_order_key("tests/groups/test_multiprocess_gpu.py", "test_group_segments[3]") == \
        gpu_order_key("tests/test_multiprocess_gpu.py")
