"""The batched-reduce tests' case table without a GPU (tests/batch/cases.py,
tests/batch/test_reduce_gpu.py):

  * the table's windows are disjoint and inside the uploads, and every bucket
    has the head, packs, tiles and tail its row claims under BatchPacker::add's
    arithmetic, at every element size;
  * NaN — compared only as NaN on the GPU — stays under the 10 % cap over the
    expected outputs of every call, and the sums' expected outputs hold
    denormals in the large buckets;
  * the table capacities the scheduler shapes rely on are nbx_kargs.h's;
  * the scheduler shapes are what their docstrings say: launches of 101 + 19
    and 384 + 16 buckets, the tile counts of their cycles, destinations
    disjoint and on their sources' misalignment."""
import os
import re

import numpy as np
import pytest

from tests.batch import cases as bc
from tests.conftest import PKG_DIR
from tests.matrix import inputs as mi

ALL_TYPES = list(range(12))
EBS = (1, 2, 4, 8)


# ---------------------------------------------------------------------------
# table geometry

@pytest.mark.parametrize("eb", EBS)
def test_table_windows_are_disjoint_and_inside_the_uploads(eb):
    rows = bc.table(eb)
    assert tuple(r[0] for r in rows) == bc.NAMES
    end = 0
    for name, start, count in rows:
        assert start >= end and count >= 0, name
        if count:
            assert start > end or start == 0, f"no gap in front of '{name}'"
        end = start + count
        assert end <= mi.max_count(eb), name
    assert max(s + c for _, s, c in rows if c) <= 1150 * (16 // eb)
    assert rows[-1][2] == 0 and all(c > 0 for _, _, c in rows[:-1])


@pytest.mark.parametrize("eb", EBS)
def test_table_buckets_reach_what_they_claim(eb):
    epp, m, head = bc.geometry(eb)
    assert (epp, m) == {1: (16, 3), 2: (8, 3), 4: (4, 3), 8: (2, 1)}[eb] and head == epp - m
    claims = bc.claims(eb)
    for name, start, count in bc.table(eb)[:-1]:
        assert (start * eb) % 16 == (m * eb if name in ("head only", "clipped head", "tile + pack") else 0), name
        assert bc.packer_geometry(start, count, eb) == claims[name], name
    # what the rows are there for
    g = {name: bc.packer_geometry(s, c, eb) for name, s, c in bc.table(eb)[:-1]}
    assert g["one element"][1:] == (0, 1, 1) and g["below a pack"][1] == 0 and g["below a pack"][3] > 0
    assert g["head only"] == (head, 0, 1, 0)
    unclamped = (16 - (bc.table(eb)[3][1] * eb) % 16) // eb
    assert g["clipped head"][0] == bc.table(eb)[3][2] <= unclamped and (eb >= 4 or g["clipped head"][0] < unclamped)
    assert g["exact tile"] == (0, bc.TILE_PACKS, 1, 0)
    assert g["tile + pack"][1] == bc.TILE_PACKS + 1 and g["tile + pack"][0] > 0 and (eb == 8) == (g["tile + pack"][3] == 1)
    assert g["ragged"][1] == 2 * bc.TILE_PACKS + 77 and g["ragged"][2] == 3 and g["ragged"][3] == epp - 1


def test_table_buckets_of_a_call():
    b = bc.table_buckets(4, [1, 2, 3, 1, 2, 3, 8])
    assert [len(x.rows) for x in b] == [1, 2, 3, 1, 2, 3, 8, 1]
    assert all(x.dstart == x.start for x in b) and b[-1].count == 0


# ---------------------------------------------------------------------------
# NaN cap and denormals

@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_nan_cap_per_call_and_denormals(oracle, dtype):
    srcs = mi.matrix_inputs(oracle, dtype)
    eb = srcs[0].itemsize
    worst = worst_large = 0.0
    for nsrc in range(1, mi.MAX_SRCS + 1):
        for label, devop, arg, npre, post, _ in mi.op_cases(oracle, dtype, nsrc):
            exp = oracle.reduce_multi(srcs[:nsrc], dtype, devop, arg, npre, post, threads=8)[0]
            share = bc.nan_share_of_call(exp, eb, dtype)
            worst = max(worst, share)
            assert share <= mi.NAN_CAP, (label, nsrc, share)
            large = {n: exp[s:s + c] for n, s, c in bc.table(eb) if n in bc.LARGE}
            worst_large = max([worst_large] + [mi.nan_share(a, dtype) for a in large.values()])
            if dtype in mi.FLOAT_TYPES and devop == mi.SUM and nsrc in (2, 8):
                n = sum(mi.denormal_count(a, dtype) for a in large.values())
                assert n >= 1, f"no denormal in the large buckets' sums of {nsrc} sources"
    print(f"{oracle.TYPE_NAMES[dtype]}: largest NaN share of a call {worst:.2%}, of a large bucket {worst_large:.2%}")
    assert worst_large <= mi.NAN_CAP


# ---------------------------------------------------------------------------
# capacities (nbx_kargs.h)

def header_constants():
    text = open(os.path.join(PKG_DIR, "csrc", "nbx_kargs.h")).read()
    found = dict(re.findall(r"constexpr int (k\w+) = ([^;]+);", text))
    return found


def test_table_capacities_are_the_headers():
    h = header_constants()
    assert int(h["kBatchTilePacks"]) == bc.TILE_PACKS == 256
    assert int(h["kBatchHeaderBytes"]) == 40 and h["kBatchWords"].replace(" ", "") == "(4096-kBatchHeaderBytes)/8"
    assert bc.KERNARG_WORDS == (4096 - 40) // 8 == 507
    assert int(h["kBatchKernargMaxBuckets"]) == bc.KERNARG_MAX_BUCKETS == 16
    assert int(h["kListMaxRecs"]) == bc.LIST_MAX_RECS == 384
    assert int(h["kBatchRecWords"]) == bc.LIST_REC_WORDS_MAX == 20
    assert int(h["kMaxKSrcs"]) == bc.MAX_SRCS == 8 and int(h["kMaxKDsts"]) == bc.MAX_DSTS == 8

    def per_table(nsrc, ndst):
        return bc.kernarg_launches([bc.Bucket("", 0, 1, tuple(range(ndst)), 0)] * 1000, nsrc)[0]
    assert per_table(2, 1) == 507 // 5 == 101
    assert per_table(8, 1) == 507 // 11 == 46
    assert per_table(8, 8) == 507 // 18 == 28
    assert 3 + bc.MAX_SRCS + bc.MAX_DSTS <= bc.LIST_REC_WORDS_MAX   # the widest work-list record


# ---------------------------------------------------------------------------
# scheduler shapes

def assert_layout(buckets, eb):
    """Windows inside the uploads; destinations on their sources' misalignment,
    disjoint per row, at least a pack of untouched bytes between neighbours."""
    epp = 16 // eb
    spans = {}
    for b in buckets:
        assert b.count > 0 and b.start + b.count <= mi.max_count(eb), b.name
        assert (b.dstart - b.start) % epp == 0, b.name
        for r in b.rows:
            spans.setdefault(r, []).append((b.dstart, b.dstart + b.count))
    for r, s in spans.items():
        s.sort()
        assert all(lo2 - hi1 >= epp for (_, hi1), (lo2, _) in zip(s, s[1:])), f"row {r}"


@pytest.mark.parametrize("eb", (2, 4))
def test_scheduler_shapes(eb):
    epp, m, head = bc.geometry(eb)
    walk = bc.kernarg_walk(eb)
    assert_layout(walk, eb)
    assert bc.kernarg_launches(walk, 2) == [101, 19]
    assert bc.tiles_of(walk, eb) == [1, 1, 1, 13] * 30
    assert sum(bc.tiles_of(walk[:101], eb)) == 401 > 1.5 * 256          # at the MI355X's 256 CUs
    assert [(b.start * eb) % 16 != 0 for b in walk] == [i % 3 == 2 for i in range(120)]
    assert all(b.count % (bc.TILE_PACKS * epp) for b in walk)   # ragged: no bucket ends on a tile

    lst = bc.list_walk(eb)
    assert_layout(lst, eb)
    assert bc.list_launches(len(lst)) == [384, 16]
    tiles = bc.tiles_of(lst, eb)
    assert tiles == [1, 1, 2, 8] * 100
    assert sum(tiles[:384]) == 1152 > 4 * 256 and sum(tiles[:64]) == 192 <= 4 * 255
    # a misaligned bucket's packs behind the head fill its tiles exactly: were the head lost on the
    # way to the kernel, the packs would start `head` elements early and need one more tile
    for b in lst:
        h, packs, t, tail = bc.packer_geometry(b.start, b.count, eb)
        if h:
            assert packs == t * bc.TILE_PACKS and tail == epp - 1 and b.count // epp == packs + 1

    wide = bc.record_width(eb)
    assert_layout(wide, eb)
    assert [len(b.rows) for b in wide] == [1, 8] * 10
    assert bc.list_launches(len(wide)) == [20]
    assert any((b.start * eb) % 16 and len(b.rows) == 8 for b in wide)
    assert any((b.start * eb) % 16 and len(b.rows) == 1 for b in wide)

    for n in (16, 17):
        small = bc.place(bc.small_set(eb, n), eb)
        assert_layout(small, eb)
        assert bc.kernarg_launches(small, 3) == [n]
