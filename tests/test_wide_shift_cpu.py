"""nbxReduceMultiWide's realigning path without a GPU: the layout function the
dispatch uses (nbxDebugWideLayout: pure arithmetic on pointer values) against
the Python mirror beside the GPU test's case tables, the threshold hook, the
binding's constants, and the NaN share of every expected result
tests/wideshift/test_reduce_gpu.py compares against."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import wideshift as ws
from tests.matrix import inputs as mi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, F32, F64, BF16, E4M3, E5M2 = 6, 7, 8, 9, 10, 11
BASE = 0x7F0000100000   # a 1 MiB boundary; nothing is dereferenced
MI355X_CUS = 256


@pytest.fixture
def threshold(nbx):
    saved = nbx.set_wide_shift_min_elts(0)
    yield nbx.set_wide_shift_min_elts
    nbx.set_wide_shift_min_elts(saved)


# ---------------------------------------------------------------------------
# symbols and constants

def test_symbols_declared_exported_and_bound(nbx):
    header = open(os.path.join(ROOT, "include", "nbx_debug.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"long long\s+nbxDebugSetWideShiftMinElts\s*\(\s*long long", code)
    assert re.search(r"int\s+nbxDebugWideLayout\s*\(", code)
    lib = nbx.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", nbx.library_path()], capture_output=True, text=True,
                         check=True).stdout
    for name in ("nbxDebugSetWideShiftMinElts", "nbxDebugWideLayout"):
        assert hasattr(lib, name)
        assert any(l.split()[-1] == name and " T " in l for l in out.splitlines()), name
    assert callable(nbx.set_wide_shift_min_elts) and callable(nbx.wide_layout)
    assert nbx.LaunchFamily.WideRealignLds == ws.FAM_WIDE_SHIFT == 16
    assert (nbx.LaunchFamily.WidePacks, nbx.LaunchFamily.WideElements) == (ws.FAM_WIDE_PACKS, ws.FAM_WIDE_ELTS)
    assert (nbx.WIDE_LAYOUT_ELEMENTS, nbx.WIDE_LAYOUT_PACKS, nbx.WIDE_LAYOUT_REALIGN) == \
        (ws.ELEMENTS, ws.PACKS, ws.REALIGN) == (0, 1, 2)
    assert (nbx.LAUNCH_OUT32, nbx.LAUNCH_PART_FIRST) == (ws.OUT32, ws.PART_FIRST)
    assert nbx.WIDE_SHIFT_MIN_ELTS_DEFAULT == ws.DEFAULT_MIN_ELTS
    assert lib.nbxAbiVersion() == 1   # additive: the ABI version stays
    assert lib.nbxKernelCount() == 6 * 5 + 6 * 4   # the new kernels live in the wide launch table


def test_records():
    assert ws.records(ws.FAM_WIDE_SHIFT, 1, False) == [(16, 1, 1, 0)]
    assert ws.records(ws.FAM_WIDE_SHIFT, 2, True) == [(16, 2, 1, 2)]
    assert ws.records(ws.FAM_WIDE_SHIFT, 3, False) == [(16, 3, 2, 0)]
    assert ws.records(ws.FAM_WIDE_SHIFT, 8, True) == [(16, 8, 2, 2)]
    assert ws.records(ws.FAM_WIDE_SHIFT, 9, False) == [(16, 8, 2, 2), (16, 2, 1, 4)]
    assert ws.records(ws.FAM_WIDE_SHIFT, 15, True) == [(16, 8, 2, 2), (16, 8, 2, 6)]
    assert ws.records(ws.FAM_WIDE_ELTS, 11, False) == [(7, 8, 1, 2), (7, 4, 1, 4)]


# ---------------------------------------------------------------------------
# the threshold hook

def test_threshold_set_and_query(nbx, threshold):
    before = threshold(0)
    assert before >= 1
    for query in (0, -1, -(1 << 40)):
        assert threshold(query) == before   # values < 1 only query
    assert threshold(1) == before
    assert threshold(0) == 1
    assert threshold(1 << 40) == 1          # a long long: out of any count's reach
    assert threshold(12345) == 1 << 40
    assert threshold(before) == 12345
    assert threshold(0) == before


def test_threshold_default_and_env(nbx):
    """The default (a fresh process without the variable) and
    NBX_WIDE_SHIFT_MIN_ELTS; values that are no positive number leave the default."""
    prog = ("import sys; sys.path.insert(0, %r); from tests.conftest import load_package; "
            "print(load_package().set_wide_shift_min_elts(0))" % ROOT)
    for value, want in ((None, ws.DEFAULT_MIN_ELTS), ("8589934592", 1 << 33), ("0", ws.DEFAULT_MIN_ELTS),
                        ("junk", ws.DEFAULT_MIN_ELTS)):
        env = {k: v for k, v in os.environ.items() if k != "NBX_WIDE_SHIFT_MIN_ELTS"}
        if value is not None:
            env["NBX_WIDE_SHIFT_MIN_ELTS"] = value
        out = subprocess.run([sys.executable, "-c", prog], env=env, capture_output=True, text=True, check=True).stdout
        assert int(out.split()[-1]) == want, (value, out)
    assert ws.DEFAULT_MIN_ELTS >= 4096 and ws.DEFAULT_MIN_ELTS & (ws.DEFAULT_MIN_ELTS - 1) == 0


# ---------------------------------------------------------------------------
# the layout function against its mirror

def layout_table(eb, out32):
    """(name, source addresses, destination addresses, wanted class or None) of
    synthetic pointer values: every class, for 1..15 sources and 1..8 destinations."""
    deb = 4 if out32 else eb
    epp = 16 // eb
    rows = [("all aligned", [BASE, BASE + 4096], [BASE + 8192], ws.PACKS),
            ("one source", [BASE + 3 * 16], [BASE + 8192, BASE + 12288], ws.PACKS),
            ("one source off its destination", [BASE + eb], [BASE + 8192], ws.REALIGN),
            ("sources on two misalignments", [BASE, BASE + 4096 + eb], [BASE + 8192], ws.REALIGN),
            ("15 sources, the last one off", [BASE + 4096 * k for k in range(14)] + [BASE + 65536 + 8], [BASE + 8192 * 9],
             ws.REALIGN),
            ("destination off", [BASE, BASE + 4096], [BASE + 8192 + deb], ws.REALIGN),
            ("8 destinations together off", [BASE, BASE + 4096], [BASE + 8192 * (d + 1) + 8 for d in range(8)], ws.REALIGN),
            ("destinations on two alignments", [BASE, BASE + 4096], [BASE + 8192, BASE + 12288 + deb], ws.ELEMENTS),
            ("mixed sources, destinations on two alignments", [BASE, BASE + 4096 + eb],
             [BASE + 8192 + 8, BASE + 12288 + 8, BASE + 16384 + 4], ws.ELEMENTS),
            ("in place on a shifted source", [BASE + eb, BASE + 4096 + 2 * eb], [BASE + 4096 + 2 * eb],
             None if out32 else ws.REALIGN)]
    # one shared source misalignment; the destination where the pack kernel needs it, and off it
    for mis in range(eb, 16, eb):
        head = (16 - mis) // eb
        good = BASE + 8192 + (-head * deb) % 16
        rows.append((f"shared misalignment {mis}", [BASE + mis, BASE + 4096 + mis], [good], ws.PACKS))
        rows.append((f"shared misalignment {mis}, destination off", [BASE + mis, BASE + 4096 + mis], [good + deb],
                     ws.REALIGN))
    # the GPU file's placements
    offs = ws.src_offsets(eb)
    for nsrc in range(1, mi.MAX_WIDE_SRCS + 1):
        d = ws.matrix_dst_offset(nsrc, eb, out32)
        rows.append((f"matrix nsrc={nsrc}", [BASE + 4096 * k + o for k, o in enumerate(offs[:nsrc])],
                     [BASE + 65536 + 4096 * j + d for j in range(1 + nsrc % 3)], ws.REALIGN))
    d = ws.shared_dst_offset(eb, out32)
    rows.append(("mixed shifts", [BASE + 4096 * k + o for k, o in enumerate(ws.mixed_shift_offsets(eb, out32)[:8])],
                 [BASE + 65536 + d], ws.REALIGN))
    assert epp in (8, 16)
    return [r for r in rows if r[3] is not None]


@pytest.mark.parametrize("out32", [False, True], ids=["same", "fp32"])
@pytest.mark.parametrize("st", mi.WIDE_TYPES)
def test_layout_function_matches_the_mirror(nbx, threshold, st, out32):
    eb = 2 if st in (F16, BF16) else 1
    deb = 4 if out32 else eb
    dt = F32 if out32 else st
    limit = 5000
    threshold(limit)
    seen = set()
    for name, srcs, dsts, want in layout_table(eb, out32):
        for count in (1, 2, 16 // deb - 1, 16 // deb, 17, limit - 1, limit, limit + 1, 1 << 20, 1 << 33):
            got = nbx.wide_layout(dsts, srcs, count, st, dt)
            mirror = ws.layout(srcs, dsts, count, eb, out32, limit)
            assert got == mirror, (name, count, got, mirror)
            cls = want if want != ws.REALIGN or count >= limit else ws.ELEMENTS   # the threshold boundary
            assert got[0] == cls, (name, count, got)
            assert 0 <= got[1] <= min(count, 16 // eb - 1), (name, count, got)    # the head, clipped by count
            if cls == ws.REALIGN:
                assert got[1] == min(count, ((16 - dsts[0] % 16) % 16) // deb) < 16 // deb
                assert all((a + got[1] * deb) % 16 == 0 for a in dsts) or got[1] == count
            if cls == ws.ELEMENTS:
                assert got[1] == 0
            seen.add(cls)
    assert seen == {ws.ELEMENTS, ws.PACKS, ws.REALIGN}
    # the threshold alone moves a realigning layout between the two kernels
    srcs, dsts = [BASE + eb, BASE + 4096], [BASE + 8192]
    threshold(1)
    assert nbx.wide_layout(dsts, srcs, 1, st, dt)[0] == ws.REALIGN
    threshold(1 << 40)
    assert nbx.wide_layout(dsts, srcs, 1 << 39, st, dt)[0] == ws.ELEMENTS
    assert nbx.wide_layout(dsts, [BASE, BASE + 4096], 1 << 39, st, dt)[0] == ws.PACKS


def test_layout_head_values(nbx, threshold):
    threshold(1)
    # bf16 -> bf16, destination 2 elements past a boundary: 6 head elements; clipped by the count
    assert nbx.wide_layout([BASE + 4], [BASE + 2, BASE + 4096], 100, BF16, BF16) == (ws.REALIGN, 6)
    assert nbx.wide_layout([BASE + 4], [BASE + 2, BASE + 4096], 5, BF16, BF16) == (ws.REALIGN, 5)
    # fp8 -> fp8: up to 15; fp32 output: at most 3
    assert nbx.wide_layout([BASE + 1], [BASE + 2, BASE + 4096 + 7], 100, E4M3, E4M3) == (ws.REALIGN, 15)
    assert nbx.wide_layout([BASE + 4], [BASE + 2, BASE + 4096 + 7], 100, E5M2, F32) == (ws.REALIGN, 3)
    assert nbx.wide_layout([BASE + 12], [BASE + 2], 100, F16, F32) == (ws.REALIGN, 1)
    assert nbx.wide_layout([BASE], [BASE + 2], 100, F16, F32) == (ws.REALIGN, 0)
    # packs: the head aligns the sources
    assert nbx.wide_layout([BASE + 6], [BASE + 6, BASE + 4096 + 6], 100, BF16, BF16) == (ws.PACKS, 5)
    assert nbx.wide_layout([BASE + 12], [BASE + 6, BASE + 4096 + 6], 3, BF16, F32) == (ws.PACKS, 3)


def test_layout_bad_arguments(nbx, threshold):
    lib = nbx.load_library()
    good = ([BASE], [BASE + 4096], 64)
    assert nbx.wide_layout(*good, BF16, BF16)[0] == ws.PACKS
    for st, dt in ((F32, F32), (2, F32), (F64, F64), (-1, F32), (12, 12), (BF16, F16), (BF16, F64), (E4M3, E5M2)):
        assert nbx.wide_layout(*good, st, dt) == (-1, 0)
    assert nbx.wide_layout([], [BASE + 4096], 64, BF16, BF16)[0] == -1
    assert nbx.wide_layout([BASE], [], 64, BF16, BF16)[0] == -1
    assert nbx.wide_layout([BASE] * 9, [BASE + 4096], 64, BF16, BF16)[0] == -1
    assert nbx.wide_layout([BASE], [BASE + 4096] * 65, 64, BF16, BF16)[0] == -1
    assert nbx.wide_layout([BASE], [BASE + 4096] * 64, 64, BF16, BF16)[0] == ws.PACKS
    assert nbx.wide_layout([BASE, 0], [BASE + 4096], 64, BF16, BF16)[0] == -1       # NULL destination
    assert nbx.wide_layout([BASE], [BASE + 4096, 0], 64, BF16, BF16)[0] == -1       # NULL source
    assert nbx.wide_layout([BASE + 1], [BASE + 4096], 64, BF16, BF16)[0] == -1      # off the element size
    assert nbx.wide_layout([BASE], [BASE + 4097], 64, BF16, BF16)[0] == -1
    assert nbx.wide_layout([BASE + 2], [BASE + 4096], 64, BF16, F32)[0] == -1       # an fp32 destination at +2
    assert nbx.wide_layout([BASE + 1], [BASE + 4097], 64, E4M3, E4M3)[0] >= 0
    assert lib.nbxDebugWideLayout(None, 1, None, 1, 64, BF16, BF16, None) == -1
    # the head pointer may be NULL
    import ctypes
    d = (ctypes.c_void_p * 1)(BASE)
    s = (ctypes.c_void_p * 1)(BASE + 4096)
    assert lib.nbxDebugWideLayout(d, 1, s, 1, 64, BF16, BF16, None) == ws.PACKS


# ---------------------------------------------------------------------------
# the GPU file's case tables

@pytest.mark.parametrize("eb", [1, 2])
def test_case_tables(eb):
    """The placements are what the GPU file takes them for: inside the
    uploads, realigning for both outputs, with the shifts and the tile
    arithmetic its docstrings state."""
    epp = 16 // eb
    offs = ws.src_offsets(eb)
    assert len(set(offs[:8])) == 8 and 0 in offs[:8] and all(o % eb == 0 and o < 16 for o in offs)
    assert ws.matrix_count(epp) + 16 <= mi.max_count(eb)
    packs = mi.LDS_PACKS
    assert packs // 256 >= 2 and packs % 256 and packs // 512 >= 2 and packs % 512   # full and ragged workgroup tiles
    for out32 in (False, True):
        deb = 4 if out32 else eb
        d = ws.shared_dst_offset(eb, out32)
        head = ws.head_of(d, eb, out32)
        assert d % deb == 0 and 0 < d < 16 and head == (epp - 2 if not out32 else 2)
        for nsrc in ws.EDGE_SRCS:
            shapes = ws.edge_shapes(eb, out32, nsrc)
            names = [s[0] for s in shapes]
            assert len(set(names)) == len(names) == 8
            for name, count, so in shapes:
                assert 1 <= count <= ws.matrix_count(epp)
                src = [BASE + 4096 * k + o for k, o in enumerate(so[:nsrc])]
                lay, h = ws.layout(src, [BASE + 65536 + d], count, eb, out32, 1)
                assert lay == ws.REALIGN and h == min(head, count), name
                shifts = [(a + h * eb) % 16 for a in src]
                if name == "some sources unshifted":
                    assert 0 in shifts and any(shifts)
            by = {s[0]: s[1] for s in shapes}
            tile = ws.shift_unroll(nsrc) * 64
            assert by["fewer than head"] < head == by["head only"]
            assert (by["head and less than a pack"] - head) // epp == 0
            assert (by["head and one pack"] - head) // epp == 1
            assert by["one wave tile"] - head == tile * epp
            assert (by["one workgroup tile and a pack"] - head) // epp == 4 * tile + 1
    for nsrc in ws.PIPE_SRCS:
        tile = ws.shift_unroll(min(nsrc, 8)) * 64
        p = ws.pipe_packs(MI355X_CUS, nsrc)
        assert -(-p // tile) == 3 * 4 * MI355X_CUS + 5 and p % tile == 37
        assert ws.pipe_count(MI355X_CUS, nsrc, epp) * eb <= 6.5e6   # about 6 MB per source


# ---------------------------------------------------------------------------
# NaN is compared only as NaN: its share of every expected result stays under the cap

@pytest.mark.parametrize("st", mi.WIDE_TYPES)
def test_nan_cap_matrix_and_edges(oracle, st):
    """Every (output, source count, case) of the matrix at its count, and every
    edge shape's prefix (measured peak: 6.0 %, the fp32 fold of 15 f16
    sources)."""
    srcs = mi.matrix_inputs(oracle, st)
    eb = srcs[0].itemsize
    epp = 16 // eb
    n = ws.matrix_count(epp)
    wide = [mi.widen(oracle, s[:n], st) for s in srcs]
    worst = 0.0
    for nsrc in range(1, mi.MAX_WIDE_SRCS + 1):
        for case in mi.wide_cases(oracle, st, nsrc):
            fold = oracle.reduce_multi(wide[:nsrc], F32, case[0], case[1], case[2], threads=8)[0]
            for out32 in (True, False):
                dt = F32 if out32 else st
                exp = fold if out32 else mi.narrow(oracle, fold, st)
                share = mi.nan_share(exp, dt)
                assert share <= mi.NAN_CAP, (nsrc, case, out32, share)
                worst = max(worst, share)
                if st in ws.EDGE_TYPES and nsrc in ws.EDGE_SRCS:
                    for name, count, _ in ws.edge_shapes(eb, out32, nsrc):
                        start = ws.EDGE_START
                        assert mi.nan_share(exp[start:start + count], dt) <= mi.NAN_CAP, (nsrc, case, out32, name)
    assert 0.0 < worst <= mi.NAN_CAP


def test_nan_cap_policy_and_graph_inputs(oracle):
    """The policy test's two sources at the default threshold and one element
    below it, and the graph test's two replays (sources 0..2 and 5..7)."""
    st = ws.POLICY_TYPE
    srcs = mi.edge_inputs(oracle, st, 2, ws.DEFAULT_MIN_ELTS, ws.POLICY_SEED)
    fold = oracle.reduce_multi([mi.widen(oracle, s, st) for s in srcs], F32, mi.SUM, threads=8)[0]
    for exp, dt in ((fold, F32), (mi.narrow(oracle, fold, st), st)):
        assert mi.nan_share(exp, dt) <= mi.NAN_CAP and mi.nan_share(exp[:-1], dt) <= mi.NAN_CAP
    srcs = mi.matrix_inputs(oracle, BF16)
    n = ws.matrix_count(8)
    for first in (0, 5):
        fold = oracle.reduce_multi([mi.widen(oracle, s[:n], BF16) for s in srcs[first:first + 3]], F32, mi.SUM)[0]
        assert mi.nan_share(mi.narrow(oracle, fold, BF16), BF16) <= mi.NAN_CAP


@pytest.mark.parametrize("nsrc", ws.PIPE_SRCS)
@pytest.mark.parametrize("st", ws.PIPE_TYPES)
def test_nan_cap_pipeline(oracle, st, nsrc):
    """The pipeline inputs (the matrix generator at the longer count, here at
    the MI355X's 256 CUs; the GPU test asserts the same at the device's count)."""
    eb = np.dtype(oracle.NP_STORAGE[st]).itemsize
    count = ws.pipe_count(MI355X_CUS, nsrc, 16 // eb)
    longest = ws.pipe_count(MI355X_CUS, 8, 16 // eb)
    srcs = mi.edge_inputs(oracle, st, nsrc, longest, ws.PIPE_SEED + st)
    case = mi.wide_cases(oracle, st, nsrc)[nsrc % 2]
    fold = oracle.reduce_multi([mi.widen(oracle, s[:count], st) for s in srcs], F32, case[0], case[1], case[2],
                               threads=8)[0]
    assert mi.nan_share(fold, F32) <= mi.NAN_CAP
    assert mi.nan_share(mi.narrow(oracle, fold, st), st) <= mi.NAN_CAP
