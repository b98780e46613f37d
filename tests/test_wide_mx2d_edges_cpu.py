"""The premises of tests/widemx2dedges/test_reduce_gpu.py, without a GPU, on the
very inputs it uses (tests/widemx2dedges/cases.py): what makes those tests
tests of a lane, a wave or a tile is where the values lie, and that is
arithmetic on the inputs, checked here. Conditions, not measurements: an input
that fails one is a wrong input."""
import numpy as np
import pytest

from tests.wide.test_reduce_gpu import BF16, E4M3, E5M2, F32
from tests.widemx.test_reduce_gpu import KIND_IDS, KINDS, reference
from tests.widemx2d.test_reduce_gpu import expected_2d
from tests.widemx2dedges import cases

OUTS = (E4M3, E5M2)
B = cases.BLOCK


@pytest.fixture(scope="module")
def tile(nbx):
    return nbx.mx2d_tile_shape()


def spike_inputs(oracle, tile):
    """Every spike matrix of the GPU file without specials: (name, kind, nsrc, case)."""
    tr, tc = tile
    out = []
    for kind, kid in zip(KINDS, KIND_IDS):
        for shift in cases.shifts(tr):
            out.append((f"{kid}-{shift}", kind, 2, cases.spike_case(oracle, tr, tc, kind, 2, shift)))
    for kind in ((BF16, False), (E4M3, True)):
        for shift in cases.shifts(tr):
            out.append((f"9-{kind}-{shift}", kind, 9, cases.spike_case(oracle, tr, tc, kind, 9, shift)))
    for n, kind, rows, cols, _ in cases.partial_tile_cases(tr, tc):
        out.append((f"partial-{n}", kind, 2,
                    cases.spike_case(oracle, tr, tc, kind, 2, cases.last_row_shift(tr, rows), rows, cols)))
    out += [(f"identity-{name}", kind, nsrc, case) for name, kind, nsrc, case, _ in identity_inputs(oracle, tile)]
    return out


def identity_inputs(oracle, tile):
    """Part 6: (name, kind, nsrc, case, tiny)."""
    tr, tc = tile
    shift = cases.shifts(tr)[1]
    out = []
    for st in (BF16, E4M3):
        for dr, nsrc in ((16, 3), (8, 3), (16, 9)):
            out.append((f"t-{st}-{dr}-{nsrc}", (st, False), nsrc,
                        cases.spike_case(oracle, tr, tc, (st, False), nsrc, shift, tr + dr, tc + 16), False))
    for tiny in (False, True):
        out.append((f"fixed-{tiny}", (BF16, False), 3,
                    cases.spike_case(oracle, tr, tc, (BF16, False), 3, shift, tr + 1, tc + 32, tiny=tiny), tiny))
    return out


def test_planted_values_survive_their_source_type(oracle, tile):
    tr, tc = tile
    every = [(name, kind, case) for name, kind, _, case in spike_inputs(oracle, tile)]
    every += [(f"{kind}-{s}", kind, cases.spike_case(oracle, tr, tc, kind, 2, cases.shifts(tr)[n % 2], special=s))
              for n, (kind, s) in enumerate(cases.special_cases())]
    for name, (st, scaled), case in every:
        back = cases.decode(oracle, case.srcs, case.scales, st, case.rows, case.cols)
        for v, b in zip(case.vals, back):
            assert cases.same_bits(v, b), name
        if scaled:
            used = set(np.unique(case.scales[0]))
            assert used <= {126, 127, 128} and (127 in used) == (case.cols > tc), name
            assert {126, 128} <= used or case.rows == 1, name


def test_every_spike_owns_its_column_block(oracle, tile):
    """The accumulator at the spike is the spike, and at least two binades above every other of its block; the
    expected scale bytes differ between neighbouring columns and between blocks above one another."""
    for name, (st, scaled), nsrc, case in spike_inputs(oracle, tile):
        acc = reference(oracle, case.srcs, case.scales, st, F32)[0].reshape(case.rows, case.cols)
        nb = case.row_in.shape[0]
        at = (B * np.arange(nb)[:, None] + case.row_in, np.broadcast_to(np.arange(case.cols), case.row_in.shape))
        assert cases.same_bits(acc[at], case.vals[case.spike_src][at]), name
        assert all(not v[at].any() for k, v in enumerate(case.vals) if k != case.spike_src), name
        if case.rows > 1:
            assert cases.spike_margins(case, acc).min() >= 2, name
        for dt in OUTS:
            s = expected_2d(oracle, case.srcs, case.scales, st, dt, case.rows, case.cols, False)["col"][1]
            be = cases.biased_exp(np.ascontiguousarray(acc[at], np.float32).reshape(-1)).reshape(nb, -1)
            assert np.array_equal(s, np.maximum(be - cases.OUT_EMAX[dt], 0)), name   # the spike alone decides S
            if not name.startswith("identity-fixed-True"):                           # (there every S is 0)
                assert (s[:, 1:] != s[:, :-1]).all() and (s[1:] != s[:-1]).all(), name


def test_spike_positions_cover_the_tile(oracle, tile):
    """Over the shifts, in full tiles: every (tile row, position in the group) and every (wave, group)."""
    tr, tc = tile
    rows, cols = cases.spike_shape(tr, tc, False)
    assert rows == 2 * tr + 20 and cols == tc + 3 * cases.GROUP and cases.spike_shape(tr, tc, True)[1] == tc + 64
    row_pos, wave_grp = set(), set()
    for shift in cases.shifts(tr):
        row_in, exps = cases.layout(tr, tc, rows, cols, shift)
        assert exps.min() == 0 and exps.max() == cases.EXPS - 1
        for i in range(rows // tr):            # the full row tiles
            for c in range(tc):                # the full column tile
                t = (B * i + row_in[i, c]) % tr
                row_pos.add((t, c % cases.GROUP))
                wave_grp.add((t // (tr // 4), c // cases.GROUP))
    assert row_pos == {(t, p) for t in range(tr) for p in range(cases.GROUP)}
    assert wave_grp == {(w, g) for w in range(4) for g in range(tc // cases.GROUP)}
    for scaled in (False, True):               # the layout the cases are built from is this one
        case = cases.spike_case(oracle, tr, tc, (E4M3, scaled), 2, cases.shifts(tr)[1])
        assert np.array_equal(case.row_in, cases.layout(tr, tc, case.rows, case.cols, cases.shifts(tr)[1])[0])


def test_partial_tiles_put_maxima_on_the_last_row_and_group(oracle, tile):
    tr, tc = tile
    table = cases.partial_tile_cases(tr, tc)
    assert len(table) == 7 * 4 + 7 * 3 and {c[4] for c in table} == {True, False}
    assert {c[2] for c in table} == {1, 7, 8, 9, 20, 31, tr + 8}
    for n, kind, rows, cols, _ in table:
        case = cases.spike_case(oracle, tr, tc, kind, 2, cases.last_row_shift(tr, rows), rows, cols)
        last = case.row_in.shape[0] - 1
        assert B * last + case.row_in[last, 0] == rows - 1                # a spike on the last row that is on
        assert case.row_in[last, cols - cases.GROUP:].size == cases.GROUP  # and 16 in the last group that is on
        assert not kind[1] or cols % B == 0


def test_specials_land_where_their_names_say(oracle, tile):
    tr, tc = tile
    for n, (kind, special) in enumerate(cases.special_cases()):
        st, scaled = kind
        case = cases.spike_case(oracle, tr, tc, kind, 2, cases.shifts(tr)[n % 2], special=special)
        sites = case.sites
        assert set(sites) == {"w0", "w1", "w2", "w3", "right", "bottom"} and len(set(sites.values())) == 6
        for w in range(4):
            i, c = sites[f"w{w}"]
            assert i < case.rows // tr and c < tc and (B * i + case.row_in[i, c]) % tr // (tr // 4) == w
        assert sites["right"][1] >= tc and sites["bottom"][0] == 2 and case.rows - 2 * tr == 20
        value, zero_block = cases.SPECIALS[special]
        acc = reference(oracle, case.srcs, case.scales, st, F32)[0].reshape(case.rows, case.cols)
        for i, c in sites.values():
            r = B * i + case.row_in[i, c]
            assert cases.same_bits(acc[r:r + 1, c], np.array([value], np.float32)), (special, i, c)
            if zero_block:
                assert np.count_nonzero(acc[B * i:B * i + B, c]) == (special == "bf16-min")
        for dt in OUTS:
            exp = expected_2d(oracle, case.srcs, case.scales, st, dt, case.rows, case.cols)
            col_s, row_s = exp["col"][1], exp["row"][1]
            where = sorted(sites.values())
            rows_of = sorted((B * i + case.row_in[i, c], c // B) for i, c in where)
            if special in ("nan", "+inf", "-inf"):
                assert sorted(zip(*np.nonzero(col_s == 0xFF))) == where
                assert sorted(zip(*np.nonzero(row_s == 0xFF))) == rows_of
            else:
                assert not (col_s == 0xFF).any() and not (row_s == 0xFF).any()
                want = {"neg-zero": 0, "bf16-min": 0, "bf16-max": 254 - cases.OUT_EMAX[dt]}[special]
                assert all(col_s[i, c] == want for i, c in where)
            if special == "neg-zero":
                assert all(exp["col"][0][B * i + case.row_in[i, c], c] == 0x80 for i, c in where)


def test_reference_is_a_fixed_point_and_transposes(oracle, tile):
    """The two identities of part 6 hold for the numpy reference on part 6's inputs."""
    tr, tc = tile
    for name, (st, _), nsrc, case, tiny in identity_inputs(oracle, tile):
        for dt in OUTS:
            exp = expected_2d(oracle, case.srcs, None, st, dt, case.rows, case.cols)
            if name.startswith("t-"):
                flipped = cases.transposed(oracle, case, st, tc)
                exp_t = expected_2d(oracle, flipped, None, st, dt, case.cols, case.rows)
                assert np.array_equal(exp["col"][0], exp_t["row"][0].T), name
                assert np.array_equal(exp["col"][1], exp_t["row"][1].T), name
                assert case.cols % 16 == 0 and (case.rows % 16 == 0) == (case.rows == tr + 16)   # tiles / generic
            else:
                codes, scl = exp["row"][0].reshape(-1), exp["row"][1].reshape(-1)
                assert case.cols % B == 0 and cases.is_fixed_point(oracle, codes, scl, dt), name
                assert (not scl.any()) == tiny and codes.any(), name
                if tiny:   # most of the fed-back values (all but the spikes) are fp32 denormals
                    fed = cases.dequantise(oracle, codes, scl, dt)
                    assert 2 * np.count_nonzero((cases.biased_exp(fed) == 0) & (fed != 0)) > fed.size
                # ... and what the second call is expected to return for them is them
                again = expected_2d(oracle, [codes], [scl], dt, dt, case.rows, case.cols)["row"]
                assert np.array_equal(again[0].reshape(-1), codes) and np.array_equal(again[1].reshape(-1), scl)
