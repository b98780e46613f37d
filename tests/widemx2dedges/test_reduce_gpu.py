"""nbxReduceMultiWideMx2d position by position (inputs: tests/widemx2dedges/cases.py,
their premises: tests/test_wide_mx2d_edges_cpu.py). Every call goes through
tests/widemx2d's run_2d — both copies bit for bit against mx_quantise down the
columns and along the rows, the guard bytes, the launch record — and what is
new is where the values lie: one known lane owns every column block's maximum,
specials in every wave and in the partial tiles, scale arrays at every 4-byte
offset, partial tiles with a wave partly on, eight destinations, a captured
graph, and two identities between device outputs that need no reference. The
file name places it with the single-GPU parity core, as tests/widemx2d's."""
import numpy as np
import pytest

from tests.wide.test_reduce_gpu import BF16, E4M3, E5M2, Dev, assert_same
from tests.widemx.test_reduce_gpu import KIND_IDS, KINDS, inputs
from tests.widemx2d.test_reduce_gpu import FAM_GENERIC, FAM_TILES, expected_2d, run_2d, sources
from tests.widemx2dedges import cases

pytestmark = pytest.mark.gpu

OUTS = (E4M3, E5M2)


def elt_bytes(st):
    return 1 if st in (E4M3, E5M2) else 2


def run_case(nbx, oracle, torch, kind, dt, case, nsrc, **kw):
    return run_2d(nbx, oracle, torch, kind, dt, case.rows, case.cols, nsrc, given=(case.srcs, case.scales), **kw)


# ---------------------------------------------------------------------------
# 1. one lane owns each column block's maximum

@pytest.mark.parametrize("k,kind", list(enumerate(KINDS)), ids=KIND_IDS)
@pytest.mark.parametrize("shift", [0, 1], ids=["shift0", "shift1"])
def test_spikes(nbx, oracle, torch_gpu, k, kind, shift):
    """Tile kernel, 2 sources: every column block's scale byte is decided by one lane, whose tile row, position in
    the group, wave and group go through every value over the two shifts."""
    tr, tc = nbx.mx2d_tile_shape()
    case = cases.spike_case(oracle, tr, tc, kind, 2, cases.shifts(tr)[shift])
    run_case(nbx, oracle, torch_gpu, kind, OUTS[(k + shift) % 2], case, 2)


@pytest.mark.parametrize("kind", [(BF16, False), (E4M3, True)], ids=["bf16", "mx-e4m3"])
@pytest.mark.parametrize("shift", [0, 1], ids=["shift0", "shift1"])
def test_spikes_nine_sources(nbx, oracle, torch_gpu, kind, shift):
    """The spikes in the last of 9 sources: slot 7 of the partial-first kernel, whose scales are srcScales[8]."""
    tr, tc = nbx.mx2d_tile_shape()
    case = cases.spike_case(oracle, tr, tc, kind, 9, cases.shifts(tr)[shift])
    run_case(nbx, oracle, torch_gpu, kind, OUTS[shift], case, 9)


@pytest.mark.parametrize("k,kind", list(enumerate(KINDS)), ids=KIND_IDS)
def test_spikes_generic_kernel(nbx, oracle, torch_gpu, k, kind):
    """The same matrices with the last source one element off: a column per lane."""
    tr, tc = nbx.mx2d_tile_shape()
    case = cases.spike_case(oracle, tr, tc, kind, 2, cases.shifts(tr)[k % 2])
    run_case(nbx, oracle, torch_gpu, kind, OUTS[k % 2], case, 2, src_off=elt_bytes(kind[0]), family=FAM_GENERIC)


@pytest.mark.parametrize("n,kind,special", [(n, k, s) for n, (k, s) in enumerate(cases.special_cases())],
                         ids=[f"{cases.KIND_ID[k]}:{s}" for k, s in cases.special_cases()])
def test_specials(nbx, oracle, torch_gpu, n, kind, special):
    """A special value instead of the spike in one block per wave, in the right partial tile and in the 20-row
    bottom tile: scale byte 0xFF (or 0, or bf16's extremes) in exactly those column and row blocks."""
    tr, tc = nbx.mx2d_tile_shape()
    case = cases.spike_case(oracle, tr, tc, kind, 2, cases.shifts(tr)[n % 2], special=special)
    dt = OUTS[n % 2]
    out, _ = run_case(nbx, oracle, torch_gpu, kind, dt, case, 2)
    if special in ("nan", "+inf", "-inf"):   # run_2d compared everything; this states the placement itself
        got = Dev.read(out["col"][1][0], np.uint8).reshape(-1, case.cols)
        assert sorted(zip(*np.nonzero(got == 0xFF))) == sorted(case.sites.values())
        got = Dev.read(out["row"][1][0], np.uint8).reshape(case.rows, -1)
        assert sorted(zip(*np.nonzero(got == 0xFF))) == sorted((32 * i + case.row_in[i, c], c // 32)
                                                               for i, c in case.sites.values())


# ---------------------------------------------------------------------------
# 2. scale arrays at every 4-byte offset

OFFSETS = [("cs4", 4, 0, FAM_TILES), ("cs8", 8, 0, FAM_TILES), ("cs12", 12, 0, FAM_TILES), ("rs4", 0, 4, FAM_TILES),
           ("rs8", 0, 8, FAM_TILES), ("rs12", 0, 12, FAM_TILES), ("cs4-rs4", 4, 4, FAM_TILES),
           ("rs1", 0, 1, FAM_GENERIC), ("rs2", 0, 2, FAM_GENERIC), ("cs3-rs1", 3, 1, FAM_GENERIC)]


@pytest.mark.parametrize("kind", [(BF16, False), (E5M2, True)], ids=["bf16", "mx-e5m2"])
@pytest.mark.parametrize("name,cs_off,rs_off,family", OFFSETS, ids=[o[0] for o in OFFSETS])
def test_scale_offsets(nbx, oracle, torch_gpu, kind, name, cs_off, rs_off, family):
    """Column and row scale arrays 4, 8 and 12 bytes past a 16-byte boundary stay with the tile kernel (the 16-byte
    column store and the dword or byte row stores at a 4-byte address); a row scale array 1 or 2 bytes off alone
    sends the call to the generic kernel. cols = tc: gathered-dword row scales; tc + 32: byte row scales."""
    tr, tc = nbx.mx2d_tile_shape()
    for cols in (tc, tc + 32):
        run_2d(nbx, oracle, torch_gpu, kind, OUTS[cols == tc], tr + 1, cols, 3, cs_off=cs_off, rs_off=rs_off,
               family=family)


# ---------------------------------------------------------------------------
# 3. partial tiles

@pytest.mark.parametrize("kind", [(BF16, False), (E4M3, True)], ids=["bf16", "mx-e4m3"])
@pytest.mark.parametrize("rows", [1, 7, 8, 9, 20, 31, "tr+8"])
def test_partial_tiles(nbx, oracle, torch_gpu, kind, rows):
    """A bottom tile with a wave partly on, exactly on, wholly off; a right tile with one, seven and eight groups
    on; the last row and the last group own column maxima."""
    tr, tc = nbx.mx2d_tile_shape()
    rows = tr + 8 if rows == "tr+8" else rows
    todo = [c for c in cases.partial_tile_cases(tr, tc) if c[1] == kind and c[2] == rows]
    assert len(todo) == (3 if kind[1] else 4)
    for n, _, _, cols, row_out in todo:
        case = cases.spike_case(oracle, tr, tc, kind, 2, cases.last_row_shift(tr, rows), rows, cols)
        run_case(nbx, oracle, torch_gpu, kind, OUTS[n // 2 % 2], case, 2, row_out=row_out)


# ---------------------------------------------------------------------------
# 4. eight destinations

@pytest.mark.parametrize("family", [FAM_TILES, FAM_GENERIC], ids=["tiles", "generic"])
def test_eight_destinations(nbx, oracle, torch_gpu, family):
    """NBX_MAX_DSTS copies of all four arrays, each checked, each with its guards."""
    tr, tc = nbx.mx2d_tile_shape()
    out, _ = run_2d(nbx, oracle, torch_gpu, (BF16, False), E4M3, tr + 1, tc + 16, 5, ndst=8, family=family,
                    cs_off=0 if family == FAM_TILES else 1)
    assert all(len(arrays) == 8 for w in ("row", "col") for arrays in out[w])


# ---------------------------------------------------------------------------
# 5. graph capture and replay

def test_graph_capture_and_replay(nbx, oracle, torch_gpu):
    """9 MX e4m3 sources -> MX e5m2, both copies: the fp32 pre-fold into scratch and the partial-first 2-D pass in
    one captured graph, replayed on its own inputs, on new ones, and on those again."""
    torch = torch_gpu
    tr, tc = nbx.mx2d_tile_shape()
    rows, cols = tr + 1, tc + 32
    n = rows * cols
    sets = [sources(oracle, E4M3, True, n, 9)]
    a, b = inputs(oracle, E4M3, True, n, seed=2), inputs(oracle, E4M3, True, n, seed=3)
    sets.append(((a[0] + b[0])[:9], (a[1] + b[1])[:9]))
    run_2d(nbx, oracle, torch, (E4M3, True), E5M2, rows, cols, 9)          # eager first
    dev = Dev(torch)
    sb = [dev.buf(n, 0, s) for s in sets[0][0]]
    ssb = [dev.buf(n // 32, 0, e) for e in sets[0][1]]
    exp0 = expected_2d(oracle, sets[0][0], sets[0][1], E4M3, E5M2, rows, cols)
    out = {w: (dev.buf(n), dev.buf(e[1].size)) for w, e in exp0.items()}
    ptr = lambda bs: [Dev.ptr(x) for x in bs]
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        nbx.reduce_multi_wide_mx2d(ptr(out["row"][:1]), ptr(out["row"][1:]), ptr(out["col"][:1]), ptr(out["col"][1:]),
                                   ptr(sb), ptr(ssb), rows, cols, E4M3, E5M2, nbx.DevRedOpFull(), 0,
                                   torch.cuda.current_stream().cuda_stream)
    for srcs, scales in (sets[0], sets[1], sets[1]):
        for buf, s in zip(sb + ssb, list(srcs) + list(scales)):
            buf[0][:s.nbytes].copy_(torch.from_numpy(s.view(np.uint8).copy()))
        for codes, scl in out.values():
            codes[0][:codes[2]].fill_(0xA5)
            scl[0][:scl[2]].fill_(0xA5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        exp = expected_2d(oracle, srcs, scales, E4M3, E5M2, rows, cols)
        for w, (codes, scl) in out.items():
            assert_same(Dev.read(codes, np.uint8), exp[w][0].reshape(-1), E5M2)
            assert np.array_equal(Dev.read(scl, np.uint8), exp[w][1].reshape(-1)), w
        for buf in sb + ssb + [x for pair in out.values() for x in pair]:
            assert Dev.guards_intact(buf)


# ---------------------------------------------------------------------------
# 6. identities between device outputs

@pytest.mark.parametrize("st", [BF16, E4M3], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("name,dr,nsrc,fam_t", [("tiles-tiles", 16, 3, FAM_TILES), ("tiles-generic", 8, 3, FAM_GENERIC),
                                                ("tiles-tiles-9", 16, 9, FAM_TILES)],
                         ids=["tiles-tiles", "tiles-generic", "tiles-tiles-9"])
def test_transposition(nbx, oracle, torch_gpu, st, name, dr, nsrc, fam_t):
    """Column blocks of M are row blocks of M^T: the column-wise copy of one call against the row-wise copy of a
    call on the host-transposed sources, device bytes against device bytes."""
    tr, tc = nbx.mx2d_tile_shape()
    kind, dt = (st, False), OUTS[nsrc % 2]
    case = cases.spike_case(oracle, tr, tc, kind, nsrc, cases.shifts(tr)[1], tr + dr, tc + 16)
    out, _ = run_case(nbx, oracle, torch_gpu, kind, dt, case, nsrc, row_out=False)
    flipped = cases.transposed(oracle, case, st, tc)
    out_t, _ = run_2d(nbx, oracle, torch_gpu, kind, dt, case.cols, case.rows, nsrc, family=fam_t, given=(flipped, None))
    codes = Dev.read(out["col"][0][0], np.uint8).reshape(case.rows, case.cols)
    scales = Dev.read(out["col"][1][0], np.uint8).reshape(-1, case.cols)
    codes_t = Dev.read(out_t["row"][0][0], np.uint8).reshape(case.cols, case.rows)
    scales_t = Dev.read(out_t["row"][1][0], np.uint8).reshape(case.cols, -1)
    assert np.array_equal(codes, codes_t.T) and np.array_equal(scales, scales_t.T)


def flat_mx(nbx, torch, dev, srcs, st, dt):
    """nbxReduceMultiWideMx of plain sources, left on the device: (codes buffer, scales buffer)."""
    n = srcs[0].size
    sb = [dev.buf(s.nbytes, 0, s) for s in srcs]
    codes, scl = dev.buf(n), dev.buf(n // 32)
    nbx.reduce_multi_wide_mx([Dev.ptr(codes)], [Dev.ptr(scl)], [Dev.ptr(b) for b in sb], None, n, st, dt,
                             nbx.DevRedOpFull(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return codes, scl


@pytest.mark.parametrize("first,dt,tiny", [("2d", E4M3, False), ("2d", E5M2, False), ("1d", E4M3, False),
                                           ("2d", E5M2, True), ("1d", E4M3, True)],
                         ids=["2d-e4m3", "2d-e5m2", "1d-e4m3", "2d-e5m2-denormal", "1d-e4m3-denormal"])
def test_row_wise_output_is_a_fixed_point(nbx, oracle, torch_gpu, first, dt, tiny):
    """The row-wise copy a first call left on the device (this function's or nbxReduceMultiWideMx's), passed as it
    lies there as the one MX source of a second call with the same output type, comes back byte for byte. denormal:
    bf16 sources of 2^-131 and below, every S = 0, so the second call's source values are fp32 denormals."""
    torch = torch_gpu
    tr, tc = nbx.mx2d_tile_shape()
    rows, cols = tr + 1, tc + 32
    case = cases.spike_case(oracle, tr, tc, (BF16, False), 3, cases.shifts(tr)[1], rows, cols, tiny=tiny)
    dev = Dev(torch)
    if first == "2d":
        out, dev = run_case(nbx, oracle, torch, (BF16, False), dt, case, 3)
        codes, scl = out["row"][0][0], out["row"][1][0]
    else:
        codes, scl = flat_mx(nbx, torch, dev, case.srcs, BF16, dt)
    fed = Dev.read(codes, np.uint8).copy(), Dev.read(scl, np.uint8).copy()
    if tiny:
        assert not fed[1].any() and fed[0].any()
    again, _ = run_2d(nbx, oracle, torch, (dt, True), dt, rows, cols, 1, given=([fed[0]], [fed[1]]),
                      staged=([codes], [scl]))
    assert np.array_equal(Dev.read(again["row"][0][0], np.uint8), fed[0])
    assert np.array_equal(Dev.read(again["row"][1][0], np.uint8), fed[1])
