"""GPU parity of nbxReduceMultiWideMx2d against the flat fp32 fold of
tests/widemx reshaped to rows x cols and quantised per column block and per row
block by the same mx_quantise, bit for bit (NaN codes compared as NaN). The
file name places it with the single-GPU parity core, as tests/widemx's."""
import functools

import numpy as np
import pytest

from tests.wide.test_reduce_gpu import BF16, E4M3, E5M2, F32, PREMULSUM, SUM, Dev, assert_same, avg3_bits, make_op
from tests.widemx.test_reduce_gpu import KIND_IDS, KINDS, MX_SCALED, PART_FIRST, inputs, mx_quantise, reference

pytestmark = pytest.mark.gpu

FAM_TILES, FAM_GENERIC = 24, 25


def blocks_along_rows(oracle, m, dt):
    """rows x cols accumulators -> (codes rows x cols, scales rows x ceil(cols / 32)); a zero pad cannot raise a maximum."""
    rows, cols = m.shape
    pad = np.zeros((rows, -(-cols // 32) * 32), np.float32)
    pad[:, :cols] = m
    codes, scales = mx_quantise(oracle, pad.reshape(-1), dt)
    return codes.reshape(pad.shape)[:, :cols], scales.reshape(rows, -1)


@functools.lru_cache(maxsize=None)
def sources(oracle, st, scaled, count, nsrc):
    """The first nsrc of tests/widemx's 8 seeded sources (and their scale bytes), of a second seed's beyond 8."""
    a = inputs(oracle, st, scaled, count)
    b = inputs(oracle, st, scaled, count, seed=1) if nsrc > 8 else ([], [])
    return (a[0] + b[0])[:nsrc], (a[1] + b[1])[:nsrc] if scaled else None


def expected_2d(oracle, srcs, scales, st, dt, rows, cols, row_out=True, devop=SUM, arg=0, npre=0):
    """{"col": (codes rows x cols, scales ceil(rows / 32) x cols), "row": (codes, scales rows x ceil(cols / 32))}
    of the flat fp32 fold, quantised down the columns and (row_out) along the rows."""
    fold = reference(oracle, srcs, scales, st, F32, devop, arg, npre)[0].reshape(rows, cols)
    col_codes, col_scales = blocks_along_rows(oracle, np.ascontiguousarray(fold.T), dt)
    exp = {"col": (np.ascontiguousarray(col_codes.T), np.ascontiguousarray(col_scales.T))}
    if row_out:
        exp["row"] = blocks_along_rows(oracle, fold, dt)
    return exp


def run_2d(nbx, oracle, torch, kind, dt, rows, cols, nsrc, row_out=True, family=FAM_TILES, ndst=1, src_off=0, cs_off=0,
           devop=SUM, arg=0, npre=0, rs_off=0, given=None, staged=None):
    """One call, checked: both copies, the guard bytes, the last launch record. The inputs are the seeded ones, or
    `given` = (sources, scale arrays or None) as host arrays; `staged` = (source buffers, scale buffers or None)
    are Dev buffers that already hold `given` and are passed as they are. rs_off / cs_off: the row / column scale
    arrays' byte offset in their allocation."""
    st, scaled = kind
    n = rows * cols
    srcs, scales = given if given is not None else sources(oracle, st, scaled, n, nsrc)
    assert len(srcs) == nsrc and all(s.size == n for s in srcs) and (scales is not None) == scaled
    exp = expected_2d(oracle, srcs, scales, st, dt, rows, cols, row_out, devop, arg, npre)
    dev = Dev(torch)
    if staged is not None:
        sb, ssb = staged
    else:
        sb = [dev.buf(s.nbytes, src_off if k == nsrc - 1 else 0, s) for k, s in enumerate(srcs)]   # src_off: the last source's
        ssb = [dev.buf(e.size, 0, e) for e in scales] if scaled else None
    out = {w: ([dev.buf(n) for _ in range(ndst)],
               [dev.buf(e[1].size, cs_off if w == "col" else rs_off) for _ in range(ndst)]) for w, e in exp.items()}
    ptrs = lambda bs: [Dev.ptr(b) for b in bs] if bs else None
    row = out.get("row", (None, None))
    nbx.launch_log_reset()
    nbx.reduce_multi_wide_mx2d(ptrs(row[0]), ptrs(row[1]), ptrs(out["col"][0]), ptrs(out["col"][1]), ptrs(sb), ptrs(ssb),
                               rows, cols, st, dt, make_op(nbx, dev, devop, arg, devop == PREMULSUM), npre,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for w, (codes, scl) in out.items():
        for c, s in zip(codes, scl):
            assert_same(Dev.read(c, np.uint8), exp[w][0].reshape(-1), dt)
            got = Dev.read(s, np.uint8)
            assert np.array_equal(got, exp[w][1].reshape(-1)), (w, np.flatnonzero(got != exp[w][1].reshape(-1))[:8])
    for b in sb + (ssb or []) + [b for codes, scl in out.values() for b in codes + scl]:
        assert Dev.guards_intact(b), "bytes around a buffer were written"
    for b, s in zip(sb + (ssb or []), list(srcs) + list(scales or [])):
        assert np.array_equal(Dev.read(b, np.uint8), s.view(np.uint8).reshape(-1)), "a source was written"
    count, log = nbx.launch_log()
    last = log[-1]
    assert last[0] == family and last[1] == min(nsrc, 8), last
    assert bool(last[3] & MX_SCALED) == scaled and bool(last[3] & PART_FIRST) == (nsrc > 8) == (count > 1), last
    return out, dev


@pytest.mark.parametrize("k,kind", list(enumerate(KINDS)), ids=KIND_IDS)
@pytest.mark.parametrize("nsrc", [1, 2, 8, 9])
def test_tile_kernel(nbx, oracle, torch_gpu, k, kind, nsrc):
    """One full tile; one lane; a one-row column block beside a 16-column partial tile whose last row block is half
    a block (a 32-column one for scaled sources, which need whole row blocks), with and without the row-wise copy."""
    tr, tc = nbx.mx2d_tile_shape()
    dt = (E4M3, E5M2)[(k + nsrc) % 2]
    edge = tc + (32 if kind[1] else 16)
    for rows, cols, row_out in ((tr, tc, True), (1, 16, True), (tr + 1, edge, True), (tr + 1, edge, False)):
        if cols % 32 == 0 or not kind[1]:
            run_2d(nbx, oracle, torch_gpu, kind, dt, rows, cols, nsrc, row_out)


@pytest.mark.parametrize("k,kind", list(enumerate(KINDS)), ids=KIND_IDS)
def test_generic_kernel(nbx, oracle, torch_gpu, k, kind):
    """Layouts the tile kernel does not take: cols no multiple of 16, a source one element off, a column scale
    array one byte off; 9 sources once (the partial then is the only 16-byte aligned source)."""
    tr, tc = nbx.mx2d_tile_shape()
    st, scaled = kind
    dt, eb = (E4M3, E5M2)[k % 2], 1 if st in (E4M3, E5M2) else 2
    gen = dict(family=FAM_GENERIC)
    if not scaled:
        run_2d(nbx, oracle, torch_gpu, kind, dt, 5, 7, 3, **gen)
        run_2d(nbx, oracle, torch_gpu, kind, dt, tr + 1, 40, 2, row_out=k < 2, **gen)
    run_2d(nbx, oracle, torch_gpu, kind, dt, tr + 1, tc + 32, 9 if k in (1, 4) else 3, src_off=eb, **gen)
    run_2d(nbx, oracle, torch_gpu, kind, dt, tr + 1, tc + 32, 1, cs_off=1, row_out=k >= 2, **gen)


@pytest.mark.parametrize("family", [FAM_TILES, FAM_GENERIC])
def test_more_tiles_than_the_grid(nbx, oracle, torch_gpu, family):
    """Several tiles per workgroup (per wave): at one workgroup per CU, the smallest bucket of 3 TR - 1 rows with
    more tiles than CUs, and for the column-per-lane kernel a 40-column one with more wave tiles than waves.
    e4m3 sources keep the distinct accumulators, and so the reference's narrowings, few."""
    tr, tc = nbx.mx2d_tile_shape()
    cus = torch_gpu.cuda.get_device_properties(0).multi_processor_count
    rows, cols = (3 * tr - 1, tc * (cus // 3 + 1)) if family == FAM_TILES else (tr * 4 * cus + 1, 40)
    nbx.set_launch_config(1, 0)
    try:
        run_2d(nbx, oracle, torch_gpu, (E4M3, family == FAM_TILES), E4M3, rows, cols, 2, family=family)
    finally:
        nbx.set_launch_config(0, 0)


@pytest.mark.parametrize("case", ["three-dsts", "three-dsts-generic", "premul-device", "premul-device-9"])
def test_other_cases(nbx, oracle, torch_gpu, case):
    tr, tc = nbx.mx2d_tile_shape()
    kw = dict(ndst=3) if case.startswith("three") else dict(devop=PREMULSUM, arg=avg3_bits(oracle), npre=3)
    if case.endswith("generic"):
        kw.update(cs_off=2, family=FAM_GENERIC)
    run_2d(nbx, oracle, torch_gpu, (BF16, False), E4M3, tr + 1, tc + 16, 9 if case.endswith("9") else 5, **kw)


@pytest.mark.parametrize("kind", [(BF16, False), (E5M2, True)], ids=["bf16", "mx-e5m2"])
def test_row_wise_copy_is_the_flat_call(nbx, oracle, torch_gpu, kind):
    """cols % 32 == 0: the row-wise codes and scales are nbxReduceMultiWideMx's for count = rows * cols."""
    tr, tc = nbx.mx2d_tile_shape()
    rows, cols, torch = tr + 1, tc + 32, torch_gpu
    out, dev = run_2d(nbx, oracle, torch, kind, E4M3, rows, cols, 3)
    srcs, scales = sources(oracle, kind[0], kind[1], rows * cols, 3)
    sb = [dev.buf(s.nbytes, 0, s) for s in srcs]
    ssb = [dev.buf(e.size, 0, e) for e in scales] if scales else None
    flat, flat_scales = dev.buf(rows * cols), dev.buf(rows * cols // 32)
    nbx.reduce_multi_wide_mx([Dev.ptr(flat)], [Dev.ptr(flat_scales)], [Dev.ptr(b) for b in sb],
                             [Dev.ptr(b) for b in ssb] if ssb else None, rows * cols, kind[0], E4M3, nbx.DevRedOpFull(),
                             0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(Dev.read(flat, np.uint8), Dev.read(out["row"][0][0], np.uint8))
    assert np.array_equal(Dev.read(flat_scales, np.uint8), Dev.read(out["row"][1][0], np.uint8))
