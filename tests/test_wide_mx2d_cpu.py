"""nbxReduceMultiWideMx2d without a GPU: the symbol, the constants and every
argument check. Every check comes before any device call, so the pointers are
fake (as tests/test_wide_mx_forms_cpu.py); a call that would pass its checks
with rows and cols > 0 is never made."""
import pytest

from tests.test_abi import declared_functions

E = 4  # ncclInvalidArgument
INT32, F16, F32, BF16, E4M3, E5M2, FP4, E2M3, E3M2 = 2, 6, 7, 9, 10, 11, 32, 33, 34
FAKE, STEP = 0x100000, 0x10000
RD, RS, CD, CS, S0, S1, SS0, SS1 = (FAKE + k * STEP for k in range(8))
ROWS, COLS = 33, 64                # 2112 elements; column scales 2 x 64 bytes, row scales 33 x 2, source scales 66
COL_SCALES, ROW_SCALES = 2 * 64, 33 * 2


def call(nbx, rows=ROWS, cols=COLS, st=BF16, dt=E4M3, rdsts=(RD,), rscales=(RS,), cdsts=(CD,), cscales=(CS,),
         srcs=(S0, S1), sscales=None, op=None):
    lst = lambda p: None if p is None else list(p)
    return nbx.reduce_multi_wide_mx2d_raw(lst(rdsts), lst(rscales), lst(cdsts), lst(cscales), lst(srcs), lst(sscales),
                                          rows, cols, st, dt, op or nbx.DevRedOpFull())


def test_symbol_and_constants(nbx):
    lib = nbx.load_library()
    assert "nbxReduceMultiWideMx2d" in nbx.PUBLIC_SYMBOLS and hasattr(lib, "nbxReduceMultiWideMx2d")
    assert {"nbxReduceMultiWideMx2d", "nbxDebugMx2dTileShape"} <= set(declared_functions())
    assert lib.nbxAbiVersion() == 1 and lib.nbxKernelCount() == 54
    assert (nbx.LaunchFamily.Mx2dTiles, nbx.LaunchFamily.Mx2dGeneric) == (24, 25)
    assert nbx.mx2d_tile_shape() == (32, 128)


def test_types_and_ops(nbx):
    mx = dict(sscales=(SS0, SS1))
    for st in (F16, BF16, E4M3, E5M2):
        for dt in (E4M3, E5M2):
            assert call(nbx, 0, COLS, st, dt) == 0 and call(nbx, ROWS, 0, st, dt) == 0
            assert call(nbx, 0, COLS, st, dt, **mx) == (0 if st in (E4M3, E5M2) else E)
            assert call(nbx, 0, COLS, st, dt, rdsts=None, rscales=None) == 0
    for dt in (F32, F16, BF16, INT32, FP4, E2M3, E3M2):                 # fp32 and FP4 / FP6 outputs
        assert call(nbx, 0, COLS, dt=dt) == E and call(nbx, 0, COLS, st=E4M3, dt=dt, **mx) == E
    for st in (F32, INT32, FP4, E2M3, E3M2):                            # ... and sources, plain or scaled
        for dt in (E4M3, st):
            assert call(nbx, 0, COLS, st=st, dt=dt) == E and call(nbx, 0, COLS, st=st, dt=dt, **mx) == E
    for devop in (1, 2, 4, 7):                                          # Prod, MinMax, SumPostDiv, not an op
        op = nbx.DevRedOpFull()
        op.op = devop
        assert call(nbx, 0, COLS, op=op) == E


def test_argument_shape(nbx):
    # at rows == 0 too: the shape of the argument lists is checked first
    for rows in (0, ROWS):
        assert call(nbx, rows, cdsts=None) == E and call(nbx, rows, cscales=None) == E
        assert call(nbx, rows, rscales=None) == E and call(nbx, rows, rdsts=None) == E   # one of the row pair alone
        assert call(nbx, rows, srcs=()) == E and call(nbx, rows, srcs=[S0] * 65) == E
        assert call(nbx, rows, cdsts=(), cscales=()) == E
        assert call(nbx, rows, rdsts=[RD] * 9, rscales=[RS] * 9, cdsts=[CD] * 9, cscales=[CS] * 9) == E
    assert call(nbx, rows=2 ** 40, cols=2 ** 40) == E                  # rows * cols overflows size_t
    assert call(nbx, cols=48, st=E4M3, sscales=(SS0, SS1)) == E        # scaled sources need cols % 32 == 0
    assert call(nbx, rows=0, cols=48, st=E4M3, sscales=(SS0, SS1)) == 0
    for kw in (dict(srcs=(S0, 0)), dict(cdsts=(0,)), dict(cscales=(0,)), dict(rdsts=(0,)), dict(rscales=(0,)),
               dict(st=E4M3, sscales=(SS0, 0)), dict(srcs=(S0 + 1, S1))):   # NULL entries; a bf16 pointer off by a byte
        assert call(nbx, **kw) == E, kw
        assert call(nbx, rows=0, **kw) == 0, kw


# every array against every other, by its last byte on the other's first; sizes for ROWS x COLS
N = ROWS * COLS
WRITTEN = {"rdsts": (RD, N), "rscales": (RS, ROW_SCALES), "cdsts": (CD, N), "cscales": (CS, COL_SCALES)}
READ = {"srcs": (S1, N), "sscales": (SS1, N // 32)}


@pytest.mark.parametrize("a", list(WRITTEN))
@pytest.mark.parametrize("b", list(WRITTEN) + list(READ))
def test_any_overlap_is_refused(nbx, a, b):
    base = dict(st=E4M3, sscales=(SS0, SS1))
    pa, na = WRITTEN[a]
    pb, nb = {**WRITTEN, **READ}[b]
    if a == b:
        # two destinations: their arrays of this kind on each other, everything else apart
        two = {k: (p, p + 0x4000) for k, (p, _) in WRITTEN.items()}
        two[a] = (pa, pa + na - 1)
        assert call(nbx, **{**base, **two}) == E
        assert call(nbx, rows=0, **{**base, **two}) == 0
        return
    for moved in (dict({a: (pb - na + 1,)}), dict({a: (pb + nb - 1,)})):   # a's last byte on b's first, a's first on b's last
        kw = {**base, **moved}
        assert call(nbx, **kw) == E, (a, b, moved)
        assert call(nbx, rows=0, **kw) == 0
    assert call(nbx, cdsts=(S1,), st=E4M3, dt=E4M3, sscales=(SS0, SS1)) == E   # no in-place form
