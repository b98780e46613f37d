"""MXFP4 (NBX_FLOAT4_E2M1) in nbxReduceMultiWideMx without a GPU: the constants,
the argument checks (every one before any device call: fake pointers, as
tests/test_wide_mx_cpu.py) and the numpy reference quantiser of tests/widemx4 on
blocks written out by hand."""
import numpy as np
import pytest

E = 4   # ncclInvalidArgument
F16, F32, BF16, E4M3, E5M2, FP4 = 6, 7, 9, 10, 11, 32
FAKE = 0x100000
D, DS, S0, S1, SS0, SS1 = FAKE, FAKE + 0x1000, FAKE + 0x2000, FAKE + 0x3000, FAKE + 0x4000, FAKE + 0x5000


def call(nbx, dsts=(D,), dscales=(DS,), srcs=(S0, S1), sscales=None, count=64, st=BF16, dt=FP4):
    return nbx.reduce_multi_wide_mx_raw(list(dsts), dscales and list(dscales), list(srcs), sscales and list(sscales),
                                        count, st, dt, nbx.DevRedOpFull())


def test_constants_and_tiles(nbx):
    lib = nbx.load_library()
    assert nbx.FLOAT4_E2M1 == FP4 and (nbx.LaunchFamily.Mx4Blocks, nbx.LaunchFamily.Mx4Generic) == (19, 20)
    assert lib.nbxKernelCount() == 54 and lib.nbxAbiVersion() == 1
    for st in (F16, BF16, FP4, F32, E4M3, E5M2):
        for n in range(0, 10):
            assert (nbx.mx4_tile_elts(st, n) > 0) == (st in (F16, BF16, FP4) and 1 <= n <= 8), (st, n)


def test_checks_come_before_any_device_call(nbx):
    mx = dict(st=FP4, sscales=(SS0, SS1))
    assert call(nbx, st=FP4) == E                                               # FP4 sources without scales
    assert call(nbx, dt=E4M3, **mx) == E and call(nbx, dt=E5M2, **mx) == E      # FP4 into MXFP8
    assert call(nbx, st=E4M3) == E and call(nbx, st=E5M2, sscales=(SS0, SS1)) == E   # fp8, plain or MX, into FP4
    assert call(nbx, dscales=None) == E and call(nbx, dscales=None, **mx) == E  # FP4 output without scales
    assert call(nbx, dt=F32, **mx) == E                                         # fp32 output with scales
    assert call(nbx, sscales=(SS0, SS1)) == E and call(nbx, st=F32) == E        # scales with 16-bit sources; fp32 sources
    assert call(nbx, sscales=(SS0, 0), st=FP4) == E and call(nbx, dscales=(0,)) == E   # NULL entries
    # overlap: an FP4 array of 65 elements is 33 bytes
    assert call(nbx, dsts=(S0 + 32,), count=65, **mx) == E                      # on the source's 33rd byte
    assert call(nbx, dsts=(S0 - 32,), count=65, **mx) == E                      # its 33rd byte is the source's first
    assert call(nbx, dsts=(S0 + 16,), count=0, **mx) == 0                       # nothing overlaps at count 0
    assert call(nbx, dsts=(S0,), **mx) == E                                     # in place with another scale array
    assert call(nbx, dsts=(S0,), dscales=(SS1,), **mx) == E                     # ... with another source's
    assert call(nbx, dsts=(S0,)) == E                                           # in place on a 16-bit source
    assert call(nbx, dt=F32, dscales=None, dsts=(S0,), **mx) == E               # fp32 destination on a source
    # count == 0 is a no-op for each accepted pair
    assert call(nbx, count=0) == 0 and call(nbx, count=0, st=F16) == 0
    assert call(nbx, count=0, **mx) == 0 and call(nbx, count=0, dt=F32, dscales=None, **mx) == 0


def test_other_entry_points_reject_the_tag(nbx):
    op = nbx.DevRedOpFull()
    for st, dt in ((FP4, FP4), (FP4, F32), (BF16, FP4)):
        assert nbx.reduce_multi_wide_raw([D], [S0, S1], 64, st, dt, op) == E
        assert nbx.reduce_multi_wide_stats_raw([D], [S0, S1], 64, st, dt, op, DS) == E
        assert nbx.reduce_multi_wide_batch_raw([([D], [S0, S1], 64)], st, dt, op) == E


# ({index: accumulator}, scale byte, {index: code}); every other element is +0 -> code 0
HAND = [
    ({3: -0.0}, 0, {3: 0x8}),                                                   # all zeros keep their signs
    ({0: 6.0, 1: 1.0}, 127, {0: 0x7, 1: 0x2}),
    ({0: 7.0, 1: 5.0, 2: -2.5, 3: 0.25, 4: 0.75}, 127, {0: 0x7, 1: 0x6, 2: 0xC, 3: 0x0, 4: 0x2}),   # (6, 8) and ties
    ({0: 48.0, 1: 10.0}, 130, {0: 0x7, 1: 0x2}),                                # 6 * 2^3; 1.25 rounds to 1
    ({0: 1.0, 1: np.nan}, 255, {}),                                             # no NaN code: the scale byte says it
    ({0: 1.0, 1: -np.inf}, 255, {}),
    ({0: 2.0 ** -127, 1: 2.0 ** -149}, 0, {0: 0x2, 1: 0x0}),                    # m denormal: R = 2^127
    ({0: -1.75, 1: 3.5, 2: -1.25, 3: 4.0, 4: 0.2499999}, 127, {0: 0xC, 1: 0x6, 2: 0xA, 3: 0x6, 4: 0x0}),
]


@pytest.mark.parametrize("acc,scale,codes", HAND)
def test_reference_quantiser_on_hand_written_blocks(acc, scale, codes):
    from tests.widemx4.test_reduce_gpu import mx4_quantise, pack, unpack
    a = np.zeros(39, np.float32)       # the block, then a partial block of 7 that holds 1.0
    a[32:] = 1.0
    for i, v in acc.items():
        a[i] = v
    exp = np.zeros(39, np.uint8)
    exp[32:] = 0x6                     # 1.0 scaled to 2^emax = 4: S = 125
    for i, c in codes.items():
        exp[i] = c
    got, s = mx4_quantise(a)
    assert got.tolist() == exp.tolist() and s.tolist() == [scale, 125]
    assert pack(got).size == 20 and pack(got)[-1] >> 4 == 0 and unpack(pack(got), 39).tolist() == exp.tolist()
