"""MXFP6 (NBX_FLOAT6_E2M3 / NBX_FLOAT6_E3M2) in nbxReduceMultiWideMx without a GPU:
the constants, the argument checks (every one before any device call: fake
pointers, as tests/test_wide_mx4_cpu.py) and the numpy reference quantiser and
packer of tests/widemx6 on include/nbx_reduce.h's worked values."""
import numpy as np
import pytest

E = 4   # ncclInvalidArgument
F16, F32, BF16, E4M3, E5M2, FP4, E2M3, E3M2 = 6, 7, 9, 10, 11, 32, 33, 34
FAKE = 0x100000
D, DS, S0, S1, SS0, SS1 = FAKE, FAKE + 0x1000, FAKE + 0x2000, FAKE + 0x3000, FAKE + 0x4000, FAKE + 0x5000


def call(nbx, dsts=(D,), dscales=(DS,), srcs=(S0, S1), sscales=None, count=64, st=BF16, dt=E2M3):
    return nbx.reduce_multi_wide_mx_raw(list(dsts), dscales and list(dscales), list(srcs), sscales and list(sscales),
                                        count, st, dt, nbx.DevRedOpFull())


def test_constants_and_tiles(nbx):
    lib = nbx.load_library()
    assert (nbx.FLOAT6_E2M3, nbx.FLOAT6_E3M2) == (E2M3, E3M2)
    assert (nbx.LaunchFamily.Mx6Blocks, nbx.LaunchFamily.Mx6Generic) == (22, 23)
    assert lib.nbxKernelCount() == 54 and lib.nbxAbiVersion() == 1
    for st in (F16, BF16, E2M3, E3M2, FP4, F32, E4M3, E5M2):
        for n in range(0, 10):
            assert (nbx.mx6_tile_elts(st, n) > 0) == (st in (F16, BF16, E2M3, E3M2) and 1 <= n <= 8), (st, n)


@pytest.mark.parametrize("t,other", [(E2M3, E3M2), (E3M2, E2M3)])
def test_checks_come_before_any_device_call(nbx, t, other):
    mx = dict(st=t, sscales=(SS0, SS1))
    assert call(nbx, st=t, dt=t) == E                                           # FP6 sources without scales
    for dt in (other, E4M3, E5M2, FP4, F16):                                    # FP6 into anything but itself or fp32
        assert call(nbx, dt=dt, **mx) == E
    for st in (E4M3, E5M2, FP4):                                                # fp8 / FP4, plain or MX, into FP6
        assert call(nbx, st=st, dt=t) == E and call(nbx, st=st, dt=t, sscales=(SS0, SS1)) == E
    assert call(nbx, dt=t, dscales=None) == E and call(nbx, dt=t, dscales=None, **mx) == E   # FP6 output without scales
    assert call(nbx, dt=F32, **mx) == E                                         # fp32 output with scales
    assert call(nbx, dt=t, sscales=(SS0, SS1)) == E and call(nbx, st=F32, dt=t) == E   # scales with 16-bit sources; fp32 sources
    assert call(nbx, dt=t, sscales=(SS0, 0), st=t) == E and call(nbx, dt=t, dscales=(0,)) == E   # NULL entries
    # overlap: an FP6 array of 65 elements is 49 bytes
    assert call(nbx, dsts=(S0 + 48,), dt=t, count=65, **mx) == E                # on the source's 49th byte
    assert call(nbx, dsts=(S0 - 48,), dt=t, count=65, **mx) == E                # its 49th byte is the source's first
    assert call(nbx, dsts=(S0 + 16,), dt=t, count=0, **mx) == 0                 # nothing overlaps at count 0
    assert call(nbx, dsts=(S0,), dt=t, **mx) == E                               # in place with another scale array
    assert call(nbx, dsts=(S0,), dscales=(SS1,), dt=t, **mx) == E               # ... with another source's
    assert call(nbx, dsts=(S0,), dt=t) == E                                     # in place on a 16-bit source
    assert call(nbx, dt=F32, dscales=None, dsts=(S0,), **mx) == E               # fp32 destination on a source
    # count == 0 is a no-op for each accepted pair
    assert call(nbx, dt=t, count=0) == 0 and call(nbx, dt=t, count=0, st=F16) == 0
    assert call(nbx, dt=t, count=0, **mx) == 0 and call(nbx, count=0, dt=F32, dscales=None, **mx) == 0


def test_other_entry_points_reject_the_tags(nbx):
    op = nbx.DevRedOpFull()
    for t in (E2M3, E3M2):
        assert nbx.mx_tile_elts(t, 2) == 0 and nbx.mx4_tile_elts(t, 2) == 0
        for st, dt in ((t, t), (t, F32), (BF16, t)):
            assert nbx.reduce_multi_wide_raw([D], [S0, S1], 64, st, dt, op) == E
            assert nbx.reduce_multi_wide_stats_raw([D], [S0, S1], 64, st, dt, op, DS) == E
            assert nbx.reduce_multi_wide_batch_raw([([D], [S0, S1], 64)], st, dt, op) == E
            sc = (SS0, SS1) if st == t else None
            assert nbx.reduce_multi_wide_mx_batch_raw([([D], None if dt == F32 else [DS], [S0, S1], sc, 64)], st, dt, op) == E


# (type, {index: accumulator} of the full block, its scale byte, {index: code}, the partial block's scale, its code):
# the worked values of include/nbx_reduce.h; every other element is +0 -> code 0
HAND = [
    (E2M3, {0: 7.5, 1: 1.0, 2: 7.75, 3: 0.0625, 4: 0.1875, 5: -1.0625}, 127,
     {0: 0x1F, 1: 0x08, 2: 0x1F, 3: 0x00, 4: 0x02, 5: 0x28}, 125, 0x18),
    (E2M3, {3: -0.0}, 0, {3: 0x20}, 125, 0x18),                                 # all zeros keep their signs
    (E2M3, {0: 1.0, 1: np.nan}, 255, {}, 125, 0x18),                            # no NaN code: the scale byte says it
    (E2M3, {0: 2.0 ** -130, 1: -2.0 ** -149}, 0, {0: 0x01, 1: 0x20}, 125, 0x18),   # m denormal: R = 2^127
    (E3M2, {0: 28.0, 1: 30.0, 2: 1.0, 3: 0.03125, 4: -31.5, 5: 26.0, 6: 22.0}, 127,
     {0: 0x1F, 1: 0x1F, 2: 0x0C, 3: 0x00, 4: 0x3F, 5: 0x1E, 6: 0x1E}, 123, 0x1C),
    (E3M2, {0: 1.0, 1: -np.inf}, 255, {}, 123, 0x1C),
]


@pytest.mark.parametrize("t,acc,scale,codes,tail_scale,tail_code", HAND)
def test_reference_quantiser_and_packer_on_worked_values(t, acc, scale, codes, tail_scale, tail_code):
    from tests.widemx6.test_reduce_gpu import mx6_quantise, pack6, unpack6
    a = np.zeros(39, np.float32)       # the block, then a partial block of 7 that holds 1.0
    a[32:] = 1.0
    for i, v in acc.items():
        a[i] = v
    exp = np.zeros(39, np.uint8)
    exp[32:] = tail_code
    for i, c in codes.items():
        exp[i] = c
    got, s = mx6_quantise(a, t)
    assert got.tolist() == exp.tolist() and s.tolist() == [scale, tail_scale]
    packed = pack6(got)                # 39 codes: 29 bytes and 2 bits, so 30 bytes with 6 spare bits
    assert packed.size == 30 and packed[-1] >> 2 == 0 and unpack6(packed, 39).tolist() == exp.tolist()
    c = got[:4].astype(int)            # the three byte formulas, written out
    assert packed[:3].tolist() == [(c[0] | c[1] << 6) & 255, (c[1] >> 2 | c[2] << 4) & 255, (c[2] >> 4 | c[3] << 2) & 255]
