"""nbxReduceMultiWideMx without a GPU: the symbol, the argument checks (every
one before any device call: fake pointers, as tests/test_wide_stats_cpu.py), and
the numpy reference quantiser of tests/widemx on blocks written out by hand."""
import numpy as np
import pytest

E = 4   # ncclInvalidArgument
F16, F32, BF16, E4M3, E5M2 = 6, 7, 9, 10, 11
PROD = 1
FAKE = 0x100000
D, DS, S0, S1, SS0, SS1 = FAKE, FAKE + 0x1000, FAKE + 0x2000, FAKE + 0x3000, FAKE + 0x4000, FAKE + 0x5000


def call(nbx, dsts=(D,), dscales=(DS,), srcs=(S0, S1), sscales=None, count=64, st=BF16, dt=E4M3, op=None):
    return nbx.reduce_multi_wide_mx_raw(list(dsts), dscales and list(dscales), list(srcs), sscales and list(sscales),
                                        count, st, dt, op or nbx.DevRedOpFull())


def test_symbol_and_launch_constants(nbx):
    lib = nbx.load_library()
    assert hasattr(lib, "nbxReduceMultiWideMx")
    assert lib.nbxAbiVersion() == 1 and lib.nbxKernelCount() == 6 * 5 + 6 * 4   # a kernel table of its own
    assert (nbx.LaunchFamily.MxBlocks, nbx.LaunchFamily.MxGeneric, nbx.LAUNCH_MX_SCALED) == (17, 18, 16)
    assert nbx.mx_tile_elts(E4M3, 8) == 4 * 256 * 16 and nbx.mx_tile_elts(BF16, 8) == 2 * 256 * 16
    assert nbx.mx_tile_elts(BF16, 3) == nbx.mx_tile_elts(E5M2, 1) == 256 * 16 and nbx.mx_tile_elts(F32, 2) == 0


def test_checks_come_before_any_device_call(nbx):
    mx = dict(st=E4M3, sscales=(SS0, SS1))
    assert call(nbx, count=0) == 0 and call(nbx, count=0, **mx) == 0          # no-op after the checks
    assert call(nbx, count=0, dt=F32, dscales=None, **mx) == 0
    # types
    assert call(nbx, st=F32) == E and call(nbx, dt=BF16) == E and call(nbx, dt=F16) == E
    assert call(nbx, st=BF16, sscales=(SS0, SS1)) == E                         # scales with a 16-bit type
    assert call(nbx, dt=F32, dscales=None) == E                                # fp32 output with plain sources
    assert call(nbx, dt=F32, **mx) == E                                        # fp32 output with scales
    assert call(nbx, dscales=None) == E                                        # MX output without
    assert call(nbx, dscales=(0,)) == E and call(nbx, sscales=(SS0, 0), st=E4M3) == E   # NULL entries
    # ops
    bad_op, null_scalar = nbx.DevRedOpFull(), nbx.DevRedOpFull()
    bad_op.op = PROD
    null_scalar.op, null_scalar.scalarArgIsPtr = 3, 1
    assert call(nbx, op=bad_op) == E and call(nbx, op=null_scalar) == E
    # the wide sum's checks
    assert call(nbx, srcs=()) == E and call(nbx, srcs=(S0,) * 65) == E and call(nbx, dsts=(), dscales=()) == E
    assert call(nbx, srcs=(S0 + 1, S1)) == E and call(nbx, dsts=(0,)) == E     # odd bf16 source, NULL destination
    assert call(nbx, dt=F32, dscales=None, dsts=(D + 2,), **mx) == E           # fp32 destination off by 2
    # overlap
    assert call(nbx, dsts=(S0,), **mx) == E                                    # in place, dst scales not the source's
    assert call(nbx, dsts=(S0 + 16,), st=E4M3) == E                            # partly on a source
    assert call(nbx, dsts=(S0,)) == E                                          # on a source of another type
    assert call(nbx, dsts=(SS1,), **mx) == E and call(nbx, dscales=(S1 + 32,)) == E   # elements on scales, scales on elements
    assert call(nbx, dsts=(S0,), dscales=(SS1,), **mx) == E                    # in place with another source's scales
    assert call(nbx, dscales=(SS1 + 1,), **mx) == E                            # scales partly on a source's
    assert call(nbx, dscales=(D + 63,)) == E                                   # a destination's own two arrays
    assert call(nbx, dt=F32, dscales=None, dsts=(S0,), **mx) == E              # fp32 destination on a source


# (output, {index: accumulator}, scale byte, {index: code}); every other element is +0 -> code 0
HAND = [
    (E4M3, {3: -0.0}, 0, {3: 0x80}),                                            # all zeros keep their signs
    (E4M3, {0: 2.0 ** -127, 1: -2.0 ** -128, 2: 2.0 ** -149}, 0, {0: 0x38, 1: 0xB0, 2: 0}),   # m denormal: R = 2^127
    (E4M3, {0: 448 * 8.0, 1: 8.0}, 130, {0: 0x7E, 1: 0x38}),                    # 448 * 2^3
    (E4M3, {0: -464 / 64, 1: 1 / 64}, 121, {0: 0xFE, 1: 0x38}),                 # 464 * 2^-6: the tie rounds to 448
    (E4M3, {0: 480 * 1024.0, 1: 465 * 1024.0}, 137, {0: 0x7E, 1: 0x7E}),        # (464, 512) saturates to 448
    (E5M2, {0: 57344 * 2.0 ** -13, 1: 2.0 ** -13}, 114, {0: 0x7B, 1: 0x3C}),
    (E5M2, {0: 59392 * 2.0 ** 20}, 147, {0: 0x7B}),                             # rounds down to 57344
    (E5M2, {0: -61440 * 2.0 ** 20}, 147, {0: 0xFB}),                            # the tie rounds up, then saturates
    (E4M3, {0: 1.0, 1: np.nan, 2: 1e30}, 255, {0: 0x38, 1: 0x7F, 2: 0x7E}),     # MX's NaN block: unscaled
    (E5M2, {0: 1.0, 1: -np.inf, 2: 1e30}, 255, {0: 0x3C, 1: 0xFC, 2: 0x7B}),
    (E4M3, {0: 256.0, 1: 2.0 ** -9, 2: 2.0 ** -10, 3: -2.0 ** -12, 4: 3 * 2.0 ** -10}, 127,
     {0: 0x78, 1: 0x01, 2: 0, 3: 0x80, 4: 0x02}),                               # small elements underflow
]


@pytest.mark.parametrize("dt,acc,scale,codes", HAND)
def test_reference_quantiser_on_hand_written_blocks(oracle, dt, acc, scale, codes):
    from tests.widemx.test_reduce_gpu import mx_quantise
    from tests.wide.test_reduce_gpu import assert_same
    a = np.zeros(40, np.float32)       # the block, then a partial block of 8 that holds 1.0
    a[32:] = 1.0
    for i, v in acc.items():
        a[i] = v
    exp = np.zeros(40, np.uint8)
    exp[32:] = 0x78                    # 1.0 scaled to 2^emax, 256 / 32768: the code 0x78 in both types
    for i, c in codes.items():
        exp[i] = c
    got, s = mx_quantise(oracle, a, dt)
    assert_same(got, exp, dt)
    assert s.tolist() == [scale, 127 - (8 if dt == E4M3 else 15)]
