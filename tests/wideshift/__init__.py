"""What the tests of nbxReduceMultiWide's realigning kernel share:
tests/wideshift/test_reduce_gpu.py and its CPU companion
tests/test_wide_shift_cpu.py.

Here are the launch record of kWideShiftedLds<W, NSRC, OUT32, PART> (family
16), a Python mirror of the call's layout rule (include/nbx_debug.h
nbxDebugWideLayout; the CPU test asserts it equal to the library's on a table
of pointer values) and the case tables of the GPU file: where the sources and
destinations sit, and the counts of the matrix, the edge shapes and the
pipeline shape. The inputs are tests/matrix/inputs.py's, the expected values
its oracle composition (widen, the oracle's fp32 fold, narrow).
"""
from tests.matrix import inputs as mi

FAM_WIDE_PACKS, FAM_WIDE_ELTS, FAM_WIDE_SHIFT = 6, 7, 16   # include/nbx_debug.h nbxDebugLaunchLog
OUT32, PART_FIRST = 2, 4                                    # flag bits 1 and 2
ELEMENTS, PACKS, REALIGN = 0, 1, 2                          # nbxDebugWideLayout
DEFAULT_MIN_ELTS = 2097152   # the merged default of NBX_WIDE_SHIFT_MIN_ELTS: the measured crossover
WAVES, WAVE = 4, 64                                         # kShiftLdsWaves, lanes

EDGE_TYPES = [mi.BF16, mi.E4M3]
EDGE_SRCS = [3, 8]
EDGE_START = 0   # the edge shapes are prefixes of the uploads; their first elements hold no NaN (CPU test)
PIPE_TYPES = [mi.BF16, mi.E5M2]
PIPE_SRCS = [2, 3, 8, 11]
PIPE_SEED = 4242
POLICY_TYPE, POLICY_SEED = mi.E5M2, 5151   # the policy test's two sources of DEFAULT_MIN_ELTS elements


def shift_unroll(nsrc):
    """shiftLdsUnroll (nbx_kargs.h): packs per lane per source and wave tile."""
    return 2 if nsrc >= 3 else 1


def wide_unroll(nsrc):
    return 4 if nsrc >= 4 else 1


def unroll_of(family, nsrc):
    return {FAM_WIDE_SHIFT: shift_unroll(nsrc), FAM_WIDE_PACKS: wide_unroll(nsrc), FAM_WIDE_ELTS: 1}[family]


def records(family, nsrc, out32):
    """The records of one nbxReduceMultiWide call of `nsrc` sources: one pass,
    or a first pass of 8 into the fp32 partial and passes of the partial and up
    to 7 more sources (9..15 sources: one such pass)."""
    o32 = OUT32 if out32 else 0
    if nsrc <= 8:
        return [(family, nsrc, unroll_of(family, nsrc), o32)]
    assert nsrc <= 15
    return [(family, 8, unroll_of(family, 8), OUT32), (family, nsrc - 7, unroll_of(family, nsrc - 7), o32 | PART_FIRST)]


def layout(src_addrs, dst_addrs, count, eb, out32, min_elts):
    """Mirror of the library's rule: (layout, head). Packs: every source on one
    misalignment modulo 16 and every destination 16-byte aligned behind the
    head elements that align the sources. Realigning: any other layout whose
    destinations share one address modulo 16, from `min_elts` elements; the
    head aligns the destinations. Elements (head 0): the rest."""
    deb = 4 if out32 else eb
    mis = src_addrs[0] % 16
    h = (16 - mis) // eb if mis else 0
    if all(a % 16 == mis for a in src_addrs) and all((a + h * deb) % 16 == 0 for a in dst_addrs):
        return PACKS, min(h, count)
    dmis = dst_addrs[0] % 16
    if any(a % 16 != dmis for a in dst_addrs) or count < min_elts:
        return ELEMENTS, 0
    return REALIGN, min(((16 - dmis) % 16) // deb, count)


# ---------------------------------------------------------------------------
# placement

def src_offsets(eb, n=mi.MAX_WIDE_SRCS):
    """Source k at ((3k + 1) * eb) % 16 (the per-step realigning matrix's rule)."""
    return [((3 * k + 1) * eb) % 16 for k in range(n)]


def shared_dst_offset(eb, out32):
    """The non-zero offset the destinations share: head EPP - 2 (source type) or 2 (fp32)."""
    return 8 if out32 else (2 * eb) % 16


def matrix_dst_offset(nsrc, eb, out32):
    return 0 if nsrc % 2 else shared_dst_offset(eb, out32)


def head_of(dst_off, eb, out32):
    return ((16 - dst_off) % 16) // (4 if out32 else eb)


def mixed_shift_offsets(eb, out32, n=mi.MAX_WIDE_SRCS):
    """Even sources 16-byte aligned behind the head of shared_dst_offset (shift
    0), odd ones at their matrix offsets (shift != 0 for some)."""
    head = head_of(shared_dst_offset(eb, out32), eb, out32)
    zero = (-head * eb) % 16
    return [zero if k % 2 == 0 else o for k, o in enumerate(src_offsets(eb, n))]


def matrix_count(epp):
    """The per-step LDS matrix's size: full and ragged 256- and 512-pack workgroup tiles, then a tail."""
    return mi.LDS_PACKS * epp + epp - 1


def edge_shapes(eb, out32, nsrc):
    """[(name, count, source offsets)] with the destinations at
    shared_dst_offset: every count at which the kernel takes another path."""
    epp = 16 // eb
    head = head_of(shared_dst_offset(eb, out32), eb, out32)
    assert head >= 2
    offs = src_offsets(eb)
    wave_tile = shift_unroll(nsrc) * WAVE
    return [("one element", 1, offs),
            ("fewer than head", head - 1, offs),
            ("head only", head, offs),
            ("head and less than a pack", head + epp - 1, offs),
            ("head and one pack", head + epp, offs),
            ("one wave tile", head + wave_tile * epp, offs),
            ("one workgroup tile and a pack", head + (WAVES * wave_tile + 1) * epp + 1, offs),
            ("some sources unshifted", head + (wave_tile + 3) * epp + 2, mixed_shift_offsets(eb, out32))]


def pipe_packs(cus, nsrc):
    """Pipeline shape at one workgroup per CU (waves = 4 x CUs): 3 x waves + 5
    wave tiles, the last one ragged at 37 packs. nsrc is the pass's count (a
    call of 11 sources runs 8, then 4: both U = 2)."""
    waves = WAVES * cus
    tile = shift_unroll(min(nsrc, 8)) * WAVE
    return (3 * waves + 4) * tile + 37


def pipe_count(cus, nsrc, epp):
    return pipe_packs(cus, nsrc) * epp + epp - 1
