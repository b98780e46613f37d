"""Every form of nbxReduceMultiWideMx in one sweep, without a GPU: which (source,
output, scale arrays) combinations the single call and the batch take, the
overlap rule on each format's array bytes, and the three tile hooks. Every check
comes before any device call, so the pointers are fake (as
tests/test_wide_mx6_cpu.py); a call that would pass its checks at count > 0 is
never made."""
import itertools

import pytest

E = 4   # ncclInvalidArgument
INT32, F16, F32, BF16, E4M3, E5M2, FP4, E2M3, E3M2 = 2, 6, 7, 9, 10, 11, 32, 33, 34
TAGS = [F16, F32, BF16, E4M3, E5M2, FP4, E2M3, E3M2, INT32]
FAKE = 0x100000
D, DS, S0, S1, SS0, SS1 = FAKE, FAKE + 0x1000, FAKE + 0x2000, FAKE + 0x3000, FAKE + 0x4000, FAKE + 0x5000

# include/nbx_reduce.h's contract, written out: (source, output, source scales, destination scales).
# Source scales are there exactly for MX sources, destination scales exactly for an MX output.
MXFP8 = ([(st, dt, False, True) for st in (F16, BF16, E4M3, E5M2) for dt in (E4M3, E5M2)] +
         [(st, dt, True, True) for st in (E4M3, E5M2) for dt in (E4M3, E5M2)] +
         [(E4M3, F32, True, False), (E5M2, F32, True, False)])
MXFP4 = [(F16, FP4, False, True), (BF16, FP4, False, True), (FP4, FP4, True, True), (FP4, F32, True, False)]
MXFP6 = ([(st, dt, False, True) for st in (F16, BF16) for dt in (E2M3, E3M2)] +
         [(E2M3, E2M3, True, True), (E2M3, F32, True, False), (E3M2, E3M2, True, True), (E3M2, F32, True, False)])
ACCEPTED = MXFP8 + MXFP4 + MXFP6
FORM_IDS = [f"{st}-{dt}-{'mx' if ss else 'plain'}" for st, dt, ss, _ in ACCEPTED]


def nbytes(t, n):
    """Bytes of an array of n elements of a type tag."""
    if t == FP4:
        return (n + 1) // 2
    if t in (E2M3, E3M2):
        return (3 * n + 3) // 4
    return n * {F32: 4, F16: 2, BF16: 2, E4M3: 1, E5M2: 1}[t]


def call(nbx, form, count, dsts=(D,), dscales=(DS,), srcs=(S0, S1), sscales=(SS0, SS1)):
    st, dt, ss, ds = form
    return nbx.reduce_multi_wide_mx_raw(list(dsts), list(dscales) if ds else None, list(srcs),
                                        list(sscales) if ss else None, count, st, dt, nbx.DevRedOpFull())


def batch(nbx, form, count):
    st, dt, ss, ds = form
    bucket = ([D], [DS] if ds else None, [S0, S1], [SS0, SS1] if ss else None, count)
    return nbx.reduce_multi_wide_mx_batch_raw([bucket], st, dt, nbx.DevRedOpFull())


def test_the_accepted_set_is_what_the_header_lists():
    assert len(ACCEPTED) == len(set(ACCEPTED)) == 14 + 4 + 8


def test_type_matrix(nbx):
    for form in itertools.product(TAGS, TAGS, (False, True), (False, True)):
        assert call(nbx, form, 0) == (0 if form in ACCEPTED else E), form


def test_batch_takes_the_mxfp8_family_only(nbx):
    for form in itertools.product(TAGS, TAGS, (False, True), (False, True)):
        assert batch(nbx, form, 0) == (0 if form in MXFP8 else E), form


@pytest.mark.parametrize("form", ACCEPTED, ids=FORM_IDS)
def test_overlap_on_array_bytes(nbx, form):
    st, dt, ss, ds = form
    n = 65                                  # three blocks, the last of one element: 3 scale bytes
    sb, db = nbytes(st, n), nbytes(dt, n)
    # every offset below keeps the element alignment (2 for a 16-bit source, 4 for an fp32 destination),
    # so it is the overlap rule that answers; at count 0 the same pointers pass
    assert (db - 1) % (2 if st in (F16, BF16) else 1) == 0 and (sb - 1) % (4 if dt == F32 else 1) == 0
    on_first = dict(srcs=(D + db - 1, S1))              # the destination's last byte on the source's first byte
    on_last = dict(dsts=(S0 + sb - 1,))                 # the source's last byte on the destination's first byte
    cases = [on_first, on_last, dict(srcs=(S0, D + db - 1))]
    if ds:
        cases.append(dict(dscales=(S0 + sb - 1,)))      # a destination scale array on a source's last byte
        cases.append(dict(dscales=(S1 - 2,)))           # its last byte on a source's first
        cases.append(dict(dscales=(D + db - 1,)))       # ... and on the destination's own last byte
    if ss:
        cases.append(dict(dsts=(SS1,)))                 # a destination on a source's scale array
        cases.append(dict(sscales=(SS0, D + db - 1)))
    if ss and ds:
        cases.append(dict(dscales=(SS0 + 2,)))          # the two kinds of scale array on each other
    for kw in cases:
        assert call(nbx, form, n, **kw) == E, kw
        assert call(nbx, form, 0, **kw) == 0, kw
    # in place: the types agree, the sources are scaled, and the scale array is that source's own
    inplace = dict(dsts=(S1,), dscales=(SS1,))
    if st == dt and ss:
        assert call(nbx, form, 0, **inplace) == 0       # at count > 0 this one would reach the device
        assert call(nbx, form, n, dsts=(S1,)) == E      # another scale array
        assert call(nbx, form, n, dsts=(S1,), dscales=(SS0,)) == E   # another source's
    elif st != dt:                                      # plain fp8 into its own type runs in place: not called here
        assert call(nbx, form, n, **inplace) == E


def test_null_entries_and_element_alignment(nbx):
    for form in ACCEPTED:
        st, dt, ss, ds = form
        assert call(nbx, form, 65, srcs=(S0, 0)) == E and call(nbx, form, 65, dsts=(0,)) == E
        if ss:
            assert call(nbx, form, 65, sscales=(SS0, 0)) == E
        if ds:
            assert call(nbx, form, 65, dscales=(0,)) == E
        if st in (F16, BF16):
            assert call(nbx, form, 65, srcs=(S0 + 1, S1)) == E
        if dt == F32:
            assert call(nbx, form, 65, dsts=(D + 2,)) == E


# unroll of the block kernel: the constexpr rules of csrc/nbx_kargs.h, written out
def unroll_mx(st, n):      # mxUnroll over wideUnroll (4 from 4 sources): an fp8 group is one pack, a 16-bit group two
    return (4 if n >= 4 else 1) if st in (E4M3, E5M2) else (2 if n >= 4 else 1)


def unroll_mx4(st, n):     # mx4Unroll
    return (8 if n <= 4 else 4) if st == FP4 else (4 if n >= 4 else 2)


def unroll_mx6(st, n):     # mx6Unroll
    return (4 if n <= 4 else 2) if st in (E2M3, E3M2) else (2 if n <= 3 else 1)


# (hook, the family's source types, elements of a lane's group, unroll)
HOOKS = [("mx_tile_elts", (F16, BF16, E4M3, E5M2), 16, unroll_mx), ("mx4_tile_elts", (F16, BF16, FP4), 8, unroll_mx4),
         ("mx6_tile_elts", (F16, BF16, E2M3, E3M2), 32, unroll_mx6)]


@pytest.mark.parametrize("hook,kinds,group,unroll", HOOKS, ids=[h[0] for h in HOOKS])
def test_tile_hooks(nbx, hook, kinds, group, unroll):
    for st in TAGS:
        for n in range(0, 10):
            exp = unroll(st, n) * 256 * group if st in kinds and 1 <= n <= 8 else 0
            assert getattr(nbx, hook)(st, n) == exp, (st, n)
