"""Inputs and shared helpers of the instantiation-matrix tests
(tests/matrix/test_reduce_gpu.py, tests/test_matrix_inputs_cpu.py).

edge_inputs() is oracle.random_inputs() with two more value classes planted in
every float source, so that a kernel that flushes denormals, fuses a multiply
into an add or mishandles inf / NaN / -0 in one of its unrolled forms does not
pass on uniform[-1, 1) values alone:

  * 1/8 of the positions, drawn per source: uniformly random bit patterns of
    the storage width (every exponent, both zeros, inf, NaN, denormals);
  * 1/16 of the positions: random sign and mantissa under a biased exponent of
    0, 1 or 2 (denormals and the two smallest normal binades). Half of these
    positions are drawn per source; the other half (1/32 of all positions) is
    one set shared by every source of a call, the values still drawn per
    source. A sum lands in the denormal range only where every term is that
    small; with per-source positions alone that is (1/16)^n of the outputs
    (about 40 of 40,000 at two sources, none at eight), so the shared half is
    what makes sums — and PreMulSum's products — of denormals occur at every
    source count.

Integers stay full-range random. Everything is seeded: the same arguments give
the same arrays.
"""
import numpy as np

FLOAT_TYPES = {6, 7, 8, 9, 10, 11}
F16, F32, F64, BF16, E4M3, E5M2 = 6, 7, 8, 9, 10, 11
MANTISSA_BITS = {F16: 10, F32: 23, F64: 52, BF16: 7, E4M3: 3, E5M2: 2}
UINT_OF = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}

NAN_CAP = 0.10   # largest NaN share of an expected result (NaN is compared only as NaN)

SUM, PROD, MINMAX, PREMULSUM, SUMPOSTDIV = range(5)   # ncclDevRedOp_t
NCCL_MAX, NCCL_MIN, NCCL_AVG = 2, 3, 4                # ncclRedOp_t
WIDE_TYPES = [F16, BF16, E4M3, E5M2]
MAX_SRCS, MAX_WIDE_SRCS = 8, 15
# 9,037 packs = 2 x 4,096 + 3 x 256 + 77: for every unroll in {1, 4, 8, 16}
# several full tiles, a ragged last tile, then tail elements; 1,301 packs does
# the same for the LDS kernel's 256- / 512-pack tiles
PACKS, LDS_PACKS, ELT_COUNT = 9037, 1301, 3001


def max_count(eb):
    """The longest count a case uses: a head up to a 128-byte line, the packs, a tail."""
    epp = 16 // eb
    return 128 // eb + PACKS * epp + epp


def seed_for(dtype):
    return 9000 + 100 * dtype


def matrix_inputs(oracle, dtype):
    """The sources of every case of one datatype: 8 (15 for the types with
    fp32-accumulating sums) arrays of max_count elements, used by prefix."""
    eb = np.dtype(oracle.NP_STORAGE[dtype]).itemsize
    n = MAX_WIDE_SRCS if dtype in WIDE_TYPES else MAX_SRCS
    return edge_inputs(oracle, dtype, n, max_count(eb), seed_for(dtype))


def pre_op_srcs(nsrc, dtype):
    """nPreOpSrcs of the PreMulSum cases: 0, nsrc and interior values all occur."""
    return (3 * nsrc + dtype) % (nsrc + 1)


def op_cases(oracle, dtype, nsrc):
    """The nbxReduceMulti ops of one (type, source count):
    (label, devop, arg, npre, post, scalar on device)."""
    mn = oracle.host_to_dev_redop(NCCL_MIN, dtype, 1)
    mx = oracle.host_to_dev_redop(NCCL_MAX, dtype, 1)
    assert mn[0] == MINMAX and mx[0] == MINMAX and mn[1] != mx[1]
    eb = np.dtype(oracle.NP_STORAGE[dtype]).itemsize
    if dtype in FLOAT_TYPES:
        devop, scalar = oracle.host_to_dev_redop(NCCL_AVG, dtype, 3)   # the 3-rank Avg scalar (inexact)
        assert devop == PREMULSUM
    else:
        scalar = (int(np.random.default_rng(77 + dtype).integers(1, 1 << 62)) | 1) & ((1 << (8 * eb)) - 1)
    npre = pre_op_srcs(nsrc, dtype)
    cases = [("sum", SUM, 0, 0, False, False), ("prod", PROD, 0, 0, False, False),
             ("min", MINMAX, mn[1], 0, False, False), ("max", MINMAX, mx[1], 0, False, False),
             (f"premulsum npre={npre}", PREMULSUM, scalar, npre, False, nsrc % 2 == 1)]
    if dtype not in FLOAT_TYPES:
        div = 3 if nsrc % 2 else 64
        cases.append((f"sumpostdiv /{div}", SUMPOSTDIV, div, 0, True, False))
        if nsrc == 5:
            cases.append(("sumpostdiv /3 postOp clear", SUMPOSTDIV, 3, 0, False, False))
    return cases


def wide_cases(oracle, st, nsrc):
    """The nbxReduceMultiWide ops of one (type, source count): (devop, arg, npre)."""
    devop, arg = oracle.host_to_dev_redop(NCCL_AVG, F32, 3)   # the 3-rank Avg scalar in fp32
    assert devop == PREMULSUM
    return [(SUM, 0, 0), (PREMULSUM, arg, pre_op_srcs(nsrc, st))]


def edge_inputs(oracle, dtype, n_srcs, count, seed):
    """n_srcs raw storage arrays of `count` elements (module docstring)."""
    srcs = oracle.random_inputs(dtype, n_srcs, count, seed=seed)
    if dtype not in FLOAT_TYPES:
        return srcs
    st = np.dtype(oracle.NP_STORAGE[dtype])
    bits = 8 * st.itemsize
    ut = UINT_OF[st.itemsize]
    man = MANTISSA_BITS[dtype]
    shared = np.random.default_rng([seed, 0x5A]).choice(count, size=count // 32, replace=False)
    out = []
    for s, a in enumerate(srcs):
        rng = np.random.default_rng([seed, s, 0xED6E])
        u = np.ascontiguousarray(a).view(ut).copy()
        idx = rng.choice(count, size=count // 8, replace=False)
        u[idx] = rng.integers(0, 1 << bits, idx.size, dtype=np.uint64, endpoint=False).astype(ut) if bits < 64 else \
            rng.integers(0, np.iinfo(np.uint64).max, idx.size, dtype=np.uint64, endpoint=True)
        tiny = np.concatenate([rng.choice(count, size=count // 32, replace=False), shared])
        code = (rng.integers(0, 2, tiny.size, dtype=np.uint64) << np.uint64(bits - 1)) \
            | (rng.integers(0, 3, tiny.size, dtype=np.uint64) << np.uint64(man)) \
            | rng.integers(0, 1 << man, tiny.size, dtype=np.uint64)
        u[tiny] = code.astype(ut)
        out.append(u.view(st))
    return out


# ---------------------------------------------------------------------------
# comparison: bit for bit, NaN as NaN (tests/test_reduce_gpu.py's rule)

def is_nan(a, dtype):
    """NaN mask of raw storage values of `dtype`."""
    if dtype in (F32, F64):
        return np.isnan(a)
    if dtype == F16:
        return ((a & 0x7C00) == 0x7C00) & ((a & 0x3FF) != 0)
    if dtype == BF16:
        return ((a & 0x7F80) == 0x7F80) & ((a & 0x7F) != 0)
    if dtype == E4M3:
        return (a & 0x7F) == 0x7F
    if dtype == E5M2:
        return ((a & 0x7C) == 0x7C) & ((a & 0x03) != 0)
    return np.zeros(a.shape, dtype=bool)


def nan_share(a, dtype):
    return float(is_nan(a, dtype).mean()) if a.size else 0.0


def assert_same(got, exp, dtype):
    assert got.shape == exp.shape
    if dtype in FLOAT_TYPES:
        gn, en = is_nan(got, dtype), is_nan(exp, dtype)
        assert np.array_equal(gn, en), f"NaN mismatch at {np.flatnonzero(gn != en)[:8]}"
        keep = ~en
        ut = UINT_OF[got.itemsize]
        bad = np.flatnonzero(got.view(ut)[keep] != exp.view(ut)[keep])
        assert bad.size == 0, f"{bad.size} mismatches, first at {np.flatnonzero(keep)[bad[:8]]}: " \
                              f"got {got.view(ut)[keep][bad[:4]]} exp {exp.view(ut)[keep][bad[:4]]}"
    else:
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, f"{bad.size} mismatches, first at {bad[:8]}: got {got[bad[:4]]} exp {exp[bad[:4]]}"


def denormal_count(a, dtype):
    """Elements of a raw storage array that are denormal (non-zero under a zero exponent)."""
    st = np.dtype(a.dtype)
    u = a.view(UINT_OF[st.itemsize]).astype(np.uint64)
    man = MANTISSA_BITS[dtype]
    exp_bits = 8 * st.itemsize - 1 - man
    e = (u >> np.uint64(man)) & np.uint64((1 << exp_bits) - 1)
    m = u & np.uint64((1 << man) - 1)
    return int(((e == 0) & (m != 0)).sum())


# ---------------------------------------------------------------------------
# the fp32-accumulating sums' reference: the oracle's codecs around its fp32 fold

_TABLES = {}


def widen(oracle, a, dtype):
    """Raw codes -> fp32, through the oracle's scalar decoder of every code."""
    if dtype not in _TABLES:
        dec = {F16: oracle.f16_to_f32, BF16: oracle.bf16_to_f32, E4M3: oracle.e4m3_to_f32,
               E5M2: oracle.e5m2_to_f32}[dtype]
        n = 256 if dtype in (E4M3, E5M2) else 65536
        _TABLES[dtype] = np.array([dec(c) for c in range(n)], dtype=np.float32)
    return _TABLES[dtype][a]


def narrow(oracle, f, dtype):
    """fp32 -> raw codes with the oracle's scalar encoder, once per distinct value."""
    enc = {F16: oracle.f32_to_f16, BF16: oracle.f32_to_bf16, E4M3: oracle.f32_to_e4m3, E5M2: oracle.f32_to_e5m2}[dtype]
    bits, inv = np.unique(f.view(np.uint32), return_inverse=True)
    codes = np.array([enc(float(v)) for v in bits.view(np.float32)], dtype=oracle.NP_STORAGE[dtype])
    return codes[inv.reshape(-1)]
