"""The instantiation-matrix tests' inputs and expectations, without a GPU
(tests/matrix/inputs.py, tests/matrix/test_reduce_gpu.py):

  * the edge-rich generator is deterministic;
  * NaN — compared only as NaN on the GPU — stays under the 10 % cap in the
    oracle's result of every type / op / source count / count the GPU file runs;
  * the generator really yields what it is there for: products and sums that
    land in the denormal range;
  * the oracle's per-step fold of these inputs equals an independent fold
    (numpy for fp32 / fp64 / integers, numpy float16 for f16, torch bfloat16
    for bf16, torch float8 with a finite clamp for fp8);
  * the GPU files that carry the parity core's basename sort with it."""
import numpy as np
import pytest

from tests.conftest import gpu_order_key
from tests.matrix import inputs as mi

ALL_TYPES = list(range(12))
F16, F32, F64, BF16, E4M3, E5M2 = mi.F16, mi.F32, mi.F64, mi.BF16, mi.E4M3, mi.E5M2
SUM, PROD = mi.SUM, mi.PROD

_INPUTS = {}


def inputs_of(oracle, dtype):
    if dtype not in _INPUTS:
        _INPUTS[dtype] = mi.matrix_inputs(oracle, dtype)
    return _INPUTS[dtype]


@pytest.fixture(scope="module", autouse=True)
def _release_inputs():
    yield
    _INPUTS.clear()


def bits(a):
    return a.view(mi.UINT_OF[a.itemsize])


# ---------------------------------------------------------------------------
# the generator

@pytest.mark.parametrize("dtype", [1, 4, F16, F32, F64, BF16, E4M3, E5M2])
def test_generator_is_deterministic(oracle, dtype):
    a = mi.edge_inputs(oracle, dtype, 3, 5000, seed=123)
    b = mi.edge_inputs(oracle, dtype, 3, 5000, seed=123)
    c = mi.edge_inputs(oracle, dtype, 3, 5000, seed=124)
    assert all(x.dtype == np.dtype(oracle.NP_STORAGE[dtype]) and x.size == 5000 for x in a)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))
    assert not any(np.array_equal(bits(x), bits(y)) for x, y in zip(a, c))
    assert not np.array_equal(bits(a[0]), bits(a[1]))   # the sources differ from each other


@pytest.mark.parametrize("dtype", sorted(mi.FLOAT_TYPES))
def test_generator_plants_both_value_classes(oracle, dtype):
    """Every float source holds denormals and NaN / inf in numbers that only
    the planted classes explain (uniform[-1, 1) values hold neither)."""
    n = 40000
    for s in mi.edge_inputs(oracle, dtype, 2, n, seed=5):
        # 1/16 of the positions get an exponent of 0, 1 or 2: a third of them denormal, but
        # for the one code in 2^mantissa that is a zero
        assert mi.denormal_count(s, dtype) > n // 16 // 3 // 2
        # 1/8 random bit patterns: one in 2^(exponent bits) is inf or NaN (e4m3fn: only
        # the all-ones mantissa under it); at least half the expected number
        u = bits(s).astype(np.uint64)
        man = mi.MANTISSA_BITS[dtype]
        top = (1 << (8 * s.itemsize - 1 - man)) - 1
        special = ((u >> np.uint64(man)) & np.uint64(top)) == top
        if dtype == E4M3:
            special &= (u & np.uint64(7)) == 7
        assert special.sum() >= (n // 8) // ((top + 1) * (8 if dtype == E4M3 else 1)) // 2 > 0


def counts_of(eb):
    """Every element count the GPU file runs at one element size."""
    epp = 16 // eb
    mis = (3 * eb) % 16 or eb
    return sorted({mi.PACKS * epp + epp - 1, (128 - mis) // eb + mi.PACKS * epp + epp - 1,
                   (16 - mis) // eb + mi.PACKS * epp + epp - 1, mi.ELT_COUNT, mi.LDS_PACKS * epp + epp - 1})


@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_nan_cap_per_step(oracle, dtype):
    srcs = inputs_of(oracle, dtype)
    eb = srcs[0].itemsize
    worst = 0.0
    for nsrc in range(1, mi.MAX_SRCS + 1):
        for label, devop, arg, npre, post, _ in mi.op_cases(oracle, dtype, nsrc):
            exp = oracle.reduce_multi(srcs[:nsrc], dtype, devop, arg, npre, post, threads=8)[0]
            for count in counts_of(eb):
                share = mi.nan_share(exp[:count], dtype)
                worst = max(worst, share)
                assert share <= mi.NAN_CAP, (label, nsrc, count, share)
    print(f"{oracle.TYPE_NAMES[dtype]}: largest NaN share {worst:.2%}")


@pytest.mark.parametrize("st", mi.WIDE_TYPES)
def test_nan_cap_wide(oracle, st):
    srcs = inputs_of(oracle, st)
    wide = [mi.widen(oracle, s, st) for s in srcs]
    worst = 0.0
    for nsrc in range(1, mi.MAX_WIDE_SRCS + 1):
        for devop, arg, npre in mi.wide_cases(oracle, st, nsrc):
            fold = oracle.reduce_multi(wide[:nsrc], F32, devop, arg, npre, threads=8)[0]
            # narrowing adds no NaN but e4m3's inf -> NaN; count those with the fold's own
            share32 = mi.nan_share(fold, F32)
            share_narrow = float((np.isnan(fold) | (np.isinf(fold) if st == E4M3 else False)).mean())
            for count in counts_of(srcs[0].itemsize):
                worst = max(worst, mi.nan_share(fold[:count], F32))
            assert share32 <= mi.NAN_CAP and share_narrow <= mi.NAN_CAP, (devop, nsrc, share32, share_narrow)
            for count in counts_of(srcs[0].itemsize):
                f = fold[:count]
                assert float((np.isnan(f) | (np.isinf(f) if st == E4M3 else False)).mean()) <= mi.NAN_CAP
    print(f"{oracle.TYPE_NAMES[st]}: largest NaN share of the fp32 fold {worst:.2%}")


@pytest.mark.parametrize("dtype,nsrc", [(F32, 8), (F64, 8)])
def test_products_land_in_the_denormal_range(oracle, dtype, nsrc):
    srcs = mi.edge_inputs(oracle, dtype, nsrc, 40000, seed=mi.seed_for(dtype))
    out = oracle.reduce_multi(srcs, dtype, PROD, threads=8)[0]
    n = mi.denormal_count(out, dtype)
    print(f"{oracle.TYPE_NAMES[dtype]} prod x{nsrc}: {n} denormal outputs of {out.size}")
    assert n > 100


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("nsrc", [2, 8])
def test_sums_land_in_the_denormal_range(oracle, dtype, nsrc):
    srcs = mi.edge_inputs(oracle, dtype, nsrc, 40000, seed=mi.seed_for(dtype))
    out = oracle.reduce_multi(srcs, dtype, SUM, threads=8)[0]
    n = mi.denormal_count(out, dtype)
    print(f"{oracle.TYPE_NAMES[dtype]} sum x{nsrc}: {n} denormal outputs of {out.size}")
    assert n > 100


# ---------------------------------------------------------------------------
# the oracle's fold of these inputs against independent arithmetic

def fold(srcs, fn):
    acc = srcs[0]
    for s in srcs[1:]:
        acc = fn(acc, s)
    return acc


def assert_fold(oracle, dtype, devop, nsrc, ref_bits):
    srcs = inputs_of(oracle, dtype)[:nsrc]
    got = oracle.reduce_multi(srcs, dtype, devop, threads=8)[0]
    mi.assert_same(got, ref_bits(srcs).view(got.dtype), dtype)


@pytest.mark.parametrize("nsrc", [2, 8])
@pytest.mark.parametrize("devop", [SUM, PROD])
@pytest.mark.parametrize("dtype", [0, 1, 2, 3, 4, 5, F32, F64])
def test_fold_matches_numpy(oracle, dtype, devop, nsrc):
    fn = np.add if devop == SUM else np.multiply

    def ref(srcs):
        with np.errstate(all="ignore"):
            if dtype in (F32, F64):
                return fold(srcs, fn)
            return fold([bits(s) for s in srcs], fn)   # integers fold as unsigned, modulo 2^n
    assert_fold(oracle, dtype, devop, nsrc, ref)


@pytest.mark.parametrize("nsrc", [2, 8])
@pytest.mark.parametrize("devop", [SUM, PROD])
def test_f16_fold_matches_numpy_float16(oracle, devop, nsrc):
    fn = np.add if devop == SUM else np.multiply

    def ref(srcs):
        with np.errstate(all="ignore"):
            return fold([s.view(np.float16) for s in srcs], fn).view(np.uint16)   # one rounding to half per step
    assert_fold(oracle, F16, devop, nsrc, ref)


@pytest.mark.parametrize("nsrc", [2, 8])
@pytest.mark.parametrize("devop", [SUM, PROD])
def test_bf16_fold_matches_torch(oracle, devop, nsrc):
    torch = pytest.importorskip("torch")

    def ref(srcs):
        ts = [torch.from_numpy(s.view(np.int16).copy()).view(torch.bfloat16) for s in srcs]
        out = fold(ts, torch.add if devop == SUM else torch.mul)
        assert out.dtype == torch.bfloat16
        return out.view(torch.int16).numpy().view(np.uint16)
    assert_fold(oracle, BF16, devop, nsrc, ref)


@pytest.mark.parametrize("nsrc", [2, 8])
@pytest.mark.parametrize("devop", [SUM, PROD])
@pytest.mark.parametrize("dtype", [E4M3, E5M2])
def test_fp8_fold_matches_torch(oracle, dtype, devop, nsrc):
    """Every step: widen, fp32 op, clamp finite values to the largest finite
    code's value (SATFINITE), cast round-to-nearest-even."""
    torch = pytest.importorskip("torch")
    tdt = torch.float8_e4m3fn if dtype == E4M3 else torch.float8_e5m2
    mx = 448.0 if dtype == E4M3 else 57344.0

    def step(a, b):
        r = (a.to(torch.float32) + b.to(torch.float32)) if devop == SUM else (a.to(torch.float32) * b.to(torch.float32))
        r = torch.where(torch.isfinite(r), r.clamp(-mx, mx), r)
        return r.to(tdt)

    def ref(srcs):
        ts = [torch.from_numpy(s.copy()).view(tdt) for s in srcs]
        return fold(ts, step).view(torch.uint8).numpy()
    assert_fold(oracle, dtype, devop, nsrc, ref)


# ---------------------------------------------------------------------------
# run order

@pytest.mark.parametrize("path", ["tests/matrix/test_reduce_gpu.py", "tests/wide/test_reduce_gpu.py",
                                  "tests/batch/test_reduce_gpu.py"])
def test_gpu_files_sort_with_the_parity_core(path):
    assert gpu_order_key(path) == gpu_order_key("tests/test_reduce_gpu.py")
    assert gpu_order_key(path, "test_pack_kernels[small_packs-0]") == gpu_order_key("tests/test_reduce_gpu.py")
