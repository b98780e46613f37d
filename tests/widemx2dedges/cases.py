"""Inputs of the position-by-position tests of nbxReduceMultiWideMx2d, shared by
the GPU tests (tests/widemx2dedges/test_reduce_gpu.py) and their CPU companion
(tests/test_wide_mx2d_edges_cpu.py), which proves on these very inputs what the
GPU tests take for granted.

Spike matrices. Sources 0 and 1 hold +-(1 + j/4) 2^-6 everywhere (exact in f16,
bf16, e4m3 and e5m2; every sum is below 2^-4), further sources zeros. In every
column block (i, c) — rows [32 i, 32 i + 32) of column c — one row rho(i, c)
holds +-(1 + j/4) 2^e(i, c), e in 0..5, in one source and zeros in the others:
the accumulator there is the spike exactly and the block's maximum by at least
two binades, so one known lane of kMx2dTiles owns the block's scale. e differs
between neighbouring columns and between blocks above one another, so a lane
that took a neighbour's maximum stores another scale byte.

    rho(i, c) = (g + p + (tr / 4) i + shift) mod h     g = (c mod tc) / 16, p = c mod 16, h the block's rows

Over shift in {0, tr / 2} and the two full row tiles, every (tile row, position
in the 16-element group) and every (wave, group) is a spike position of a full
tile. The spike sits in source 0 of two sources and in the last of more, which
with 9 sources is the last slot behind the partial.

MX sources carry scale byte 127, but 126 / 128 by the parity of row + block in
the first column tile, with the codes doubled / halved: the values stay.

Specials replace the spike at `sites`: one block per wave of a full tile, one
in the right partial tile, one in the bottom partial tile."""
import functools
from collections import namedtuple

import numpy as np

from tests.wide.test_reduce_gpu import BF16, E4M3, E5M2, narrow, widen
from tests.widemx.test_reduce_gpu import KIND_IDS, KINDS, mx_quantise, scale_in

BLOCK, GROUP = 32, 16
EXPS = 6                                       # spike exponents 0 .. 5
KIND_ID = dict(zip(KINDS, KIND_IDS))
OUT_EMAX = {E4M3: 8, E5M2: 15}

Case = namedtuple("Case", "rows cols vals srcs scales row_in exps sites spike_src")


def shifts(tr):
    return (0, tr // 2)


def spike_shape(tr, tc, scaled):
    """Two full row tiles and a 20-row one; a full column tile and a 3- (MX sources: 4-) group one."""
    return 3 * tr - 12, tc + (64 if scaled else 48)


def layout(tr, tc, rows, cols, shift):
    """(row of the spike inside its block, spike exponent), each ceil(rows / 32) x cols."""
    i = np.arange(-(-rows // BLOCK))[:, None]
    c = np.arange(cols)[None, :]
    h = np.minimum(BLOCK, rows - BLOCK * i)
    row_in = ((c % tc) // GROUP + c % GROUP + (tr // 4) * i + shift) % h
    return row_in, (c + i) % EXPS


def last_row_shift(tr, rows):
    """The shift that puts column 0's spike of the last block on the bucket's last row."""
    i = (rows - 1) // BLOCK
    return (rows - BLOCK * i - 1 - (tr // 4) * i) % tr


def find_sites(tr, tc, rows, cols, row_in):
    """name -> (block row, column): w0 .. w3 in full tiles, by the wave of the spike's row; right; bottom."""
    sites = {}
    full = [i for i in range(rows // tr)]
    for w in range(4):
        start = 37 * w + 5
        sites[f"w{w}"] = next((i, c) for c in list(range(start, tc)) + list(range(start))
                              for i in (full[w % len(full)], full[(w + 1) % len(full)])
                              if (BLOCK * i + row_in[i, c]) % tr // (tr // 4) == w)
    sites["right"] = (0, tc + 20)
    sites["bottom"] = (-(-rows // BLOCK) - 1, cols - 3)
    return sites


SPECIALS = {   # name -> (value, the rest of the column block is zeroed)
    "nan": (np.nan, False), "+inf": (np.inf, False), "-inf": (-np.inf, False), "neg-zero": (-0.0, True),
    "bf16-max": (2.0 ** 127, False), "bf16-min": (2.0 ** -130, True),
}


def special_cases():
    """(kind, special) pairs: NaN and the zero block for every kind, the infinities where the type has them."""
    out = []
    for kind in KINDS:
        names = ["nan", "neg-zero"] + (["+inf", "-inf"] if kind[0] != E4M3 else [])
        out += [(kind, s) for s in names + (["bf16-max", "bf16-min"] if kind[0] == BF16 else [])]
    return out


def encode(oracle, vals, st, scaled, tc):
    """fp32 matrices -> (flat codes per source, flat scale bytes per source or None)."""
    rows, cols = vals[0].shape
    if not scaled:
        return [narrow(oracle, np.ascontiguousarray(v).reshape(-1), st) for v in vals], None
    r, j = np.indices((rows, cols // BLOCK))
    sb = np.where(j < tc // BLOCK, np.where((r + j) % 2 == 0, 126, 128), 127).astype(np.uint8)
    x = np.repeat(np.ldexp(np.float32(1), sb.astype(np.int32) - 127), BLOCK, axis=1).astype(np.float32)
    with np.errstate(all="ignore"):
        codes = [narrow(oracle, (v / x).astype(np.float32).reshape(-1), st) for v in vals]
    return codes, [sb.reshape(-1).copy() for _ in vals]


def decode(oracle, srcs, scales, st, rows, cols):
    """What the kernel folds: the widened (and scaled) sources as fp32 matrices."""
    out = []
    for k, s in enumerate(srcs):
        w = widen(oracle, s, st)
        if scales is not None:
            with np.errstate(all="ignore"):
                w = (w * np.repeat(scale_in(scales[k]), BLOCK)).astype(np.float32)
        out.append(w.reshape(rows, cols))
    return out


@functools.lru_cache(maxsize=None)
def spike_case(oracle, tr, tc, kind, nsrc, shift, rows=None, cols=None, special=None, tiny=False):
    """The spike matrices of one (source kind, source count, shift), encoded. tiny: every value times 2^-125
    (bf16 denormals; every block's S is 0)."""
    st, scaled = kind
    assert nsrc >= 2 and tr == BLOCK
    dr, dc = spike_shape(tr, tc, scaled)
    rows, cols = rows or dr, cols or dc
    rng = np.random.default_rng(20 * shift + nsrc + 1000 * st + 7 * scaled + rows * cols)
    mant = lambda shape: (1 - 2 * rng.integers(0, 2, shape)) * (1 + rng.integers(0, 4, shape) / 4)
    vals = [np.ldexp(mant((rows, cols)), -6).astype(np.float32) for _ in range(2)]
    vals += [np.zeros((rows, cols), np.float32) for _ in range(nsrc - 2)]
    row_in, exps = layout(tr, tc, rows, cols, shift)
    at = (BLOCK * np.arange(row_in.shape[0])[:, None] + row_in, np.broadcast_to(np.arange(cols), row_in.shape))
    spike_src = 0 if nsrc == 2 else nsrc - 1
    for v in vals:
        v[at] = 0
    vals[spike_src][at] = np.ldexp(mant(row_in.shape), exps).astype(np.float32)
    if tiny:
        vals = [np.ldexp(v, -125).astype(np.float32) for v in vals]
    sites = {}
    if special is not None:
        value, zero_block = SPECIALS[special]
        sites = find_sites(tr, tc, rows, cols, row_in)
        for i, c in sites.values():
            r = BLOCK * i + row_in[i, c]
            for k, v in enumerate(vals):
                if zero_block:
                    v[BLOCK * i:BLOCK * i + BLOCK, c] = 0
                    if special == "neg-zero":
                        v[r, c] = -0.0           # in every source: -0 + +0 would be +0
                if k == spike_src:
                    v[r, c] = value
    srcs, scales = encode(oracle, vals, st, scaled, tc)
    for a in vals + srcs + (scales or []):
        a.setflags(write=False)
    return Case(rows, cols, vals, srcs, scales, row_in, exps, sites, spike_src)


def transposed(oracle, case, st, tc):
    """The same (plain) sources as cols x rows matrices."""
    vals = [np.ascontiguousarray(v.T) for v in case.vals]
    return encode(oracle, vals, st, False, tc)[0]


def partial_tile_cases(tr, tc):
    """(index, kind, rows, cols, row-wise copy wanted) of part 3; the spike of column 0's last block is on the last row."""
    grid = [((BF16, False), r, c) for r in (1, 7, 8, 9, 20, 31, tr + 8) for c in (16, tc - 16, tc, tc + 16)]
    grid += [((E4M3, True), r, c) for r in (1, 7, 8, 9, 20, 31, tr + 8) for c in (32, tc - 32, tc)]
    return [(n, kind, r, c, n % 2 == 0) for n, (kind, r, c) in enumerate(grid)]


# ---------------------------------------------------------------------------
# predicates (numpy alone)

def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.array_equal(a.view(np.uint32)[~np.isnan(a)], b.view(np.uint32)[~np.isnan(b)]) and \
        np.array_equal(np.isnan(a), np.isnan(b))


def biased_exp(acc):
    return ((acc.view(np.uint32) & 0x7FFFFFFF) >> 23).astype(np.int64)


def spike_margins(case, acc):
    """Per column block: (biased exponent of the accumulator at the spike) - (the largest among the block's others)."""
    be = biased_exp(np.ascontiguousarray(acc, np.float32))
    nb = case.row_in.shape[0]
    out = np.zeros(case.row_in.shape, np.int64)
    for i in range(nb):
        blk = be[BLOCK * i:BLOCK * i + BLOCK].copy()
        cols = np.arange(case.cols)
        top = blk[case.row_in[i], cols].copy()
        blk[case.row_in[i], cols] = -1
        out[i] = top - blk.max(axis=0) if blk.shape[0] > 1 else top + 1
    return out


def dequantise(oracle, codes, scale_bytes, dt):
    """Flat codes and their flat scale bytes (32-element blocks) -> fp32."""
    with np.errstate(all="ignore"):
        return (widen(oracle, codes, dt) * np.repeat(scale_in(scale_bytes), BLOCK)[:codes.size]).astype(np.float32)


def is_fixed_point(oracle, codes, scale_bytes, dt):
    """mx_quantise of the dequantised (codes, scales) gives them back (flat blocks, a whole number of them)."""
    again = mx_quantise(oracle, dequantise(oracle, codes, scale_bytes, dt), dt)
    return np.array_equal(again[0], codes) and np.array_equal(again[1], scale_bytes)
