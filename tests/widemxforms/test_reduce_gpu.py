"""The launch record of every form of nbxReduceMultiWideMx in one sweep: block
kernel or any-alignment kernel, family, unroll and flags for each accepted
(source, output) pair and 1..8 sources, the pass sequence of 9 sources, and the
same bits from the aligned and the offset run. What the bits are is the
per-format files' business (tests/widemx, widemx4, widemx6)."""
import functools

import numpy as np
import pytest

from tests.test_wide_mx_forms_cpu import (ACCEPTED, BF16, E2M3, E3M2, E4M3, E5M2, F16, F32, FORM_IDS, FP4, nbytes,
                                          unroll_mx, unroll_mx4, unroll_mx6)
from tests.wide.test_reduce_gpu import Dev, many_inputs

pytestmark = pytest.mark.gpu

OUT32, PART_FIRST, MX_SCALED = 2, 4, 16
# output type -> (block family, any-alignment family, unroll rule): the output names the family of a form
FAMILY = {E4M3: (17, 18, unroll_mx), E5M2: (17, 18, unroll_mx), FP4: (19, 20, unroll_mx4),
          E2M3: (22, 23, unroll_mx6), E3M2: (22, 23, unroll_mx6)}
SRC_FAMILY = {E4M3: FAMILY[E4M3], E5M2: FAMILY[E4M3], FP4: FAMILY[FP4], E2M3: FAMILY[E2M3], E3M2: FAMILY[E2M3]}
MX_FAMILIES = {17, 18, 19, 20, 22, 23}
N = 33          # one full block and a one-element tail: a tile of the block kernel and its tail lanes


def family(form):
    st, dt, _, _ = form
    return FAMILY[dt] if dt != F32 else SRC_FAMILY[st]


@functools.lru_cache(maxsize=None)
def inputs(oracle, st, scaled):
    """9 seeded sources of N finite elements, and their scale bytes (2^-7 .. 2^7, never the NaN block)."""
    rng = np.random.default_rng(100 + st)
    if st in (F16, BF16, E4M3, E5M2):
        srcs = many_inputs(oracle, st, 9, N, seed=7000 + st)
    else:                                   # every FP4 / FP6 code is a finite value
        srcs = [rng.integers(0, 256, nbytes(st, N), dtype=np.uint8) for _ in range(9)]
    return srcs, [rng.integers(120, 135, 2, dtype=np.uint8) for _ in range(9)] if scaled else None


class Staged:
    """The sources of one form on the device once, an aligned destination and one a byte (fp32: an element) off."""

    def __init__(self, nbx, oracle, torch, form):
        self.nbx, self.torch, self.form = nbx, torch, form
        st, dt, ss, ds = form
        srcs, scales = inputs(oracle, st, ss)
        self.dev = Dev(torch)
        self.srcs = [self.dev.buf(s.nbytes, 0, s) for s in srcs]
        self.scales = [self.dev.buf(2, 0, e) for e in scales] if ss else None
        self.out = {off: self.dev.buf(nbytes(dt, N), off) for off in (0, 4 if dt == F32 else 1)}
        self.osc = self.dev.buf(2) if ds else None

    def run(self, nsrc, off):
        """-> (destination bytes, scale bytes or None, the call's launch records)."""
        st, dt, ss, ds = self.form
        out = self.out[off]
        out[0].fill_(0xA5)
        if ds:
            self.osc[0].fill_(0xA5)
        self.nbx.launch_log_reset()
        self.nbx.reduce_multi_wide_mx([Dev.ptr(out)], [Dev.ptr(self.osc)] if ds else None,
                                      [Dev.ptr(b) for b in self.srcs[:nsrc]],
                                      [Dev.ptr(b) for b in self.scales[:nsrc]] if ss else None, N, st, dt,
                                      self.nbx.DevRedOpFull(), 0, self.torch.cuda.current_stream().cuda_stream)
        self.torch.cuda.synchronize()
        total, log = self.nbx.launch_log()
        assert total == len(log)
        for b in [out] + ([self.osc] if ds else []) + self.srcs + (self.scales or []):
            assert Dev.guards_intact(b), "bytes around a buffer were written"
        return Dev.read(out, np.uint8).copy(), Dev.read(self.osc, np.uint8).copy() if ds else None, log


def same_bits(a, b):
    assert np.array_equal(a[0], b[0]), f"destination bytes differ at {np.flatnonzero(a[0] != b[0])[:8]}"
    assert (a[1] is None and b[1] is None) or np.array_equal(a[1], b[1]), "scale bytes differ"


@pytest.mark.parametrize("form", ACCEPTED, ids=FORM_IDS)
def test_launch_record_of_every_form(nbx, oracle, torch_gpu, form):
    st, dt, ss, ds = form
    blocks, generic, unroll = family(form)
    flags = (MX_SCALED if ss else 0) | (OUT32 if dt == F32 else 0)
    staged = Staged(nbx, oracle, torch_gpu, form)
    for nsrc in range(1, 9):
        aligned = staged.run(nsrc, 0)
        assert aligned[2] == [(blocks, nsrc, unroll(st, nsrc), flags)], (nsrc, aligned[2])
        offset = staged.run(nsrc, 4 if dt == F32 else 1)
        assert offset[2] == [(generic, nsrc, 1, flags)], (nsrc, offset[2])
        same_bits(aligned, offset)


# one plain and one scaled kind per family, the scaled one into both of its outputs
NINE = [(BF16, E4M3, False, True), (E4M3, E5M2, True, True), (E5M2, F32, True, False),
        (F16, FP4, False, True), (FP4, FP4, True, True), (FP4, F32, True, False),
        (BF16, E3M2, False, True), (E2M3, E2M3, True, True), (E3M2, F32, True, False)]


@pytest.mark.parametrize("form", NINE, ids=[FORM_IDS[ACCEPTED.index(f)] for f in NINE])
def test_pass_sequence_of_nine_sources(nbx, oracle, torch_gpu, form):
    st, dt, ss, ds = form
    blocks, generic, unroll = family(form)
    out = OUT32 if dt == F32 else 0
    staged = Staged(nbx, oracle, torch_gpu, form)
    runs = []
    for off, fam in ((0, blocks), (4 if dt == F32 else 1, generic)):
        u = (lambda n: unroll(st, n)) if fam == blocks else (lambda n: 1)
        runs.append(staged.run(9, off))
        mx = [r for r in runs[-1][2] if r[0] in MX_FAMILIES]
        if ss:      # an fp32-output pass of 8 into the partial, then the PART pass of the partial and the ninth
            assert mx == [(fam, 8, u(8), MX_SCALED | OUT32), (fam, 2, u(2), MX_SCALED | PART_FIRST | out)], mx
            assert len(runs[-1][2]) == 2
        else:       # the first two sources are the wide sum's fp32 fold; one PART pass of the partial and seven
            assert mx == [(fam, 8, u(8), PART_FIRST)], mx
            assert len(runs[-1][2]) >= 2 and runs[-1][2][-1] == mx[0]
    same_bits(runs[0], runs[1])
