"""GPU parity of nbxReduceMultiWideMxBatch (kMxBatchList, launch family 21)
against tests/widemx's numpy reference — its `inputs` with the planted edge
blocks, `reference`, `mx_quantise` — bit for bit, NaN codes compared as NaN, and
against nbxReduceMultiWideMx bucket by bucket, byte for byte. Sources are
shared between buckets of one shape (buckets need only be independent in what
they write); every destination sits between guard bytes. The file name places
it with the single-GPU parity core (tests/conftest.py GPU_FILE_ORDER)."""
import numpy as np
import pytest

from tests.wide.test_reduce_gpu import BF16, E4M3, E5M2, F32, PREMULSUM, SUM, Dev, assert_same, avg3_bits, make_op
from tests.widemx.test_reduce_gpu import KIND_IDS, KINDS, inputs, reference

pytestmark = pytest.mark.gpu

T = 4096
COUNTS = [1, 31, 32, 33, T - 32, T, T + 37, 2 * T + 17]
FAM_BLOCKS, FAM_GENERIC, FAM_BATCH, OUT32, MX_SCALED, SEGS = 17, 18, 21, 2, 16, 8


@pytest.fixture
def batch_mode(nbx):
    lib = nbx.load_library()
    saved = lib.nbxDebugSetBatchMode(1)
    yield lib.nbxDebugSetBatchMode
    lib.nbxDebugSetBatchMode(saved)


class Table:
    """Buckets of one call: device buffers, expected values, the two ways to run them."""

    def __init__(self, nbx, oracle, torch, st, scaled, dt, devop=SUM, arg=0, npre=0):
        self.nbx, self.oracle, self.torch, self.dev = nbx, oracle, torch, Dev(torch)
        self.st, self.scaled, self.dt, self.fold = st, scaled, dt, (devop, arg, npre)
        self.shared, self.buckets = {}, []

    def host(self, count, nsrc, seed):
        parts = [inputs(self.oracle, self.st, self.scaled, count, seed=seed + s) for s in range((nsrc + 7) // 8)]
        return [x for p in parts for x in p[0]][:nsrc], [x for p in parts for x in p[1]][:nsrc] if self.scaled else None

    def add(self, nsrc, count, ndst=1, seed=0, src_off=0, dscale_off=0, inplace=False):
        """src_off: bytes source 1 (or 0) sits off its 16-byte boundary; inplace: destination 0 is source 1."""
        key = (nsrc, count, seed, src_off)
        if key not in self.shared or inplace:
            srcs, scales = self.host(count or 32, nsrc, seed)   # an empty bucket still has arrays
            nb = (count + 31) // 32 or 1
            sb = [self.dev.buf(s.nbytes, src_off if k == min(1, nsrc - 1) else 0, s) for k, s in enumerate(srcs)]
            ssb = [self.dev.buf(nb, 0, e) for e in scales] if self.scaled else None
            exp = reference(self.oracle, srcs, scales, self.st, self.dt, *self.fold) if count else None
            self.shared[key] = (sb, ssb, exp)
        sb, ssb, exp = self.shared.pop(key) if inplace else self.shared[key]
        self.buckets.append(dict(sb=sb, ssb=ssb, exp=exp, count=count, ndst=ndst, dscale_off=dscale_off,
                                 inplace=inplace))

    def outputs(self):
        """Fresh destinations for every bucket: (element buffers, scale buffers or None) each."""
        outs = []
        for b in self.buckets:
            n, nb = b["count"], (b["count"] + 31) // 32
            if b["inplace"]:
                outs.append(([b["sb"][1]], [b["ssb"][1] if b["ssb"] else self.dev.buf(nb)]))
            else:
                outs.append(([self.dev.buf(n * (4 if self.dt == F32 else 1)) for _ in range(b["ndst"])],
                             [self.dev.buf(nb, b["dscale_off"]) for _ in range(b["ndst"])] if self.dt != F32 else None))
        return outs

    def args(self, outs):
        p = lambda bufs: [Dev.ptr(x) for x in bufs] if bufs is not None else None
        return [(p(o), p(osc), p(b["sb"]), p(b["ssb"]), b["count"]) for b, (o, osc) in zip(self.buckets, outs)]

    def run(self, outs=None, per_bucket=False, on_device=False):
        """One batched call (or one single call per bucket); returns (destinations, launch record)."""
        outs = outs or self.outputs()
        op = make_op(self.nbx, self.dev, self.fold[0], self.fold[1], on_device)
        stream = self.torch.cuda.current_stream().cuda_stream
        self.nbx.launch_log_reset()
        if per_bucket:
            for a in self.args(outs):
                self.nbx.reduce_multi_wide_mx(*a, self.st, self.dt, op, self.fold[2], stream)
        else:
            self.nbx.reduce_multi_wide_mx_batch(self.args(outs), self.st, self.dt, op, self.fold[2], stream)
        self.torch.cuda.synchronize()
        return outs, self.nbx.launch_log()

    def read(self, outs):
        return [([Dev.read(x, np.uint8) for x in o], [Dev.read(x, np.uint8) for x in osc or []]) for o, osc in outs]

    def check(self, outs):
        for k, (b, (o, osc)) in enumerate(zip(self.buckets, outs)):
            for buf in o + (osc or []):
                assert Dev.guards_intact(buf), f"bucket {k}: bytes around a destination were written"
            if b["count"] == 0:
                continue
            for d in range(len(o)):
                assert_same(Dev.read(o[d], np.float32 if self.dt == F32 else np.uint8), b["exp"][0], self.dt)
                if osc:
                    got = Dev.read(osc[d], np.uint8)
                    assert np.array_equal(got, b["exp"][1]), f"bucket {k}: scale bytes differ"

    def batch_records(self, nsrcs):
        """One family-21 launch per source count present, with that count's buckets."""
        flags = (OUT32 if self.dt == F32 else 0) | (MX_SCALED if self.scaled else 0)
        return [(FAM_BATCH, n, 1, flags | nsrcs.count(n) << SEGS) for n in sorted(set(nsrcs))]


# plain sources store MX only (their fp32 sum is nbxReduceMultiWide's): 4 x 2 + 2 x 3 pairs
PAIRS = [(kind, dt) for kind in KINDS for dt in (E4M3, E5M2, F32) if dt != F32 or kind[1]]
PAIR_IDS = [f"{k}-{ {E4M3: 'e4m3', E5M2: 'e5m2', F32: 'fp32'}[dt] }" for k, kind in zip(KIND_IDS, KINDS)
            for dt in (E4M3, E5M2, F32) if dt != F32 or kind[1]]


@pytest.mark.parametrize("kind,dt", PAIRS, ids=PAIR_IDS)
def test_every_instantiation(nbx, oracle, torch_gpu, batch_mode, kind, dt):
    t = Table(nbx, oracle, torch_gpu, *kind, dt)
    nsrcs = [1 + k % 8 for k in range(16)]
    for k, nsrc in enumerate(nsrcs):
        t.add(nsrc, COUNTS[(k + k // 8) % 8], ndst=1 + k % 3)   # every count, each source count at two of them
    outs, (total, recs) = t.run()
    t.check(outs)
    assert (total, recs) == (8, t.batch_records(nsrcs))


@pytest.mark.parametrize("kind,nsrc,n,launches", [((BF16, False), 2, 150, [150]), ((E4M3, True), 8, 334, [333, 1])],
                         ids=["search", "split"])
def test_record_search_and_width(nbx, oracle, torch_gpu, batch_mode, kind, nsrc, n, launches):
    """>= 130 records: the ballot search takes a second and a third step; nDsts 1 and 2 share a launch
    (recWords 23 for 8 scaled sources: 333 records fill a slot, the 334th is a second launch)."""
    t = Table(nbx, oracle, torch_gpu, *kind, E4M3)
    for k in range(n):
        t.add(nsrc, [1, 33, 64, T + 37][k % 4], ndst=1 + k % 2)
    outs, (total, recs) = t.run()
    t.check(outs)
    flags = MX_SCALED if kind[1] else 0
    assert (total, recs) == (len(launches), [(FAM_BATCH, nsrc, 1, flags | m << SEGS) for m in launches])


@pytest.mark.parametrize("mode", [1, 0], ids=["lists", "lists-off"])
@pytest.mark.parametrize("kind", [(BF16, False), (E4M3, True)], ids=["bf16", "mx-e4m3"])
def test_equals_per_bucket_calls(nbx, oracle, torch_gpu, batch_mode, kind, mode):
    """Buckets that leave the table among buckets that stay: identical bytes either way."""
    batch_mode(mode)
    t = Table(nbx, oracle, torch_gpu, *kind, E5M2)
    eb = 2 if kind[0] == BF16 else 1
    t.add(3, T + 37)
    t.add(3, 2 * T + 17, src_off=eb)          # a source one element off: generic
    t.add(2, 33, ndst=2, dscale_off=1)        # a destination scale pointer at offset 1: generic
    t.add(9, T + 37)
    t.add(17, 33, seed=3)
    t.add(3, 31, ndst=2)
    t.add(8, T)
    outs, (total, recs) = t.run()
    t.check(outs)
    alone, (_, recs_alone) = t.run(per_bucket=True)
    for (a, asc), (b, bsc) in zip(t.read(outs), t.read(alone)):
        assert all(np.array_equal(x, y) for x, y in zip(a + asc, b + bsc))
    fams = [r[0] for r in recs]
    if mode == 0:
        assert sorted(recs) == sorted(recs_alone) and FAM_BATCH not in fams
    else:   # the four that run alone first, in bucket order, then one launch per source count
        assert fams[:2] == [FAM_GENERIC, FAM_GENERIC] and FAM_GENERIC not in fams[2:]
        assert recs[-2:] == t.batch_records([3, 3, 8]) and FAM_BATCH not in fams[:-2]
        assert recs[-3][0] == FAM_BLOCKS and recs[-3][3] & 4   # the 17 sources' last, partial-first pass


@pytest.mark.parametrize("case", ["premul-value", "premul-device", "avg", "in-place", "in-place-plain", "empty-middle"])
def test_other_cases(nbx, oracle, torch_gpu, batch_mode, case):
    st, scaled = (BF16, False) if case in ("premul-value", "avg") else (E4M3, case != "in-place-plain")
    fold = ()
    if case.startswith("premul"):
        fold = (PREMULSUM, avg3_bits(oracle), 3)
    elif case == "avg":
        op = nbx.host_to_dev_redop(nbx.ncclRedOp.ncclAvg, F32, 5)   # the fp32 Avg scalar: every source pre-multiplied
        fold = (op.op, op.scalarArg, 5)
    t = Table(nbx, oracle, torch_gpu, st, scaled, E4M3, *fold)
    t.add(5, T + 37, inplace=case.startswith("in-place"))
    t.add(5, 0 if case == "empty-middle" else 33, ndst=2)
    t.add(5, 2 * T + 17, inplace=case.startswith("in-place"))
    outs, (total, recs) = t.run(on_device=case == "premul-device")
    t.check(outs)
    assert (total, recs) == (1, t.batch_records([5] * (2 if case == "empty-middle" else 3)))


def test_graph_capture_and_replay(nbx, oracle, torch_gpu, batch_mode):
    """Two launches captured (3 and 8 MX sources), replayed on new inputs; their slots are the graph's."""
    torch, lib = torch_gpu, nbx.load_library()
    dev_id = torch.cuda.current_device()
    t = Table(nbx, oracle, torch, E4M3, True, E5M2)
    shapes = [(3, T + 37), (8, 33), (3, 2 * T + 17), (8, T)]
    for nsrc, count in shapes:
        t.add(nsrc, count)
    outs, _ = t.run()   # eager first: the arena exists before the capture
    t.check(outs)
    owned0 = lib.nbxDebugBatchListSlots(dev_id, 2)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        nbx.reduce_multi_wide_mx_batch(t.args(outs), E4M3, E5M2, nbx.DevRedOpFull(), 0,
                                       torch.cuda.current_stream().cuda_stream)
    assert lib.nbxDebugBatchListSlots(dev_id, 2) == owned0 + 2
    for seed in (4, 8, 8):
        for b, (nsrc, count) in zip(t.buckets, shapes):
            srcs, scales = t.host(count, nsrc, seed)
            b["exp"] = reference(oracle, srcs, scales, E4M3, E5M2)
            for buf, s in zip(b["sb"] + b["ssb"], srcs + scales):
                buf[0][:s.nbytes].copy_(torch.from_numpy(s.view(np.uint8).copy()))
        for o, osc in outs:
            o[0][0][:o[0][2]].fill_(0xA5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        t.check(outs)
        assert lib.nbxDebugBatchListSlots(dev_id, 2) == owned0 + 2
    del g
    torch.cuda.synchronize()
    assert lib.nbxDebugBatchListSlots(dev_id, 2) in (owned0, owned0 + 2)
