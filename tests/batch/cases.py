"""Case table of the batched-reduce tests, shared by the GPU test
(tests/batch/test_reduce_gpu.py) and its CPU companion
(tests/test_batch_matrix_cpu.py).

kReduceBatch<Fn, NSRC> and kReduceBatchList<Fn, NSRC> (nbx_kernels.h) are one
kernel per (functor, source count) and launch form: 16 of the 52 kernels that
makeKernelSet compiles per functor. Each carries its own tile loop — packs by
ldPack / foldStore, head and tail elements by the scalar pre / red / post of
batchElt — so every (type, op, source count) goes through both forms here with
tests/matrix/inputs.py's edge-rich inputs, against the oracle bit for bit.

Every bucket of a call is a window [start, start + count) of the type's eight
uploads (matrix_inputs, at offset 0 past a 256-byte boundary) and writes the
same window of each of its destination rows: its shared misalignment is
(start * eb) % 16 on every pointer, destinations of different buckets are
disjoint because the windows are, and the expected result is the window of the
oracle's fold of the whole prefix.

In elements: epp = 16 / eb; m = ((3 * eb) % 16 or eb) / eb, the matrix tests'
shared misalignment (3 elements, 1 for 8-byte types); head = epp - m, the
elements in front of the first 16-byte boundary. A tile is 256 packs.

  bucket        start        count                     head  packs  tiles  tail
  one element   0            1                         0     0      1      1
  below a pack  2 epp        max(1, epp - 1)           0     0      1      count
  head only     4 epp + m    head                      head  0      1      0
  clipped head  6 epp + m    max(1, head - 1)          count 0      1      0
  exact tile    8 epp        256 epp                   0     256    1      0
  tile + pack   272 epp + m  head + 257 epp + epp - 1  head  257    2      epp - 1
  ragged        560 epp      589 epp + epp - 1         0     589    3      epp - 1
  empty         1200 epp     0                         (never in a launch)

One element and below a pack: no pack at all, yet the bucket owns a tile whose
workgroup folds the elements. Head only: head = count, nothing behind it.
Clipped head: the host's `head > count` clamp (for 4- and 8-byte types head is
1 and the row equals the one above). Exact tile: the last-tile branch with
neither head nor tail. Tile + pack: head, a full tile, a last tile of one
pack, a tail. Ragged: two full tiles, a 77-pack last tile, a tail. The end is
below 1,150 packs, inside mi.max_count; the empty bucket has valid pointers,
is skipped by the host and is absent from the launch record.

The scheduler shapes (kernarg_walk, list_walk, record_width) are independent
of the functor: they pin kReduceBatch's cursor walk over many records in one
step, kReduceBatchList's 64-wide record search past its first 64 totals, a
chunk of tiles that crosses bucket boundaries and a workgroup's second turn
to sizes that must take them. Their buckets read windows of the same uploads
(sources may overlap between buckets) and write disjoint stretches of a
destination arena of their own, every stretch on its source window's
misalignment and one pack or more away from its neighbours.
"""
import collections

from tests.matrix import inputs as mi

FAM_KERNARG, FAM_LIST = 13, 14          # include/nbx_debug.h nbxDebugLaunchLog
SEGS_SHIFT = 8                           # flags bits 8..: the launch's buckets
MODE_KERNARG, MODE_DEFAULT, MODE_LIST = 0, 1, 2   # nbxDebugSetBatchMode

# restated from nbx_kargs.h
TILE_PACKS = 256                         # kBatchTilePacks
KERNARG_WORDS = (4096 - 40) // 8         # kBatchWords: the table of one kernel-argument launch
KERNARG_MAX_BUCKETS = 16                 # kBatchKernargMaxBuckets: mode 1 keeps sets up to this in kernel arguments
LIST_MAX_RECS = 384                      # kListMaxRecs: buckets per work-list launch
LIST_REC_WORDS_MAX = 20                  # kBatchRecWords
MAX_SRCS = MAX_DSTS = 8

# a bucket: sources' window [start, start + count) of the uploads; the same
# count at element `dstart` of every destination row in `rows`
Bucket = collections.namedtuple("Bucket", "name start count rows dstart")

NAMES = ("one element", "below a pack", "head only", "clipped head", "exact tile", "tile + pack", "ragged", "empty")
LARGE = ("exact tile", "tile + pack", "ragged")


def geometry(eb):
    """(epp, m, head) in elements."""
    epp = 16 // eb
    m = ((3 * eb) % 16 or eb) // eb
    return epp, m, epp - m


def table(eb):
    """[(name, start, count)] of the module docstring's table."""
    epp, m, head = geometry(eb)
    return [("one element", 0, 1),
            ("below a pack", 2 * epp, max(1, epp - 1)),
            ("head only", 4 * epp + m, head),
            ("clipped head", 6 * epp + m, max(1, head - 1)),
            ("exact tile", 8 * epp, 256 * epp),
            ("tile + pack", 272 * epp + m, head + 257 * epp + epp - 1),
            ("ragged", 560 * epp, 589 * epp + epp - 1),
            ("empty", 1200 * epp, 0)]


def claims(eb):
    """{name: (head, packs, tiles, tail)} of the table's last columns."""
    epp, m, head = geometry(eb)
    return {"one element": (0, 0, 1, 1),
            "below a pack": (0, 0, 1, max(1, epp - 1)),
            "head only": (head, 0, 1, 0),
            "clipped head": (max(1, head - 1), 0, 1, 0),
            "exact tile": (0, 256, 1, 0),
            "tile + pack": (head, 257, 2, epp - 1),
            "ragged": (0, 589, 3, epp - 1)}


def packer_geometry(start, count, eb):
    """(head, packs, tiles, tail) of a bucket whose pointers lie start * eb
    bytes past a 16-byte boundary: bucketTiles' arithmetic (nbx_reduce_batch.cc;
    BatchPacker::add and launchBatchList call it)."""
    epp = 16 // eb
    mis = (start * eb) % 16
    head = (16 - mis) // eb if mis else 0
    head = min(head, count)
    packs = (count - head) // epp
    tiles = (packs + TILE_PACKS - 1) // TILE_PACKS or 1   # a bucket below one pack still owns a tile
    return head, packs, tiles, count - head - packs * epp


def table_buckets(eb, ndsts):
    """The table as one call's buckets; ndsts: destinations of the seven
    non-empty buckets, in table order (the empty one takes one)."""
    out = []
    for (name, start, count), nd in zip(table(eb), list(ndsts) + [1]):
        out.append(Bucket(name, start, count, tuple(range(nd)), start))
    return out


def kernarg_launches(buckets, nsrc):
    """Buckets per launch when BatchPacker packs `buckets` (count > 0) of one
    source count: a record is 2 + nsrc + nDsts words and a table is launched
    when the next record does not fit."""
    out, used, n = [], 0, 0
    for b in buckets:
        words = 2 + nsrc + len(b.rows)
        if used + words > KERNARG_WORDS:
            out.append(n)
            used = n = 0
        used += words
        n += 1
    return out + [n] if n else out


def list_launches(n_buckets):
    """Buckets per work-list launch (tile totals far below 2^32)."""
    return [min(LIST_MAX_RECS, n_buckets - i) for i in range(0, n_buckets, LIST_MAX_RECS)]


def records(family, nsrc, launches):
    return [(family, nsrc, 1, n << SEGS_SHIFT) for n in launches]


def tiles_of(buckets, eb):
    return [packer_geometry(b.start, b.count, eb)[2] for b in buckets]


# ---------------------------------------------------------------------------
# scheduler shapes

def place(specs, eb, rows_of=lambda i: (0,)):
    """Buckets from [(name, start, count)]: destination stretches laid out one
    after the other in the arena's rows, each on its source window's offset
    modulo a pack, a pack or more of untouched bytes between neighbours."""
    epp = 16 // eb
    out, pos = [], 0
    for i, (name, start, count) in enumerate(specs):
        dstart = pos + start % epp
        out.append(Bucket(name, start, count, tuple(rows_of(i)), dstart))
        pos = (dstart + count + 2 * epp - 1) // epp * epp
    return out


def arena_elts(buckets, eb):
    return max(b.dstart + b.count for b in buckets) + 16 // eb


def _walk_specs(eb, n, cycle, exact_tail_when_misaligned):
    epp, m, head = geometry(eb)
    specs = []
    for i in range(n):
        tiles = cycle[i % len(cycle)]
        mis = m if i % 3 == 2 else 0
        start = ((37 * i) % 64) * epp + mis
        if mis and exact_tail_when_misaligned:
            # whole tiles of packs behind the head, then a tail: the host's tile
            # count is exact only for the head it recorded (with the head lost,
            # the packs would start `head` elements early and spill one pack
            # past the bucket's tiles)
            count = head + tiles * TILE_PACKS * epp + epp - 1
        else:
            count = tiles * TILE_PACKS * epp - (1 + (5 * i) % (2 * epp + 1))   # a ragged remainder of 1 .. 2 epp + 1
        specs.append((f"bucket {i} ({tiles} tiles{', misaligned' if mis else ''})", start, count))
    return specs


KERNARG_WALK_CYCLE, LIST_WALK_CYCLE = (1, 1, 1, 13), (1, 1, 2, 8)


def kernarg_walk(eb):
    """120 two-source, one-destination buckets (5 words each: 101 per table),
    tile counts cycling (1, 1, 1, 13), every bucket tiles x 256 packs minus a
    ragged remainder, every third misaligned by m. Four records hold 16 tiles,
    so with one workgroup per CU a workgroup's second tile lies CUs / 4 records
    past its first: one cursor step walks dozens of records."""
    buckets = place(_walk_specs(eb, 120, KERNARG_WALK_CYCLE, False), eb)
    assert tiles_of(buckets, eb) == [KERNARG_WALK_CYCLE[i % 4] for i in range(120)]
    return buckets


def list_walk(eb):
    """400 two-source buckets, tile counts cycling (1, 1, 2, 8): 384 in the
    first launch. The first 64 running totals cover 192 tiles, so a workgroup
    whose first chunk starts at or past tile 192 finds no match among them, and
    a workgroup's second turn lies hundreds of records past its first. Chunks
    of 4 tiles cross the one- and two-tile buckets' boundaries."""
    buckets = place(_walk_specs(eb, 400, LIST_WALK_CYCLE, True), eb)
    assert tiles_of(buckets, eb) == [LIST_WALK_CYCLE[i % 4] for i in range(400)]
    return buckets


def record_width(eb):
    """20 eight-source buckets whose destination counts alternate 1 and 8: the
    launch's records are 3 + 8 + 8 = 19 words, the one-destination buckets'
    last seven destination slots padding."""
    epp, m, head = geometry(eb)
    specs = []
    for i in range(20):
        mis = m if i % 3 == 2 else 0
        count = (head if mis else 0) + (1 + 97 * (i % 4)) * epp + (i % epp)
        specs.append((f"bucket {i} ({8 if i % 2 else 1} destinations)", ((11 * i) % 32) * epp + mis, count))
    return place(specs, eb, rows_of=lambda i: range(8 if i % 2 else 1))


def small_set(eb, n, first=0):
    """n small one-destination buckets of a few ragged sizes (launch policy)."""
    epp, m, head = geometry(eb)
    specs = []
    for i in range(first, first + n):
        mis = m if i % 3 == 1 else 0
        specs.append((f"bucket {i}", ((7 * i) % 16) * epp + mis, (head if mis else 0) + (3 + 50 * (i % 5)) * epp + i % epp))
    return specs


def nan_share_of_call(exp, eb, dtype):
    """NaN share of a table call's expected outputs taken together."""
    import numpy as np
    parts = [exp[s:s + c] for _, s, c in table(eb) if c]
    return mi.nan_share(np.concatenate(parts), dtype)
