/*
 * nbx_reduce.h — internal C ABI of the MI355X reduction core.
 *
 * This is the hot path the library is built around: NCCL's device-side
 * multi-source element-wise reduction ("ReduceOrCopyMulti"),
 *   reduceCopy / reduceCopyPacks   /root/reference/src/device/common_kernel.h:28-239
 *   functors                       /root/reference/src/device/reduce_kernel.h:34-526
 *   one-rank launch                /root/reference/src/device/onerank.cu:48-79
 *   host op encoding               /root/reference/src/enqueue.cc:1436-1512
 * exposed as plain C so that the NCCL API layer, a multi-GPU sharder, a test
 * harness or an emulator can call it with raw device pointers.
 *
 * Semantics of nbxReduceMulti (identical to reduceCopy, common_kernel.h:79-158):
 *   for every element i in [0, count):
 *     acc = pre_0(srcs[0][i])
 *     for s = 1 .. nSrcs-1:  acc = Fn(acc, pre_s(srcs[s][i]))    (ordered left fold)
 *     if postOp:             acc = post(acc)
 *     for d in dsts:         dsts[d][i] = acc
 *   where pre_s is the PreMulSum pre-multiply for s < nPreOpSrcs (identity
 *   otherwise) and post is the SumPostDiv integer divide.
 */
#ifndef NBX_REDUCE_H_
#define NBX_REDUCE_H_

#include "nccl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device reduction opcode — /root/reference/src/include/device.h:26-30 (same order). */
typedef enum {
  nbxDevSum = 0,
  nbxDevProd = 1,
  nbxDevMinMax = 2,
  nbxDevPreMulSum = 3,
  nbxDevSumPostDiv = 4,
  nbxNumDevRedOps = 5
} nbxDevRedOp_t;

/* Full device op — /root/reference/src/include/device.h:31-36 (ncclDevRedOpFull).
 * scalarArg: MinMax xormask, PreMulSum scalar bits (element type, low bytes),
 * SumPostDiv divisor. If scalarArgIsPtr, scalarArg is a device address of the
 * PreMulSum scalar, dereferenced by the kernel while it runs (ncclScalarDevice,
 * common.h:100-119 / onerank.cu:32-42). */
typedef struct {
  int32_t op;             /* nbxDevRedOp_t */
  int32_t scalarArgIsPtr; /* bool */
  uint64_t scalarArg;
} nbxDevRedOpFull;

#define NBX_MAX_SRCS 64   /* > 8 sources run as ordered multi-pass folds (one source per rank up to 64) */
#define NBX_MAX_DSTS 8    /* NCCL_MAX_DIRECT_ARITY + 1 (device.h:147): local output + 7 peers */

/* Host-side op encoding: replaces hostToDevRedOp, enqueue.cc:1436-1512, for
 * the built-in ops (Sum/Prod/Max/Min/Avg). nRanks feeds ncclAvg. */
ncclResult_t nbxHostToDevRedOp(nbxDevRedOpFull* out, ncclRedOp_t op,
                               ncclDataType_t datatype, int nRanks);

/* The reduction core: replaces reduceCopy<...>(...) (common_kernel.h:183-239)
 * plus its kernel shell (onerank.cu:14-45, common.h:121-210).
 * Stream-ordered and asynchronous; returns once the kernel is enqueued.
 * count == 0 is a no-op. Any pointer alignment is accepted (16-B packs when
 * the pointers share one alignment, element packs otherwise — common_kernel.h:209-238).
 * Errors: ncclInvalidArgument for nSrcs outside [1, NBX_MAX_SRCS], nDsts
 * outside [1, NBX_MAX_DSTS], a NULL pointer with count > 0, a bad datatype,
 * op or op/type combination (SumPostDiv on floats: reduce_kernel.h:506-509);
 * ncclUnhandledCudaError if the launch fails. */
ncclResult_t nbxReduceMulti(void* const* dsts, int nDsts,
                            const void* const* srcs, int nSrcs,
                            size_t count, ncclDataType_t datatype,
                            nbxDevRedOpFull op, int nPreOpSrcs, int postOp,
                            ncclStream_t stream);

/* fp32-accumulating ("wide") form of the sum, for low-precision sources:
 * every source is widened once, the fold runs in fp32, and the result is
 * narrowed once or not at all. This is NOT the reference's rule (which
 * nbxReduceMulti keeps: the accumulator is rounded to the element type after
 * every source, so 1.0 + 7 x 2^-9 in bf16 stays 1.0); it is opt-in.
 *   for every element i in [0, count):
 *     acc = f32(srcs[0][i]);                 if 0 < nPreOpSrcs: acc = acc * s
 *     for k = 1 .. nSrcs-1:  v = f32(srcs[k][i]);  if k < nPreOpSrcs: v = v * s;  acc = acc + v
 *     every dsts[d][i] = (dstType == ncclFloat32) ? acc : narrow(acc)
 * f32() is exact; every multiply and add is one IEEE fp32 round-to-nearest-even
 * operation (never fused, denormals kept), folded in source order, so the
 * result is deterministic. narrow() is the type's narrowing applied once:
 * RNE for f16 / bf16 (f16 overflow -> inf), RNE behind SATFINITE for fp8
 * (finite overflow -> +-max finite; inf and NaN as in nbxReduceMulti).
 * srcType: ncclFloat16, ncclBfloat16, ncclFloat8e4m3, ncclFloat8e5m2.
 * dstType: srcType, or ncclFloat32 (all destinations share it).
 * op: nbxDevSum or nbxDevPreMulSum. The PreMulSum scalar s is an FP32 value
 * whatever srcType is: by value the low 32 bits of scalarArg, or with
 * scalarArgIsPtr the device address of a float (non-NULL, 4-byte aligned),
 * read while the kernel runs. nbxHostToDevRedOp(&op, ncclAvg, ncclFloat32, n)
 * therefore yields the wide average. Prod, MinMax (already exact through
 * nbxReduceMulti) and SumPostDiv: ncclInvalidArgument.
 * Limits and errors as nbxReduceMulti, every check before any device call;
 * count == 0 is a no-op after the type and op checks. Pointers are aligned to
 * their own element size. A destination of srcType may be one of the sources
 * (in place); an fp32 destination whose range overlaps any source range is
 * ncclInvalidArgument. 16-byte packs when the sources share one misalignment
 * modulo 16 and every destination is 16-byte aligned behind the head elements
 * that align them (an fp32 destination: (dst + 4 * head) % 16 == 0). Any other
 * layout whose destinations share one address modulo 16 — sources on
 * misalignments of their own, such as the blocks of a reduce-scatter whose
 * count is no multiple of a pack — runs the realigning kernel from
 * NBX_WIDE_SHIFT_MIN_ELTS elements (default 2097152, the measured crossover):
 * 16-byte packs on the destinations' side, the sources staged through LDS by
 * LDS-DMA and realigned on the way out, 2.3-8.0 times the element rate and
 * 85-113 % of the pack rate at 256 MiB per input. Destinations on different
 * alignments, and shorter calls, run one element per lane. The result is the
 * same bits whichever kernel runs. More than 8 sources fold in ordered passes
 * through an fp32 partial
 * (dsts[0] for an fp32 output, else stream-ordered scratch of 4 * count
 * bytes), so the result is still the single fp32 left fold.
 * Stream-ordered, asynchronous and graph-capturable. */
ncclResult_t nbxReduceMultiWide(void* const* dsts, int nDsts,
                                const void* const* srcs, int nSrcs,
                                size_t count, ncclDataType_t srcType,
                                ncclDataType_t dstType, nbxDevRedOpFull op,
                                int nPreOpSrcs, ncclStream_t stream);

/* The same sum inside the collectives: an operator for ncclAllReduce /
 * ncclReduceScatter / ncclReduce on `comm`:
 * base = ncclSum or ncclAvg over `datatype` (fp16, bf16, fp8 e4m3 / e5m2),
 * accumulated in fp32 and narrowed once. Destroyed with ncclRedOpDestroy.
 * Every rank's input is widened once, the inputs are added in fp32 in the
 * direct schedule's operand order (block b of an AllReduce or ReduceScatter:
 * ranks b+1, ..., b; a Reduce: root+1, ..., root) and the result is narrowed
 * once: nbxReduceMultiWide's arithmetic over those sources, bit for bit, where
 * the per-step operators round to `datatype` after every rank (the reference's
 * rule). ncclAvg multiplies EVERY input by the fp32 scalar of
 * nbxHostToDevRedOp(&op, ncclAvg, ncclFloat32, nRanks) before the adds. The
 * bytes between the ranks are today's: every direct schedule (LL, LL128 one-
 * and two-shot, direct Simple, the in-process clique's fold) moves raw inputs,
 * and only the fold differs. The protocol is chosen as for any call. The ring
 * schedule moves partials of `datatype`, so on a communicator created with
 * NCCL_ALGO=Ring a Simple-sized wide call runs the direct schedule — every
 * rank decides that from the operator all ranks pass alike. At one rank the
 * result is the input. The handle lives in the communicator's user-operator
 * table like a PreMulSum handle: ncclRedOpDestroy frees it, a call with
 * another datatype is ncclInvalidArgument, its state is copied at enqueue, and
 * calls with it can be captured in a graph as per-step calls can.
 * ncclInvalidArgument for a NULL op or comm, a base other than ncclSum /
 * ncclAvg (a user handle included), a datatype outside the four.
 * NBX_WIDE_ACCUM=1 at communicator creation (equal on every rank) gives the
 * built-in ncclSum / ncclAvg on the four types this operator on that
 * communicator, for programs that cannot call a new function; unset or 0,
 * nothing changes.
 * Not provided: a wide PreMulSum with per-rank scalars (each rank's scalar
 * would have to travel with its input), an fp32 output, Prod / Min / Max
 * (Min / Max are exact already), a wide ring schedule. */
ncclResult_t nbxRedOpCreateWide(ncclRedOp_t* op, ncclRedOp_t base,
                                ncclDataType_t datatype, ncclComm_t comm);

/* One bucket of a batched reduction (same meaning as nbxReduceMulti's arguments). */
typedef struct {
  void* const* dsts;
  int nDsts;
  const void* const* srcs;
  int nSrcs;
  size_t count;
} nbxReduceTask;

/* Batched form: nTasks independent buckets with one datatype and op, as if
 * nbxReduceMulti were called for each — the analogue of NCCL packing grouped
 * collectives into one kernel's work list (enqueue.cc:67-91
 * appendWorkElemColl, NCCL_MAX_WORK_ELEMENTS, device.h:230). Buckets with the
 * same source count (<= 8) and one shared pointer alignment run together
 * (46 to 101 single-destination buckets per launch, from 8 down to 2
 * sources), their tiles in one index space, so many small buckets fill the
 * GPU like one large one; large buckets of 3+ sources, > 8 sources or mixed
 * alignments run as single-bucket launches. Buckets must be independent: no bucket's destinations
 * may overlap another bucket's sources or destinations (they may run
 * concurrently, in any order). Every bucket is checked before anything is
 * enqueued; errors as nbxReduceMulti (nTasks < 0 or tasks == NULL with
 * nTasks > 0: ncclInvalidArgument). nTasks == 0 is a no-op. */
ncclResult_t nbxReduceMultiBatch(const nbxReduceTask* tasks, int nTasks,
                                 ncclDataType_t datatype, nbxDevRedOpFull op,
                                 int nPreOpSrcs, int postOp, ncclStream_t stream);

/* Batched form of nbxReduceMultiWide: nTasks independent buckets with one
 * source type, destination type and op, as if nbxReduceMultiWide(t.dsts,
 * t.nDsts, t.srcs, t.nSrcs, t.count, srcType, dstType, op, nPreOpSrcs, stream)
 * were called for every bucket t — the same arithmetic (exact widening, one
 * unfused fp32 multiply or add per step in source order, denormals kept, one
 * narrowing or an fp32 store), so the results are bit-identical to the
 * per-bucket calls for every layout. Buckets of <= 8 sources whose layout
 * nbxReduceMultiWide's pack kernel takes (sources on one misalignment modulo
 * 16, every destination 16-byte aligned behind the head elements) run
 * together from a work-list table, up to 384 per launch and one launch series
 * per source count; every other bucket (mixed layouts, > 8 sources, 4+
 * sources large enough to fill the GPU alone, launch variant 2) and any bucket
 * that got no table slot runs as its own nbxReduceMultiWide launch — the
 * realigning kernel where that call would take it, the element kernel
 * otherwise; the work-list table stays pack-layout only — and nothing
 * waits for a slot. Buckets must be independent, as for nbxReduceMultiBatch;
 * a destination of srcType may be one of its own bucket's sources.
 * Type, op and scalar checks as nbxReduceMultiWide, made even for nTasks ==
 * 0 (then a no-op); nTasks < 0 or tasks == NULL with nTasks > 0:
 * ncclInvalidArgument. Every bucket is checked (counts, NULL pointers, element
 * alignment, an fp32 destination overlapping one of its own sources) before
 * anything is enqueued and before any device call; buckets of count 0 are
 * skipped, the pointers in their arrays unexamined, as in the single call.
 * Stream-ordered, asynchronous and graph-capturable. */
ncclResult_t nbxReduceMultiWideBatch(const nbxReduceTask* tasks, int nTasks,
                                     ncclDataType_t srcType, ncclDataType_t dstType,
                                     nbxDevRedOpFull op, int nPreOpSrcs, ncclStream_t stream);

/* Statistics of a bucket the fp32-accumulating sum has just produced, taken
 * from the fold's registers: no second pass over the fp32 masters. */
typedef struct {
  double   sumSq;     /* sum over i of acc_i * acc_i */
  float    amax;      /* max over i of |acc_i|, NaN > +inf > every finite value */
  uint32_t reserved;  /* written as 0 */
} nbxWideStats;       /* 16 bytes, 8-byte aligned, DEVICE memory */

/* nbxReduceMultiWide that also writes *stats (device memory, overwritten, never
 * accumulated into). acc_i is element i's final fp32 accumulator BEFORE the
 * narrowing: the value nbxReduceMultiWide narrows, or stores for an fp32
 * output. The destinations receive the bits nbxReduceMultiWide gives with the
 * same arguments: every layout, up to NBX_MAX_SRCS sources, in place.
 *   amax   exact and order-independent, numpy.max(numpy.abs(acc)): a NaN if
 *          any acc_i is NaN, else +inf if any is +-inf, else the largest
 *          |acc_i| (+0.0 for an all-zero bucket). An fp16 output that
 *          overflows on narrowing still reports the finite magnitude.
 *   sumSq  NaN if any acc_i is NaN, else +inf if any is inf; else the exact
 *          sum of acc_i^2 within a relative L * 2^-24, L = 32. L counts the
 *          fp32 roundings on the longest path into one fp64 partial: a lane
 *          squares and adds with one fma (one rounding) per element into two
 *          fp32 sums, one per half of an accumulator pair, for the length of
 *          one tile, and a tile is at most 4 packs per lane of 16 fp8 elements
 *          (4+ sources): 4 x 16 / 2 = 32 per sum. 16-bit sources reach 16, the
 *          realigning kernel 8 / 16, the element kernel and every head or tail
 *          element 8 or fewer, a batched bucket 4 / 8. Everything above a
 *          tile is added in fp64 (a few dozen adds on any path: negligible
 *          against L * 2^-24). The bound holds while the true sum is
 *          below 2^120 — above that a lane's fp32 sum may overflow and sumSq
 *          be +inf — and for accumulators whose squares are normal fp32
 *          numbers (|acc_i| >= 2^-63; smaller squares round to fp32 denormals
 *          or to zero, an absolute 2^-150 each).
 * Reproducible: the statistics are a function of the arguments and of the
 * kernel family and its tile shape alone — not of the grid (nbxSetLaunchConfig
 * blocksPerCU), the CU count, the static or dynamic tile schedule, or which
 * workgroup ran which tile. Every tile's waves write one 16-byte partial each
 * to a slot indexed by tile and wave (stream-ordered scratch, 16 bytes per 64
 * to 4096 elements), and a second, small kernel sums the slots in a tree fixed
 * by the slot index. Two identical calls give identical bits.
 * count == 0 writes {0, 0, 0}. More than 8 sources: only the last pass
 * contributes (nothing of the intermediate fp32 partial).
 * Checks as nbxReduceMultiWide, and stats == NULL or not 8-byte aligned:
 * ncclInvalidArgument; every check before any device call.
 * Stream-ordered, asynchronous and graph-capturable.
 * Not provided: statistics inside ncclAllReduce / ncclReduceScatter /
 * ncclReduce, for the per-step nbxReduceMulti, and a host-staged form. */
ncclResult_t nbxReduceMultiWideStats(void* const* dsts, int nDsts,
                                     const void* const* srcs, int nSrcs,
                                     size_t count, ncclDataType_t srcType,
                                     ncclDataType_t dstType, nbxDevRedOpFull op,
                                     int nPreOpSrcs, nbxWideStats* stats,
                                     ncclStream_t stream);

/* nbxReduceMultiWideBatch that also writes stats[k] for every bucket k
 * (nTasks entries, overwritten), as if nbxReduceMultiWideStats were called per
 * bucket: the same destinations, the same definitions and bound; an empty
 * bucket's record is {0, 0, 0}. A bucket that runs as its own launch (mixed
 * layout, > 8 sources, no table slot) takes the single call's kernels, so its
 * sumSq may differ from the batched kernel's in the last bits (another tile
 * shape); amax never does. Checks as nbxReduceMultiWideBatch; stats == NULL
 * with nTasks > 0, or not 8-byte aligned: ncclInvalidArgument. */
ncclResult_t nbxReduceMultiWideBatchStats(const nbxReduceTask* tasks, int nTasks,
                                          ncclDataType_t srcType, ncclDataType_t dstType,
                                          nbxDevRedOpFull op, int nPreOpSrcs,
                                          nbxWideStats* stats, ncclStream_t stream);

/* MXFP8 block-scaled form of nbxReduceMultiWide (OCP microscaling, MX v1.0):
 * 32-element blocks of fp8 codes with one E8M0 power-of-two scale byte each,
 * as a destination, as the sources, or both. The fold is nbxReduceMultiWide's,
 * bit for bit: every source widened exactly, one unfused fp32 multiply or add
 * per step in source order, denormals kept, more than 8 sources in passes
 * through an fp32 partial that is never narrowed.
 * Blocks: block b is elements [32 b, 32 b + 32) of the bucket, counted from
 * element 0 whatever the pointers' alignment; the last block holds count % 32
 * elements when that is not 0. A scale array has ceil(count / 32) bytes.
 * MX sources (srcScales != NULL, every entry non-NULL, srcType ncclFloat8e4m3
 * or ncclFloat8e5m2): element i of source k is f32(code) * X, one fp32
 * multiply, X = 2^(e - 127) for the scale byte e of its block (e = 0: the fp32
 * denormal 2^-127; e = 0xFF: a NaN); the PreMulSum multiply (k < nPreOpSrcs)
 * comes after it. srcScales == NULL: plain f16 / bf16 / fp8 sources.
 * MX output (dstType ncclFloat8e4m3 or ncclFloat8e5m2, dstScales and every
 * dstScales[d] non-NULL; dstType need not be srcType): with emax = 8 (e4m3) or
 * 15 (e5m2) and m = max |a_i| over the block's final accumulators under
 * nbxWideStats' amax rule (NaN if any a_i is NaN, else +inf if any is +-inf),
 *   m finite:  the scale byte is S = max(be - emax, 0), be the biased exponent
 *              field of m as fp32 (0 for zero and denormals) — MX v1.0's
 *              floor(log2 m) - emax, biased by 127 and clamped at -127 — and
 *              element i is narrow(a_i * R), R = 2^(127 - S) as fp32: one fp32
 *              multiply, then the type's RNE-behind-SATFINITE narrowing (e4m3:
 *              scaled values in (464, 512) store 448). An all-zero block has
 *              scale byte 0 and keeps its signed zeros.
 *   otherwise: the scale byte is 0xFF (MX's NaN block) and element i is
 *              narrow(a_i), unscaled: the non-finite positions stay visible.
 * The multiply by R is exact except where the product falls below 2^-126, and
 * such a value narrows to +-0 whether it was rounded or flushed: the stored
 * bits are a function of the arguments alone, whichever kernel runs.
 * fp32 output (dstType ncclFloat32, dstScales NULL): the accumulators as they
 * are; only with MX sources (plain sources into fp32 is nbxReduceMultiWide:
 * here ncclInvalidArgument).
 * op: nbxDevSum or nbxDevPreMulSum with the fp32 scalar of nbxReduceMultiWide
 * (by value or by device pointer); everything else ncclInvalidArgument. Every
 * check of nbxReduceMultiWide applies, and every check is made before any
 * device call; count == 0 is a no-op after the type and op checks. Element
 * pointers are aligned to their element size, scale pointers to nothing.
 * Overlap: a destination's element buffer may be one of the sources only when
 * srcType == dstType, and if that source carries scales the destination's
 * scale array must be that source's; any other overlap between a destination
 * (elements or scales) and a source (elements or scales), or between the two
 * arrays of one destination, is ncclInvalidArgument.
 * Every element pointer 16-byte aligned and every destination scale pointer
 * 4-byte aligned runs the block kernel (a lane pair per block, the scale bytes
 * stored as dwords); any other layout one element per lane. Same bits.
 * Stream-ordered, asynchronous and graph-capturable.
 *
 * MXFP4 (OCP E2M1) elements: NBX_FLOAT4_E2M1 as srcType, dstType or both, a tag
 * only this function accepts. An FP4 buffer holds ceil(count / 2) bytes:
 * element 2 j is the low nibble of byte j, element 2 j + 1 the high nibble;
 * element 0 is always a low nibble, so the pointer is byte-aligned. For an odd
 * count a destination's last high nibble is stored as 0 and a source's is
 * ignored. A code is a sign (bit 3) over the magnitudes 0, 0.5, 1, 1.5, 2, 3,
 * 4, 6 (codes 0 - 7). Blocks and scale arrays are as above.
 *   ncclFloat16 / ncclBfloat16 sources (srcScales NULL) into MXFP4 (dstScales
 *     given);
 *   MXFP4 sources (srcScales and every entry non-NULL) into MXFP4, or into
 *     fp32 (dstScales NULL).
 * An MXFP4 source element is f32(code) * X with the X above (exact for every
 * code and finite scale), the PreMulSum multiply after it. The fold is the
 * same. MXFP4 output follows the MX output rule with emax = 2: for finite m,
 * S = max(be - 2, 0), R = 2^(127 - S), and element i is narrow4(a_i * R): one
 * fp32 multiply, then round-to-nearest-even onto the eight magnitudes (the
 * ties 0.25, 1.25, 2.5 and 5 round down, 0.75, 1.75 and 3.5 up), everything
 * above 6 stored as +-6 (the scaled maximum lies in [4, 8), so (6, 8)
 * saturates, as e4m3's (464, 512)), the sign kept: -0 is 0x8 and magnitudes
 * below 0.25 give +-0. The type has no NaN or inf code: for a non-finite m the
 * scale byte is 0xFF and EVERY code of the block is 0, and a reader — this
 * function included — takes every element of a 0xFF block as NaN.
 * Overlap as above with ceil(count / 2) as an FP4 array's size; in place only
 * MXFP4 into MXFP4, on the source's own scale array. The block kernel (a lane
 * quad per block) needs the same alignments; any other layout runs one FP4
 * byte per lane. Same bits.
 *
 * MXFP6 (OCP E2M3 / E3M2) elements: NBX_FLOAT6_E2M3 or NBX_FLOAT6_E3M2 as
 * srcType, dstType or both, tags only this function accepts. A code is 6 bits,
 * a sign in bit 5 over a 5-bit magnitude; neither type has an inf or NaN code.
 *   E2M3: exponent in bits 4:3 (bias 1), mantissa m in bits 2:0. Exponent
 *     field 0: m / 8; else (1 + m / 8) * 2^(e - 1). Largest 7.5 (0x1F), emax 2.
 *   E3M2: exponent in bits 4:2 (bias 3), mantissa m in bits 1:0. Exponent
 *     field 0: m / 16; else (1 + m / 4) * 2^(e - 3). Largest 28 (0x1F), emax 4.
 * An FP6 buffer is a dense little-endian bit stream of ceil(3 * count / 4)
 * bytes: element i occupies bits [6 i, 6 i + 6), so four elements c0..c3 are
 * the three bytes b0 = c0 | c1 << 6, b1 = c1 >> 2 | c2 << 4, b2 = c2 >> 4 |
 * c3 << 2 (each truncated to 8 bits). Element 0 starts at bit 0, so the pointer
 * is byte-aligned. The unused high bits of a destination's last byte are
 * stored as 0, those of a source's last byte are ignored. Blocks and scale
 * arrays are as above: block b is elements [32 b, 32 b + 32), 24 bytes when
 * full, and a scale array has ceil(count / 32) bytes.
 *   ncclFloat16 / ncclBfloat16 sources (srcScales NULL) into MXFP6 of either
 *     type (dstScales given);
 *   MXFP6 sources (srcScales and every entry non-NULL) into MXFP6 of the same
 *     type, or into fp32 (dstScales NULL).
 * An MXFP6 source element is f32(code) * X with the X above (one fp32
 * multiply; a 0xFF block is NaN), the PreMulSum multiply after it. The fold is
 * the same. MXFP6 output follows the MX output rule with the type's emax (2
 * for E2M3, 4 for E3M2): for finite m, S = max(be - emax, 0), R = 2^(127 - S),
 * and element i is narrow6(a_i * R): one fp32 multiply, then
 * round-to-nearest-even onto the type's grid, subnormals included. Every
 * magnitude above the largest stores the largest, a tie that would round up
 * past it too: E2M3 everything above 7.5, so (7.5, 8) saturates; E3M2
 * everything above 28, so (28, 32) saturates. The sign is kept: -0 is 0x20,
 * and magnitudes that round to zero keep their sign. For a non-finite m the
 * scale byte is 0xFF and EVERY code of the block is 0, as for MXFP4. The stored
 * bits are a function of the arguments alone, whichever kernel runs.
 * Overlap as above with ceil(3 * count / 4) as an FP6 array's size; in place
 * only MXFP6 into the same type, on the source's own scale array. count == 0
 * is a no-op after the type and op checks. The block kernel (a block per lane
 * at the converters, nbx_mx6.h) needs the same alignments; any other layout
 * runs four elements (three bytes) per lane. Same bits.
 * Not provided (ncclInvalidArgument): E2M3 <-> E3M2, FP6 <-> FP8 / FP4 pairs;
 * FP6 sources without scales; fp8 sources, plain or MX, into
 * MXFP4; MXFP4 sources into MXFP8; MXFP4 sources without scales; block sizes
 * other than 32; blocks down the columns of a 2-D bucket (MXFP8 has them:
 * nbxReduceMultiWideMx2d); a batched form of MXFP4 or MXFP6 (MXFP8 has one:
 * nbxReduceMultiWideMxBatch), a statistics form, a form inside the
 * collectives, a host-staged form, a realigning LDS-DMA form. */
#define NBX_FLOAT4_E2M1 ((ncclDataType_t)32)
#define NBX_FLOAT6_E2M3 ((ncclDataType_t)33)
#define NBX_FLOAT6_E3M2 ((ncclDataType_t)34)
ncclResult_t nbxReduceMultiWideMx(void* const* dsts, void* const* dstScales, int nDsts,
                                  const void* const* srcs, const void* const* srcScales, int nSrcs,
                                  size_t count, ncclDataType_t srcType, ncclDataType_t dstType,
                                  nbxDevRedOpFull op, int nPreOpSrcs, ncclStream_t stream);

/* One bucket of nbxReduceMultiWideMxBatch: nbxReduceMultiWideMx's arrays and
 * count. dstScales is NULL for an fp32 output, srcScales for plain sources. */
typedef struct {
  void* const* dsts;        void* const* dstScales;        int nDsts;
  const void* const* srcs;  const void* const* srcScales;  int nSrcs;
  size_t count;
} nbxReduceMxTask;

/* Batched form of nbxReduceMultiWideMx for MXFP8: behaves as if
 * nbxReduceMultiWideMx(t.dsts, t.dstScales, t.nDsts, t.srcs, t.srcScales,
 * t.nSrcs, t.count, srcType, dstType, op, nPreOpSrcs, stream) were called for
 * every bucket t, in far fewer launches; the results are the same bits for
 * every layout. Buckets in the block kernel's layout (every element pointer
 * 16-byte aligned, every destination scale pointer 4-byte aligned) with at
 * most 8 sources share work-list launches per source count, up to 384 buckets
 * each (fewer for wide records: 219 for 8 scaled sources and 8 MX
 * destinations), tiles of 4096 elements in one index space; every other
 * bucket — any other layout, more than 8 sources, 4+ sources filling the GPU
 * alone, no table slot left — is one nbxReduceMultiWideMx launch.
 * Types: the six source kinds of nbxReduceMultiWideMx's MXFP8 form (f16, bf16,
 * e4m3, e5m2 plain; e4m3, e5m2 with scales) into MX e4m3, MX e5m2 and, for
 * scaled sources, fp32. NBX_FLOAT4_E2M1 on either side: ncclInvalidArgument.
 * Scaled or plain is a property of the call: every task's srcScales is NULL or
 * every task's is non-NULL, empty buckets included; a mixture is
 * ncclInvalidArgument, and so is a task whose dstScales does not suit dstType.
 * Checks: the type, op and scalar checks of nbxReduceMultiWideMx, made even
 * for nTasks == 0 (then a no-op); nTasks < 0 or tasks == NULL with nTasks > 0:
 * ncclInvalidArgument. Every bucket gets every check of the single call
 * (counts of pointers, NULL entries, element alignment, the overlap rules, in
 * place only with equal types on the source's own scale array) before
 * anything is enqueued and before any device call; buckets of count 0 are
 * skipped, the entries of their arrays unexamined, as in the single call.
 * Buckets must be independent of each other, scale arrays included: no
 * bucket's destination or destination scales may overlap anything another
 * bucket reads or writes (the caller's contract, as for
 * nbxReduceMultiWideBatch; not checked).
 * Stream-ordered, asynchronous and graph-capturable: a table written during
 * capture belongs to the graph until it is destroyed. Nothing ever waits for a
 * table slot.
 * Not provided: MXFP4 in the batch, statistics, a kernel-argument form. */
ncclResult_t nbxReduceMultiWideMxBatch(const nbxReduceMxTask* tasks, int nTasks,
                                       ncclDataType_t srcType, ncclDataType_t dstType,
                                       nbxDevRedOpFull op, int nPreOpSrcs, ncclStream_t stream);

/* 2-D form of nbxReduceMultiWideMx for MXFP8: one fold of a matrix, stored with
 * blocks down the columns and, when asked, along the rows too — the two
 * quantised copies a consumer keeps of a matrix it contracts along either
 * dimension — with the sources read once.
 * Bucket: a dense row-major rows x cols matrix; element (r, c) is flat element
 * r * cols + c and count = rows * cols.
 * Fold: nbxReduceMultiWideMx's over the flat bucket, bit for bit: sources
 * widened exactly, each step one unfused fp32 multiply or add in source order
 * with denormals kept, the PreMulSum scalar by value or by device pointer, more
 * than 8 sources in passes through an fp32 partial that is never narrowed.
 * Column-wise output (colDsts, colScales: required, nDsts entries each, all
 * non-NULL): block (i, c) is rows [32 i, 32 i + 32) of column c; the last block
 * row holds rows % 32 rows when that is not 0. colDsts[d] has the bucket's own
 * row-major layout, one fp8 code per element; colScales[d] is row-major
 * ceil(rows / 32) x cols, the byte of block (i, c) at i * cols + c. Scale byte
 * and codes follow the MX output rule above unchanged: m under the amax rule,
 * S = max(be - emax, 0), R = 2^(127 - S), each code narrow(a * R); a non-finite
 * m gives scale byte 0xFF and unscaled narrowing.
 * Row-wise output (rowDsts, rowScales: both NULL, or both given with nDsts
 * non-NULL entries): block (r, j) is columns [32 j, 32 j + 32) of row r; the
 * last block of a row holds cols % 32 columns. rowScales[d] is row-major
 * rows x ceil(cols / 32). When cols % 32 == 0 the row-wise codes and scales
 * are exactly nbxReduceMultiWideMx's output for count = rows * cols.
 * Types: sources f16, bf16, e4m3 or e5m2 plain (srcScales NULL), or e4m3 / e5m2
 * with scales; output MX e4m3 or MX e5m2 (dstType need not equal srcType).
 * Scaled sources carry the flat 1-D scale arrays of nbxReduceMultiWideMx and
 * require cols % 32 == 0, so a row-wise output of this function or of the 1-D
 * one feeds straight back in; scaled sources with another cols are
 * ncclInvalidArgument. Not provided (ncclInvalidArgument): FP4 / FP6 tags, an
 * fp32 output, column-scaled sources, in place.
 * Checks, every one before any device call: the type, op and scalar checks of
 * nbxReduceMultiWideMx; nSrcs in [1, NBX_MAX_SRCS], nDsts in [1, NBX_MAX_DSTS];
 * NULL entries; element alignment to the element size; rows * cols must not
 * overflow size_t. rows == 0 or cols == 0 is a no-op after the type and op
 * checks. Any overlap is ncclInvalidArgument: any written array (codes or
 * scales, row or column) against any source array (elements or scales), and any
 * two written arrays against each other. There is no in-place form: the
 * any-layout kernel reads the sources twice.
 * Every element pointer 16-byte aligned, cols % 16 == 0 and every destination
 * scale pointer 4-byte aligned runs the tile kernel (a workgroup per 32 x 128
 * tile, the accumulators in registers across one barrier, every source byte
 * read once); any other layout runs a column per lane and reads the sources
 * twice. Same bits. Stream-ordered, asynchronous and graph-capturable.
 * Not provided: FP4 / FP6 elements, a batched form, a statistics form. */
ncclResult_t nbxReduceMultiWideMx2d(void* const* rowDsts, void* const* rowScales,
                                    void* const* colDsts, void* const* colScales, int nDsts,
                                    const void* const* srcs, const void* const* srcScales, int nSrcs,
                                    size_t rows, size_t cols,
                                    ncclDataType_t srcType, ncclDataType_t dstType,
                                    nbxDevRedOpFull op, int nPreOpSrcs, ncclStream_t stream);

/* Host-staged form of nbxReduceMulti: sources and destinations in HOST memory
 * (pinned for full speed; pageable works), the path NCCL's NET/SHM transports
 * stage through (host-pinned proxy FIFOs net.cc:735/883, /dev/shm buffers
 * shm.cc:86-114) — where an emulator's proxy/net buffers live. Data is chunked
 * (NBX_HOST_CHUNK_BYTES per source, default 16 MiB) through a two-slot device
 * staging ring so H2D, the reduction and D2H of consecutive chunks overlap.
 * When every buffer is pinned and device-mapped (hipHostMalloc /
 * hipHostRegister), the kernel instead reads and writes them in place over
 * PCIe (zero-copy; env NBX_HOST_MODE=auto|staged|zerocopy, zerocopy on
 * pageable memory: ncclInvalidArgument).
 * Ordered after prior work on `stream`; BLOCKING: returns when every host
 * destination holds the result. Same semantics and errors as nbxReduceMulti. */
ncclResult_t nbxReduceMultiHost(void* const* hostDsts, int nDsts,
                                const void* const* hostSrcs, int nSrcs,
                                size_t count, ncclDataType_t datatype,
                                nbxDevRedOpFull op, int nPreOpSrcs, int postOp,
                                ncclStream_t stream);

/* Launch knobs (NCCL_NTHREADS / NCCL_MAX_NCHANNELS analogues, tuning.cc:12,
 * connect.cc:314): blocksPerCU caps the grid at CUs x blocksPerCU workgroups
 * (0 = default: 1 for big tiles, 3-5 for small; env NBX_BLOCKS_PER_CU);
 * variant 0 = auto tile choice, 1 = force small tiles (and, for sources
 * misaligned against the destinations, the 1-pack run-time-source-count
 * realigning kernel), 2 = force big tiles. */
ncclResult_t nbxSetLaunchConfig(int blocksPerCU, int variant);
ncclResult_t nbxGetLaunchConfig(int* blocksPerCU, int* variant);

/* Number of (datatype, device op) kernel sets compiled in (for the ABI test). */
int nbxKernelCount(void);

/* Version of the core ABI (bumped on incompatible changes). */
int nbxAbiVersion(void);

#ifdef __cplusplus
}
#endif

#endif /* NBX_REDUCE_H_ */
