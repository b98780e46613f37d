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
