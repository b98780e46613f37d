/*
 * nbx_debug.h — test hooks of libnbxccl.so (no GPU needed).
 */
#ifndef NBX_DEBUG_H_
#define NBX_DEBUG_H_

#include <stdint.h>

#include "nccl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Connects rank `rank` of `nranks` to the bootstrap root named by `id` (from
 * ncclGetUniqueId) and runs `rounds` allgathers of rank-stamped payloads of
 * varying length, verifying every contribution. Exercises the host bootstrap
 * that multi-process ncclCommInitRank uses (the role of src/bootstrap.cc). */
ncclResult_t nbxBootstrapSelfTest(const ncclUniqueId* id, int rank, int nranks, int rounds);

/* The Simple protocol's kernels (direct schedule, or ring when `ring`) for n
 * "ranks" driven from ONE process on the current device: staging, flag words and
 * counters laid out as ncclCommInitRank lays them out, every rank's kernel on
 * its own stream, all n launches of a call running together (n x gridMax
 * workgroups must fit the GPU at once). kind 0 AllReduce, 1 ReduceScatter
 * (count = recvcount), 2 Reduce (to `root`); sends[r] / recvs[r] are rank r's
 * device buffers (recvs[r] may be NULL on Reduce non-roots). Runs one untimed
 * and `iters` timed calls; *msPerCall = mean device time per call. Returns an
 * ncclResult_t (ncclRemoteError if a device wait timed out). Tuning and tests
 * only: the multi-process communicator's data path without its processes. */
int nbxDebugSimpleRun(int n, int kind, int ring, size_t count, int datatype, int op, const void* const* sends,
                      void* const* recvs, int root, int gridMax, size_t sliceBytes, int slots, int prefetch,
                      int iters, float* msPerCall);

/* NCCL_PROTO parsing (tuning.cc:254-259 list syntax: "LL,LL128", "^Simple",
 * case-insensitive; NULL or "" = all): bit 0 LL, bit 1 LL128, bit 2 Simple. */
int nbxDebugProtoMask(const char* ncclProto);

/* The multi-process communicator's per-message protocol choice: 0 LL, 1 LL128
 * (one-shot), 2 Simple, 3 LL128 two-shot, for a message of slotBytes (per-rank
 * block for ReduceScatter) whose direct-schedule block is blockBytes;
 * twoShotKind = 1 for AllReduce / Reduce, 0 for ReduceScatter. */
int nbxDebugChooseProto(int protoMask, int twoShotKind, uint64_t slotBytes, uint64_t blockBytes, int nRanks,
                        uint64_t llMaxBytes, uint64_t ll128MaxBytes, uint64_t ll128OneShotMax);

/* The protocol set a communicator starts from for NCCL_PROTO = ncclProto
 * (NULL: unset) when its ranks span more than one GPU (multiGpu = 1) or share
 * one: across GPUs LL128 is left out unless NCCL_PROTO names it (not in a
 * "^list") or NBX_LL128_ACROSS_GPUS=1 — the reference enables LL128 by default
 * only on validated fabrics (tuning.cc:287-297). NBX_DEBUG_ASSUME_MULTI_GPU=1
 * (test hook) applies the gate to ranks sharing a GPU. */
int nbxDebugGatedProtoMask(const char* ncclProto, int multiGpu);

/* The protocol set a communicator runs with (bits as nbxDebugProtoMask): its
 * NCCL_PROTO at creation gated as nbxDebugGatedProtoMask, minus LL128 if the
 * creation-time LL128 self-test failed (multi-rank communicators and clique
 * ranks; -1 for others or a bad handle). NBX_LL128_SELFTEST_FAIL=1 makes that
 * self-test report a failure (test hook). */
int nbxDebugCommProtoMask(ncclComm_t comm);

/* The transport settings a communicator runs with (after NCCL_BUFFSIZE /
 * NCCL_LL_BUFFSIZE / NCCL_LL128_BUFFSIZE / NCCL_MAX_NCHANNELS /
 * NCCL_MIN_NCHANNELS and the NBX_* overrides are applied at creation):
 * out[0] LL max bytes, [1] LL128 max bytes, [2] Simple slice bytes, [3] Simple
 * slots, [4] Simple grid, [5] LL grid cap, [6] LL128 grid cap, [7] group
 * batching, [8] connection buffers re-exported at creation because a peer's
 * IPC mapping of them showed other memory (verified before first use), [9]
 * plan checks on (NBX_CHECK_PLANS / NCCL_CHECK_POINTERS), [10] Simple slice
 * checksums on (NBX_CHECK_SLICES), [11] built-in ncclSum / ncclAvg accumulate
 * in fp32 on fp16, bf16 and fp8 (NBX_WIDE_ACCUM; include/nbx_reduce.h
 * nbxRedOpCreateWide). Writes min(nOut, 12) values and returns that
 * count; -1 for a bad handle or a communicator without a multi-rank transport. */
int nbxDebugCommSettings(ncclComm_t comm, int64_t* out, int nOut);

/* The settings a transport of nRanks ranks would be created with under the
 * current environment, with no communicator and no GPU (comm_mp_settings.cc
 * mpSettings): the smallest GPU has minCus CUs, at most maxShare ranks share a
 * GPU, the ranks span several GPUs (multiGpu = 1) or not; minCTAs / maxCTAs as
 * ncclConfig_t holds them (NCCL_CONFIG_UNDEF_INT: unset), checkPointers the
 * communicator's NCCL_CHECK_POINTERS. out[0..10] as nbxDebugCommSettings
 * ([8], re-exports, is 0), [11] protocol mask (as nbxDebugGatedProtoMask),
 * [12] ring schedule (NCCL_ALGO=Ring), [13] LL128 one-shot max bytes, [14] LL
 * lines per slot, [15] LL128 lines per slot, [16] NBX_WIDE_ACCUM
 * (nbxDebugCommSettings' [11]). Writes min(nOut, 17) values and
 * returns that count; -1 for a NULL out, nRanks outside 2..64, minCus or
 * maxShare below 1. */
int nbxDebugTransportSettings(int nRanks, int minCus, int maxShare, int multiGpu, int minCTAs, int maxCTAs,
                              int checkPointers, int64_t* out, int nOut);

/* The Simple transport's protocol state of a communicator (its own, or a
 * clique rank's in-process transport's), read once the device is idle: the
 * call synchronises the device, then copies this rank's 4 * nRanks * grid
 * counter words (what its workgroups carry from call to call: 0 RS sent, 1 RS
 * received, 2 AG sent, 3 AG received, per peer) and its own 4 * nRanks * grid
 * flag words (what its peers post into: 0 RS ready, 1 RS credit, 2 AG ready,
 * 3 AG credit, per poster) to the host; grid is out[4] of
 * nbxDebugCommSettings. Index of both arrays: (kind * nRanks + who) * grid + g
 * for peer `who` and workgroup g (nbx_simple.h simpleFlag). *prefetch: whether
 * the direct schedule pushes the next round before it folds this one
 * (NBX_SIMPLE_PREFETCH). Returns the words per array; -1 for a bad handle or a
 * NULL pointer, a communicator without that transport or still being created,
 * nWords (the capacity of each array) too small, or a HIP error. Read-only
 * host code: no kernel, nothing on any data path changes. The peers' posts
 * into the flag words are only final once every rank's device is idle: a test
 * synchronises every rank and meets on the host before it reads. A
 * communicator that reported an asynchronous error is still read (its state
 * is the evidence); the caller must not race the call with ncclCommDestroy or
 * ncclCommAbort of the same communicator. Test hook. */
int nbxDebugSimpleState(ncclComm_t comm, uint64_t* counters, uint64_t* flags, size_t nWords, int* prefetch);

/* Config D's xGMI transport alone, on a multi-process
 * communicator: an AllReduce-shaped call of the direct Simple schedule (forced
 * for any size and NCCL_ALGO) that moves every byte an AllReduce of `count`
 * elements moves between the ranks, with the fold reduced to a copy of the
 * own input; recvbuff receives junk. Collective (every rank, same count and
 * datatype), stream-ordered like ncclAllReduce. Measurement only. */
ncclResult_t nbxDebugTransportAllReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                                        ncclComm_t comm, ncclStream_t stream);

/* Per-link fabric rate of a multi-process communicator (the roofline config
 * D is priced against): each rank pushes (pull = 0, the Simple transport's
 * system-scope stores) or pulls (pull = 1, its system-scope loads)
 * bytesPerPeer to / from every peer's staging at once, in its own part of
 * each peer's slice area, on workgroupsPerPeer workgroups per peer (0: 32).
 * One kernel on `stream`; *bytesMovedPerPeer = the bytes one launch moves per
 * peer (bytesPerPeer rounded up to whole passes). Not ordered against
 * collectives and it overwrites the peers' staging: the caller keeps every
 * rank's communicator quiet around it. ncclInvalidArgument without a
 * multi-process transport. Measurement only. */
ncclResult_t nbxDebugLinkProbe(ncclComm_t comm, size_t bytesPerPeer, int pull, int workgroupsPerPeer,
                               ncclStream_t stream, size_t* bytesMovedPerPeer);

/* Stream ceilings in the caller's process (SURVEY §8(d) "a measured stream
 * ceiling"): kind 0 reads nSrcs == 8 buffers of `bytes` each with the hot
 * kernel's loads and tile (16-B nontemporal, 8 x 4 packs per lane, one
 * workgroup per CU) and stores nothing; kind 1 writes `bytes` to dst with its
 * stores (plain 16-B); kind 2 is the 8:1 mixed stream: the read kernel's
 * tile and the fold's schedule (dynamic tiles from 16 tiles per workgroup),
 * every load kept live without arithmetic, source 0 stored to dst (bytes per
 * source). Buffers 16-B aligned, bytes a multiple of 16;
 * blocksPerCU 0 = the production shape. Asynchronous on `stream` (a
 * hipStream_t). The 1:1 copy ceiling is nbxReduceMulti with one source. */
ncclResult_t nbxDebugStream(int kind, void* dst, const void* const* srcs, int nSrcs, size_t bytes, int blocksPerCU,
                            ncclStream_t stream);

/* A deliberately torn LL128 line against the collectives' own line reader
 * (nbx_ll.h l128Poll + l128FoldLine), one GPU: a writer kernel stores the
 * line's last 32 bytes, waits delayUs, then its first 32 bytes (tear = 1; 0
 * stores it whole); a reader kernel on another stream polls it. Returns 0 if
 * the reader folded exactly the new payload and (tear = 1) accepted the line
 * only after its second half was issued; 1 stale payload folded; 2 accepted
 * early; 3 the reader timed out; < 0 HIP error. *acceptAfterTornTicks =
 * acceptance time minus second-half issue time (100 MHz ticks). */
int nbxDebugLL128TearTest(int delayUs, int tear, long long* acceptAfterTornTicks);

/* Batched-reduce launch form (nbxReduceMultiBatch): 1 = work-list kernels
 * (bucket records in a table in device memory, or pinned host memory without
 * a large BAR, up to 384 buckets per launch; the default, env NBX_BATCH_LIST;
 * sets of <= 16 buckets that fit one kernel-argument table still use it),
 * 2 = work lists for every set, 0 = kernel-argument tables only; any other
 * value only queries. Returns the mode in force before the call. */
int nbxDebugSetBatchMode(int mode);

/* Work-list table slots of `device` in `state` (0 free, 1 read by an eager
 * launch that may still run, 2 owned by a captured graph); state 3: launches
 * so far that found no free slot and fell back to kernel-argument tables;
 * -1 bad device. */
int nbxDebugBatchListSlots(int device, int state);

/* Dynamic tile scheduling threshold of the big-tile reduce kernel: launches
 * with at least this many tiles per workgroup take tiles from the stream's
 * counter, shorter ones run the static grid stride (default 16, env
 * NBX_DYN_MIN_TILES_PER_WG; 1 makes every big-tile launch dynamic). Values < 1
 * only query. Returns the threshold in force before the call. */
int nbxDebugSetDynMinTiles(int tilesPerWorkgroup);

/* Threshold of the fp32-accumulating sums' realigning kernel
 * (nbxReduceMultiWide, kWideShiftedLds): a call outside the pack layout whose
 * destinations share one address modulo 16 takes it from this many elements,
 * the element kernel below (default 2097152, the crossover measured by
 * scripts/ab_wide_shift.py on an MI355X, profiles/r9/ab_wide_shift_mi355x.txt;
 * env NBX_WIDE_SHIFT_MIN_ELTS; 1 sends every such call to the realigning
 * kernel). Values < 1 only query. Returns the threshold in force before the
 * call. */
long long nbxDebugSetWideShiftMinElts(long long elts);

/* The layout nbxReduceMultiWide decides once per call, from the pointer
 * values alone (no device call, nothing dereferenced): 0 elements
 * (kWideElts), 1 packs (kWidePacks: every source on one misalignment modulo
 * 16, every destination 16-byte aligned behind the head elements that align
 * the sources), 2 realigning (kWideShiftedLds: any other layout whose
 * destinations share one address modulo 16, from the threshold above), -1 bad
 * arguments (types, counts of pointers, NULL or a pointer off its element
 * size). *head (may be NULL): the elements folded one by one in front of the
 * 16-byte body, at most count — those that align the sources (packs) or the
 * destinations (realigning; < 16 / destination element size), 0 for the
 * element kernel. The launch variant does not enter. */
int nbxDebugWideLayout(void* const* dsts, int nDsts, const void* const* srcs, int nSrcs, size_t count,
                       ncclDataType_t srcType, ncclDataType_t dstType, size_t* head);

/* Per-stream counters allocated so far on `device` by the dynamic schedules
 * (which: 0 = big-tile reduce's tile counters, 1 = realigning kernel's class
 * counters); keyed by stream handle (nbx_policy.cc). -1 bad device. */
int nbxDebugDynStreamSlots(int device, int which);

/* Holds `stream` with a one-wave kernel until nbxDebugReleaseStream(hold) or
 * timeoutMs pass, so a test can queue work behind it deterministically
 * (instead of racing a sleep against the host). Returns the hold (>= 0), -1
 * no free hold (16 at once) or bad timeout, -2 HIP error. Test hook. */
int nbxDebugHoldStream(ncclStream_t stream, int timeoutMs);
int nbxDebugReleaseStream(int hold);

/* Launch record (test hook): every kernel pass that nbxReduceMulti /
 * nbxReduceMultiWide / nbxReduceMultiBatch / nbxReduceMultiWideBatch launch
 * from the calling thread, and
 * every collective kernel a multi-rank communicator launches from it, appends
 * {family, nSrcs, unroll, flags} to a thread-local log, so a test can see
 * which kernel a call took.
 * Reduction core — family: 1 small-tile packs, 2 big-tile packs,
 * 3 elements, 4 realigning LDS-DMA (one kernel per source count), 5 realigning
 * run-time source count, 6 wide packs, 7 wide elements, 16 wide realigning
 * LDS-DMA (kWideShiftedLds, one kernel per source count; unroll 2 from 3
 * sources, else 1; never dynamic). nSrcs: the pass's
 * sources (a later pass of a > 8-source call counts its partial). unroll:
 * packs per lane per source and tile (1 for the element kernels). flags:
 * bit 0 dynamic tile schedule, bit 1 fp32 output (wide), bit 2 the first
 * source is the fp32 partial of earlier passes (wide).
 * Collective launches of a multi-rank communicator (comm_mp_launch.cc
 * mpLaunchLL / mpLaunchSimple), one record per kernel launched — family:
 * 8 LL (kLLColl), 9 LL128 one-shot (kLL128Coll), 10 LL128 two-shot
 * (kLL128AllReduce2), 11 Simple direct (kSimpleColl; the transport-only call
 * of nbxDebugTransportAllReduce too), 12 Simple ring (kSimpleRing). nSrcs:
 * the communicator's rank count. unroll: 1 for LL / LL128; 0 for Simple,
 * whose kernel picks its fold's unroll on the device from the sources of each
 * fold (16 for <= 2, 8 for <= 4, else 4: nbx_simple.h simpleFold), which the
 * host does not know. flags: bit 0 the checking instantiation (LL family:
 * plan checks, NBX_CHECK_PLANS / NCCL_CHECK_POINTERS; Simple: slice
 * checksums, NBX_CHECK_SLICES), bit 1 the fp32-accumulating instantiation
 * (a handle of nbxRedOpCreateWide, or NBX_WIDE_ACCUM; its Simple fold unrolls
 * 8 / 4 / 4 at <= 2 / <= 4 / more sources; never family 12: a wide call on a
 * ring communicator is family 11), bits 8.. the segments of a group's calls
 * run as one launch (0: a single call). An in-process clique's fold of a wide
 * call leaves the wide core's records (families 6 / 7 / 16). A call is recorded on the thread that
 * launches it, after the launch succeeded: the caller's thread for
 * ncclAllReduce / ncclReduceScatter / ncclReduce outside a group, the thread
 * of the outermost ncclGroupEnd for grouped calls. The LL128 self-test of
 * communicator creation launches collectives too: on the creating thread, or
 * on the background thread of a non-blocking ncclCommInitRankConfig — reset
 * the log after creation.
 * Batched launches of nbxReduceMultiBatch (nbx_reduce_batch.cc BatchPacker::flush /
 * launchBatchList), one record per kernel launched, after the launch
 * succeeded — family: 13 kernel-argument batch (kReduceBatch), 14 work-list
 * batch (kReduceBatchList). nSrcs: the launch's source count. unroll: 1.
 * flags: bit 0 unused, bits 8.. the buckets of that launch (buckets of count
 * 0 are never in a launch and are not counted). Buckets that do not go into
 * a batch (mixed alignment, > 8 sources, 4+ sources filling the GPU alone,
 * launch variant 2) leave the records of the single-bucket path, families
 * 1-5. Order of one call's records: those single buckets first, in bucket
 * order; then, per source count ascending, that count's work-list launches
 * followed by its kernel-argument launches (the buckets no free table slot
 * was left for; all of them with work lists off or for a small set).
 * Batched launches of nbxReduceMultiWideBatch (nbx_reduce_batch.cc
 * launchBatchList), one record per kernel launched, after the launch
 * succeeded — family: 15 wide work-list batch (kWideBatchList). nSrcs: the
 * launch's source count. unroll: 1. flags: bit 1 fp32 output, bits 8.. the
 * buckets of that launch (buckets of count 0 are never counted). Buckets that
 * do not go into a batch leave the records of nbxReduceMultiWide, families 6,
 * 7 and 16 (a bucket in the realigning layout is family 16 from the threshold
 * of nbxDebugSetWideShiftMinElts, family 7 below it, in the same place of the
 * order). Order of one call's records: first, in bucket order, the buckets
 * that run alone (mixed layouts, > 8 sources, 4+ sources filling the GPU
 * alone, every bucket under launch variant 2); then, per source count
 * ascending, that count's work-list launches followed by one family-6 launch
 * for each of its buckets that got no table slot (arena exhausted — counted
 * in nbxDebugBatchListSlots(dev, 3) as for the per-step batch —, a capture
 * that cannot take a slot, batch mode 0). Batch modes 1 and 2 both mean work
 * lists here: there is no kernel-argument form.
 * Plain host stores; the log keeps the newest 64 passes.
 * nbxDebugLaunchLog returns the number of passes since the last
 * nbxDebugLaunchLogReset() and copies the newest min(maxRecords, 64, that
 * number) of them, oldest first, four int32 each, to `out`. */
int nbxDebugLaunchLog(int32_t* out, int maxRecords);
void nbxDebugLaunchLogReset(void);

#ifdef __cplusplus
}
#endif

#endif /* NBX_DEBUG_H_ */
