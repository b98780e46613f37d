// comm_mp_init.cc — the multi-process communicator's creation.
// Multi-process communicator (ncclCommInitRank with nranks > 1, one process
// per rank on one node). Replaces NCCL's bootstrap + P2P transport setup
// (bootstrap.cc, transport/p2p.cc:190-381) with a TCP bootstrap for the
// init-time allgathers and connection buffers that the library allocates and
// every peer IPC-maps ONCE, at init (p2pMap / p2pSendConnect / p2pRecvConnect,
// p2p.cc:290-330,450-520):
//   * LL / LL128 line buffers (nbx_ll.h) for small and medium messages;
//   * the Simple protocol's staging and flag words (nbx_simple.h) for the rest,
//     direct or ring schedule (NCCL_ALGO=Ring).
// Peers never touch the caller's buffers and no call exchanges anything on
// the host: a collective is one kernel on the caller's stream whose flow
// control (the reference's waitPeer / postPeer, prims_simple.h:129-185)
// runs inside it. All sequencing state is device-resident, so graph capture
// and replay need nothing special.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <exception>
#include <random>
#include <unistd.h>
#include "nbx_comm.h"

namespace nbxcomm {

namespace {
// Exchanged before anything is allocated: where every rank runs.
struct MpPreInfo {
  uint64_t pciKey;   // (domain, bus, device) of this rank's GPU: identifies it across processes
  int32_t device;
  int32_t cus;
};

// The settings every rank must share — every rank must pick the same protocol,
// grid and staging layout for the same call — grouped by the message a
// difference is reported with. Exchanged as MpInitInfo::agreed, in this order.
struct Agreed {
  int group;
  uint64_t (*get)(const MpState*);
};
#define NBX_AGREED(group, field) {group, [](const MpState* mp) { return (uint64_t)mp->field; }}
const Agreed kAgreed[kNumAgreed] = {
    NBX_AGREED(0, llMaxBytes), NBX_AGREED(0, l128MaxBytes), NBX_AGREED(0, l128OneShotMax), NBX_AGREED(0, protoMask),
    NBX_AGREED(1, ring),       NBX_AGREED(1, sliceBytes),   NBX_AGREED(1, slots),          NBX_AGREED(1, simpleGrid),
    // a group's calls become one launch or one per call, and every launch
    // advances the device-resident sequence by one: ranks must cut alike
    NBX_AGREED(2, groupBatch),
    // a checking rank would wait for plan words a non-checking peer never stamps
    NBX_AGREED(3, checkPlans),
    // a checking consumer would compare against sums a non-checking producer never stamps
    NBX_AGREED(4, checkSlices),
    // a wide rank and a per-step rank would fold the same lines differently
    NBX_AGREED(5, wideAccum)};
#undef NBX_AGREED
const char* const kAgreedDiffer[] = {
    "NCCL_PROTO / NBX_LL_MAX_BYTES / NBX_LL128_MAX_BYTES / NBX_LL128_ONESHOT_MAX differ across ranks",
    "NCCL_ALGO / NBX_SIMPLE_MAX_GRID / NBX_SIMPLE_SLICE_BYTES / NBX_SIMPLE_SLOTS differ across ranks",
    "NBX_GROUP_BATCH differs across ranks", "NBX_CHECK_PLANS / NCCL_CHECK_POINTERS differ across ranks",
    "NBX_CHECK_SLICES differs across ranks", "NBX_WIDE_ACCUM differs across ranks"};

}  // namespace

// A device spin gave up (host error word set): name the wait, the peer, the
// value it waited for and the last one it saw (nbx_diag.h), once per record.
void mpReportDeviceError(ncclComm* c) {
  MpState* mp = mpOf(c);
  if (!mp || !mp->hostWords || mp->hostWords[1] == 0) return;
  const volatile uint64_t* d = (const volatile uint64_t*)((const volatile char*)mp->hostWords + nbx::kDiagByteOffset);
  static thread_local uint64_t lastReported[nbx::kDiagWords] = {};
  uint64_t rec[nbx::kDiagWords];
  for (int i = 0; i < nbx::kDiagWords; i++) rec[i] = d[i];
  if (std::memcmp(rec, lastReported, sizeof(rec)) == 0) return;
  std::memcpy(lastReported, rec, sizeof(rec));
  if (mp->hostWords[1] == 2) {
    warn("comm %p rank %d: a device wait was aborted (ncclCommAbort)", (void*)c, c->rank);
    return;
  }
  if (rec[0] == nbx::kDiagSimpleSlice) {
    warn("comm %p rank %d: device check failed: %s: from peer %lld, slot use %llu: the peer stamped sum %08llx, "
         "this rank read sum %08llx (use %llu) (workgroup %llu)", (void*)c, c->rank, nbx::diagSiteName(rec[0]),
         (long long)(int64_t)rec[1], (unsigned long long)(rec[2] >> 32), (unsigned long long)(rec[2] & 0xffffffffu),
         (unsigned long long)(rec[3] & 0xffffffffu), (unsigned long long)(rec[3] >> 32), (unsigned long long)rec[4]);
    return;
  }
  if (nbx::diagIsPlanCheck(rec[0])) {
    warn("comm %p rank %d: device check failed after %.3f s: %s: peer %lld, our plan %llx, its plan %llx "
         "(workgroup %llu)", (void*)c, c->rank, (double)rec[5] * 1e-8, nbx::diagSiteName(rec[0]),
         (long long)(int64_t)rec[1], (unsigned long long)rec[2], (unsigned long long)rec[3],
         (unsigned long long)rec[4]);
    return;
  }
  warn("comm %p rank %d: device wait timed out after %.3f s: %s of peer %lld, waited for %llu, last saw %llu "
       "(workgroup %llu)", (void*)c, c->rank, (double)rec[5] * 1e-8, nbx::diagSiteName(rec[0]),
       (long long)(int64_t)rec[1], (unsigned long long)rec[2], (unsigned long long)rec[3],
       (unsigned long long)rec[4]);
}

ncclResult_t mpInit(ncclComm* c, const ncclUniqueId& id) {
  MpState* mp = new MpState();
  c->mp = mp;
  const int n = c->nRanks, me = c->rank;
  NCCLCHECK(nbx::bootstrapConnect(id, me, n, &mp->bs));
  // where every rank runs: decides LL128's self-test and the Simple grid
  MpPreInfo pre{};
  {
    int dom = 0, bus = 0, dv = 0, cus = 0;
    (void)hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, c->device);
    (void)hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, c->device);
    (void)hipDeviceGetAttribute(&dv, hipDeviceAttributePciDeviceId, c->device);
    HIPCHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    pre.pciKey = ((uint64_t)(uint32_t)dom << 32) | ((uint64_t)(uint32_t)bus << 8) | (uint64_t)(uint32_t)dv;
    pre.device = c->device;
    pre.cus = cus;
  }
  std::vector<MpPreInfo> pres(n);
  NCCLCHECK(nbx::bootstrapAllGather(mp->bs, &pre, sizeof(pre), pres.data()));
  int minCus = pre.cus, maxShare = 1;
  bool multiGpu = false;
  for (int j = 0; j < n; j++) {
    multiGpu |= pres[j].pciKey != pre.pciKey;
    minCus = std::min(minCus, (int)pres[j].cus);
    int share = 0;
    for (int q = 0; q < n; q++) share += pres[q].pciKey == pres[j].pciKey;
    maxShare = std::max(maxShare, share);
  }
  mpSettings(mp, n, minCus, maxShare, multiGpu, c->minCTAs, c->maxCTAs, c->checkPointers);
  NCCLCHECK(mpAlloc(mp, n, /*ipc=*/true, /*simple=*/true, c));
  HIPCHECK(hipDeviceSynchronize());   // zeroed before any peer can map and write them

  MpInitInfo mine{};
  mine.device = c->device;
  for (int k = 0; k < kNumAgreed; k++) mine.agreed[k] = kAgreed[k].get(mp);
  mine.nonce = std::random_device{}() * 0x100000001ull ^ (uint64_t)std::random_device{}() ^
               ((uint64_t)getpid() << 20) ^ (uint64_t)(uintptr_t)mp;
  for (int t = 0; t < kNumConn; t++) mine.handle[t] = mp->conn[t].handle;
  std::vector<MpInitInfo> all(n);
  NCCLCHECK(nbx::bootstrapAllGather(mp->bs, &mine, sizeof(mine), all.data()));
  for (int j = 0; j < n; j++) {
    for (int k = 0; k < kNumAgreed; k++)
      if (all[j].agreed[k] != mine.agreed[k]) {
        warn("ncclCommInitRank : %s", kAgreedDiffer[kAgreed[k].group]);
        return ncclInvalidUsage;
      }
    if (j == me || all[j].device == c->device) continue;
    int can = 0;
    HIPCHECK(hipDeviceCanAccessPeer(&can, c->device, all[j].device));
    if (!can) {
      // every data path here is a kernel store to peer memory; there is no
      // host-staged transport, so fail cleanly instead of faulting later
      warn("ncclCommInitRank : device %d cannot access peer device %d (no P2P)", c->device, all[j].device);
      return ncclSystemError;
    }
    hipError_t e = hipDeviceEnablePeerAccess(all[j].device, 0);
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIPCHECK(e);
    (void)hipGetLastError();
  }
  // every peer buffer mapped and checked before the first collective
  NCCLCHECK(mpConnect(c, all));
  NCCLCHECK(mpLL128SelfTest(c));
  info("comm %p rank %d nranks %d device %d: multi-process communicator ready (Simple grid %d, slice %llu B, "
       "staging %llu MiB)", (void*)c, me, n, c->device, mp->simpleGrid, (unsigned long long)mp->sliceBytes,
       (unsigned long long)(mp->conn[kConnStage].bytes >> 20));
  return ncclSuccess;
}

// LL128 correctness probe at communicator creation. LL128 relies on a 64-byte
// line written by one store instruction arriving whole (the flag in its last
// 8 bytes vouches for the 56 payload bytes, nbx_ll.h). That holds for every
// configuration measured here, but it is a property of the fabric between the
// GPUs of this communicator, so each communicator checks it before use:
// NBX_LL128_SELFTEST_ITERS (default 24; 0 = skip) AllReduces of integer data
// that changes every call, at one-shot and at two-shot sizes, each result
// compared exactly on the host. If any rank sees any wrong element, every rank
// drops LL128 from its protocol set (decided from an allgather, so the choice
// stays identical everywhere) and LL / Simple carry those sizes.
ncclResult_t mpLL128SelfTest(ncclComm* c) {
  MpState* mp = c->mp;
  if (!(mp->protoMask & kProtoLL128) || mp->l128MaxBytes == 0) return ncclSuccess;
  // only across GPUs (within one GPU the 64-byte line was stress-tested, DESIGN
  // §6), unless NBX_LL128_SELFTEST_ITERS asks for it explicitly; multiGpu is
  // the same on every rank (derived from every rank's PCI key)
  const char* v = std::getenv("NBX_LL128_SELFTEST_ITERS");
  const long iters = (v && *v) ? std::atol(v) : (mp->multiGpu ? 24 : 0);
  if (iters <= 0) return ncclSuccess;
  const int n = c->nRanks, me = c->rank;
  // one-shot (just above the LL limit) and two-shot (n > 2, above the one-shot limit) sizes
  std::vector<size_t> counts = {(size_t)(mp->llMaxBytes / 4 + 1024)};
  const uint64_t twoShot = std::min<uint64_t>(mp->l128OneShotMax * 2, mp->l128MaxBytes);
  if (n > 2 && twoShot > mp->l128OneShotMax) counts.push_back((size_t)(twoShot / 4 - 13));
  size_t maxCount = 0;
  for (size_t k : counts) maxCount = std::max(maxCount, k);
  DevGuard g(c->device);
  hipStream_t st = nullptr;
  int32_t* dSend = nullptr;
  int32_t* dRecv = nullptr;
  HIPCHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  HIPCHECK(hipMalloc((void**)&dSend, maxCount * sizeof(int32_t)));
  HIPCHECK(hipMalloc((void**)&dRecv, maxCount * sizeof(int32_t)));
  std::vector<int32_t> hIn(maxCount), hOut(maxCount);
  nbxDevRedOpFull sum{nbxDevSum, 0, 0};
  int32_t bad = 0;
  ncclResult_t r = ncclSuccess;
  for (size_t count : counts) {
    for (long it = 0; it < iters && r == ncclSuccess; it++) {
      for (size_t i = 0; i < count; i++) hIn[i] = (int32_t)((i * 7 + (size_t)me * 13 + (size_t)it * 101) % 1000);
      if (hipMemcpyAsync(dSend, hIn.data(), count * 4, hipMemcpyHostToDevice, st) != hipSuccess) {
        r = ncclUnhandledCudaError;
        break;
      }
      const MpCall call{kAllReduce, dSend, dRecv, count, ncclInt32, sum, 0, st};
      r = runMpColl(c, call);
      if (r != ncclSuccess) break;
      if (hipMemcpyAsync(hOut.data(), dRecv, count * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess) {
        r = ncclUnhandledCudaError;
        break;
      }
      if (mp->hostWords[1] != 0) {   // a device wait gave up: an error, not a torn line
        mpReportDeviceError(c);
        warn("comm %p rank %d: LL128 self-test call %ld (%zu elements) did not complete", (void*)c, me, it, count);
        r = ncclRemoteError;
        break;
      }
      for (size_t i = 0; i < count && !bad; i++) {
        int64_t want = 0;
        for (int q = 0; q < n; q++) want += (int64_t)((i * 7 + (size_t)q * 13 + (size_t)it * 101) % 1000);
        if (hOut[i] != (int32_t)want) bad = 1;
      }
    }
  }
  const char* fail = std::getenv("NBX_LL128_SELFTEST_FAIL");   // test hook: simulate a torn line
  if (fail && std::strcmp(fail, "1") == 0) bad = 1;
  (void)hipStreamSynchronize(st);
  (void)hipFree(dSend);
  (void)hipFree(dRecv);
  (void)hipStreamDestroy(st);
  mp->lastSeq = 0;   // the probe's work is complete; its stream is gone
  if (r != ncclSuccess) return r;
  std::vector<int32_t> all(n);
  NCCLCHECK(nbx::bootstrapAllGather(mp->bs, &bad, sizeof(bad), all.data()));
  bool anyBad = false;
  for (int32_t b : all) anyBad |= b != 0;
  if (anyBad) {
    warn("comm %p rank %d: LL128 self-test found torn lines on this fabric; LL128 disabled for this communicator",
         (void*)c, me);
    mp->protoMask &= ~kProtoLL128;
  }
  return ncclSuccess;
}

}  // namespace nbxcomm

using namespace nbxcomm;

NBX_API(ncclResult_t, ncclGetUniqueId, ncclUniqueId* out) {
  if (out == nullptr) return ncclInvalidArgument;
  return nbx::bootstrapCreateRoot(out);   // bootstrap.cc: the root listens for the ranks
}

NBX_API(ncclResult_t, ncclCommInitRankConfig, ncclComm_t* newcomm, int nranks, ncclUniqueId commId, int myrank,
        ncclConfig_t* config) {
  if (newcomm == nullptr) return ncclInvalidArgument;
  if (nranks < 1 || myrank < 0 || myrank >= nranks) {
    warn("Invalid rank requested : %d/%d", myrank, nranks);
    return ncclInvalidArgument;
  }
  ncclConfig_t cfg;
  NCCLCHECK(parseConfig(config, &cfg));   // parseCommConfig (init.cc:1526-1594)
  if (std::memcmp(commId.internal, kIdMagic, sizeof(kIdMagic)) != 0) {
    warn("ncclCommInitRank : unique id was not produced by ncclGetUniqueId");
    return ncclInvalidArgument;
  }
  if (nranks > kMaxMpRanks) {   // one staging source region and one counter set per rank (kSimpleMaxRanks)
    warn("ncclCommInitRank : %d ranks requested, this build supports up to %d per communicator", nranks,
         kMaxMpRanks);
    return ncclInvalidArgument;
  }
  int dev = 0;
  HIPCHECK(hipGetDevice(&dev));
  if (nranks == 1) {
    NCCLCHECK(newComm(newcomm, 1, 0, dev, &cfg));
    return (*newcomm)->blocking ? ncclSuccess : ncclInProgress;   // nothing to wait for: already ready
  }
  if (!nbx::bootstrapIdHasRoot(commId)) {
    warn("ncclCommInitRank : unique id carries no bootstrap root");
    return ncclInvalidArgument;
  }
  ncclComm* c = nullptr;
  NCCLCHECK(newComm(&c, nranks, myrank, dev, &cfg));
  auto init = [](ncclComm* cm, ncclUniqueId id) -> ncclResult_t {
    ncclResult_t r;
    try {
      r = mpInit(cm, id);
    } catch (const std::exception& e) {
      warn("internal exception: %s", e.what());
      r = ncclInternalError;
    }
    if (r != ncclSuccess) mpFree(cm);
    return r;
  };
  if (!c->blocking) {
    // non-blocking (init.cc:1757-1771, group.cc:390-415): the communicator is
    // handed out at once and initialised by a background thread;
    // ncclCommGetAsyncError reports ncclInProgress until it is done
    c->asyncError.store(ncclInProgress);
    *newcomm = c;
    try {
      c->initThread = std::thread([c, commId, dev, init] {
        (void)hipSetDevice(dev);
        nbx::bootstrapSetAbortFlag(&c->initAbort);
        c->asyncError.store(init(c, commId));
        nbx::bootstrapSetAbortFlag(nullptr);
      });
    } catch (const std::exception& e) {
      warn("ncclCommInitRankConfig : cannot start the initialisation thread: %s", e.what());
      c->asyncError.store(ncclSystemError);
      return ncclSystemError;
    }
    return ncclInProgress;
  }
  const ncclResult_t r = init(c, commId);
  if (r != ncclSuccess) {
    delete c;
    return r;
  }
  *newcomm = c;
  return ncclSuccess;
}

NBX_API(ncclResult_t, ncclCommInitRank, ncclComm_t* newcomm, int nranks, ncclUniqueId commId, int myrank) {
  return ncclCommInitRankConfig(newcomm, nranks, commId, myrank, nullptr);
}

NBX_EXPORT int nbxDebugCommProtoMask(ncclComm_t comm) {
  if (comm == nullptr || comm->magic != kCommMagic || mpOf(comm) == nullptr) return -1;
  return mpOf(comm)->protoMask;   // a clique rank: its in-process transport's
}

// The transport settings a communicator runs with (its own, or a clique
// rank's in-process transport's): out[0] LL max bytes, [1] LL128 max bytes,
// [2] Simple slice bytes, [3] Simple slots, [4] Simple grid, [5] LL grid cap,
// [6] LL128 grid cap, [7] group batching, [8] connection buffers re-exported
// at creation because a peer's mapping of them was wrong (mpConnect), [9] plan
// checks on (NBX_CHECK_PLANS / NCCL_CHECK_POINTERS), [10] slice checksums on
// (NBX_CHECK_SLICES), [11] built-in Sum / Avg accumulate in fp32 on the 16-bit
// and fp8 types (NBX_WIDE_ACCUM). Returns how many were written, -1
// for a bad handle or a communicator without that transport.
NBX_EXPORT int nbxDebugCommSettings(ncclComm_t comm, int64_t* out, int nOut) {
  if (comm == nullptr || comm->magic != kCommMagic || out == nullptr) return -1;
  if (comm->asyncError.load() != ncclSuccess) return -1;
  const MpState* mp = mpOf(comm);
  if (mp == nullptr) return -1;
  int64_t v[kNumSettingsValues];
  mpSettingsValues(mp, v);
  int k = 0;
  for (; k < nOut && k < kNumCommSettings; k++) out[k] = v[k];
  if (k == kNumCommSettings && k < nOut) out[k++] = v[kSettingWideAccum];
  return k;
}

// The Simple transport's protocol state after the device went idle: this
// rank's counter words and its own flag words (the ones its peers post into),
// 4 * nRanks * simpleGrid each, index (kind * nRanks + who) * simpleGrid + g
// (nbx_simple.h simpleFlag). Read-only: a device synchronisation and two
// copies to the host. Returns the words per array, -1 for a bad handle, a
// communicator without that transport, nWords too small or a HIP error.
NBX_EXPORT int nbxDebugSimpleState(ncclComm_t comm, uint64_t* counters, uint64_t* flags, size_t nWords,
                                   int* prefetch) {
  if (comm == nullptr || comm->magic != kCommMagic || counters == nullptr || flags == nullptr || prefetch == nullptr)
    return -1;
  if (comm->asyncError.load() == ncclInProgress) return -1;   // still being created
  const MpState* mp = mpOf(comm);
  if (mp == nullptr || mp->scounters == nullptr || mp->own(kConnFlags) == nullptr || mp->simpleGrid < 1) return -1;
  const size_t words = 4 * (size_t)comm->nRanks * (size_t)mp->simpleGrid;
  if (nWords < words || words > (size_t)INT32_MAX) return -1;
  DevGuard g(comm->device);
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(counters, mp->scounters, words * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (hipMemcpy(flags, mp->own(kConnFlags), words * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  *prefetch = mp->simplePrefetch;
  return (int)words;
}

NBX_EXPORT ncclResult_t nbxBootstrapSelfTest(const ncclUniqueId* id, int rank, int nranks, int rounds) {
  if (id == nullptr || nranks < 1 || rank < 0 || rank >= nranks || rounds < 0) return ncclInvalidArgument;
  nbx::Bootstrap* b = nullptr;
  NCCLCHECK(nbx::bootstrapConnect(*id, rank, nranks, &b));
  ncclResult_t res = ncclSuccess;
  for (int r = 0; r < rounds && res == ncclSuccess; r++) {
    const size_t len = 8 + (size_t)(r * 37) % 4096;
    std::vector<unsigned char> mine(len), all(len * (size_t)nranks);
    for (size_t i = 0; i < len; i++) mine[i] = (unsigned char)(rank * 31 + r * 7 + i);
    res = nbx::bootstrapAllGather(b, mine.data(), len, all.data());
    for (int j = 0; j < nranks && res == ncclSuccess; j++)
      for (size_t i = 0; i < len; i++)
        if (all[(size_t)j * len + i] != (unsigned char)(j * 31 + r * 7 + i)) {
          res = ncclInternalError;
          break;
        }
  }
  nbx::bootstrapClose(b);
  return res;
}
