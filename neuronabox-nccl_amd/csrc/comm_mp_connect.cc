// comm_mp_connect.cc — the connection buffers of a multi-rank transport
// (MpState::conn): the pool of exported buffers, their allocation, the check and
// repair of every peer's IPC mapping (mpConnect), the peer tables, the release.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <array>
#include <strings.h>
#include "nbx_comm.h"

namespace nbxcomm {

// Memory that other GPUs write and this GPU reads (LL lines, Simple staging
// and flag words). Uncached (MTYPE UC) by default: a peer's stores over xGMI
// land in HBM and no XCD L2 can hold a stale copy, which is what RCCL uses
// for its connection buffers too. NBX_SYNC_MEM=coarse selects plain hipMalloc
// (A/B measurement only).
// A connection buffer every peer maps: uncached device memory, its size
// rounded up to whole 2 MiB pages so the buffer is an allocation of its own,
// and its IPC handle taken at once.
// The runtime rule behind the retry (scripts/probe_ipc_export.py: N processes
// replaying communicator creation / destruction with the library's buffer
// sizes, raw HIP, no libnbxccl; profiles/r4/probe_ipc_export_r4*.jsonl):
// once exported allocations are freed, hipIpcGetMemHandle now and then refuses
// ('invalid argument') a new allocation — 25 of 62,400 exports, 20 of them at
// an address whose earlier allocation had been exported and freed; the same
// pointer was refused again on an immediate retry 23 times of 25, and a fresh
// allocation (the refused one still held, so at another address) was
// accepted 23 times of 23. With exported buffers never freed: 0 of 19,200. So
// a refused allocation is held aside while the next one is made (at most 4
// tries), then freed. The same runtime condition also makes a successful
// export name the wrong memory now and then (mpConnect, which verifies every
// mapping and re-exports what is wrong).
//
// Exported buffers are never given back to the runtime (the pool below).
// A rank that destroys its communicator used to hipFree what its peers still
// had mapped (a peer closes its mappings at its own destroy, and nothing makes
// the ranks meet there), and every later communicator exported fresh
// allocations at addresses whose earlier allocation had been exported and
// freed — the one condition under which the probe above saw refused and wrong
// exports (0 of 19,200 with exported buffers never freed). So freeSyncMem
// keeps an exported buffer, with the IPC handle it was exported under, and
// allocSyncMem hands it to the next communicator of this process that asks
// for the same size on the same device; the caller clears it as it clears a
// new allocation. A buffer whose export mpConnect found wrong is kept but not
// handed out again. The pool holds at most what the process's communicators
// held at their peak, per distinct size (sizes are whole 2 MiB pages).
struct ExportedBuf {
  void* p;
  size_t bytes;
  int device;
  hipIpcMemHandle_t handle;
  bool inUse, retired;
};
std::mutex g_exportedMu;
std::vector<ExportedBuf> g_exported;

hipError_t allocSyncMem(void** p, size_t bytes, hipIpcMemHandle_t* handle /* nullptr: in-process only */) {
  static const bool coarse = [] {
    const char* v = std::getenv("NBX_SYNC_MEM");
    return v && strcasecmp(v, "coarse") == 0;
  }();
  const size_t page = (size_t)2 << 20;
  bytes = (bytes + page - 1) / page * page;
  int device = -1;
  if (handle != nullptr) {
    if (hipGetDevice(&device) != hipSuccess) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> g(g_exportedMu);
    for (ExportedBuf& b : g_exported)
      if (!b.inUse && !b.retired && b.bytes == bytes && b.device == device) {
        b.inUse = true;
        *p = b.p;
        *handle = b.handle;
        return hipSuccess;
      }
  }
  std::vector<void*> refused;
  hipError_t e = hipSuccess;
  for (int attempt = 0; attempt < 4; attempt++) {
    *p = nullptr;
    e = coarse ? hipMalloc(p, bytes) : hipExtMallocWithFlags(p, bytes, hipDeviceMallocUncached);
    if (e != hipSuccess || handle == nullptr) break;
    e = hipIpcGetMemHandle(handle, *p);
    if (e == hipSuccess) break;
    (void)hipGetLastError();
    info("hipIpcGetMemHandle refused a %zu-byte connection buffer at %p (%s): a reused exported address; "
         "allocating another", bytes, *p, hipGetErrorString(e));
    refused.push_back(*p);
    *p = nullptr;
  }
  for (void* q : refused) (void)hipFree(q);
  if (e == hipSuccess && handle != nullptr) {
    std::lock_guard<std::mutex> g(g_exportedMu);
    g_exported.push_back(ExportedBuf{*p, bytes, device, *handle, true, false});
  }
  return e;
}

// Gives a buffer of allocSyncMem back: an exported one to the pool (`wrong`:
// its export named other memory, it is never handed out again), any other to
// the runtime.
void freeSyncMem(void* p, bool wrong = false) {
  if (p == nullptr) return;
  {
    std::lock_guard<std::mutex> g(g_exportedMu);
    for (ExportedBuf& b : g_exported)
      if (b.p == p) {
        b.inUse = false;
        b.retired = b.retired || wrong;
        return;
      }
  }
  (void)hipFree(p);
}

// The 16-byte mapping self-check word rank `from` leaves at slot `at`.
void checkWord(uint64_t nonce, int from, int at, uint64_t out[2]) {
  out[0] = nonce ^ (0x9e3779b97f4a7c15ull * (uint64_t)(from + 1));
  out[1] = ~nonce ^ (0xc2b2ae3d27d4eb4full * (uint64_t)(at + 1));
}

// Every connection buffer carries a check region after its used bytes:
// 16 bytes per writer rank plus the owner's own word (mpConnect).
uint64_t connCheckOff(uint64_t used) { return (used + 15) & ~(uint64_t)15; }
uint64_t connAllocBytes(uint64_t used, int n) { return connCheckOff(used) + 16ull * (uint64_t)(n + 1); }

// One connection buffer of `b->bytes` used bytes among n ranks: uncached,
// with its check region, exported when `ipc`, zeroed.
ncclResult_t connAlloc(ConnBuf* b, int n, bool ipc) {
  const uint64_t bytes = connAllocBytes(b->bytes, n);
  HIPCHECK(allocSyncMem(&b->own, bytes, ipc ? &b->handle : nullptr));
  HIPCHECK(hipMemset(b->own, 0, bytes));
  return ncclSuccess;
}

// One rank's transport state on the current device, after mpSettings:
// completion word, sequencing state, host abort / error words, the connection
// buffers with used bytes (IPC handles taken when `ipc`; a clique's buffers
// stay in-process) and, with `simple`, the Simple protocol's staging, flag
// words and counters.
ncclResult_t mpAlloc(MpState* mp, int n, bool ipc, bool simple, const ncclComm* comm) {
  HIPCHECK(hipMalloc((void**)&mp->orderMem, 1024));
  HIPCHECK(hipMemset(mp->orderMem, 0, 1024));
  HIPCHECK(hipMalloc((void**)&mp->llState, sizeof(nbx::LLState)));
  HIPCHECK(hipMemset(mp->llState, 0, sizeof(nbx::LLState)));
  if (comm->hostWords == nullptr) return ncclInternalError;
  mp->hostWords = comm->hostWords;
  mp->hostWordsDev = comm->hostWordsDev;
  const bool wanted[kNumConn] = {true, true, simple, simple};
  for (int t = 0; t < kNumConn; t++)
    if (wanted[t] && mp->conn[t].bytes != 0) NCCLCHECK(connAlloc(&mp->conn[t], n, ipc));
  if (!simple) return ncclSuccess;
  HIPCHECK(hipMalloc((void**)&mp->scounters, mp->conn[kConnFlags].bytes));
  HIPCHECK(hipMemset(mp->scounters, 0, mp->conn[kConnFlags].bytes));
  return ncclSuccess;
}

ncclResult_t connUploadTables(MpState* mp, int n, const std::function<void*(int, int)>& peerOf) {
  std::vector<void*> table(n);
  for (int t = 0; t < kNumConn; t++) {
    ConnBuf& b = mp->conn[t];
    if (b.own == nullptr) continue;
    for (int j = 0; j < n; j++) table[j] = peerOf(j, t);
    HIPCHECK(hipMalloc((void**)&b.peersDev, n * sizeof(void*)));
    HIPCHECK(hipMemcpy(b.peersDev, table.data(), n * sizeof(void*), hipMemcpyHostToDevice));
  }
  return ncclSuccess;
}

// Opens every peer's connection buffers and checks every mapping before first
// use, re-exporting any buffer whose mapping is wrong (the reference maps its
// peers' buffers once at connection time, transport/p2p.cc:290-330 p2pMap).
// Why the check is needed: scripts/probe_ipc_export.py (raw HIP, N processes
// on one GPU replaying communicator creation / destruction with this
// library's buffer sizes and memory kinds) found IPC mappings that do not
// show the exported allocation — an importer reads zeros or ANOTHER rank's
// buffer through it (89 canary reads), and its stores never reach the owner
// (164), out of 62,400 imports, in the library's own memory kind as in plain
// hipMalloc memory; the same wrong bytes are seen by every importer of that
// handle (so it is the export, not one importer's mapping, that is wrong),
// mostly at owner addresses that an earlier, freed allocation of the owner
// had been exported from; with exported buffers never freed, none. Round 2's
// wrong results (peers reading stale bytes through a mapping of a freshly
// allocated buffer, their stores lost) are the same failure.
// Check, per buffer and round (each with a fresh per-communicator nonce):
// every rank stores a 16-byte word through its mapping of every peer's buffer
// (slot = its rank) and its own word into its own buffer (slot n), all in the
// check region after the used bytes; after a bootstrap barrier every rank
// checks the words its peers stored into its buffers and reads every peer's
// own word through its mappings. A wrong (owner, buffer) seen by anyone —
// agreed by an allgather — is re-exported: its owner allocates a new buffer
// (the old one held until the end, so the new one lands elsewhere), every
// peer closes the wrong mapping and opens the new handle, and the round
// repeats (at most 4). Only then does ncclCommInitRank fail (ncclSystemError).
// NBX_IPC_VERIFY_FAIL=<rank>:<buffer> (test hook) makes round 0 report that
// rank's buffer (0 LL, 1 LL128, 2 staging, 3 flags) wrong.
// A buffer the communicator does not have (LL128 with n > 8) is absent on
// every rank alike.
ncclResult_t mpConnect(ncclComm* c, const std::vector<MpInitInfo>& all) {
  MpState* mp = c->mp;
  const int n = c->nRanks, me = c->rank;
  ConnBuf* conn = mp->conn;
  std::vector<std::array<char*, kNumConn>> peer(n);
  std::vector<hipIpcMemHandle_t> cur((size_t)n * kNumConn);   // the handle each mapping was opened from
  for (int j = 0; j < n; j++)
    for (int t = 0; t < kNumConn; t++) cur[(size_t)j * kNumConn + t] = all[j].handle[t];
  auto open = [&](int j, int t) -> ncclResult_t {
    void* p = nullptr;
    HIPCHECK(hipIpcOpenMemHandle(&p, cur[(size_t)j * kNumConn + t], hipIpcMemLazyEnablePeerAccess));
    mp->peerMaps.push_back(p);
    peer[j][t] = (char*)p;
    return ncclSuccess;
  };
  for (int j = 0; j < n; j++)
    for (int t = 0; t < kNumConn; t++)
      if (j != me && conn[t].own) NCCLCHECK(open(j, t));
  int failRank = -1, failBuf = -1;
  if (const char* v = std::getenv("NBX_IPC_VERIFY_FAIL"); v && *v) std::sscanf(v, "%d:%d", &failRank, &failBuf);
  std::vector<void*> retired;
  ncclResult_t res = ncclSuccess;
  constexpr int kRounds = 4;
  for (int round = 0;; round++) {
    const uint64_t salt = 0x632be59bd9b4e019ull * (uint64_t)(round + 1);
    auto nonceOf = [&](int j, int t) { return all[j].nonce ^ salt ^ (0xd6e8feb86659fd93ull * (uint64_t)(t + 1)); };
    uint64_t w[2];
    for (int t = 0; t < kNumConn; t++) {
      if (!conn[t].own) continue;
      const uint64_t off = connCheckOff(conn[t].bytes);
      for (int j = 0; j < n; j++) {
        if (j == me) continue;
        checkWord(nonceOf(me, t), me, j, w);
        HIPCHECK(hipMemcpy(peer[j][t] + off + 16ull * (uint64_t)me, w, 16, hipMemcpyHostToDevice));
      }
      checkWord(nonceOf(me, t), me, n, w);
      HIPCHECK(hipMemcpy((char*)conn[t].own + off + 16ull * (uint64_t)n, w, 16, hipMemcpyHostToDevice));
    }
    HIPCHECK(hipDeviceSynchronize());
    std::vector<uint8_t> bad((size_t)n * kNumConn, 0), allBad((size_t)n * n * kNumConn);
    int32_t dummy = 0;
    std::vector<int32_t> gathered(n);
    NCCLCHECK(nbx::bootstrapAllGather(mp->bs, &dummy, sizeof(dummy), gathered.data()));   // every word stored
    std::vector<uint64_t> mine(2 * (size_t)(n + 1));
    for (int t = 0; t < kNumConn; t++) {
      if (!conn[t].own) continue;
      const uint64_t off = connCheckOff(conn[t].bytes);
      HIPCHECK(hipMemcpy(mine.data(), (char*)conn[t].own + off, 16ull * (uint64_t)(n + 1), hipMemcpyDeviceToHost));
      for (int j = 0; j < n; j++) {
        if (j == me) continue;
        checkWord(nonceOf(j, t), j, me, w);
        if (mine[2 * j] != w[0] || mine[2 * j + 1] != w[1]) {
          info("comm %p rank %d: rank %d's store through its mapping of my buffer %d did not land (round %d)",
               (void*)c, me, j, t, round);
          bad[(size_t)me * kNumConn + t] = 1;
        }
        uint64_t got[2];
        HIPCHECK(hipMemcpy(got, peer[j][t] + off + 16ull * (uint64_t)n, 16, hipMemcpyDeviceToHost));
        checkWord(nonceOf(j, t), j, n, w);
        if (got[0] != w[0] || got[1] != w[1]) {
          info("comm %p rank %d: my mapping of rank %d's buffer %d shows other bytes (round %d)", (void*)c, me, j, t,
               round);
          bad[(size_t)j * kNumConn + t] = 1;
        }
      }
    }
    if (round == 0 && failRank == me && failBuf >= 0 && failBuf < kNumConn && conn[failBuf].own)
      bad[(size_t)me * kNumConn + failBuf] = 1;
    NCCLCHECK(nbx::bootstrapAllGather(mp->bs, bad.data(), bad.size(), allBad.data()));
    for (int q = 0; q < n; q++)
      for (size_t i = 0; i < bad.size(); i++) bad[i] |= allBad[(size_t)q * bad.size() + i];
    int nBad = 0;
    for (uint8_t b : bad) nBad += b;
    if (nBad == 0) break;
    if (round + 1 == kRounds) {
      warn("ncclCommInitRank : %d peer mapping(s) still wrong after %d re-exports; giving up", nBad, kRounds - 1);
      res = ncclSystemError;
      break;
    }
    mp->ipcRepairs += nBad;
    // re-export: the owner of a wrong buffer allocates another (the old one held)
    struct Fresh {
      hipIpcMemHandle_t h[kNumConn];
    } fresh{};
    for (int t = 0; t < kNumConn; t++) {
      if (!bad[(size_t)me * kNumConn + t]) continue;
      retired.push_back(conn[t].own);
      conn[t].own = nullptr;
      NCCLCHECK(connAlloc(&conn[t], n, /*ipc=*/true));
      fresh.h[t] = conn[t].handle;
      info("comm %p rank %d: buffer %d re-exported at %p (round %d)", (void*)c, me, t, conn[t].own, round);
    }
    HIPCHECK(hipDeviceSynchronize());
    std::vector<Fresh> allFresh(n);
    NCCLCHECK(nbx::bootstrapAllGather(mp->bs, &fresh, sizeof(fresh), allFresh.data()));
    for (int j = 0; j < n; j++) {
      if (j == me) continue;
      for (int t = 0; t < kNumConn; t++) {
        if (!bad[(size_t)j * kNumConn + t]) continue;
        auto it = std::find(mp->peerMaps.begin(), mp->peerMaps.end(), (void*)peer[j][t]);
        if (it != mp->peerMaps.end()) mp->peerMaps.erase(it);
        HIPCHECK(hipIpcCloseMemHandle(peer[j][t]));
        cur[(size_t)j * kNumConn + t] = allFresh[j].h[t];
        NCCLCHECK(open(j, t));
      }
    }
  }
  for (void* q : retired) freeSyncMem(q, /*wrong=*/true);
  NCCLCHECK(res);
  // the device tables of peer buffers (own entry: own buffer)
  return connUploadTables(mp, n, [&](int j, int t) { return j == me ? conn[t].own : (void*)peer[j][t]; });
}

void mpFreeState(MpState* mp, int device) {
  DevGuard g(device);
  (void)hipDeviceSynchronize();
  for (void* p : mp->peerMaps) (void)hipIpcCloseMemHandle(p);
  for (int t = kNumConn - 1; t >= 0; t--)
    if (mp->conn[t].peersDev) (void)hipFree(mp->conn[t].peersDev);
  for (void* p : {(void*)mp->scounters, (void*)mp->llState, (void*)mp->orderMem, (void*)mp->probeSink})
    if (p) (void)hipFree(p);
  // the connection buffers: what peers may still have mapped stays allocated (allocSyncMem)
  // (after an abort or a device wait that gave up a peer's kernel may still store into them: kept, not reused)
  const bool failed = mp->hostWords != nullptr && (mp->hostWords[0] != 0 || mp->hostWords[1] != 0);
  for (int t = kNumConn - 1; t >= 0; t--) freeSyncMem(mp->conn[t].own, failed);
  for (hipEvent_t e : mp->groupEvents) (void)hipEventDestroy(e);
  nbx::bootstrapClose(mp->bs);
  delete mp;
}

void mpFree(ncclComm* c) {
  if (c->mp) mpFreeState(c->mp, c->device);
  if (c->lt) mpFreeState(c->lt, c->device);
  c->mp = nullptr;
  c->lt = nullptr;
}

}  // namespace nbxcomm
