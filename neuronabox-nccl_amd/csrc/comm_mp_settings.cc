// comm_mp_settings.cc — every setting of a multi-rank transport, read from the
// environment and the communicator's config before anything is allocated:
// NCCL_PROTO / NCCL_ALGO and the per-message protocol choice, the reference's
// knobs, the layout of the connection buffers (mpSettings). No HIP calls.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <string>
#include <strings.h>
#include "nbx_comm.h"

namespace nbxcomm {

// NCCL_PROTO (tuning.cc:254-259, parseList): a comma-separated list of the
// enabled protocols among LL, LL128, Simple, or "^list" for all but those.
// Per message (per-rank block for ReduceScatter) the first enabled protocol
// whose buffer holds it is used: LL up to NBX_LL_MAX_BYTES (64 KiB), LL128 up
// to NBX_LL128_MAX_BYTES (1 MiB; n <= 8 ranks), else Simple (also the
// fallback when Simple is disabled and nothing else fits).
// Read when the communicator is created (as NCCL reads its tuning env at init).
int protoFromString(const char* v) {
  if (v == nullptr || *v == 0) return kProtoAll;
  bool exclude = v[0] == '^';
  std::string list(exclude ? v + 1 : v);
  int mask = 0;
  size_t pos = 0;
  while (pos <= list.size()) {
    size_t e = list.find(',', pos);
    if (e == std::string::npos) e = list.size();
    std::string tok = list.substr(pos, e - pos);
    if (strcasecmp(tok.c_str(), "ll") == 0) mask |= kProtoLL;
    else if (strcasecmp(tok.c_str(), "ll128") == 0) mask |= kProtoLL128;
    else if (strcasecmp(tok.c_str(), "simple") == 0) mask |= kProtoSimple;
    else if (!tok.empty()) warn("NCCL_PROTO: unknown protocol '%s' ignored", tok.c_str());
    pos = e + 1;
  }
  return exclude ? (kProtoAll & ~mask) : mask;
}

// LL128 across GPUs is enabled by default only where it was validated — the
// reference's rule (tuning.cc:250-297: protoEnable[LL128] = 2 "default", and
// parseList turns it into 1 only when NCCL_PROTO lists LL128; a "^list"
// leaves it at 2). LL128 trusts a 64-byte line written by one store to arrive
// whole; within one GPU that was stress-tested, over xGMI it has
// not been, so ranks on different GPUs drop LL128 from the default set until a
// node run validates it (DESIGN §6 states the flip rule). It stays on when
// NCCL_PROTO names it explicitly, or with NBX_LL128_ACROSS_GPUS=1.
// NBX_DEBUG_ASSUME_MULTI_GPU=1 (test hook) applies this gate to ranks that
// share a GPU, and nothing else of the multi-GPU settings.
bool protoLL128Explicit(const char* v) {
  if (v == nullptr || *v == 0 || v[0] == '^') return false;
  return (protoFromString(v) & kProtoLL128) != 0;
}
int protoGateAcrossGpus(int mask, bool multiGpu, const char* ncclProto) {
  const bool assume = envLong("NBX_DEBUG_ASSUME_MULTI_GPU", 0) != 0;
  if (!(multiGpu || assume) || protoLL128Explicit(ncclProto)) return mask;
  if (envLong("NBX_LL128_ACROSS_GPUS", 0) != 0) return mask;
  return mask & ~kProtoLL128;
}

// Per message: LL up to the LL max; LL128 up to the LL128 max: one-shot (every
// rank pushes the whole message to every target), for AllReduce / Reduce with
// more than 2 ranks only up to the one-shot max and the two-shot AllReduce /
// Reduce (reduce-scatter + gather hops, a rank's block in half an LL128 slot)
// above it; else Simple. ReduceScatter is one hop by nature: one-shot up to
// the LL128 max.
// Lines per (parity, source) slot: holds maxBytes one-shot, and each half (a
// two-shot sub-slot) holds maxBytes / 2.
uint64_t l128SlotLinesFor(uint64_t maxBytes) {
  const uint64_t half = (maxBytes + 1) / 2;
  return 2 * ((half + nbx::kL128DataBytesHost - 1) / nbx::kL128DataBytesHost);
}
MpProto chooseProtoFor(int mask, bool twoShotKind, uint64_t slotBytes, uint64_t blockBytes, int n, uint64_t llMax,
                       uint64_t l128Max, uint64_t oneShotMax) {
  if (slotBytes == 0 || n > 64) return kMpSimple;
  if ((mask & kProtoLL) && slotBytes <= llMax) return kMpLL;
  if ((mask & kProtoLL128) && l128Max != 0 && n <= nbx::kL128MaxRanksHost) {
    if (!twoShotKind || n <= 2 || slotBytes <= oneShotMax) {
      if (slotBytes <= l128Max) return kMpLL128;
    } else if (slotBytes <= l128Max && blockBytes <= (l128SlotLinesFor(l128Max) / 2) * nbx::kL128DataBytesHost) {
      return kMpLL128x2;
    }
  }
  return kMpSimple;
}

// NCCL_ALGO (tuning.cc:254-259): "Ring" selects the ring schedule for the
// Simple protocol; anything else (default) the direct schedule.
// Read when the communicator is created.
static bool algoRingFromEnv() {
  const char* v = std::getenv("NCCL_ALGO");
  return v && strcasecmp(v, "ring") == 0;
}

long envLong(const char* name, long dflt) {
  const char* v = std::getenv(name);
  return (v && *v) ? std::atol(v) : dflt;
}

// NBX_WIDE_ACCUM=1: an unmodified NCCL program cannot call nbxRedOpCreateWide,
// so with it the built-in ncclSum / ncclAvg on f16, bf16 and fp8 take the
// fp32-accumulating operator on every communicator created under it (the
// ranks of one must agree: their kernels differ). Unset or 0: nothing changes.
bool wideAccumFromEnv() { return envLong("NBX_WIDE_ACCUM", 0) != 0; }

// The reference's own tuning knobs on this path, read at communicator
// creation like NCCL reads them (init.cc:523-541 computeBuffSizes,
// connect.cc:314-315, tuning.cc:12), each mapped onto the setting that plays
// its role here; the NBX_* variable of that setting, when set, wins:
//   NCCL_BUFFSIZE       Simple connection buffer per (peer, channel): the
//                       Simple staging per (peer, workgroup, region) is
//                       slots x slice, so slice = NCCL_BUFFSIZE / slots
//                       (NBX_SIMPLE_SLICE_BYTES) — only below the 64 KiB
//                       default (mpSettings);
//   NCCL_LL_BUFFSIZE    LL buffer: half of every 8-byte line is flag, so LL
//                       carries messages up to NCCL_LL_BUFFSIZE / 2 (NBX_LL_MAX_BYTES);
//   NCCL_LL128_BUFFSIZE LL128 buffer: 48 payload bytes per 64-byte line, so
//                       LL128 carries up to 3/4 of it (NBX_LL128_MAX_BYTES);
//   NCCL_MAX_NCHANNELS / NCCL_MIN_NCHANNELS  a channel is a workgroup here:
//                       the Simple grid (NBX_SIMPLE_MAX_GRID) and the LL /
//                       LL128 grids are capped at the max, and the Simple grid
//                       raised to the min (both within the co-residency cap).
// Unset, the measured defaults stay (64 KiB slices, 64 KiB LL, 1 MiB LL128,
// 128 Simple workgroups). NCCL_NTHREADS has no counterpart: every
// kernel is compiled for 256-thread workgroups (a warning says it is ignored).
long ncclEnvMapped(const char* nbxName, const char* ncclName, long dflt, long num, long den) {
  const char* v = std::getenv(nbxName);
  if (v && *v) return std::atol(v);
  const char* w = std::getenv(ncclName);
  if (w && *w && std::atol(w) > 0) return std::atol(w) / den * num;
  return dflt;
}

// Every environment-derived and layout field of one rank's transport among
// `n` ranks: the smallest GPU of the communicator has `minCus` CUs, at most
// `maxShare` ranks share one GPU, `multiGpu`: the ranks span more than one.
// minCTAs / maxCTAs / checkPointers: the communicator's (ncclComm).
void mpSettings(MpState* mp, int n, int minCus, int maxShare, bool multiGpu, int minCTAs, int maxCTAs,
                bool checkPointers) {
  // Grid caps and Simple settings. Simple grid: one workgroup per CU, all
  // co-resident (workgroup g of a rank waits on workgroup g of its peers);
  // ranks sharing a GPU split its CUs, and so do the LL family's spinning
  // grids (the env caps still apply on top).
  // connect.cc:418-422: channels = min(NCCL_MAX_NCHANNELS, config maxCTAs) and
  // at least max(NCCL_MIN_NCHANNELS, config minCTAs); a channel is a workgroup here
  long maxCh = envLong("NCCL_MAX_NCHANNELS", 0), minCh = envLong("NCCL_MIN_NCHANNELS", 0);
  if (maxCTAs != NCCL_CONFIG_UNDEF_INT && maxCTAs > 0) maxCh = maxCh > 0 ? std::min<long>(maxCh, maxCTAs) : maxCTAs;
  if (minCTAs != NCCL_CONFIG_UNDEF_INT && minCTAs > 0) minCh = std::max<long>(minCh, minCTAs);
  long g = envLong("NBX_SIMPLE_MAX_GRID", 0);
  if (g <= 0) {
    g = 128;
    if (maxCh > 0) g = std::min(g, maxCh);
    if (minCh > 0) g = std::max(g, minCh);
  }
  g = std::min<long>(g, std::max(1, minCus / maxShare));
  mp->llGridCap = (uint32_t)std::max(1, 4 * minCus / maxShare);
  mp->l128GridCap = (uint32_t)std::max(1, minCus / maxShare);
  if (maxCh > 0) {   // a channel is a workgroup here
    mp->llGridCap = std::min<uint32_t>(mp->llGridCap, (uint32_t)maxCh);
    mp->l128GridCap = std::min<uint32_t>(mp->l128GridCap, (uint32_t)maxCh);
  }
  mp->simpleGrid = (int)std::max<long>(1, std::min<long>(g, nbx::kSimpleMaxGrid));
  mp->slots = (int)std::max<long>(2, std::min<long>(envLong("NBX_SIMPLE_SLOTS", 2), 8));
  // NCCL_BUFFSIZE is the reference's buffer per (peer, channel) and its own
  // default is 4 MiB, which job scripts often set explicitly; here it would
  // become a 1 MiB slice per (peer, workgroup, region, slot) — 4 GiB of staging
  // at 8 ranks. So it is honoured only where it LOWERS the slice
  // below the 64 KiB default (a memory cap, its use in the reference); an
  // explicit NBX_SIMPLE_SLICE_BYTES sets the slice (16 B .. 1 MiB) as asked.
  long sl = envLong("NBX_SIMPLE_SLICE_BYTES", 0);
  if (sl <= 0) {
    sl = 64 << 10;
    const long bs = envLong("NCCL_BUFFSIZE", 0);
    if (bs > 0 && bs / mp->slots < sl) sl = bs / mp->slots;
    else if (bs > 0)
      info("NCCL_BUFFSIZE=%ld ignored: the Simple slice stays %ld bytes (only smaller buffers are honoured)", bs, sl);
  }
  sl = std::max<long>(nbx::kSimpleMinSliceBytes, std::min<long>(sl, 1 << 20));
  mp->sliceBytes = (uint64_t)(sl + 15) & ~(uint64_t)15;
  if (const char* nt = std::getenv("NCCL_NTHREADS"); nt && *nt && std::atol(nt) != 256)
    info("NCCL_NTHREADS=%s ignored: every kernel of this library runs 256-thread workgroups", nt);
  mp->simplePrefetch = envLong("NBX_SIMPLE_PREFETCH", 1) != 0;
  // Simple staging: the slices, then one 16-byte plan header per slice cell
  // (nbx_simple.h simpleHdr); flag words [4][n][grid]
  const uint64_t cells = (uint64_t)n * (uint64_t)mp->simpleGrid;
  mp->stageHdrOff = 2ull * (uint64_t)mp->slots * cells * mp->sliceBytes;
  mp->conn[kConnStage].bytes = mp->stageHdrOff + 2ull * (uint64_t)mp->slots * cells * 16u;
  mp->conn[kConnFlags].bytes = 4 * cells * sizeof(uint64_t);

  const char* t = std::getenv("NBX_TIMEOUT_SEC");
  if (t && std::atof(t) > 0) mp->timeoutSec = std::atof(t);
  mp->ring = algoRingFromEnv();
  mp->multiGpu = multiGpu;
  const char* ncclProto = std::getenv("NCCL_PROTO");
  mp->protoMask = protoGateAcrossGpus(protoFromString(ncclProto), multiGpu, ncclProto);
  mp->streamOrder = envLong("NBX_MP_STREAM_ORDER", 1) != 0;
  mp->groupBatch = envLong("NBX_GROUP_BATCH", 1) != 0;
  // Plan checks (nbx_ll.h plan words, nbx_simple.h slice headers): a launch
  // fails, naming the peer, when ranks issue mismatched calls or cut a group
  // differently — instead of a timeout or folded misplaced data. Off unless
  // asked for (NBX_CHECK_PLANS=1, or the reference's own argument-checking
  // knob NCCL_CHECK_POINTERS=1): they cost 0.7-1.9 us per small call on the
  // shared-GPU rig, and the reference does not check this either.
  mp->checkPlans = envLong("NBX_CHECK_PLANS", checkPointers ? 1 : 0) != 0;
  // Slice checksums (nbx_simple.h): every Simple staging slice carries a hash of
  // its elements that the consumer recomputes from what it read; a difference
  // (a slot read before its stores landed, a stale or misplaced slice) fails
  // the launch naming the peer and slot use. A debug knob: the producer and
  // consumer hash every element (off by default; equal on every rank).
  mp->checkSlices = envLong("NBX_CHECK_SLICES", 0) != 0;
  mp->sliceFaultRank = (int)envLong("NBX_DEBUG_SLICE_FAULT", -1);
  mp->wideAccum = wideAccumFromEnv();
  // LL buffer: 2 parities x n sources x 2 lines per 8-byte pack
  {
    uint64_t mx = (uint64_t)ncclEnvMapped("NBX_LL_MAX_BYTES", "NCCL_LL_BUFFSIZE", 64 << 10, 1, 2);
    mx = (mx + 15) & ~(uint64_t)15;
    if (mx < 1024) mx = 1024;
    mp->llMaxBytes = mx;
    mp->llSlotLines = 2 * (mx / 8);
    mp->llDoneOff = 2 * (uint64_t)n * mp->llSlotLines;
    mp->llPlanOff = mp->llDoneOff + (uint64_t)n + 1;
    mp->conn[kConnLL].bytes = (mp->llPlanOff + 2 * (uint64_t)n) * sizeof(uint64_t);
  }
  // LL128 buffer: 2 parities x n sources x 64-byte lines of 48 payload bytes (n <= 8)
  if (n <= nbx::kL128MaxRanksHost) {
    // 1 MiB: where Simple overtakes LL128 (48 payload bytes per 64-byte line) on
    // the shared-GPU rig — 2 ranks: 1 MiB 15.4 vs 15.6 us, 2 MiB 25.8 vs 16.4,
    // 4 MiB 43.8 vs 18.7; 4 ranks: 2 MiB 34.5 vs 25.4 (profiles/r4/proto_sweep_r4z)
    uint64_t mx = (uint64_t)ncclEnvMapped("NBX_LL128_MAX_BYTES", "NCCL_LL128_BUFFSIZE", 1 << 20, 3, 4);
    mp->l128OneShotMax = (uint64_t)envLong("NBX_LL128_ONESHOT_MAX", 256 << 10);
    if (mx > (64u << 20)) mx = 64u << 20;   // keeps the buffer under the 4 GiB descriptor range
    if (mx != 0) {
      mx = (mx + 15) & ~(uint64_t)15;
      mp->l128MaxBytes = mx;
      mp->l128SlotLines = l128SlotLinesFor(mx);
      mp->conn[kConnL128].bytes = 2 * (uint64_t)n * mp->l128SlotLines * nbx::kL128LineBytesHost;
    }
  }
}

void mpSettingsValues(const MpState* mp, int64_t v[kNumSettingsValues]) {
  const int64_t s[kNumSettingsValues] = {
      (int64_t)mp->llMaxBytes, (int64_t)mp->l128MaxBytes, (int64_t)mp->sliceBytes, mp->slots, mp->simpleGrid,
      (int64_t)mp->llGridCap, (int64_t)mp->l128GridCap, mp->groupBatch, mp->ipcRepairs, mp->checkPlans,
      mp->checkSlices, mp->protoMask, mp->ring, (int64_t)mp->l128OneShotMax, (int64_t)mp->llSlotLines,
      (int64_t)mp->l128SlotLines, mp->wideAccum};
  std::copy(s, s + kNumSettingsValues, v);
}

}  // namespace nbxcomm

using namespace nbxcomm;

NBX_EXPORT int nbxDebugProtoMask(const char* ncclProto) { return protoFromString(ncclProto); }

// The protocol set a communicator starts from (before its LL128 self-test):
// NCCL_PROTO = ncclProto, its ranks on more than one GPU or not (the LL128
// gate above; NBX_LL128_ACROSS_GPUS and NBX_DEBUG_ASSUME_MULTI_GPU apply).
NBX_EXPORT int nbxDebugGatedProtoMask(const char* ncclProto, int multiGpu) {
  return protoGateAcrossGpus(protoFromString(ncclProto), multiGpu != 0, ncclProto);
}

NBX_EXPORT int nbxDebugChooseProto(int protoMask, int twoShotKind, uint64_t slotBytes, uint64_t blockBytes, int nRanks,
                                   uint64_t llMaxBytes, uint64_t ll128MaxBytes, uint64_t ll128OneShotMax) {
  return (int)chooseProtoFor(protoMask, twoShotKind != 0, slotBytes, blockBytes, nRanks, llMaxBytes, ll128MaxBytes,
                             ll128OneShotMax);
}

// mpSettings on given inputs, without a communicator or a GPU (nbx_debug.h).
NBX_EXPORT int nbxDebugTransportSettings(int nRanks, int minCus, int maxShare, int multiGpu, int minCTAs, int maxCTAs,
                                         int checkPointers, int64_t* out, int nOut) {
  if (out == nullptr || nRanks < 2 || nRanks > kMaxMpRanks || minCus < 1 || maxShare < 1) return -1;
  MpState mp;
  mpSettings(&mp, nRanks, minCus, maxShare, multiGpu != 0, minCTAs, maxCTAs, checkPointers != 0);
  int64_t v[kNumSettingsValues];
  mpSettingsValues(&mp, v);
  int k = 0;
  for (; k < nOut && k < kNumSettingsValues; k++) out[k] = v[k];
  return k;
}
