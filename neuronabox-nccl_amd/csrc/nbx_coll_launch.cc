// nbx_coll_launch.cc — launchers of the collective kernels (nbx_internal.h):
// LL, LL128, LL128 two-shot (nbx_ll.h) and Simple (nbx_simple.h). Sequencing
// is device-resident; the communicator layer (comm_mp_launch.cc) builds the
// arguments and records the launch.
#include <cstdlib>
#include <mutex>

#include "nbx_launch.h"
#include "nbx_ll_args.h"

namespace nbx {
namespace {
// Workgroup cap of the LL-family kernels from an env knob, clamped to [1, 1024].
size_t gridCapFromEnv(const char* name, long dflt) {
  const char* v = std::getenv(name);
  long g = (v && *v) ? std::atol(v) : dflt;
  return (size_t)(g < 1 ? 1 : g > 1024 ? 1024 : g);
}

// one 8-byte pack per thread; NBX_LL_MAX_GRID caps the workgroups (default
// 1024), e.g. when several ranks share one GPU and every rank's grid must
// stay co-resident for the ranks' spinning blocks to make progress
size_t llMaxGrid() {
  static const size_t maxGrid = gridCapFromEnv("NBX_LL_MAX_GRID", 1024);
  return maxGrid;
}

// 64 lines (4 lanes each) per 256-thread workgroup, at most one workgroup per
// CU by default (every block of the grid co-resident on its GPU, so a block
// waiting for its peers' lines never holds back a block they wait for).
// NBX_LL128_MAX_GRID lowers the cap, e.g. when several ranks share one GPU.
size_t ll128MaxGrid() {
  static const size_t maxGrid = gridCapFromEnv("NBX_LL128_MAX_GRID", 256);
  return maxGrid;
}
constexpr size_t kLL128LinesPerBlock = 256 / kL128LanesHost;

const KernelSet* collKernels(ncclDataType_t dt, const nbxDevRedOpFull& op) {
  if ((int)dt < 0 || (int)dt >= kNumTypes || op.op < 0 || op.op >= kNumDevOps) return nullptr;
  return &table()[(int)dt][op.op];
}

// The fp32-accumulating kernels (nbx_wide_coll.h): their own table, so
// KernelSet and nbxKernelCount stay as they are.
WideCollTable g_wideColl;
std::once_flag g_wideCollOnce;
const WideCollSet* wideCollKernels(ncclDataType_t dt, const nbxDevRedOpFull& op) {
  std::call_once(g_wideCollOnce, [] {
    std::memset(&g_wideColl, 0, sizeof(g_wideColl));
    fillWideColl16(g_wideColl);
    fillWideColl8(g_wideColl);
  });
  if ((int)dt < 0 || (int)dt >= kNumTypes || !g_wideColl[(int)dt].valid) return nullptr;
  if ((op.op != nbxDevSum && op.op != nbxDevPreMulSum) || op.scalarArgIsPtr) return nullptr;
  return &g_wideColl[(int)dt];
}

// The one instantiation's scalar (FnWide): the PreMulSum's fp32 bits, 1.0f for a Sum.
template <class A>
void setWideScalarArg(A& a, const nbxDevRedOpFull& op) {
  a.arg = op.op == nbxDevPreMulSum ? (op.scalarArg & 0xffffffffull) : 0x3f800000ull;
  a.argPtr = nullptr;
}

// One LL-family launch: the plain kernel, or the one with plan words when
// a.planSig != 0; `units` packs or lines at unitsPerBlock per 256-thread
// workgroup, capped by the environment and by a.gridCap.
ncclResult_t launchLLFamily(ncclDataType_t dt, const nbxDevRedOpFull& op, LLArgs& a, const void* KernelSet::*plain,
                            const void* KernelSet::*checked, const void* WideCollSet::*widePlain,
                            const void* WideCollSet::*wideChecked, bool wide, uint64_t units, size_t unitsPerBlock,
                            size_t (*maxGrid)(), hipStream_t stream) {
  const void* kPlain = nullptr;
  const void* kChecked = nullptr;
  if (wide) {
    const WideCollSet* ws = wideCollKernels(dt, op);
    if (ws == nullptr) return ncclInvalidArgument;
    kPlain = ws->*widePlain;
    kChecked = ws->*wideChecked;
    setWideScalarArg(a, op);
  } else {
    const KernelSet* ks = collKernels(dt, op);
    if (ks == nullptr || !ks->valid) return ncclInvalidArgument;
    kPlain = ks->*plain;
    kChecked = ks->*checked;
    setScalarArg(a, op);
  }
  if (kPlain == nullptr || kChecked == nullptr) return ncclInvalidArgument;
  size_t grid = (units + unitsPerBlock - 1) / unitsPerBlock;
  if (grid < 1) grid = 1;
  if (grid > maxGrid()) grid = maxGrid();
  if (a.gridCap != 0 && grid > a.gridCap) grid = a.gridCap;
  void* args[] = {&a};
  hipError_t e = hipLaunchKernel(a.planSig != 0 ? kChecked : kPlain, dim3((unsigned)grid), dim3(256), args, 0, stream);
  return e != hipSuccess ? ncclUnhandledCudaError : ncclSuccess;
}
}  // namespace

ncclResult_t launchLLColl(ncclDataType_t dt, const nbxDevRedOpFull& op, LLArgs& a, hipStream_t stream, bool wide) {
  return launchLLFamily(dt, op, a, &KernelSet::ll, &KernelSet::llChk, &WideCollSet::ll, &WideCollSet::llChk, wide,
                        a.nPacks, 256, llMaxGrid, stream);
}

ncclResult_t launchLL128Coll(ncclDataType_t dt, const nbxDevRedOpFull& op, LLArgs& a, hipStream_t stream, bool wide) {
  return launchLLFamily(dt, op, a, &KernelSet::ll128, &KernelSet::ll128Chk, &WideCollSet::ll128,
                        &WideCollSet::ll128Chk, wide, a.nLines, kLL128LinesPerBlock, ll128MaxGrid, stream);
}

ncclResult_t launchLL128AllReduce2(ncclDataType_t dt, const nbxDevRedOpFull& op, LLArgs& a, uint64_t blockLines,
                                   hipStream_t stream, bool wide) {
  return launchLLFamily(dt, op, a, &KernelSet::ll128x2, &KernelSet::ll128x2Chk, &WideCollSet::ll128x2,
                        &WideCollSet::ll128x2Chk, wide, blockLines, kLL128LinesPerBlock, ll128MaxGrid, stream);
}

ncclResult_t launchSimple(ncclDataType_t dt, const nbxDevRedOpFull& op, SimpleArgs& a, unsigned grid, bool ring,
                          hipStream_t stream, bool wide) {
  const void* k = nullptr;
  if (wide) {
    const WideCollSet* ws = ring ? nullptr : wideCollKernels(dt, op);   // the ring moves partials: no wide form
    if (ws == nullptr) return ncclInvalidArgument;
    k = a.checkSlices ? ws->simpleChk : ws->simple;
  } else {
    const KernelSet* ks = collKernels(dt, op);
    if (ks == nullptr || !ks->valid) return ncclInvalidArgument;
    k = a.checkSlices ? (ring ? ks->simpleRingChk : ks->simpleChk) : (ring ? ks->simpleRing : ks->simple);
  }
  if (k == nullptr || grid < 1 || grid > (unsigned)a.gridMax || a.gridMax > kSimpleMaxGrid ||
      a.nRanks < 2 || a.nRanks > kSimpleMaxRanks)
    return ncclInvalidArgument;
  if (wide) setWideScalarArg(a, op);
  else setScalarArg(a, op);
  void* args[] = {&a};
  hipError_t e = hipLaunchKernel(k, dim3(grid), dim3(kBlock), args, 0, stream);
  return e != hipSuccess ? ncclUnhandledCudaError : ncclSuccess;
}
}  // namespace nbx
