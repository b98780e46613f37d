// Body of kWideShiftedLds / kWideShiftedLdsStats (nbx_wide.h): `a`, `slots`, STATS.
  using E = typename W::Elt;
  constexpr int EPP = W::kEPP, Q = EPP / 4;
  static_assert(!PART || NSRC >= 2, "a pass that reads a partial folds at least one more source");
  static_assert(kShiftLdsWaves * 64 == kBlock, "the head and tail elements count on kBlock lanes");
  constexpr int F = PART ? 1 : 0;   // first staged source
  constexpr int NST = NSRC - F;     // staged sources
  constexpr int U = shiftLdsUnroll(NSRC), S = kShiftLdsStages, WV = kShiftLdsWaves;
  constexpr int P = U * 64 + 1;     // packs per source per stage
  constexpr uint64_t kTile = (uint64_t)U * 64;
  __shared__ u32x4 sm[WV][S][NST][P];
  WideLaneStats ls;   // STATS only: the plain kernel never names it
  if constexpr (STATS) ls.reset();
  acquirePeerData(a);
  const float sc = loadWideArg(a.argPtr, a.arg);
  const uint64_t head = (uint64_t)a.headElts;
  const uint64_t n = a.nPacks;
  const u32x4* base[NSRC];
  uint32_t sh[NSRC];
  uint64_t lim[NSRC];
#pragma unroll
  for (int s = F; s < NSRC; s++) {
    alignDown16((uintptr_t)a.src[s] + head * sizeof(E), base[s], sh[s]);
    lim[s] = sh[s] ? n : (n ? n - 1 : 0);
  }
  const u32x4* partial = (const u32x4*)((const char*)a.src[0] + head * sizeof(float));   // PART only
  u32x4* dst[kMaxKDsts];
#pragma unroll
  for (int d = 0; d < kMaxKDsts; d++) dst[d] = (u32x4*)((char*)a.dst[d] + head * (OUT32 ? sizeof(float) : sizeof(E)));
  const int nDsts = a.nDsts;
  const bool pre = a.preMask != 0;   // uniform: the fold is chosen per tile, never per element
  float mul[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; s++) mul[s] = ((a.preMask >> s) & 1u) ? sc : 1.0f;
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
  const uint64_t nTiles = (n + kTile - 1) / kTile;
  const uint64_t nWaves = (uint64_t)gridDim.x * WV, gw = (uint64_t)blockIdx.x * WV + (uint64_t)wave;
  auto issue = [&](uint64_t t, int st) {
    const uint64_t p0 = t * kTile;
#pragma unroll
    for (int s = F; s < NSRC; s++) {
#pragma unroll
      for (int u = 0; u < U; u++) {
        const uint64_t q = p0 + (uint64_t)(u * 64 + lane);
        __builtin_amdgcn_global_load_lds((const void*)(base[s] + (q < lim[s] ? q : lim[s])),
                                         (__attribute__((address_space(3))) void*)&sm[wave][st][s - F][u * 64], 16, 0,
                                         2 /* nt */);
      }
      if (lane == 0) {
        const uint64_t q = p0 + kTile;
        __builtin_amdgcn_global_load_lds((const void*)(base[s] + (q < lim[s] ? q : lim[s])),
                                         (__attribute__((address_space(3))) void*)&sm[wave][st][s - F][kTile], 16, 0,
                                         2);
      }
    }
  };
  // the fp32 partial of wave tile t (lanes past the body read its last pack)
  auto loadPart = [&](uint64_t t, u32x4 (&part)[U][Q]) {
    if constexpr (PART) {
#pragma unroll
      for (int u = 0; u < U; u++) {
        const uint64_t q = t * kTile + (uint64_t)(u * 64 + lane);
        const uint64_t qc = q < n ? q : n - 1;
#pragma unroll
        for (int j = 0; j < Q; j++) part[u][j] = ldPack(partial + qc * Q + j);
      }
    }
  };
  // fold wave tile t from stage st (its DMA has landed) and store it
  auto foldTile = [&](uint64_t t, int st, const u32x4 (&part)[U][Q]) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint64_t q = t * kTile + (uint64_t)(u * 64 + lane);
      if (q < n) {
        u32x4 part1[1][Q];
        u32x4 v1[NSRC][1];
        if constexpr (PART) {
#pragma unroll
          for (int j = 0; j < Q; j++) part1[0][j] = part[u][j];
        }
#pragma unroll
        for (int s = F; s < NSRC; s++) {
          v1[s][0] = stageRead(&sm[wave][st][s - F][0], sh[s], (uint32_t)(u * 64 + lane));
        }
        if (pre) NBX_WIDE_FOLD(1, PART, true, part1, v1, mul, dst, nDsts, q);
        else NBX_WIDE_FOLD(1, PART, false, part1, v1, mul, dst, nDsts, q);
      }
    }
    // this stage's LDS reads have returned before a later iteration refills it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if constexpr (STATS) wideStatsFlush(ls, slots + t);   // one slot per wave tile
  };
#pragma unroll
  for (int k = 0; k < S - 1; k++) {
    const uint64_t t = gw + (uint64_t)k * nWaves;
    if (t < nTiles) issue(t, k);
  }
  int st = 0;
  for (uint64_t t = gw; t < nTiles; t += nWaves) {
    u32x4 part[U][Q];
    loadPart(t, part);
    if (t + (uint64_t)(S - 1) * nWaves < nTiles) {
      issue(t + (uint64_t)(S - 1) * nWaves, (st + S - 1) % S);
      // everything but the newer tiles' DMA (NST x (U + 1) instructions each)
      // has landed: this tile's DMA and its partial; stores counted in vmcnt
      // only make the wait stricter
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((S - 1) * NST * (U + 1)) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    foldTile(t, st, part);
    st = st + 1 == S ? 0 : st + 1;
  }

  // head (before the destinations' 16-B boundary) and tail elements
  if (blockIdx.x == gridDim.x - 1) {
    const int h = a.headElts;
    const uint64_t tailStart = head + n * EPP;
    const int tail = (int)(a.nElts - tailStart);
    const int th = (int)threadIdx.x;
    if (th < h) NBX_WIDE_ELT(a, sc, NSRC, (uint64_t)th);
    else if (th < h + tail) NBX_WIDE_ELT(a, sc, NSRC, tailStart + (uint64_t)(th - h));
    if constexpr (STATS)
      if (th < 64) wideStatsFlush(ls, slots + nTiles);
  }
