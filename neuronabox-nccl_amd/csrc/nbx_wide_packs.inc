// Body of kWidePacks / kWidePacksStats (nbx_wide.h): `a`, `slots`, STATS.
  using E = typename W::Elt;
  constexpr int EPP = W::kEPP, Q = EPP / 4;
  static_assert(!PART || NSRC >= 2, "a pass that reads a partial folds at least one more source");
  WideLaneStats ls;   // STATS only: the plain kernel never names it
  if constexpr (STATS) ls.reset();
  acquirePeerData(a);   // a clique's fold reads its peers' buffers (reduceMultiWideEx)
  const float sc = loadWideArg(a.argPtr, a.arg);
  const uint64_t head = (uint64_t)a.headElts;
  const u32x4* src[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; s++)
    src[s] = (const u32x4*)((const char*)a.src[s] + head * (PART && s == 0 ? sizeof(float) : sizeof(E)));
  u32x4* dst[kMaxKDsts];
#pragma unroll
  for (int d = 0; d < kMaxKDsts; d++) dst[d] = (u32x4*)((char*)a.dst[d] + head * (OUT32 ? sizeof(float) : sizeof(E)));
  const int nDsts = a.nDsts;
  const bool pre = a.preMask != 0;   // uniform: the fold is chosen per tile, never per element
  float mul[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; s++) mul[s] = ((a.preMask >> s) & 1u) ? sc : 1.0f;
  const uint64_t n = a.nPacks;
  constexpr uint64_t kTile = (uint64_t)U * kBlock;
  forEachTile(a, (n + kTile - 1) / kTile, [&](uint64_t t) {
    const uint64_t p = t * kTile + threadIdx.x;
    if (p + (uint64_t)(U - 1) * kBlock < n) {
      // full tile: issue every load first, then fold
      u32x4 part[U][Q];
      u32x4 v[NSRC][U];
      wideLoadTile<W, NSRC, U, PART>(part, v, src, p);
      __builtin_amdgcn_sched_barrier(0);
      if (pre) NBX_WIDE_FOLD(U, PART, true, part, v, mul, dst, nDsts, p);
      else NBX_WIDE_FOLD(U, PART, false, part, v, mul, dst, nDsts, p);
    } else {
      // last, partial tile
#pragma unroll
      for (int u = 0; u < U; u++) {
        const uint64_t q = p + (uint64_t)u * kBlock;
        if (q < n) {
          u32x4 part1[1][Q];
          u32x4 v1[NSRC][1];
          wideLoadTile<W, NSRC, 1, PART>(part1, v1, src, q);
          NBX_WIDE_FOLD(1, PART, true, part1, v1, mul, dst, nDsts, q);
        }
      }
    }
    if constexpr (STATS) wideStatsFlush(ls, slots + t * (kBlock / 64) + (threadIdx.x >> 6));
  });

  // head (< EPP elements before the aligned body) and tail (< EPP after it)
  if (blockIdx.x == gridDim.x - 1) {
    const int h = a.headElts;
    const uint64_t tailStart = head + n * EPP;
    const int tail = (int)(a.nElts - tailStart);
    const int t = (int)threadIdx.x;
    if (t < h) NBX_WIDE_ELT(a, sc, NSRC, (uint64_t)t);
    else if (t < h + tail) NBX_WIDE_ELT(a, sc, NSRC, tailStart + (uint64_t)(t - h));
    // h + tail < 2 * EPP <= 32 lanes: all of them in wave 0
    if constexpr (STATS)
      if (t < 64) wideStatsFlush(ls, slots + (n + kTile - 1) / kTile * (kBlock / 64));
  }
