// Body of kWideBatchList / kWideBatchListStats (nbx_wide.h): `a`, `slots`, STATS.
  using E = typename W::Elt;
  constexpr int EPP = W::kEPP, Q = EPP / 4;
  WideLaneStats ls;   // STATS only: the plain kernel never names it
  if constexpr (STATS) ls.reset();
  const float sc = loadWideArg(a.argPtr, a.arg);
  const uint32_t preMask = a.preMask;
  const bool pre = preMask != 0;   // uniform per launch: the fold is never chosen per element
  float mul[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; s++) mul[s] = ((preMask >> s) & 1u) ? sc : 1.0f;
  const uint64_t T = a.totalTiles, C = a.chunk, step = (uint64_t)gridDim.x * C;
  const int nRecs = a.nRecs, lane = (int)(threadIdx.x & 63u);
  int k = -1;
  uint64_t tBegin = 0, tEnd = 0, nElts = 0, n = 0;
  int nDsts = 1, head = 0;
  const E* sb[NSRC];
  void* db[kMaxKDsts];
  const u32x4* src[NSRC];
  u32x4* dst[kMaxKDsts];
  for (uint64_t c0 = (uint64_t)blockIdx.x * C; c0 < T; c0 += step) {
    const uint64_t c1 = c0 + C < T ? c0 + C : T;
    for (uint64_t tile = c0; tile < c1; tile++) {
      if (tile >= tEnd) {   // next bucket holding this tile (uniform per wave)
        for (int base = k + 1;; base += 64) {
          const int idx = base + lane;
          const uint64_t e = idx < nRecs ? (uint64_t)a.tileEnd[idx] : ~0ull;
          const uint64_t m = __ballot(e > tile);
          if (m != 0) {
            k = __builtin_amdgcn_readfirstlane(base + (int)__builtin_ctzll(m));
            break;
          }
        }
        const uint64_t* r = a.recs + (uint64_t)k * a.recWords;
        tBegin = r[0];
        tEnd = r[1];
        const uint64_t meta = r[2];
        nDsts = (int)(meta >> 60);
        nElts = meta & kBatchCountMask;
        head = (int)((meta >> 56) & 15u);
        n = (nElts - (uint64_t)head) / EPP;
#pragma unroll
        for (int s = 0; s < NSRC; s++) {
          sb[s] = (const E*)r[3 + s];
          src[s] = (const u32x4*)(sb[s] + head);
        }
#pragma unroll
        for (int d = 0; d < kMaxKDsts; d++) {
          db[d] = (void*)r[3 + NSRC + (d < nDsts ? d : 0)];
          dst[d] = (u32x4*)((char*)db[d] + (uint64_t)head * (OUT32 ? sizeof(float) : sizeof(E)));
        }
      }
      const uint64_t p = (tile - tBegin) * kBatchTilePacks + threadIdx.x;
      if (p < n) {
        u32x4 part[1][Q];   // no partial-first form: unused
        u32x4 v[NSRC][1];
#pragma unroll
        for (int s = 0; s < NSRC; s++) v[s][0] = ldPack(src[s] + p);
        // every load issued before the fold starts, as in kWidePacks (without
        // this the widening of the first sources is scheduled between the
        // loads, and a flat load's wait is a wait for all of them)
        __builtin_amdgcn_sched_barrier(0);
        if (pre) NBX_WIDE_FOLD(1, false, true, part, v, mul, dst, nDsts, p);
        else NBX_WIDE_FOLD(1, false, false, part, v, mul, dst, nDsts, p);
      }
      // one slot per tile and wave, record k's shifted by k: its own slot for
      // the head and tail elements closes the record's contiguous range
      if constexpr (STATS) wideStatsFlush(ls, slots + tile * (kBlock / 64) + (uint64_t)k + (threadIdx.x >> 6));
      if (tile == tEnd - 1) {   // the bucket's last tile: its head and tail elements
        const uint64_t tailStart = (uint64_t)head + n * EPP;
        const int tail = (int)(nElts - tailStart);
        const int th = (int)threadIdx.x;
        if (th < head) NBX_WIDE_BATCH_ELT(sb, db, nDsts, preMask, sc, (uint64_t)th);
        else if (th < head + tail)
          NBX_WIDE_BATCH_ELT(sb, db, nDsts, preMask, sc, tailStart + (uint64_t)(th - head));
        if constexpr (STATS)
          if (th < 64) wideStatsFlush(ls, slots + tEnd * (kBlock / 64) + (uint64_t)k);
      }
    }
  }
