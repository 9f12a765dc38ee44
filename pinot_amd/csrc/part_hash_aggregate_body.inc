// part_hash_aggregate_body.inc -- the body of K8h (partition.h), shared as text by part_hash_aggregate_kernel
// (FX = false, pp a KPartParams) and part_hash_aggregate_fx_kernel (FX = true, pp a KPartParamsFx), as
// part_aggregate_body.inc is.
  extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
  const KParams& p = pp.base;
  const int tid = threadIdx.x, lane = tid & 63;
  if (p.deadline && p.stats[STAT_TIMED_OUT]) return;
  const int S = 1 << pp.sbits;
  const int ns = p.num_slots, nst = pp.num_streams;
  uint32_t* keys = reinterpret_cast<uint32_t*>(lds + (size_t)ns * S);
  __shared__ uint32_t pending;
  __shared__ uint32_t wave_tot[kBlock / 64];
  __shared__ unsigned long long blk_base;
  // this partition's range of every slot's words over all rounds (order-preserving u64: min at [s], max at [ns + s])
  __shared__ unsigned long long blk_mm[2 * kMaxSlots];
  if (pp.out_mm)
    for (int i = tid; i < 2 * ns; i += kBlock) blk_mm[i] = i < ns ? ~0ull : 0ull;
  const uint32_t r0 = pp.part_start[blockIdx.x];
  uint32_t n = pp.part_start[blockIdx.x + 1] - r0;
  const int64_t cap = pp.rec_cap;
  constexpr int NB = 8;
  // COUNT + SUM in one LDS word (slot 0's row) when the partition's records bound both halves (uniform per
  // workgroup): (1 << 40) | (value - pack_min) per record, split when the round's groups are written
  const bool cs = pp.cs_pack && n < (1u << 24) && (uint64_t)n * (uint64_t)pp.pack_range < (1ull << 40);
  while (n > 0) {
    for (int i = tid; i < S; i += kBlock) keys[i] = ~0u;
    for (int i = tid; i < ns * S; i += kBlock) lds[i] = slot_init(p.slot_kind[i >> pp.sbits]);
    if (tid == 0) pending = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += NB * kBlock) {
      uint32_t key[NB];  // hashed keys
      uint64_t v[NB][kHashPartStreams];
      uint32_t w32[NB];  // fine_pack: the packed records as read (written back as they are when left pending)
      if (pp.fine_pack) {
        const uint32_t* __restrict__ r32 = reinterpret_cast<const uint32_t*>(pp.rec_val);
        const int lb = 32 - pp.pbits;
        const uint32_t hi = (uint32_t)blockIdx.x << lb, hlow = (1u << lb) - 1u;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const uint32_t i = base + b * kBlock + tid;
          w32[b] = r32[r0 + (i < n ? i : 0u)];
          key[b] = i < n ? hi | (w32[b] & hlow) : ~0u;
          v[b][0] = (uint64_t)(pp.pack_min + (int64_t)(w32[b] >> lb));
#pragma unroll
          for (int st = 1; st < kHashPartStreams; ++st) v[b][st] = 0ull;
        }
      } else {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const uint32_t i = base + b * kBlock + tid;
          const uint32_t r = r0 + (i < n ? i : 0u);
          w32[b] = 0;
          key[b] = i < n ? pp.rec_key32[r] : ~0u;
#pragma unroll
          for (int st = 0; st < kHashPartStreams; ++st)
            v[b][st] = st >= nst ? 0ull
                       : pp.val32 ? (uint64_t)(int64_t)reinterpret_cast<const int32_t*>(pp.rec_val)[st * cap + r]
                                  : pp.rec_val[st * cap + r];
        }
      }
      __syncthreads();  // the batch is in registers before any record of it is overwritten by a pending one
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (key[b] == ~0u) continue;
        const int slot = lds_hash_slot(keys, key[b], pp.pbits, pp.sbits);
        if (slot < 0) {
          const uint32_t at = r0 + atomicAdd(&pending, 1u);
          if (pp.fine_pack) {
            reinterpret_cast<uint32_t*>(pp.rec_val)[at] = w32[b];
            continue;
          }
          pp.rec_key32[at] = key[b];
#pragma unroll
          for (int st = 0; st < kHashPartStreams; ++st)
            if (st < nst) {
              if (pp.val32) reinterpret_cast<uint32_t*>(pp.rec_val)[st * cap + at] = (uint32_t)v[b][st];
              else pp.rec_val[st * cap + at] = v[b][st];
            }
          continue;
        }
        if (cs) {
          atomicAdd(reinterpret_cast<unsigned long long*>(lds) + slot,
                    (1ull << 40) | (unsigned long long)((int64_t)v[b][0] - pp.pack_min));
          continue;
        }
        for (int s = 0; s < ns; ++s) {
          const int st = pp.slot_stream[s];
          uint64_t w = 0;
#pragma unroll
          for (int j = 0; j < kHashPartStreams; ++j)
            if (j == st) w = v[b][j];
          if (FX && p.slot_kind[s] == SLOT_SUM_FX) {
            // the column's W adjacent digit slots from the one operand word in registers (fx_sum.h's chain); a record
            // left pending above went back as that word, so a later round splits it again
            const KFxSplit& fx = part_fx(pp);
            if (fx.j[s] != 0) continue;  // added with the column's digit 0
            const int K = fx.k[s];
            double t = ldexp(__longlong_as_double((long long)w), (int)fx.sh[s]);
            for (int j = 0; s + j < ns && p.slot_kind[s + j] == SLOT_SUM_FX && fx.j[s + j] == j; ++j) {
              const double d = trunc(t);
              atomicAdd(reinterpret_cast<unsigned long long*>(lds + (int64_t)(s + j) * S) + slot, (unsigned long long)(long long)d);
              t = ldexp(t - d, K);
            }
            continue;
          }
          accumulate<MODE_LDS>(lds + (int64_t)s * S, slot, p.slot_kind[s], (int64_t)w,
                               __longlong_as_double((long long)w));
        }
      }
    }
    __syncthreads();
    // append this round's groups with one reservation per workgroup (a single global counter: per-wave atomics
    // would queue 4 x 2^sbits / 256 of them per partition at one address): waves count their entries by ballot, the
    // workgroup reserves their sum, each wave writes a contiguous run
    uint32_t mine = 0;
    for (int i0 = 0; i0 < S; i0 += kBlock) {
      const int i = i0 + tid;
      mine += (uint32_t)__popcll(__ballot(i < S && keys[i] != ~0u));
    }
    if (lane == 0) wave_tot[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0) {
      uint32_t tot = 0;
      for (int w = 0; w < kBlock / 64; ++w) tot += wave_tot[w];
      blk_base = tot ? atomicAdd(pp.out_count, (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    uint64_t at = blk_base;
    for (int w = 0; w < (tid >> 6); ++w) at += wave_tot[w];
    // the slot ranges of the groups written, tracked in registers while writing them when there are few slots (the
    // compact result's widths; order-preserving u64), else by a pass over the table below
    constexpr int kMmRegs = 4;
    const bool mm_regs = pp.out_mm && ns <= kMmRegs;
    unsigned long long rlo[kMmRegs], rhi[kMmRegs];
#pragma unroll
    for (int s = 0; s < kMmRegs; ++s) {
      rlo[s] = ~0ull;
      rhi[s] = 0ull;
    }
    for (int i0 = 0; i0 < S; i0 += kBlock) {
      const int i = i0 + tid;
      const bool occ = i < S && keys[i] != ~0u;
      const uint64_t bal = __ballot(occ);
      if (occ) {
        const uint64_t r = at + (uint64_t)__popcll(bal & ((1ull << lane) - 1ull));
        uint64_t* o = pp.out_rec + r * (uint64_t)(1 + ns);
        const bool in_cap = r < (uint64_t)pp.out_cap;  // past it: counted, not written; finalize reports the overflow
        if (in_cap) o[0] = (uint64_t)(keys[i] * kHashInv);  // the composite key back from its hash
        if (cs) {
          const uint64_t w = lds[i], c = w >> 40;
          const uint64_t sum = (uint64_t)((int64_t)(w & ((1ull << 40) - 1)) + (int64_t)c * pp.pack_min);
          if (in_cap) {
            o[1] = c;
            o[2] = sum;
          }
          rlo[0] = min(rlo[0], (unsigned long long)(c ^ (1ull << 63)));
          rhi[0] = max(rhi[0], (unsigned long long)(c ^ (1ull << 63)));
          rlo[1] = min(rlo[1], (unsigned long long)(sum ^ (1ull << 63)));
          rhi[1] = max(rhi[1], (unsigned long long)(sum ^ (1ull << 63)));
        } else if (mm_regs) {
#pragma unroll
          for (int s = 0; s < kMmRegs; ++s)
            if (s < ns) {
              const uint64_t w = lds[(int64_t)s * S + i];
              if (in_cap) o[1 + s] = w;
              rlo[s] = min(rlo[s], (unsigned long long)(w ^ (1ull << 63)));
              rhi[s] = max(rhi[s], (unsigned long long)(w ^ (1ull << 63)));
            }
        } else if (in_cap) {
          for (int s = 0; s < ns; ++s) o[1 + s] = lds[(int64_t)s * S + i];
        }
      }
      at += (uint64_t)__popcll(bal);
    }
    if (mm_regs) {
#pragma unroll
      for (int s = 0; s < kMmRegs; ++s) {
        if (s >= ns) continue;
        unsigned long long lo = rlo[s], hi = rhi[s];
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long a = (unsigned long long)__shfl_xor((long long)lo, o);
          const unsigned long long b = (unsigned long long)__shfl_xor((long long)hi, o);
          lo = a < lo ? a : lo;
          hi = b > hi ? b : hi;
        }
        if (lane == 0) {
          atomicMin(&blk_mm[s], lo);
          atomicMax(&blk_mm[ns + s], hi);
        }
      }
    } else if (pp.out_mm) {  // many slots: per slot a pass over the round's entries, per wave one LDS atomic each
      for (int s = 0; s < ns; ++s) {
        unsigned long long lo = ~0ull, hi = 0ull;
        for (int i = tid; i < S; i += kBlock) {
          if (keys[i] == ~0u) continue;
          uint64_t w;
          if (cs) {
            const uint64_t x = lds[i], c = x >> 40;
            w = s == 0 ? c : (uint64_t)((int64_t)(x & ((1ull << 40) - 1)) + (int64_t)c * pp.pack_min);
          } else {
            w = lds[(int64_t)s * S + i];
          }
          const unsigned long long o = w ^ (1ull << 63);
          lo = o < lo ? o : lo;
          hi = o > hi ? o : hi;
        }
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long a = (unsigned long long)__shfl_xor((long long)lo, o);
          const unsigned long long b = (unsigned long long)__shfl_xor((long long)hi, o);
          lo = a < lo ? a : lo;
          hi = b > hi ? b : hi;
        }
        if (lane == 0) {
          atomicMin(&blk_mm[s], lo);
          atomicMax(&blk_mm[ns + s], hi);
        }
      }
    }
    __syncthreads();
    n = pending;
    __syncthreads();
  }
  if (pp.out_mm)
    for (int i = tid; i < 2 * ns; i += kBlock) pp.out_mm[(int64_t)blockIdx.x * 2 * ns + i] = blk_mm[i];
