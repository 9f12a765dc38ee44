// part_aggregate_body.inc -- the body of K8d (partition.h), shared as text by part_aggregate_kernel (FX = false, pp a
// KPartParams) and part_aggregate_fx_kernel (FX = true, pp a KPartParamsFx: plans with SLOT_SUM_FX slots), as
// scan_direct_body.inc is: the existing kernel keeps its code.  FX plans carry doubles (no val32 / packed records).
  extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
  const KParams& p = pp.base;
  const int tid = threadIdx.x;
  if (p.deadline && p.stats[STAT_TIMED_OUT]) return;
  const int PR = 1 << pp.pshift;
  const int ns = p.num_slots;
  // cs_pack: one word per key (LDS of PR words, part_aggregate_lds), COUNT + SUM from 0; else every slot's row
  for (int i = tid; i < (pp.cs_pack ? PR : ns * PR); i += kBlock) lds[i] = pp.cs_pack ? 0ull : slot_init(p.slot_kind[i / PR]);
  __syncthreads();
  const uint32_t r0 = pp.part_start[blockIdx.x], r1 = pp.part_start[blockIdx.x + 1];
  // COUNT + SUM in one LDS word per key (the table is PR words, 32 KB for C5: four workgroups per CU instead of
  // two), over chunks of records small enough that every key's count stays below 2^24 and its sum of offsets below
  // 2^40; the first chunk stores the partition's slice of both rows, later ones (a partition of more than ~10^9
  // offsets' worth of records) add to it -- the partition is this workgroup's alone.
  if (pp.cs_pack) {
    constexpr int NB = 16;
    const uint32_t* __restrict__ r32 = reinterpret_cast<const uint32_t*>(pp.rec_val);
    const uint32_t low = (1u << pp.pshift) - 1u;
    unsigned long long* w64 = reinterpret_cast<unsigned long long*>(lds);  // slot 0's words
    const uint64_t by_sum = (1ull << 40) / (uint64_t)(pp.pack_range > 0 ? pp.pack_range : 1);
    const uint32_t lim = (uint32_t)(by_sum < (1ull << 24) - 1 ? (by_sum > 0 ? by_sum : 1) : (1ull << 24) - 1);
    const int64_t G = p.num_keys_total;
    const int64_t k0 = (int64_t)blockIdx.x * PR;
    const int n = (int)(G - k0 < PR ? G - k0 : PR);
    uint32_t c0 = r0;
    do {
      const uint32_t c1 = r1 - c0 > lim ? c0 + lim : r1;
      if (c0 != r0) {
        for (int i = tid; i < PR; i += kBlock) lds[i] = 0ull;
        __syncthreads();
      }
      for (uint32_t base = c0 + tid; base < c1; base += NB * kBlock) {
        uint32_t wr[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const uint32_t r = base + b * kBlock;
          wr[b] = r32[r < c1 ? r : c0];
        }
#pragma unroll
        for (int b = 0; b < NB; ++b)
          if (base + b * kBlock < c1)
            atomicAdd(w64 + (wr[b] & low), (1ull << 40) | (unsigned long long)(wr[b] >> pp.pshift));
      }
      __syncthreads();
      const bool last = c1 >= r1;
      uint32_t present = 0;
      long long mn[2] = {INT64_MAX, INT64_MAX}, mx[2] = {INT64_MIN, INT64_MIN};
      for (int i = tid; i < n; i += kBlock) {
        const uint64_t w = lds[i];
        uint64_t cnt = w >> 40;
        uint64_t sum = (uint64_t)((int64_t)(w & ((1ull << 40) - 1)) + (int64_t)cnt * pp.pack_min);
        if (c0 == r0) {
          p.table[k0 + i] = cnt;      // COUNT (slot 0)
          p.table[G + k0 + i] = sum;  // SUM
        } else {
          cnt += p.table[k0 + i];
          sum += p.table[G + k0 + i];
          p.table[k0 + i] = cnt;
          p.table[G + k0 + i] = sum;
        }
        if (last && pp.chunk_cnt && cnt) {  // the compaction's count pass, from the words in hand
          ++present;
          mn[0] = min(mn[0], (long long)cnt);
          mx[0] = max(mx[0], (long long)cnt);
          mn[1] = min(mn[1], (long long)sum);
          mx[1] = max(mx[1], (long long)sum);
        }
      }
      if (last && pp.chunk_cnt) {  // workgroup-uniform
        __shared__ unsigned long long red_cnt[kBlock / 64];
        __shared__ long long red_mm[kBlock / 64][4];
        const int lane = tid & 63, wv = tid >> 6;
        unsigned long long c = present;
        for (int off = 32; off > 0; off >>= 1) {
          c += __shfl_xor(c, off);
          for (int s = 0; s < 2; ++s) {
            mn[s] = min(mn[s], (long long)__shfl_xor(mn[s], off));
            mx[s] = max(mx[s], (long long)__shfl_xor(mx[s], off));
          }
        }
        if (lane == 0) {
          red_cnt[wv] = c;
          red_mm[wv][0] = mn[0];
          red_mm[wv][1] = mn[1];
          red_mm[wv][2] = mx[0];
          red_mm[wv][3] = mx[1];
        }
        __syncthreads();
        if (tid < 4) {
          long long v = tid < 2 ? INT64_MAX : INT64_MIN;
          for (int w = 0; w < kBlock / 64; ++w) v = tid < 2 ? min(v, red_mm[w][tid]) : max(v, red_mm[w][tid]);
          pp.chunk_mm[4 * (int64_t)blockIdx.x + tid] = v;
        }
        if (tid == 0) {
          unsigned long long t = 0;
          for (int w = 0; w < kBlock / 64; ++w) t += red_cnt[w];
          pp.chunk_cnt[blockIdx.x] = (uint32_t)t;
        }
      }
      __syncthreads();  // the words are read before the next chunk clears them
      c0 = c1;
    } while (c0 < r1);
    return;
  }
  // Two workgroups per CU (the LDS table), so latency is hidden by loads in flight per lane: NB records per lane
  // per step, every load issued unconditionally (records past r1 re-read record r0 and are not accumulated).
  constexpr int NB = 16;
  for (uint32_t base = r0 + tid; base < r1; base += NB * kBlock) {
    uint32_t ri[NB];
    int k[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const uint32_t r = base + b * kBlock;
      ri[b] = r < r1 ? r : r0;
    }
    int64_t pv[NB];  // fine_pack: the records' values
    if (pp.fine_pack) {
      const uint32_t* __restrict__ r32 = reinterpret_cast<const uint32_t*>(pp.rec_val);
      const uint32_t low = (1u << pp.pshift) - 1u;
      uint32_t wr[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) wr[b] = r32[ri[b]];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        k[b] = (int)(wr[b] & low);
        pv[b] = pp.pack_min + (int64_t)(wr[b] >> pp.pshift);
      }
    } else {
#pragma unroll
      for (int b = 0; b < NB; ++b) k[b] = pp.rec_key[ri[b]];
    }
    for (int s = 0; s < ns; ++s) {
      const int kind = p.slot_kind[s];
      const int st = pp.slot_stream[s];
      if (FX && kind == SLOT_SUM_FX) {
        // the W digit slots of one column (adjacent, digits 0 .. W - 1): the record's double is loaded once and its
        // digits come off the chain of fx_sum.h in registers, each added to its slot's row as a 64-bit integer
        const KFxSplit& fx = part_fx(pp);
        if (fx.j[s] != 0) continue;  // added with the column's digit 0
        const int K = fx.k[s];
        const uint64_t* __restrict__ r64 = pp.rec_val + (int64_t)st * pp.rec_cap;
        double t[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) t[b] = ldexp(__longlong_as_double((long long)r64[ri[b]]), (int)fx.sh[s]);
        for (int j = 0; s + j < ns && p.slot_kind[s + j] == SLOT_SUM_FX && fx.j[s + j] == j; ++j) {
          unsigned long long* row = reinterpret_cast<unsigned long long*>(lds + (int64_t)(s + j) * PR);
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            const double d = trunc(t[b]);
            if (base + b * kBlock < r1) atomicAdd(row + k[b], (unsigned long long)(long long)d);
            t[b] = ldexp(t[b] - d, K);
          }
        }
        continue;
      }
      uint64_t w[NB];
      if (st < 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) w[b] = 0ull;
      } else if (pp.fine_pack) {
#pragma unroll
        for (int b = 0; b < NB; ++b) w[b] = (uint64_t)pv[b];
      } else if (pp.val32) {
        const int32_t* __restrict__ r32 = reinterpret_cast<const int32_t*>(pp.rec_val) + (int64_t)st * pp.rec_cap;
#pragma unroll
        for (int b = 0; b < NB; ++b) w[b] = (uint64_t)(int64_t)r32[ri[b]];
      } else {
        const uint64_t* __restrict__ r64 = pp.rec_val + (int64_t)st * pp.rec_cap;
#pragma unroll
        for (int b = 0; b < NB; ++b) w[b] = r64[ri[b]];
      }
#pragma unroll
      for (int b = 0; b < NB; ++b)
        if (base + b * kBlock < r1)
          accumulate<MODE_LDS>(lds + (int64_t)s * PR, k[b], kind, (int64_t)w[b], __longlong_as_double((long long)w[b]));
    }
  }
  __syncthreads();
  const int64_t G = p.num_keys_total;
  const int64_t k0 = (int64_t)blockIdx.x * PR;
  const int n = (int)(G - k0 < PR ? G - k0 : PR);
  for (int s = 0; s < ns; ++s)
    for (int i = tid; i < n; i += kBlock) p.table[(int64_t)s * G + k0 + i] = lds[(int64_t)s * PR + i];
