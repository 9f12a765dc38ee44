// tile_split.h — the scan's split of a launch's tiles among its workgroups and the layout of its dynamic LDS block,
// written once for the kernel (scan_direct.h), the host that sizes and launches it (rt_plan.cpp, rt_exec.cpp) and the
// exhaustive host check (tools/tile_split_check.cpp).  Integer arithmetic only; needs nothing but <stdint.h>.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define PGPU_HD __host__ __device__
#else
#define PGPU_HD
#endif

namespace pgpu {

constexpr int kBlock = 256;                 // threads per workgroup (4 waves of 64)
constexpr int kMaxStack = 8;                // filter evaluation stack depth
constexpr int kWaveQ = 256;                 // direct kernel: per-wave queue of sparse matched docs (LDS, u32)
// STATS_LEAP2 bytes of a workgroup's tiles are buffered in LDS (one per tile and wave) until the end of its run: no
// workgroup of any launch takes more tiles than this (configure raises the grid of huge plans, set_slot_weights
// declines weights that would pass it)
constexpr int64_t kLeapLdsTiles = 4096;
// chunked runs are weighted by CU slot only in launches of at least this many tiles per workgroup
constexpr int64_t kSlotWeightMinShare = 32;
constexpr int kMaxCuSlots = 4;              // resident workgroups per CU the weights know of (KParams.slot_w)

// ------------------------------------------------------------------------------------------------ LDS layout
// filter_groupby_kernel's dynamic LDS block, byte offsets from its start:
//   [table (MODE_LDS: table_words u64)] [filter stack (general programs)] [per-wave match queues] [LEAP2 bytes]
// The plan's lds_bytes is `maps` for plans without LEAP2 statistics, `maps + scan_lds_maps_bytes(tiles)` with.
struct ScanLds {
  int64_t stack;   // u32 [kMaxStack][kBlock], absent in pure-AND plans
  int64_t queues;  // u32 [kBlock / 64][2][kWaveQ]: wave w's docs at w * 2 * kWaveQ, its segments kWaveQ further
  int64_t maps;    // u8 [tiles of the workgroup's run][kBlock / 64]
};
PGPU_HD inline ScanLds scan_lds_layout(int64_t table_words, bool pure_and) {
  ScanLds l;
  l.stack = table_words * 8;
  l.queues = l.stack + (pure_and ? 0 : (int64_t)kMaxStack * kBlock * 4);
  l.maps = l.queues + (int64_t)(kBlock / 64) * 2 * kWaveQ * 4;
  return l;
}
// bytes of the LEAP2 list for runs of at most `tiles` tiles (a multiple of 16)
PGPU_HD inline int64_t scan_lds_maps_bytes(int64_t tiles) { return (tiles * (kBlock / 64) + 15) & ~int64_t(15); }

// ------------------------------------------------------------------------------------------------ the split
struct TileRun {
  int64_t begin, end, step;  // tiles begin, begin + step, ... below end
  PGPU_HD int64_t count() const { return end > begin ? (end - begin + step - 1) / step : 0; }
};

// total weight of an XCD's workgroups [0, j) of its nx: those of slot s are [nx s / n, nx (s + 1) / n)
PGPU_HD inline int64_t slot_weight_cum(int64_t j, int64_t nx, int slot_n, const uint16_t* slot_w) {
  int64_t c = 0;
  for (int s = 0; s < slot_n; ++s) {
    const int64_t a = nx * s / slot_n, e = nx * (s + 1) / slot_n;
    c += (j <= a ? 0 : j < e ? j - a : e - a) * (int64_t)slot_w[s];
  }
  return c;
}

// The static run of workgroup `block` of `grid` in a launch of T tiles.  Grids that are a multiple of the 8 XCDs (and
// >= 64): workgroups b and b + 8 share an XCD (round-robin dispatch), XCD x takes the x-th eighth of the tiles, and its
// workgroups take contiguous runs of it (tile_chunks; weighted by CU slot when slot_n > 1) or its tiles in turn.
// Other grids: contiguous equal runs.  TS: the tiles split statically (T, or the claim base of the A/B build with
// run-time claims, which applies to chunked launches only).
PGPU_HD inline TileRun tile_split(int64_t block, int64_t grid, int64_t T, int tile_chunks, int slot_n,
                                  const uint16_t* slot_w, int64_t TS) {
  TileRun r;
  if (grid >= 64 && (grid & 7) == 0 && tile_chunks) {
    const int64_t x = block & 7, i = block >> 3, nx = grid >> 3;
    const int64_t lo = x * TS / 8, len = (x + 1) * TS / 8 - lo;
    if (slot_n > 1) {
      const int64_t tot = slot_weight_cum(nx, nx, slot_n, slot_w);
      r.begin = lo + len * slot_weight_cum(i, nx, slot_n, slot_w) / tot;
      r.end = lo + len * slot_weight_cum(i + 1, nx, slot_n, slot_w) / tot;
    } else {
      r.begin = lo + i * len / nx;
      r.end = lo + (i + 1) * len / nx;
    }
    r.step = 1;
  } else if (grid >= 64 && (grid & 7) == 0) {
    const int64_t x = block & 7;
    r.begin = x * T / 8 + (block >> 3);
    r.end = (x + 1) * T / 8;
    r.step = grid >> 3;
  } else {
    r.begin = block * T / grid;
    r.end = (block + 1) * T / grid;
    r.step = 1;
  }
  return r;
}

// ------------------------------------------------------------------------------------------------ host side
// Bounds of the longest run, in O(slots).  A run is floor(A + D) - floor(A) <= ceil(D) tiles, D its exact share:
//   equal shares (all three branches): D <= ceil(T / 8) / (grid / 8) or T / grid, so ceil(T / grid);
//   weighted: D = len w_s / tot with len <= ceil(T / 8), largest in the slot of the largest weight.
inline int64_t equal_run_bound(int64_t T, int64_t grid) { return grid > 0 ? (T + grid - 1) / grid : T; }
inline int64_t weighted_run_bound(int64_t T, int64_t grid, int slot_n, const uint16_t* slot_w) {
  const int64_t nx = grid >> 3, len = (T + 7) / 8;
  const int64_t tot = slot_weight_cum(nx, nx, slot_n, slot_w);
  int64_t w = 0;
  for (int s = 0; s < slot_n; ++s)
    if (nx * (s + 1) / slot_n > nx * s / slot_n && slot_w[s] > w) w = slot_w[s];
  return tot > 0 ? (len * w + tot - 1) / tot : len;
}

// The weights of a launch of T tiles on `grid` workgroups, a whole number S of them per CU: slot s weighs
// 1 + step (S - 1 - s) in 1/256ths (at most 16).  Returns S and fills slot_w, or 0 (equal shares) when the launch
// is not one the weights are for, or when its longest run could pass max_run tiles (what the plan reserved LDS for).
// The caller has checked what the launch itself decides (chunked, no run-time claims, alone on the CUs).
inline int slot_weights(int64_t T, int64_t grid, int num_cus, double step, int64_t max_run, uint16_t* slot_w,
                        bool* declined = nullptr) {
  if (declined) *declined = false;
  const int S = num_cus > 0 && grid % num_cus == 0 ? (int)(grid / num_cus) : 0;
  if (!(step > 0.0) || S < 2 || S > kMaxCuSlots || (grid & 7) || T < kSlotWeightMinShare * grid) return 0;
  uint16_t w[kMaxCuSlots];
  for (int s = 0; s < S; ++s) {
    const double q = (1.0 + step * (S - 1 - s)) * 256.0 + 0.5;
    w[s] = (uint16_t)(q < 4096.0 ? q : 4096.0);
  }
  if (weighted_run_bound(T, grid, S, w) > max_run) {
    if (declined) *declined = true;
    return 0;
  }
  for (int s = 0; s < S; ++s) slot_w[s] = w[s];
  return S;
}

// The most tiles any workgroup of any launch of a plan can take: the plan has at most tile_bound tiles and `grid`
// workgroups, and each of its launches has T <= tile_bound tiles on min(grid, T) workgroups, weighted (only possible
// with T >= kSlotWeightMinShare * grid, hence on the full grid) or not.  Both bounds grow with T.
inline int64_t scan_max_run(int64_t tile_bound, int64_t grid, int num_cus, double step) {
  const int64_t T = tile_bound > 1 ? tile_bound : 1;
  if (grid < 1) grid = 1;
  int64_t run = equal_run_bound(T, grid);
  uint16_t w[kMaxCuSlots];
  const int S = slot_weights(T, grid, num_cus, step, INT64_MAX, w);
  if (S) {
    const int64_t wr = weighted_run_bound(T, grid, S, w);
    if (wr > run) run = wr;
  }
  return run;
}

// The LEAP2 reservation of a plan, tiles per workgroup: scan_max_run with the plan's weights, or with equal shares
// where the weighted runs would pass the cap (set_slot_weights then declines them).  configure has made the grid
// large enough for the equal shares.
inline int64_t scan_leap_tiles(int64_t tile_bound, int64_t grid, int num_cus, double step) {
  const int64_t run = scan_max_run(tile_bound, grid, num_cus, step);
  return run <= kLeapLdsTiles ? run : scan_max_run(tile_bound, grid, num_cus, 0.0);
}

// The longest run of one launch, exactly: every workgroup's tile_split (O(grid x slots); introspection and checks,
// not the query path).
inline int64_t launch_longest_run(int64_t T, int64_t grid, int tile_chunks, int slot_n, const uint16_t* slot_w) {
  int64_t m = 0;
  for (int64_t b = 0; b < grid; ++b) {
    const int64_t c = tile_split(b, grid, T, tile_chunks, slot_n, slot_w, T).count();
    if (c > m) m = c;
  }
  return m;
}

}  // namespace pgpu
