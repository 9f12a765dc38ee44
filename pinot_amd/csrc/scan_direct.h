// scan_direct.h — the fused filter / group-by / aggregation scan (K1+K2+K3) with direct loads: the kernel of
// the path.  Instantiated per family and accumulator mode in k_direct.hip, from kScanInstances (internal.h).
#pragma once
#include "device.h"

namespace pgpu {

// numEntriesScannedInFilter of an AND of two scans A, B (AndDocIdIterator.java:40-67 over SVScanDocIdIterators):
// the iterators hand the scan back and forth, so each doc is scanned once, plus once more when the scanner at that
// doc matches it (the other iterator then evaluates the same doc).  Scanner after a doc: B after a doc A matches
// and B does not, A after a doc B matches, unchanged otherwise -- so only a group's first matching doc depends on
// the scanner the group is entered with.  Each lane builds the scanner state over its 32 docs (5-step segmented
// fill), counts its entries with the entry state the wave's ballots give it (the exit of the previous lane with a
// match), and the wave stores one byte for the rest: whether it has a match, its exit state, and the count
// difference at its first match between entering in B and in A (leap2_compose_kernel chains the bytes of a
// segment in doc order).  The byte goes to the workgroup's LDS list (one per tile and wave), stored to global
// memory once after the tile loop.  Returns the lane's entries (entering the wave in A).
__device__ __forceinline__ uint32_t leap2_entries(uint8_t* __restrict__ maps, int64_t slot, int lane, uint32_t a,
                                                  uint32_t b, uint32_t v) {
  a &= v;
  b &= v;
  const uint32_t e = a | b;
  // scanner after doc i: B (1) where the last matching doc <= i matched A only, A (0) otherwise -- the A-only docs'
  // ones carried up through the docs B does not match, by one addition (a set bit p of y inside a run of ~b ones
  // flips the run from p up, so (~b + y) ^ ~b marks it; y's own bits are put back for runs holding several)
  const uint32_t y = a & ~b, nb = ~b;
  const uint32_t fill = (nb & ((nb + y) ^ nb)) | y;
  const uint32_t before = fill << 1;  // scanner before each doc, entering in A
  uint32_t c = __popc(v) + __popc((a & ~before) | (b & before));
  const int f = e ? __builtin_ctz(e) : 0;
  const int d = e ? (int)((b >> f) & 1u) - (int)((a >> f) & 1u) : 0;  // entering in B instead, at the first match
  // wave-wide state from ballots only (scalar masks, no lane shuffles, no divergent branch)
  const uint64_t evm = __ballot(e != 0u), exm = __ballot(e != 0u && (fill >> 31));
  const uint64_t below = evm & ((1ull << lane) - 1ull);
  if (below && ((exm >> (63 - __builtin_clzll(below))) & 1ull)) c += d;
  uint32_t m = 0;
  if (evm) {
    const int first = __builtin_ctzll(evm), last = 63 - __builtin_clzll(evm);
    const int df = __builtin_amdgcn_readlane(d, first);  // the first matching lane's difference
    m = 1u | (uint32_t)(((exm >> last) & 1ull) << 1) | ((uint32_t)(df + 1) << 2);
  }
  if (lane == 0) maps[slot] = (uint8_t)m;  // an LDS slot: global stores inside the tile loop cost the loop registers
  return c;
}

// ---------------------------------------------------------------------------------------------- K3 fused
// DENSE: the plan expects dense tiles (estimated selectivity >= 1/4, rt_plan.cpp): wave-tiles with >= kDenseGroupMin matches
// decode whole groups of the group-by / aggregated columns (aggregate_group).  A separate instance because that
// path needs ~45 more VGPRs, which would halve the occupancy of the sparse path.
// LANE_BATCH: matched docs per aggregate_batch where a lane's 32-doc group has more than 2 -- 4 in the pure-AND sparse
// instance for plans of estimated selectivity >= 1/16 (C4's scan path at 15 %: 174 -> 150 us), 2 elsewhere (4 cost
// C3, where that path is rare, 1.5 % -- 710 -> 722 us -- and the dense instance's C2 2 %).
// FX: the instances of plans with fixed-point FLOAT / DOUBLE sums (SLOT_SUM_FX slots, fx_sum.h) -- kernels of their
// own (filter_groupby_fx_kernel, family SCAN_FX, with KParamsFx), so the others keep their registers and arguments.
// DC: the instances of plans with DISTINCTCOUNT aggregations (SLOT_DISTINCT slots and their side bitmaps) -- kernels of
// their own again (filter_groupby_dc_kernel, family SCAN_DC, with KParamsDc).
// HIST: the instances of plans with PERCENTILE aggregations (SLOT_PERCENTILE slots and their side histograms) --
// filter_groupby_hist_kernel, family SCAN_HIST, with KParamsHist.
// EXPR: the instances of plans with expression aggregations (slots that take a program's value, KExpr) --
// filter_groupby_expr_kernel, family SCAN_EXPR, with KParamsExpr.
// The kernels share their body as text (scan_direct_body.inc): a body function inlined into them changed the
// scalar register allocation of the existing instances.
#ifndef PGPU_MIN_WAVES
#define PGPU_MIN_WAVES 1
#endif
#ifndef PGPU_DENSE_MIN_WAVES
#define PGPU_DENSE_MIN_WAVES 4
#endif
#ifndef PGPU_SIMPLE_MIN_WAVES
#define PGPU_SIMPLE_MIN_WAVES 4
#endif
template <int MODE, bool DENSE, bool SIMPLE = false, bool PAIR = false, bool FAST = false, int LANE_BATCH = 2>
__global__ __launch_bounds__(kBlock, DENSE ? (SIMPLE ? PGPU_SIMPLE_MIN_WAVES : PGPU_DENSE_MIN_WAVES) : PGPU_MIN_WAVES) void filter_groupby_kernel(const KParams p) {
  constexpr bool FX = false;
  constexpr int DC = kSideNone;
#include "scan_direct_body.inc"
}

// The sparse (general filter programs and pure-AND ones alike) and the dense instance for plans with SLOT_SUM_FX slots.
template <int MODE, bool DENSE>
__global__ __launch_bounds__(kBlock, DENSE ? PGPU_DENSE_MIN_WAVES : PGPU_MIN_WAVES) void filter_groupby_fx_kernel(const KParamsFx p) {
  constexpr bool FX = true, SIMPLE = false, PAIR = false, FAST = false;
  constexpr int LANE_BATCH = 2, DC = kSideNone;
#include "scan_direct_body.inc"
}

// The sparse and the dense instance for plans with SLOT_DISTINCT slots (DISTINCTCOUNT): MODE_LDS and MODE_GLOBAL.
template <int MODE, bool DENSE>
__global__ __launch_bounds__(kBlock, DENSE ? PGPU_DENSE_MIN_WAVES : PGPU_MIN_WAVES) void filter_groupby_dc_kernel(const KParamsDc p) {
  constexpr bool FX = false, SIMPLE = false, PAIR = false, FAST = false;
  constexpr int LANE_BATCH = 2, DC = kSideBitmap;
#include "scan_direct_body.inc"
}

// The sparse and the dense instance for plans with SLOT_PERCENTILE slots (PERCENTILE, and DISTINCTCOUNT beside it):
// MODE_LDS and MODE_GLOBAL.
template <int MODE, bool DENSE>
__global__ __launch_bounds__(kBlock, DENSE ? PGPU_DENSE_MIN_WAVES : PGPU_MIN_WAVES) void filter_groupby_hist_kernel(const KParamsHist p) {
  constexpr bool FX = false, SIMPLE = false, PAIR = false, FAST = false;
  constexpr int LANE_BATCH = 2, DC = kSideHist;
#include "scan_direct_body.inc"
}

// The sparse and the dense instance for plans with expression aggregations (SUM(price * qty): KExpr, expr_eval.h).
// Sparse, in every accumulator mode: any filter program, matched docs aggregated in per-lane batches (aggregate_batch),
// where the operand columns of a program are gathered once per batch and the program is interpreted over a register
// stack.  Dense (MODE_LDS and MODE_GLOBAL): dense tiles decode whole groups, kExprStep = 4 docs of a lane's group per
// step (aggregate_step_expr).
template <int MODE, bool DENSE>
__global__ __launch_bounds__(kBlock, DENSE ? PGPU_DENSE_MIN_WAVES : PGPU_MIN_WAVES) void filter_groupby_expr_kernel(const KParamsExpr p) {
  constexpr bool FX = false, SIMPLE = false, PAIR = false, FAST = false;
  constexpr int LANE_BATCH = 2, DC = kSideExpr;
#include "scan_direct_body.inc"
}

}  // namespace pgpu
