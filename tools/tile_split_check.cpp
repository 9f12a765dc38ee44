// tile_split_check.cpp -- exhaustive host check of the scan's tile split (pinot_amd/csrc/tile_split.h, the header the
// kernel and the plan share; nothing else of the library is included or linked).  Built under AddressSanitizer +
// UndefinedBehaviorSanitizer by pinot_amd.build.build_tile_split_check, run by tests/test_tile_split_cpu.py.
//
// For plans of B tiles on G workgroups (S workgroups per CU, slot weights of step s) and their launches of T <= B tiles
// on min(G, T) workgroups, in every branch of tile_split (chunked, XCD-interleaved, plain):
//   partition  every tile of [0, T) belongs to exactly one workgroup's run;
//   bound      no run is longer than the plan's LEAP2 reservation (scan_leap_tiles), nor than kLeapLdsTiles when weighted;
//   weights    a slot-s run is within one tile of len w_s / sum(w) of its XCD's eighth; without weights the runs are the
//              literal equal split; weights are declined only where the cap forces it;
//   overflow   T up to INT32_MAX and grids up to 65 536 (runs only; UBSan reports any overflow).
// Exit status 0 = all held.  --parent-reservation replays the reservation before this check existed,
// ceil(B / G) + 3 with weights never declined: the check must fail on it (the test asserts that it does).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tile_split.h"

using namespace pgpu;

static bool g_parent = false;
static long long g_launches = 0, g_runs = 0, g_failures = 0;

struct Ctx {
  int64_t B, G, T, g;
  int S;
  double step;
  int tile_chunks;
};

static void failure(const Ctx& c, const char* what, long long a, long long b) {
  if (++g_failures <= 40)
    printf("FAIL %s: %lld vs %lld  (plan B=%lld G=%lld slots=%d step=%.2f; launch T=%lld grid=%lld chunks=%d)\n", what,
           a, b, (long long)c.B, (long long)c.G, c.S, c.step, (long long)c.T, (long long)c.g, c.tile_chunks);
}

static int64_t reserve(int64_t B, int64_t G, int num_cus, double step) {
  if (g_parent) return (B + G - 1) / (G > 1 ? G : 1) + 3;
  return scan_leap_tiles(B, G, num_cus, step);
}

// One launch: partition, bound, weights.  Returns its longest run.
static int64_t check_launch(const Ctx& c, int slot_n, const uint16_t* w, int64_t reserved) {
  const int64_t T = c.T, g = c.g;
  const bool xcd = g >= 64 && (g & 7) == 0;
  int64_t longest = 0;
  ++g_launches;
  if (xcd) {
    const int64_t nx = g >> 3;
    const int64_t tot = slot_n > 1 ? slot_weight_cum(nx, nx, slot_n, w) : 0;
    int64_t at = 0;  // the tiles below are covered exactly once
    for (int64_t x = 0; x < 8; ++x) {
      const int64_t lo = x * T / 8, len = (x + 1) * T / 8 - lo;
      if (lo != at) failure(c, "XCD eighth does not abut", lo, at);
      int64_t counted = 0;
      for (int64_t i = 0; i < nx; ++i) {
        const TileRun r = tile_split(i * 8 + x, g, T, c.tile_chunks, slot_n, w, T);
        const int64_t n = r.count();
        ++g_runs;
        if (n > longest) longest = n;
        if (c.tile_chunks) {
          if (r.step != 1) failure(c, "step of a chunked run", r.step, 1);
          if (r.begin != at) failure(c, "run does not abut", r.begin, at);
          if (r.end < r.begin) failure(c, "run ends before it begins", r.end, r.begin);
          at = r.end;
          if (slot_n > 1) {
            int s = 0;
            while (s + 1 < slot_n && i >= nx * (s + 1) / slot_n) ++s;
            const int64_t d = n * tot - len * (int64_t)w[s];  // (run - len w_s / tot) tot
            if (d >= tot || -d >= tot) failure(c, "weighted run not within one tile of its share (x tot)", n * tot, len * w[s]);
          } else {
            if (r.begin != lo + i * len / nx) failure(c, "equal chunked begin", r.begin, lo + i * len / nx);
            if (r.end != lo + (i + 1) * len / nx) failure(c, "equal chunked end", r.end, lo + (i + 1) * len / nx);
          }
        } else {
          // interleaved: workgroup i takes lo + i, lo + i + nx, ... below lo + len -- the residues mod nx are
          // distinct, so the eighth is covered once if the counts add up to it
          if (r.begin != lo + i) failure(c, "interleaved begin", r.begin, lo + i);
          if (r.end != lo + len) failure(c, "interleaved end", r.end, lo + len);
          if (r.step != nx) failure(c, "interleaved step", r.step, nx);
          counted += n;
        }
      }
      if (!c.tile_chunks) {
        if (counted != len) failure(c, "interleaved tiles counted", counted, len);
        at = lo + len;
      }
    }
    if (at != T) failure(c, "tiles covered", at, T);
  } else {
    int64_t at = 0;
    for (int64_t b = 0; b < g; ++b) {
      const TileRun r = tile_split(b, g, T, c.tile_chunks, slot_n, w, T);
      ++g_runs;
      if (r.step != 1) failure(c, "step of a plain run", r.step, 1);
      if (r.begin != at) failure(c, "run does not abut", r.begin, at);
      if (r.begin != b * T / g || r.end != (b + 1) * T / g) failure(c, "plain run", r.begin, b * T / g);
      at = r.end;
      if (r.count() > longest) longest = r.count();
    }
    if (at != T) failure(c, "tiles covered", at, T);
  }
  if (longest > reserved) failure(c, "longest run exceeds the LEAP2 reservation", longest, reserved);
  if (!g_parent && slot_n > 1 && longest > kLeapLdsTiles) failure(c, "weighted run exceeds kLeapLdsTiles", longest, kLeapLdsTiles);
  if (launch_longest_run(T, g, c.tile_chunks, slot_n, w) != longest)
    failure(c, "launch_longest_run", launch_longest_run(T, g, c.tile_chunks, slot_n, w), longest);
  return longest;
}

static const double kSteps[] = {0.0, 0.11, 1.0, 3.0, 4.0};

// A plan of B tiles on G workgroups and launches of some T <= B: unweighted in both tile orders, then every
// (slots per CU, step) whose weights apply.
static void check_plan(int64_t B, int64_t G, bool sub_launches) {
  std::vector<int64_t> Ts{B};
  if (sub_launches)
    for (int64_t t : {B - 1, B / 2, kSlotWeightMinShare * G, kSlotWeightMinShare * G - 1, G, G - 1, G + 1, (int64_t)1}) {
      bool have = t < 1 || t > B;
      for (int64_t u : Ts) have |= u == t;
      if (!have) Ts.push_back(t);
    }
  const int64_t reserved0 = reserve(B, G, 0, 0.0);
  std::vector<int64_t> longest0(Ts.size(), 0);
  for (size_t k = 0; k < Ts.size(); ++k)
    for (int tc = 0; tc < 2; ++tc) {
      Ctx c{B, G, Ts[k], Ts[k] < G ? Ts[k] : G, 0, 0.0, tc};
      const int64_t l = check_launch(c, 0, nullptr, reserved0);
      if (l > longest0[k]) longest0[k] = l;
    }
  for (int S = 2; S <= 4; ++S) {
    if (G % S) continue;
    const int num_cus = (int)(G / S);
    for (double step : kSteps) {
      const int64_t reserved = reserve(B, G, num_cus, step);
      if (!g_parent && reserved > kLeapLdsTiles && reserved0 <= kLeapLdsTiles) {
        Ctx c{B, G, B, G, S, step, 1};
        failure(c, "reservation past the cap where equal shares fit", reserved, kLeapLdsTiles);
      }
      for (size_t k = 0; k < Ts.size(); ++k) {
        Ctx c{B, G, Ts[k], Ts[k] < G ? Ts[k] : G, S, step, 1};
        uint16_t w[kMaxCuSlots] = {0, 0, 0, 0};
        bool declined = false;
        const int64_t limit = g_parent ? INT64_MAX : (reserved < kLeapLdsTiles ? reserved : kLeapLdsTiles);
        const int n = slot_weights(c.T, c.g, num_cus, step, limit, w, &declined);
        if (n == 0) {
          // equal shares, checked above; the reservation of this plan must cover them too
          if (longest0[k] > reserved) failure(c, "longest equal run exceeds the LEAP2 reservation", longest0[k], reserved);
          // declined only where the cap forces the plan to reserve for equal shares alone
          if (declined) {
            uint16_t w2[kMaxCuSlots];
            const int n2 = slot_weights(B, G, num_cus, step, INT64_MAX, w2);
            if (!n2 || weighted_run_bound(B, G, n2, w2) <= kLeapLdsTiles)
              failure(c, "weights declined though the plan's weighted runs fit the cap", n2, reserved);
          }
          continue;
        }
        if (n != S) failure(c, "slot count", n, S);
        for (int s = 0; s < S; ++s) {  // the quantisation's shape: 256 for the last slot, non-increasing, <= 4096
          if (w[S - 1] != 256) failure(c, "weight of the last slot", w[S - 1], 256);
          if (s && w[s] > w[s - 1]) failure(c, "weights increase", w[s], w[s - 1]);
          if (w[s] > 4096) failure(c, "weight past 16", w[s], 4096);
        }
        check_launch(c, n, w, reserved);
      }
    }
  }
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--parent-reservation")) g_parent = true;
    else { fprintf(stderr, "usage: %s [--parent-reservation]\n", argv[0]); return 2; }
  }
  const auto t0 = std::chrono::steady_clock::now();
  // the two shapes the reservation was first seen to miss (300 and 1000 segments of 123 tiles on 256 CUs x 4)
  for (int64_t G : {(int64_t)1024, (int64_t)768, (int64_t)512})
    for (int64_t B : {(int64_t)36900, (int64_t)123000}) check_plan(B, G, true);
  std::vector<int64_t> grids;
  for (int64_t G = 1; G <= 80; ++G) grids.push_back(G);
  for (int64_t G : {248, 256, 504, 512, 768, 1016, 1024, 1032, 2048}) grids.push_back(G);
  for (int64_t G : grids) {
    // every T up to 2 G (runs of 0, 1 and 2 tiles, T below the grid), then an odd stride up to 40 G
    const int64_t stride = (G <= 80 ? G / 8 : G / 2) | 1;
    int64_t k = 0;
    for (int64_t B = 1; B <= 40 * G; B += (B < 2 * G && G <= 80 ? 1 : stride), ++k) check_plan(B, G, G <= 80 || k % 8 == 0);
    check_plan(40 * G, G, true);
    check_plan(36900, G, G >= 64);
    check_plan(123000, G, G >= 64);
  }
  // no overflow: T up to INT32_MAX, grids up to 65 536
  for (int64_t G : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)1024, (int64_t)4096, (int64_t)65528, (int64_t)65536})
    for (int64_t B : {(int64_t)INT32_MAX, (int64_t)INT32_MAX - 1, (int64_t)INT32_MAX - 7, (int64_t)1 << 30})
      check_plan(B, G, false);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  printf("tile_split_check%s: %lld launches, %lld runs, %lld failures, %.0f ms\n", g_parent ? " (parent reservation)" : "",
         g_launches, g_runs, g_failures, ms);
  return g_failures ? 1 : 0;
}
