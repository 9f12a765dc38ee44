// rt_finalize.cpp -- finalize: an executed plan's group table read back as a result (rt.h).  One function per table
// form (small dense, large dense, hash) over one context, then the result's description; and the lazy decodes of a
// result held compact or as fixed-point digits.
#include "rt_decls.h"

namespace pgpu {

// Group-by dictIds of composite key k: (k / stride[j]) % card[j] (DictionaryBasedGroupKeyGenerator.java:276-323).
static void decode_keys(const pgpu_plan_s* P, pgpu_result_s* R, int64_t row, uint64_t key) {
  for (int j = 0; j < R->num_keys; ++j)
    R->gid(j)[row] = (int32_t)((key / (uint64_t)P->key_stride[j]) % (uint64_t)P->key_card[j] + P->key_off[j]);
}

namespace {

// The large dense and hash paths' pinned readback: the group / record count, the statistics words up to
// STAT_TIMED_OUT, then each slot's (lo, hi) range for the compact form's widths.
constexpr int kRbCount = 0, kRbStats = 1, kRbRanges = 8;
constexpr size_t kRbHeadBytes = kRbRanges * 8;
static_assert(kRbStats + kStatsReadWords <= kRbRanges, "the statistics words end before the slot ranges");

struct FinCtx {
  pgpu_plan_s* P;
  Scratch* sc;
  hipStream_t stream;
  const uint64_t* table;
  int64_t key_begin, G;  // the table holds keys [key_begin, key_begin + G)
  int nslots, nk;
  pgpu_result_s* R;
  ExecStats st;
  int64_t n = 0;  // groups
  // PGPU_TRACE: the table form and the result form that ran, and the host times of the two waits
  const char* form = "";
  const char* emit = "";
  double t_start = 0, t_sync1 = 0;

  int64_t words() const { return (int64_t)nslots * G; }
  // this execution's whole table, unchanged since (no combine, the whole key range)
  bool whole_own_table() const { return table == P->d_table_used && key_begin == 0 && G == P->num_keys; }
};

// Records the compaction of a global hash table can produce (its buffer's capacity).
int64_t hash_record_cap(const pgpu_plan_s* P, int64_t G) {
  return std::max<int64_t>(1, std::min<int64_t>(G, P->merged_records >= 0 ? P->merged_records
                                                                         : std::max<int64_t>(P->total_docs, 1)));
}

// The buffers filled before the wait: growing one frees the old one, and hipFree waits for the whole device -- it
// would hold the wait (and a pgpu_plan_cancel or the query's deadline) until the scan is done.  When one must grow,
// the plan's work is waited for first (cancel- and deadline-aware), then the buffers grow.
int grow_before_wait(FinCtx& F) {
  const pgpu_plan_s* P = F.P;
  Scratch* sc = F.sc;
  bool grow = sc->counter.cap < 64 + (size_t)kMaxSlots * 16 || sc->readback.cap < kRbHeadBytes + (size_t)F.nslots * 16;
  if (!P->hash && F.words() * 8 <= kHostCompactBytes) grow |= sc->readback.cap < (size_t)F.words() * 8 + kStatsBytes;
  else if (!P->hash) grow |= sc->cslots.cap < compact_scratch_bytes(F.G, F.nslots);
  else if (!P->part_hash_live) grow |= sc->ckeys.cap < (size_t)hash_record_cap(P, F.G) * 8 * (1 + F.nslots);
  if (grow) {
    TRY(wait_plan(F.P, F.stream));
    TRY(sc->counter.ensure(64 + (size_t)kMaxSlots * 16));
  }
  return 0;
}

// Waits for the plan's work and decodes the statistics words copied to `w` (`nwords` of them).
int wait_and_read_stats(FinCtx& F, const uint64_t* w, int nwords) {
  TRY(wait_plan(F.P, F.stream));
  F.t_sync1 = trace_on() ? now_us() : 0;
  F.st = decode_stats(w, nwords);
  return F.st.timed_out ? timeout_fail(F.P) : 0;
}

void publish_star_stats(FinCtx& F) {
  F.P->star_docs_read = F.st.star_docs_read;
  F.P->star_metric_bytes = F.st.star_metric_bytes;  // -1 where STAT_STAR_SECTORS was not read back
}

// Small dense table: one or two copies (table + stats) and one sync; compacted on the host in key order.
int finalize_small_dense(FinCtx& F) {
  pgpu_plan_s* P = F.P;
  pgpu_result_s* R = F.R;
  const int64_t words = F.words(), G = F.G;
  TRY(F.sc->readback.ensure((size_t)words * 8 + kStatsBytes));
  uint64_t* st = reinterpret_cast<uint64_t*>(F.sc->readback.p);
  F.form = "small-dense";
  if (reinterpret_cast<const uint8_t*>(P->d_stats) == reinterpret_cast<const uint8_t*>(F.table) + words * 8) {
    F.emit = "one-copy";  // table + stats
    HIP_TRY(hipMemcpyAsync(st, F.table, (size_t)words * 8 + kStatsBytes, hipMemcpyDeviceToHost, F.stream));
  } else {
    F.emit = "two-copies";
    HIP_TRY(hipMemcpyAsync(st, F.table, (size_t)words * 8, hipMemcpyDeviceToHost, F.stream));
    HIP_TRY(hipMemcpyAsync(st + words, P->d_stats, kStatsBytes, hipMemcpyDeviceToHost, F.stream));
  }
  TRY(wait_and_read_stats(F, st + words, kStatsWords));
  publish_star_stats(F);
  for (int64_t k = 0; k < G; ++k) F.n += st[k] != 0;
  TRY(R->alloc(F.nk, F.nslots, F.n));
  int64_t j = 0;
  for (int64_t k = 0; k < G; ++k) {
    if (!st[k]) continue;
    decode_keys(P, R, j, (uint64_t)(F.key_begin + k));
    for (int s = 0; s < F.nslots; ++s) R->slot(s)[j] = st[(int64_t)s * G + k];
    ++j;
  }
  return 0;
}

// Each slot's narrowest width for the compact forms, from the (lo, hi) ranges read back at rb + kRbRanges.  flip:
// the hash path's ranges are order-preserving unsigned keys (sign bit flipped).
std::vector<int32_t> slot_widths(const FinCtx& F, const uint64_t* rb, uint64_t flip) {
  std::vector<int32_t> width(F.nslots, 8);
  for (int s = 0; s < F.nslots; ++s) {
    const long long lo = (long long)(rb[kRbRanges + s] ^ flip), hi = (long long)(rb[kRbRanges + F.nslots + s] ^ flip);
    width[s] = F.n > 0 ? compact_slot_width(lo, hi, F.P->slot_kind[s]) : 8;
  }
  return width;
}

// The slots' areas of a compact result after `first` bytes of keys (bitmap or key column), each 8-aligned; returns
// the whole size.
template <class T>
size_t compact_slot_offsets(int64_t n, const std::vector<int32_t>& width, size_t first, T* off) {
  for (size_t s = 0; s < width.size(); ++s) {
    off[s] = (T)first;
    first += ((size_t)n * width[s] + 7) & ~size_t(7);
  }
  return first;
}

// The compact result's description and its pinned buffer of `bytes` (R->cslot_off is the caller's).
int compact_header(FinCtx& F, const std::vector<int32_t>& width, size_t bytes) {
  pgpu_result_s* R = F.R;
  R->num_keys = F.nk;
  R->num_slots = F.nslots;
  R->n = F.n;
  R->cstride = F.P->key_stride;
  R->ccard = F.P->key_card;
  R->coff = F.P->key_off;
  R->cwidth = width;
  if (R->pool) R->cbuf = R->pool->take();
  return R->cbuf.ensure(bytes);
}

int compact_publish(FinCtx& F) {
  HIP_TRY(hipStreamSynchronize(F.stream));
  F.R->compact.store(true, std::memory_order_release);
  F.emit = "compact";
  return 0;
}

// Large dense, compact form: a presence bitmap over the keys plus each slot's words at its narrowest width.
int dense_emit_compact(FinCtx& F, const std::vector<int32_t>& width, const long long* d_minmax) {
  const pgpu_plan_s* P = F.P;
  Scratch* sc = F.sc;
  pgpu_result_s* R = F.R;
  const int nslots = F.nslots;
  const int64_t n = F.n, cap = n, bitmap_words = (F.G + 63) / 64;
  TRY(sc->ckeys.ensure((size_t)bitmap_words * 8 + (size_t)nslots * cap * 8));
  uint8_t* dev = sc->ckeys.as<uint8_t>();
  if (launch_compact_dense_scatter(F.table, nslots, F.G, P->slot_kind.data(), sc->cslots.as<uint32_t>(), d_minmax,
                                   reinterpret_cast<uint64_t*>(dev), dev + bitmap_words * 8, cap, F.stream))
    return fail(PGPU_ERR_DEVICE, "compact scatter launch failed: %s", hipGetErrorString(hipGetLastError()));
  R->ckey_base = F.key_begin;
  R->cbits = F.G;
  R->cslot_off.assign(nslots, 0);
  const size_t bytes = compact_slot_offsets(n, width, (size_t)bitmap_words * 8, R->cslot_off.data());
  TRY(compact_header(F, width, bytes));
  uint8_t* h = reinterpret_cast<uint8_t*>(R->cbuf.p);
  HIP_TRY(hipMemcpyAsync(h, dev, (size_t)bitmap_words * 8, hipMemcpyDeviceToHost, F.stream));
  for (int s = 0; s < nslots; ++s)
    HIP_TRY(hipMemcpyAsync(h + R->cslot_off[s], dev + bitmap_words * 8 + (size_t)s * cap * 8, (size_t)n * width[s],
                           hipMemcpyDeviceToHost, F.stream));
  return compact_publish(F);
}

// Large dense, columnar form: dictIds + 8-byte words scattered in key order on the device.
int dense_emit_columnar(FinCtx& F) {
  const pgpu_plan_s* P = F.P;
  Scratch* sc = F.sc;
  pgpu_result_s* R = F.R;
  const int nslots = F.nslots, nk = F.nk;
  const int64_t n = F.n, cap = std::max<int64_t>(2, (n + 1) & ~int64_t(1));
  TRY(sc->ckeys.ensure((size_t)cap * (4 * nk + 8 * nslots) + 8));
  if (launch_compact_ordered_scatter(F.table, nslots, F.G, F.key_begin, P->key_stride.data(), P->key_card.data(),
                                     P->key_off.data(), nk, sc->cslots.as<uint32_t>(), sc->ckeys.p, cap, F.stream))
    return fail(PGPU_ERR_DEVICE, "compact launch failed: %s", hipGetErrorString(hipGetLastError()));
  TRY(R->alloc(nk, nslots, n));
  if (n > 0) {
    const uint8_t* dev = sc->ckeys.as<uint8_t>();
    for (int j = 0; j < nk; ++j)
      HIP_TRY(hipMemcpyAsync(R->gid_raw(j), dev + (size_t)j * cap * 4, (size_t)n * 4, hipMemcpyDeviceToHost, F.stream));
    for (int s = 0; s < nslots; ++s)
      HIP_TRY(hipMemcpyAsync(R->slot_raw(s), dev + (size_t)nk * cap * 4 + (size_t)s * cap * 8, (size_t)n * 8,
                             hipMemcpyDeviceToHost, F.stream));
  }
  HIP_TRY(hipStreamSynchronize(F.stream));
  F.emit = "columnar";
  return 0;
}

// Large dense table: ordered compaction on the device (count / scan, then a scatter in key order), copied back into
// the pinned result buffer.  Two forms: the columnar dictIds + 8-byte words, or -- when it moves fewer bytes, as for
// C5's 10M groups of 10M keys -- a presence bitmap over the keys plus each slot's words at the narrowest width their
// range allows (decoded on the host on first access).
int finalize_large_dense(FinCtx& F) {
  const pgpu_plan_s* P = F.P;
  Scratch* sc = F.sc;
  const int nslots = F.nslots;
  TRY(sc->counter.ensure(64 + (size_t)nslots * 16));
  TRY(sc->cslots.ensure(compact_scratch_bytes(F.G, nslots)));
  long long* d_minmax = reinterpret_cast<long long*>(sc->counter.as<uint8_t>() + 64);
  const bool counted = P->k8d_counts && F.whole_own_table();  // K8d already counted this table by chunk
  F.form = counted ? "large-dense-k8d-counts" : "large-dense";
  if (launch_compact_dense_count(F.table, nslots, F.G, sc->cslots.as<uint32_t>(), sc->counter.as<unsigned long long>(),
                                 d_minmax, F.stream, counted))
    return fail(PGPU_ERR_DEVICE, "compact count launch failed: %s", hipGetErrorString(hipGetLastError()));
  TRY(sc->readback.ensure(kRbHeadBytes + (size_t)nslots * 16));
  uint64_t* rb = reinterpret_cast<uint64_t*>(sc->readback.p);
  HIP_TRY(hipMemcpyAsync(rb + kRbCount, sc->counter.p, 8, hipMemcpyDeviceToHost, F.stream));
  HIP_TRY(hipMemcpyAsync(rb + kRbStats, P->d_stats, kStatsReadBytes, hipMemcpyDeviceToHost, F.stream));
  HIP_TRY(hipMemcpyAsync(rb + kRbRanges, d_minmax, (size_t)nslots * 16, hipMemcpyDeviceToHost, F.stream));
  TRY(wait_and_read_stats(F, rb + kRbStats, kStatsReadWords));
  const int64_t n = F.n = (int64_t)std::min<uint64_t>(rb[kRbCount], (uint64_t)F.G);
  publish_star_stats(F);
  const std::vector<int32_t> width = slot_widths(F, rb, 0);
  int64_t narrow_bytes = 0;
  for (int s = 0; s < nslots; ++s) narrow_bytes += n * width[s];
  const int64_t bitmap_words = (F.G + 63) / 64;
  const bool compact =
      P->cfg.compact_results && n > 0 && bitmap_words * 8 + narrow_bytes < n * (4 * F.nk + 8 * nslots);
  return compact ? dense_emit_compact(F, width, d_minmax) : dense_emit_columnar(F);
}

// The hash table's groups as entry-major records (key, then the slot words) in sc->ckeys, their count in sc->counter:
// K8h wrote both at execute; a global table is compacted here.  *cap: the records the buffer holds.
int hash_records(FinCtx& F, int64_t* cap) {
  const pgpu_plan_s* P = F.P;
  Scratch* sc = F.sc;
  if (P->part_hash_live) {
    F.form = "hash-k8h";
    *cap = part_hash_out_cap(P);
    return 0;
  }
  F.form = P->merged_records >= 0 ? "hash-merged" : "hash-global";
  *cap = hash_record_cap(P, F.G);
  TRY(sc->counter.ensure(64));
  TRY(sc->ckeys.ensure((size_t)*cap * 8 * (1 + F.nslots)));
  HIP_TRY(hipMemsetAsync(sc->counter.p, 0, 8, F.stream));
  if (launch_compact(F.table, sc->hash_keys.as<unsigned long long>(), F.nslots, F.G,
                     sc->counter.as<unsigned long long>(), sc->ckeys.as<uint64_t>(), *cap, F.stream))
    return fail(PGPU_ERR_DEVICE, "compact launch failed");
  return 0;
}

// Each slot's range over the records (the compact form's widths), read back with their count and the statistics;
// the wait; the table's error flags.  Sets F.n.
int hash_count_and_ranges(FinCtx& F, int64_t cap, bool want_compact, uint64_t** rb_out) {
  pgpu_plan_s* P = F.P;
  Scratch* sc = F.sc;
  const int nslots = F.nslots;
  const bool k8h = P->part_hash_live;
  TRY(sc->counter.ensure(64 + (size_t)kMaxSlots * 16));  // (no regrowth: the first allocation is 4 KB)
  unsigned long long* d_mm = reinterpret_cast<unsigned long long*>(sc->counter.as<uint8_t>() + 64);
  if (want_compact &&
      (k8h ? launch_hash_minmax_parts(sc->part_mm.as<unsigned long long>(), P->num_parts, nslots, d_mm, F.stream)
           : launch_hash_minmax(sc->ckeys.as<uint64_t>(), sc->counter.as<unsigned long long>(), cap, nslots, d_mm,
                                F.stream)))
    return fail(PGPU_ERR_DEVICE, "slot range launch failed: %s", hipGetErrorString(hipGetLastError()));
  TRY(sc->readback.ensure(kRbHeadBytes + (size_t)nslots * 16));
  uint64_t* rb = *rb_out = reinterpret_cast<uint64_t*>(sc->readback.p);
  HIP_TRY(hipMemcpyAsync(rb + kRbCount, sc->counter.p, 8, hipMemcpyDeviceToHost, F.stream));
  HIP_TRY(hipMemcpyAsync(rb + kRbStats, P->d_stats, kStatsReadBytes, hipMemcpyDeviceToHost, F.stream));
  if (want_compact)
    HIP_TRY(hipMemcpyAsync(rb + kRbRanges, d_mm, (size_t)nslots * 16, hipMemcpyDeviceToHost, F.stream));
  TRY(wait_and_read_stats(F, rb + kRbStats, kStatsReadWords));
  if (F.st.hash_full)  // the table was sized below the plan's groups
    return fail(PGPU_ERR_DEVICE, "group hash table of %lld slots overflowed (plan bound %lld groups)",
                (long long)F.G, (long long)P->group_bound);
  if (k8h && rb[kRbCount] > (uint64_t)cap) return part_hash_overflow(P, rb[kRbCount]);
  F.n = (int64_t)std::min<uint64_t>(rb[kRbCount], (uint64_t)cap);
  publish_star_stats(F);
  if (P->groups_seen && P->merged_records < 0) P->groups_seen->store(F.n, std::memory_order_relaxed);
  return 0;
}

// Hash records held in compact form: composite keys at 4 or 8 bytes instead of the decoded dictIds, and each slot at
// the narrowest width of its range (as the dense compact form); the host decodes it on first access (result_expand).
int hash_emit_compact(FinCtx& F, int32_t key_width, const std::vector<int32_t>& width,
                      const std::vector<int64_t>& woff, size_t cbytes) {
  Scratch* sc = F.sc;
  pgpu_result_s* R = F.R;
  TRY(sc->hsort.ensure(cbytes + 256));
  uint8_t* out = sc->hsort.as<uint8_t>();
  if (launch_hash_compact(sc->ckeys.as<uint64_t>(), F.n, F.nslots, key_width, width.data(), woff.data(), out,
                          F.stream))
    return fail(PGPU_ERR_DEVICE, "hash compact launch failed: %s", hipGetErrorString(hipGetLastError()));
  R->ckey_width = key_width;
  R->cslot_off.assign(woff.begin(), woff.end());
  TRY(compact_header(F, width, cbytes));
  HIP_TRY(hipMemcpyAsync(R->cbuf.p, out, cbytes, hipMemcpyDeviceToHost, F.stream));
  return compact_publish(F);
}

// Hash records decoded into the columnar result on the device: one copy back.
int hash_emit_decoded(FinCtx& F) {
  const pgpu_plan_s* P = F.P;
  Scratch* sc = F.sc;
  pgpu_result_s* R = F.R;
  const int64_t n = F.n;
  const size_t slot_off = pgpu_result_s::slot_offset(F.nk, n);
  const size_t out_bytes = slot_off + (size_t)F.nslots * n * 8;
  TRY(sc->hsort.ensure(out_bytes + 256));
  uint8_t* out = sc->hsort.as<uint8_t>();
  if (launch_hash_decode(sc->ckeys.as<uint64_t>(), n, F.nslots, F.nk, P->key_stride.data(), P->key_card.data(),
                         P->key_off.data(), out, slot_off, F.stream))
    return fail(PGPU_ERR_DEVICE, "hash decode launch failed: %s", hipGetErrorString(hipGetLastError()));
  TRY(R->alloc(F.nk, F.nslots, n));
  HIP_TRY(hipMemcpyAsync(R->buf.p, out, out_bytes, hipMemcpyDeviceToHost, F.stream));
  HIP_TRY(hipStreamSynchronize(F.stream));
  F.emit = "decoded";
  return 0;
}

// ARRAY_MAP: row r's dictIds from its record key, walking the stage tables back -- last group first: its key's slot
// part names the previous group's key.
int decode_staged_key(const FinCtx& F, int64_t r, uint64_t cur, const std::vector<uint64_t>& stages,
                      const std::vector<int64_t>& stage_off) {
  const pgpu_plan_s* P = F.P;
  for (int g = (int)P->stage_space.size() - 1; g >= 0; --g) {
    const uint64_t local = cur % (uint64_t)P->stage_space[g], slot = cur / (uint64_t)P->stage_space[g];
    const int j0 = g == 0 ? 0 : P->stage_end[g - 1], j1 = g < (int)P->stage_end.size() ? P->stage_end[g] : F.nk;
    for (int j = j0; j < j1; ++j)
      F.R->gid(j)[r] = (int32_t)((local / (uint64_t)P->key_stride[j]) % (uint64_t)P->key_card[j]);
    if (g > 0) {
      if (slot >= (uint64_t)P->stage_cap[g - 1]) return fail(PGPU_ERR_DEVICE, "ARRAY_MAP stage slot out of range");
      cur = stages[(size_t)(stage_off[g - 1] + (int64_t)slot)];
    }
  }
  return 0;
}

// Hash records copied back and put in key order on the host (fewer than 4096 groups, or ARRAY_MAP stages).
int hash_emit_sorted(FinCtx& F) {
  const pgpu_plan_s* P = F.P;
  Scratch* sc = F.sc;
  pgpu_result_s* R = F.R;
  const int64_t n = F.n, rec = 1 + F.nslots;
  const bool staged = !P->stage_end.empty();
  const uint64_t* st = reinterpret_cast<const uint64_t*>(sc->readback.p);
  if (n > 0) {
    TRY(sc->readback.ensure((size_t)n * rec * 8));
    st = reinterpret_cast<const uint64_t*>(sc->readback.p);
    HIP_TRY(hipMemcpyAsync(sc->readback.p, sc->ckeys.p, (size_t)n * rec * 8, hipMemcpyDeviceToHost, F.stream));
    HIP_TRY(hipStreamSynchronize(F.stream));
  }
  std::vector<uint64_t> stages;  // ARRAY_MAP: the stage tables (slot -> that group's key), back to back
  std::vector<int64_t> stage_off;
  if (staged && n > 0) {
    int64_t total = 0;
    for (int64_t c : P->stage_cap) { stage_off.push_back(total); total += c; }
    stages.resize((size_t)total);
    HIP_TRY(hipMemcpyAsync(stages.data(), sc->stage_keys.p, (size_t)total * 8, hipMemcpyDeviceToHost, F.stream));
    HIP_TRY(hipStreamSynchronize(F.stream));
  }
  std::vector<int64_t> order(n);
  for (int64_t i = 0; i < n; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return st[a * rec] < st[b * rec]; });
  TRY(R->alloc(F.nk, F.nslots, n));
  for (int64_t r = 0; r < n; ++r) {
    const uint64_t* e = st + order[r] * rec;
    if (staged) TRY(decode_staged_key(F, r, e[0], stages, stage_off));
    else decode_keys(P, R, r, e[0]);
    for (int s = 0; s < F.nslots; ++s) R->slot(s)[r] = e[1 + s];
  }
  F.emit = staged ? "sorted-stages" : "sorted";
  return 0;
}

// Hash table: unordered compaction, then one of three result forms.  From 4096 groups on (and no ARRAY_MAP stages)
// the records are decoded on the device in one streaming pass, in their (hash / partition) order -- the LONG_MAP
// holder's iteration order is fastutil's hash order (DictionaryBasedGroupKeyGenerator.java:693, :719) and no consumer
// depends on group order -- held in compact form when that moves fewer bytes (C5-sized results: 10M groups).  Below
// that, key order on the host.
int finalize_hash(FinCtx& F) {
  const pgpu_plan_s* P = F.P;
  const int nslots = F.nslots, nk = F.nk;
  int64_t cap = 0;
  TRY(hash_records(F, &cap));
  const bool want_compact = P->stage_end.empty() && P->cfg.compact_results;
  uint64_t* rb = nullptr;
  TRY(hash_count_and_ranges(F, cap, want_compact, &rb));
  const int64_t n = F.n;
  if (n < 4096 || !P->stage_end.empty()) return hash_emit_sorted(F);
  if (!want_compact) return hash_emit_decoded(F);  // (the ranges were not read back)
  int key_bits = 1;
  {
    const long double space = (long double)P->key_stride[nk - 1] * (long double)P->key_card[nk - 1];
    while (key_bits < 64 && (long double)(INT64_C(1) << key_bits) < space) ++key_bits;
  }
  const int32_t key_width = key_bits <= 32 ? 4 : 8;
  const std::vector<int32_t> width = slot_widths(F, rb, 1ull << 63);
  std::vector<int64_t> woff(nslots, 0);
  const size_t cbytes = compact_slot_offsets(n, width, ((size_t)n * key_width + 7) & ~size_t(7), woff.data());
  if (cbytes < (size_t)n * (4 * nk + 8 * nslots)) return hash_emit_compact(F, key_width, width, woff, cbytes);
  return hash_emit_decoded(F);
}

// What the result's rows are: keys, aggregations and how each aggregation's slot word reads (agg_conv).
void describe_result(const pgpu_plan_s* P, pgpu_result_s* R) {
  const int na = (int)P->agg_fn.size();
  R->num_aggs = na;
  R->agg_slot = P->agg_slot;
  R->slot_kind = P->slot_kind;
  R->key_cols = P->key_cols;
  R->key_dicts.assign(P->key_dicts.begin(), P->key_dicts.end());
  R->key_types.clear();
  for (int c : P->key_cols) R->key_types.push_back(P->table->col_type(c));
  R->agg_fn = P->agg_fn;
  R->agg_col = P->agg_col;
  R->agg_conv.assign(na, RCONV_I64);
  for (int a = 0; a < na; ++a) {
    const int fn = P->agg_fn[a];
    if (fn == PGPU_AGG_COUNT) continue;  // CountAggregationFunction: exact count (held as double by Pinot)
    if (fn == PGPU_AGG_DISTINCTCOUNT) continue;  // the set's size (DistinctCountAggregationFunction.extractFinalResult)
    if (fn == PGPU_AGG_PERCENTILE) {  // the selected value's double (percentile_select_kernel)
      R->agg_conv[a] = RCONV_F64;
      continue;
    }
    if (fn == PGPU_AGG_SUM || fn == PGPU_AGG_AVG)
      R->agg_conv[a] = P->slot_kind[P->agg_slot[a]] == SLOT_SUM_I64 ? RCONV_I64 : RCONV_F64;
    else
      // (MIN / MAX of an expression, a virtual column past the table's real ones: the key of its double)
      R->agg_conv[a] = P->agg_col[a] < (int)P->table->names.size() && is_int_type(P->table->types[P->agg_col[a]])
                           ? RCONV_I64 : RCONV_KEY_F64;
  }
  // fixed-point FLOAT / DOUBLE sums (PGPU_OPT_EXACT_FP_SUM): W digit sums from the aggregation's slot on, converted to
  // the one double on the result's first read -- after the merge for the parts of a composite plan
  R->agg_fx.clear();
  if (P->fx) {
    R->agg_fx.assign(na, FxFormat{});
    bool any = false;
    for (int a = 0; a < na; ++a) {
      const int sl = P->agg_slot[a];
      if (P->agg_fn[a] == PGPU_AGG_COUNT || sl < 0 || P->slot_fx[sl] < 0) continue;
      R->agg_fx[a] = P->slot_fmt[sl];
      R->agg_conv[a] = RCONV_FX;
      any = true;
    }
    R->fx_pending.store(any && !P->fx_part, std::memory_order_release);
    R->fx_agreed = P->fx_agreed;
  }
}

// numEntriesScannedInFilter of the plan's STATS_GENERIC segments: their leaves' bitmaps (copied into maskstage by the
// stream, synchronised since) replayed on the host.
int64_t generic_entries_scanned(const pgpu_plan_s* P) {
  if (P->generic.empty()) return 0;
  const uint32_t* words = reinterpret_cast<const uint32_t*>(P->scratch->maskstage.p);
  std::vector<int64_t> part(P->generic.size(), 0);
  auto replay = [&](int i) {
    const auto& g = P->generic[i];
    const int64_t ngroups = ((int64_t)g.num_docs + 31) / 32;
    std::vector<const uint32_t*> masks(P->num_leaves);
    for (int k = 0; k < P->num_leaves; ++k) masks[P->leaf_perm[k]] = words + g.out_word + (int64_t)k * ngroups;
    part[i] = simulate_entries_scanned(g.tree, masks, g.num_docs);
  };
  if (P->generic.size() > 4) host_pool().run((int)P->generic.size(), replay);
  else for (size_t i = 0; i < P->generic.size(); ++i) replay((int)i);
  int64_t total = 0;
  for (int64_t v : part) total += v;
  return total;
}

void fill_stats_row(const FinCtx& F, int64_t generic_entries) {
  const pgpu_plan_s* P = F.P;
  pgpu_result_s* R = F.R;
  // GroupByCombineOperator.mergeResults (:215-219): the merged map holds >= numGroupsLimit groups (PQL mode only)
  R->groups_limit_reached = P->pql_cap && F.nk > 0 && P->num_groups_limit > 0 && F.n >= P->num_groups_limit;
  R->stats[0] = (int64_t)F.st.matched;
  R->stats[1] = P->scanned_entries_model + (int64_t)F.st.entries + generic_entries;
  R->stats[2] = ((int64_t)F.st.matched - P->post_exempt_docs) * P->num_projected;
  R->stats[3] = P->total_docs;
  R->stats[4] = (int64_t)P->segs.size();
  R->stats[5] = P->segments_matched_filter;
}

}  // namespace

// key_begin / key_count: a shard [slots][key_count] of the dense table holding keys [key_begin, key_begin +
// key_count) (after a reduce-scatter across GPUs); the whole table is (0, num_keys).
int plan_finalize_impl(pgpu_plan_s* P, hipStream_t stream, const void* d_table, int64_t key_begin, int64_t key_count,
                       pgpu_result_s* R) {
  FinCtx F{P, P->scratch, stream, nullptr, key_begin, key_count, (int)P->slot_kind.size(), (int)P->key_cols.size(), R};
  F.t_start = trace_on() ? now_us() : 0;
  if (!P->executed) return fail(PGPU_ERR_INVALID_ARGUMENT, "plan not executed");
  F.table = reinterpret_cast<const uint64_t*>(d_table ? d_table : P->d_table_used);
  P->star_metric_bytes = -1;  // read back by the small-table path only
  R->pool = P->table->result_pool;
  TRY(grow_before_wait(F));
  if (!P->hash && F.words() * 8 <= kHostCompactBytes) TRY(finalize_small_dense(F));
  else if (!P->hash) TRY(finalize_large_dense(F));
  else TRY(finalize_hash(F));
  const double t_sync2 = trace_on() ? now_us() : 0;
  describe_result(P, R);
  fill_stats_row(F, generic_entries_scanned(P));
  if (trace_on())
    fprintf(stderr, "[pgpu] finalize: launch+sync1 %.1f us, copy+sync2 %.1f us, decode %.1f us (n=%lld) branch %s/%s\n",
            F.t_sync1 - F.t_start, t_sync2 - F.t_sync1, now_us() - t_sync2, (long long)F.n, F.form, F.emit);
  return 0;
}

}  // namespace pgpu

void pgpu::result_resolve_fx(pgpu_result_s* R) {
  if (R->compact.load(std::memory_order_acquire) && result_expand(R)) return;
  std::lock_guard<std::mutex> g(R->expand_mu);
  if (!R->fx_pending.load(std::memory_order_acquire)) return;
  for (int a = 0; a < R->num_aggs && a < (int)R->agg_fx.size(); ++a) {
    if (R->agg_conv[a] != RCONV_FX) continue;
    const FxFormat f = R->agg_fx[a];
    const int s0 = R->agg_slot[a];
    bool done = false;  // SUM and AVG of a column share their digit slots: converted once
    for (int b = 0; b < a; ++b) done |= R->agg_slot[b] == s0 && b < (int)R->agg_fx.size() && R->agg_fx[b].mode != FX_NONE;
    if (done) {
      R->agg_conv[a] = RCONV_F64;
      continue;
    }
    uint64_t* out = R->slot_raw(s0);
    const uint64_t* d1 = R->slot_raw(s0 + 1);
    const uint64_t* d2 = f.W > 2 ? R->slot_raw(s0 + 2) : nullptr;
    for (int64_t i = 0; i < R->n; ++i) {
      const int64_t digits[kFxMaxDigits] = {(int64_t)out[i], (int64_t)d1[i], d2 ? (int64_t)d2[i] : 0};
      const double v = fx_result(digits, f);
      memcpy(&out[i], &v, 8);
    }
    R->agg_conv[a] = RCONV_F64;
    if (s0 < (int)R->slot_kind.size()) R->slot_kind[s0] = SLOT_SUM_F64;
  }
  R->fx_pending.store(false, std::memory_order_release);
}

// Columnar form of a compact result: rows are the bitmap's set bits in key order; each block of 4096 bitmap words is
// decoded by one task of the host pool (a prefix of its popcounts gives its first row).
int pgpu::result_expand(pgpu_result_s* R) {
  std::lock_guard<std::mutex> g(R->expand_mu);
  if (!R->compact.load(std::memory_order_acquire)) return 0;
  const int nk = R->num_keys, ns = R->num_slots;
  const int64_t n = R->n;
  TRY(R->alloc(nk, ns, n));
  if (R->ckey_width) {  // composite keys (hash-mode results): decode each row's key
    const uint8_t* kb = reinterpret_cast<const uint8_t*>(R->cbuf.p);
    constexpr int64_t kRowsPerTask = 1 << 20;
    const int64_t ktasks = (n + kRowsPerTask - 1) / kRowsPerTask;
    auto keys = [&](int t) {
      const int64_t r0 = t * kRowsPerTask, r1 = std::min(n, r0 + kRowsPerTask);
      for (int64_t r = r0; r < r1; ++r) {
        const uint64_t key = R->ckey_width == 4 ? (uint64_t)reinterpret_cast<const uint32_t*>(kb)[r]
                                                : reinterpret_cast<const uint64_t*>(kb)[r];
        for (int j = 0; j < nk; ++j)
          R->gid_raw(j)[r] = (int32_t)((key / (uint64_t)R->cstride[j]) % (uint64_t)R->ccard[j] + R->coff[j]);
      }
    };
    if (ktasks > 1) host_pool().run((int)ktasks, keys);
    else if (ktasks == 1) keys(0);
  }
  const uint64_t* bm = reinterpret_cast<const uint64_t*>(R->cbuf.p);
  const int64_t words = R->ckey_width ? 0 : (R->cbits + 63) / 64;
  constexpr int64_t kBlockWords = 4096;
  const int64_t nb = (words + kBlockWords - 1) / kBlockWords;
  std::vector<int64_t> first(nb + 1, 0);
  auto count = [&](int b) {
    int64_t c = 0;
    for (int64_t w = b * kBlockWords; w < std::min(words, (b + 1) * kBlockWords); ++w) c += __builtin_popcountll(bm[w]);
    first[b + 1] = c;
  };
  auto decode = [&](int b) {
    int64_t row = first[b];
    std::vector<int32_t*> gid(nk);
    for (int j = 0; j < nk; ++j) gid[j] = R->gid_raw(j);
    for (int64_t w = b * kBlockWords; w < std::min(words, (b + 1) * kBlockWords); ++w) {
      for (uint64_t bits = bm[w]; bits; bits &= bits - 1, ++row) {
        if (row >= n) return;
        const uint64_t key = (uint64_t)(R->ckey_base + w * 64 + __builtin_ctzll(bits));
        for (int j = 0; j < nk; ++j)
          gid[j][row] = (int32_t)((key / (uint64_t)R->cstride[j]) % (uint64_t)R->ccard[j] + R->coff[j]);
      }
    }
  };
  if (nb > 1) host_pool().run((int)nb, count);
  else if (nb == 1) count(0);
  for (int64_t b = 0; b < nb; ++b) first[b + 1] += first[b];
  if (nb > 1) host_pool().run((int)nb, decode);
  else if (nb == 1) decode(0);
  // the words, sign-extended from their compact widths
  const uint8_t* base = reinterpret_cast<const uint8_t*>(R->cbuf.p);
  constexpr int64_t kRows = 1 << 20;
  const int64_t tasks = (n + kRows - 1) / kRows;
  auto widen = [&](int t) {
    const int64_t r0 = t * kRows, r1 = std::min(n, r0 + kRows);
    for (int s = 0; s < ns; ++s) {
      const uint8_t* src = base + R->cslot_off[s];
      uint64_t* dst = R->slot_raw(s);
      switch (R->cwidth[s]) {
        case 1: for (int64_t r = r0; r < r1; ++r) dst[r] = (uint64_t)(int64_t)reinterpret_cast<const int8_t*>(src)[r]; break;
        case 2: for (int64_t r = r0; r < r1; ++r) dst[r] = (uint64_t)(int64_t)reinterpret_cast<const int16_t*>(src)[r]; break;
        case 3:  // 24-bit little-endian, sign-extended
          for (int64_t r = r0; r < r1; ++r) {
            const uint32_t u = (uint32_t)src[3 * r] | (uint32_t)src[3 * r + 1] << 8 | (uint32_t)src[3 * r + 2] << 16;
            dst[r] = (uint64_t)(int64_t)((int32_t)(u << 8) >> 8);
          }
          break;
        case 4: for (int64_t r = r0; r < r1; ++r) dst[r] = (uint64_t)(int64_t)reinterpret_cast<const int32_t*>(src)[r]; break;
        default: memcpy(dst + r0, reinterpret_cast<const uint64_t*>(src) + r0, (size_t)(r1 - r0) * 8); break;
      }
    }
  };
  if (tasks > 1) host_pool().run((int)tasks, widen);
  else if (tasks == 1) widen(0);
  R->compact.store(false, std::memory_order_release);
  return 0;
}
