// rt_exec.cpp -- query execution: the wait, and the launches in phases (rt.h).  Finalize is rt_finalize.cpp.
#include "expr_leaf.h"
#include "rt_decls.h"

namespace pgpu {
// ---- query deadlines (BaseCombineOperator.java:79-132: the combine waits until QueryContext.getEndTimeMs and then
// returns a timeout block; GroupByCombineOperator.java:193-203 for group-by).  The persistent scans compare the
// device wall clock against the deadline converted to clock ticks and stop taking tiles past it.
static double epoch_us() {
  return (double)std::chrono::duration_cast<std::chrono::microseconds>(
             std::chrono::system_clock::now().time_since_epoch()).count();
}

// Device clock ticks at host epoch time end_ms, never earlier than the true reading (the calibration pairs a clock
// value with a host time taken before the kernel that read it, so queueing delay only makes deadlines later).
static int deadline_ticks(pgpu_table_s* t, int64_t end_ms, uint64_t* out) {
  std::lock_guard<std::mutex> g(t->clock_mu);
  if (!t->clock_stream) {
    int khz = 0;
    HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, t->device));
    if (khz <= 0) return fail(PGPU_ERR_DEVICE, "device wall clock rate unavailable");
    t->clock_rate_khz = khz;
    HIP_TRY(hipStreamCreateWithFlags(&t->clock_stream, hipStreamNonBlocking));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&t->clock_pinned), 64, hipHostMallocDefault));
  }
  const double steady = now_us();
  if (t->clock_steady_us < 0 || steady - t->clock_steady_us > 10e6) {
    double best = 1e300;
    for (int i = 0; i < 3 && best > 200.0; ++i) {  // the tightest of up to 3 readings
      const double h0 = epoch_us();
      if (launch_read_clock(t->clock_pinned, t->clock_stream))
        return fail(PGPU_ERR_DEVICE, "clock read launch failed: %s", hipGetErrorString(hipGetLastError()));
      HIP_TRY(hipStreamSynchronize(t->clock_stream));
      const double h1 = epoch_us();
      if (h1 - h0 < best) {
        best = h1 - h0;
        t->clock_host_us = h0;
        t->clock_ticks = *reinterpret_cast<volatile uint64_t*>(t->clock_pinned);
      }
    }
    t->clock_steady_us = steady;
  }
  const double dt_us = (double)end_ms * 1000.0 - t->clock_host_us;
  *out = t->clock_ticks + (dt_us > 0 ? (uint64_t)(dt_us * t->clock_rate_khz / 1000.0) : 0);
  if (*out == 0) *out = 1;
  return 0;
}

// The combine's timeout: aggregation-only plans report BaseCombineOperator's EXECUTION_TIMEOUT_ERROR (250),
// group-by plans GroupByCombineOperator's QUERY_EXECUTION_ERROR (200) wrapping a TimeoutException.
int timeout_fail(const pgpu_plan_s* P) {
  if (P->key_cols.empty())
    return fail(PGPU_ERR_TIMEOUT, "QueryException 250 (EXECUTION_TIMEOUT_ERROR): Timed out while polling results block");
  return fail(PGPU_ERR_TIMEOUT, "QueryException 200 (QUERY_EXECUTION_ERROR): Timed out while combining group-by results "
              "after %lldms", (long long)(P->end_time_ms - P->exec_start_ms));
}

// Leaves the plan's scratch to the device work still queued on `stream` (see Scratch::busy).
int abandon_scratch(Scratch* sc, hipStream_t stream) {
  if (!sc) return 0;
  if (!sc->busy) HIP_TRY(hipEventCreateWithFlags(&sc->busy, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(sc->busy, stream));
  sc->abandoned = true;
  return 0;
}

// Waits for the plan's work on `stream`.  With an end time the wait gives up at it, as the combine's
// _blockingQueue.poll(endTimeMs - now) / _operatorLatch.await(timeoutMs) do (BaseCombineOperator.java:193-203,
// GroupByCombineOperator.java:193-203): the query returns PGPU_ERR_TIMEOUT at its deadline and the device work
// left running keeps its scratch out of the pool until it completes.
static int cancel_fail() {
  return fail(PGPU_ERR_CANCELLED, "QueryException 503 (QUERY_CANCELLATION_ERROR): Query was cancelled");
}

bool cancelled(const pgpu_plan_s* P) { return __atomic_load_n(&P->cancel, __ATOMIC_ACQUIRE) != 0; }

// table->scans_inflight: counted from the execution's launch until its completion is seen or the plan is destroyed
static void inflight_begin(pgpu_plan_s* P) {
  if (P->inflight_counted) {
    P->alone = P->table->scans_inflight.load(std::memory_order_relaxed) == 1;
    return;
  }
  P->alone = P->table->scans_inflight.fetch_add(1, std::memory_order_relaxed) == 0;
  P->inflight_counted = true;
}
void inflight_end(pgpu_plan_s* P) {
  if (!P || !P->inflight_counted || !P->table) return;
  P->table->scans_inflight.fetch_sub(1, std::memory_order_relaxed);
  P->inflight_counted = false;
}

int wait_plan(pgpu_plan_s* P, hipStream_t stream) {
  if (!P->scratch) {
    HIP_TRY(hipStreamSynchronize(stream));
    inflight_end(P);
    return 0;
  }
  Scratch* sc = P->scratch;
  if (cancelled(P)) return abandon_scratch(sc, stream) ? PGPU_ERR_DEVICE : cancel_fail();
  if (!sc->busy) HIP_TRY(hipEventCreateWithFlags(&sc->busy, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(sc->busy, stream));
  // Polled, not a blocking synchronise: a pgpu_plan_cancel from another thread must end the wait.  Spinning (as the
  // HIP runtime's own synchronise does) for the first ~2 ms keeps the wake-up latency of short queries at the
  // poll interval; longer waits back off to 20 us sleeps.
  const auto t0 = std::chrono::steady_clock::now();
  // a combined plan's stream holds collectives that complete only when every peer joins them: the wait also ends at
  // the communicator's timeout, and an expired wait aborts the communicator (the collectives' kernels exit)
  int64_t comm_lim = P->comm_used ? P->comm_used->timeout_ms.load(std::memory_order_relaxed) : 0;
  if (P->comm_used && P->comm_dense && P->end_time_ms <= 0)
    comm_lim = comm_lim > 0 ? std::min(comm_lim, kDenseCombineWaitMs) : kDenseCombineWaitMs;
  for (int spin = 0;; ++spin) {
    const hipError_t e = hipEventQuery(sc->busy);
    if (e == hipSuccess) {
      inflight_end(P);
      return 0;
    }
    if (e != hipErrorNotReady) return fail(PGPU_ERR_DEVICE, "query wait failed: %s", hipGetErrorString(e));
    if (cancelled(P)) {
      sc->abandoned = true;
      if (P->comm_used) P->comm_used->abort();
      return cancel_fail();
    }
    if (P->end_time_ms > 0 && epoch_us() >= (double)P->end_time_ms * 1000.0) {
      sc->abandoned = true;
      if (P->comm_used) P->comm_used->abort();
      return timeout_fail(P);
    }
    if (comm_lim > 0 && (spin & 63) == 63 &&
        std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(comm_lim)) {
      sc->abandoned = true;
      P->comm_used->abort();
      return fail(PGPU_ERR_TIMEOUT, "the combine's collectives did not complete within the communicator's timeout "
                  "(%lld ms): a peer rank never joined them; communicator aborted", (long long)comm_lim);
    }
    if ((spin & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2))
      std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
}

// Raw-value leaves of a plan: its tasks, their 256-group jobs and IN keys staged through pinned memory in one device
// buffer, then raw_leaf_bitmap_kernel writes the leaves' docbits regions (sc->docbits, sized by the caller).
int launch_raw_leaves(const pgpu_plan_s* P, Scratch* sc, hipStream_t stream) {
  if (P->raw_tasks.empty()) return 0;
  std::vector<KRawJob> jobs;
  for (size_t i = 0; i < P->raw_tasks.size(); ++i) {
    const int64_t ngroups = ((int64_t)P->raw_tasks[i].num_docs + 31) / 32;
    for (int64_t g0 = 0; g0 < ngroups; g0 += kBlock) jobs.push_back(KRawJob{(int32_t)i, (int32_t)g0});
  }
  const size_t tb = P->raw_tasks.size() * sizeof(KRawTask), jb = (jobs.size() * sizeof(KRawJob) + 15) & ~size_t(15);
  const size_t vb = std::max<size_t>(P->raw_vals.size(), 1) * 8;
  TRY(sc->rawtasks.ensure(tb + jb + vb));
  TRY(sc->rawstage.ensure(tb + jb + vb));
  uint8_t* hs = reinterpret_cast<uint8_t*>(sc->rawstage.p);
  memcpy(hs, P->raw_tasks.data(), tb);
  if (!jobs.empty()) memcpy(hs + tb, jobs.data(), jobs.size() * sizeof(KRawJob));
  if (!P->raw_vals.empty()) memcpy(hs + tb + jb, P->raw_vals.data(), P->raw_vals.size() * 8);
  HIP_TRY(hipMemcpyAsync(sc->rawtasks.p, hs, tb + jb + vb, hipMemcpyHostToDevice, stream));
  uint8_t* d = sc->rawtasks.as<uint8_t>();
  if (launch_raw_leaf_bitmaps(reinterpret_cast<const KRawJob*>(d + tb), (int64_t)jobs.size(),
                              reinterpret_cast<const KRawTask*>(d), reinterpret_cast<const int64_t*>(d + tb + jb),
                              sc->docbits.as<uint32_t>(), stream))
    return fail(PGPU_ERR_DEVICE, "raw-value filter launch failed: %s", hipGetErrorString(hipGetLastError()));
  return 0;
}

// Expression leaves of a plan, staged and launched as the raw-value leaves are: expr_leaf_bitmap_kernel evaluates each
// leaf's program per doc into its docbits region.
int launch_expr_leaves(const pgpu_plan_s* P, Scratch* sc, hipStream_t stream) {
  if (P->expr_tasks.empty()) return 0;
  std::vector<KExprLeafJob> jobs;
  expr_leaf_jobs(P->expr_tasks, &jobs);
  const size_t tb = (P->expr_tasks.size() * sizeof(KExprLeafTask) + 15) & ~size_t(15);
  const size_t jb = (jobs.size() * sizeof(KExprLeafJob) + 15) & ~size_t(15);
  const size_t vb = std::max<size_t>(P->expr_vals.size(), 1) * 8;
  TRY(sc->exprtasks.ensure(tb + jb + vb));
  TRY(sc->exprstage.ensure(tb + jb + vb));
  uint8_t* hs = reinterpret_cast<uint8_t*>(sc->exprstage.p);
  memcpy(hs, P->expr_tasks.data(), P->expr_tasks.size() * sizeof(KExprLeafTask));
  if (!jobs.empty()) memcpy(hs + tb, jobs.data(), jobs.size() * sizeof(KExprLeafJob));
  if (!P->expr_vals.empty()) memcpy(hs + tb + jb, P->expr_vals.data(), P->expr_vals.size() * 8);
  HIP_TRY(hipMemcpyAsync(sc->exprtasks.p, hs, tb + jb + vb, hipMemcpyHostToDevice, stream));
  uint8_t* d = sc->exprtasks.as<uint8_t>();
  if (launch_expr_leaf_bitmaps(reinterpret_cast<const KExprLeafJob*>(d + tb), (int64_t)jobs.size(),
                               reinterpret_cast<const KExprLeafTask*>(d), reinterpret_cast<const int64_t*>(d + tb + jb),
                               sc->docbits.as<uint32_t>(), stream))
    return fail(PGPU_ERR_DEVICE, "expression filter launch failed: %s", hipGetErrorString(hipGetLastError()));
  return 0;
}

// ---- execution, in three phases so that plan_create can launch segment chunks while it still plans the rest
// (streamed plans): prologue (buffers, table init, stats), one launch per chunk of segment records, epilogue
// (star-tree kernels, slab reduce).  A plan that is not streamed is one chunk.
// KParams.pack_slot (planned with the LDS table's rows, lds_pack_slot) and narrow of a dense LDS plan, from the value
// ranges of its integer columns in every segment (sorted dictionaries: first and last entries; raw columns: their
// decoded range).  PGPU_NO_DENSE_NARROW=1: no 32-bit min / max (A/B).
static void dense_lds_forms(const pgpu_plan_s* P, int32_t* pack_slot, uint32_t* narrow) {
  *pack_slot = P->mode == MODE_LDS || P->mode == MODE_HASH ? P->pack_slot : -1;  // planned with the table layout
  *narrow = 0;
  if (!P->dense || P->mode != MODE_LDS || P->num_keys <= 1 || !P->star.empty() || P->grid <= 0) return;
  for (size_t s = 0; s < P->slot_kind.size() && s < 32; ++s) {
    const int kind = P->slot_kind[s], c = P->slot_tcol[s];
    if ((kind != SLOT_MIN_KEY && kind != SLOT_MAX_KEY) || c < 0 || c == kDocIdColumn) continue;
    if (!is_int_type(P->table->types[c])) continue;
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    bool known = true;
    for (const Segment* seg : P->segs) {
      const Column& col = seg->cols[c];
      if (col.raw) { lo = std::min(lo, col.raw_min); hi = std::max(hi, col.raw_max); }
      else if (!col.dict.iv.empty()) { lo = std::min(lo, col.dict.iv.front()); hi = std::max(hi, col.dict.iv.back()); }
      else if (col.dict.size() != 0) { known = false; break; }
    }
    if (!known || lo > hi || lo < 0) continue;
    if (hi < INT64_C(0xFFFFFFFF)) *narrow |= 1u << s;
  }
}

// ---- the prologue's phases, in stream order
// The checks that launch nothing (cancelled, past the end time), the deadline in device ticks (0: none), and the
// plan's per-execution state.
static int exec_begin(pgpu_plan_s* P, ExecCtx& X, uint64_t* deadline) {
  inflight_begin(P);
  X.t_start = trace_on() ? now_us() : 0;
  if (cancelled(P)) return cancel_fail();  // nothing is launched for a cancelled query
  *deadline = 0;
  if (P->end_time_ms > 0) {  // past the end time already: nothing is launched
    P->exec_start_ms = (int64_t)(epoch_us() / 1000.0);
    if (P->exec_start_ms >= P->end_time_ms) return timeout_fail(P);
    TRY(deadline_ticks(P->table, P->end_time_ms, deadline));
  }
  // the state a previous execution's combine left (pgpu_plan_combine): planned slot kinds, no shard, no merged table
  if (!P->slot_kind_planned.empty()) {
    P->slot_kind = P->slot_kind_planned;
    P->slot_kind_planned.clear();
  }
  P->shard = nullptr;
  P->shard_begin = P->shard_count = 0;
  P->comm_used = nullptr;
  P->comm_dense = false;
  P->k8d_counts = false;
  P->merged_records = -1;
  X.nslots = (int)P->slot_kind.size();
  X.words = P->part_hash ? 0 : (int64_t)X.nslots * P->num_keys;  // hashed partitions: records, no table
  return 0;
}

// The scratch's timing events: the four of an execution and a (start, end) pair per scan launch.
static int exec_events(Scratch* sc, int max_chunks) {
  for (auto& e : sc->ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  if ((int)sc->cev.size() < 2 * max_chunks) {
    const size_t old = sc->cev.size();
    sc->cev.resize(2 * max_chunks, nullptr);
    for (size_t i = old; i < sc->cev.size(); ++i) HIP_TRY(hipEventCreate(&sc->cev[i]));
  }
  return 0;
}

// The upload buffers and the statistics block (zeroed on the stream; P->d_stats).
static int exec_buffers(pgpu_plan_s* P, hipStream_t stream, void* d_table, ExecCtx& X) {
  Scratch* sc = P->scratch;
  TRY(sc->sets.ensure(std::max<size_t>(std::max<size_t>(P->set_words.size(), (size_t)P->set_words_bound) * 4, 16)));
  const size_t rec_cap = std::max<size_t>((size_t)P->segs.size() * P->seg_stride, P->segrec.size());
  TRY(sc->segrec.ensure(std::max<size_t>(rec_cap, 16)));
  TRY(sc->stage.ensure(std::max<size_t>(rec_cap + (size_t)std::max<int64_t>(P->set_words_bound,
                                                                             (int64_t)P->set_words.size()) * 4, 16)));
  // The statistics block (StatsWord, internal.h): right after the group table when the table is internal, so
  // finalize reads both with one copy.  (A ring of entries zeroed 256 executions at a time, instead of this fill per
  // query, was measured in r06 sessions i, j, m: no gain on C1 / C3, and C4's pipelined star-tree step lost
  // 0.17 -> 0.21 ms with the second copy it needs; not kept.)
  unsigned long long* stats;
  if (!d_table) {
    TRY(sc->table.ensure((size_t)X.words * 8 + kStatsBytes));
    stats = reinterpret_cast<unsigned long long*>(sc->table.as<uint8_t>() + (size_t)X.words * 8);
  } else {
    TRY(sc->stats.ensure(kStatsBytes));
    stats = sc->stats.as<unsigned long long>();
  }
  HIP_TRY(hipMemsetAsync(stats, 0, kStatsBytes, stream));
  P->d_stats = stats;
  X.external = d_table != nullptr;
  return 0;
}

// Where the execution's records, bitsets and tile map live: the scratch, or the cached plan's device image (built
// here once; later executions wait for it).
static int exec_image(pgpu_plan_s* P, hipStream_t stream, ExecCtx& X) {
  Scratch* sc = P->scratch;
  X.segrec = sc->segrec.as<uint8_t>();
  X.sets = sc->sets.as<uint32_t>();
  TRY(sc->tile_seg.ensure((size_t)std::max<int64_t>(std::max<int64_t>(P->num_tiles, P->tile_bound), 1) * 4));
  X.tile_seg = sc->tile_seg.as<int32_t>();
  X.from_image = P->image && P->chunks.size() == 1 && P->docbit_words == 0 && !P->set_words_bound && !P->tile_bound;
  sc->image = X.from_image ? P->image : nullptr;
  if (X.from_image) {  // build the cached plan's device image once; later executions wait for it
    DeviceImage& im = *P->image;
    std::lock_guard<std::mutex> g(im.mu);
    if (!im.uploaded) {
      const size_t rn = P->segrec.size(), sn = P->set_words.size() * 4;
      TRY(im.segrec.ensure(std::max<size_t>(rn, 16)));
      TRY(im.sets.ensure(std::max<size_t>(sn, 16)));
      TRY(im.tile_seg.ensure((size_t)std::max<int64_t>(P->num_tiles, 1) * 4));
      if (!im.built) HIP_TRY(hipEventCreateWithFlags(&im.built, hipEventDisableTiming));
      uint8_t* stage = reinterpret_cast<uint8_t*>(sc->stage.p);
      if (rn) memcpy(stage, P->segrec.data(), rn);
      for (const auto& f : P->set_fix) {
        const uint32_t* ptr = im.sets.as<uint32_t>() + f.second;
        memcpy(stage + f.first, &ptr, sizeof ptr);
      }
      if (sn) memcpy(stage + rn, P->set_words.data(), sn);
      if (rn) HIP_TRY(hipMemcpyAsync(im.segrec.p, stage, rn, hipMemcpyHostToDevice, stream));
      if (sn) HIP_TRY(hipMemcpyAsync(im.sets.p, stage + rn, sn, hipMemcpyHostToDevice, stream));
      // the plan's scan records (segments its filter prunes or its star-trees answer have none)
      const int32_t nrec = P->seg_stride > 0 ? (int32_t)(P->segrec.size() / P->seg_stride) : 0;
      if (nrec > 0 &&
          launch_expand_tiles(im.segrec.as<uint8_t>(), P->seg_stride, nrec, im.tile_seg.as<int32_t>(), 0,
                              P->d_stats, stream))
        return fail(PGPU_ERR_DEVICE, "expand launch failed: %s", hipGetErrorString(hipGetLastError()));
      HIP_TRY(hipEventRecord(im.built, stream));
      im.uploaded = true;
    } else if (!im.ready) {
      if (hipEventQuery(im.built) == hipSuccess) im.ready = true;
      else HIP_TRY(hipStreamWaitEvent(stream, im.built, 0));
    }
    X.segrec = im.segrec.as<uint8_t>();
    X.sets = im.sets.as<uint32_t>();
    X.tile_seg = im.tile_seg.as<int32_t>();
  }
  return 0;
}

// The filter's per-query docId bitmaps: inverted-index leaves, raw-value leaves and expression leaves.
static int exec_filter_bitmaps(pgpu_plan_s* P, hipStream_t stream) {
  Scratch* sc = P->scratch;
  if (P->docbit_words > 0) TRY(sc->docbits.ensure((size_t)P->docbit_words * 4));
  if (!P->bit_blocks.empty()) {  // BitmapBasedFilterOperator leaves: OR the matching dictIds' containers
    TRY(sc->bittasks.ensure(std::max<size_t>(P->bit_tasks.size(), 1) * sizeof(KBitTask)));
    TRY(sc->bitblocks.ensure(P->bit_blocks.size() * sizeof(KBitBlock)));
    // staged through pinned memory: asynchronous copies (pageable sources would block the host)
    const size_t tb = P->bit_tasks.size() * sizeof(KBitTask), bb = P->bit_blocks.size() * sizeof(KBitBlock);
    TRY(sc->bitstage.ensure(tb + bb));
    uint8_t* hs = reinterpret_cast<uint8_t*>(sc->bitstage.p);
    if (tb) memcpy(hs, P->bit_tasks.data(), tb);
    memcpy(hs + tb, P->bit_blocks.data(), bb);
    if (tb) HIP_TRY(hipMemcpyAsync(sc->bittasks.p, hs, tb, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(sc->bitblocks.p, hs + tb, bb, hipMemcpyHostToDevice, stream));
    if (launch_inv_materialize(sc->bitblocks.as<KBitBlock>(), (int64_t)P->bit_blocks.size(),
                               sc->bittasks.as<KBitTask>(), sc->docbits.as<uint32_t>(), stream))
      return fail(PGPU_ERR_DEVICE, "inverted-index materialise launch failed: %s",
                  hipGetErrorString(hipGetLastError()));
  }
  TRY(launch_raw_leaves(P, sc, stream));  // raw-value leaves' docbits regions
  return launch_expr_leaves(P, sc, stream);  // expression leaves' likewise
}

// X.kp: what every launch of the execution shares (no buffer but the statistics block; exec_tables adds the rest).
static void fill_kparams(const pgpu_plan_s* P, uint64_t deadline, ExecCtx& X) {
  const int nslots = X.nslots;
  KParams& kp = X.kp;
  memset(&kp, 0, sizeof kp);
  kp.pack_slot = -1;
  kp.deadline = deadline;
  kp.seg_stride = P->seg_stride;
  kp.num_cols = (int)P->query_cols.size();
  kp.num_ops = (int)P->ops.size();
  kp.pure_and = P->pure_and ? 1 : 0;
  for (size_t i = 0; i < P->ops.size(); ++i) kp.ops[i] = P->ops[i];
  kp.num_leaves = P->num_leaves;
  for (int i = 0; i < P->num_leaves; ++i) kp.leaf_col[i] = P->leaf_slot[i];
  kp.num_keys = (int)P->key_cols.size();
  for (size_t j = 0; j < P->key_cols.size(); ++j) {
    int slot = 0;
    for (size_t i = 0; i < P->query_cols.size(); ++i) if (P->query_cols[i] == P->key_cols[j]) slot = (int)i;
    kp.key_col[j] = slot;
    kp.key_stride[j] = P->key_stride[j];
  }
  kp.num_keys_total = P->num_keys;
  kp.key_bias = P->key_bias;
  kp.tile_shift = P->tile_shift;
  // Tile order: interleaved (the tiles in flight on an XCD come from ~one segment: its dictionaries stay in that
  // XCD's L2 for the per-doc gathers) or chunked (a workgroup's tiles follow each other in one segment: its records
  // and leaf registers are loaded once per run).  Plans with many matches (dense, and the sparse ones of estimated
  // selectivity >= 1/16) gather enough to want the former: C4's scan path 151 -> 141 us interleaved, where C3
  // (0.18 %) loses 7 % and the indexed C3 15 % (profiles/r05_ab_summary.txt, session za).
#ifdef PGPU_CHUNK_ALL  // (an A/B build of the library: contiguous runs for the dense and wide plans too)
  kp.tile_chunks = 1;
#else
  kp.tile_chunks = P->dense || P->fast_wide ? 0 : 1;  // (the plan's property, not P->variant: FX / DC plans differ)
#endif
  kp.num_slots = nslots;
  for (int sl = 0; sl < nslots; ++sl) { kp.slot_kind[sl] = P->slot_kind[sl]; kp.slot_col[sl] = P->slot_col[sl]; }
  for (int sl = 0; sl < nslots && P->fx; ++sl)  // the scan's view of the fixed-point digits (fx_split has the rest)
    if (P->slot_fx[sl] >= 0) kp.slot_kind[sl] = SLOT_SUM_FX;
  for (const pgpu_plan_s::Distinct& d : P->dc) kp.slot_kind[d.slot] = SLOT_DISTINCT;  // (X.dc has the bitmaps)
  if (!P->pct.empty()) {  // histograms only (X.hs): the rows the post-scan kernel writes, DISTINCTCOUNT's among them
    for (const pgpu_plan_s::Distinct& d : P->dc) kp.slot_kind[d.slot] = SLOT_PERCENTILE;
    for (const pgpu_plan_s::Percentile& e : P->pct) kp.slot_kind[e.slot] = SLOT_PERCENTILE;
  }
  // expression aggregations (X.ex): the programs with their operands as record indexes, and each slot's program
  memset(&X.ex, 0, sizeof X.ex);
  for (int sl = 0; sl < kMaxSlots; ++sl) X.ex.slot_prog[sl] = sl < nslots ? P->slot_expr[sl] : -1;
  X.ex.n = (int32_t)P->exprs.size();
  for (size_t e = 0; e < P->exprs.size(); ++e) {
    ExprProg& g = X.ex.prog[e];
    g = P->exprs[e].prog;
    for (int c = 0; c < g.ncols; ++c)  // (bound by plan_expr; launch_scan refuses an index outside the records)
      g.col[c] = (int32_t)(std::find(P->query_cols.begin(), P->query_cols.end(), g.col[c]) - P->query_cols.begin());
  }
  kp.pair_leaves = 1;
  dense_lds_forms(P, &kp.pack_slot, &kp.narrow);
  kp.pack_shift = P->pack_shift;
  kp.stats = P->d_stats;
}

// DISTINCTCOUNT: the aggregations' side bitmaps (X.dc), back to back in the arena's buffer and zeroed on the stream
// for this execution.
static int exec_histograms(pgpu_plan_s* P, hipStream_t stream, ExecCtx& X);
static int exec_distinct_bitmaps(pgpu_plan_s* P, hipStream_t stream, ExecCtx& X) {
  memset(&X.dc, 0, sizeof X.dc);
  memset(&X.hs, 0, sizeof X.hs);
  memset(&X.sel, 0, sizeof X.sel);
  if (!P->pct.empty()) return exec_histograms(P, stream, X);  // a plan with a PERCENTILE keeps histograms only
  if (P->dc.empty()) return 0;
  if (P->mode == MODE_HASH || (int)P->dc.size() > kMaxDistinct)
    return fail(PGPU_ERR_UNSUPPORTED, "DISTINCTCOUNT outside the dense group tables");
  Scratch* sc = P->scratch;
  int64_t words = 0;
  for (const pgpu_plan_s::Distinct& d : P->dc) words += P->num_keys * d.words;
  if (words * 8 > kDistinctMaxBytes) return fail(PGPU_ERR_UNSUPPORTED, "DISTINCTCOUNT bitmaps above the cap");
  TRY(sc->dc_bits.ensure((size_t)words * 8));
  HIP_TRY(hipMemsetAsync(sc->dc_bits.p, 0, (size_t)words * 8, stream));
  int64_t off = 0;
  X.dc.n = (int32_t)P->dc.size();
  for (size_t i = 0; i < P->dc.size(); ++i) {
    const pgpu_plan_s::Distinct& d = P->dc[i];
    X.dc.bits[i] = sc->dc_bits.as<unsigned long long>() + off;
    X.dc.words[i] = (int32_t)d.words;
    X.dc.col[i] = d.qcol;
    X.dc.slot[i] = d.slot;
    off += P->num_keys * d.words;
  }
  return 0;
}

// PERCENTILE: the side histograms (X.hs) and what the selection kernel resolves from them (X.sel).  The histograms lie
// back to back in the arena's buffer for side structures (rows 16-byte aligned: strides are multiples of 4 cells)
// and are zeroed on the stream for this execution.
static int exec_histograms(pgpu_plan_s* P, hipStream_t stream, ExecCtx& X) {
  if (P->mode == MODE_HASH || (int)P->hist.size() > kMaxDistinct || (int)P->pct.size() > kMaxSlots)
    return fail(PGPU_ERR_UNSUPPORTED, "PERCENTILE outside the dense group tables");
  Scratch* sc = P->scratch;
  int64_t cells = 0;
  for (const pgpu_plan_s::Hist& h : P->hist) cells += P->num_keys * h.stride;
  if (cells * 4 > kDistinctMaxBytes) return fail(PGPU_ERR_UNSUPPORTED, "PERCENTILE histograms above the cap");
  TRY(sc->dc_bits.ensure((size_t)cells * 4));
  HIP_TRY(hipMemsetAsync(sc->dc_bits.p, 0, (size_t)cells * 4, stream));
  int64_t off = 0;
  X.hs.n = (int32_t)P->hist.size();
  for (size_t i = 0; i < P->hist.size(); ++i) {
    const pgpu_plan_s::Hist& h = P->hist[i];
    X.hs.cells[i] = sc->dc_bits.as<uint32_t>() + off;
    X.hs.stride[i] = (int32_t)h.stride;
    X.hs.col[i] = h.qcol;
    X.sel.values[i] = h.values ? reinterpret_cast<const double*>(h.values->p) : nullptr;
    X.sel.dc_slot[i] = h.dc_slot;
    off += P->num_keys * h.stride;
  }
  for (size_t i = P->hist.size(); i < (size_t)kMaxDistinct; ++i) X.sel.dc_slot[i] = -1;
  X.sel.npct = (int32_t)P->pct.size();
  for (size_t a = 0; a < P->pct.size(); ++a) {
    X.sel.pct_slot[a] = P->pct[a].slot;
    X.sel.pct_hist[a] = P->pct[a].hist;
    X.sel.pct_e4[a] = P->pct[a].p_e4;
  }
  return 0;
}

// The accumulators: LEAP2 maps, the slabs of an LDS-table plan, or the global / hash table (initialised here) with
// its key tables.
static int exec_tables(pgpu_plan_s* P, hipStream_t stream, int max_chunks, ExecCtx& X) {
  Scratch* sc = P->scratch;
  KParams& kp = X.kp;
  const int nslots = X.nslots;
  uint64_t* table = X.table;
  if (P->leap_reserved) {  // one byte per (tile, wave) of the plan, written by the scan kernel for LEAP2 segments
    TRY(sc->leap_maps.ensure((size_t)std::max<int64_t>(std::max<int64_t>(P->num_tiles, P->tile_bound), 1) *
                             (kBlock / 64)));
    kp.leap_maps = sc->leap_maps.as<uint8_t>();
  }
  const int star_blocks = P->star_batches * P->star_chunks;
  if (P->mode == MODE_LDS) {
    TRY(sc->slab.ensure((size_t)std::max(max_chunks * P->grid + star_blocks, 1) * X.words * 8));
    kp.slab = sc->slab.as<uint64_t>();
  } else {
    if (P->mode == MODE_HASH && !P->part_hash) {
      TRY(sc->hash_keys.ensure((size_t)P->num_keys * 8));
      kp.hash_keys = sc->hash_keys.as<unsigned long long>();
      if (!P->stage_end.empty()) {
        int64_t total = 0;
        kp.num_stages = (int)P->stage_end.size();
        for (int s = 0; s < kp.num_stages; ++s) {
          kp.stage_end[s] = P->stage_end[s];
          kp.stage_cap[s] = P->stage_cap[s];
          kp.stage_mult[s] = P->stage_mult[s];
          kp.stage_off[s] = total;
          total += P->stage_cap[s];
        }
        TRY(sc->stage_keys.ensure((size_t)total * 8));
        HIP_TRY(hipMemsetAsync(sc->stage_keys.p, 0xFF, (size_t)total * 8, stream));  // every slot empty (~0)
        kp.stage_keys = sc->stage_keys.as<unsigned long long>();
      }
    }
    if (!P->partitioned &&  // the partitioned path stores every table word itself
        launch_table_init(table, P->slot_kind.data(), nslots, P->num_keys, kp.hash_keys, stream))
      return fail(PGPU_ERR_DEVICE, "table init launch failed: %s", hipGetErrorString(hipGetLastError()));
    kp.table = table;
  }
  return exec_distinct_bitmaps(P, stream, X);
}

int exec_prologue(pgpu_plan_s* P, hipStream_t stream, void* d_table, int max_chunks, ExecCtx& X) {
  uint64_t deadline = 0;
  TRY(exec_begin(P, X, &deadline));
  Scratch* sc = P->scratch;
  TRY(exec_events(sc, max_chunks));
  X.mark("events");
  PGPU_TIMING_RECORD(P, sc->ev[0], stream);
  X.mark("event 0 recorded");
  TRY(exec_buffers(P, stream, d_table, X));
  X.mark("buffers");
  TRY(exec_image(P, stream, X));
  X.mark("image");
  TRY(exec_filter_bitmaps(P, stream));
  X.table = d_table ? reinterpret_cast<uint64_t*>(d_table) : sc->table.as<uint64_t>();
  P->d_table_used = X.table;
  fill_kparams(P, deadline, X);
  TRY(exec_tables(P, stream, max_chunks, X));
  P->launches_done = 0;
  return 0;
}

// Uploads chunk c's records (SET pointers patched to the device bitsets) and its bitset words.
int exec_upload_chunk(pgpu_plan_s* P, hipStream_t stream, const ExecCtx& X, const LaunchChunk& C) {
  if (X.from_image) return 0;  // the cached plan's device image holds the records
  Scratch* sc = P->scratch;
  uint8_t* stage = reinterpret_cast<uint8_t*>(sc->stage.p);
  const size_t r0 = (size_t)C.rec_begin * P->seg_stride, rn = (size_t)C.num_recs * P->seg_stride;
  if (rn) memcpy(stage + r0, P->segrec.data() + r0, rn);
  for (int64_t i = C.fix_begin; i < C.fix_end; ++i) {
    const auto& f = P->set_fix[i];
    const uint32_t* ptr = sc->sets.as<uint32_t>() + f.second;
    memcpy(stage + f.first, &ptr, sizeof ptr);
  }
  for (const auto& f : P->bit_fix)
    if (f.first >= (int64_t)r0 && f.first < (int64_t)(r0 + rn)) {
      const uint32_t* ptr = sc->docbits.as<uint32_t>() + f.second;
      memcpy(stage + f.first, &ptr, sizeof ptr);
    }
  if (rn) HIP_TRY(hipMemcpyAsync(sc->segrec.as<uint8_t>() + r0, stage + r0, rn, hipMemcpyHostToDevice, stream));
  if (C.set_end > C.set_begin) {
    const size_t set_off = (size_t)P->segs.size() * P->seg_stride + (size_t)C.set_begin * 4;
    const size_t bytes = (size_t)(C.set_end - C.set_begin) * 4;
    if (set_off + bytes > sc->stage.cap) return fail(PGPU_ERR_DEVICE, "set staging overflow");
    memcpy(stage + set_off, P->set_words.data() + C.set_begin, bytes);
    HIP_TRY(hipMemcpyAsync(sc->sets.as<uint32_t>() + C.set_begin, stage + set_off, bytes, hipMemcpyHostToDevice,
                           stream));
  }
  return 0;
}

// PGPU_TRACE=check (diagnostics): before a scan launch, the records and tile map the kernel will read are copied
// back and compared with the plan's host records (pointer fields patched at upload skipped); a mismatch fails the
// query (PGPU_ERR_DEVICE) instead of launching on them.
bool check_launch_on() {
  static const bool on = diag("check");
  return on;
}
static int check_launch_inputs(const pgpu_plan_s* P, hipStream_t stream, const ExecCtx& X, const LaunchChunk& C) {
  HIP_TRY(hipStreamSynchronize(stream));
  const size_t r0 = (size_t)C.rec_begin * P->seg_stride, rn = (size_t)C.num_recs * P->seg_stride;
  std::vector<uint8_t> dev(rn);
  std::vector<int32_t> tiles((size_t)std::max<int64_t>(C.num_tiles, 0));
  if (rn) HIP_TRY(hipMemcpy(dev.data(), X.segrec + r0, rn, hipMemcpyDeviceToHost));
  if (!tiles.empty()) HIP_TRY(hipMemcpy(tiles.data(), X.tile_seg + C.tile_begin, tiles.size() * 4, hipMemcpyDeviceToHost));
  if (P->segrec.size() >= r0 + rn) {
    std::vector<char> skip(rn, 0);
    auto mark = [&](int64_t off) {
      if (off >= (int64_t)r0 && off + 8 <= (int64_t)(r0 + rn)) memset(skip.data() + (off - r0), 1, 8);
    };
    for (const auto& f : P->set_fix) mark(f.first);
    for (const auto& f : P->bit_fix) mark(f.first);
    for (size_t i = 0; i < rn; ++i)
      if (!skip[i] && dev[i] != P->segrec[r0 + i])
        return fail(PGPU_ERR_DEVICE, "launch check: device record byte %zu differs from the plan (%u vs %u)", r0 + i,
                    dev[i], P->segrec[r0 + i]);
  }
  int32_t prev = 0;
  for (size_t i = 0; i < tiles.size(); ++i) {
    if (tiles[i] < prev || tiles[i] >= C.num_recs)
      return fail(PGPU_ERR_DEVICE, "launch check: tile %zu maps to record %d of %lld", i, tiles[i],
                  (long long)C.num_recs);
    prev = tiles[i];
  }
  return 0;
}

// The split parameters of the plan's SLOT_SUM_FX slots (KParamsFx / KStarParams.fx).
KFxSplit fx_split(const pgpu_plan_s* P) {
  KFxSplit x;
  memset(&x, 0, sizeof x);
  for (size_t sl = 0; sl < P->slot_fx.size() && sl < (size_t)kMaxSlots && P->fx; ++sl) {
    if (P->slot_fx[sl] < 0) continue;
    const FxFormat& f = P->slot_fmt[sl];
    x.sh[sl] = (int16_t)(f.K - f.E);
    x.k[sl] = (int8_t)f.K;
    x.j[sl] = (int8_t)P->slot_fx[sl];
  }
  return x;
}

// PGPU_TRACE=wgtimes with a PGPU_DIAG_WG_TIMES build: every scan launch is synchronised and its workgroups' start /
// tile-loop end / end times (wall clock, relative to the earliest start) summarised on stderr -- how much of a launch
// is its ramp, its tail and the imbalance of the static tile split.
static unsigned long long* g_diag_times = nullptr;
static int diag_wg_times_begin(KParams& kp, int grid, hipStream_t stream) {
  constexpr int kMaxWgs = 1 << 16;
  if (grid > kMaxWgs) return 0;
  if (!g_diag_times) HIP_TRY(hipMalloc(&g_diag_times, (size_t)kMaxWgs * 64));
  HIP_TRY(hipMemsetAsync(g_diag_times, 0, (size_t)grid * 64, stream));
  kp.diag_times = g_diag_times;
  return 0;
}

static int diag_wg_times_report(pgpu_table_s* t, const KParams& kp, int grid, hipStream_t stream) {
  if (!kp.diag_times) return 0;
  std::vector<unsigned long long> h((size_t)grid * 8);
  HIP_TRY(hipMemcpyAsync(h.data(), kp.diag_times, h.size() * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  int khz = 100000;
  hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, t->device);
  const double us = 1000.0 / khz;
  unsigned long long t0 = ~0ull;
  for (int b = 0; b < grid; ++b) if (h[8 * b + 2]) t0 = std::min(t0, h[8 * b]);
  if (t0 == ~0ull) return 0;
  std::vector<double> st, le, en, tiles;
  double xcd_end[8] = {0};
  // PGPU_WGTIMES_OUT=<file>: every workgroup's raw row appended (launch separator "# grid tiles")
  FILE* raw = getenv("PGPU_WGTIMES_OUT") ? fopen(getenv("PGPU_WGTIMES_OUT"), "a") : nullptr;
  if (raw) fprintf(raw, "# %d %lld\n", grid, (long long)kp.num_tiles);
  for (int b = 0; b < grid; ++b) {
    const unsigned long long* d = &h[8 * (size_t)b];
    if (!d[2]) continue;
    st.push_back((d[0] - t0) * us);
    le.push_back((d[1] - t0) * us);
    en.push_back((d[2] - t0) * us);
    tiles.push_back((double)(d[3] & 0xffffffffu));
    xcd_end[d[5] & 7] = std::max(xcd_end[d[5] & 7], en.back());
    if (raw)
      fprintf(raw, "%d %.2f %.2f %.2f %llu %llu %llu %llu\n", b, st.back(), le.back(), en.back(), d[3] & 0xffffffffu,
              d[3] >> 32, d[4], d[5]);
  }
  if (raw) fclose(raw);
  auto pct = [](std::vector<double> v, double q) {
    std::sort(v.begin(), v.end());
    return v[std::min(v.size() - 1, (size_t)(q * (v.size() - 1) + 0.5))];
  };
  fprintf(stderr, "[pgpu] wgtimes grid %d tiles %d: start p50 %.1f max %.1f | loop end p0 %.1f p10 %.1f p50 %.1f p90 %.1f "
          "max %.1f | end max %.1f us | tiles/wg %.0f..%.0f | xcd end %.1f %.1f %.1f %.1f %.1f %.1f %.1f %.1f\n",
          grid, kp.num_tiles, pct(st, 0.5), pct(st, 1.0), pct(le, 0.0), pct(le, 0.1), pct(le, 0.5), pct(le, 0.9),
          pct(le, 1.0), pct(en, 1.0), pct(tiles, 0.0), pct(tiles, 1.0), xcd_end[0], xcd_end[1], xcd_end[2], xcd_end[3],
          xcd_end[4], xcd_end[5], xcd_end[6], xcd_end[7]);
  return 0;
}

// Run-time claims of a chunked scan launch (KParams.claim; library builds with -DPGPU_TILE_CLAIMS only): the static
// runs cover the first PGPU_CLAIM_STATIC_PM / 1000 of the tiles and the rest is claimed in runs of 1/PGPU_CLAIM_DIV
// of a workgroup's share.  The counters are the four u32 at STAT_TILE_CLAIMS of the statistics block (zeroed per
// execution; they alias STAT_STAR_SECTORS, see internal.h): launches
// 0-3 of a plan.  Measured on MI355X and not the default (r06 session b, profiles/r06_ab_summary.txt): C3's scan
// 729 -> 711 us at 1000 segments but its pipelined step 0.687 -> 0.719 ms, and at 125 segments 119 -> 145 us (every
// claimed tile reloads its segment's records behind a workgroup barrier).
#ifndef PGPU_CLAIM_STATIC_PM
#define PGPU_CLAIM_STATIC_PM 750
#endif
#ifndef PGPU_CLAIM_DIV
#define PGPU_CLAIM_DIV 16
#endif
// Chunked scans: each workgroup's run of tiles weighted by the CU slot it is dispatched to (KParams.slot_w), for a
// launch that has the CUs to itself (P->alone: its workgroups' slots are their dispatch order; beside another query's
// scan the freed slots go to the newcomers in no such order) and >= kSlotWeightMinShare tiles per workgroup.  The SIMDs
// issue the oldest wave first: equal shares end slot by slot, 1 : 1.08 : 1.17 : 1.27 (C3, 125 and 1000 segments), and
// weighted by those ratios the per-tile times spread further (4.55 / 4.92 / 5.47 / 6.06 us at 1000 segments), so
// pgpu_config.slot_weight_step defaults to the latter's inverse, 1 + 0.11 (S-1-s) (r06 sessions f, g:
// profiles/r06_ab_summary.txt); 0 gives equal shares.  max_run: the tiles per workgroup the plan reserved LDS for
// (STATS_LEAP2 bytes; the kernel's tile loop has no bound of its own) -- weights whose longest run could pass it are
// declined (returns false, equal shares), as are those past kLeapLdsTiles (slot_weights, tile_split.h).
bool set_slot_weights(KParams& kp, int grid, int num_cus, double step, int64_t max_run) {
  kp.slot_n = 0;
  if (!kp.tile_chunks || kp.claim) return true;
  bool declined = false;
  kp.slot_n = slot_weights(kp.num_tiles, grid, num_cus, step, std::min(max_run, kLeapLdsTiles), kp.slot_w, &declined);
  return !declined;
}

static void set_tile_claims(KParams& kp, unsigned long long* d_stats, int grid, int launch) {
  kp.claim = nullptr;
#ifdef PGPU_TILE_CLAIMS
  const int64_t share = (int64_t)kp.num_tiles / std::max(grid, 1);
  if (!kp.tile_chunks || grid < 64 || (grid & 7) || launch >= 4 || share < 8) return;
  kp.claim = reinterpret_cast<unsigned int*>(d_stats + STAT_TILE_CLAIMS) + launch;
  kp.claim_base = (int32_t)((int64_t)kp.num_tiles * PGPU_CLAIM_STATIC_PM / 1000);
  kp.claim_tiles = (int32_t)std::max<int64_t>(1, share / PGPU_CLAIM_DIV);
#endif
}

// ---- KPartParams of the partitioned pipeline (K8a count, scan, K8c scatter, K8d / K8h aggregate), filled in the
// order its buffers are taken
// The streams, the partition shape and the fill counters; cap: the records the chunk can produce.
static int part_shape_buffers(const pgpu_plan_s* P, int nslots, int64_t cap, KPartParams& pp) {
  Scratch* sc = P->scratch;
  pp.pshift = P->part_shift;
  pp.num_parts = P->num_parts;
  pp.num_streams = (int)P->stream_col.size();
  for (size_t j = 0; j < P->stream_col.size(); ++j) { pp.stream_col[j] = P->stream_col[j]; pp.stream_f64[j] = P->stream_f64[j]; }
  for (int sl = 0; sl < nslots; ++sl) pp.slot_stream[sl] = P->slot_stream[sl];
  TRY(sc->part_start.ensure((size_t)(P->num_parts + 1) * 4));
  const int cshift = part_coarse_shift(P->num_parts);
  pp.cshift = cshift;
  pp.num_coarse = part_coarse_runs(P->num_parts);
  pp.chunks_per_coarse = std::max(1, 1024 / pp.num_coarse);
  {  // K8e batch: as many records as fit 96 KB of LDS beside the per-partition counters, a multiple of kBlock
    const int kb = P->part_hash ? 4 : 2;  // staged key bytes
    const int64_t fixed = (int64_t)part_split_lds(cshift, pp.num_streams, 0, kb);
    const int64_t b = (96 * 1024 - fixed) / (8 * pp.num_streams + 4 + kb) / kBlock * kBlock;
    pp.split_batch = (int)std::max<int64_t>(kBlock, std::min<int64_t>(kSplitBatch, b));
  }
  TRY(sc->coarse_fill.ensure((size_t)pp.num_coarse * 4));
  TRY(sc->fine_fill.ensure((size_t)P->num_parts * 4));
  if (cshift > 0) {
    TRY(sc->mid_key.ensure((size_t)cap * 4));
    TRY(sc->mid_val.ensure(std::max<size_t>((size_t)cap * 8 * pp.num_streams, 8)));
    pp.mid_key = sc->mid_key.as<uint32_t>();
    pp.mid_val = sc->mid_val.as<uint64_t>();
  }
  pp.coarse_fill = sc->coarse_fill.as<uint32_t>();
  pp.fine_fill = sc->fine_fill.as<uint32_t>();
  return 0;
}

// The record buffers; for hashed partitions also K8h's outputs: the groups' compacted records, where finalize's
// compaction of a hash table would put them, their count and each partition's slot ranges.
static int part_record_buffers(pgpu_plan_s* P, hipStream_t stream, int nslots, int64_t cap, KPartParams& pp) {
  Scratch* sc = P->scratch;
  if (P->part_hash) {
    pp.hashed = 1;
    pp.mid_pair = pp.cshift > 0 && pp.num_streams == 1 && P->part_val32 && !P->stream_f64[0] ? 1 : 0;
    pp.pbits = P->part_pbits;
    pp.sbits = P->part_sbits;
    TRY(sc->rec_key32.ensure((size_t)cap * 4));
    pp.rec_key32 = sc->rec_key32.as<uint32_t>();
    const int64_t ocap = part_hash_out_cap(P);
    TRY(sc->ckeys.ensure((size_t)ocap * 8 * (1 + nslots)));
    TRY(sc->counter.ensure(64));
    HIP_TRY(hipMemsetAsync(sc->counter.p, 0, 8, stream));
    pp.out_rec = sc->ckeys.as<uint64_t>();
    pp.out_count = sc->counter.as<unsigned long long>();
    pp.out_cap = ocap;
    TRY(sc->part_mm.ensure((size_t)P->num_parts * 2 * nslots * 8));
    pp.out_mm = sc->part_mm.as<unsigned long long>();
    P->part_hash_live = true;
  } else {
    TRY(sc->rec_key.ensure((size_t)cap * 2));
  }
  TRY(sc->rec_val.ensure(std::max<size_t>((size_t)cap * 8 * pp.num_streams, 8)));
  pp.part_start = sc->part_start.as<uint32_t>();
  pp.rec_key = sc->rec_key.as<uint16_t>();
  pp.rec_val = sc->rec_val.as<uint64_t>();
  pp.rec_cap = cap;
  pp.val32 = P->part_val32 ? 1 : 0;
  return 0;
}

// One-word records, where the operand's range leaves room for it beside the key bits: (value - pack_min) packed above
// the partition bits of a hashed record's hk, or into the free bits of a dense record's key.  cs_pack: the
// aggregating kernel's COUNT + SUM_I64 form of such records.
static void part_record_packing(const pgpu_plan_s* P, int nslots, KPartParams& pp) {
  if (P->part_pack_range < 0) return;
  const bool count_sum = nslots == 2 && P->slot_kind[0] == SLOT_COUNT && P->slot_kind[1] == SLOT_SUM_I64 &&
                         P->slot_stream[1] == 0;
  if (P->part_hash && pp.num_streams == 1 && pp.val32 && P->part_pbits >= 1) {
    int vb = 0;
    while (vb < 32 && (P->part_pack_range >> vb) != 0) ++vb;
    if (vb <= P->part_pbits) {
      pp.fine_pack = 1;
      pp.pack_min = P->part_pack_min;
      pp.pack_range = P->part_pack_range;
      pp.cs_pack = count_sum ? 1 : 0;
    }
  } else if (!P->part_hash && pp.cshift > 0) {
    const int free_bits = 32 - (pp.pshift + pp.cshift);
    int vb = 0;
    while (vb < free_bits && (P->part_pack_range >> vb) != 0) ++vb;
    if ((P->part_pack_range >> vb) == 0) {
      pp.pack_bits = std::max(vb, 1);
      pp.pack_min = P->part_pack_min;
      pp.fine_pack = pp.pshift + pp.pack_bits <= 32 && pp.num_streams == 1 ? 1 : 0;
      pp.cs_pack = pp.fine_pack && count_sum ? 1 : 0;
      pp.pack_range = P->part_pack_range;
    }
  }
}

// pp.staged and the grid of the record passes.
static int part_staged_grid(pgpu_plan_s* P, KPartParams& pp) {
  int grid = P->part_grid;
#ifndef PGPU_PART_NO_STAGE  // (defined only by an A/B build of the library: every record stored from its lane)
  // one-word records with <= 64 coarse runs: K8c stages each wave's records by run in LDS and stores them in runs;
  // the grid (K8a's too) follows that instance's occupancy
  pp.staged = pp.cshift > 0 && pp.num_coarse <= 64 ? (pp.pack_bits > 0 ? 1 : pp.mid_pair ? 2 : 0) : 0;
  if (pp.staged) {
    if (P->part_grid_staged[pp.staged - 1] <= 0) {
      const int per_cu =
          std::max(1, std::min(occupancy_part_pass(P->part_lds, P->num_parts, pp.num_coarse, pp.staged), 4));
      P->part_grid_staged[pp.staged - 1] =
          (int)std::max<int64_t>(1, std::min<int64_t>(P->num_tiles, (int64_t)P->table->num_cus * per_cu));
    }
    grid = P->part_grid_staged[pp.staged - 1];
  }
#endif
  return grid;
}

// K8d's partitions are the ordered compaction's chunks (C5): K8d writes their counts and ranges, and finalize skips
// compact_count_kernel's pass over the table (P->k8d_counts).
static int part_k8d_counts(pgpu_plan_s* P, int nslots, KPartParams& pp) {
  Scratch* sc = P->scratch;
  const int64_t G = P->num_keys, nch = compact_ordered_chunks(G);
  if (pp.cs_pack && !P->hash && ((int64_t)1 << pp.pshift) == kCompactChunkKeys && nch == P->num_parts &&
      (int64_t)nslots * G * 8 > kHostCompactBytes) {
    TRY(sc->cslots.ensure(compact_scratch_bytes(G, nslots)));
    pp.chunk_cnt = sc->cslots.as<uint32_t>();
    pp.chunk_mm = reinterpret_cast<long long*>(sc->cslots.as<uint8_t>() + ((nch * 4 + 7) & ~int64_t(7)));
    P->k8d_counts = true;
  }
  return 0;
}

static int launch_partitioned_chunk(pgpu_plan_s* P, hipStream_t stream, const ExecCtx& X, const KParams& kp) {
  Scratch* sc = P->scratch;
  const int nslots = X.nslots;
  const int64_t cap = std::max<int64_t>(P->total_docs, 1);
  KPartParams pp;
  memset(&pp, 0, sizeof pp);
  pp.base = kp;
  TRY(part_shape_buffers(P, nslots, cap, pp));
  TRY(part_record_buffers(P, stream, nslots, cap, pp));
  part_record_packing(P, nslots, pp);
  const int grid = part_staged_grid(P, pp);
  TRY(sc->block_off.ensure((size_t)grid * pp.num_coarse * 4));
  pp.block_off = sc->block_off.as<uint32_t>();
  TRY(part_k8d_counts(P, nslots, pp));
  const KFxSplit fxs = fx_split(P);  // (plans with SLOT_SUM_FX slots: K8d / K8h split the records' doubles)
  if (launch_partitioned(pp, grid, P->part_lds, stream, P->fx ? &fxs : nullptr))
    return fail(PGPU_ERR_DEVICE, "partitioned group-by launch failed: %s", hipGetErrorString(hipGetLastError()));
  return 0;
}

// The direct scan of a chunk's tiles: claims and slot weights, what the launch looked like (P->last_scan), the
// plan's scan instance.
static int launch_scan_chunk(pgpu_plan_s* P, hipStream_t stream, ExecCtx& X, KParams& kp, int grid, int c) {
  static const bool wg_times = diag("wgtimes");
  if (wg_times) TRY(diag_wg_times_begin(kp, grid, stream));
  set_tile_claims(kp, P->d_stats, grid, c);
  bool fits = true;
  if (P->alone)
    fits = set_slot_weights(kp, grid, P->table->num_cus, P->cfg.slot_weight_step,
                            P->leap_reserved ? P->leap_tiles : kLeapLdsTiles);
  P->last_scan.tiles = kp.num_tiles;
  P->last_scan.grid = grid;
  P->last_scan.tile_chunks = kp.tile_chunks;
  P->last_scan.slot_n = kp.slot_n;
  for (int s = 0; s < kMaxCuSlots; ++s) P->last_scan.slot_w[s] = kp.slot_n ? kp.slot_w[s] : 0;
  P->last_scan.alone = P->alone;
  P->last_scan.declined = !fits;
  // (the instance's family takes what it needs: the split of the fixed-point slots, the side bitmaps, or neither)
  if (launch_scan(kp, fx_split(P), X.dc, X.hs, X.ex, P->mode, P->variant, grid, P->lds_bytes, stream))
    return fail(PGPU_ERR_DEVICE, "scan launch failed: %s", hipGetErrorString(hipGetLastError()));
  X.mark("scan launched");
  if (wg_times) TRY(diag_wg_times_report(P->table, kp, grid, stream));
  return 0;
}

// Launches the scan of chunk c (records already uploaded): tile map of its records, then the scan kernel (or the
// partitioned group-by) over its tiles into slab region c.
int exec_launch_chunk(pgpu_plan_s* P, hipStream_t stream, ExecCtx& X, const LaunchChunk& C, int c) {
  Scratch* sc = P->scratch;
  KParams kp = X.kp;
  kp.segs = X.segrec + (size_t)C.rec_begin * P->seg_stride;
  kp.num_segs = (int)C.num_recs;
  kp.num_tiles = (int32_t)C.num_tiles;
  kp.tile_seg = X.tile_seg + C.tile_begin;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(P->grid, C.num_tiles));
  if (P->mode == MODE_LDS) kp.slab = X.kp.slab + X.slabs_used * X.words;
  if (kp.leap_maps) kp.leap_maps += C.tile_begin * (kBlock / 64);
  if (X.from_image) {  // the tile map is in the image; only the deadline gate remains (and only with a deadline)
    if (C.num_tiles > 0 && kp.deadline && launch_deadline_gate(kp.deadline, kp.stats, stream))
      return fail(PGPU_ERR_DEVICE, "gate launch failed: %s", hipGetErrorString(hipGetLastError()));
  } else if (C.num_recs > 0 && launch_expand_tiles(kp.segs, kp.seg_stride, kp.num_segs, X.tile_seg + C.tile_begin,
                                                   kp.deadline, kp.stats, stream)) {
    return fail(PGPU_ERR_DEVICE, "expand launch failed: %s", hipGetErrorString(hipGetLastError()));
  }
  if (check_launch_on()) TRY(check_launch_inputs(P, stream, X, C));
  X.mark("chunk set up");
  if (c == 0) PGPU_TIMING_RECORD(P, sc->ev[1], stream);
  PGPU_TIMING_RECORD(P, sc->cev[2 * c], stream);
  if (C.num_tiles > 0 && P->partitioned) TRY(launch_partitioned_chunk(P, stream, X, kp));
  else if (C.num_tiles > 0) TRY(launch_scan_chunk(P, stream, X, kp, grid, c));
  PGPU_TIMING_RECORD(P, sc->cev[2 * c + 1], stream);
  if (C.num_tiles > 0 && P->any_leap2 && P->leap_reserved && !P->partitioned) {
    if (P->chunks.size() == 1 && P->mode == MODE_LDS) {  // folded into the epilogue's launch
      X.leap_segs = kp.segs;
      X.leap_nsegs = kp.num_segs;
    } else if (launch_leap2_compose(kp.segs, kp.seg_stride, kp.num_segs, kp.leap_maps, kp.stats, stream)) {
      return fail(PGPU_ERR_DEVICE, "filter statistics launch failed: %s", hipGetErrorString(hipGetLastError()));
    }
  }
  if (C.num_tiles > 0 && !P->partitioned && P->mode == MODE_LDS) X.slabs_used += grid;
  P->launches_done = c + 1;
  return 0;
}

// Star-tree segments: their records (this scratch's work buffers, the plan's match sets), then the K5 traversal and
// the K6 residual scan + aggregation into the same group table.
static int epilogue_star(pgpu_plan_s* P, hipStream_t stream, ExecCtx& X) {
  Scratch* sc = P->scratch;
  const int nslots = X.nslots;
  const int64_t words = X.words;
  const KParams& kp = X.kp;
  X.mark("before star buffers");
  TRY(sc->starwork.ensure((size_t)P->star_work_bytes + P->star.size() * 8 + 16));
  int64_t* seg_total = reinterpret_cast<int64_t*>(sc->starwork.as<uint8_t>() + P->star_work_bytes);
  {
    const void* before = sc->starrec.p;
    TRY(sc->starrec.ensure(P->star.size() * sizeof(KStarSeg)));
    if (sc->starrec.p != before) sc->starrec_sent.clear();  // a new buffer holds nothing yet
  }
  std::vector<KStarSeg> recs = P->star;
  for (size_t i = 0; i < recs.size(); ++i) {
    uint8_t* base = sc->starwork.as<uint8_t>() + P->star_work_off[i];
    const int64_t nn = recs[i].num_nodes;
    recs[i].ranges = reinterpret_cast<int32_t*>(base);
    recs[i].prefix = reinterpret_cast<int64_t*>(base + ((2 * nn * 4 + 7) & ~int64_t(7)));
    recs[i].frontier = reinterpret_cast<int32_t*>(base + ((2 * nn * 4 + 7) & ~int64_t(7)) + (nn + 1) * 8);
    recs[i].out = recs[i].frontier + 6 * nn;
  }
  for (auto& f : P->star_match_fix)
    recs[std::get<0>(f)].match[std::get<1>(f)] = X.sets + std::get<2>(f);
  // The records (this scratch's work buffers, the plan's match sets) are the same for every execution of a cached
  // plan on this scratch: uploaded when they differ from the last upload.  A small host-to-device copy could block
  // the host for milliseconds behind other streams' work (C4 at 3 queries in flight: 5.4 ms in one execution).
  const size_t rbytes = recs.size() * sizeof(KStarSeg);
  X.mark("star buffers + records built");
  if (sc->starrec_sent.size() != rbytes || memcmp(sc->starrec_sent.data(), recs.data(), rbytes) != 0) {
    TRY(sc->starstage.ensure(rbytes));
    memcpy(sc->starstage.p, recs.data(), rbytes);
    HIP_TRY(hipMemcpyAsync(sc->starrec.p, sc->starstage.p, rbytes, hipMemcpyHostToDevice, stream));
    sc->starrec_sent.assign(reinterpret_cast<const uint8_t*>(recs.data()),
                            reinterpret_cast<const uint8_t*>(recs.data()) + rbytes);
  }
  X.mark("star records copy queued");
  if (launch_startree_traverse(sc->starrec.as<KStarSeg>(), (int)recs.size(), seg_total, kp.deadline, kp.stats,
                               stream))
    return fail(PGPU_ERR_DEVICE, "star-tree traversal launch failed: %s", hipGetErrorString(hipGetLastError()));
  X.mark("K5 launched");
  KStarParams sp;
  memset(&sp, 0, sizeof sp);
  sp.num_wgs = P->star_chunks;
  sp.range_cache = P->star_range_cache;
  sp.num_keys = (int)P->key_cols.size();
  for (size_t j = 0; j < P->key_cols.size(); ++j) sp.key_stride[j] = P->key_stride[j];
  sp.key_bias = P->key_bias;
  sp.num_keys_total = P->num_keys;
  sp.num_slots = nslots;
  for (int sl = 0; sl < nslots; ++sl) {
    sp.slot_kind[sl] = X.kp.slot_kind[sl];  // (SLOT_SUM_FX where the plan has fixed-point digits)
    sp.slot_int[sl] = sl > 0 && P->slot_tcol[sl] >= 0 && is_int_type(P->table->types[P->slot_tcol[sl]]) ? 1 : 0;
  }
  sp.fx = fx_split(P);
  sp.table = kp.table;
  sp.slab = P->mode == MODE_LDS ? kp.slab + X.slabs_used * words : nullptr;
  sp.hash_keys = kp.hash_keys;
  sp.stats = kp.stats;
  sp.deadline = kp.deadline;
  sp.cache_ints = P->star_cache_ints;
  for (int b = 0; b < P->star_batches; ++b) {  // kStarMaxSegs segments per launch, slabs back to back
    const int s0 = b * kStarMaxSegs;
    sp.segs = sc->starrec.as<KStarSeg>() + s0;
    sp.num_segs = (int)std::min<int64_t>(kStarMaxSegs, (int64_t)recs.size() - s0);
    sp.seg_total = seg_total + s0;
    if (P->mode == MODE_LDS) sp.slab = kp.slab + (X.slabs_used + (int64_t)b * P->star_chunks) * words;
    if (launch_startree_scan(sp, P->mode, P->fx, P->star_lds_bytes, stream))
      return fail(PGPU_ERR_DEVICE, "star-tree scan launch failed: %s", hipGetErrorString(hipGetLastError()));
    X.mark("K6 launched");
  }
  return 0;
}

// STATS_GENERIC segments: the leaves' match bitmaps, read back and replayed on the host at finalize.
static int epilogue_generic_masks(pgpu_plan_s* P, hipStream_t stream, const ExecCtx& X) {
  Scratch* sc = P->scratch;
  std::vector<KMaskJob> jobs;
  for (const auto& g : P->generic)
    for (int64_t g0 = 0; g0 < ((int64_t)g.num_docs + 31) / 32; g0 += kBlock)
      jobs.push_back(KMaskJob{(int32_t)g.rec, (int32_t)g0, g.out_word});
  TRY(sc->mask_jobs.ensure(std::max<size_t>(jobs.size(), 1) * sizeof(KMaskJob)));
  TRY(sc->leaf_masks.ensure((size_t)std::max<int64_t>(P->generic_words, 1) * 4));
  TRY(sc->maskstage.ensure(std::max<size_t>(jobs.size() * sizeof(KMaskJob), (size_t)P->generic_words * 4) + 16));
  memcpy(sc->maskstage.p, jobs.data(), jobs.size() * sizeof(KMaskJob));
  HIP_TRY(hipMemcpyAsync(sc->mask_jobs.p, sc->maskstage.p, jobs.size() * sizeof(KMaskJob), hipMemcpyHostToDevice,
                         stream));
  KParams mp = X.kp;
  mp.segs = X.segrec;
  if (launch_leaf_masks(mp, sc->mask_jobs.as<KMaskJob>(), (int32_t)jobs.size(), sc->leaf_masks.as<uint32_t>(),
                        stream))
    return fail(PGPU_ERR_DEVICE, "leaf mask launch failed: %s", hipGetErrorString(hipGetLastError()));
  HIP_TRY(hipMemcpyAsync(sc->maskstage.p, sc->leaf_masks.p, (size_t)P->generic_words * 4, hipMemcpyDeviceToHost,
                         stream));
  return 0;
}

// MODE_LDS: folds every slab written -- the scan launches' (back to back) and the star-tree chunks' after them -- into
// the table, with the deferred leap-frog statistics in the same launch; no slab: the table's initial values.
static int epilogue_fold(pgpu_plan_s* P, hipStream_t stream, ExecCtx& X) {
  const KParams& kp = X.kp;
  const int64_t all = X.slabs_used + (int64_t)P->star_batches * P->star_chunks;
  if (all == 0) {
    if (launch_table_init(X.table, P->slot_kind.data(), X.nslots, P->num_keys, nullptr, stream))
      return fail(PGPU_ERR_DEVICE, "table init launch failed");
  } else if (launch_epilogue(kp.slab, P->slot_kind.data(), X.nslots, P->num_keys, (int32_t)all, X.table, X.leap_segs,
                             P->seg_stride, X.leap_nsegs, kp.leap_maps, kp.stats, stream)) {
    return fail(PGPU_ERR_DEVICE, "reduce launch failed: %s", hipGetErrorString(hipGetLastError()));
  }
  X.leap_nsegs = 0;
  X.mark("epilogue launched");
  return 0;
}

// PGPU_TRACE: the execution's host time, and its marks when it took over a millisecond.
static void trace_execution(const ExecCtx& X) {
  const double end = now_us();
  fprintf(stderr, "[pgpu] execute: %.1f us host\n", end - X.t_start);
  static const bool all_marks = diag("marks");  // PGPU_TRACE=1,marks: every execution's marks
  if (end - X.t_start > 1000.0 || all_marks) {
    double prev = X.t_start;
    for (const auto& m : X.marks) {
      fprintf(stderr, "[pgpu]   %s +%.1f us\n", m.first, m.second - prev);
      prev = m.second;
    }
    fprintf(stderr, "[pgpu]   (end) +%.1f us\n", end - prev);
  }
}

int exec_epilogue(pgpu_plan_s* P, hipStream_t stream, ExecCtx& X) {
  Scratch* sc = P->scratch;
  const KParams& kp = X.kp;
  if (P->launches_done == 0) PGPU_TIMING_RECORD(P, sc->ev[1], stream);
  if (!P->star.empty()) TRY(epilogue_star(P, stream, X));
  if (!P->generic.empty()) TRY(epilogue_generic_masks(P, stream, X));
  PGPU_TIMING_RECORD(P, sc->ev[2], stream);
  X.mark("event 2 recorded");
  if (P->mode == MODE_LDS) TRY(epilogue_fold(P, stream, X));
  if (P->mode == MODE_HASH && !P->part_hash && kp.pack_slot >= 0 &&
      launch_hash_unpack(X.table, kp.hash_keys, P->num_keys, kp.pack_slot, kp.pack_shift, stream))
    return fail(PGPU_ERR_DEVICE, "hash unpack launch failed: %s", hipGetErrorString(hipGetLastError()));
  // DISTINCTCOUNT: the table is whole (slabs folded) -- its rows take the per-key popcounts of the side bitmaps
  if (X.dc.n > 0 && launch_distinct_popcount(X.dc, X.table, P->num_keys, stream))
    return fail(PGPU_ERR_DEVICE, "distinct popcount launch failed: %s", hipGetErrorString(hipGetLastError()));
  // PERCENTILE: likewise -- its rows take the values selected from the side histograms (and DISTINCTCOUNT's the
  // non-zero cells)
  if (X.hs.n > 0 && launch_percentile_select(X.hs, X.sel, X.table, P->num_keys, stream))
    return fail(PGPU_ERR_DEVICE, "percentile selection launch failed: %s", hipGetErrorString(hipGetLastError()));
  if (X.leap_nsegs > 0 &&  // deferred but no fold ran (cannot happen for a plan with scan tiles; kept exact)
      launch_leap2_compose(X.leap_segs, P->seg_stride, X.leap_nsegs, kp.leap_maps, kp.stats, stream))
    return fail(PGPU_ERR_DEVICE, "filter statistics launch failed: %s", hipGetErrorString(hipGetLastError()));
  PGPU_TIMING_RECORD(P, sc->ev[3], stream);
  P->last_stream = stream;
  P->executed = true;
  if (trace_on()) trace_execution(X);
  return 0;
}

int plan_execute_impl(pgpu_plan_s* P, hipStream_t stream, void* d_table) {
  const int nl = (int)P->chunks.size();
  ExecCtx X;
  TRY(exec_prologue(P, stream, d_table, std::max(nl, 1), X));
  for (int c = 0; c < nl; ++c) {
    TRY(exec_upload_chunk(P, stream, X, P->chunks[c]));
    TRY(exec_launch_chunk(P, stream, X, P->chunks[c], c));
  }
  return exec_epilogue(P, stream, X);
}

}  // namespace pgpu
