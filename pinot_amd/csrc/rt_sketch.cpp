// rt_sketch.cpp -- byte-code sketches of wide dictionary filter columns (col_sketch.h): built once when a segment is
// pinned or generated, and the C ABI that controls and reports them.  A pinned segment is immutable, so the 8-bit copy
// is made once in its life and every later query whose predicate it answers exactly scans 8 bits per doc instead of the
// column's 12..31.
#include "rt_decls.h"

namespace pgpu {

namespace {
// columns of more dictIds than this get no sketch (the histogram's pass grid; no segment comes near it)
constexpr int32_t kSketchMaxCard = 1 << 28;
}  // namespace

// Step 1 of 2, queued on `st`: the doc histogram of every qualifying column -- dictionary-encoded, fixed-bit, not
// sorted, at least min_bits wide -- and its copy into b->h_counts.  The caller synchronises `st` (the pin's own
// synchronize) before sketch_finish.
int sketch_begin(pgpu_table_s* t, Segment* seg, hipStream_t st, SketchBuild* b) {
  int32_t min_bits;
  {
    std::lock_guard<std::mutex> g(t->cfg_mu);
    min_bits = t->sketch_min_bits;
    b->min_cover = t->sketch_min_cover;
  }
  b->cols.clear();
  b->off.clear();
  if (min_bits <= 0 || seg->num_docs <= 0) return 0;
  int64_t total = 0;
  for (size_t c = 0; c < seg->cols.size(); ++c) {
    const Column& col = seg->cols[c];
    if (col.raw || col.sorted || !col.d_fwd || col.bits < min_bits || col.bits <= kSketchBits || col.card <= 0 ||
        col.card > kSketchMaxCard)
      continue;
    b->cols.push_back((int)c);
    b->off.push_back(total);
    total += col.card;
  }
  if (b->cols.empty()) return 0;
  TRY(b->d_counts.ensure((size_t)total * 4));
  HIP_TRY(hipMemsetAsync(b->d_counts.p, 0, (size_t)total * 4, st));
  for (size_t k = 0; k < b->cols.size(); ++k) {
    const Column& col = seg->cols[b->cols[k]];
    if (launch_sketch_hist(col.d_fwd, col.bits, seg->num_docs, col.card, b->d_counts.as<uint32_t>() + b->off[k], st))
      return fail(PGPU_ERR_DEVICE, "sketch histogram launch failed: %s", hipGetErrorString(hipGetLastError()));
  }
  b->h_counts.resize((size_t)total);
  HIP_TRY(hipMemcpyAsync(b->h_counts.data(), b->d_counts.p, (size_t)total * 4, hipMemcpyDeviceToHost, st));
  return 0;
}

// Step 2 of 2, after `st` was synchronised: the code assignment per column; a sketch whose singleton codes cover at
// least min_cover of the docs is kept -- its dictId -> code table goes to the device and the encode kernel writes the
// code bytes -- and counted in the table's device_bytes.  Synchronises `st` itself before its staging memory goes.
int sketch_finish(pgpu_table_s* t, Segment* seg, hipStream_t st, SketchBuild* b) {
  if (b->cols.empty()) return 0;
  std::vector<size_t> kept;
  std::vector<int64_t> lut_off;
  std::vector<uint8_t> luts;  // the kept columns' tables, each 256-byte aligned
  for (size_t k = 0; k < b->cols.size(); ++k) {
    Column& col = seg->cols[b->cols[k]];
    ColSketch s;
    sketch_assign(b->h_counts.data() + b->off[k], col.card, &s);
    if (s.ncodes <= 0 || s.total_docs != seg->num_docs) continue;  // (a forward index with dictIds past the dictionary)
    if ((double)s.singleton_docs < b->min_cover * (double)s.total_docs) continue;
    lut_off.push_back((int64_t)luts.size());
    luts.insert(luts.end(), s.lut.begin(), s.lut.end());
    luts.resize((luts.size() + 255) & ~size_t(255), 0);
    col.sketch = std::move(s);
    kept.push_back(k);
  }
  if (kept.empty()) return 0;
  DevBuf d_luts;
  struct Release { DevBuf& b; ~Release() { b.release(); } } release_luts{d_luts};
  TRY(d_luts.ensure(luts.size()));
  HIP_TRY(hipMemcpyAsync(d_luts.p, luts.data(), luts.size(), hipMemcpyHostToDevice, st));
  int rc = 0;
  for (size_t i = 0; i < kept.size() && !rc; ++i) {
    Column& col = seg->cols[b->cols[kept[i]]];
    const int64_t bytes = padded_fwd_words(seg->num_docs, kSketchBits) * 4;
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, (size_t)bytes);
    if (e != hipSuccess) {
      rc = fail(e == hipErrorOutOfMemory ? PGPU_ERR_OUT_OF_MEMORY : PGPU_ERR_DEVICE, "sketch of column %d: %s",
                b->cols[kept[i]], hipGetErrorString(e));
      break;
    }
    col.d_sketch = reinterpret_cast<uint8_t*>(p);
    col.sketch_bytes = bytes;
    t->device_bytes += bytes;
    if (hipMemsetAsync(p, 0, (size_t)bytes, st) != hipSuccess ||
        launch_sketch_encode(col.d_fwd, col.bits, seg->num_docs, col.card, d_luts.as<uint8_t>() + lut_off[i],
                             reinterpret_cast<uint32_t*>(p), st))
      rc = fail(PGPU_ERR_DEVICE, "sketch encode launch failed: %s", hipGetErrorString(hipGetLastError()));
  }
  const hipError_t es = hipStreamSynchronize(st);
  if (!rc && es != hipSuccess) rc = fail(PGPU_ERR_DEVICE, "sketch build: %s", hipGetErrorString(es));
  if (rc) {  // no half-built sketch is left for a plan to find (the bytes go with account_unpin / ~Segment)
    for (size_t k : kept) seg->cols[b->cols[k]].sketch = ColSketch();
  }
  return rc;
}

}  // namespace pgpu

extern "C" {

int pgpu_table_set_filter_sketch(pgpu_table t, int32_t min_bits, double min_cover) try {
  PGPU_ABI_GUARD;
  if (!t || min_bits < 0 || min_bits > 31 || !(min_cover >= 0.0 && min_cover <= 1.0))
    return fail(PGPU_ERR_INVALID_ARGUMENT, "bad filter-sketch arguments");
  {
    std::lock_guard<std::mutex> g(t->cfg_mu);
    t->sketch_min_bits = min_bits;
    t->sketch_min_cover = min_cover;
  }
  t->version.fetch_add(1);  // compiled plans were made with the previous setting
  plan_cache_clear(t);
  return 0;
} PGPU_ABI_CATCH

int pgpu_segment_sketch_info(pgpu_table t, int64_t h, int32_t column, int32_t* ncodes, int64_t* singleton_docs,
                             int64_t* bytes, int32_t* first_id_out, int32_t cap) try {
  PGPU_ABI_GUARD;
  if (!t || !ncodes || cap < 0 || (cap > 0 && !first_id_out)) return fail(PGPU_ERR_INVALID_ARGUMENT, "bad arguments");
  std::lock_guard<std::mutex> lk(t->mu);
  auto it = t->segments.find(h);
  if (it == t->segments.end()) return fail(PGPU_ERR_NOT_FOUND, "unknown segment handle %lld", (long long)h);
  const Segment& seg = *it->second;
  if (column < 0 || column >= (int)seg.cols.size()) return fail(PGPU_ERR_INVALID_ARGUMENT, "bad column %d", column);
  const Column& col = seg.cols[column];
  const bool has = col.d_sketch && col.sketch.ncodes > 0;
  *ncodes = has ? col.sketch.ncodes : 0;
  if (singleton_docs) *singleton_docs = has ? col.sketch.singleton_docs : 0;
  if (bytes) *bytes = has ? col.sketch_bytes : 0;
  for (int32_t k = 0; has && k < cap && k <= col.sketch.ncodes; ++k) first_id_out[k] = col.sketch.first_id[k];
  return 0;
} PGPU_ABI_CATCH

int pgpu_plan_sketch_leaves(pgpu_plan P, int64_t* pairs_using_sketch, int64_t* pairs_declined) try {
  PGPU_ABI_GUARD;
  if (!P || !pairs_using_sketch || !pairs_declined) return fail(PGPU_ERR_INVALID_ARGUMENT, "bad arguments");
  *pairs_using_sketch = P->sketch_leaves[0];
  *pairs_declined = P->sketch_leaves[1];
  for (const auto& part : P->parts) {
    *pairs_using_sketch += part.plan->sketch_leaves[0];
    *pairs_declined += part.plan->sketch_leaves[1];
  }
  return 0;
} PGPU_ABI_CATCH

}  // extern "C"
