// rt_regex.cpp -- REGEXP_LIKE / LIKE on the host side of the device: the pattern compiled (regex_dfa.h), a STRING
// column's table-global dictionary kept on the device per snapshot, the DFA run over it (k_regex.hip) and the matching
// global dictIds turned into the bitsets over the planned segments' local dictIds that the scan reads as LEAF_SETs.
// Everything here runs when a plan is made: the dictionary's device copy and the LUTs are taken under the table mutex
// (regex_job_snapshot), the kernels run after it is released (regex_job_run), in a pooled scratch's memory; a plan's
// executions read the words it was planned with.
#include "rt_decls.h"

namespace pgpu {
namespace {

// PGPU_TRACE=regex: the two kernels between event pairs, one line per call on stderr
struct Events {
  hipEvent_t e[4] = {};
  bool on;
  explicit Events(bool on_) : on(on_) { for (auto& x : e) if (on) hipEventCreate(&x); }
  ~Events() { for (auto& x : e) if (x) hipEventDestroy(x); }
  void mark(int k, hipStream_t st) { if (on) hipEventRecord(e[k], st); }
  double us(int k) const { float ms = 0; return on && hipEventElapsedTime(&ms, e[k], e[k + 1]) == hipSuccess ? ms * 1e3 : 0.0; }
};

// (under the table mutex) The current snapshot of column col's global dictionary on the device: the values back to
// back, padded to whole 8-byte words plus one (the widest load of the last value stays inside), and offsets[n + 1].
// The snapshot's flag -- every value ASCII without \n or \r, computed here where the strings are -- is kept with it;
// a snapshot outside the limit is declined and nothing is uploaded.  The entry becomes the snapshot's only once
// everything has succeeded: a failed upload leaves the previous entry, and the next call tries again.
int ensure_device_dict(pgpu_table_s* t, int col, hipStream_t stream) {
  if (t->ddicts.size() < t->global.size()) t->ddicts.resize(t->global.size());
  pgpu_table_s::DeviceDict& dd = t->ddicts[col];
  const uint64_t version = t->global_version[col];
  if (dd.version != version) {
    const Dict& g = *t->global[col];
    int64_t total = 0, bad = -1;
    for (size_t i = 0; i < g.sv.size(); ++i) {
      total += (int64_t)g.sv[i].size();
      if (bad < 0 && !regex_value_ok(reinterpret_cast<const uint8_t*>(g.sv[i].data()), g.sv[i].size())) bad = (int64_t)i;
    }
    pgpu_table_s::DeviceDict nd;
    nd.n = (int64_t)g.sv.size();
    nd.bad_value = bad;
    nd.too_large = total >= (INT64_C(1) << 31);
    if (bad < 0 && !nd.too_large) {
      const size_t padded = (((size_t)total + 7) & ~size_t(7)) + 8;
      std::vector<uint8_t> blob(padded, 0);
      std::vector<uint32_t> offs(g.sv.size() + 1, 0);
      size_t at = 0;
      for (size_t i = 0; i < g.sv.size(); ++i) {
        memcpy(blob.data() + at, g.sv[i].data(), g.sv[i].size());
        at += g.sv[i].size();
        offs[i + 1] = (uint32_t)at;
      }
      auto b = std::make_shared<DevMem>(), o = std::make_shared<DevMem>();
      HIP_TRY(hipMalloc(&b->p, padded));
      HIP_TRY(hipMalloc(&o->p, offs.size() * 4));
      HIP_TRY(hipMemcpyAsync(b->p, blob.data(), padded, hipMemcpyHostToDevice, stream));
      HIP_TRY(hipMemcpyAsync(o->p, offs.data(), offs.size() * 4, hipMemcpyHostToDevice, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      nd.blob = std::move(b);
      nd.offsets = std::move(o);
      nd.bytes = (int64_t)(padded + offs.size() * 4);
    }
    nd.version = version;
    t->device_bytes += nd.bytes - dd.bytes;
    dd = std::move(nd);  // (the previous snapshot's arrays live on in the jobs that still reference them)
  }
  if (dd.bad_value >= 0)
    return fail(PGPU_ERR_UNSUPPORTED, "REGEXP_LIKE on column %s: its dictionary holds a value with a non-ASCII byte, a \\n "
                "or a \\r (global dictId %lld), where the automaton is not the reference's matcher",
                t->names[col].c_str(), (long long)dd.bad_value);
  if (dd.too_large)
    return fail(PGPU_ERR_UNSUPPORTED, "REGEXP_LIKE on column %s: a dictionary of 2^31 bytes or more", t->names[col].c_str());
  return 0;
}

}  // namespace

int regex_compile_pattern(const char* pattern, RegexDfa* d) {
  if (!pattern) return fail(PGPU_ERR_INVALID_ARGUMENT, "REGEXP_LIKE: null pattern");
  std::string err;
  if (regex_compile(pattern, strlen(pattern), d, &err))
    return fail(PGPU_ERR_UNSUPPORTED, "REGEXP_LIKE pattern outside the accepted subset: %s", err.c_str());
  return 0;
}

int regex_check(const char* pattern, int32_t* states, int32_t* classes, int64_t* table_bytes) {
  RegexDfa d;
  TRY(regex_compile_pattern(pattern, &d));
  if (states) *states = d.num_states;
  if (classes) *classes = d.num_classes;
  if (table_bytes) *table_bytes = d.table_bytes();
  return 0;
}

int regex_match_host(const char* pattern, const uint8_t* value, int64_t len, int32_t* matched) {
  // the pattern compiled last on this thread is kept: a caller that tries many values against one pattern compiles once
  thread_local std::string last;
  thread_local RegexDfa dfa;
  thread_local bool have = false;
  if (!pattern) return fail(PGPU_ERR_INVALID_ARGUMENT, "REGEXP_LIKE: null pattern");
  if (!have || last != pattern) {
    have = false;
    TRY(regex_compile_pattern(pattern, &dfa));
    last = pattern;
    have = true;
  }
  *matched = regex_match(dfa, value, (size_t)len) ? 1 : 0;
  return 0;
}

// A REGEXP_LIKE predicate's column: a real STRING dictionary column (RegexpLikePredicateEvaluatorFactory.java:47).
int regex_check_column(const pgpu_table_s* t, const std::vector<Segment*>& segs, int col) {
  if (col < 0 || col >= (int)t->names.size())
    return fail(PGPU_ERR_UNSUPPORTED, "REGEXP_LIKE on column %d, which is no column of the table's own (a virtual or "
                "derived column)", col);
  if (t->types[col] != PGPU_STRING)
    return fail(PGPU_ERR_UNSUPPORTED, "REGEXP_LIKE on column %s, which is not a STRING column", t->names[col].c_str());
  for (const Segment* s : segs)
    if (s->cols[col].raw)
      return fail(PGPU_ERR_UNSUPPORTED, "REGEXP_LIKE on raw (no-dictionary) column %s", t->names[col].c_str());
  return 0;
}

int regex_job_snapshot(pgpu_table_s* t, const std::vector<Segment*>& segs, int col, RegexJob* job) {
  TRY(ensure_device_dict(t, col, t->stream));
  const pgpu_table_s::DeviceDict& dd = t->ddicts[col];
  job->col = col;
  job->name = t->names[col];
  job->blob = dd.blob;
  job->offsets = dd.offsets;
  job->n = dd.n;
  job->dict_bytes = dd.bytes;
  // the LUTs of the same snapshot (taken under the same lock): every global id they hold is inside the bitmap
  job->tasks.assign(segs.size(), KRegexSetTask{});
  job->luts.clear();
  job->out_words = 0;
  job->max_card = 0;
  job->affine = 0;
  for (size_t i = 0; i < segs.size(); ++i) {
    TRY(ensure_lut(t, *segs[i], col, t->stream));
    const Column& c = segs[i]->cols[col];
    job->luts.push_back(c.lut);
    KRegexSetTask& k = job->tasks[i];
    k.lut = c.lut_off >= 0 ? nullptr : reinterpret_cast<const int32_t*>(c.lut->p);
    k.lut_off = c.lut_off;
    k.card = c.card;
    k.dst = job->out_words;
    job->out_words += regex_set_words(c.card);
    job->max_card = std::max(job->max_card, c.card);
    job->affine += c.lut_off >= 0;
  }
  return 0;
}

namespace {
int regex_job_run_on(pgpu_table_s* t, RegexJob* job, uint64_t* global_out, hipStream_t stream, Scratch* sc,
                     std::vector<uint8_t>& stage, std::vector<uint32_t>& out);
}

// The work itself is regex_job_run_on's.  Whatever it returns, nothing it queued is left behind: the stream is
// synchronised before the scratch goes back to the pool and before the host buffers of the asynchronous copies (kept
// here, so that they outlive every return of the work) are destroyed.
int regex_job_run(pgpu_table_s* t, RegexJob* job, uint64_t* global_out) {
  hipStream_t stream = hipStreamPerThread;  // only this call's work is waited for
  std::vector<uint8_t> stage;
  std::vector<uint32_t> out;
  Scratch* sc = acquire_scratch(t);
  const int rc = regex_job_run_on(t, job, global_out, stream, sc, stage, out);
  if (rc) hipStreamSynchronize(stream);  // (a failure's own code is the one reported)
  release_scratch(t, sc);
  return rc;
}

namespace {
int regex_job_run_on(pgpu_table_s* t, RegexJob* job, uint64_t* global_out, hipStream_t stream, Scratch* sc,
                     std::vector<uint8_t>& stage, std::vector<uint32_t>& out) {
  static const bool timed = diag("regex");
  const double t_begin = timed ? now_us() : 0;
  const RegexDfa& d = job->dfa;
  // one upload: the class map, the table padded to whole 8-byte words, the tasks
  const size_t table_bytes = ((size_t)d.table_bytes() + 7) & ~size_t(7);
  const size_t tasks_at = kRegexClsBytes + table_bytes, tasks_bytes = job->tasks.size() * sizeof(KRegexSetTask);
  stage.assign(tasks_at + tasks_bytes, 0);
  memcpy(stage.data(), d.cls, kRegexClsBytes);
  memcpy(stage.data() + kRegexClsBytes, d.table.data(), (size_t)d.table_bytes());
  if (tasks_bytes) memcpy(stage.data() + tasks_at, job->tasks.data(), tasks_bytes);
  const size_t words = (size_t)std::max<int64_t>((job->n + 63) / 64, 1);
  // device memory of the pooled scratch: grown when needed, never allocated and freed per plan
  TRY(sc->rawtasks.ensure(stage.size()));
  TRY(sc->bitmap.ensure(words * 8));
  TRY(sc->sets.ensure(std::max<size_t>((size_t)job->out_words * 4, 16)));
  Events ev(timed);
  HIP_TRY(hipMemcpyAsync(sc->rawtasks.p, stage.data(), stage.size(), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(sc->bitmap.p, 0, words * 8, stream));
  ev.mark(0, stream);
  const uint8_t* p = sc->rawtasks.as<uint8_t>();
  if (launch_regex_match_dict(p, reinterpret_cast<const uint16_t*>(p + kRegexClsBytes), (int32_t)d.table.size(),
                              d.num_classes, d.start_row, d.cls[kRegexEos], reinterpret_cast<const uint8_t*>(job->blob->p),
                              reinterpret_cast<const uint32_t*>(job->offsets->p), job->n, sc->bitmap.as<uint64_t>(), stream))
    return fail(PGPU_ERR_DEVICE, "regex match launch failed: %s", hipGetErrorString(hipGetLastError()));
  ev.mark(1, stream);
  out.assign((size_t)job->out_words, 0u);
  const bool local = !job->tasks.empty() && job->out_words > 0;
  if (local) {
    HIP_TRY(hipMemsetAsync(sc->sets.p, 0, (size_t)job->out_words * 4, stream));
    ev.mark(2, stream);
    if (launch_regex_local_sets(reinterpret_cast<const KRegexSetTask*>(p + tasks_at), (int32_t)job->tasks.size(),
                                job->max_card, sc->bitmap.as<uint64_t>(), sc->sets.as<uint32_t>(), stream))
      return fail(PGPU_ERR_DEVICE, "regex local sets launch failed: %s", hipGetErrorString(hipGetLastError()));
    ev.mark(3, stream);
    HIP_TRY(hipMemcpyAsync(out.data(), sc->sets.p, (size_t)job->out_words * 4, hipMemcpyDeviceToHost, stream));
  }
  if (global_out && job->n > 0)
    HIP_TRY(hipMemcpyAsync(global_out, sc->bitmap.p, (size_t)((job->n + 63) / 64) * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  job->sets.assign(job->tasks.size(), {});
  for (size_t i = 0; i < job->tasks.size(); ++i) {
    const size_t nw = ((size_t)job->tasks[i].card + 31) / 32;
    job->sets[i].assign(out.begin() + job->tasks[i].dst, out.begin() + job->tasks[i].dst + nw);
  }
  if (timed)
    fprintf(stderr, "[pgpu] regex column %s values %lld dict_bytes %lld states %d classes %d table_bytes %lld segments "
            "%zu: match_us %.1f local_sets_us %.1f run_us %.1f\n", job->name.c_str(), (long long)job->n,
            (long long)job->dict_bytes, d.num_states, d.num_classes, (long long)d.table_bytes(), job->tasks.size(),
            ev.us(0), local ? ev.us(2) : 0.0, now_us() - t_begin);
  return 0;
}
}  // namespace

int regex_global_ids(pgpu_table_s* t, int col, const char* pattern, uint64_t* bitmap, int64_t words) {
  RegexJob job;
  TRY(regex_compile_pattern(pattern, &job.dfa));
  TRY(regex_check_column(t, {}, col));
  {
    std::lock_guard<std::mutex> lk(t->mu);
    TRY(regex_job_snapshot(t, {}, col, &job));
  }
  const int64_t need = (job.n + 63) / 64;
  if (words < need)
    return fail(PGPU_ERR_INVALID_ARGUMENT, "bitmap of %lld words, the dictionary needs %lld", (long long)words, (long long)need);
  TRY(regex_job_run(t, &job, bitmap));
  for (int64_t w = need; w < words; ++w) bitmap[w] = 0;
  return 0;
}

}  // namespace pgpu
