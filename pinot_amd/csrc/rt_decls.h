// rt_decls.h -- prototypes of the functions and variables the runtime's sources share (see rt.h).
#pragma once
#include "regex_dfa.h"
#include "rt.h"

namespace pgpu {

// rt_core.cpp
void crash_trace_handler(int sig, siginfo_t* si, void* uc);
bool diag(const char* word);
void install_crash_trace();
extern thread_local std::string g_err;
bool trace_on();
double now_us();
int fail(int code, const char* fmt, ...);

// rt_dict.cpp
int parse_dictionary(int type, const pgpu_column_buffers& cb, Dict* d);
bool dbl_less(double a, double b);
bool merge_dict(std::shared_ptr<const Dict>& g, const Dict& src);
int64_t global_index_of(const Dict& g, const Dict& local, size_t i);
int ensure_lut(pgpu_table_s* t, Segment& s, int col, hipStream_t stream);
int ensure_values(pgpu_table_s* t, Segment& s, int col, hipStream_t stream);
int ensure_global_values(pgpu_table_s* t, int col, hipStream_t stream);
int ensure_value_map(pgpu_table_s* t, Segment& s, int col);
int ensure_docid(pgpu_table_s* t, int64_t n, hipStream_t stream);
int check_expr_segment(const pgpu_table_s* t, const Segment& s, const ExprProg& prog, bool long_result, const char* what);
int ensure_derived(pgpu_table_s* t, Segment& s, int col, hipStream_t stream);
int segment_column(pgpu_table_s* t, Segment& s, int col, const Column** out);
int table_reader_dict(pgpu_table_s* t, int col);
void account_unpin(pgpu_table_s* t, const Segment* s);
int64_t padded_fwd_words(int64_t num_docs, int bits);
int64_t lz4_decode_block(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap);
int decode_raw_forward_index(int type, const uint8_t* b, int64_t n, int32_t num_docs, int c, RawValues* out);
int parse_raw_column(int type, const pgpu_column_buffers& cb, int32_t num_docs, int c, Column* col, RawValues* out);
int64_t register_segment(pgpu_table_s* t, std::unique_ptr<Segment> seg_in);

// rt_sketch.cpp (byte-code sketches of filter columns, col_sketch.h): what the two steps of a segment's build share --
// the qualifying columns, where each one's histogram starts in the count buffers, and the cover rule as read at the start.
struct SketchBuild {
  std::vector<int> cols;
  std::vector<int64_t> off;
  DevBuf d_counts;
  std::vector<uint32_t> h_counts;
  double min_cover = 0;
  SketchBuild() = default;
  SketchBuild(const SketchBuild&) = delete;
  SketchBuild& operator=(const SketchBuild&) = delete;
  ~SketchBuild() { d_counts.release(); }
};
int sketch_begin(pgpu_table_s* t, Segment* seg, hipStream_t st, SketchBuild* b);
int sketch_finish(pgpu_table_s* t, Segment* seg, hipStream_t st, SketchBuild* b);

// rt_regex.cpp (PGPU_PRED_REGEXP_LIKE)
// pgpu_regex_check / pgpu_regex_match_host: the pattern compiled, and the host interpreter of its table.
int regex_check(const char* pattern, int32_t* states, int32_t* classes, int64_t* table_bytes);
int regex_match_host(const char* pattern, const uint8_t* value, int64_t len, int32_t* matched);
// The predicate's column must be a real STRING dictionary column, in every one of `segs`.
int regex_check_column(const pgpu_table_s* t, const std::vector<Segment*>& segs, int col);
// The pattern compiled, or the decline (PGPU_ERR_UNSUPPORTED, the message names REGEXP_LIKE and what was met).
int regex_compile_pattern(const char* pattern, RegexDfa* d);
// One REGEXP_LIKE leaf of a plan being made: its DFA (compiled once, when the query's columns are bound), what
// regex_job_snapshot takes under the table mutex -- the column's dictionary on the device and the planned segments' LUTs,
// of one snapshot, kept alive by the job -- and what regex_job_run computes from them outside it.
struct RegexJob {
  RegexDfa dfa;
  int col = -1;
  std::string name;
  std::shared_ptr<DevMem> blob, offsets;
  int64_t n = 0, dict_bytes = 0;
  std::vector<KRegexSetTask> tasks;  // one per segment
  std::vector<std::shared_ptr<DevMem>> luts;
  int64_t out_words = 0;
  int32_t max_card = 0, affine = 0;  // affine: the tasks that go through lut_off
  std::vector<std::vector<uint32_t>> sets;  // per segment: the bitset over its local dictIds that match (a LEAF_SET's words)
};
int regex_job_snapshot(pgpu_table_s* t, const std::vector<Segment*>& segs, int col, RegexJob* job);
// Both kernels on the calling thread's stream, in a pooled scratch's device memory, and one synchronisation; global_out
// (may be null): ceil(n / 64) words, the matching global dictIds.
int regex_job_run(pgpu_table_s* t, RegexJob* job, uint64_t* global_out);
// The global dictIds of column col that match, computed on the device, as a bitmap (takes the table mutex itself).
int regex_global_ids(pgpu_table_s* t, int col, const char* pattern, uint64_t* bitmap, int64_t words);

// rt_plan.cpp
int64_t hash_capacity(int64_t groups);
Scratch* acquire_scratch(pgpu_table_s* t);
void release_scratch(pgpu_table_s* t, Scratch* s);
bool parse_literal(int type, const char* lit, bool allow_star, Literal* out);
int insertion_index(const Column& c, const Literal& v);
int parse_predicate(int type, const pgpu_predicate& p, ParsedPred* out);
void to_inverted_leaf(const Column& c, const pgpu_predicate& p, const Segment& s, LeafHost* L);
int translate_predicate(const Column& c, const pgpu_predicate& p, const ParsedPred& pp, LeafHost* L,
                        std::vector<int>& ids);
int translate_predicate_dict(const Column& c, const pgpu_predicate& p, const ParsedPred& pp, LeafHost* L,
                             std::vector<int>& ids);
void translate_raw_predicate(int type, const pgpu_predicate& p, const ParsedPred& pp, LeafHost* L);
double estimate_selectivity(const std::vector<int32_t>& ops, const std::vector<double>& leaf);
Tri fold_program(const std::vector<int32_t>& ops, const std::vector<Tri>& leaf);
bool star_composites(const std::vector<int32_t>& ops, const pgpu_query* q, std::vector<std::vector<int>>* out);
void leaf_bitset(const LeafHost& L, int32_t card, std::vector<uint32_t>& w);
int plan_star_segment(pgpu_plan_s* P, size_t seg_index, Segment* s, const pgpu_query* q,
                      const std::vector<std::vector<int>>& comps, const std::vector<LeafHost>& leaves, bool* used);
SegStats classify_segment_stats(const pgpu_plan_s* P, uint64_t sig);
bool column_int_ends(const Column& c, int64_t* lo, int64_t* hi);
// The integer values of a table column over a segment list lie in [lo, hi] (lo > hi: there are none); `known` is
// false when a segment has a non-empty dictionary without integer values.
struct IntRange {
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  bool known = true;
};
IntRange int_column_range(const std::vector<Segment*>& segs, int col);
bool int_sum_fits(const std::vector<Segment*>& segs, int col);
long double int_sum_bound(const std::vector<Segment*>& segs, int col);
FxRange fx_operand_range(pgpu_table_s* t, const std::vector<Segment*>& segs, const pgpu_query* q, int tcol, int64_t* docs);
int query_fp_sum_ranges(pgpu_table_s* t, const std::vector<Segment*>& segs, const pgpu_query* q, FxAgree* out);
int32_t pack_slot_for(const pgpu_table_s* t, const pgpu_plan_s* P, const pgpu_query* q, int64_t max_count,
                      int shift);
int32_t lds_pack_slot(const pgpu_table_s* t, const pgpu_plan_s* P, const pgpu_query* q, int64_t G);
int32_t hash_pack_slot(const pgpu_table_s* t, const pgpu_plan_s* P, const pgpu_query* q, int* shift);
bool part_hash_eligible(const pgpu_plan_s* P, int64_t G);
bool dense_part_eligible(const pgpu_plan_s* P, int nslots, int64_t G);
bool part_eligible(const pgpu_plan_s* P, int nslots, int64_t G);
void hash_part_bits(const pgpu_config& cfg, int64_t groups, int nslots, int* pbits, int* sbits);
int part_coarse_shift(int num_parts);
int part_coarse_runs(int num_parts);
bool part_pass_shape(pgpu_plan_s* P, int64_t parts, int64_t tiles);
void hash_part_resize(pgpu_plan_s* P, int64_t groups);
int64_t part_hash_out_cap(const pgpu_plan_s* P);
int part_hash_overflow(const pgpu_plan_s* P, uint64_t groups);

// rt_plan_create.cpp
int plan_create_impl(pgpu_table_s* t, const int64_t* handles, int32_t nsegs, const pgpu_query* q, pgpu_plan_s* P,
                     const StreamExec* se = nullptr);

// rt_exec.cpp
int timeout_fail(const pgpu_plan_s* P);
int abandon_scratch(Scratch* sc, hipStream_t stream);
bool cancelled(const pgpu_plan_s* P);
int wait_plan(pgpu_plan_s* P, hipStream_t stream);
int launch_raw_leaves(const pgpu_plan_s* P, Scratch* sc, hipStream_t stream);
int launch_expr_leaves(const pgpu_plan_s* P, Scratch* sc, hipStream_t stream);
int exec_prologue(pgpu_plan_s* P, hipStream_t stream, void* d_table, int max_chunks, ExecCtx& X);
int exec_upload_chunk(pgpu_plan_s* P, hipStream_t stream, const ExecCtx& X, const LaunchChunk& C);
bool check_launch_on();
bool set_slot_weights(KParams& kp, int grid, int num_cus, double step, int64_t max_run);
void inflight_end(pgpu_plan_s* P);
int exec_launch_chunk(pgpu_plan_s* P, hipStream_t stream, ExecCtx& X, const LaunchChunk& C, int c);
int exec_epilogue(pgpu_plan_s* P, hipStream_t stream, ExecCtx& X);
int plan_execute_impl(pgpu_plan_s* P, hipStream_t stream, void* d_table);

// rt_finalize.cpp (result_expand and result_resolve_fx: host_result.h)
int plan_finalize_impl(pgpu_plan_s* P, hipStream_t stream, const void* d_table, int64_t key_begin, int64_t key_count,
                       pgpu_result_s* R);

// rt_groups.cpp
// agreed: the ranges of pgpu_plan_create_agreed (one per aggregation), handed to the parts; null for a plain plan
int split_for_groups_limit(pgpu_table_s* t, const int64_t* handles, int32_t nsegs, const pgpu_query* q,
                           pgpu_plan_s* P, bool* composite, const FxAgree* agreed = nullptr);
int composite_finalize(pgpu_plan_s* P, hipStream_t stream, pgpu_result_s* R);
bool plan_cache_enabled(const pgpu_table_s* t, const pgpu_query* q);
std::string plan_cache_key(pgpu_table_s* t, const int64_t* handles, int32_t nsegs, const pgpu_query* q);
bool plan_cache_get(pgpu_table_s* t, const std::string& key, pgpu_plan_s* P);
void plan_cache_clear(pgpu_table_s* t);
void plan_cache_put(pgpu_table_s* t, const std::string& key, pgpu_plan_s& P);

}  // namespace pgpu

