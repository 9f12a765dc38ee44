/*
 * pinotgpu.h — C ABI of libpinotgpu.so, the MI355X (gfx950) executor for Apache Pinot's server-side
 * filter -> group-by -> aggregation path over dictionary-encoded immutable segments.
 *
 * Plain C: pointers, sizes and status codes; no C++ or torch types cross this boundary and no C++ exception
 * escapes it.  Every call returns PGPU_OK (0) or a negative status; the message of the last failure on the
 * calling thread is available from pgpu_last_error().
 *
 * Each entry point names the reference interface it stands in for.  Citations use SURVEY.md's abbreviations:
 *   core/     = pinot-core/src/main/java/org/apache/pinot/core/
 *   seglocal/ = pinot-segment-local/src/main/java/org/apache/pinot/segment/local/
 *   segspi/   = pinot-segment-spi/src/main/java/org/apache/pinot/segment/spi/
 * The Java-side bindings a maintainer adds (JNI, and the ctypes binding used by this repo's tests) are in
 * INTEGRATION.md.
 *
 * Threading: every entry point is thread-safe, and any number of queries may run concurrently on one table
 * (Pinot runs many queries at once over the same segments, BaseCombineOperator.java:85-115).  Each plan owns a
 * per-query device arena (scratch buffers, statistics, group table) taken from the table's pool; plan creation holds
 * the table's mutex only to take its segment references and build lazily made per-segment arrays, so concurrent
 * cache-miss plans translate their predicates in parallel.  Give concurrent queries their own streams for their
 * device work to overlap (stream NULL = the table's stream: correct, but those queries' kernels run one after
 * another).  Pinned segments are immutable and reference-counted like Pinot's SegmentDataManager: unpinning a
 * segment that a live plan references frees its device memory when that plan is destroyed.  Global dictionaries
 * are snapshots: a pin that grows one never changes the ids of plans and results made before it.  Attach inverted
 * indexes and star-trees at segment load, before queries reference the segment.
 */
#ifndef PINOTGPU_H
#define PINOTGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGPU_ABI_VERSION 3  /* 2: pgpu_query.end_time_ms, PGPU_ERR_TIMEOUT; 3: pgpu_comm, pgpu_plan_combine */

/* ---- status codes (BaseCombineOperator.java:101-107 maps failures to ProcessingException; the Java shim maps
 * these codes the same way and keeps Pinot's CPU operator for PGPU_ERR_UNSUPPORTED). */
#define PGPU_OK 0
#define PGPU_ERR_INVALID_ARGUMENT (-1)
#define PGPU_ERR_BAD_QUERY (-2)      /* literal does not convert to the column type: BadQueryRequestException
                                        (core/operator/filter/predicate/PredicateEvaluatorProvider.java:85-88) */
#define PGPU_ERR_UNSUPPORTED (-3)    /* query shape outside the GPU path (caller runs Pinot's own operator) */
#define PGPU_ERR_DEVICE (-4)         /* HIP runtime / kernel failure */
#define PGPU_ERR_OUT_OF_MEMORY (-5)
#define PGPU_ERR_NOT_FOUND (-6)      /* unknown segment handle / column */
#define PGPU_ERR_TIMEOUT (-7)        /* the query's end time passed before its device work completed: the combine's
                                        timeout (BaseCombineOperator.java:193-203 EXECUTION_TIMEOUT_ERROR for
                                        aggregation-only, GroupByCombineOperator.java:193-203 QUERY_EXECUTION_ERROR
                                        wrapping a TimeoutException for group-by); no partial result is returned */
#define PGPU_ERR_CANCELLED (-8)      /* pgpu_plan_cancel: the caller abandoned the query (BaseOperator.nextBlock's
                                        EarlyTerminationException after Future.cancel(true), BaseOperator.java:37-39,
                                        BaseCombineOperator.java:124-130); no partial result is returned */

/* FieldSpec.DataType subset of dictionary-encoded single-value columns. */
enum pgpu_data_type { PGPU_INT = 0, PGPU_LONG = 1, PGPU_FLOAT = 2, PGPU_DOUBLE = 3, PGPU_STRING = 4 };

/* Forward-index formats:
 *   PGPU_FWD_FIXED_BIT    FixedBitSVForwardIndexReaderV2 bytes (seglocal/segment/index/readers/forward/
 *                         FixedBitSVForwardIndexReaderV2.java:33-96: MSB-first big-endian bit packing, PinotDataBitSet);
 *   PGPU_FWD_SORTED_PAIRS SortedIndexReaderImpl (seglocal/segment/index/readers/sorted/SortedIndexReaderImpl.java:
 *                         37-116: BIG_ENDIAN (startDocId, endDocId) int pairs per dictId);
 *   PGPU_FWD_RAW_FIXED    a raw (no-dictionary) INT / LONG / FLOAT / DOUBLE column as FixedByteChunkSVForwardIndexWriter
 *                         writes it, versions 2 / 3, chunks PASS_THROUGH, LZ4 or LZ4_LENGTH_PREFIXED
 *                         (BaseChunkSVForwardIndexWriter.java:130-193; BaseChunkSVForwardIndexReader.java:56-154) --
 *                         cardinality 0, no dictionary; decoded once at pin into per-doc values: an aggregation
 *                         operand (SUM / MIN / MAX / AVG) and a raw-value predicate column (EQ / NOT_EQ / IN / NOT_IN /
 *                         RANGE, RangePredicateEvaluatorFactory.java:60-102,268-448).  SNAPPY / ZSTANDARD chunks:
 *                         PGPU_ERR_UNSUPPORTED. */
enum pgpu_fwd_format { PGPU_FWD_FIXED_BIT = 0, PGPU_FWD_SORTED_PAIRS = 1, PGPU_FWD_RAW_FIXED = 2 };

int pgpu_abi_version(void);
/* Process start-up / shut-down of the executor (the server's lifecycle around PlanMaker, ServerInstance.java:86-90):
 * pgpu_init brings up the HIP runtime on devices 0..n_gpus-1 (n_gpus <= 0: every visible device) so the first query
 * pays no context creation, and returns the number of devices initialised (or a negative status); pgpu_shutdown
 * waits for every initialised device's queued work.  Tables, plans and results own their memory and are released by
 * their destroy calls (segments on unpin / table destroy, as ImmutableSegmentImpl.destroy frees them). */
int pgpu_init(int n_gpus);
int pgpu_shutdown(void);
/* Copies the calling thread's last error message (NUL-terminated, truncated to len). Returns its full length. */
int pgpu_last_error(char* buf, size_t len);
int pgpu_device_count(int* count);

/* ============================================================================ tables and pinned segments */

typedef struct pgpu_table_s* pgpu_table;

/* A table owns the per-column global dictionaries: the key space shared by all of its segments, replacing the
 * by-value merge of GroupByCombineOperator (core/operator/combine/GroupByCombineOperator.java:132-151). */
int pgpu_table_create(int device, int num_columns, const char* const* column_names, const int32_t* data_types,
                      pgpu_table* out);
int pgpu_table_destroy(pgpu_table table);

/* Executor settings of a table: what a Pinot server's configuration sets.  The JNI shim maps its
 * pinot.server.query.executor.gpu.* keys (PinotConfiguration, as InstancePlanMakerImplV2 reads its
 * max.execution.threads / num.groups.limit / min.segment.group.trim.size keys, InstancePlanMakerImplV2.java:75-110)
 * onto these fields; INTEGRATION.md lists the mapping.  pgpu_config_default fills every field with the library's
 * default, which a new table starts with.  Settings apply to plans made after pgpu_table_set_config (the table's
 * compiled-plan cache is cleared); a plan already made keeps the settings it was planned with. */
typedef struct {
  int32_t struct_size;            /* sizeof(pgpu_config) as the caller compiled it: later fields keep their defaults */
  int32_t plan_cache;             /* 1 (default): a repeated query (same bytes, same segments) reuses its compiled
                                     plan; 0: every query is planned afresh (pgpu_query.options can opt out per query) */
  int32_t partitioned_group_by;   /* 1 (default): dense key spaces whose table is >= 32 MB are radix-partitioned and
                                     aggregated per partition in LDS (K8a-K8d); 0: global atomics into the table */
  int32_t hash_partitions;        /* 1 (default): key spaces past every dense table and below 2^31 are aggregated by
                                     hashed partitions (K8h, LDS hash tables); 0: the global hash table */
  int32_t hash_partition_bits;    /* most partition bits of hashed partitions, 0..14 (default 14) */
  int32_t hash_partition_lds_kb;  /* LDS of one hashed partition's table, KB, 1..128 (default 0: 20 KB-class tables) */
  int32_t lds_table_kb;           /* largest group table privatised in LDS per workgroup, KB (default 112) */
  int32_t plan_chunk_segments;    /* segments per host planning task (default 4096) */
  int32_t stream_chunks;          /* scan launches of pgpu_plan_create_execute's streamed plan (default 1) */
  int32_t compact_results;        /* 1 (default): large results cross PCIe in the compact form (presence bitmap /
                                     keys + narrowed slot words) and are decoded on first access; 0: columnar */
  int32_t star_tree_workgroups;   /* workgroups of the star-tree document scan (default 0: the library's choice) */
  double dense_selectivity;       /* estimated selectivity from which plans take the dense scan instance
                                     (default 0.25; > 1 = never) */
  double slot_weight_step;        /* chunked scans launched with no other query's scan in flight: the workgroup
                                     dispatched to CU slot s of S takes a share of tiles weighted 1 + step (S-1-s)
                                     (the SIMDs issue the oldest wave first; default 0.11; 0 = equal shares) */
} pgpu_config;
int pgpu_config_default(pgpu_config* out);
int pgpu_table_set_config(pgpu_table table, const pgpu_config* config);
int pgpu_table_get_config(pgpu_table table, pgpu_config* out);

/* One column of an ImmutableSegment as Pinot holds it in memory (PinotDataBuffer views; the JNI shim takes the
 * addresses from PinotDataBuffer.toDirectByteBuffer, segspi/memory/PinotDataBuffer.java:382). */
typedef struct {
  int32_t cardinality;        /* Dictionary.length() (segspi/index/reader/Dictionary.java:49) */
  int32_t bits_per_element;   /* column.X.bitsPerElement = PinotDataBitSet.getNumBitsPerValue(card - 1) */
  int32_t entry_width;        /* bytes per dictionary entry (numBytesPerValue) */
  int32_t padding_byte;       /* string dictionaries: segment.padding.character (0 for current segments) */
  int32_t fwd_format;         /* enum pgpu_fwd_format */
  int32_t reserved;
  const uint8_t* dict;        /* BIG_ENDIAN fixed-width sorted values (BaseImmutableDictionary.java:45-60) */
  int64_t dict_len;
  const uint8_t* fwd;         /* forward index bytes */
  int64_t fwd_len;
} pgpu_column_buffers;

typedef struct {
  int32_t num_docs;
  int32_t num_columns;        /* must equal the table's column count; entries follow the table's column order */
  const pgpu_column_buffers* columns;
} pgpu_segment_desc;

/* Pins one ImmutableSegment into HBM (the H2D copy happens here, once; ImmutableSegmentLoader.load,
 * seglocal/indexsegment/immutable/ImmutableSegmentLoader.java:67-201, is where the shim calls it). */
int pgpu_pin_segment(pgpu_table table, const pgpu_segment_desc* desc, int64_t* segment_handle);
/* Frees the device copy (ImmutableSegmentImpl.destroy, seglocal/indexsegment/immutable/ImmutableSegmentImpl.java:147). */
int pgpu_unpin_segment(pgpu_table table, int64_t segment_handle);
int pgpu_table_num_segments(pgpu_table table, int32_t* count);
int64_t pgpu_table_device_bytes(pgpu_table table);

/* Adds values to a column's global dictionary (multi-GPU: every rank merges the union of all ranks' values so
 * per-GPU group tables share one key space before the RCCL reduce).  Numeric columns read `values_i64` (INT/LONG)
 * or `values_f64` (FLOAT/DOUBLE); STRING columns read blob + offsets[n+1]. */
int pgpu_table_add_dictionary_values(pgpu_table table, int column, int64_t n, const int64_t* values_i64,
                                     const double* values_f64, const uint8_t* blob, const int64_t* offsets);
/* Global dictionary of a column (sorted, ascending); gid = index. */
int pgpu_table_dictionary_size(pgpu_table table, int column, int64_t* size);
int pgpu_table_dictionary_i64(pgpu_table table, int column, int64_t* out);       /* INT / LONG */
int pgpu_table_dictionary_f64(pgpu_table table, int column, double* out);        /* FLOAT / DOUBLE */
/* STRING: writes all values as blob + offsets (offsets has size+1 entries); blob_cap in bytes. */
int pgpu_table_dictionary_str(pgpu_table table, int column, uint8_t* blob, int64_t blob_cap, int64_t* offsets);

/* ============================================================================ single-segment readers */

/* ForwardIndexReader.readDictIds (segspi/index/reader/ForwardIndexReader.java:83; implemented by
 * FixedBitSVForwardIndexReaderV2.readDictIds :62-96): host docIds in, host dictIds out, decoded on the GPU
 * from the pinned copy by the unpack kernel (K1). */
int pgpu_read_dict_ids(pgpu_table table, int64_t segment_handle, int column, const int32_t* doc_ids, int32_t n,
                       int32_t* dict_ids_out);

/* Device-level K1: unpack n values starting at `start` from a packed MSB-first buffer already in device memory
 * into int32 (all pointers are device pointers; stream may be NULL). */
int pgpu_unpack_fixed_bit_device(const void* d_fwd, int64_t fwd_len, int32_t bits, int64_t start, int64_t n,
                                 int32_t* d_out, void* stream);

/* ============================================================================ queries */

/* Predicate types (segspi Predicate.Type subset on dictionary columns). RANGE literal pair uses "*" for
 * unbounded (RangePredicate.UNBOUNDED). Literals are strings, converted per column type exactly as
 * PredicateUtils.getStoredValue + Dictionary.insertionIndexOf do.
 * A predicate on an arithmetic expression -- WHERE price * qty > 1000, the reference's ExpressionFilterOperator
 * (FilterPlanNode.java:179-186) -- names the expression's virtual column (pgpu_table_add_expression) in `column`.  The
 * expression's value is a DOUBLE without a dictionary, so its evaluator is the raw DOUBLE one: the literals are read by
 * Double.parseDouble; RANGE and EQ / NOT_EQ compare as Java doubles (0.0 equals -0.0, a NaN value matches no RANGE and
 * no EQ, hence every NOT_EQ), IN / NOT_IN by Double.doubleToLongBits (0.0 and -0.0 differ).  One kernel in front of the
 * scan evaluates the leaf for every doc of every planned segment into a per-query docId bitmap, which the scan reads
 * as it reads an inverted-index leaf's; the leaf is never folded to match-all or empty, a filter with such a leaf never
 * takes a star-tree, and the leaf runs wherever a raw-value leaf does (every accumulator mode, the partitioned
 * pipelines, pgpu_filter_bitmap; one launch, never streamed).  Its operands are filter columns: they do not count in
 * numEntriesScannedPostFilter.  numEntriesScannedInFilter counts it as ExpressionScanDocIdIterator does
 * (PGPU_LEAF_EXPRESSION below).  Declined as for expression aggregations (STRING, raw or virtual operands:
 * PGPU_ERR_UNSUPPORTED, the message names "expression").
 *
 * PGPU_PRED_REGEXP_LIKE: REGEXP_LIKE(col, 'p'), and col LIKE 'p' after the reference's conversion of the LIKE pattern
 * (RegexpPatternConverterUtils.likeToRegexpLike; RequestContextUtils.java:230-236, 326-331).  num_values is 1 and
 * values[0] the Java pattern text; the column is a STRING dictionary column of the table's own.  The reference
 * evaluates Pattern.compile(p, CASE_INSENSITIVE | UNICODE_CASE).matcher(value).find() per scanned doc
 * (RegexpLikePredicateEvaluatorFactory.java:64-80).  Here the pattern is compiled once into a DFA, the DFA runs once
 * over the column's table-global dictionary on the GPU when the plan is made, and every planned segment's leaf is the
 * set of its matching dictIds, read by the scan as an IN's is.  As in the reference without an FST index the leaf is
 * always a scan leaf -- on a sorted column and on one with an inverted index too --, is never folded to match-all or
 * empty (a pattern that matches nothing is still scanned and counted in numEntriesScannedInFilter), has the scan
 * priority in an AND, and a filter that holds one never takes a star-tree.  The pattern is part of the query and so of
 * the plan-cache key.
 * The answer is the reference's or a decline, so only a subset of java.util.regex whose meaning is unambiguous is
 * accepted: ASCII patterns of literals (letters match case-insensitively), '.', '^' and '$' anywhere, groups ( ) and
 * (?: ), alternation (empty alternatives too), the greedy quantifiers * + ? {n} {n,} {n,m} with bounds <= 64, classes
 * [..] and [^..] of single characters, backslash-escaped non-alphanumerics, \d \w \s \D \W \S, ranges whose ends are
 * both digits, both lower-case or both upper-case letters, '-' first, last or escaped and '^' not first (a class
 * matches case-insensitively, a negated class excludes both cases), and outside a class the escapes backslash +
 * non-alphanumeric (that literal), \t, \d \D \w \W \s \S (Java's default ASCII meanings).  The empty pattern matches
 * every value.
 * Declined with PGPU_ERR_UNSUPPORTED (the message names REGEXP_LIKE and what was met): any other backslash + letter or
 * digit (back-references, \b \B \A \z \Z \G \Q \E \p \P \x \u \0 \c \h \v \R \k, \n \r \f \a \e; inside a class \t
 * too); a '(?' other than '(?:'; lazy and possessive quantifiers; a quantifier with nothing to repeat, after another
 * quantifier, or applied to '^' / '$'; {,n}; {n,m} with n > m or a bound above 64; a '{' that does not open a
 * well-formed quantifier; an unescaped ']' or '}' outside its construct; inside a class '[', '&&', a leading ']', any
 * other range and any other '-'; a non-ASCII byte; a trailing backslash; unbalanced parentheses or brackets; groups
 * nested deeper than 200; a pattern longer than 1024 bytes; repeats that unroll into more than 32768 NFA states; a DFA
 * whose transition table (states x byte classes x 2 bytes) is above PGPU_REGEX_MAX_TABLE_BYTES, the table the kernel
 * keeps in LDS.  Declined likewise: a column that is not STRING, a virtual or derived column, a raw column, a
 * dictionary of 2^31 bytes, and a column whose global dictionary snapshot holds a value with a byte >= 0x80, a \n or a
 * \r (within that limit UNICODE_CASE is ASCII folding, '.' matches every byte and '$' means the end of input). */
enum pgpu_predicate_type { PGPU_PRED_EQ = 0, PGPU_PRED_NOT_EQ = 1, PGPU_PRED_IN = 2, PGPU_PRED_NOT_IN = 3,
                           PGPU_PRED_RANGE = 4, PGPU_PRED_REGEXP_LIKE = 5 };
#define PGPU_REGEX_MAX_TABLE_BYTES 32768
typedef struct {
  int32_t type;
  int32_t column;             /* a table column, or a virtual column (an expression: see above) */
  int32_t num_values;         /* EQ/NOT_EQ 1, IN/NOT_IN k, RANGE 2 (lower, upper), REGEXP_LIKE 1 (the pattern) */
  int32_t lower_inclusive;
  const char* const* values;
  int32_t upper_inclusive;
  int32_t reserved;
} pgpu_predicate;

/* Filter tree (FilterContext AND / OR / PREDICATE, plus NOT) as a postfix program. */
enum pgpu_filter_opcode { PGPU_OP_PRED = 0, PGPU_OP_AND = 1, PGPU_OP_OR = 2, PGPU_OP_NOT = 3 };
typedef struct {
  int32_t op;   /* PRED: arg = predicate index; AND / OR: arg = number of operands popped; NOT: unused */
  int32_t arg;
} pgpu_filter_op;

/* AggregationFunctionType subset (core/query/aggregation/function/{Count,Sum,Min,Max,Avg,DistinctCount}
 * AggregationFunction).
 * PGPU_AGG_DISTINCTCOUNT(col): per group, the number of distinct values of a dictionary-encoded single-value column of
 * any type (INT / LONG / FLOAT / DOUBLE / STRING) among the matched docs -- DistinctCountAggregationFunction.java:
 * 131-143 collects the docs' dictIds in a RoaringBitmap per group and counts the values they stand for.  Here the
 * per-group set is a bitmap over the column's table-global dictIds (the same ids on every segment, so segments merge
 * by OR in any order); the result is an exact integer: pgpu_result_values_i64 and pgpu_result_words_view (form 0)
 * return it, pgpu_result_values as a double; ORDER BY and the trims compare it like a COUNT; no match gives 0.
 * The column counts as projected (numEntriesScannedPostFilter); a segment carrying a star-tree is scanned
 * (StarTreeUtils finds no function-column pair for it); an aggregation-only query whose functions are all MIN / MAX /
 * DISTINCTCOUNT over match-all segments reports numEntriesScannedPostFilter 0 (AggregationPlanNode.java:233-246).
 * Supported: dense key spaces (the LDS and global group tables, aggregation-only queries included); planned as with
 * pgpu_config.partitioned_group_by = 0, hash_partitions = 0 and stream_chunks = 1.
 * Declined with PGPU_ERR_UNSUPPORTED (the message names DISTINCTCOUNT): side bitmaps (keys x ceil(cardinality / 64)
 * x 8 bytes per distinct column) above 1 GiB in one plan; key spaces that take the hash table (past 2^26 keys, or
 * ARRAY_MAP stages); numGroupsLimit plans that split per segment; a raw (no-dictionary) column; more than 8 distinct
 * columns; the combination with PGPU_OPT_EXACT_FP_SUM; pgpu_result_datatable (Pinot ships the value set as an
 * OBJECT); and, because per-rank counts do not add, every cross-GPU or external-merge entry point but one:
 * pgpu_plan_exchange_*, pgpu_plan_finalize_range, an external d_table (execute, finalize, pgpu_plan_combine),
 * pgpu_result_exchange_rows / merge_rows / combine_rows, and a pgpu_plan_combine_mode whose ranks do not agree on a
 * dense mode (they would meet as rows).
 * Across GPUs: pgpu_plan_combine_mode / pgpu_plan_combine merge it in PGPU_COMBINE_ALL_REDUCE and
 * PGPU_COMBINE_REDUCE_SCATTER on the plan's own table (d_table NULL), as DistinctCountAggregationFunction.merge does
 * (the union of the sets) -- see pgpu_plan_combine.  The ranks union the dictionaries of the distinct columns, like
 * those of the group-by columns, first (pgpu_table_add_dictionary_values): bit i must mean one value everywhere. */
/* PGPU_AGG_PERCENTILE_OF(p_e4)(col): the exact percentile of a dictionary-encoded single-value numeric column per group
 * -- PercentileAggregationFunction.java:83-165 collects the matched values of a group, sorts them and returns the one
 * at index size - 1 for the 100th percentile, else (int)((double)size * percentile / 100.0), size being the group's
 * matched docs; the product and the quotient are IEEE doubles, each rounded on its own (10000 docs at 0.57 give index
 * 56).  The percentile travels inside pgpu_agg.fn: bits 0..7 hold the function code PGPU_AGG_PERCENTILE, bits 8..31
 * the percentile in ten-thousandths, 0 .. 1000000 (PERCENTILE95 = PGPU_AGG_PERCENTILE_OF(950000), PERCENTILE(x, 99.9)
 * = PGPU_AGG_PERCENTILE_OF(999000)); the double the arithmetic uses is p_e4 / 10000.0, which equals the double of the
 * decimal literal for every code.  Codes 0..5 have zero upper bits; PGPU_AGG_FN / PGPU_AGG_PERCENTILE_E4 take a
 * pgpu_agg.fn apart.  Being part of fn, the percentile is part of the plan-cache key.
 * Here the per-group sorted list is a histogram over the column's table-global dictIds (dictionary order is value
 * order), filled with one 32-bit add per matched doc; segments merge by addition in any order and the answer is exact.
 * The result is the selected value as a double ((double)value for INT / LONG): pgpu_result_values returns it; ORDER BY
 * and both trims compare it as a double, the PQL trim largest first (as MAX).  A group without a match is absent; an
 * aggregation-only query without a matched doc leaves the caller Pinot's default, -inf.  The column counts as
 * projected (numEntriesScannedPostFilter), also for an unfiltered aggregation-only query, which is scanned (no
 * dictionary-based answer: AggregationPlanNode's exemption is for MIN / MAX / DISTINCTCOUNT); a segment carrying a
 * star-tree is scanned.  All percentiles of one column share its histogram; in a plan with a PERCENTILE the columns of
 * DISTINCTCOUNT aggregations are counted from histograms too (the number of non-zero cells).
 * Supported: dense key spaces (the LDS and global group tables, aggregation-only queries included); planned as with
 * pgpu_config.partitioned_group_by = 0, hash_partitions = 0 and stream_chunks = 1.
 * Declined -- a code above 1000000 with PGPU_ERR_INVALID_ARGUMENT, the rest with PGPU_ERR_UNSUPPORTED (the message
 * names PERCENTILE): side histograms (keys x cardinality rounded up to 4 x 4 bytes per distinct column, those of
 * DISTINCTCOUNT columns included) above 1 GiB in one plan; plans whose segments hold 2^32 docs or more (a cell could
 * wrap); a STRING column; a raw (no-dictionary) column; key spaces that take the hash table (past 2^26 keys, or
 * ARRAY_MAP stages); numGroupsLimit plans that split per segment; more than 8 side columns (histograms) in one query;
 * the combination with PGPU_OPT_EXACT_FP_SUM; every cross-GPU or external-merge entry point (pgpu_plan_combine_mode,
 * pgpu_plan_combine, pgpu_plan_exchange_*, pgpu_plan_finalize_range, an external d_table, pgpu_result_exchange_rows /
 * merge_rows / combine_rows: per-rank percentiles do not merge) and pgpu_result_datatable (Pinot ships the value list
 * as an OBJECT). */
enum pgpu_agg_fn { PGPU_AGG_COUNT = 0, PGPU_AGG_SUM = 1, PGPU_AGG_MIN = 2, PGPU_AGG_MAX = 3, PGPU_AGG_AVG = 4,
                   PGPU_AGG_DISTINCTCOUNT = 5, PGPU_AGG_PERCENTILE = 6 };
#define PGPU_AGG_PERCENTILE_MAX_E4 1000000
#define PGPU_AGG_PERCENTILE_OF(p_e4) ((int32_t)(PGPU_AGG_PERCENTILE | ((int32_t)(p_e4) << 8)))
#define PGPU_AGG_FN(fn) ((int32_t)((fn) & 0xFF))                           /* the function code of a pgpu_agg.fn */
#define PGPU_AGG_PERCENTILE_E4(fn) ((int32_t)(((uint32_t)(fn)) >> 8))      /* its percentile in ten-thousandths */
typedef struct {
  int32_t fn;
  int32_t column;   /* -1 for COUNT(*); a virtual column (pgpu_table_add_expression) for an expression */
} pgpu_agg;

/* Arithmetic expressions inside aggregations (and in predicates: pgpu_predicate) -- SUM(price * qty), AVG(revenue - cost), MAX(a / b): the reference's
 * TransformOperator between projection and aggregation, for its four arithmetic transform functions
 * (core/operator/transform/function/{Addition,Subtraction,Multiplication,Division}TransformFunction.java).  An
 * expression is a virtual column of the table: pgpu_table_add_expression registers its postfix program and returns a
 * column index at or above the table's real columns, which a pgpu_agg.column may name from then on.  Registering an
 * identical program again returns the same index, so a query's bytes -- the plan-cache key -- stay the same.
 * Semantics, bit for bit per doc: every function yields a double.  A column operand is its getDoubleValuesSV value
 * ((double) of an INT, LONG or FLOAT value), a literal a double.  Every operation is one IEEE double operation rounded
 * on its own; nothing is fused into a multiply-add.  All ops are binary: the caller emits the reference's n-ary
 * ADD(x1..xn) as ((0.0 + literals in argument order) + v1) + v2 ... over the non-literal arguments in argument order
 * (the leading 0.0 + is part of the semantics: ADD(x, y) of two -0.0 is +0.0), MULT likewise from 1.0.  SUB(a, b) is
 * a - b, DIV(a, b) is a / b (x / 0 is +-inf).  A NaN result is treated as the NaN of a DOUBLE column is (one canonical
 * NaN key, above +inf, for MIN / MAX).
 * Aggregations: SUM and AVG of an expression add the doubles (float64 sums; AVG divides by the COUNT), MIN and MAX
 * compare them in double order (-0.0 below +0.0), COUNT(expr) is COUNT(*) -- pass column -1.  The virtual column is a
 * DOUBLE to everything downstream of the scan: finalize, ORDER BY and the trims, the cross-GPU combine (ranks must
 * have registered the same programs in the same order), the DataTable, which names the aggregation by the expression's
 * name, e.g. sum(mult(price,qty)).  numEntriesScannedPostFilter counts every distinct real column the query projects
 * once: the group-by columns and every column named by an aggregation or inside its expression.  A segment carrying a
 * star-tree is scanned for such a query.  The values are computed per matched doc inside the fused scan, by a
 * pair of instances of its own (pgpu_plan_scan_geometry word 15 = 12: sparse, in every accumulator mode -- LDS, global
 * and hash tables; 13: dense, the whole-group decode of plans of estimated selectivity >= dense_selectivity).
 * Limits (PGPU_ERR_INVALID_ARGUMENT otherwise): 1..PGPU_EXPR_MAX_OPS ops; an evaluation stack of at most
 * PGPU_EXPR_MAX_DEPTH values; at most PGPU_EXPR_MAX_COLUMNS distinct columns; a well-formed postfix program (no
 * underflow, an op code of the enum, column indexes of the table) that leaves exactly one value; at least one column
 * operand; at most PGPU_EXPR_MAX_PER_TABLE expressions per table.
 * Declined with PGPU_ERR_UNSUPPORTED (the message names "expression"): an operand that is a STRING column or itself a
 * virtual column (at registration); an operand that is a raw (no-dictionary) column in a planned segment (multi-value
 * columns cannot be pinned at all); DISTINCTCOUNT or PERCENTILE of an expression; an expression aggregation in one
 * query with a DISTINCTCOUNT or PERCENTILE (those plans take another scan instance); the combination with
 * PGPU_OPT_EXACT_FP_SUM (pgpu_query_fp_sum_ranges and pgpu_plan_create_agreed included); more than 8 distinct
 * expressions in one query; an external d_table (execute, finalize, pgpu_plan_combine); numGroupsLimit plans that
 * split per segment; a virtual column in GROUP BY (PGPU_ERR_INVALID_ARGUMENT: bad column).  None of this list but the
 * operand rules applies to a virtual column named by a predicate, which changes nothing after the filter.  Plans with
 * an expression aggregation never take the radix- or hash-partitioned pipelines: they are planned as with
 * pgpu_config.partitioned_group_by = 0, hash_partitions = 0 and stream_chunks = 1.
 *
 * Conditional expressions -- SUM(CASE WHEN country_id = 3 THEN revenue ELSE 0 END), WHERE CASE WHEN a > 1 THEN b ELSE c
 * END > 3: the reference's CaseTransformFunction, BinaryOperatorTransformFunction, And / OrOperatorTransformFunction and
 * LiteralTransformFunction.  A stack entry is a number or a boolean; the program is type-checked at registration
 * (PGPU_ERR_INVALID_ARGUMENT, "bad operand type"): arithmetic and comparisons take numbers, AND / OR booleans, SELECT
 * (number, number, boolean), and the program leaves one number.
 *   EQ NE GT GE LT LE  pop b, then a, push the boolean Double.compare(a, b) <op> 0: the total order of
 *                      Double.doubleToLongBits, in which -0.0 is below +0.0 and every NaN is one value that equals itself
 *                      and lies above +inf.  This is not the rule of a pgpu_predicate on a column, where 0.0 == -0.0.
 *   AND OR             pop two booleans, push one; the reference's n-ary form is a left-to-right chain.
 *   SELECT             pops cond (top), then `then`, then `else`; pushes cond ? then : else.  CASE WHEN c1 THEN r1 ..
 *                      WHEN cN THEN rN ELSE e END is e, rN, cN, SELECT, .., r1, c1, SELECT, so the first matching WHEN
 *                      wins (getSelectedArray) and the stack stays at 4 for any number of WHENs over simple operands.
 *                      Every branch is evaluated for every doc; x / 0 in an unselected branch is harmless.
 * A condition stands above the two numbers its SELECT reads, so two comparisons joined by AND / OR need a stack of 5
 * and are refused by the depth limit: lower them to SELECTs.  WHEN c1 OR c2 THEN r is WHEN c1 THEN r WHEN c2 THEN r;
 * WHEN c1 AND c2 THEN r ELSE e is WHEN !c1 THEN e WHEN !c2 THEN e ELSE r, where !(a > b) is a <= b in the total order.
 * The caller's duty for literals: the evaluator is all-double, so bit parity rests on each literal being the double the
 * reference reads.  The server sees Long.toString of an integer literal and Double.toString of a decimal one; its type
 * is NumberUtils.createNumber of that text (commons-lang3 3.5): an integer is INT if it fits int32, else LONG if it fits
 * int64; a decimal with at most 7 digits between the point and the E (or the end) whose float is finite and not
 * zero-from-nonzero is FLOAT (0.1, 0.0, 2.5 and 1.0E10 are), else with at most 16 digits DOUBLE; BigInteger /
 * BigDecimal texts, literals of more than 15 significant digits, true / false, timestamps and strings are to be
 * declined.  The type R of a CASE (calculateResultMetadata) folds ELSE, then the THENs in order: equal types keep, INT
 * and LONG give LONG, every other mix gives DOUBLE; an arithmetic node is DOUBLE, a nested CASE has its own R.  A THEN /
 * ELSE literal is (double) of the literal read as R: its integer under INT / LONG, (double)(float) of it under FLOAT
 * (all branches FLOAT: THEN 0.1 ELSE 0.0 adds 0.10000000149011612 per doc), its plain double under DOUBLE (THEN 0.1
 * ELSE d_col adds 0.1).  A comparison's literal is read as its own type: a FLOAT one is always (double)(float) of it
 * (d > 0.1 compares with 0.10000000149011612).  Every accepted type pair is Double.compare of the widened values
 * (integer pairs are Integer.compare / Long.compare: the same within +-2^53).
 * To be declined by the caller: a LONG side (column, LONG literal or LONG-typed CASE) compared with a FLOAT or DOUBLE
 * side (the reference applies its operator twice there, BinaryOperatorTransformFunction.java:313-325, which this
 * project does not reproduce); STRING operands; IN inside WHEN; a missing ELSE (the reference's NULL makes R a STRING); a
 * boolean used as a number (SUM(a > 5)); a literal-only condition.  Declined at plan time (PGPU_ERR_UNSUPPORTED, the
 * message names "expression"): a LONG column that reaches a comparison as it is -- pushed and compared, or passed on by
 * SELECTs only -- while one of its dictionary values in a planned segment lies outside +-2^53.
 *
 * Math and time functions -- SUM(price * floor(qty / 10)), GROUP BY dateTimeConvert(ts,'1:MILLISECONDS:EPOCH',
 * '1:HOURS:EPOCH','1:HOURS'), WHERE timeConvert(days,'DAYS','SECONDS') = x: the reference's
 * SingleParamMathTransformFunction, ModuloTransformFunction, TimeConversionTransformFunction and the epoch-to-epoch form
 * of DateTimeConversionTransformFunction.  Op code 15 is not an op.
 *   ABS CEIL FLOOR SQRT  number -> number, the depth stays: Java's Math.abs / ceil / floor / sqrt, bit for bit (all four
 *                      are correctly rounded).  abs(-0.0) is +0.0, ceil(-0.5) is -0.0, sqrt of a negative is NaN,
 *                      sqrt(-0.0) is -0.0.
 *   MOD                pop b, then a, push a % b of Java's doubles (C's fmod): exact, the dividend's sign; x % 0 and
 *                      inf % y are NaN, x % inf is x.
 *   LDIV               pop b, then a, push (double)((long)a / (long)b): Java's long division, truncated toward zero
 *                      (-1 / 86400000 is 0, and a zero quotient is +0.0).  The divisor is the LITERAL op right before
 *                      it, a positive integer of at most 2^53.  The dividend is integral: a COLUMN of type INT or LONG;
 *                      x, LITERAL n, MULT over an integral x and a positive integer n of at most 2^53 (the literal on
 *                      top: the long product -- LITERAL, x, MULT is arithmetic's double product and not integral); or
 *                      another LDIV.  PGPU_ERR_INVALID_ARGUMENT otherwise, as for a boolean operand of any of these ops.
 * EXP and LN are not ops: Java's Math.exp / Math.log are not correctly rounded, so their bits cannot be promised.
 * A time function is a chain of such MULTs and LDIVs over its column, in the reference's order of operations:
 * timeConvert(x, IN, OUT) is TimeUnit.convert -- x * (IN / OUT) where OUT is finer, x / (OUT / IN) where it is coarser,
 * x itself for equal units; OUT = WEEKS is toMillis then / 604800000 (CustomTimeUnitTransformer).
 * dateTimeConvert(x, 'n:IN:EPOCH', 'm:OUT:EPOCH', 'g:UNIT') is EpochToEpochTransformer: x * n, toMillis (a MULT; an LDIV
 * for MICROSECONDS and NANOSECONDS), / G then * G with G the granularity in milliseconds, fromMillis (an LDIV; a MULT for
 * MICROSECONDS and NANOSECONDS; WEEKS is / 604800000), / m.  Steps by 1 are left out and adjacent MULTs may be one; the
 * longest chain is 13 ops.  The result type of both is LONG, that of the math functions DOUBLE.
 * Declined at plan time (PGPU_ERR_UNSUPPORTED; the message names "expression", or "GROUP BY expression" for a derived
 * column): a chain -- any x, LITERAL n, MULT or LDIV run that starts at an INT or LONG column -- whose column, any
 * intermediate value or result leaves +-2^53 over the ends of that column's dictionary in a planned segment (all
 * constants are positive, so a chain is monotone; the check is exact integer arithmetic).  Past +-2^53 a double is no
 * longer the long, and further out Java's TimeUnit saturates.
 * The caller's duty: a time function's first argument is an INT or LONG column (the reference casts every other
 * argument to long, and there is no cast op); SIMPLE_DATE_FORMAT formats (their values are strings), MONTHS / YEARS as
 * an output unit (the joda chronology) and WEEKS / MONTHS / YEARS as an input unit are to be declined.  A predicate on
 * a LONG-typed expression (pgpu_predicate.column naming the virtual column of a time function) is the reference's raw
 * LONG evaluator: each literal is read by Long.parseLong -- a decimal (= 1.5) or a value past int64 is its
 * BadQueryRequestException and is to be declined -- and passed on as decimal text.  Within +-2^53, which the plan
 * guarantees, comparing the doubles is comparing the longs, and no -0.0 can arise. */
enum pgpu_expr_opcode { PGPU_EXPR_COLUMN = 0, PGPU_EXPR_LITERAL = 1, PGPU_EXPR_ADD = 2, PGPU_EXPR_SUB = 3,
                        PGPU_EXPR_MULT = 4, PGPU_EXPR_DIV = 5,
                        PGPU_EXPR_EQ = 6, PGPU_EXPR_NE = 7, PGPU_EXPR_GT = 8, PGPU_EXPR_GE = 9, PGPU_EXPR_LT = 10,
                        PGPU_EXPR_LE = 11, PGPU_EXPR_AND = 12, PGPU_EXPR_OR = 13, PGPU_EXPR_SELECT = 14,
                        /* (15 is not an op) */
                        PGPU_EXPR_ABS = 16, PGPU_EXPR_CEIL = 17, PGPU_EXPR_FLOOR = 18, PGPU_EXPR_SQRT = 19,
                        PGPU_EXPR_MOD = 20, PGPU_EXPR_LDIV = 21 };
#define PGPU_EXPR_MAX_OPS 16
#define PGPU_EXPR_MAX_DEPTH 4
#define PGPU_EXPR_MAX_COLUMNS 4
#define PGPU_EXPR_MAX_PER_TABLE 256
typedef struct {
  int32_t op;       /* pgpu_expr_opcode; ADD / SUB / MULT / DIV pop b then a and push a op b */
  int32_t column;   /* PGPU_EXPR_COLUMN: a real column of the table */
  double literal;   /* PGPU_EXPR_LITERAL */
} pgpu_expr_op;
/* Registers ops[0, n) as a virtual column named `name` -- the expression in the reference's function form, e.g.
 * "mult(price,qty)" or "add(div(a,b),2.5)"; NULL = built from the program -- and returns its index in *column.  An
 * identical program (same ops, literals compared by their bits) registered before returns that index and keeps its
 * name. */
int pgpu_table_add_expression(pgpu_table table, const pgpu_expr_op* ops, int32_t n, const char* name, int32_t* column);
/* A virtual column's program and name: *n = its ops (ops receives min(cap, *n) of them; ops may be NULL when cap is 0),
 * name receives at most name_cap bytes, NUL-terminated.  PGPU_ERR_NOT_FOUND for a column that is no virtual one. */
int pgpu_table_expression(pgpu_table table, int32_t column, pgpu_expr_op* ops, int32_t cap, int32_t* n, char* name,
                          int32_t name_cap);

/* Expressions in GROUP BY -- GROUP BY CASE WHEN age < 18 THEN 0 WHEN age < 65 THEN 1 ELSE 2 END, GROUP BY a + b, GROUP
 * BY country, clicks / impressions: the reference's NoDictionary*GroupKeyGenerator over a transform function.  A
 * group-by expression is a *derived column* of the table: per pinned segment a dictionary and a fixed-bit forward
 * index, what the segment creator would have written had the expression been ingested as a column.  It is built on the
 * GPU when a plan (or one of the readers below) first names it in a segment, under the table's mutex, and kept with the
 * segment until the segment is unpinned; pgpu_table_device_bytes counts it.  Everything after the scan's forward-index
 * read sees an ordinary dictionary column: every group table (LDS, global, hash, partitioned), numGroupsLimit with its
 * first-seen meaning, DISTINCTCOUNT / PERCENTILE / expression aggregations beside it, finalize, ORDER BY and the trims.
 * pgpu_table_add_group_expression registers the program (pgpu_table_add_expression's validation and limits) with the
 * reference's result type R of the expression -- DOUBLE for arithmetic; INT, LONG, FLOAT or DOUBLE as a CASE folds its
 * branches -- and returns an index in a range of its own, PGPU_GROUP_EXPR_COLUMN_BASE + k, above every real column and
 * every index pgpu_table_add_expression returns.  The identity is (program, result_type): an identical registration
 * returns the same index.  pgpu_query.group_by[] may name the index; a predicate or an aggregation naming it is
 * PGPU_ERR_INVALID_ARGUMENT, as a pgpu_table_add_expression column in group_by stays (bad column).
 * Values: the evaluator's double per doc, read as R -- the integer of it under INT / LONG, the float under FLOAT (the
 * double is (double)(float) of one by construction), the double itself under DOUBLE.  Two docs share a group iff their
 * values have the same bits in the dictionaries' order (Double.doubleToLongBits, as the reference's
 * Double2IntOpenHashMap compares): -0.0 and +0.0 are two groups, every NaN is one group that sorts above +inf.  The
 * result's key column has type R (pgpu_result_key_dictionary*) and is named by the expression's function form.
 * numEntriesScannedPostFilter counts the distinct real columns the query projects -- the operands of group-by
 * expressions among them, the derived column itself not.  A segment carrying a star-tree is scanned for such a query.
 * Readers that accept the index (and build the derived column of that segment on first use):
 * pgpu_segment_column_info / _bytes, pgpu_read_dict_ids, pgpu_table_dictionary_size / _i64 / _f64.
 * Declined with PGPU_ERR_UNSUPPORTED (the message names "GROUP BY expression"): a STRING operand (at registration); a
 * raw (no-dictionary) operand in a planned segment; a product of the operands' dictionary sizes in a planned segment
 * above PGPU_GROUP_EXPR_MAX_PRODUCT (the candidate values are enumerated over it); R = LONG with an operand LONG column
 * whose dictionary in a planned segment leaves +-2^53 (a LONG operand that reaches a comparison as it is likewise, as
 * in an aggregation's CASE); an external d_table (pgpu_plan_create_execute, pgpu_plan_execute, pgpu_plan_finalize);
 * every cross-GPU or key-range entry point -- pgpu_plan_finalize_range, pgpu_plan_exchange_*, pgpu_result_exchange_rows
 * / _merge_rows, pgpu_plan_combine_mode, pgpu_plan_combine, pgpu_result_combine_rows: a derived dictionary belongs to
 * one table on one rank, and merging them is not built.  pgpu_result_datatable is made (values travel in it, not
 * dictIds).  No group-table path is declined on account of a derived column.  At most PGPU_GROUP_EXPR_MAX_PER_TABLE
 * expressions per table (PGPU_ERR_INVALID_ARGUMENT). */
#define PGPU_GROUP_EXPR_COLUMN_BASE (1 << 20)
#define PGPU_GROUP_EXPR_MAX_PER_TABLE 64
#define PGPU_GROUP_EXPR_MAX_PRODUCT (1 << 22)
int pgpu_table_add_group_expression(pgpu_table table, const pgpu_expr_op* ops, int32_t n, const char* name,
                                    int32_t result_type /* PGPU_INT .. PGPU_DOUBLE */, int32_t* column);

typedef struct {
  int32_t num_predicates;
  int32_t num_filter_ops;     /* 0 = no filter (MatchAllFilterOperator) */
  const pgpu_predicate* predicates;
  const pgpu_filter_op* filter;
  int32_t num_group_by;       /* >= 1 (the group-by path) */
  int32_t num_aggs;
  const int32_t* group_by;    /* table column indices */
  const pgpu_agg* aggs;
  int32_t num_groups_limit;   /* InstancePlanMakerImplV2.DEFAULT_NUM_GROUPS_LIMIT = 100000 (:70); <= 0 = unlimited */
  int32_t options;            /* PGPU_OPT_* bits */
  int64_t end_time_ms;        /* QueryContext.getEndTimeMs(): absolute deadline in ms since the Unix epoch (the
                                 broker's arrival time + timeoutMs); 0 = none.  Checked before launch and on the
                                 device (the persistent scans stop taking tiles past it): PGPU_ERR_TIMEOUT.  Not part
                                 of the compiled-plan cache key. */
} pgpu_query;

/* Query options: debug option useStarTree=false (StarTreeUtils.isStarTreeDisabled, core/startree/StarTreeUtils.java:
 * 51-59) keeps the scan path on segments that carry a star-tree. */
#define PGPU_OPT_NO_STAR_TREE 1
/* Group-by combine of SQL mode (queryOptions groupByMode=sql: GroupByOrderByCombineOperator) instead of the default
 * PQL GroupByCombineOperator: no inter-segment cap of 2 x numGroupsLimit (GroupByCombineOperator.java:61,78-80,138)
 * and no numGroupsLimitReached flag (GroupByOrderByCombineOperator.java:246).  Either way a segment whose group-key
 * space exceeds numGroupsLimit keeps its first numGroupsLimit groups in first-seen docId order
 * (DictionaryBasedGroupKeyGenerator.java:1101-1113), as Pinot's map-based holders do. */
#define PGPU_OPT_SQL_GROUP_BY 2
/* Compile the plan afresh instead of reusing the table's cached compilation of the same query over the same
 * segments (the cache is dropped whenever pinned state changes; PGPU_PLAN_CACHE=0 disables it process-wide). */
#define PGPU_OPT_NO_PLAN_CACHE 4
/* Record HIP timing events around the execution's kernels for pgpu_plan_timing.  Off by default: each event is a
 * marker packet between two dependent dispatches of the stream (about 10 us per query of gaps at 125 segments,
 * measured), so a serving query carries none.  Not part of the plan-cache key. */
#define PGPU_OPT_TIMING 8
/* Bit-reproducible SUM / AVG over FLOAT / DOUBLE columns (and over integer columns whose sums could pass int64 and
 * are therefore summed as doubles).  Without it such a sum is accumulated with floating-point atomics in whatever
 * order the scan's workgroups reach a group, and its last bits can differ between two runs of one query.  With it
 * every operand is split into W = 2 or 3 fixed-point digits of K bits below 2^E, the digits are summed as integers
 * (any order gives the same sums) and the result is rounded to a double once: the same bits in every run, for every
 * segment layout, accumulator mode and tile order.  The plan picks (E, K, W) from the values it can read -- the
 * segments' dictionaries, raw columns and star-tree metrics -- and the docs it covers (pgpu_plan_fp_sum_format):
 *   exact      the digits hold every bit of every operand: the result is the correctly rounded exact sum;
 *   quantised  operands span more than W K bits: each is truncated toward zero to a multiple of 2^(E - W K) first,
 *              an error below 2^-(W K) of the largest operand per doc -- less than one rounding of a running double
 *              sum costs; the result is the correctly rounded sum of the truncated operands, still order-independent.
 * A column with a NaN or an infinity among its values keeps the floating-point accumulator (mode 0).
 * A plan with such sums takes W accumulator slots per summed column (the limit of 24 counts them) and runs as one
 * launch from pgpu_plan_create_execute.  Part of the plan-cache key.  Queries without such a sum plan and run exactly
 * as without the option.
 * Plain plans (pgpu_plan_create / pgpu_plan_create_execute) derive (E, K, W) from this rank's segments alone.  They
 * take the scan kernel's LDS / global / hash tables, not the radix- or hash-partitioned pipelines (planned as with
 * pgpu_config.partitioned_group_by = 0 and hash_partitions = 0), and are declined with PGPU_ERR_UNSUPPORTED by the
 * cross-GPU entry points (pgpu_plan_combine*, pgpu_plan_exchange_*, pgpu_result_exchange_rows / merge_rows /
 * combine_rows, pgpu_plan_finalize_range, an external d_table): digit sums of different formats do not add.
 * Agreed plans (pgpu_plan_create_agreed, below) take their formats from ranges every rank agreed on: they pass all of
 * those entry points -- after the scan their digits are int64 SUM rows, merged by the collectives as such, and the
 * merged result is the same bits for every rank count, segment-to-rank assignment and collective algorithm -- and
 * they take the partitioned pipelines, whose aggregate kernels split the records' operands (K8d / K8h FX). */
#define PGPU_OPT_EXACT_FP_SUM 16

/* A query compiled against a list of pinned segments (InstancePlanMakerImplV2.makeInstancePlan +
 * per-segment AggregationGroupByPlanNode: predicate evaluators per segment, group-key layout, accumulators). */
typedef struct pgpu_plan_s* pgpu_plan;
typedef struct pgpu_result_s* pgpu_result;

int pgpu_plan_create(pgpu_table table, const int64_t* segment_handles, int32_t num_segments, const pgpu_query* q,
                     pgpu_plan* out);
int pgpu_plan_destroy(pgpu_plan plan);

/* Dense group table layout of a plan: num_slots rows of num_keys 8-byte words (row s holds accumulator s of
 * every group key; row 0 is the COUNT row).  slot_kinds[s] (enum pgpu_slot_kind) gives the element type and the
 * RCCL reduce op that merges two ranks' tables: COUNT/SUM_I64 -> int64 sum, SUM_F64 -> float64 sum,
 * MIN_KEY -> int64 min, MAX_KEY -> int64 max.  num_keys = 0 when the plan uses the hash table (high cardinality). */
enum pgpu_slot_kind { PGPU_SLOT_COUNT = 0, PGPU_SLOT_SUM_I64 = 1, PGPU_SLOT_SUM_F64 = 2, PGPU_SLOT_MIN_KEY = 3,
                      PGPU_SLOT_MAX_KEY = 4 };
int pgpu_plan_layout(pgpu_plan plan, int32_t* num_slots, int64_t* num_keys, int32_t* slot_kinds /* >= 32 */);

/* Cancels the plan's query from any thread (the broker abandoned it; Pinot's BaseCombineOperator cancels the
 * segment tasks' futures, whose operators stop at the next block, BaseOperator.java:37-39).  A finalize waiting for
 * the plan's device work -- or any later one -- returns PGPU_ERR_CANCELLED at once; launches the plan has not
 * issued yet are not issued, and the device work already queued runs out while the plan's scratch stays out of the
 * pool until it has (as for a timeout).  The table and its other queries are unaffected.  Idempotent. */
int pgpu_plan_cancel(pgpu_plan plan);

/* Diagnostics: how the plan's leaves run in the kernels, as (segment, leaf) pairs of the scanned segments per kernel
 * leaf kind (counts[9]: NONE, ALL, RANGE, SET, DOCRANGE, BITMAP (a docId bitmap materialised per query),
 * RAW_RANGE, RAW_IN, BITDIR (inverted-index containers read in place)). */
int pgpu_plan_leaf_kinds(pgpu_plan plan, int64_t* counts);

/* Byte-code sketches of wide filter columns.  When a segment is pinned (or generated), every dictionary-encoded,
 * fixed-bit, unsorted column of at least min_bits bits gets a second forward index of one byte per doc: a code that is
 * monotone in the dictId, where up to 127 of the segment's most frequent dictIds have a code of their own and the
 * dictIds between them share interval codes.  The sketch is kept if the docs of those 127 dictIds are at least
 * min_cover of the segment's.  A plan then scans the 8-bit codes instead of the dictIds for the predicates the codes
 * answer exactly -- an equality or IN on frequent values, a range that ends on code boundaries -- per (segment,
 * column), and only if they answer every scan leaf of the query on that column; results and statistics are the same
 * bit for bit.  Defaults: on, min_bits 12, min_cover 1/8.  pgpu_table_set_filter_sketch: min_bits 0 switches sketches
 * off for segments pinned afterwards and for planning (sketches already built stay pinned, unused); like
 * pgpu_table_set_config it applies to plans made afterwards and clears the compiled-plan cache.
 * pgpu_segment_sketch_info: *ncodes 0 = the column has no sketch; else its codes, the docs whose dictId has a code
 * of its own, the device bytes of the code bytes (counted in pgpu_table_device_bytes) and, where cap > 0, the first
 * min(cap, ncodes + 1) entries of first_id (code c holds the dictIds [first_id[c], first_id[c + 1]); first_id[ncodes]
 * is the cardinality).  pgpu_plan_sketch_leaves: the plan's (scanned segment, scan leaf) pairs on sketched columns
 * that read the sketch, and those that stayed on the dictIds. */
int pgpu_table_set_filter_sketch(pgpu_table table, int32_t min_bits, double min_cover);
int pgpu_segment_sketch_info(pgpu_table table, int64_t segment_handle, int32_t column, int32_t* ncodes,
                             int64_t* singleton_docs, int64_t* bytes, int32_t* first_id_out, int32_t cap);
int pgpu_plan_sketch_leaves(pgpu_plan plan, int64_t* pairs_using_sketch, int64_t* pairs_declined);

/* Diagnostics of PGPU_PRED_REGEXP_LIKE.  pgpu_regex_check compiles the pattern only: PGPU_OK with the DFA's states, byte
 * classes and table bytes (each pointer may be NULL), or the decline with its message.  pgpu_regex_match_host runs the
 * host interpreter of the same table over value[0, len) (*matched 0 / 1).  pgpu_table_regexp_dict_ids returns the
 * table-global dictIds of a STRING column that match, as computed on the GPU: bit i of `bitmap` (`words` 64-bit words,
 * at least ceil(dictionary size / 64); the spare bits are 0) is set when global dictId i matches.
 * pgpu_plan_regexp_stats: what making the plan built for its REGEXP_LIKE leaves -- out4[0] the (segment, leaf) local
 * sets written on the GPU, out4[1] how many of them went through an affine local-to-global mapping (no LUT read),
 * out4[2] the device bytes of the leaves' dictionaries (blob + offsets, as counted in pgpu_table_device_bytes), out4[3]
 * the bytes of their DFA tables. */
int pgpu_plan_regexp_stats(pgpu_plan plan, int64_t* out4);
int pgpu_regex_check(const char* pattern, int32_t* states, int32_t* classes, int64_t* table_bytes);
int pgpu_regex_match_host(const char* pattern, const void* value, int64_t len, int32_t* matched);
int pgpu_table_regexp_dict_ids(pgpu_table table, int32_t column, const char* pattern, uint64_t* bitmap, int64_t words);

/* Diagnostics: the group-by path the plan's scan takes (a numGroupsLimit plan: its first part's).  LDS: tables
 * privatised per workgroup in LDS; GLOBAL: a dense table with global atomics; HASH: the global open-addressing hash
 * table (sparse key spaces); PARTITIONED: radix-partitioned dense keys aggregated per partition in LDS; HASH_PARTITIONED:
 * hash-partitioned sparse keys aggregated per partition in LDS hash tables. */
enum pgpu_group_path { PGPU_PATH_LDS = 0, PGPU_PATH_GLOBAL = 1, PGPU_PATH_HASH = 2, PGPU_PATH_PARTITIONED = 3,
                       PGPU_PATH_HASH_PARTITIONED = 4 };
int pgpu_plan_group_path(pgpu_plan plan, int32_t* path);

/* Runs the plan on `stream` (hipStream_t; NULL = the table's stream): predicate translation results are
 * uploaded, the fused filter/group/aggregate kernel runs over every segment, and the dense group table is
 * written to d_table (device pointer, num_slots * num_keys * 8 bytes, caller-owned; may be NULL to use an
 * internal buffer).  Asynchronous: nothing is copied back.  Replaces the per-segment operator loop
 * (AggregationGroupByOperator.getNextBlock, core/operator/query/AggregationGroupByOperator.java:62-79) and the
 * combine (GroupByCombineOperator.processSegments, :113-160) for the segments of the plan. */
int pgpu_plan_execute(pgpu_plan plan, void* stream, void* d_table);

/* Compacts the (possibly RCCL-reduced) dense group table into a result: groups with COUNT > 0, their global
 * dictionary ids and finished aggregation values.  Synchronises `stream`. */
int pgpu_plan_finalize(pgpu_plan plan, void* stream, const void* d_table, pgpu_result* out);

/* Finalize of one key-range shard of a dense group table: d_table_shard is [num_slots][key_count] words holding
 * the composite keys [key_begin, key_begin + key_count) -- a rank's part after a reduce-scatter of the per-GPU
 * tables (the multi-GPU combine of large key spaces; every rank then returns its own disjoint groups, as Pinot
 * servers return partial tables).  PGPU_ERR_UNSUPPORTED for hash-mode tables and for queries whose
 * numGroupsLimit is below the key space (those finalize the whole table). */
int pgpu_plan_finalize_range(pgpu_plan plan, void* stream, const void* d_table_shard, int64_t key_begin,
                             int64_t key_count, pgpu_result* out);

/* ---- cross-GPU combine of hash-mode tables (key spaces past 2^26): a hash-partitioned all-to-all instead of the
 * element-wise merge of dense tables.  Replaces GroupByOrderByCombineOperator's IndexedTable.upsert loop
 * (core/operator/combine/GroupByOrderByCombineOperator.java:170-181) across GPUs: every rank splits its executed
 * table's groups by owner rank (a hash of the global composite key, the same on every rank), the records travel over
 * RCCL (all_to_all), and each owner merges what it receives into a fresh table and finalizes its own disjoint groups.
 * A record is 1 + num_slots int64 words: the composite key, then the slot words.  `kinds` (num_slots entries, or
 * NULL = the plan's own) are the kinds every rank agreed on: an int64 SUM may travel as float64 when another rank's
 * sum of that slot is float64.  Plans with ARRAY_MAP key stages (rank-local keys) and numGroupsLimit plans exchange
 * their finalized result rows instead (pgpu_result_exchange_rows). */
/* Per-owner group counts of the executed table (counts[nparts], nparts <= 64); waits for the plan's work. */
int pgpu_plan_exchange_counts(pgpu_plan plan, void* stream, int32_t nparts, int64_t* counts);
/* The records, grouped by owner in rank order, into d_out (device, cap records). */
int pgpu_plan_exchange_export(pgpu_plan plan, void* stream, int32_t nparts, const int32_t* kinds, void* d_out,
                              int64_t cap);
/* Replaces the plan's table by the merge of n received records (device); pgpu_plan_finalize then returns them. */
int pgpu_plan_exchange_merge(pgpu_plan plan, void* stream, const int32_t* kinds, const void* d_records, int64_t n);

/* ---- communicator and the one-call cross-GPU combine (what a Pinot server calls instead of the combine merge when
 * its segments are spread over the GPUs of a node; GroupByCombineOperator.java:113-160 /
 * GroupByOrderByCombineOperator.java:170-181).  One process (or thread) per GPU; every rank issues the same
 * combine calls in the same order, as with any RCCL communicator.
 *   PGPU_COMM_RCCL  RCCL over xGMI, one rank per GPU; collectives run on the caller's stream.  librccl.so.1 is opened
 *                   on first use (the copy already in the process if there is one).
 *   PGPU_COMM_HOST  processes of one machine exchanging through /dev/shm: the same combine with several ranks on one
 *                   GPU (RCCL refuses two ranks per device).  Synchronous, staged through host memory; for
 *                   rehearsals and tests, never the measured path.
 * The unique id (PGPU_COMM_ID_BYTES) is made by one rank and handed to the others out of band (the JVM's own
 * cluster channel, torch's TCPStore, ...), as ncclUniqueId is. */
typedef struct pgpu_comm_s* pgpu_comm;
#define PGPU_COMM_RCCL 0
#define PGPU_COMM_HOST 1
#define PGPU_COMM_ID_BYTES 128
int pgpu_comm_unique_id(int32_t kind, void* id /* PGPU_COMM_ID_BYTES */);
int pgpu_comm_create(int32_t kind, const void* id, int32_t nranks, int32_t rank, int32_t device, pgpu_comm* out);
/* Drops the handle; the communicator goes with the last plan combined on it (pgpu_plan_finalize / _destroy). */
int pgpu_comm_destroy(pgpu_comm comm);
int pgpu_comm_rank(pgpu_comm comm, int32_t* rank, int32_t* nranks);
/* Host memory, blocking: recv[nranks * bytes] = every rank's `bytes` bytes in rank order (dictionary unions, the
 * mode agreement, timing barriers -- the small control exchanges of a multi-GPU query). */
int pgpu_comm_allgather(pgpu_comm comm, const void* send, int64_t bytes, void* recv);
/* Waits on peers -- the host exchanges above and in the combine, and a combined plan's finalize waiting for its
 * stream-ordered collectives -- end with PGPU_ERR_TIMEOUT after timeout_ms (<= 0: no limit of the communicator's
 * own; default 600 000), or earlier at the query's end_time_ms / pgpu_plan_cancel.  An expired wait aborts the
 * communicator (RCCL: ncclCommAbort, so collectives a peer never joined stop waiting on the device); every later call
 * on it fails with PGPU_ERR_DEVICE and the caller creates a new one (BaseCombineOperator's timeout,
 * BaseCombineOperator.java:193-203: the combine always ends by the query deadline). */
int pgpu_comm_set_timeout(pgpu_comm comm, int64_t timeout_ms);
/* Gives the communicator up from any thread (a server shutting a query down); see pgpu_comm_set_timeout. */
int pgpu_comm_abort(pgpu_comm comm);
/* *aborted = 1 once the communicator was given up (a wait on peers expired, or pgpu_comm_abort): every collective on
 * it fails with PGPU_ERR_DEVICE until pgpu_comm_recreate. */
int pgpu_comm_status(pgpu_comm comm, int32_t* aborted);
/* Collective over the handle's ranks: a fresh communicator of the same transport, ranks and device from a new id
 * (made by one rank with pgpu_comm_unique_id and handed to the others out of band, as for pgpu_comm_create -- the
 * aborted one cannot carry it), replacing the handle's; the timeout carries over.  The recovery after one rank's
 * failure aborted the communicator (BaseCombineOperator.java:101-107, 193-203: a failed or timed-out combine fails
 * that query only, the server keeps serving): every rank calls it, then the next query combines as before.  Plans
 * combined on the old communicator keep it alive until they are finalized or destroyed.  No other call may use the
 * handle while it runs. */
int pgpu_comm_recreate(pgpu_comm comm, const void* id);

/* How the ranks' partial results of one query merge. */
#define PGPU_COMBINE_LOCAL 0          /* one rank: nothing to merge */
#define PGPU_COMBINE_ALL_REDUCE 1     /* dense tables, element-wise, every rank ends with the merged table */
#define PGPU_COMBINE_REDUCE_SCATTER 2 /* dense tables >= shard_bytes: rank r ends with keys [r*chunk, (r+1)*chunk) */
#define PGPU_COMBINE_HASH 3           /* hash-mode tables: groups hashed to an owner rank, all-to-all, owner merges */
#define PGPU_COMBINE_ROWS 4           /* numGroupsLimit plans / ARRAY_MAP key stages: finalized rows, by owner */
/* Collective: the mode every rank agrees on for this query (a plan, executed or not, of the query over the rank's
 * segments), and in kinds[num_slots] the slot kinds the merge runs in (an int64 SUM travels as float64 when another
 * rank's sum of the slot is float64).  Modes that differ between ranks fall back to ROWS, which merges any plan
 * kind.  PGPU_ERR_INVALID_ARGUMENT when the ranks' group-by dictionaries differ (pgpu_table_add_dictionary_values
 * with the union first), and likewise -- the message names DISTINCTCOUNT and the column -- when their snapshots of a
 * DISTINCTCOUNT column's global dictionary differ.  A plan with DISTINCTCOUNT whose ranks do not agree on ALL_REDUCE or
 * REDUCE_SCATTER is declined (PGPU_ERR_UNSUPPORTED: its rows do not merge).  The caller may reuse the answer for every
 * later query of the same shape. */
int pgpu_plan_combine_mode(pgpu_plan plan, pgpu_comm comm, int64_t shard_bytes, int32_t* mode, int32_t* kinds);
/* Collective, ordered on `stream`: merges the executed plan's table (d_table as given to execute, NULL = the plan's
 * own) with the other ranks' in `mode` (ALL_REDUCE, REDUCE_SCATTER or HASH).  For REDUCE_SCATTER, d_shard (NULL = the
 * plan's scratch) receives [num_slots][key_count] words, key_begin / key_count say which keys; they are 0 / num_keys
 * otherwise.  pgpu_plan_finalize(plan, stream, d_table) then returns this rank's share of the merged groups (all of
 * them for ALL_REDUCE; disjoint shares otherwise).
 * PGPU_AGG_DISTINCTCOUNT (ALL_REDUCE and REDUCE_SCATTER, d_table NULL; a caller table is declined as at execute): the
 * sets merge by OR, which no collective offers, so the side bitmaps are reduce-scattered by key range first.  With
 * chunk = ceil(num_keys / nranks), rank r owns keys [min(num_keys, r*chunk), min(num_keys, (r+1)*chunk)) -- the
 * REDUCE_SCATTER split.  A bitmap is key-major, so per distinct column one all-to-all sends each peer its range's
 * rows straight from the bitmap; the owner ORs the nranks blocks into its own rows, stores their popcounts into the
 * aggregation's row of the table and zeroes that row outside its range.  The int64 SUM of the all-reduce /
 * reduce-scatter that follows then yields the merged count on every rank (in the owner's shard).  Memory: the
 * receive area holds nranks x (owned keys) x ceil(cardinality / 64) x 8 bytes per distinct column -- about the side
 * bitmaps (at most 1 GiB per plan) once more; link bytes: (nranks - 1) / nranks of the rank's bitmaps sent, on top of
 * the table's collectives.  The receive area is allocated before any collective and the ranks exchange their status
 * once (a host round trip only plans with DISTINCTCOUNT pay), so a rank that fails there fails with its peers.
 * Afterwards the rank holds the merged value *sets* of its own key range only (the counts are in the table); nothing
 * returns the sets yet.  With one rank the same code runs and gives the local answer. */
int pgpu_plan_combine(pgpu_plan plan, pgpu_comm comm, void* stream, void* d_table, int32_t mode, const int32_t* kinds,
                      void* d_shard, int64_t* key_begin, int64_t* key_count);
/* Collective, ROWS mode: the finalized result's rows split by owner, exchanged, merged by the owner as the broker
 * merges server responses.  *out = this rank's disjoint share. */
int pgpu_result_combine_rows(pgpu_result r, pgpu_comm comm, pgpu_result* out);

/* One-call form: plan + execute + finalize (the whole per-server query path). */
int pgpu_execute_groupby(pgpu_table table, const int64_t* segment_handles, int32_t num_segments, const pgpu_query* q,
                         void* stream, pgpu_result* out);

/* Plan + execute in one call, streamed: the segment list is planned in equal chunks and each chunk's scan is
 * launched as soon as it is planned, so the GPU scans while the host still translates predicates for the next
 * chunk (one launch per chunk; plans with star-tree segments, partitioned or staged scans run as one launch).
 * The plan is returned executed: finalize (or merge across GPUs, then finalize) as after pgpu_plan_execute. */
int pgpu_plan_create_execute(pgpu_table table, const int64_t* segment_handles, int32_t num_segments,
                             const pgpu_query* q, void* stream, void* d_table, pgpu_plan* out);

/* Timing of the last execution of this plan (HIP events on the execution stream; the query carried PGPU_OPT_TIMING,
 * else PGPU_ERR_INVALID_ARGUMENT), microseconds:
 * [0] whole execute, [1] the scan kernel launches (summed), [2] number of scan launches, [3] the star-tree kernels
 * (traversal + pre-aggregated document scan; 0 without star-tree segments).  out holds 4 doubles. */
int pgpu_plan_timing(pgpu_plan plan, double* out4);

/* The fixed-point format of aggregation `agg` of a plan made with PGPU_OPT_EXACT_FP_SUM: out = {mode, E, K, W}, mode
 * 0 = none (not a FLOAT / DOUBLE sum, the option is off, or the column holds a non-finite value: E = K = W = 0),
 * 1 = exact, 2 = quantised; K is the digit width the kernels use. */
int pgpu_plan_fp_sum_format(pgpu_plan plan, int agg, int32_t out[4]);

/* Agreement on the fixed-point formats of PGPU_OPT_EXACT_FP_SUM across ranks (GroupByDataTableReducer merges the
 * servers' partial sums by AggregationFunction.merge, SumAggregationFunction.java:120-123, in arrival order: the
 * reproducible counterpart needs one format on every server).  One pgpu_fp_sum_range per aggregation of the query:
 * what this rank's plan could read for it. */
typedef struct {
  int32_t is_sum;        /* 1: SUM / AVG over a numeric column; 0: COUNT / MIN / MAX (other fields 0) */
  int32_t any, finite;   /* any: a finite non-zero operand exists; finite: no operand is a NaN or an infinity */
  int32_t E, L;          /* valid when any: |v| < 2^E, lowest set mantissa bit >= 2^L over those operands */
  int32_t reserved;
  int64_t docs;          /* documents of this rank's segments (the digits' headroom counts them) */
  double  int_sum_bound; /* integer columns: sum over segments of numDocs x max|value|, rounded up; else 0 */
} pgpu_fp_sum_range;
/* Local, no device work beyond what planning needs: out[a] for each of q's num_aggs aggregations, read from what a
 * plan of q over these segments reads -- their dictionaries, raw columns' values and the pre-aggregated doubles of
 * star-trees that may answer q (SumAggregationFunction.java:66-73 is the operand: the value as a double). */
int pgpu_query_fp_sum_ranges(pgpu_table table, const int64_t* segment_handles, int32_t num_segments,
                             const pgpu_query* q, pgpu_fp_sum_range* out);
/* Pure host: all[r * num_aggs + a] of nranks ranks -> out[a].  finite: AND; any: OR; E: max and L: min over the ranks
 * with any; docs and int_sum_bound: sums.  PGPU_ERR_INVALID_ARGUMENT when ranks differ on an aggregation's is_sum. */
int pgpu_fp_sum_ranges_merge(const pgpu_fp_sum_range* all, int32_t nranks, int32_t num_aggs, pgpu_fp_sum_range* out);
/* Collective: pgpu_comm_allgather of every rank's ranges and the merge, in place. */
int pgpu_comm_agree_fp_sum_ranges(pgpu_comm comm, pgpu_fp_sum_range* ranges, int32_t num_aggs);
/* pgpu_plan_create over agreed ranges, one per aggregation (a single rank passes its own: the plan then has the
 * formats of its plain plan).  q carries PGPU_OPT_EXACT_FP_SUM, else PGPU_ERR_INVALID_ARGUMENT.  An integer column's
 * sum is an int64 slot iff the agreed int_sum_bound is below 2^62, on every rank alike; every other sum has the
 * format of the agreed {E, L, any, finite} and the agreed docs, or the float64 slot when finite is 0.  The agreed
 * ranges are part of the plan-cache key; a numGroupsLimit plan hands them to its parts. */
int pgpu_plan_create_agreed(pgpu_table table, const int64_t* segment_handles, int32_t num_segments,
                            const pgpu_query* q, const pgpu_fp_sum_range* agreed, pgpu_plan* out);

/* Star-tree work of the last execution (after finalize): [0] segments answered from their star-tree, [1] their
 * tree nodes (28 bytes each, OffHeapStarTreeNode), [2] star-tree documents the residual scan read. */
int pgpu_plan_star_work(pgpu_plan plan, int64_t* out3);
/* Geometry of the plan's scan and of its last scan launch (after an execution; the partitioned group-by has its own
 * passes and leaves [4..14] zero).  out holds 16 values:
 * [0] the plan's grid (workgroups of a launch with at least that many tiles), [1] the scan's dynamic LDS bytes,
 * [2] tiles per workgroup the LDS reserves for the STATS_LEAP2 bytes (0: the plan keeps none), [3] the plan's tiles;
 * of the last launch: [4] 1 = contiguous runs per workgroup, 0 = XCD-interleaved tiles, [5] CU slots the runs are
 * weighted by (0 = equal shares), [6..9] their weights in 1/256ths (pgpu_config.slot_weight_step), [10] the most
 * tiles any of its workgroups took, [11] its workgroups, [12] its tiles, [13] 1 = no other execution of the table
 * was in flight (weights are for such launches only), [14] 1 = weights were declined because the longest weighted
 * run could pass [2]; [15] the scan kernel's instance: 0 sparse, 1 dense, 2 dense without gathers, 3 - 5 the sparse
 * specialisations (index + scan pair, pure AND, pure AND with 4-doc batches), 6 / 7 the sparse / dense instance of
 * plans with fixed-point sums (PGPU_OPT_EXACT_FP_SUM), 8 / 9: sparse / dense of plans with PGPU_AGG_DISTINCTCOUNT,
 * 10 / 11: sparse / dense of plans with PGPU_AGG_PERCENTILE (side histograms), 12 / 13: sparse / dense of plans with
 * expression aggregations (pgpu_table_add_expression). */
int pgpu_plan_scan_geometry(pgpu_plan plan, int64_t* out16);
/* Bytes of the star-tree metric arrays the last execution's document scan read (after finalize): the 64-byte
 * sectors holding at least one matched document, summed over the arrays read; -1 where finalize did not read the
 * counter back (tables past 512 KB).  The star path's line-granular bytes model (bench.py). */
int pgpu_plan_star_metric_bytes(pgpu_plan plan, int64_t* bytes);

/* Per plan segment (plan order): 1 if the segment is scanned, 0 if its filter folds to always-false against the
 * segment's dictionaries (EmptyFilterOperator, core/plan/FilterPlanNode.java:146-176).  out holds num_segments. */
int pgpu_plan_scanned_segments(pgpu_plan plan, uint8_t* out);

/* numEntriesScannedInFilter of one segment (ExecutionStatistics, AndDocIdSet.getNumEntriesScannedInFilter,
 * core/operator/docidsets/AndDocIdSet.java:148-155) from the doc sets of its predicates: `filter` is the query's
 * postfix program; leaf_types[i] is predicate i's leaf operator in this segment (enum pgpu_leaf_type, the outcome
 * of FilterOperatorUtils.getLeafFilterOperator, core/operator/filter/FilterOperatorUtils.java:42-82) and
 * leaf_masks[i] its matching docs (bit d % 32 of word d / 32; may be NULL for EMPTY / ALL leaves).  Pinot's
 * iterators (AndDocIdSet / OrDocIdSet merging, SVScanDocIdIterator.applyAnd, AndDocIdIterator leap-frog,
 * OrDocIdIterator) are replayed over the sets.  The plans compute the same statistic on the device; this entry is
 * the host form (a caller holding the doc sets, tests).  PGPU_LEAF_RANGE_INDEX (RangeIndexBasedFilterOperator) is an
 * index-based leaf ranked after the bitmap leaves; the entries of its own partial-match scan are not included (the
 * caller adds them: pgpu_range_index_partial_entries).  PGPU_LEAF_EXPRESSION (ExpressionFilterOperator, a predicate
 * on an expression) is a scan-based leaf ranked after every other AND child (priority 10, stable;
 * FilterOperatorUtils.java:171-172) whose iterator is ExpressionScanDocIdIterator: applyAnd counts the docs it is
 * handed; next() evaluates blocks of up to 10000 docs (DocIdSetPlanNode.MAX_DOC_PER_CALL), counting every doc of a
 * block, until one holds a match; advance(target) looks inside the current block, uncounted, when the target lies in
 * it and otherwise starts the next block at the target.  So a lone leaf or an OR child counts numDocs, and in a
 * leap-frog AND the blocks start wherever the other children's docs land. */
enum pgpu_leaf_type { PGPU_LEAF_EMPTY = 0, PGPU_LEAF_MATCH_ALL = 1, PGPU_LEAF_SCAN = 2, PGPU_LEAF_SORTED = 3,
                      PGPU_LEAF_BITMAP = 4, PGPU_LEAF_RANGE_INDEX = 5, PGPU_LEAF_EXPRESSION = 6 };
int pgpu_filter_entries_scanned(const pgpu_filter_op* filter, int32_t num_filter_ops, const int32_t* leaf_types,
                                const uint32_t* const* leaf_masks, int32_t num_leaves, int32_t num_docs,
                                int64_t* out);

/* ---- after the combine: server trim, server response, broker reduce (the step after the device path) */
/* ORDER BY expression over the result: a group-by column (index = its position in the GROUP BY) or an aggregation
 * (index = its position in the query; compared by its final result, as TableResizer's extractors do). */
enum pgpu_order_kind { PGPU_ORDER_GROUP_BY = 0, PGPU_ORDER_AGGREGATION = 1 };
typedef struct {
  int32_t kind;
  int32_t index;
  int32_t ascending;
} pgpu_order_by;
/* SQL-mode query options of the combine (QueryContext / InstancePlanMakerImplV2.java:64-84). */
typedef struct {
  int32_t num_order_by;
  const pgpu_order_by* order_by;
  int32_t limit;                       /* LIMIT (SQL default 10) */
  int32_t min_server_group_trim_size;  /* min.server.group.trim.size (default 5000); <= 0 disables server trim */
  int32_t group_trim_threshold;        /* groupby.trim.threshold (default 1000000) */
  int32_t num_select;                  /* broker reduce: the SELECT list in order (kind / index as for ORDER BY; */
  const pgpu_order_by* select;         /* ascending unused); 0 = every group-by column, then every aggregation */
} pgpu_sql_trim;

/* The server's SQL-mode combined table (GroupByOrderByCombineOperator.java:82-97 + IndexedTable.finish,
 * core/data/table/IndexedTable.java:62-89): with ORDER BY the top max(limit * 5, minServerGroupTrimSize) groups in
 * ORDER BY order; without it `limit` groups (Pinot keeps the first keys its threads insert -- thread-order
 * dependent; here the smallest composite keys); trim disabled: every group (sorted if ORDER BY).  Ties order by
 * composite key.  Pinot resizes lossily past groupby.trim.threshold groups; the device combine is exact, so the
 * result is the exact top records.  `out` is a new result (destroy both). */
int pgpu_result_trim_sql(pgpu_result r, const pgpu_sql_trim* spec, pgpu_result* out);

/* PQL-mode trim (AggregationGroupByTrimmingService.trimIntermediateResultsMap, :54-120): per aggregation the rows of
 * its top max(limit * 5, 5000) groups (MIN: smallest values, the others largest; by final result), applied only past
 * 4 x that many groups; final_results != 0 gives the broker's trimFinalResults (:126-150): the top `limit`.
 * rows is [num_aggs][cap] (may be NULL to get counts[num_aggs] only). */
int pgpu_result_trim_pql(pgpu_result r, int32_t limit, int32_t final_results, int64_t* rows, int64_t cap,
                         int64_t* counts);

/* Server response of a SQL-mode group-by (IntermediateResultsBlock.getResultDataTable, core/operator/blocks/
 * IntermediateResultsBlock.java:329-345; DataTableBuilder.java:55-103; DataTableImplV3.toBytes :183-290): DataTable V3
 * bytes with the group-by columns and the aggregations' intermediate results (COUNT LONG, SUM / MIN / MAX DOUBLE,
 * AVG an AvgPair OBJECT) of every row of `r`, and the block's execution statistics as metadata.  `table` supplies
 * the group keys' values and column names.  out == NULL: *len = the size needed. */
int pgpu_result_datatable(pgpu_result r, pgpu_table table, void* out, int64_t cap, int64_t* len);

/* Broker reduce of SQL-mode group-by responses (GroupByDataTableReducer.java:290-330): the servers' DataTable V3
 * bytes merged by key (AggregationFunction.merge), final results, ORDER BY (ties by key), LIMIT, and summed
 * statistics, written as the BrokerResponseNative JSON (resultTable + statistics) into json (NUL-terminated;
 * json == NULL: *len = the length needed without the NUL). */
int pgpu_broker_reduce_sql(const void* const* tables, const int64_t* lens, int32_t num_tables,
                           const pgpu_sql_trim* spec, char* json, int64_t cap, int64_t* len);

/* ---- results: AggregationGroupByResult (core/query/aggregation/groupby/AggregationGroupByResult.java:31-81) */
int pgpu_result_num_groups(pgpu_result r, int64_t* n);
/* The table-global dictionary that group-by column `key`'s ids index, as the result's plan saw it: a pin that grows
 * the table's dictionary while the query runs does not re-label this result (GroupKeyGenerator.getKeys reads the
 * segment dictionaries the operator was built on).  *snapshot_id identifies the snapshot (callers cache the values
 * by it); *size its entries.  Values as for pgpu_table_dictionary_{i64,f64,str}. */
int pgpu_result_key_dictionary(pgpu_result r, int key, uint64_t* snapshot_id, int64_t* size);
int pgpu_result_key_dictionary_i64(pgpu_result r, int key, int64_t* out);
int pgpu_result_key_dictionary_f64(pgpu_result r, int key, double* out);
int pgpu_result_key_dictionary_str(pgpu_result r, int key, uint8_t* blob, int64_t blob_cap, int64_t* offsets);
/* [n][num_group_by] global dictionary ids, in the result's group order: ascending composite key for dense tables
 * (Pinot's ARRAY / INT_MAP holders) and hash-mode results below 4096 groups; larger hash-mode results (the LONG_MAP
 * holder, whose iterator runs in fastutil hash order) come in partition order, which may differ between runs.  The
 * trims (pgpu_result_trim_sql / _trim_pql) compare composite keys themselves, so their output never depends on it. */
int pgpu_result_group_ids(pgpu_result r, int32_t* out);
/* Column `key` of the above ([n] dictIds of group-by column `key`): a plain copy, the layout the result holds. */
int pgpu_result_group_ids_column(pgpu_result r, int key, int32_t* out);
/* Zero-copy views valid until pgpu_result_destroy (a JNI caller wraps them in direct ByteBuffers):
 * the [n] dictIds of group-by column `key`, and the [n] accumulator words of aggregation `agg` (agg = -1: the
 * COUNT words, i.e. AvgPair.count) with their form: 0 = exact int64, 1 = IEEE double bits, 2 = order-preserving
 * int64 key of a double (MIN/MAX over FLOAT/DOUBLE; pgpu_result_values converts it). */
int pgpu_result_group_ids_view(pgpu_result r, int key, const int32_t** out);
int pgpu_result_words_view(pgpu_result r, int agg, const uint64_t** out, int32_t* form);
/* Per aggregation i (query order): value per group as Pinot's intermediate result holds it (double) — COUNT,
 * SUM, MIN, MAX, and AVG's AvgPair.sum; AVG's AvgPair.count via pgpu_result_avg_counts. */
int pgpu_result_values(pgpu_result r, int agg, double* out);
int pgpu_result_avg_counts(pgpu_result r, int agg, int64_t* out);
/* Exact integer accumulators where the aggregation is integer-valued (COUNT, AVG count, SUM over INT/LONG):
 * returns PGPU_ERR_INVALID_ARGUMENT for floating-point sums. */
int pgpu_result_values_i64(pgpu_result r, int agg, int64_t* out);
/* ExecutionStatistics (core/operator/ExecutionStatistics.java:42): numDocsScanned, numEntriesScannedInFilter,
 * numEntriesScannedPostFilter, numTotalDocs, plus [4] numSegmentsProcessed, [5] numSegmentsMatched. */
int pgpu_result_stats(pgpu_result r, int64_t* out6);
/* numGroupsLimitReached (GroupByCombineOperator.java:215-219, PQL mode): 1 when the combined groups reach
 * numGroupsLimit. */
int pgpu_result_groups_limit_reached(pgpu_result r, int32_t* out);
/* Accumulator slots of a result (num_slots, and kinds[num_slots], enum pgpu_slot_kind; slot 0 = COUNT). */
int pgpu_result_slot_kinds(pgpu_result r, int32_t* num_slots, int32_t* kinds);
/* Cross-rank merge of finalized results (any plan kind; each GPU as one Pinot server): the result's rows as int64
 * records [num_keys dictIds, num_slots words] grouped by owner rank (a hash of the dictIds), into rows (n records),
 * counts[nparts] per owner; `kinds` as for pgpu_plan_exchange_export.  The ranks' dictionaries must agree (union). */
int pgpu_result_exchange_rows(pgpu_result r, int32_t nparts, const int32_t* kinds, int64_t* rows, int64_t* counts);
/* The owner's merge of n received records (GroupByDataTableReducer's merge across servers, AggregationFunction.merge)
 * into a new result in ascending key order, with tmpl's aggregations, dictionaries and statistics. */
int pgpu_result_merge_rows(pgpu_result tmpl, const int64_t* rows, int64_t n, const int32_t* kinds, pgpu_result* out);
int pgpu_result_destroy(pgpu_result r);
/* The same as pgpu_result_destroy (the name SURVEY.md §8b lists). */
int pgpu_free_result(pgpu_result r);

/* Docid match bitmap of one segment's filter (the FilterOperator's doc set, K2): bit d of 64-bit word d/64.
 * out_words must hold ceil(num_docs / 64) words. */
int pgpu_filter_bitmap(pgpu_table table, int64_t segment_handle, const pgpu_query* q, uint64_t* out_words);

/* ============================================================================ star-tree index */

/* A star-tree of one segment (StarTreeV2: seglocal/startree/OffHeapStarTree.java:38-80 + the star-tree's own
 * documents).  Dimension / metric columns are indexes into the segment's (= the table's) columns.
 *   nodes      : num_nodes records of 7 little-endian int32 {dimensionId, dimensionValue, startDocId, endDocId,
 *                aggregatedDocId, firstChildId, lastChildId} in BFS order (OffHeapStarTreeNode.java:28-64; the
 *                node array of the star-tree file, after its header);
 *   dim_fwd[d] : the star-tree documents' dictIds of dimension d, BIG_ENDIAN fixed-bit with the segment column's
 *                bitsPerElement (StarTreeLoaderUtils.java:73-92); STAR = dictId 0 (StarTreeV2Constants.java:38);
 *   metrics    : the function-column pairs (AggregationFunctionColumnPair, segspi/index/startree/
 *                AggregationFunctionColumnPair.java:25-50); COUNT's column is -1;
 *   metric_f64 : per pair, the pre-aggregated double per star-tree document (SUM / MIN / MAX, AVG's sum), NULL for
 *                COUNT — the values of the PASS_THROUGH raw chunk column "fn__col" (BaseSingleTreeBuilder.java:
 *                471-475), decoded by the caller;
 *   metric_i64 : per pair, COUNT's long (and AVG's count) per star-tree document, NULL otherwise. */
typedef struct {
  int32_t num_dims;
  int32_t num_metrics;
  int32_t num_nodes;
  int32_t num_docs;
  const int32_t* dim_columns;
  const uint8_t* nodes;
  const uint8_t* const* dim_fwd;
  const int64_t* dim_fwd_len;
  const pgpu_agg* metrics;
  const double* const* metric_f64;
  const int64_t* const* metric_i64;
} pgpu_startree_desc;

/* Pins a star-tree for a pinned segment (StarTreeIndexContainer at ImmutableSegmentLoader.java:198-201).  Queries
 * that fit it (StarTreeUtils.isFitForStarTree, core/startree/StarTreeUtils.java:151-176) then traverse it on the
 * GPU (StarTreeFilterOperator, core/startree/operator/StarTreeFilterOperator.java:234-338) and aggregate the
 * pre-aggregated documents (StarTreeGroupByExecutor, core/startree/executor/StarTreeGroupByExecutor.java:60-71). */
int pgpu_attach_startree(pgpu_table table, int64_t segment_handle, const pgpu_startree_desc* desc);

/* Pins the bitmap inverted index of one column of a pinned segment: `bytes` is the `<column>.bitmap.inv` file
 * (v1) or the column's `inverted_index` buffer of columns.psf (v3) verbatim -- (cardinality + 1) big-endian int32
 * bitmap offsets, then one portable-format RoaringBitmap per dictId (BitmapInvertedIndexWriter /
 * BitmapInvertedIndexReader, seglocal/segment/index/readers/BitmapInvertedIndexReader.java:40-70; the reader the
 * DefaultIndexReaderProvider hands to the DataSource).  From then on EQ / NOT_EQ / IN / NOT_IN predicates on an
 * unsorted column of that segment are BitmapBasedFilterOperator leaves (FilterOperatorUtils.java:72-79): the
 * matching dictIds' containers are ORed into a docId bitmap on the device per query, and the leaf scans no
 * forward-index entries.  Malformed bitmaps (bad cookie, overruns, docIds >= numDocs) return
 * PGPU_ERR_INVALID_ARGUMENT.  Attach at segment load, before queries reference the segment (as Pinot builds its
 * DataSource readers): re-attaching replaces the column's index and must not race plan creation on that segment;
 * plans created before a re-attach (or an unpin) keep the index they were planned on alive until destroyed. */
int pgpu_attach_inverted_index(pgpu_table table, int64_t segment_handle, int32_t column, const void* bytes,
                               int64_t num_bytes);
/* The same file checked on the host without a device or a table (a loader can reject a bad index before it pins
 * the segment): the offsets and every Roaring bitmap are validated exactly as pgpu_attach_inverted_index does for a
 * column of `cardinality` values in a segment of num_docs documents; *total_docs (may be NULL) = the summed bitmap
 * cardinalities (num_docs for a single-value column's complete index). */
int pgpu_inverted_index_check(const void* bytes, int64_t num_bytes, int32_t cardinality, int32_t num_docs,
                              int64_t* total_docs);

/* A range index (`<column>.bitmap.range`, DefaultIndexReaderProvider.newRangeIndexReader,
 * seglocal/segment/index/readers/DefaultIndexReaderProvider.java:128-139) of a dictionary-encoded column of a pinned
 * segment.  A RANGE predicate on the column (unless it is sorted) then runs as RangeIndexBasedFilterOperator
 * (FilterOperatorUtils.java:57-62): an index-based leaf, ordered after the bitmap leaves in an AND (:143-178), whose
 * docs are exactly the predicate's matches (read here from the forward index) and whose numEntriesScannedInFilter is
 * its partial-match scan (RangeIndexBasedFilterOperator.java:110-126):
 *   version 1 (RangeIndexCreator / RangeIndexReaderImpl): header (version, value type "INT", range count, the ranges'
 *             first dictIds + the last range's end, bitmap offsets) and one Roaring bitmap per range, all read and
 *             validated; the partial matches are the first and last ranges the predicate touches
 *             (RangeIndexReaderImpl.java:198-264);
 *   version 2 (BitSlicedRangeIndexCreator / BitSlicedRangeIndexReader): exact, no partial matches (0 entries); only
 *             the header is read.
 * Another version is skipped as Pinot skips it (no range index, PGPU_OK); a malformed version-1 file fails with
 * PGPU_ERR_INVALID_ARGUMENT; raw (no-dictionary) columns: PGPU_ERR_UNSUPPORTED.  Re-attaching replaces the index;
 * num_bytes = 0 detaches it.  Plans created before keep what they planned with. */
int pgpu_attach_range_index(pgpu_table table, int64_t segment_handle, int32_t column, const void* bytes,
                            int64_t num_bytes);
/* Host check of a range index file without a table: *version (0 = not a range index Pinot loads), *num_ranges and
 * the documents of its ranges (total_docs, the column's docs for a complete index). */
int pgpu_range_index_check(const void* bytes, int64_t num_bytes, int32_t cardinality, int32_t num_docs,
                           int32_t* version, int32_t* num_ranges, int64_t* total_docs);
/* numEntriesScannedInFilter of RangeIndexBasedFilterOperator for the dictId range [lo, hi] (inclusive) over a range
 * index file: the documents of its partial-match bitmap (0 for version 2). */
int pgpu_range_index_partial_entries(const void* bytes, int64_t num_bytes, int32_t cardinality, int32_t num_docs,
                                     int32_t lo, int32_t hi, int64_t* entries);

/* Host-side reader of a raw forward index (PGPU_FWD_RAW_FIXED bytes; FixedByteChunkSVForwardIndexReader.readValuesSV
 * over every chunk, LZ4 chunks decompressed as LZ4Decompressor / LZ4WithLengthDecompressor do): num_docs values of a
 * column of `data_type` -- INT / LONG into out_i64, every type as double into out_f64 (either may be NULL).  The
 * decoder pgpu_pin_segment uses; pure host code. */
int pgpu_raw_forward_index_values(const void* fwd, int64_t fwd_len, int32_t data_type, int32_t num_docs,
                                  int64_t* out_i64, double* out_f64);

/* Host-side bitmap inverted-index creator (OffHeapBitmapInvertedIndexCreator + BitmapInvertedIndexWriter,
 * seglocal/segment/creator/impl/inv/BitmapInvertedIndexWriter.java:60-78) over a fixed-bit forward index: writes
 * the `<column>.bitmap.inv` bytes (portable Roaring without run containers) into `out` (capacity out_cap) and their
 * length into *out_len; out == NULL only reports the length.  Pure host code, for segment fixtures and benches. */
int pgpu_build_inverted_index(const void* fwd, int64_t fwd_len, int32_t bits, int32_t num_docs, int32_t cardinality,
                              void* out, int64_t out_cap, int64_t* out_len);

/* Host-side star-tree builder (BaseSingleTreeBuilder + OnHeapSingleTreeBuilder, seglocal/startree/v2/builder/):
 * builds the star-tree of a segment given in Pinot's byte format (the pgpu_segment_desc of pgpu_pin_segment;
 * column_types per column), split order (column indexes), dimensions without star nodes (indexes into the split
 * order), function-column pairs and maxLeafRecords (<= 0: StarTreeV2BuilderConfig default 10000).  Pure host code:
 * no device is needed.  The result is read with pgpu_startree_get_desc and released with pgpu_startree_destroy. */
typedef struct pgpu_startree_s* pgpu_startree;
int pgpu_startree_build(const pgpu_segment_desc* segment, const int32_t* column_types, const int32_t* split_order,
                        int32_t num_dims, const int32_t* skip_star_dims, int32_t num_skip, const pgpu_agg* pairs,
                        int32_t num_pairs, int32_t max_leaf_records, pgpu_startree* out);
int pgpu_startree_get_desc(pgpu_startree st, pgpu_startree_desc* out);
/* Star-tree `star_tree_id` of a segment from Pinot's own files, as StarTreeLoaderUtils.loadStarTreeV2 reads them
 * (seglocal/startree/v2/store/StarTreeLoaderUtils.java:57-107): `index` is the segment's star_tree_index file (v1;
 * in a v3 segment the star-tree buffer of columns.psf), `index_map` the text of star_tree_index_map
 * (StarTreeIndexMapUtils.java:150-190: "<id>.<column>.<STAR_TREE|FORWARD_INDEX>.<OFFSET|SIZE> = n").  The
 * OffHeapStarTree buffer is validated as its constructor does (magic 0xBADDA55B00DAD00D, version 1, header length,
 * buffer size; OffHeapStarTree.java:45-80); its dimension names (the split order) are matched against
 * column_names (the table's columns); dimension forward indexes are FixedBitSVForwardIndexReaderV2 bytes with the
 * segment column's bits_per_element[column]; each "<fn>__<col>" pair's raw PASS_THROUGH chunk forward index
 * (versions 2 / 3) is decoded -- COUNT as LONG, SUM / MIN / MAX as DOUBLE (FixedByteChunkSVForwardIndexReader),
 * AVG as AvgPair bytes (VarByteChunkSVForwardIndexReader) -- and pairs of other functions are skipped.  num_docs is
 * the star-tree's total docs (metadata startree.v2.<id>.total.docs).  Pure host code; attach the result with
 * pgpu_startree_get_desc + pgpu_attach_startree, release it with pgpu_startree_destroy. */
int pgpu_startree_load(const void* index, int64_t index_len, const char* index_map, int64_t index_map_len,
                       int32_t star_tree_id, int32_t num_docs, int32_t num_columns, const char* const* column_names,
                       const int32_t* bits_per_element, pgpu_startree* out);
/* Number of star-tree records that come straight from the segment (sorted + aggregated rows), before the star-node
 * and aggregated documents (-1 for star-trees read by pgpu_startree_load: the files do not record it). */
int pgpu_startree_num_raw_records(pgpu_startree st, int32_t* n);
int pgpu_startree_destroy(pgpu_startree st);

/* ============================================================================ synthetic segments (bench) */

/* Column generators of BASELINE.md §3: value = f(splitmix64(seed_c ^ global_row)),
 * seed_c = (0x5EED0000 + column_index) << 32.  UNIFORM: lo + h % (hi - lo); ZIPF: ids[first k with cdf[k] > u];
 * TABLE: table[h % n].  The segment (dictionary = sorted distinct values present, fixed-bit forward index) is
 * built on the device and pinned directly; bytes are identical to Pinot's segment creator on the same values. */
enum pgpu_gen_kind { PGPU_GEN_UNIFORM = 0, PGPU_GEN_ZIPF = 1, PGPU_GEN_TABLE = 2 };
typedef struct {
  int32_t kind;
  int32_t column_index;
  int64_t lo, hi;             /* UNIFORM */
  int32_t n;                  /* ZIPF ranks / TABLE size */
  int32_t reserved;
  const double* cdf;          /* ZIPF cumulative distribution (host) */
  const int64_t* ids;         /* ZIPF rank -> value (host), ascending-id order not required */
  const double* table;        /* TABLE values (host) */
} pgpu_gen_column;
int pgpu_generate_segment(pgpu_table table, const pgpu_gen_column* columns, int32_t num_columns, int64_t row0,
                          int32_t num_docs, int64_t* segment_handle);
/* Copies a pinned segment column's bytes back to the host (parity checks of the generator). */
int pgpu_segment_column_info(pgpu_table table, int64_t segment_handle, int column, int32_t* cardinality,
                             int32_t* bits, int64_t* dict_len, int64_t* fwd_len);
int pgpu_segment_column_bytes(pgpu_table table, int64_t segment_handle, int column, uint8_t* dict_out,
                              uint8_t* fwd_out);

#ifdef __cplusplus
}
#endif
#endif
