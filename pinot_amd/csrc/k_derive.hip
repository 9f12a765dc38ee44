// k_derive.hip -- gfx950 kernels that build the derived column of a group-by expression in one pinned segment (GROUP BY
// a + b, GROUP BY CASE WHEN ..: derive.h, rt_dict.cpp ensure_derived).  A one-off per (segment, expression): the scan
// then reads the result as any dictionary column.  An object of its own, so that no existing kernel is compiled
// differently.
#include "derive.h"
#include "expr_docs.h"

namespace pgpu {

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Candidates: thread p is one combination of the operands' segment-local dictIds (mixed radix, operand 0 fastest); its
// key is what a doc holding those dictIds would have.  The task is a kernel argument: program, pointers and radices are
// scalar operands.
__global__ __launch_bounds__(256) void derive_candidates_kernel(const KDeriveTask T, const int64_t product,
                                                                int64_t* __restrict__ keys) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= product) return;
  const int nc = T.prog.ncols;
  double v[kExprMaxCols][1], out[1];
  int64_t rest = p;
#pragma unroll
  for (int c = 0; c < kExprMaxCols; ++c) {
    v[c][0] = 0.0;
    if (c < nc) {  // wave-uniform
      const int64_t card = T.card[c];
      const int64_t id = rest % card;  // < card: inside the operand's dictId -> double table
      rest /= card;
      v[c][0] = gp(T.ops.dval[c])[id];
    }
  }
  expr_eval<1>(T.prog, v, out);
  keys[p] = expr_value_key(out[0]);
}

// Ids, the hot kernel: one lane per doc, four 64-doc steps of a wave at a time (expr_eval_docs, expr_docs.h).  The
// doc's key is then looked up in the sorted candidates (every key a doc can have is among them: the candidates enumerate
// the operands' whole dictionaries) and the index stored, 4 bytes per doc, coalesced.  Marking: a candidate's word is
// tested before it is written, so the three candidates of a CASE over a million docs take a handful of plain stores of
// the same 1, not an atomic per doc; racing stores write the same value.
__global__ __launch_bounds__(256) void derive_ids_kernel(const KDeriveTask T, const int64_t* __restrict__ cand,
                                                         const int32_t ncand, uint32_t* __restrict__ scratch,
                                                         uint32_t* __restrict__ used) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t num_docs = T.num_docs;
  gmem<int64_t>* __restrict__ set = gp(cand);
  constexpr int kWaveDocs = kDeriveBlockDocs / 4;
  constexpr int kU = 4;  // 64-doc steps in flight per wave
  for (int it = 0; it < kWaveDocs / (64 * kU); ++it) {
    const int64_t base = (int64_t)blockIdx.x * kDeriveBlockDocs + wave * kWaveDocs + it * (64 * kU);  // wave-uniform
    if (base >= num_docs) break;
    bool live[kU];
    double out[kU];
    expr_eval_docs<kU>(T.ops, T.prog, base, lane, num_docs, live, out);
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      if (!live[u]) continue;
      int a = key_lower_bound(set, ncand, expr_value_key(out[u]));
      if (a >= ncand) a = ncand - 1;  // (cannot happen: the key is a candidate; keeps every index inside `used`)
      scratch[base + u * 64 + lane] = (uint32_t)a;
      if (used[a] == 0u) used[a] = 1u;
    }
  }
}

// Pack: one workgroup per forward-index tile of 8192 docs = 256 * bits big-endian words.  The docs' local dictIds
// (remap of the candidate index) are staged in LDS with coalesced reads -- lane-adjacent docs -- and every thread then
// assembles whole output words from it, lane-adjacent words, so the stores coalesce too.  The LDS row is padded by one
// word per 32 docs: a thread's docs start 32 / bits apart from its neighbour's, which at 1 bit would put a wave's reads on
// one bank.  Docs past num_docs are dictId 0, and the last workgroup zeroes the kFwdPadWords spare words: the layout
// pgpu_pin_segment gives a column, whole.
__global__ __launch_bounds__(256) void derive_pack_kernel(const uint32_t* __restrict__ scratch,
                                                          const int32_t* __restrict__ remap, const int32_t num_docs,
                                                          const int32_t bits, uint32_t* __restrict__ fwd,
                                                          const int64_t fwd_words) {
  __shared__ uint32_t ids[kDeriveBlockDocs + kDeriveBlockDocs / 32];
  const int64_t doc0 = (int64_t)blockIdx.x * kDeriveBlockDocs;
  for (int k = 0; k < kDeriveBlockDocs / 256; ++k) {
    const int d = k * 256 + threadIdx.x;
    uint32_t id = 0;
    if (doc0 + d < num_docs) id = (uint32_t)remap[scratch[doc0 + d]];
    ids[d + (d >> 5)] = id;
  }
  __syncthreads();
  const int64_t word0 = (int64_t)blockIdx.x * 256 * bits;
  for (int k = 0; k < bits; ++k) {
    const int w = k * 256 + threadIdx.x;  // word of the tile: stream bits [32 w, 32 w + 32)
    const int first = (32 * w) / bits, last = (32 * w + 31) / bits;  // docs with a bit in it; last < 8192
    uint32_t word = 0;
    for (int d = first; d <= last; ++d) {
      const uint64_t id = ids[d + (d >> 5)];
      const int sh = 32 - (d * bits - 32 * w) - bits;  // the id's lowest bit, counted from the word's lowest
      word |= sh >= 0 ? (uint32_t)(id << sh) : (uint32_t)(id >> -sh);
    }
    if (word0 + w < fwd_words) fwd[word0 + w] = bswap32(word);
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x < kFwdPadWords) {
    const int64_t w = (int64_t)gridDim.x * 256 * bits + threadIdx.x;
    if (w < fwd_words) fwd[w] = 0u;
  }
}

int launch_derive_candidates(const KDeriveTask& T, int64_t product, int64_t* keys, void* stream) {
  if (product <= 0) return 0;
  const int64_t grid = (product + 255) / 256;
  if (grid > INT32_MAX) return -1;
  hipLaunchKernelGGL(derive_candidates_kernel, dim3((unsigned)grid), dim3(256), 0, S(stream), T, product, keys);
  return PGPU_HIP_OK(hipGetLastError());
}

int launch_derive_ids(const KDeriveTask& T, const int64_t* cand, int32_t ncand, uint32_t* scratch, uint32_t* used,
                      void* stream) {
  if (T.num_docs <= 0 || ncand <= 0) return 0;
  const int64_t grid = ((int64_t)T.num_docs + kDeriveBlockDocs - 1) / kDeriveBlockDocs;
  hipLaunchKernelGGL(derive_ids_kernel, dim3((unsigned)grid), dim3(256), 0, S(stream), T, cand, ncand, scratch, used);
  return PGPU_HIP_OK(hipGetLastError());
}

int launch_derive_pack(const uint32_t* scratch, const int32_t* remap, int32_t num_docs, int32_t bits, uint32_t* fwd,
                       int64_t fwd_words, void* stream) {
  if (bits < 1 || bits > 31) return -1;
  const int64_t grid = ((int64_t)num_docs + kDeriveBlockDocs - 1) / kDeriveBlockDocs;
  if (grid <= 0) return 0;  // (no docs: the caller zeroes the spare words)
  hipLaunchKernelGGL(derive_pack_kernel, dim3((unsigned)grid), dim3(256), 0, S(stream), scratch, remap, num_docs, bits,
                     fwd, fwd_words);
  return PGPU_HIP_OK(hipGetLastError());
}

}  // namespace pgpu
