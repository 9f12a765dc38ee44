// k_regex.hip -- gfx950 kernels of REGEXP_LIKE / LIKE (regex_dfa.h, rt_regex.cpp): the pattern's DFA run once over a
// STRING column's table-global dictionary, and the matching global dictIds turned into each planned segment's bitset
// over its local dictIds -- the words a LEAF_SET of the scan reads.  Both run when a plan is made, never per doc.  An
// object of its own, so that no existing kernel is compiled differently.
#include "device.h"
#include "regex_dfa.h"

namespace pgpu {

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

constexpr int kRegexTableEntries = kRegexMaxTableBytes / 2;

// One dictionary value per lane.  The class map and the transition table are copied into LDS once per workgroup (the
// table's cap leaves room for four workgroups a CU); a lane then walks its value's bytes and EOS, one LDS class lookup
// and one LDS table lookup per byte, and stops once it is in the accepting row 0.  The values of a sorted dictionary
// are neighbours in the blob, so the lanes of a wave read the same cache lines: each lane loads the aligned 8-byte word
// that holds its next byte and consumes what of it is the value's.  The last word of the last value lies inside the
// allocation because the blob is padded to whole words.  A wave's 64 results become one word through the ballot.
__global__ __launch_bounds__(256) void regex_match_dict_kernel(const uint8_t* __restrict__ cls_g,
                                                               const uint16_t* __restrict__ table_g,
                                                               const int32_t table_entries, const uint32_t start_row,
                                                               const uint32_t eos_class,
                                                               const uint64_t* __restrict__ blob,
                                                               const uint32_t* __restrict__ offsets, const int64_t n,
                                                               uint64_t* __restrict__ out) {
  // (both are filled through 4-byte words)
  __shared__ alignas(8) uint16_t tab[kRegexTableEntries];
  __shared__ alignas(8) uint8_t cls[kRegexClsBytes];
  {  // (the device copy of the table is padded to whole 8-byte words; table_entries <= kRegexTableEntries, even cap)
    const uint32_t* tg = reinterpret_cast<const uint32_t*>(table_g);
    uint32_t* tl = reinterpret_cast<uint32_t*>(tab);
    for (int k = threadIdx.x; k < (table_entries + 1) / 2; k += 256) tl[k] = tg[k];
    const uint32_t* cg = reinterpret_cast<const uint32_t*>(cls_g);
    uint32_t* cl = reinterpret_cast<uint32_t*>(cls);
    for (int k = threadIdx.x; k < kRegexClsBytes / 4; k += 256) cl[k] = cg[k];
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool matched = false;
  if (i < n) {
    uint32_t p = offsets[i];
    const uint32_t end = offsets[i + 1];
    uint32_t row = start_row;
    while (p < end && row != 0) {
      uint64_t w = blob[p >> 3] >> ((p & 7u) * 8u);
      uint32_t nb = min(8u - (p & 7u), end - p);
      p += nb;
      for (; nb; --nb) {  // (row 0 is absorbing: the bytes behind a match change nothing)
        row = tab[row + cls[w & 0xFFu]];
        w >>= 8;
      }
    }
    if (row != 0) row = tab[row + eos_class];
    matched = row == 0;
  }
  const unsigned long long m = __ballot(matched);
  if ((threadIdx.x & 63) == 0 && i < n) out[i >> 6] = m;
}

int launch_regex_match_dict(const uint8_t* cls, const uint16_t* table, int32_t table_entries, int32_t num_classes,
                            int32_t start_row, int32_t eos_class, const uint8_t* blob, const uint32_t* offsets, int64_t n, uint64_t* out,
                            void* stream) {
  // every row offset the kernel adds a class to is a multiple of num_classes below table_entries (regex_dfa.h), so a
  // class below num_classes keeps every table read inside the table_entries copied into LDS
  if (num_classes < 1 || table_entries < num_classes || table_entries > kRegexTableEntries ||
      table_entries % num_classes || start_row < 0 || start_row >= table_entries || start_row % num_classes ||
      eos_class < 0 || eos_class >= num_classes)
    return -1;
  const int64_t grid = (n + 255) / 256;
  if (grid <= 0) return 0;
  if (grid > INT32_MAX) return -1;
  hipLaunchKernelGGL(regex_match_dict_kernel, dim3((unsigned)grid), dim3(256), 0, S(stream), cls, table, table_entries,
                     (uint32_t)start_row, (uint32_t)eos_class, reinterpret_cast<const uint64_t*>(blob), offsets, n, out);
  return PGPU_HIP_OK(hipGetLastError());
}

// One local dictId per lane: its global dictId through the column's LUT (or the affine lut_off + l), that bit of the
// global bitmap, 64 of them one ballot word.  blockIdx.y is the task; a task with fewer values than the largest one
// leaves its spare workgroups at once.
__global__ __launch_bounds__(256) void regex_local_sets_kernel(const KRegexSetTask* __restrict__ tasks,
                                                               const uint32_t* __restrict__ gbits,
                                                               uint32_t* __restrict__ out) {
  const KRegexSetTask t = tasks[blockIdx.y];
  const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if ((int64_t)blockIdx.x * 256 >= t.card) return;  // workgroup-uniform
  bool bit = false;
  if (l < t.card) {
    const uint32_t g = t.lut ? (uint32_t)t.lut[l] : (uint32_t)(t.lut_off + (int32_t)l);
    bit = (gbits[g >> 5] >> (g & 31u)) & 1u;
  }
  const unsigned long long m = __ballot(bit);
  if ((threadIdx.x & 63) == 0 && l < t.card) reinterpret_cast<uint64_t*>(out + t.dst)[l >> 6] = m;
}

int launch_regex_local_sets(const KRegexSetTask* tasks, int32_t num_tasks, int32_t max_card, const uint64_t* global_bits,
                            uint32_t* out, void* stream) {
  const int64_t gx = ((int64_t)max_card + 255) / 256;
  if (gx <= 0) return 0;
  for (int32_t t0 = 0; t0 < num_tasks; t0 += 65535) {  // (gridDim.y's limit)
    const int32_t nt = std::min<int32_t>(65535, num_tasks - t0);
    hipLaunchKernelGGL(regex_local_sets_kernel, dim3((unsigned)gx, (unsigned)nt), dim3(256), 0, S(stream), tasks + t0,
                       reinterpret_cast<const uint32_t*>(global_bits), out);
    if (PGPU_HIP_OK(hipGetLastError())) return -1;
  }
  return 0;
}

}  // namespace pgpu
