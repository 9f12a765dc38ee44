// k_sketch.hip -- gfx950 kernels that build the byte-code sketch of a wide dictionary filter column when its segment is
// pinned (col_sketch.h, rt_sketch.cpp): the per-dictId doc histogram the code assignment starts from, and the encode
// pass that writes one code byte per doc.  A one-off per (segment, column); the scans then read the result as an 8-bit
// forward index.  An object of its own, so that no existing kernel is compiled differently.
#include "device.h"

namespace pgpu {

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// dictIds one workgroup counts in LDS per pass (64 KiB of u32 cells)
constexpr int kSketchHistRange = 16384;
// 8192-doc tiles per workgroup of the histogram
constexpr int kSketchHistTiles = 8;

// Histogram: workgroup (x, y) counts the docs of its kSketchHistTiles tiles whose dictId lies in pass y's range
// [y * range, y * range + range) in LDS, then adds the non-zero cells to `counts`.  A hot dictId (C3's queried account
// holds 8 % of the docs) thus meets in LDS -- a few lanes of a wave on one LDS address -- and reaches global memory as one
// atomic per workgroup, not one per doc: same-address global atomics serialise.  A dictId >= card (a forward index not
// yet validated) is counted nowhere; docs past num_docs are padding.
__global__ __launch_bounds__(256) void sketch_hist_kernel(const uint32_t* __restrict__ fwd, const int32_t bits,
                                                          const int32_t num_docs, const int32_t card,
                                                          uint32_t* __restrict__ counts) {
  __shared__ uint32_t h[kSketchHistRange];
  const int tid = threadIdx.x;
  const int32_t base = (int32_t)blockIdx.y * kSketchHistRange;
  const uint32_t n = (uint32_t)(card - base < kSketchHistRange ? card - base : kSketchHistRange);
  for (uint32_t i = tid; i < n; i += 256) h[i] = 0;
  __syncthreads();
  const int64_t ngroups = ((int64_t)num_docs + 31) >> 5;
  for (int k = 0; k < kSketchHistTiles; ++k) {
    const int64_t group = ((int64_t)blockIdx.x * kSketchHistTiles + k) * 256 + tid;
    if (group >= ngroups) break;
    const int64_t doc0 = group << 5;
    uint32_t ids[16];
    decode_group<0>(fwd, bits, group, ids);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t id = ids[i] - (uint32_t)base;
      if (doc0 + i < num_docs && id < n) atomicAdd(&h[id], 1u);
    }
    decode_group<16>(fwd, bits, group, ids);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t id = ids[i] - (uint32_t)base;
      if (doc0 + 16 + i < num_docs && id < n) atomicAdd(&h[id], 1u);
    }
  }
  __syncthreads();
  for (uint32_t i = tid; i < n; i += 256) {
    const uint32_t v = h[i];
    if (v) atomicAdd(counts + base + i, v);
  }
}

// Encode: one lane per 32-doc group; its dictIds go through the dictId -> code table (card bytes, cache-resident) and
// leave as 32 code bytes, doc i of the segment at byte i -- the layout of an 8-bit forward index (leaf_range_b<8>).
// Docs past num_docs get code 0; the words past the last group stay as the caller zeroed them.
__global__ __launch_bounds__(256) void sketch_encode_kernel(const uint32_t* __restrict__ fwd, const int32_t bits,
                                                            const int32_t num_docs, const int32_t card,
                                                            const uint8_t* __restrict__ lut, uint32_t* __restrict__ out) {
  const int64_t group = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ngroups = ((int64_t)num_docs + 31) >> 5;
  if (group >= ngroups) return;
  const int64_t doc0 = group << 5;
  gmem<uint8_t>* __restrict__ t = gp(lut);
  uint32_t w[8];
  uint32_t ids[16];
  decode_group<0>(fwd, bits, group, ids);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = q * 4 + j;
      const uint32_t id = ids[i];
      const uint32_t c = (doc0 + i < num_docs && id < (uint32_t)card) ? (uint32_t)t[id] : 0u;
      word |= c << (8 * j);
    }
    w[q] = word;
  }
  decode_group<16>(fwd, bits, group, ids);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = q * 4 + j;
      const uint32_t id = ids[i];
      const uint32_t c = (doc0 + 16 + i < num_docs && id < (uint32_t)card) ? (uint32_t)t[id] : 0u;
      word |= c << (8 * j);
    }
    w[4 + q] = word;
  }
  uint32_t* o = out + group * 8;
#pragma unroll
  for (int q = 0; q < 8; ++q) o[q] = w[q];
}

int launch_sketch_hist(const uint32_t* fwd, int32_t bits, int32_t num_docs, int32_t card, uint32_t* counts,
                       void* stream) {
  if (num_docs <= 0 || card <= 0) return 0;
  if (bits < 1 || bits > 31) return -1;
  const int64_t tiles = ((int64_t)num_docs + kTileDocs - 1) / kTileDocs;
  const int64_t gx = (tiles + kSketchHistTiles - 1) / kSketchHistTiles;
  const int64_t gy = ((int64_t)card + kSketchHistRange - 1) / kSketchHistRange;
  if (gx > INT32_MAX || gy > 65535) return -1;
  hipLaunchKernelGGL(sketch_hist_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, S(stream), fwd, bits, num_docs,
                     card, counts);
  return PGPU_HIP_OK(hipGetLastError());
}

int launch_sketch_encode(const uint32_t* fwd, int32_t bits, int32_t num_docs, int32_t card, const uint8_t* lut,
                         uint32_t* out, void* stream) {
  if (num_docs <= 0 || card <= 0) return 0;
  if (bits < 1 || bits > 31) return -1;
  const int64_t grid = ((((int64_t)num_docs + 31) >> 5) + 255) / 256;
  hipLaunchKernelGGL(sketch_encode_kernel, dim3((unsigned)grid), dim3(256), 0, S(stream), fwd, bits, num_docs, card, lut,
                     out);
  return PGPU_HIP_OK(hipGetLastError());
}

}  // namespace pgpu
