// MI355X (gfx950, CDNA4) kernels for the gradient-boosted-tree engine.
//
// MI355X-native replacement for XGBoost's CUDA gpu_hist updater internals
// (the reference delegates them to libxgboost):
//   - quantize_gpair: fp32 gradient pairs -> int64 fixed point
//   - bin_matrix:     fp32 features -> uint8 quantile bins (LDS-cached cuts)
//   - gather + build_histogram: LDS-tiled per-(node,feature,bin) int64
//     gradient histograms, 64-wide-wave layout, deterministic by integer
//     associativity (no float atomics anywhere)
//   - find_splits:    sequential-per-(node,feature) scan, bitwise-identical
//     to the CPU torch reference (same add/divide order)
//   - partition_rows: stable two-pass partition (ballot prefix + scatter;
//     two-phase begin/finish entry, device-planned variant)
//   - apply_tree_binned: row-order walk of one finished tree over the
//     binned matrix, leaf value added into the margin (the tree finish)
//   - grad_fused:     fused objective gradient + |g|/|h| block maxes
//   - predict_trees:  packed-node tree walk (LDS tree-tiled serving path)
//   - predict_leaf / saabas_contribs: the same walk writing leaf indices /
//                     Saabas attributions (float64 sums in an LDS column)
//   - tree_shap:      exact TreeSHAP contributions / interactions in path
//     form, float64, one row per thread (no atomics)
//   - mvs_score / mvs_stats / mvs_hist / mvs_sample: gradient-based row
//     sampling, the sample decided in integer arithmetic
//
// Design notes (per /opt/skills/guides/cdna_hip_programming.md):
//   wave = 64 lanes; LDS = 160 KiB/CU; histogram tiles sized so 1-2
//   workgroups fit per CU; all global traffic vectorized where layout
//   permits; grids sized >> 256 CUs.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#define WAVE 64
#define CHECK_HIP(x)                                                         \
  do {                                                                       \
    hipError_t err = (x);                                                    \
    TORCH_CHECK(err == hipSuccess, "HIP error: ", hipGetErrorString(err));   \
  } while (0)

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// torch spells the ROCm GPU device type with its legacy vendor name in the
// public tensor API; isolate that single spelling here.
static inline bool on_gpu(const torch::Tensor& t) { return t.is_cuda(); }

// ---------------------------------------------------------------------------
// quantize_gpair: [n,2] f32 -> [n,2] i64 (round to nearest)
// ---------------------------------------------------------------------------
// int32 pairs: |q| <= 2^30 by scale construction, so int32 holds each
// row exactly and int64 accumulators hold any sum - half the gradient
// traffic of int64 pairs at identical numerics.
// SUMS: the pass also emits the column sums of what it wrote (the root
// node's quantized gradient totals), so nobody re-reads `out` for them.
// Each block writes its own int64 pair to partials[2 * blockIdx.x ..]; a
// single small block adds the partials up (no same-address global atomics).
// Integer sums are order-free: the result equals out.sum(0) exactly.
#define QUANT_THREADS 256
template <bool SUMS>
__global__ __launch_bounds__(QUANT_THREADS) void quantize_gpair_kernel(
    const float2* __restrict__ gpair, int2* __restrict__ out, double scale_g,
    double scale_h, int64_t n, long long* __restrict__ partials) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  long long sg = 0, sh = 0;
  for (; i < n; i += stride) {
    float2 gp = gpair[i];
    int2 q;
    q.x = (int)llrint((double)gp.x * scale_g);
    q.y = (int)llrint((double)gp.y * scale_h);
    out[i] = q;
    if (SUMS) {
      sg += q.x;
      sh += q.y;
    }
  }
  if (SUMS) {
    #pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
      sg += __shfl_down(sg, off, WAVE);
      sh += __shfl_down(sh, off, WAVE);
    }
    __shared__ long long wsum[QUANT_THREADS / WAVE][2];
    const int wave_id = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) {
      wsum[wave_id][0] = sg;
      wsum[wave_id][1] = sh;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      long long tg = 0, th = 0;
      for (int w = 0; w < QUANT_THREADS / WAVE; ++w) {
        tg += wsum[w][0];
        th += wsum[w][1];
      }
      partials[2 * blockIdx.x] = tg;
      partials[2 * blockIdx.x + 1] = th;
    }
  }
}

// one block: sums[0..1] = column sums of partials [n_blocks, 2]
__global__ __launch_bounds__(QUANT_THREADS) void reduce_pair_partials_kernel(
    const long long* __restrict__ partials, int n_blocks,
    long long* __restrict__ sums) {
  long long sg = 0, sh = 0;
  for (int i = threadIdx.x; i < n_blocks; i += QUANT_THREADS) {
    sg += partials[2 * i];
    sh += partials[2 * i + 1];
  }
  #pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    sg += __shfl_down(sg, off, WAVE);
    sh += __shfl_down(sh, off, WAVE);
  }
  __shared__ long long wsum[QUANT_THREADS / WAVE][2];
  const int wave_id = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    wsum[wave_id][0] = sg;
    wsum[wave_id][1] = sh;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long tg = 0, th = 0;
    for (int w = 0; w < QUANT_THREADS / WAVE; ++w) {
      tg += wsum[w][0];
      th += wsum[w][1];
    }
    sums[0] = tg;
    sums[1] = th;
  }
}

// ---------------------------------------------------------------------------
// bin_matrix: values [n,F] -> bins u8 [n,F].
// bin = count of cuts <= v (upper_bound), clamped to nb-1; NaN -> 255.
// Cuts staged in LDS when they fit (F*max_bin floats; 200*255*4B = 204KB
// does NOT fit -> fall back to L2-resident global reads, still fast since
// cuts are tiny and re-read by every CU via L3).
// ---------------------------------------------------------------------------
template <bool LDS_CUTS>
__global__ void bin_matrix_kernel(const float* __restrict__ values,
                                  uint8_t* __restrict__ out,
                                  const float* __restrict__ cuts,
                                  const int64_t* __restrict__ cut_ptr,
                                  int64_t n, int F, int total_cuts,
                                  int64_t out_stride) {
  extern __shared__ float lds_cuts[];
  const float* C = cuts;
  if (LDS_CUTS) {
    for (int i = threadIdx.x; i < total_cuts; i += blockDim.x)
      lds_cuts[i] = cuts[i];
    __syncthreads();
    C = lds_cuts;
  }
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t total = n * (int64_t)F;
  for (; idx < total; idx += stride) {
    int f = (int)(idx % F);
    float v = values[idx];
    int lo = (int)cut_ptr[f], hi = (int)cut_ptr[f + 1];
    int nb = hi - lo;
    uint8_t b;
    if (isnan(v)) {
      b = 255;
    } else if (nb == 0) {
      b = 0;
    } else {
      // upper_bound: first cut > v
      int l = 0, r = nb;
      while (l < r) {
        int m = (l + r) >> 1;
        if (C[lo + m] <= v) l = m + 1; else r = m;
      }
      if (l > nb - 1) l = nb - 1;
      b = (uint8_t)l;
    }
    out[(idx / F) * out_stride + f] = b;
  }
}

// ---------------------------------------------------------------------------
// gather_gpair_seg: gpair_seg[i] = gpair_q[ridx[i]] for i in [0, n_seg)
// (coalesced writes; the gather read hits L2/L3). Done once per depth so
// the histogram kernel reads gradients coalesced per feature block.
// ---------------------------------------------------------------------------
__global__ void gather_gpair_kernel(const int2* __restrict__ gpair,
                                    const int32_t* __restrict__ ridx,
                                    int2* __restrict__ out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = gpair[(int64_t)(uint32_t)ridx[i]];
}

// ---------------------------------------------------------------------------
// build_histogram: LDS-tiled int64 gradient-pair histograms.
//
// Grid: x = flattened (node, row-chunk), y = feature block.
// Each workgroup accumulates a [FB][n_bins][2] int64 tile in LDS with
// ds-atomics, then merges once into the global histogram with device
// atomics. Integer accumulation => order-independent, bitwise
// deterministic (the checkpoint-determinism contract).
// ---------------------------------------------------------------------------
#define HIST_THREADS 512
static int hist_rows_per_wg() {
  static int v = [] {
    const char* e = getenv("RXGB_HIST_ROWS");
    int r = e ? atoi(e) : 16384;
    return (r >= 1024 && r <= 262144) ? r : 16384;
  }();
  return v;
}
#define HIST_ROWS_PER_WG hist_rows_per_wg()

// VEC16: the binned matrix row stride is 16-byte aligned (padded layout,
// pad bytes == 255) -> one uint4 load fetches a whole 16-feature block of
// a row. Lane rotation spreads one wave-instruction's LDS atomics over 16
// different features (max 4 lanes per feature histogram) so same-bin
// serialization on skewed features drops ~16x.
// One row's 16-feature uint4 -> LDS tile atomics with word-granular lane
// rotation (shared by the single-block and multi-block kernels below).
//
// LDS layout is SoA: g-plane at [f*n_bins + b], h-plane at
// [16*n_bins + f*n_bins + b]. Interleaved (g,h) pairs put the bank index
// at (b*4)%64 -> only bin%16 distinguishes banks; the split doubles the
// spread to bin%32 (PMC: conflict/active 0.74 interleaved).
__device__ __forceinline__ void hist_accum_packed16(
    unsigned long long* lds_hist, uint4 packed, int n_bins, int lane,
    longlong2 gp) {
  const int hplane = 16 * n_bins;
  const int r4 = lane & 3;
  const uint32_t w0 = packed.x, w1 = packed.y, w2 = packed.z, w3 = packed.w;
  const bool s1 = (r4 & 1) != 0, s2 = (r4 & 2) != 0;
  const uint32_t t01 = s1 ? w1 : w0, t23 = s1 ? w3 : w2;
  const uint32_t u01 = s1 ? w2 : w1, u23 = s1 ? w0 : w3;
  const uint32_t rw0 = s2 ? t23 : t01;  // w[(0+r4)&3]
  const uint32_t rw1 = s2 ? u23 : u01;  // w[(1+r4)&3]
  const uint32_t rw2 = s2 ? t01 : t23;  // w[(2+r4)&3]
  const uint32_t rw3 = s2 ? u01 : u23;  // w[(3+r4)&3]
  const uint32_t rws[4] = {rw0, rw1, rw2, rw3};
  // byte-granular second rotation: the 16 lanes sharing a word-rotation
  // phase split 4 ways over the word's features (one v_alignbit), so one
  // wave instruction hits 16 distinct features instead of 4 -> 4x fewer
  // same-bin collisions. The dynamic rotate keeps everything in named
  // registers (rule 20: no runtime-indexed arrays).
  const uint32_t rsh = 8u * ((lane >> 2) & 3);
  const int r2 = (lane >> 2) & 3;
  #pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const uint32_t w = rws[jj];
    const uint32_t wr = (w >> rsh) | (w << ((32u - rsh) & 31u));
    const int fw = ((jj + r4) & 3) * 4;
    #pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int b = (wr >> (8 * kk)) & 0xFF;
      if (b != 255) {
        const int f = fw + ((kk + r2) & 3);
        // XOR swizzle: bank index (cell*2)%64 was feature-independent;
        // ^ (f&7) staggers features across 8 bank offsets. Only valid
        // when b^7 cannot leave the feature's bin range (n_bins==256).
        const int cell =
            (f * n_bins + b) ^ (n_bins == 256 ? (f & 7) : 0);
        unsigned long long* c = &lds_hist[cell];
        atomicAdd(c, (unsigned long long)gp.x);
        atomicAdd(c + hplane, (unsigned long long)gp.y);
      }
    }
  }
}

__device__ __forceinline__ void hist_accum_row16(
    unsigned long long* lds_hist, const uint8_t* __restrict__ bins,
    uint64_t r, int64_t row_stride, int f0, int n_bins, int lane,
    longlong2 gp) {
  const uint4 packed =
      *reinterpret_cast<const uint4*>(bins + r * row_stride + f0);
  hist_accum_packed16(lds_hist, packed, n_bins, lane, gp);
}

// Tiny-node fast path: accumulate a node's rows straight into the
// GLOBAL histogram. For a node with c rows the LDS route pays a
// 16*n_bins*2-cell tile zero + scan per workgroup regardless of c; for
// c*2*16 atomics < that cost (c below ~512 at 256 bins) direct global
// int64 atomics are cheaper - and identically deterministic (integer
// adds in any order). The caller zeroes hist, so partial adds compose.
__device__ inline void hist_direct_rows(
    const uint8_t* __restrict__ bins, const int2* __restrict__ gpair_seg,
    const int32_t* __restrict__ ridx, long long* __restrict__ ghist_node,
    int64_t seg_start, int64_t row_lo, int64_t row_hi, int64_t row_stride,
    int f0, int fcount, int n_bins, int tid, int nthreads) {
  for (int64_t i = row_lo + tid; i < row_hi; i += nthreads) {
    const int64_t seg_i = seg_start + i;
    const int2 gpi = gpair_seg[seg_i];
    const uint64_t r = (uint32_t)ridx[seg_i];
    const uint8_t* rowb = bins + r * row_stride + f0;
    #pragma unroll 4
    for (int f = 0; f < fcount; ++f) {
      const int b = rowb[f];
      if (b != 255) {
        long long* cell =
            &ghist_node[(((size_t)(f0 + f)) * n_bins + b) * 2];
        atomicAdd((unsigned long long*)cell,
                  (unsigned long long)(long long)gpi.x);
        atomicAdd((unsigned long long*)cell + 1,
                  (unsigned long long)(long long)gpi.y);
      }
    }
  }
}

template <int VFB>  // 16: uint4 row loads; 8: uint2; 0: byte fallback
__global__ __launch_bounds__(HIST_THREADS) void build_histogram_kernel(
    const uint8_t* __restrict__ bins,        // [n_rows_total, row_stride]
    const int2* __restrict__ gpair_seg,      // [seg_total] segment order
    const int32_t* __restrict__ ridx,        // [seg_total]
    const int64_t* __restrict__ node_start,  // [K] segment starts
    const int64_t* __restrict__ chunk_off,   // [K+1] cumulative chunks
    long long* __restrict__ hist,            // [K, F, n_bins, 2]
    int K, int F, int n_bins, int fb_size, int64_t row_stride, int f_base,
    int rows_per_wg, int direct_rows) {
  // locate (node, chunk) from blockIdx.x via binary search on chunk_off
  int wg = blockIdx.x;
  int lo = 0, hi = K;
  while (lo + 1 < hi) {
    int m = (lo + hi) >> 1;
    if (chunk_off[m] <= wg) lo = m; else hi = m;
  }
  const int node = lo;
  const int64_t chunk_in_node = wg - chunk_off[node];
  const int64_t seg_start = node_start[node];
  // rows of this chunk within the node's segment
  const int64_t row_lo = chunk_in_node * (int64_t)rows_per_wg;

  const int fb = blockIdx.y;
  const int f0 = f_base + fb * fb_size;
  const int fcount = fb_size < (F - f0) ? fb_size : (F - f0);

  {
    const int64_t node_count_e = node_start[K + node];
    if (node_count_e < (int64_t)direct_rows) {
      int64_t row_hi_e = row_lo + rows_per_wg;
      if (row_hi_e > node_count_e) row_hi_e = node_count_e;
      hist_direct_rows(bins, gpair_seg, ridx,
                       hist + ((size_t)node * F) * (size_t)n_bins * 2,
                       seg_start, row_lo, row_hi_e, row_stride, f0, fcount,
                       n_bins, threadIdx.x, blockDim.x);
      return;
    }
  }

  extern __shared__ unsigned long long lds_hist[];  // [fb_size][n_bins][2]
  // VFB==16 uses the SoA g/h-plane layout (see hist_accum_row16): zero
  // both full planes even for a partial last block.
  const int tile = (VFB == 16 ? 16 : fcount) * n_bins * 2;
  for (int i = threadIdx.x; i < tile; i += blockDim.x) lds_hist[i] = 0ull;
  __syncthreads();

  // row loop: lanes take consecutive rows -> gpair reads coalesced
  // (segment order), bin reads are per-row contiguous byte runs.
  // counts are stored at node_start[K..2K) (cat_start_count layout)
  const int64_t node_count = node_start[K + node];
  int64_t row_hi = row_lo + rows_per_wg;
  if (row_hi > node_count) row_hi = node_count;

  const int lane = threadIdx.x & (WAVE - 1);
  for (int64_t i = row_lo + threadIdx.x; i < row_hi; i += blockDim.x) {
    const int64_t seg_i = seg_start + i;
    const int2 gpi = gpair_seg[seg_i];
    const longlong2 gp = {(long long)gpi.x, (long long)gpi.y};
    const uint64_t r = (uint32_t)ridx[seg_i];
    if constexpr (VFB == 16) {
      // fb_size == 16 and row base 16B-aligned by construction.
      // Word-granular lane rotation: lane l processes its row's feature
      // words in order (l&3), (l&3)+1, ... so one wave-instruction's LDS
      // atomics spread over 4 feature groups (4x fewer same-address
      // serializations on skewed features). The rotation is done with
      // branchless selects on NAMED registers - a runtime-indexed byte
      // array would go to scratch (5x slowdown).
      hist_accum_row16(lds_hist, bins, r, row_stride, f0, n_bins, lane, gp);
    } else if constexpr (VFB == 8) {
      const uint2 packed =
          *reinterpret_cast<const uint2*>(bins + r * row_stride + f0);
      const int r2 = lane & 1;
      const uint32_t w0 = packed.x, w1 = packed.y;
      const uint32_t rw0 = r2 ? w1 : w0;  // w[(0+r2)&1]
      const uint32_t rw1 = r2 ? w0 : w1;  // w[(1+r2)&1]
      const uint32_t rws[2] = {rw0, rw1};
      #pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const uint32_t w = rws[jj];
        const int fw = ((jj + r2) & 1) * 4;
        #pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int b = (w >> (8 * kk)) & 0xFF;
          if (b != 255) {
            const int f = fw + kk;
            unsigned long long* cell =
                &lds_hist[((size_t)f * n_bins + b) * 2];
            atomicAdd(cell, (unsigned long long)gp.x);
            atomicAdd(cell + 1, (unsigned long long)gp.y);
          }
        }
      }
    } else {
      const uint8_t* rowb = bins + r * row_stride + f0;
      #pragma unroll 4
      for (int f = 0; f < fcount; ++f) {
        const int b = rowb[f];
        if (b != 255) {
          unsigned long long* cell = &lds_hist[((size_t)f * n_bins + b) * 2];
          atomicAdd(cell, (unsigned long long)gp.x);
          atomicAdd(cell + 1, (unsigned long long)gp.y);
        }
      }
    }
  }
  __syncthreads();

  // merge LDS tile into the global (interleaved [.,2]) histogram
  long long* ghist =
      hist + (((size_t)node * F + f0) * n_bins) * 2;
  if constexpr (VFB == 16) {
    // re-interleave while merging: consecutive lanes write consecutive
    // global u64s (a strided 2i/2i+1 pattern doubled global transactions)
    const int n2 = fcount * n_bins * 2;
    const int hplane = 16 * n_bins;
    for (int j = threadIdx.x; j < n2; j += blockDim.x) {
      const int cell = j >> 1;
      const int scell =
          cell ^ (n_bins == 256 ? ((cell / n_bins) & 7) : 0);
      const unsigned long long v = lds_hist[(j & 1) * hplane + scell];
      if (v) atomicAdd((unsigned long long*)&ghist[j], v);
    }
  } else {
    for (int i = threadIdx.x; i < tile; i += blockDim.x) {
      const unsigned long long v = lds_hist[i];
      if (v != 0ull) {
        atomicAdd((unsigned long long*)&ghist[i], v);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// build_histogram_multifb: multi-feature-block variant for wide matrices.
//
// At F=200 (13 blocks of 16) the baseline kernel re-reads gpair_seg (8 B)
// + ridx (4 B) per row per block: 156 B/row/depth where only 12 B are
// needed. Here ONE workgroup loops over every feature block of its range,
// keeping its R rows/thread of gradient pairs + row indices in registers
// across blocks. Occupancy is LDS-bound anyway (64 KiB tile -> 2 WGs/CU
// = 4 waves/SIMD), so up to ~128 VGPRs the caching is free.
// Same LDS tile, same lane rotation, same int64 atomics => bitwise
// identical histograms to the baseline kernel.
// ---------------------------------------------------------------------------
template <int R>  // rows cached per thread; rows_per_wg = R * HIST_THREADS
__global__ __launch_bounds__(HIST_THREADS) void build_histogram_multifb_kernel(
    const uint8_t* __restrict__ bins,        // [n_rows_total, row_stride]
    const int2* __restrict__ gpair_seg,      // [seg_total] segment order
    const int32_t* __restrict__ ridx,        // [seg_total]
    const int64_t* __restrict__ node_start,  // [K] starts, [K..2K) counts
    const int64_t* __restrict__ chunk_off,   // [K+1] cumulative chunks
    long long* __restrict__ hist,            // [K, F, n_bins, 2]
    int K, int F, int n_bins, int n_fb, int64_t row_stride, int f_base) {
  int wg = blockIdx.x;
  int lo = 0, hi = K;
  while (lo + 1 < hi) {
    int m = (lo + hi) >> 1;
    if (chunk_off[m] <= wg) lo = m; else hi = m;
  }
  const int node = lo;
  const int64_t chunk_in_node = wg - chunk_off[node];
  const int64_t seg_start = node_start[node];
  const int64_t row_lo = chunk_in_node * (int64_t)(R * HIST_THREADS);
  const int64_t node_count = node_start[K + node];
  int64_t row_hi = row_lo + (int64_t)(R * HIST_THREADS);
  if (row_hi > node_count) row_hi = node_count;

  // Cache this thread's rows once. Strided assignment (i = row_lo + tid +
  // rr*512) keeps the loads coalesced per wave; validity is a prefix in
  // rr, so the block loop can predicate on rr < nvalid.
  int2 gp_reg[R];
  uint32_t rx_reg[R];
  int nvalid = 0;
  #pragma unroll
  for (int rr = 0; rr < R; ++rr) {
    const int64_t i = row_lo + threadIdx.x + (int64_t)rr * HIST_THREADS;
    if (i < row_hi) {
      const int64_t s = seg_start + i;
      gp_reg[rr] = gpair_seg[s];
      rx_reg[rr] = (uint32_t)ridx[s];
      nvalid = rr + 1;
    }
  }

  extern __shared__ unsigned long long lds_hist[];
  const int tile_full = 16 * n_bins * 2;
  const int hplane = 16 * n_bins;
  const int lane = threadIdx.x & (WAVE - 1);
  for (int blk = 0; blk < n_fb; ++blk) {
    const int f0 = f_base + blk * 16;
    for (int i = threadIdx.x; i < tile_full; i += blockDim.x)
      lds_hist[i] = 0ull;
    __syncthreads();
    #pragma unroll
    for (int rr = 0; rr < R; ++rr) {
      if (rr < nvalid) {
        const longlong2 gp = {(long long)gp_reg[rr].x,
                              (long long)gp_reg[rr].y};
        hist_accum_row16(lds_hist, bins, (uint64_t)rx_reg[rr], row_stride,
                         f0, n_bins, lane, gp);
      }
    }
    __syncthreads();
    // merge only real features (partial last block: pad bins==255 were
    // skipped in accumulation, but hist rows past F-1 must not be touched);
    // LDS is SoA g/h planes, global stays interleaved [.,2]
    const int fcount = 16 < (F - f0) ? 16 : (F - f0);
    const int n2 = fcount * n_bins * 2;
    long long* ghist = hist + (((size_t)node * F + f0) * n_bins) * 2;
    for (int j = threadIdx.x; j < n2; j += blockDim.x) {
      const int cell = j >> 1;
      const int scell =
          cell ^ (n_bins == 256 ? ((cell / n_bins) & 7) : 0);
      const unsigned long long v = lds_hist[(j & 1) * hplane + scell];
      if (v) atomicAdd((unsigned long long*)&ghist[j], v);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// build_histogram_xcd: XCD-swizzled (chunk, block) grid for wide matrices.
//
// The multifb kernel re-fetches each row's bin lines once per feature
// block over a long window - no L2 survival. Here each (row-chunk,
// feature-block) pair is its own workgroup again, but the flat index is
// swizzled so ALL n_fb blocks of one chunk land on the SAME XCD
// (consecutive blockIdx round-robin over the 8 XCDs; stride-8 indices
// share one): the chunk's bin lines are fetched once into that XCD's L2
// and every 16 B uint4 of each 64 B line is consumed by a co-resident
// workgroup. gpair_seg/ridx re-reads hit L2 the same way (the 13 blocks
// read the same 48 KB of segment data).
// ---------------------------------------------------------------------------
template <int THREADS>
__global__ __launch_bounds__(THREADS) void build_histogram_xcd_kernel(
    const uint8_t* __restrict__ bins,        // [n_rows_total, row_stride]
    const int2* __restrict__ gpair_seg,      // [seg_total] segment order
    const int32_t* __restrict__ ridx,        // [seg_total]
    const int64_t* __restrict__ node_start,  // [K] starts, [K..2K) counts
    const int64_t* __restrict__ chunk_off,   // [K+1] cumulative chunks
    long long* __restrict__ hist,            // [K, F, n_bins, 2]
    int K, int F, int n_bins, int n_fb, int64_t row_stride, int f_base,
    int rows_per_wg, int total_chunks, int direct_rows,
    // device-limit form (nullptr: off): {K, KK, total_chunks} written by
    // plan_next_depth_kernel. K and total_chunks are then BOUNDS, excess
    // workgroups exit, and node_start is the depth's histogram meta
    // [starts K | counts K | chunk_off K+1] at true-K offsets.
    const int64_t* __restrict__ limits) {
  const int flat = blockIdx.x;
  const int octet = flat / (8 * n_fb);
  const int rem = flat % (8 * n_fb);
  const int fb = rem / 8;
  const int wg = octet * 8 + (rem % 8);  // row-chunk id
  if (limits != nullptr) {
    K = (int)limits[0];
    total_chunks = (int)limits[2];
    chunk_off = node_start + 2 * (int64_t)K;
  }
  if (wg >= total_chunks) return;        // tail of the last chunk-octet

  int lo = 0, hi = K;
  while (lo + 1 < hi) {
    int m = (lo + hi) >> 1;
    if (chunk_off[m] <= wg) lo = m; else hi = m;
  }
  const int node = lo;
  const int64_t chunk_in_node = wg - chunk_off[node];
  const int64_t seg_start = node_start[node];
  const int64_t row_lo = chunk_in_node * (int64_t)rows_per_wg;
  const int f0 = f_base + fb * 16;
  const int fcount = 16 < (F - f0) ? 16 : (F - f0);

  {
    const int64_t node_count_e = node_start[K + node];
    if (node_count_e < (int64_t)direct_rows) {
      int64_t row_hi_e = row_lo + rows_per_wg;
      if (row_hi_e > node_count_e) row_hi_e = node_count_e;
      hist_direct_rows(bins, gpair_seg, ridx,
                       hist + ((size_t)node * F) * (size_t)n_bins * 2,
                       seg_start, row_lo, row_hi_e, row_stride, f0, fcount,
                       n_bins, threadIdx.x, blockDim.x);
      return;
    }
  }

  extern __shared__ unsigned long long lds_hist[];
  const int hplane = 16 * n_bins;
  for (int i = threadIdx.x; i < 2 * hplane; i += blockDim.x)
    lds_hist[i] = 0ull;
  __syncthreads();

  const int64_t node_count = node_start[K + node];
  int64_t row_hi = row_lo + rows_per_wg;
  if (row_hi > node_count) row_hi = node_count;
  const int lane = threadIdx.x & (WAVE - 1);
  // 2-row software pipeline: both rows' random uint4 gathers are in
  // flight before either LDS-atomic burst starts (SQ_WAIT_ANY was 17x
  // SQ_BUSY with one outstanding gather per thread)
  for (int64_t i = row_lo + threadIdx.x; i < row_hi;
       i += 2 * (int64_t)blockDim.x) {
    const int64_t i2 = i + blockDim.x;
    const int64_t seg_i = seg_start + i;
    const int2 gpi = gpair_seg[seg_i];
    const uint64_t r1 = (uint32_t)ridx[seg_i];
    const uint4 p1 = *reinterpret_cast<const uint4*>(
        bins + r1 * row_stride + f0);
    const bool v2 = i2 < row_hi;
    int2 gpi2 = {0, 0};
    uint4 p2 = {0, 0, 0, 0};
    if (v2) {
      const int64_t seg_i2 = seg_start + i2;
      gpi2 = gpair_seg[seg_i2];
      const uint64_t r2 = (uint32_t)ridx[seg_i2];
      p2 = *reinterpret_cast<const uint4*>(bins + r2 * row_stride + f0);
    }
    hist_accum_packed16(lds_hist, p1, n_bins, lane,
                        {(long long)gpi.x, (long long)gpi.y});
    if (v2)
      hist_accum_packed16(lds_hist, p2, n_bins, lane,
                          {(long long)gpi2.x, (long long)gpi2.y});
  }
  __syncthreads();

  const int n2 = fcount * n_bins * 2;
  long long* ghist = hist + (((size_t)node * F + f0) * n_bins) * 2;
  for (int j = threadIdx.x; j < n2; j += blockDim.x) {
    const int cell = j >> 1;
    const int scell =
        cell ^ (n_bins == 256 ? ((cell / n_bins) & 7) : 0);
    const unsigned long long v = lds_hist[(j & 1) * hplane + scell];
    if (v) atomicAdd((unsigned long long*)&ghist[j], v);
  }
}

// ---------------------------------------------------------------------------
// find_splits: one thread per (node, feature); sequential 256-bin scan in
// the exact same FP order as the CPU torch reference (int64 -> double per
// bin, then left-to-right adds) so CPU and GPU grow identical trees.
// ---------------------------------------------------------------------------
struct SplitCand {
  double gain;
  int bin;
  int default_left;
  long long left_g;
  long long left_h;
};

__device__ inline double calc_score(double G, double H, double lam, double alpha) {
  if (alpha > 0.0) {
    double t = fabs(G) - alpha;
    G = t > 0.0 ? copysign(t, G) : 0.0;
  }
  double denom = H + lam;
  return denom > 0.0 ? G * G / denom : 0.0;
}

// One WAVE per (node, feature): 64 lanes cooperatively stage the 256-bin
// histogram into LDS (coalesced), then lane 0 runs the sequential scan
// from LDS in the exact CPU FP order. ~100x the parallelism of a
// thread-per-(k,f) scan at shallow depths, with identical numerics.
__device__ inline double calc_weight_d(double G, double H, double lam,
                                       double alpha) {
  if (alpha > 0.0) {
    double t = fabs(G) - alpha;
    G = t > 0.0 ? copysign(t, G) : 0.0;
  }
  double denom = H + lam;
  return denom > 0.0 ? -G / denom : 0.0;
}

__global__ __launch_bounds__(256) void find_splits_kf_kernel(
    long long* hist,  // [K, F, B, 2]; rows >= K_built written when deriving
    // sibling derivation (prev_hist == nullptr: off): scan slot
    // k >= K_built is parent - built sibling,
    // hist[k] = prev_hist[pslots[k-K_built]] - hist[spos[k-K_built]]
    const long long* __restrict__ prev_hist,  // [K_prev, F, B, 2] or null
    const int64_t* __restrict__ pslots, const int64_t* __restrict__ spos,
    int K_built,
    const long long* __restrict__ parent_g, const long long* __restrict__ parent_h,
    const int32_t* __restrict__ feat_bins, double scale_g, double scale_h,
    double lam, double alpha, double gamma, double mcw,
    const int8_t* __restrict__ mono,    // [F] or nullptr
    const double* __restrict__ bounds,  // [K, 2] node weight bounds
    const uint8_t* __restrict__ allowed,  // [K, F] interaction gate or null
    double* __restrict__ out_gain,     // [K, F]
    int32_t* __restrict__ out_bin,     // [K, F]
    uint8_t* __restrict__ out_dl,      // [K, F]
    long long* __restrict__ out_lg,    // [K, F]
    long long* __restrict__ out_lh,    // [K, F]
    int K, int F, int B,
    // device-limit form (nullptr: off): limits = {K_built, K, ...} and the
    // depth's scan meta [sumg K | sumh K | starts K | counts K | pslot nd |
    // spos nd] at true-K offsets, both written by plan_next_depth_kernel.
    // The K argument is then a BOUND and excess waves exit.
    const int64_t* __restrict__ limits, const int64_t* __restrict__ dmeta) {
  if (limits != nullptr) {
    K_built = (int)limits[0];
    K = (int)limits[1];
    parent_g = reinterpret_cast<const long long*>(dmeta);
    parent_h = parent_g + K;
    pslots = dmeta + 4 * (int64_t)K;
    spos = pslots + (K - K_built);
  }
  // ONE 64-lane wave per (node, feature). The per-bin left sums come
  // from an INT64 inclusive wave-scan (lane-local serial prefix over a
  // contiguous bin chunk + shfl_up scan of lane totals) - integer adds
  // are exact under any order, so the scan reassociation cannot change a
  // single bit. Each bin's gain is then an independent f64 expression of
  // its exact prefix (mirrored 1:1 by the CPU oracle, which dequantizes
  // the same int cumsum), so 64 lanes evaluate 4 bins each in parallel
  // where the previous design ran a 255-step dependent f64 chain on 2
  // lanes (52% issue-stall, and nearly histogram-sized total time).
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int waves_per_block = blockDim.x / WAVE;
  int64_t kf = (int64_t)blockIdx.x * waves_per_block + wave;
  if (kf >= (int64_t)K * F) return;
  const int k = (int)(kf / F);
  const int f = (int)(kf % F);
  const int bpl = (B + WAVE - 1) / WAVE;  // <= 4 for B <= 256
  // this lane's contiguous bin chunk, loaded once; a derived row is
  // parent - sibling, stored for the next depth (ALL B bins, and before
  // any early return: the next depth reads the row as its parent even
  // when this (node, feature) is gated off) and scanned from registers.
  // Integer subtraction is exact, so the scan sees the same int64 values
  // as a separately materialized difference.
  long long vg[4], vh[4];
  {
    const size_t row = (size_t)F * B * 2;
    const size_t fo = (size_t)f * B * 2;
    const bool derive = prev_hist != nullptr && k >= K_built;
    const longlong2* src = (const longlong2*)(hist + (size_t)k * row + fo);
    const longlong2* par = nullptr;
    longlong2* dst = nullptr;
    if (derive) {
      const int j = k - K_built;
      par = (const longlong2*)(prev_hist + (size_t)pslots[j] * row + fo);
      src = (const longlong2*)(hist + (size_t)spos[j] * row + fo);
      dst = (longlong2*)(hist + (size_t)k * row + fo);
    }
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      vg[j] = 0;
      vh[j] = 0;
      const int b = lane * bpl + j;
      if (j < bpl && b < B) {
        longlong2 v = src[b];
        if (derive) {
          const longlong2 p = par[b];
          v.x = p.x - v.x;
          v.y = p.y - v.y;
          dst[b] = v;
        }
        vg[j] = v.x;
        vh[j] = v.y;
      }
    }
  }
  if (allowed != nullptr && allowed[kf] == 0) {
    // interaction constraints: disallowed (node, feature) -> the same
    // no-split sentinel the CPU oracle produces (gain -1, dl 0)
    if (lane == 0) {
      out_gain[kf] = -1.0;
      out_bin[kf] = 0;
      out_dl[kf] = 0;
      out_lg[kf] = 0;
      out_lh[kf] = 0;
    }
    return;
  }
  const double inv_g = 1.0 / scale_g;
  const double inv_h = 1.0 / scale_h;
  const int nb = feat_bins[f];

  // lane-local inclusive prefixes over this lane's contiguous bin chunk
  long long lpg[4], lph[4];
  long long gsum = 0, hsum = 0;
  #pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < bpl) {
      gsum += vg[j];
      hsum += vh[j];
      lpg[j] = gsum;
      lph[j] = hsum;
    }
  }
  // inclusive wave-scan of lane totals -> exclusive offset per lane
  long long gscan = gsum, hscan = hsum;
  #pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const long long ug = __shfl_up(gscan, d, WAVE);
    const long long uh = __shfl_up(hscan, d, WAVE);
    if (lane >= d) {
      gscan += ug;
      hscan += uh;
    }
  }
  const long long goff = gscan - gsum;   // exclusive prefix offset
  const long long hoff = hscan - hsum;
  const long long Gtot_q = __shfl(gscan, WAVE - 1, WAVE);
  const long long Htot_q = __shfl(hscan, WAVE - 1, WAVE);

  const double Gp = (double)parent_g[k] * inv_g;
  const double Hp = (double)parent_h[k] * inv_h;
  const double parent_score = calc_score(Gp, Hp, lam, alpha);
  const double Gmiss = Gp - (double)Gtot_q * inv_g;
  const double Hmiss = Hp - (double)Htot_q * inv_h;
  const long long Gmiss_q = parent_g[k] - Gtot_q;
  const long long Hmiss_q = parent_h[k] - Htot_q;

  const int c = (mono != nullptr) ? mono[f] : 0;
  double blo = 0.0, bup = 0.0;
  if (c != 0) {
    blo = bounds[(size_t)k * 2];
    bup = bounds[(size_t)k * 2 + 1];
  }

  // candidate ordering = CPU oracle order: gain desc, then dl=1 before
  // dl=0 (strictly-greater replacement across the two passes), then
  // lowest bin (ascending scan, strictly-greater replacement)
  SplitCand best = {-1.0, 0x7fffffff, -1, 0, 0};
  #pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j >= bpl) break;
    const int b = lane * bpl + j;
    if (b >= nb - 1 || b >= B) continue;
    const long long GLq = goff + lpg[j];
    const long long HLq = hoff + lph[j];
    const double GLd = (double)GLq * inv_g;
    const double HLd = (double)HLq * inv_h;
    #pragma unroll
    for (int dl = 1; dl >= 0; --dl) {
      const double gl = dl ? GLd + Gmiss : GLd;
      const double hl = dl ? HLd + Hmiss : HLd;
      const double gr = Gp - gl, hr = Hp - hl;
      if (hl < mcw || hr < mcw) continue;
      if (c != 0) {
        double wl = calc_weight_d(gl, hl, lam, alpha);
        double wr = calc_weight_d(gr, hr, lam, alpha);
        wl = fmin(fmax(wl, blo), bup);
        wr = fmin(fmax(wr, blo), bup);
        if (c > 0 ? (wl > wr) : (wl < wr)) continue;
      }
      const double gain = 0.5 * (calc_score(gl, hl, lam, alpha) +
                                 calc_score(gr, hr, lam, alpha) -
                                 parent_score) -
                          gamma;
      const bool take =
          (gain > best.gain) ||
          (gain == best.gain &&
           (dl > best.default_left ||
            (dl == best.default_left && b < best.bin)));
      if (take) {
        best.gain = gain;
        best.bin = b;
        best.default_left = dl;
        best.left_g = dl ? GLq + Gmiss_q : GLq;
        best.left_h = dl ? HLq + Hmiss_q : HLq;
      }
    }
  }

  // wave argmax reduction with the same comparator
  #pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    const double og = __shfl_down(best.gain, off, WAVE);
    const int ob = __shfl_down(best.bin, off, WAVE);
    const int odl = __shfl_down(best.default_left, off, WAVE);
    const long long olg = __shfl_down(best.left_g, off, WAVE);
    const long long olh = __shfl_down(best.left_h, off, WAVE);
    const bool take =
        (og > best.gain) ||
        (og == best.gain &&
         (odl > best.default_left ||
          (odl == best.default_left && ob < best.bin)));
    if (take) {
      best.gain = og;
      best.bin = ob;
      best.default_left = odl;
      best.left_g = olg;
      best.left_h = olh;
    }
  }
  if (lane != 0) return;
  if (best.gain <= -1.0) {
    // no-split sentinel keeps the CPU contract (gain -1, dl 0, bin 0)
    best.bin = 0;
    best.default_left = 0;
    best.left_g = 0;
    best.left_h = 0;
  }
  out_gain[kf] = best.gain;
  out_bin[kf] = best.bin;
  out_dl[kf] = (uint8_t)best.default_left;
  out_lg[kf] = best.left_g;
  out_lh[kf] = best.left_h;
}

// packs the per-node best split into ONE int64 [K, 6] row:
// (f32 gain bits, feature, bin, default_left, left_g, left_h) so the
// driver retrieves the whole depth's splits with a single D2H copy
// (dozens of tiny pageable copies per depth were the training loop's
// dominant host-side cost).
__global__ void find_splits_reduce_kernel(
    const double* __restrict__ kf_gain, const int32_t* __restrict__ kf_bin,
    const uint8_t* __restrict__ kf_dl, const long long* __restrict__ kf_lg,
    const long long* __restrict__ kf_lh,
    long long* __restrict__ out_packed,  // [K, 6]
    int K, int F) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  double bg = -1.0;
  int bf = -1, bb = 0, bdl = 0;
  long long blg = 0, blh = 0;
  // CPU semantics: dl=1 candidates evaluated first over all (f,b), dl=0
  // overrides only with strictly greater gain. Within one dl, first
  // occurrence (lowest feature) wins ties.
  for (int want_dl = 1; want_dl >= 0; --want_dl) {
    for (int f = 0; f < F; ++f) {
      int64_t kf = (int64_t)k * F + f;
      if ((int)kf_dl[kf] != want_dl) continue;
      if (kf_gain[kf] > bg) {
        bg = kf_gain[kf];
        bf = f; bb = kf_bin[kf]; bdl = want_dl;
        blg = kf_lg[kf]; blh = kf_lh[kf];
      }
    }
  }
  long long* row = out_packed + (size_t)k * 6;
  float gf = (float)bg;
  row[0] = (long long)(int)__float_as_int(gf);
  row[1] = bf;
  row[2] = bb;
  row[3] = bdl;
  row[4] = blg;
  row[5] = blh;
}

// ---------------------------------------------------------------------------
// partition_rows: stable two-pass partition of each node's ridx segment.
// Pass 1 counts left-rows per 256-row block; host does a cumsum; pass 2
// scatters with an in-block ballot prefix. Stability preserved because
// blocks are processed in segment order and lanes in row order.
// ---------------------------------------------------------------------------
#define PART_THREADS 256
#define PART_ROWS_PER_THREAD 8
#define PART_CHUNK (PART_THREADS * PART_ROWS_PER_THREAD)
#define PART_WAVES (PART_THREADS / WAVE)

// Pass 1: evaluate the split predicate ONCE per row (a ~64B cache-line
// gather from the binned matrix), cache it as one flag byte per row, and
// count per-256-row-block lefts. Pass 2 then re-reads 1 B/row instead of
// repeating the gather - halves the partition's memory cost.
// meta layout (both modes): [starts Ks | counts Ks | chunk_off Ks+1 |
// feat Ks | bin Ks | dl Ks]. Legacy: Ks = K (host-staged meta),
// limits == nullptr. Device mode: limits = {n_split, total_chunks}
// written by plan_partition_kernel; grids are BOUNDS and excess
// workgroups exit here.
__global__ void partition_count_kernel(
    const uint8_t* __restrict__ bins, const int32_t* __restrict__ ridx,
    const int64_t* __restrict__ meta,
    const int64_t* __restrict__ limits,  // nullptr or [2]
    int32_t* __restrict__ block_counts,  // [total_chunks]
    uint8_t* __restrict__ flags,         // [n] go-left per segment position
    int K, int64_t row_stride,
    const uint8_t* __restrict__ bins_T,  // [F, n] column-major copy or null
    int64_t n_rows_total) {
  int wg = blockIdx.x;
  int64_t Ks = K;
  if (limits != nullptr) {
    if (wg >= limits[1]) return;
    Ks = limits[0];
  }
  const int64_t* node_start = meta;            // starts, counts at [Ks..2Ks)
  const int64_t* chunk_off = meta + 2 * Ks;
  const int64_t* split_feat = meta + 3 * Ks + 1;
  const int64_t* split_bin = meta + 4 * Ks + 1;
  const int64_t* default_left = meta + 5 * Ks + 1;
  int lo = 0, hi = (int)Ks;
  while (lo + 1 < hi) {
    int m = (lo + hi) >> 1;
    if (chunk_off[m] <= wg) lo = m; else hi = m;
  }
  const int node = lo;
  const int64_t chunk_in_node = wg - chunk_off[node];
  const int64_t row_lo = chunk_in_node * PART_CHUNK;
  const int64_t count = node_start[Ks + node];
  const int64_t seg_start = node_start[node];
  const int feat = (int)split_feat[node], sbin = (int)split_bin[node];
  const int dl = (int)default_left[node];

  // preload all stripes' row indices + bin gathers so 8 independent
  // random-latency loads are in flight per thread (the kernel was 86%
  // memory-parked at one row per thread), accumulate the per-wave ballot
  // popcounts in a register, and reduce with ONE barrier at the end (the
  // per-stripe sync ping-pong serialized the old 4-stripe version).
  uint8_t bv[PART_ROWS_PER_THREAD];
  bool valid[PART_ROWS_PER_THREAD];
  // column-major copy: the gather touches a dense per-feature column
  // (ridx ascending within a segment -> near-sequential lines) instead
  // of one 64 B row-major line per row (64x the line traffic).
  const uint8_t* colbase =
      bins_T ? bins_T + (int64_t)feat * n_rows_total : nullptr;
  #pragma unroll
  for (int sstripe = 0; sstripe < PART_ROWS_PER_THREAD; ++sstripe) {
    const int64_t i = row_lo + sstripe * PART_THREADS + threadIdx.x;
    valid[sstripe] = i < count;
    uint64_t r = valid[sstripe] ? (uint32_t)ridx[seg_start + i] : 0;
    bv[sstripe] = colbase ? colbase[r]
                          : bins[r * (uint64_t)row_stride + feat];
  }
  __shared__ int wave_sums[PART_WAVES];
  const int wave_id = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  int wsum = 0;
  #pragma unroll
  for (int sstripe = 0; sstripe < PART_ROWS_PER_THREAD; ++sstripe) {
    const int64_t i = row_lo + sstripe * PART_THREADS + threadIdx.x;
    bool flag = false;
    if (valid[sstripe]) {
      const int b = bv[sstripe];
      flag = (b == 255) ? (dl != 0) : (b <= sbin);
      flags[seg_start + i] = flag ? 1 : 0;
    }
    wsum += __popcll(__ballot(flag));
  }
  if (lane == 0) wave_sums[wave_id] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int w = 0; w < PART_WAVES; ++w) total += wave_sums[w];
    block_counts[wg] = total;
  }
}


// Per-node exclusive prefix of per-chunk left counts, on device: one WG
// per node walks its chunk range in 256-wide blocks with an LDS
// Hillis-Steele scan. Replaces a 100 KB D2H pull + host loop + 200 KB
// H2D push per depth (and their stream syncs) with one kernel and a
// K-element total pull.
__global__ void partition_prefix_kernel(
    const int32_t* __restrict__ block_counts,  // [total_chunks]
    const int64_t* __restrict__ meta,          // layout as count kernel
    const int64_t* __restrict__ limits,        // nullptr or [2]
    int64_t* __restrict__ left_before,         // [total_chunks]
    int64_t* __restrict__ node_left_total,     // [K]
    int K) {
  const int k = blockIdx.x;
  int64_t Ks = K;
  if (limits != nullptr) Ks = limits[0];
  if (k >= Ks) return;
  const int64_t* chunk_off = meta + 2 * Ks;
  const int64_t c0 = chunk_off[k], c1 = chunk_off[k + 1];
  __shared__ int64_t sc[256];
  __shared__ int64_t sc2[256];
  int64_t run = 0;
  for (int64_t base = c0; base < c1; base += 256) {
    const int nin = (int)min((int64_t)256, c1 - base);
    const int64_t v =
        threadIdx.x < nin ? (int64_t)block_counts[base + threadIdx.x] : 0;
    sc[threadIdx.x] = v;
    __syncthreads();
    // inclusive Hillis-Steele scan over 256 entries (LDS ping-pong)
    int64_t* src = sc;
    int64_t* dst = sc2;
    for (int off = 1; off < 256; off <<= 1) {
      const int64_t x = src[threadIdx.x];
      dst[threadIdx.x] =
          threadIdx.x >= off ? x + src[threadIdx.x - off] : x;
      __syncthreads();
      int64_t* t = src; src = dst; dst = t;
    }
    if (threadIdx.x < nin)
      left_before[base + threadIdx.x] = run + src[threadIdx.x] - v;
    run += src[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) node_left_total[k] = run;
}

// Same outputs from a wave shuffle scan: each of the 4 waves scans its 64
// chunk counts with __shfl_up, one 4-entry LDS step carries the wave
// totals across - two barriers per 256 chunks instead of nine. Workgroups
// past the split-node count write a 0 left total, so the caller needs no
// zero fill of node_left_total. int64 throughout, like the LDS version.
__global__ __launch_bounds__(PART_THREADS) void partition_prefix_shfl_kernel(
    const int32_t* __restrict__ block_counts,  // [total_chunks]
    const int64_t* __restrict__ meta,          // layout as count kernel
    const int64_t* __restrict__ limits,        // nullptr or [2]
    int64_t* __restrict__ left_before,         // [total_chunks]
    int64_t* __restrict__ node_left_total,     // [K]
    int K) {
  const int k = blockIdx.x;
  int64_t Ks = K;
  if (limits != nullptr) Ks = limits[0];
  if (k >= Ks) {
    if (threadIdx.x == 0 && k < K) node_left_total[k] = 0;
    return;
  }
  const int64_t* chunk_off = meta + 2 * Ks;
  const int64_t c0 = chunk_off[k], c1 = chunk_off[k + 1];
  __shared__ int64_t wave_tot[PART_WAVES];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave_id = threadIdx.x / WAVE;
  int64_t run = 0;
  for (int64_t base = c0; base < c1; base += PART_THREADS) {
    const int nin = (int)min((int64_t)PART_THREADS, c1 - base);
    const int64_t v =
        (int)threadIdx.x < nin ? (int64_t)block_counts[base + threadIdx.x] : 0;
    long long incl = v;
    #pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const long long u = __shfl_up(incl, d, WAVE);
      if (lane >= d) incl += u;
    }
    if (lane == WAVE - 1) wave_tot[wave_id] = incl;
    __syncthreads();
    int64_t woff = 0, tot = 0;
    #pragma unroll
    for (int w = 0; w < PART_WAVES; ++w) {
      const int64_t t = wave_tot[w];
      if (w < wave_id) woff += t;
      tot += t;
    }
    if ((int)threadIdx.x < nin)
      left_before[base + threadIdx.x] = run + woff + incl - v;
    run += tot;
    __syncthreads();  // wave_tot is rewritten by the next block of chunks
  }
  if (threadIdx.x == 0) node_left_total[k] = run;
}

__global__ void partition_scatter_kernel(
    const uint8_t* __restrict__ flags, const int32_t* __restrict__ ridx,
    int32_t* __restrict__ ridx_out,
    const int2* __restrict__ gseg,      // segment-ordered gradient pairs
    int2* __restrict__ gseg_out,        // permuted alongside ridx
    const int64_t* __restrict__ meta,   // layout as count kernel
    const int64_t* __restrict__ limits,  // nullptr or [2]
    const int64_t* __restrict__ left_before,   // [total_chunks] excl. prefix within node
    const int64_t* __restrict__ node_left_total,  // [K]
    int K) {
  int wg = blockIdx.x;
  int64_t Ks = K;
  if (limits != nullptr) {
    if (wg >= limits[1]) return;
    Ks = limits[0];
  }
  const int64_t* node_start = meta;
  const int64_t* chunk_off = meta + 2 * Ks;
  int lo = 0, hi = (int)Ks;
  while (lo + 1 < hi) {
    int m = (lo + hi) >> 1;
    if (chunk_off[m] <= wg) lo = m; else hi = m;
  }
  const int node = lo;
  const int64_t chunk_in_node = wg - chunk_off[node];
  const int64_t row_lo = chunk_in_node * PART_CHUNK;
  const int64_t count = node_start[Ks + node];
  const int64_t seg_start = node_start[node];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave_id = threadIdx.x / WAVE;

  // Load every stripe's row data upfront (3 coalesced streams, all in
  // flight), publish every (stripe, wave) ballot popcount to LDS, ONE
  // barrier, then compute each row's exclusive left-prefix from the LDS
  // table and write. No cross-stripe serialization.
  int32_t rv[PART_ROWS_PER_THREAD];
  int2 gv[PART_ROWS_PER_THREAD];
  bool fl[PART_ROWS_PER_THREAD];
  bool valid[PART_ROWS_PER_THREAD];
  unsigned long long masks[PART_ROWS_PER_THREAD];
  __shared__ int wave_sums[PART_ROWS_PER_THREAD][PART_WAVES];
  #pragma unroll
  for (int s = 0; s < PART_ROWS_PER_THREAD; ++s) {
    const int64_t i = row_lo + s * PART_THREADS + threadIdx.x;
    valid[s] = i < count;
    rv[s] = 0;
    gv[s] = {0, 0};
    fl[s] = false;
    if (valid[s]) {
      rv[s] = ridx[seg_start + i];
      if (gseg != nullptr) gv[s] = gseg[seg_start + i];
      fl[s] = flags[seg_start + i] != 0;
    }
    masks[s] = __ballot(fl[s]);
    if (lane == 0) wave_sums[s][wave_id] = __popcll(masks[s]);
  }
  __syncthreads();

  int stripe_base = 0;  // lefts in earlier stripes of this chunk
  #pragma unroll
  for (int s = 0; s < PART_ROWS_PER_THREAD; ++s) {
    const int64_t i = row_lo + s * PART_THREADS + threadIdx.x;
    int wave_left_before = stripe_base;
    for (int w = 0; w < wave_id; ++w) wave_left_before += wave_sums[s][w];
    const int prefix_in_wave = __popcll(
        masks[s] & ((lane == 0) ? 0ull : ((~0ull) >> (64 - lane))));
    if (valid[s]) {
      // lefts strictly before row i in the whole node segment: earlier
      // chunks + earlier stripes of this chunk + this stripe's ballot
      const int64_t my_left_prefix =
          left_before[wg] + wave_left_before + prefix_in_wave;
      const int64_t pos = fl[s]
                              ? my_left_prefix
                              : node_left_total[node] + (i - my_left_prefix);
      ridx_out[seg_start + pos] = rv[s];
      if (gseg_out != nullptr) gseg_out[seg_start + pos] = gv[s];
    }
    for (int w = 0; w < PART_WAVES; ++w) stripe_base += wave_sums[s][w];
  }
}

// ---------------------------------------------------------------------------
// predict_trees: one thread per row, sequential over trees.
// ---------------------------------------------------------------------------
// Packed node: one 16-byte uint4 per node -> a tree-walk step is ONE
// vector load (vs 4 scattered loads of feat/thr/left/default_left).
// x = feature | (default_left << 30) | (is_leaf << 31)
// y = threshold bits (or leaf value bits), z = left child, w = unused.
__global__ void pack_nodes_kernel(
    const int32_t* __restrict__ feat, const float* __restrict__ thr,
    const int32_t* __restrict__ left, const uint8_t* __restrict__ default_left,
    const float* __restrict__ value, uint4* __restrict__ packed, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int f = feat[i];
  uint4 p;
  if (f < 0) {
    p.x = 0x80000000u;
    p.y = __float_as_uint(value[i]);
    p.z = 0;
  } else {
    p.x = (uint32_t)f | ((default_left[i] != 0) ? 0x40000000u : 0u);
    p.y = __float_as_uint(thr[i]);
    p.z = (uint32_t)left[i];
  }
  p.w = 0;
  packed[i] = p;
}

// R consecutive rows per thread: their tree walks interleave, so R
// independent node loads are in flight per step (the walk is L2-latency
// bound; one chain per thread leaves the memory pipe idle).
template <int R>
__global__ void predict_trees_kernel(
    const float* __restrict__ X, const uint4* __restrict__ nodes,
    const int32_t* __restrict__ tree_ptr, float* __restrict__ out,
    float tree_weight, int64_t n, int F, int T) {
  int64_t grp = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t gstride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n_grp = (n + R - 1) / R;
  for (; grp < n_grp; grp += gstride) {
    const int64_t i0 = grp * R;
    float acc[R];
    bool valid[R];
    #pragma unroll
    for (int r = 0; r < R; ++r) {
      acc[r] = 0.0f;
      valid[r] = (i0 + r) < n;
    }
    for (int t = 0; t < T; ++t) {
      const int base = tree_ptr[t];
      uint4 p[R];
      bool act[R];
      #pragma unroll
      for (int r = 0; r < R; ++r) {
        act[r] = valid[r];
        p[r] = nodes[base];
      }
      bool any = true;
      while (any) {
        any = false;
        #pragma unroll
        for (int r = 0; r < R; ++r) {
          if (!act[r]) continue;
          if (p[r].x & 0x80000000u) {
            acc[r] += __uint_as_float(p[r].y);
            act[r] = false;
          } else {
            const float v = X[(i0 + r) * (int64_t)F +
                              (p[r].x & 0x3FFFFFFFu)];
            const bool goleft =
                isnan(v) ? ((p[r].x & 0x40000000u) != 0)
                         : (v < __uint_as_float(p[r].y));
            p[r] = nodes[base + (int)p[r].z + (goleft ? 0 : 1)];
            any = true;
          }
        }
      }
    }
    #pragma unroll
    for (int r = 0; r < R; ++r) {
      if (valid[r]) out[i0 + r] += acc[r] * tree_weight;
    }
  }
}

// ---------------------------------------------------------------------------
// update_margins: margin[ridx[seg]] += leaf_val[node]
// ---------------------------------------------------------------------------
// 8 rows per thread: the margin update is a random-line RMW per row
// (leaf rows are ~n_leaves apart in the dense margin vector); one row
// per thread left the kernel latency-parked at 3.4x the write floor.
#define MARGIN_ROWS_PER_THREAD 8
#define MARGIN_CHUNK (PART_THREADS * MARGIN_ROWS_PER_THREAD)
__global__ void update_margins_kernel(
    float* __restrict__ margin, const int32_t* __restrict__ ridx,
    const int32_t* __restrict__ ridx_b,      // second ping-pong buffer
    const int64_t* __restrict__ node_start,  // [K] + counts at [K..2K)
    const int64_t* __restrict__ chunk_off,   // [K+1]
    const int64_t* __restrict__ parity,      // [K] 0 -> ridx, 1 -> ridx_b
    const float* __restrict__ leaf_vals, int K) {
  int wg = blockIdx.x;
  int lo = 0, hi = K;
  while (lo + 1 < hi) {
    int m = (lo + hi) >> 1;
    if (chunk_off[m] <= wg) lo = m; else hi = m;
  }
  const int node = lo;
  const int64_t chunk_in_node = wg - chunk_off[node];
  const int64_t row_lo = chunk_in_node * MARGIN_CHUNK;
  const int64_t count = node_start[K + node];
  const int64_t seg_start = node_start[node];
  if (parity != nullptr && parity[node]) ridx = ridx_b;
  const float v = leaf_vals[node];
  int32_t rv[MARGIN_ROWS_PER_THREAD];
  bool valid[MARGIN_ROWS_PER_THREAD];
  #pragma unroll
  for (int s = 0; s < MARGIN_ROWS_PER_THREAD; ++s) {
    const int64_t i = row_lo + s * PART_THREADS + threadIdx.x;
    valid[s] = i < count;
    rv[s] = valid[s] ? ridx[seg_start + i] : 0;
  }
  #pragma unroll
  for (int s = 0; s < MARGIN_ROWS_PER_THREAD; ++s) {
    if (valid[s]) margin[(uint32_t)rv[s]] += v;
  }
}

// ---------------------------------------------------------------------------
// apply_tree_binned: margin[r * margin_stride] += value[leaf(r)] in ROW
// order, the leaf found by walking the finished tree over the row's own
// bin bytes (the predicate is partition_count_kernel's, so every row lands
// in the leaf the partition put it in). One coalesced pass over bins and
// margin replaces the last-level partition plus the scattered
// update_margins read-modify-write.
//   packed node (8 B): x = feature | split_bin << 16 | default_left << 24
//                          | is_leaf << 31
//                      y = left child index, or the leaf's f32 value bits
// The node table is staged into LDS when it fits ATB_LDS_NODES (depth 12 =
// 8191 nodes = 64 KB); larger trees read the same table from global memory.
// NDW > 0: the row is NDW dwords, loaded whole (coalesced 16 B loads) into
// registers held as ONE clang vector value; a level's bin byte is a
// variable-index element of that vector, which the backend turns into a
// compare/select chain over the registers (a runtime-indexed ARRAY, or a
// hand-written select chain over one, goes to scratch: the optimizer folds
// the selects back into an indexed load). NDW == 0: any row stride,
// one byte load per level from the row's already-touched lines.
// The walk is bounded by max_steps (<= n_nodes): a malformed table cannot
// spin, and a row that has not reached a leaf by then is left untouched.
// ---------------------------------------------------------------------------
#define ATB_THREADS 256
#define ATB_LDS_NODES 8192
#define ATB_LEAF 0x80000000u

// row registers: one clang vector of NV dwords (12-dword rows ride in 16)
template <int NV>
struct AtbRow {
  typedef uint32_t type __attribute__((ext_vector_type(NV)));
};

template <int NDW, int R, bool LDS_TAB>
__global__ __launch_bounds__(ATB_THREADS) void apply_tree_binned_kernel(
    const uint8_t* __restrict__ bins, const uint2* __restrict__ nodes,
    float* __restrict__ margin, int64_t n, int64_t row_stride,
    int64_t margin_stride, int n_nodes, int max_steps) {
  extern __shared__ __align__(16) uint2 atb_lds[];
  const uint2* tab = nodes;
  if (LDS_TAB) {
    for (int i = threadIdx.x; i < n_nodes; i += ATB_THREADS)
      atb_lds[i] = nodes[i];
    __syncthreads();
    tab = atb_lds;
  }
  const int64_t chunk = (int64_t)ATB_THREADS * R;
  const int64_t n_chunks = (n + chunk - 1) / chunk;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t r0 = c * chunk + threadIdx.x;
    bool valid[R];
    uint2 nd[R];
    constexpr int NV = NDW == 0 ? 1 : (NDW == 12 ? 16 : NDW);
    typename AtbRow<NV>::type w[R];
    #pragma unroll
    for (int s = 0; s < R; ++s) {
      const int64_t r = r0 + (int64_t)s * ATB_THREADS;
      valid[s] = r < n;
      if (NDW > 0) {
        const uint4* rp = reinterpret_cast<const uint4*>(
            bins + (valid[s] ? r : 0) * row_stride);
        typename AtbRow<NV>::type row = 0;
        #pragma unroll
        for (int q = 0; q < NDW / 4; ++q) {
          const uint4 v = rp[q];
          row[4 * q + 0] = v.x;
          row[4 * q + 1] = v.y;
          row[4 * q + 2] = v.z;
          row[4 * q + 3] = v.w;
        }
        w[s] = row;
      }
    }
    const uint2 root = tab[0];
    #pragma unroll
    for (int s = 0; s < R; ++s) {
      nd[s] = root;
      if (!valid[s]) nd[s].x = ATB_LEAF;  // parked: never walks or writes
    }
    for (int step = 0; step < max_steps; ++step) {
      bool any = false;
      uint32_t b[R];
      // issue every row's byte fetch before any is consumed
      #pragma unroll
      for (int s = 0; s < R; ++s) {
        const uint32_t feat = nd[s].x & 0xFFFFu;
        if (NDW > 0) {
          // variable-index vector element: the backend expands it into
          // a compare/select chain over the row's registers
          b[s] = (w[s][(feat >> 2) & (NV - 1)] >> ((feat & 3u) * 8u)) & 0xFFu;
        } else {
          b[s] = 255u;
          if (!(nd[s].x & ATB_LEAF)) {
            const int64_t r = r0 + (int64_t)s * ATB_THREADS;
            b[s] = bins[r * row_stride + feat];
          }
        }
      }
      #pragma unroll
      for (int s = 0; s < R; ++s) {
        if (nd[s].x & ATB_LEAF) continue;
        const uint32_t sbin = (nd[s].x >> 16) & 0xFFu;
        const bool dl = ((nd[s].x >> 24) & 1u) != 0;
        const bool go_left = (b[s] == 255u) ? dl : (b[s] <= sbin);
        uint32_t child = nd[s].y + (go_left ? 0u : 1u);
        // host-validated; the clamp only keeps a bad table in bounds
        child = child < (uint32_t)n_nodes ? child : 0u;
        nd[s] = tab[child];
        any = true;
      }
      if (!any) break;
    }
    #pragma unroll
    for (int s = 0; s < R; ++s) {
      const int64_t r = r0 + (int64_t)s * ATB_THREADS;
      if (valid[s] && (nd[s].x & ATB_LEAF))
        margin[r * margin_stride] += __uint_as_float(nd[s].y);
    }
  }
}

// ---------------------------------------------------------------------------
// leaf_quantile_hist: one pass of the MSB-first radix select behind the
// adaptive (exact weighted quantile) leaves of reg:quantileerror.
//   hist[leaf][digit] += W[row]  over the leaf's rows whose order-preserving
//   key matches prefix[leaf] in its top 8*pass bits.
// Same segment/chunk geometry as update_margins (one chunk = one leaf), a
// 256-bin int64 LDS histogram per chunk, non-zero bins flushed with global
// 64-bit atomics. Integer sums only -> order-free, bitwise == CPU oracle.
// LDS scheme: one sub-histogram per wave (4 x 2 KB) with plain per-lane
// LDS atomics, summed at the flush. In pass 0 the digit is sign + 7
// exponent bits, so a wave hits one or two bins; a single 2 KB histogram
// with ballot-based pre-aggregation of equal digits measured the same
// (the kernel is bound by the gathered resid/weight loads, not the
// atomics), so the simpler form is kept.
// ---------------------------------------------------------------------------
#define LQH_THREADS PART_THREADS
#define LQH_ROWS_PER_THREAD 8
#define LQH_CHUNK (LQH_THREADS * LQH_ROWS_PER_THREAD)
#define LQH_WAVES (LQH_THREADS / WAVE)

__device__ __forceinline__ uint32_t lqh_key(float r) {
  r += 0.0f;  // -0.0 folds into +0.0
  const uint32_t u = __float_as_uint(r);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(LQH_THREADS) void leaf_quantile_hist_kernel(
    const float* __restrict__ resid,         // [n] residuals (by row id)
    const int64_t* __restrict__ weight,      // [n] integer weights or null
    const int32_t* __restrict__ ridx, const int32_t* __restrict__ ridx_b,
    const int64_t* __restrict__ node_start,  // [K] + counts at [K..2K)
    const int64_t* __restrict__ chunk_off,   // [K+1]
    const int64_t* __restrict__ parity,      // [K] or null
    const int64_t* __restrict__ prefix,      // [K] top 8*pass key bits
    long long* __restrict__ hist,            // [K,256] accumulated into
    int K, int pass) {
  __shared__ unsigned long long lds[LQH_WAVES * 256];
  for (int i = threadIdx.x; i < LQH_WAVES * 256; i += LQH_THREADS)
    lds[i] = 0ull;
  int wg = blockIdx.x;
  int lo = 0, hi = K;
  while (lo + 1 < hi) {
    int m = (lo + hi) >> 1;
    if (chunk_off[m] <= wg) lo = m; else hi = m;
  }
  const int node = lo;
  const int64_t chunk_in_node = wg - chunk_off[node];
  const int64_t row_lo = chunk_in_node * LQH_CHUNK;
  const int64_t count = node_start[K + node];
  const int64_t seg_start = node_start[node];
  if (parity != nullptr && parity[node]) ridx = ridx_b;
  const uint32_t pfx = (uint32_t)prefix[node];
  const int hi_shift = 32 - 8 * pass;  // bits above the digit (32 in pass 0)
  const int lo_shift = 24 - 8 * pass;
  __syncthreads();

  int32_t rv[LQH_ROWS_PER_THREAD];
  bool valid[LQH_ROWS_PER_THREAD];
  #pragma unroll
  for (int s = 0; s < LQH_ROWS_PER_THREAD; ++s) {
    const int64_t i = row_lo + s * LQH_THREADS + threadIdx.x;
    valid[s] = i < count;
    rv[s] = valid[s] ? ridx[seg_start + i] : 0;
  }
  unsigned long long* my = lds + (threadIdx.x / WAVE) * 256;
  #pragma unroll
  for (int s = 0; s < LQH_ROWS_PER_THREAD; ++s) {
    if (!valid[s]) continue;
    const uint32_t key = lqh_key(resid[(uint32_t)rv[s]]);
    if (pass != 0 && (key >> hi_shift) != pfx) continue;
    // the weight is gathered only for rows that pass the prefix test
    const unsigned long long w =
        weight != nullptr ? (unsigned long long)weight[(uint32_t)rv[s]]
                          : 1ull;
    if (w != 0ull) atomicAdd(&my[(key >> lo_shift) & 255u], w);
  }
  __syncthreads();
  {
    const int b = threadIdx.x;  // LQH_THREADS == 256 bins
    unsigned long long v = lds[b];
    #pragma unroll
    for (int wv = 1; wv < LQH_WAVES; ++wv) v += lds[wv * 256 + b];
    if (v != 0ull)
      atomicAdd((unsigned long long*)&hist[(size_t)node * 256 + b], v);
  }
}

// ---------------------------------------------------------------------------
// lambdarank_grad: pairwise LambdaRank gradients, one workgroup per query
// group; each thread owns docs i = tid, tid+256, ... and loops all other
// docs j sequentially, so per-doc accumulation order is fixed ->
// deterministic across runs (no atomics). NDCG variant weights each pair
// by |delta NDCG| from precomputed ranks + idcg.
// ---------------------------------------------------------------------------
__global__ void lambdarank_kernel(
    const float* __restrict__ margin, const float* __restrict__ label,
    const int64_t* __restrict__ group_ptr,  // [G+1]
    const int32_t* __restrict__ rank,       // [n] rank within group
    const double* __restrict__ idcg,        // [G] (ndcg mode) or nullptr
    float2* __restrict__ out,               // [n] (grad, hess)
    int use_ndcg) {
  const int g = blockIdx.x;
  const int64_t s0 = group_ptr[g], s1 = group_ptr[g + 1];
  const int len = (int)(s1 - s0);
  const double inv_idcg =
      (use_ndcg && idcg[g] > 0.0) ? 1.0 / idcg[g] : 0.0;
  if (use_ndcg && inv_idcg == 0.0) {
    for (int i = threadIdx.x; i < len; i += blockDim.x)
      out[s0 + i] = make_float2(0.f, 0.f);
    return;
  }
  for (int i = threadIdx.x; i < len; i += blockDim.x) {
    const float yi = label[s0 + i];
    const float mi = margin[s0 + i];
    const double gain_i = use_ndcg ? (exp2((double)yi) - 1.0) : 0.0;
    const double disc_i =
        use_ndcg ? 1.0 / log2((double)rank[s0 + i] + 2.0) : 0.0;
    double gacc = 0.0, hacc = 0.0;
    for (int j = 0; j < len; ++j) {
      const float yj = label[s0 + j];
      if (yj == yi) continue;
      const float mj = margin[s0 + j];
      double w = 1.0;
      if (use_ndcg) {
        const double gain_j = exp2((double)yj) - 1.0;
        const double disc_j = 1.0 / log2((double)rank[s0 + j] + 2.0);
        w = fabs((gain_i - gain_j) * (disc_i - disc_j)) * inv_idcg;
      }
      if (yi > yj) {
        // i should rank above j: pair (i, j)
        const double rho = 1.0 / (1.0 + exp((double)(mi - mj)));
        double hij = rho * (1.0 - rho);
        if (hij < 1e-16) hij = 1e-16;
        gacc += -rho * w;
        hacc += hij * w;
      } else {
        // j should rank above i: pair (j, i), i is the loser
        const double rho = 1.0 / (1.0 + exp((double)(mj - mi)));
        double hij = rho * (1.0 - rho);
        if (hij < 1e-16) hij = 1e-16;
        gacc += rho * w;
        hacc += hij * w;
      }
    }
    out[s0 + i] = make_float2((float)gacc, (float)hacc);
  }
}

// ---------------------------------------------------------------------------
// Gradient-based row sampling (minimal-variance sampling; the contract is
// in docs/parity.md "Gradient-based sampling"). Everything that decides
// WHICH rows are kept is integer arithmetic, so these kernels are
// array_equal to the ops.cpu oracles:
//   mvs_score   c = isqrt(rne((g^2 + 0.1 h^2) * sv)), c in [0, 2^30]
//   mvs_stats   (#{c > 0}, max c, sum c)
//   mvs_hist    one MSB-first radix pass: per digit (count, sum c)
//   mvs_sample  keep mask + reweighted pairs from (S, M) and a counter hash
// Rows are read in identity order (coalesced, no gather). Every launch
// covers exactly its rows: one row per thread (score, sample) or one
// MVS_CHUNK per workgroup (stats, hist); no address depends on a gradient
// value beyond `digit & 255`.
// ---------------------------------------------------------------------------
#define MVS_THREADS 256
#define MVS_ROWS_PER_THREAD 16
#define MVS_CHUNK (MVS_THREADS * MVS_ROWS_PER_THREAD)
#define MVS_WAVES (MVS_THREADS / WAVE)
#define MVS_VMAX (1ll << 60)

__global__ __launch_bounds__(MVS_THREADS) void mvs_score_kernel(
    const float2* __restrict__ gpair, uint32_t* __restrict__ c, double sv,
    int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * MVS_THREADS + threadIdx.x;
  if (i >= n) return;
  const float2 gp = gpair[i];
  const double g = (double)gp.x, h = (double)gp.y;
  // float32 squares are exact in float64; no contraction (build flag)
  const double v = g * g + 0.1 * (h * h);
  const double x = v * sv;
  long long V = MVS_VMAX;  // "not < 2^60" includes NaN
  if (x < (double)MVS_VMAX) V = llrint(x);
  if (V < 0) V = 0;
  // integer square root: start from the float one, then correct, so the
  // result does not depend on how sqrt (or the int64 -> double step) rounds
  long long r = (long long)sqrt((double)V);
  for (int it = 0; it < 4 && r * r > V; ++it) --r;
  for (int it = 0; it < 4 && (r + 1) * (r + 1) <= V; ++it) ++r;
  c[i] = (uint32_t)r;
}

__device__ __forceinline__ unsigned long long mvs_shfl_down_u64(
    unsigned long long v, int off) {
  return (unsigned long long)__shfl_down((long long)v, off, WAVE);
}

// partials[block] = (#{c > 0}, max c, sum c) of the block's chunk; one
// mvs_stats_fold_kernel block folds them (no same-address global atomics,
// as in quantize_gpair_kernel)
__global__ __launch_bounds__(MVS_THREADS) void mvs_stats_kernel(
    const uint32_t* __restrict__ c, int64_t n,
    unsigned long long* __restrict__ partials) {  // [gridDim.x, 3]
  const int64_t row_lo = (int64_t)blockIdx.x * MVS_CHUNK;
  unsigned long long nz = 0ull, mx = 0ull, sum = 0ull;
  #pragma unroll
  for (int s = 0; s < MVS_ROWS_PER_THREAD; ++s) {
    const int64_t i = row_lo + s * MVS_THREADS + threadIdx.x;
    if (i < n) {
      const unsigned long long v = c[i];
      nz += v != 0ull;
      mx = v > mx ? v : mx;
      sum += v;
    }
  }
  #pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    nz += mvs_shfl_down_u64(nz, off);
    const unsigned long long o = mvs_shfl_down_u64(mx, off);
    mx = o > mx ? o : mx;
    sum += mvs_shfl_down_u64(sum, off);
  }
  __shared__ unsigned long long part[MVS_WAVES][3];
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    part[threadIdx.x / WAVE][0] = nz;
    part[threadIdx.x / WAVE][1] = mx;
    part[threadIdx.x / WAVE][2] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < MVS_WAVES; ++w) {
      nz += part[w][0];
      mx = part[w][1] > mx ? part[w][1] : mx;
      sum += part[w][2];
    }
    partials[3 * (size_t)blockIdx.x] = nz;
    partials[3 * (size_t)blockIdx.x + 1] = mx;
    partials[3 * (size_t)blockIdx.x + 2] = sum;
  }
}

// one block: stats = fold of partials [n_blocks, 3]
__global__ __launch_bounds__(MVS_THREADS) void mvs_stats_fold_kernel(
    const unsigned long long* __restrict__ partials, int64_t n_blocks,
    unsigned long long* __restrict__ stats) {
  unsigned long long nz = 0ull, mx = 0ull, sum = 0ull;
  for (int64_t i = threadIdx.x; i < n_blocks; i += MVS_THREADS) {
    nz += partials[3 * i];
    const unsigned long long o = partials[3 * i + 1];
    mx = o > mx ? o : mx;
    sum += partials[3 * i + 2];
  }
  #pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    nz += mvs_shfl_down_u64(nz, off);
    const unsigned long long o = mvs_shfl_down_u64(mx, off);
    mx = o > mx ? o : mx;
    sum += mvs_shfl_down_u64(sum, off);
  }
  __shared__ unsigned long long part[MVS_WAVES][3];
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    part[threadIdx.x / WAVE][0] = nz;
    part[threadIdx.x / WAVE][1] = mx;
    part[threadIdx.x / WAVE][2] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < MVS_WAVES; ++w) {
      nz += part[w][0];
      mx = part[w][1] > mx ? part[w][1] : mx;
      sum += part[w][2];
    }
    stats[0] = nz;
    stats[1] = mx;
    stats[2] = sum;
  }
}

// hist[digit] += (1, c) over the rows whose top 8*pass bits equal pfx;
// digit = the next 8 bits. One (count, sum) LDS sub-histogram per wave,
// non-zero bins flushed with 64-bit global atomics (integer: order-free)
// into copy blockIdx.x % n_slots of the histogram, which spreads the
// same-address atomics of the early passes (a whole chunk shares a few
// digits there); mvs_hist_fold_kernel adds the copies up.
#define MVS_HIST_SLOTS 32
__global__ __launch_bounds__(MVS_THREADS) void mvs_hist_kernel(
    const uint32_t* __restrict__ c, int64_t n, uint32_t pfx, int pass,
    unsigned long long* __restrict__ slots, int n_slots) {  // [n_slots, 512]
  unsigned long long* hist = slots + (size_t)(blockIdx.x % n_slots) * 512;
  __shared__ unsigned long long lds[MVS_WAVES * 512];
  for (int i = threadIdx.x; i < MVS_WAVES * 512; i += MVS_THREADS)
    lds[i] = 0ull;
  const int hi_shift = 32 - 8 * pass;  // bits above the digit (32 in pass 0)
  const int lo_shift = 24 - 8 * pass;
  const int64_t row_lo = (int64_t)blockIdx.x * MVS_CHUNK;
  __syncthreads();
  unsigned long long* my = lds + (threadIdx.x / WAVE) * 512;
  #pragma unroll
  for (int s = 0; s < MVS_ROWS_PER_THREAD; ++s) {
    const int64_t i = row_lo + s * MVS_THREADS + threadIdx.x;
    if (i >= n) continue;
    const uint32_t v = c[i];
    if (pass != 0 && (v >> hi_shift) != pfx) continue;
    const uint32_t d = (v >> lo_shift) & 255u;
    atomicAdd(&my[2 * d], 1ull);
    if (v != 0u) atomicAdd(&my[2 * d + 1], (unsigned long long)v);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 512; b += MVS_THREADS) {
    unsigned long long v = lds[b];
    #pragma unroll
    for (int wv = 1; wv < MVS_WAVES; ++wv) v += lds[wv * 512 + b];
    if (v != 0ull) atomicAdd(&hist[b], v);
  }
}

// one block: hist[b] = sum over the n_slots copies, b in [0, 512)
__global__ __launch_bounds__(512) void mvs_hist_fold_kernel(
    const unsigned long long* __restrict__ slots, int n_slots,
    unsigned long long* __restrict__ hist) {
  const int b = threadIdx.x;
  unsigned long long v = 0ull;
  for (int s = 0; s < n_slots; ++s) v += slots[(size_t)s * 512 + b];
  hist[b] = v;
}

__device__ __forceinline__ unsigned long long mvs_splitmix64(
    unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// keep row i iff c > 0 and (S == 0 or c*M >= S or u*S < (c*M) * 2^32),
// u = splitmix64(key + i) >> 32. floor(u*S / 2^32) < c*M is that 128-bit
// comparison (the low 32 bits of u*S cannot lift it past a multiple of
// 2^32). A row kept with p < 1 is scaled by S / (c*M) in float64.
__global__ __launch_bounds__(MVS_THREADS) void mvs_sample_kernel(
    const float2* __restrict__ gpair, const uint32_t* __restrict__ c,
    unsigned long long S, unsigned long long M, unsigned long long key,
    uint8_t* __restrict__ keep, float2* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * MVS_THREADS + threadIdx.x;
  if (i >= n) return;
  const unsigned long long ci = c[i];
  const float2 gp = gpair[i];
  float2 o = make_float2(0.f, 0.f);
  uint8_t k = 0;
  if (ci != 0ull) {
    const unsigned long long cm = ci * M;
    if (S == 0ull || cm >= S) {
      k = 1;
      o = gp;
    } else {
      const unsigned long long u =
          mvs_splitmix64(key + (unsigned long long)i) >> 32;
      const unsigned long long q = (__umul64hi(u, S) << 32) | ((u * S) >> 32);
      if (q < cm) {
        k = 1;
        const double f = (double)(long long)S / (double)(long long)cm;
        o.x = (float)((double)gp.x * f);
        o.y = (float)((double)gp.y * f);
      }
    }
  }
  keep[i] = k;
  out[i] = o;
}

// ===========================================================================
// Host-side launchers / bindings
// ===========================================================================

static torch::Tensor make_chunk_off_cpu(const torch::Tensor& counts_cpu,
                                        int64_t rows_per_chunk,
                                        int64_t* total) {
  const int64_t K = counts_cpu.size(0);
  auto off = torch::zeros({K + 1}, torch::kInt64);
  auto acc = off.accessor<int64_t, 1>();
  auto cacc = counts_cpu.accessor<int64_t, 1>();
  for (int64_t k = 0; k < K; ++k) {
    acc[k + 1] = acc[k] + (cacc[k] + rows_per_chunk - 1) / rows_per_chunk;
  }
  *total = acc[K];
  return off;
}

static torch::Tensor cat_start_count(const torch::Tensor& starts_cpu,
                                     const torch::Tensor& counts_cpu,
                                     torch::Device dev) {
  // layout used by kernels: [0..K) starts, [K..2K) counts
  return torch::cat({starts_cpu, counts_cpu}).to(dev);
}

torch::Tensor quantize_gpair(torch::Tensor gpair, double scale_g, double scale_h) {
  TORCH_CHECK(on_gpu(gpair) && gpair.dtype() == torch::kFloat32);
  auto out = torch::empty_like(gpair, gpair.options().dtype(torch::kInt32));
  int64_t n = gpair.size(0);
  if (n == 0) return out;
  auto stream = c10::hip::getCurrentHIPStream();
  int64_t blocks = std::min<int64_t>(ceil_div(n, QUANT_THREADS), 8192);
  hipLaunchKernelGGL(quantize_gpair_kernel<false>, dim3(blocks),
                     dim3(QUANT_THREADS), 0, stream.stream(),
                     (const float2*)gpair.data_ptr<float>(),
                     (int2*)out.data_ptr<int32_t>(), scale_g, scale_h, n,
                     (long long*)nullptr);
  return out;
}

// quantize_gpair that also returns int64 [2] = out.sum(0) (device).
std::vector<torch::Tensor> quantize_gpair_sums(torch::Tensor gpair,
                                               double scale_g,
                                               double scale_h) {
  TORCH_CHECK(on_gpu(gpair) && gpair.dtype() == torch::kFloat32);
  TORCH_CHECK(gpair.is_contiguous() && gpair.dim() == 2 && gpair.size(1) == 2,
              "quantize_gpair_sums: gpair must be contiguous [n, 2]");
  auto out = torch::empty_like(gpair, gpair.options().dtype(torch::kInt32));
  auto optsl = gpair.options().dtype(torch::kInt64);
  int64_t n = gpair.size(0);
  if (n == 0) return {out, torch::zeros({2}, optsl)};
  auto sums = torch::empty({2}, optsl);
  auto stream = c10::hip::getCurrentHIPStream();
  int64_t blocks = std::min<int64_t>(ceil_div(n, QUANT_THREADS), 8192);
  auto partials = torch::empty({blocks, 2}, optsl);
  hipLaunchKernelGGL(quantize_gpair_kernel<true>, dim3(blocks),
                     dim3(QUANT_THREADS), 0, stream.stream(),
                     (const float2*)gpair.data_ptr<float>(),
                     (int2*)out.data_ptr<int32_t>(), scale_g, scale_h, n,
                     reinterpret_cast<long long*>(
                         partials.data_ptr<int64_t>()));
  hipLaunchKernelGGL(reduce_pair_partials_kernel, dim3(1),
                     dim3(QUANT_THREADS), 0, stream.stream(),
                     reinterpret_cast<const long long*>(
                         partials.data_ptr<int64_t>()),
                     (int)blocks,
                     reinterpret_cast<long long*>(sums.data_ptr<int64_t>()));
  return {out, sums};
}

torch::Tensor bin_matrix(torch::Tensor values, torch::Tensor cuts_flat,
                         torch::Tensor cut_ptr) {
  TORCH_CHECK(on_gpu(values) && values.dim() == 2);
  int64_t n = values.size(0);
  int F = (int)values.size(1);
  // padded allocation: 16B-aligned row stride, pad bytes = 255 (missing)
  // so the vectorized histogram path can read whole uint4 feature blocks
  int64_t F_pad = ((int64_t)F + 15) / 16 * 16;
  auto full = torch::full({n, F_pad}, 255,
                          values.options().dtype(torch::kUInt8));
  auto out = full.narrow(1, 0, F);
  if (n == 0) return out;
  int total_cuts = (int)cuts_flat.size(0);
  auto stream = c10::hip::getCurrentHIPStream();
  int64_t blocks = std::min<int64_t>(ceil_div(n * F, 256), 16384);
  size_t lds = (size_t)total_cuts * sizeof(float);
  if (lds <= 64 * 1024) {
    hipLaunchKernelGGL((bin_matrix_kernel<true>), dim3(blocks), dim3(256), lds,
                       stream.stream(), values.data_ptr<float>(),
                       full.data_ptr<uint8_t>(), cuts_flat.data_ptr<float>(),
                       cut_ptr.data_ptr<int64_t>(), n, F, total_cuts, F_pad);
  } else {
    hipLaunchKernelGGL((bin_matrix_kernel<false>), dim3(blocks), dim3(256), 0,
                       stream.stream(), values.data_ptr<float>(),
                       full.data_ptr<uint8_t>(), cuts_flat.data_ptr<float>(),
                       cut_ptr.data_ptr<int64_t>(), n, F, total_cuts, F_pad);
  }
  return out;
}


// ---------------------------------------------------------------------------
// Pinned staging: pageable H2D/D2H around every per-depth launch blocks the
// host in the driver's staging path. Each call site owns a cached pinned
// buffer; an event guards against overwriting a buffer whose async H2D is
// still in flight (can happen in the chunked-overlap histogram path where
// several builds are enqueued back-to-back with no intervening sync).
// ---------------------------------------------------------------------------
struct PinnedStager {
  torch::Tensor buf;
  hipEvent_t ev = nullptr;
  bool pending = false;
  torch::Tensor get(int64_t n, torch::Dtype dt = torch::kInt64) {
    if (pending) {
      (void)hipEventSynchronize(ev);
      pending = false;
    }
    if (!buf.defined() || buf.numel() < n || buf.scalar_type() != dt) {
      int64_t cap = 4096;
      while (cap < n) cap *= 2;
      buf = torch::empty({cap},
                         torch::TensorOptions().dtype(dt).pinned_memory(true));
    }
    return buf.narrow(0, 0, n);
  }
  void mark(hipStream_t s) {
    if (!ev) (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    (void)hipEventRecord(ev, s);
    pending = true;
  }
};

// cat into a pinned stager view. The view's length MUST equal the summed
// input length: torch::cat_out resizes a mismatched output, and the
// resized allocation is pageable — silently defeating the pinned staging
// (and flooding stderr with Resize.cpp warnings). Checked, not assumed.
static void cat_into_pinned(torch::Tensor out,
                            std::vector<torch::Tensor> parts) {
  int64_t total = 0;
  for (auto& p : parts) total += p.numel();
  TORCH_CHECK(out.numel() == total, "pinned stager size mismatch: have ",
              out.numel(), " need ", total);
  TORCH_CHECK(out.is_pinned(), "stager buffer lost pinning");
  torch::cat_out(out, parts);
}

// Histogram kernel flavour and its geometry for one launch: decided from
// the matrix layout, the feature range, the built-node count and the
// RXGB_HIST_* knobs. Shared by build_histogram and the whole-tree enqueue,
// which must agree on rows_per_wg with the device-planned chunk offsets.
struct HistConfig {
  int64_t row_stride;
  bool vec16;       // 16-byte-aligned row stride, n_bins <= 256
  int fb;           // requested feature-block size (RXGB_HIST_FB)
  bool multifb;     // register-cached block-sweep kernel
  bool xcd;         // XCD-swizzled co-resident grid (default, >= 2 blocks)
  int rows_per_wg;
  int xcd_threads;
  int direct_rows;
  int mfb_r;
};

static HistConfig hist_config(const torch::Tensor& bins, int64_t n_bins,
                              int64_t f_lo, int64_t f_hi, int K) {
  HistConfig hc;
  hc.row_stride = bins.stride(0);
  hc.vec16 = (hc.row_stride % 16 == 0) && n_bins <= 256;
  hc.fb = 16;
  if (const char* e = getenv("RXGB_HIST_FB")) {
    if (atoi(e) == 8) hc.fb = 8;
  }
  const int n_fb_pre =
      hc.vec16 ? (int)ceil_div(f_hi - f_lo, (int64_t)hc.fb) : 1;
  // multifb: one WG sweeps all feature blocks with register-cached
  // gpairs/ridx (see kernel comment). Default on for multi-block ranges;
  // RXGB_HIST_MULTIFB=0 disables, RXGB_HIST_MULTIFB_R in {8,16,32}.
  // any multi-block range: with the SoA LDS layout + interleaved merge
  // it wins at 2 blocks too (HIGGS 8.18 vs 8.31 ms/round) and by 11% at
  // 13 blocks (100M x 200: 138.7 vs 155.6 ms/round at R=8).
  bool multifb = hc.vec16 && hc.fb == 16 && n_fb_pre >= 2;
  if (const char* e = getenv("RXGB_HIST_MULTIFB")) {
    if (atoi(e) == 0) multifb = false;
  }
  // Default mode for multi-block ranges: XCD-swizzled co-resident grid
  // (hist 102 -> 56 ms at 100M x 200; HIGGS 8.31 -> 7.25 ms/round).
  // RXGB_HIST_MODE=multifb selects the register-cached block-sweep
  // variant instead; =base the original (chunk, block) 2-D grid.
  bool xcd_mode = multifb;
  if (const char* e = getenv("RXGB_HIST_MODE")) {
    if (strcmp(e, "multifb") == 0) xcd_mode = false;
    else if (strcmp(e, "base") == 0) { xcd_mode = false; multifb = false; }
  }
  if (xcd_mode) multifb = false;
  hc.multifb = multifb;
  hc.xcd = xcd_mode;
  // depth-aware chunk size: large frontiers (deep depths) have small
  // per-node segments where 8192-row chunks load-balance better
  // (measured d12 6.81 vs 6.84 ms/round); shallow depths keep 16384
  // (fewer LDS tile merges per node; 16384 won the 100M sweep)
  int xcd_rows = K >= 512 ? 8192 : 16384;
  if (const char* e = getenv("RXGB_HIST_XCD_ROWS")) {
    int v = atoi(e);
    if (v >= 512 && v <= 65536) xcd_rows = v;
  }
  // R=8 (4096 rows/WG) measured best at 100M x 200: finer chunks load-
  // balance deep depths better than R=16/32, and occupancy is LDS-bound.
  // tiny-node threshold for the direct-to-global path. Default OFF:
  // measured on HIGGS-11Mx28 depth 12, direct=512/1024/2048 gave
  // 11.84/12.14/12.88 ms/round vs 11.65 with the LDS route - the
  // skip-if-zero merge already makes empty tiles cheap, and the direct
  // path's global-atomic latency is not hidden at 256-thread occupancy.
  // Kept as an env knob for wider matrices / other shapes.
  hc.direct_rows = 0;
  if (const char* e = getenv("RXGB_HIST_DIRECT_ROWS")) {
    int v = atoi(e);
    if (v >= 0 && v <= 65536) hc.direct_rows = v;
  }
  hc.mfb_r = 8;
  if (const char* e = getenv("RXGB_HIST_MULTIFB_R")) {
    int v = atoi(e);
    if (v == 4 || v == 8 || v == 16 || v == 32) hc.mfb_r = v;
  }
  hc.rows_per_wg = multifb ? hc.mfb_r * HIST_THREADS
                   : xcd_mode ? xcd_rows
                              : HIST_ROWS_PER_WG;
  // 1024-thread WGs double waves/SIMD (2 WGs/CU within 160 KB LDS
  // either way) and win on huge matrices (100M: hist 55.6 -> 53.9 ms)
  // but lose ~3% on 11M-row shapes (deep-depth tail waste), so gate on
  // matrix size; RXGB_HIST_XCD_THREADS=512/1024 overrides.
  hc.xcd_threads = bins.size(0) > (int64_t)32 * 1024 * 1024 ? 1024 : 512;
  if (const char* e = getenv("RXGB_HIST_XCD_THREADS")) {
    int v = atoi(e);
    if (v == 512 || v == 1024) hc.xcd_threads = v;
  }
  return hc;
}

// One launch of build_histogram_xcd_kernel over feature range [f_lo, F) of
// a 16-byte-stride matrix. `limits` null: K/total_chunks exact, meta =
// starts|counts at [0, 2K) and chunk_off separate; non-null: bounds, and
// `meta` is the device-planned histogram meta (chunk_off ignored).
static void launch_hist_xcd(const HistConfig& hc, const torch::Tensor& bins,
                            const int2* gpair_seg, const int32_t* ridx,
                            const int64_t* meta, const int64_t* chunk_off,
                            long long* hist, int K, int n_bins, int f_lo,
                            int f_hi, int64_t total_chunks,
                            const int64_t* limits, hipStream_t stream) {
  const int F = (int)bins.size(1);
  const int n_fb = (int)ceil_div(f_hi - f_lo, 16);
  const size_t lds = (size_t)16 * n_bins * 2 * sizeof(long long);
  const int64_t grid = ceil_div(total_chunks, 8) * 8 * (int64_t)n_fb;
  if (grid == 0) return;
  auto launch_xcd = [&](auto tc) {
    hipLaunchKernelGGL((build_histogram_xcd_kernel<decltype(tc)::value>),
                       dim3((uint32_t)grid), dim3(decltype(tc)::value), lds,
                       stream, bins.data_ptr<uint8_t>(), gpair_seg, ridx, meta,
                       chunk_off, hist, K, F, n_bins, n_fb, hc.row_stride,
                       f_lo, hc.rows_per_wg, (int)total_chunks,
                       hc.direct_rows, limits);
  };
  if (hc.xcd_threads == 512)
    launch_xcd(std::integral_constant<int, 512>{});
  else
    launch_xcd(std::integral_constant<int, 1024>{});
}

torch::Tensor build_histogram(torch::Tensor bins, torch::Tensor gpair_q,
                              torch::Tensor ridx, torch::Tensor starts,
                              torch::Tensor counts, int64_t n_bins,
                              int64_t f_lo, int64_t f_hi,
                              torch::Tensor hist, bool pregathered) {
  // builds features [f_lo, f_hi) into the caller-provided [K, F, n_bins, 2]
  // histogram (zeroed by the caller); ranges let the driver overlap the
  // RCCL AllReduce of one feature block with the build of the next.
  TORCH_CHECK(on_gpu(bins) && bins.dtype() == torch::kUInt8);
  const int K = (int)starts.size(0);
  const int F = (int)bins.size(1);
  auto dev = bins.device();
  if (K == 0) return hist;
  auto starts_cpu = starts.to(torch::kCPU).to(torch::kInt64);
  auto counts_cpu = counts.to(torch::kCPU).to(torch::kInt64);

  // feature-block config decides the kernel flavor, which decides the
  // row-chunk size, so resolve it before computing chunk offsets.
  const HistConfig hc = hist_config(bins, n_bins, f_lo, f_hi, K);
  const int64_t row_stride0 = hc.row_stride;
  const bool vec16_pre = hc.vec16;
  const int fb_pre = hc.fb;
  const bool multifb = hc.multifb, xcd_mode = hc.xcd;
  const int direct_rows = hc.direct_rows, mfb_r = hc.mfb_r;
  const int rows_per_wg = hc.rows_per_wg;

  int64_t total_chunks = 0;
  auto chunk_off_cpu =
      make_chunk_off_cpu(counts_cpu, rows_per_wg, &total_chunks);
  if (total_chunks == 0) return hist;

  // gather gpairs into segment order once (coalesced hist reads)
  auto starts_acc = starts_cpu.accessor<int64_t, 1>();
  auto counts_acc = counts_cpu.accessor<int64_t, 1>();
  // Segments are contiguous [start, start+count) spans of ridx; gather the
  // covering range [min_start, max_end) in one kernel.
  int64_t min_start = INT64_MAX, max_end = 0;
  for (int k = 0; k < K; ++k) {
    min_start = std::min(min_start, starts_acc[k]);
    max_end = std::max(max_end, starts_acc[k] + counts_acc[k]);
  }
  if (min_start == INT64_MAX) { min_start = 0; max_end = 0; }
  auto stream = c10::hip::getCurrentHIPStream();
  int64_t span = max_end - min_start;
  TORCH_CHECK(gpair_q.dtype() == torch::kInt32,
              "gpair_q must be int32 packed pairs");
  torch::Tensor gpair_seg;
  if (pregathered) {
    // gpair_q is ALREADY in segment order aligned with ridx (the
    // partition scatter permutes it) - no gather pass needed
    gpair_seg = gpair_q;
    min_start = 0;
  } else {
    gpair_seg = torch::empty({std::max<int64_t>(span, 1), 2},
                             gpair_q.options());
    if (span > 0) {
      int64_t blocks = std::min<int64_t>(ceil_div(span, 256), 8192);
      hipLaunchKernelGGL(gather_gpair_kernel, dim3(blocks), dim3(256), 0,
                         stream.stream(),
                         (const int2*)gpair_q.data_ptr<int32_t>(),
                         ridx.data_ptr<int32_t>() + min_start,
                         (int2*)gpair_seg.data_ptr<int32_t>(), span);
    }
  }
  // ONE H2D copy for all control data: [starts_adj(K) | counts(K) |
  // chunk_off(K+1)] - tiny pageable copies around kernel launches were
  // the training loop's dominant host cost.
  auto starts_adj = starts_cpu - min_start;
  static thread_local PinnedStager hist_meta_stager;
  auto meta_cpu = hist_meta_stager.get(3 * K + 1);
  cat_into_pinned(meta_cpu, {starts_adj, counts_cpu, chunk_off_cpu});
  auto meta = meta_cpu.to(dev, /*non_blocking=*/true);
  hist_meta_stager.mark(stream.stream());
  int64_t* mp = meta.data_ptr<int64_t>();
  int64_t* sc_adj_p = mp;          // starts at [0..K), counts at [K..2K)
  int64_t* chunk_off_p = mp + 2 * K;

  // feature-block size: fit the LDS tile (fb * n_bins * 16 B) within the
  // 64 KiB dynamic-LDS default so two workgroups co-reside per CU.
  // Padded (16B-aligned row stride) matrices take the vectorized path:
  // fb = 16 features per uint4 row load.
  const int64_t row_stride = row_stride0;
  const bool vec16 = vec16_pre;
  int fb_size = vec16
                    ? 16
                    : (int)std::min<int64_t>(F, (64 * 1024) / (n_bins * 16));
  if (fb_size < 1) fb_size = 1;
  // experiment knob: RXGB_HIST_FB=8 halves the LDS tile (4 workgroups/CU
  // instead of 2) at the cost of 2x gradient re-reads per depth
  if (vec16 && fb_pre == 8) fb_size = 8;
  TORCH_CHECK(f_lo % fb_size == 0 && f_lo < f_hi && f_hi <= F,
              "feature range must align to the block size ", fb_size);
  const int n_fb = (int)ceil_div(f_hi - f_lo, fb_size);
  const size_t lds = (size_t)fb_size * n_bins * 2 * sizeof(long long);

  // ridx pointer offset so seg indices align with gpair_seg
  if (xcd_mode) {
    launch_hist_xcd(hc, bins, (const int2*)gpair_seg.data_ptr<int32_t>(),
                    ridx.data_ptr<int32_t>() + min_start, sc_adj_p,
                    chunk_off_p,
                    reinterpret_cast<long long*>(hist.data_ptr<int64_t>()), K,
                    (int)n_bins, (int)f_lo, (int)f_hi, total_chunks, nullptr,
                    stream.stream());
  } else if (multifb) {
    auto launch_mfb = [&](auto rc) {
      hipLaunchKernelGGL((build_histogram_multifb_kernel<decltype(rc)::value>),
                         dim3((uint32_t)total_chunks), dim3(HIST_THREADS),
                         lds, stream.stream(), bins.data_ptr<uint8_t>(),
                         (const int2*)gpair_seg.data_ptr<int32_t>(),
                         ridx.data_ptr<int32_t>() + min_start, sc_adj_p,
                         chunk_off_p,
                         reinterpret_cast<long long*>(hist.data_ptr<int64_t>()),
                         K, F, (int)n_bins, n_fb, row_stride, (int)f_lo);
    };
    if (mfb_r == 4)
      launch_mfb(std::integral_constant<int, 4>{});
    else if (mfb_r == 16)
      launch_mfb(std::integral_constant<int, 16>{});
    else if (mfb_r == 32)
      launch_mfb(std::integral_constant<int, 32>{});
    else
      launch_mfb(std::integral_constant<int, 8>{});
  } else if (vec16 && fb_size == 8) {
    hipLaunchKernelGGL((build_histogram_kernel<8>),
                       dim3((uint32_t)total_chunks, n_fb),
                       dim3(HIST_THREADS), lds, stream.stream(),
                       bins.data_ptr<uint8_t>(),
                       (const int2*)gpair_seg.data_ptr<int32_t>(),
                       ridx.data_ptr<int32_t>() + min_start,
                       sc_adj_p, chunk_off_p,
                       reinterpret_cast<long long*>(hist.data_ptr<int64_t>()),
                       K, F, (int)n_bins, fb_size, row_stride, (int)f_lo,
                       rows_per_wg, direct_rows);
  } else if (vec16) {
    hipLaunchKernelGGL((build_histogram_kernel<16>),
                       dim3((uint32_t)total_chunks, n_fb),
                       dim3(HIST_THREADS), lds, stream.stream(),
                       bins.data_ptr<uint8_t>(),
                       (const int2*)gpair_seg.data_ptr<int32_t>(),
                       ridx.data_ptr<int32_t>() + min_start,
                       sc_adj_p, chunk_off_p,
                       reinterpret_cast<long long*>(hist.data_ptr<int64_t>()),
                       K, F, (int)n_bins, fb_size, row_stride, (int)f_lo,
                       rows_per_wg, direct_rows);
  } else {
    hipLaunchKernelGGL((build_histogram_kernel<0>),
                       dim3((uint32_t)total_chunks, n_fb),
                       dim3(HIST_THREADS), lds, stream.stream(),
                       bins.data_ptr<uint8_t>(),
                       (const int2*)gpair_seg.data_ptr<int32_t>(),
                       ridx.data_ptr<int32_t>() + min_start,
                       sc_adj_p, chunk_off_p,
                       reinterpret_cast<long long*>(hist.data_ptr<int64_t>()),
                       K, F, (int)n_bins, fb_size, row_stride, (int)f_lo,
                       rows_per_wg, direct_rows);
  }
  return hist;
}

using OptTensor = c10::optional<torch::Tensor>;

// The (node, feature) scan: launches find_splits_kf_kernel and returns
// {kf_gain, kf_bin, kf_dl, kf_lg, kf_lh}, each [K*F]. With prev_hist /
// pslots[nd] / spos[nd] given, the last nd rows of hist are derived
// in-kernel as prev_hist[pslots] - hist[spos] (spos < K - nd) and stored.
std::vector<torch::Tensor> find_splits_kf(
    torch::Tensor hist, torch::Tensor parent_g, torch::Tensor parent_h,
    torch::Tensor feat_bins, double scale_g, double scale_h, double lam,
    double alpha, double gamma, double mcw, torch::Tensor mono,
    torch::Tensor bounds, torch::Tensor allowed, OptTensor prev_hist,
    OptTensor pslots, OptTensor spos, OptTensor limits, OptTensor dmeta) {
  const int K = (int)hist.size(0);
  const int F = (int)hist.size(1);
  const int B = (int)hist.size(2);
  auto dev = hist.device();
  const long long* prev_p = nullptr;
  const int64_t* pslots_p = nullptr;
  const int64_t* spos_p = nullptr;
  const int64_t* limits_p = nullptr;
  const int64_t* dmeta_p = nullptr;
  int K_built = K;
  if (limits.has_value()) {
    // device-limit form: hist.size(0) bounds the frontier; node sums and
    // the sibling map come from dmeta, parent_g/parent_h/pslots/spos are
    // not read. prev_hist (when given) must hold every parent slot.
    TORCH_CHECK(dmeta.has_value() && on_gpu(*limits) && on_gpu(*dmeta) &&
                    limits->scalar_type() == torch::kInt64 &&
                    dmeta->scalar_type() == torch::kInt64 &&
                    limits->numel() >= 3 && dmeta->is_contiguous() &&
                    dmeta->numel() >= 5 * (int64_t)K,
                "find_splits: limits form needs device int64 limits[3] and "
                "dmeta[>= 5K]");
    limits_p = limits->data_ptr<int64_t>();
    dmeta_p = dmeta->data_ptr<int64_t>();
    if (prev_hist.has_value()) {
      TORCH_CHECK(prev_hist->is_contiguous() && prev_hist->dim() == 4 &&
                      prev_hist->size(1) == F && prev_hist->size(2) == B &&
                      prev_hist->scalar_type() == torch::kInt64 &&
                      prev_hist->data_ptr() != hist.data_ptr(),
                  "find_splits: prev_hist must be contiguous int64 "
                  "[*, F, B, 2] and must not alias hist");
      prev_p =
          reinterpret_cast<const long long*>(prev_hist->data_ptr<int64_t>());
    }
  } else if (prev_hist.has_value() && pslots.has_value() &&
             pslots->numel() > 0) {
    TORCH_CHECK(spos.has_value() && spos->numel() == pslots->numel(),
                "find_splits: pslots and spos must have equal length");
    const int64_t nd = pslots->numel();
    TORCH_CHECK(nd <= K, "find_splits: more derived rows than scan slots");
    TORCH_CHECK(hist.is_contiguous() && prev_hist->is_contiguous() &&
                    prev_hist->dim() == 4 && prev_hist->size(1) == F &&
                    prev_hist->size(2) == B &&
                    prev_hist->scalar_type() == torch::kInt64,
                "find_splits: prev_hist must be contiguous int64 [*, F, B, 2]");
    TORCH_CHECK(on_gpu(*pslots) && on_gpu(*spos) &&
                    pslots->scalar_type() == torch::kInt64 &&
                    spos->scalar_type() == torch::kInt64 &&
                    pslots->is_contiguous() && spos->is_contiguous(),
                "find_splits: pslots/spos must be contiguous device int64");
    TORCH_CHECK(prev_hist->data_ptr() != hist.data_ptr(),
                "find_splits: prev_hist must not alias hist");
    prev_p = reinterpret_cast<const long long*>(prev_hist->data_ptr<int64_t>());
    pslots_p = pslots->data_ptr<int64_t>();
    spos_p = spos->data_ptr<int64_t>();
    K_built = K - (int)nd;
  }
  TORCH_CHECK(hist.is_contiguous() && hist.size(3) == 2 &&
                  reinterpret_cast<uintptr_t>(hist.data_ptr()) % 16 == 0 &&
                  (prev_p == nullptr ||
                   reinterpret_cast<uintptr_t>(prev_p) % 16 == 0),
              "find_splits: hist must be contiguous [K, F, B, 2], 16B-aligned");
  auto optsd = torch::TensorOptions().dtype(torch::kFloat64).device(dev);
  auto optsi = torch::TensorOptions().dtype(torch::kInt32).device(dev);
  auto optsl = torch::TensorOptions().dtype(torch::kInt64).device(dev);
  auto optsb = torch::TensorOptions().dtype(torch::kUInt8).device(dev);
  auto kf_gain = torch::empty({(int64_t)K * F}, optsd);
  auto kf_bin = torch::empty({(int64_t)K * F}, optsi);
  auto kf_dl = torch::empty({(int64_t)K * F}, optsb);
  auto kf_lg = torch::empty({(int64_t)K * F}, optsl);
  auto kf_lh = torch::empty({(int64_t)K * F}, optsl);
  int64_t total = (int64_t)K * F;
  if (total == 0) return {kf_gain, kf_bin, kf_dl, kf_lg, kf_lh};
  auto stream = c10::hip::getCurrentHIPStream();
  // one 64-lane wave per (k, f), four waves per 256-thread block; no LDS
  const int waves_per_block = 4;
  hipLaunchKernelGGL(find_splits_kf_kernel,
                     dim3((uint32_t)ceil_div(total, waves_per_block)),
                     dim3(waves_per_block * WAVE), 0,
                     stream.stream(),
                     reinterpret_cast<long long*>(hist.data_ptr<int64_t>()),
                     prev_p, pslots_p, spos_p, K_built,
                     reinterpret_cast<const long long*>(parent_g.data_ptr<int64_t>()),
                     reinterpret_cast<const long long*>(parent_h.data_ptr<int64_t>()),
                     feat_bins.data_ptr<int32_t>(), scale_g, scale_h, lam,
                     alpha, gamma, mcw,
                     mono.numel() ? mono.data_ptr<int8_t>() : nullptr,
                     bounds.numel() ? bounds.data_ptr<double>() : nullptr,
                     allowed.numel() ? allowed.data_ptr<uint8_t>() : nullptr,
                     kf_gain.data_ptr<double>(),
                     kf_bin.data_ptr<int32_t>(), kf_dl.data_ptr<uint8_t>(),
                     reinterpret_cast<long long*>(kf_lg.data_ptr<int64_t>()),
                     reinterpret_cast<long long*>(kf_lh.data_ptr<int64_t>()), K, F, B,
                     limits_p, dmeta_p);
  return {kf_gain, kf_bin, kf_dl, kf_lg, kf_lh};
}

static void launch_reduce(const std::vector<torch::Tensor>& kf,
                          torch::Tensor out_packed, int K, int F) {
  if (K == 0) return;
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(find_splits_reduce_kernel, dim3((uint32_t)ceil_div(K, 64)),
                     dim3(64), 0, stream.stream(), kf[0].data_ptr<double>(),
                     kf[1].data_ptr<int32_t>(), kf[2].data_ptr<uint8_t>(),
                     reinterpret_cast<const long long*>(kf[3].data_ptr<int64_t>()),
                     reinterpret_cast<const long long*>(kf[4].data_ptr<int64_t>()),
                     reinterpret_cast<long long*>(out_packed.data_ptr<int64_t>()),
                     K, F);
}

std::vector<torch::Tensor> find_splits(torch::Tensor hist, torch::Tensor parent_g,
                                       torch::Tensor parent_h,
                                       torch::Tensor feat_bins, double scale_g,
                                       double scale_h, double lam, double alpha,
                                       double gamma, double mcw,
                                       torch::Tensor mono, torch::Tensor bounds,
                                       torch::Tensor allowed, bool pull,
                                       OptTensor prev_hist, OptTensor pslots,
                                       OptTensor spos) {
  const int K = (int)hist.size(0);
  const int F = (int)hist.size(1);
  auto kf = find_splits_kf(hist, parent_g, parent_h, feat_bins, scale_g,
                           scale_h, lam, alpha, gamma, mcw, mono, bounds,
                           allowed, prev_hist, pslots, spos, c10::nullopt,
                           c10::nullopt);
  auto out_packed = torch::empty(
      {K, 6}, torch::TensorOptions().dtype(torch::kInt64).device(hist.device()));
  launch_reduce(kf, out_packed, K, F);
  if (!pull) return {out_packed};  // device [K,6]: consumed by the
                                   // fused partition (single-sync path)
  // pinned D2H: the caller consumes (copies out of) the result
  // immediately, so returning a view of the cached buffer is safe
  static thread_local PinnedStager split_out_stager;
  auto out_cpu = split_out_stager.get((int64_t)K * 6).view({K, 6});
  out_cpu.copy_(out_packed);
  return {out_cpu};
}


// ---------------------------------------------------------------------------
// plan_partition: ONE device kernel turns the depth's packed split
// results ([K,6]: f32-gain bits, feat, bin, dl, lg, lh) into the
// compacted partition metadata the partition kernels consume
// (starts|counts|chunk_off|feat|bin|dl of the SPLIT nodes only), so the
// partition can launch without the host ever seeing the splits. The
// split predicate (gain > 0, feat >= 0, finite) is bit-identical to the
// host replay's numpy predicate - both read the same f32 bits.
// Single workgroup: K <= 8192 and the work per node is trivial.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void plan_partition_kernel(
    const long long* __restrict__ packed,      // [K, 6]
    const int64_t* __restrict__ starts_ord,    // [K] scan-slot order
    const int64_t* __restrict__ counts_ord,    // [K]
    int64_t* __restrict__ meta,     // [6K+1] compacted partition meta
    int64_t* __restrict__ scalars,  // [2]: n_split, total_chunks
    int K) {
  __shared__ int64_t s_ok[1024];
  __shared__ int64_t s_ch[1024];
  const int per = (K + blockDim.x - 1) / blockDim.x;
  const int lo = threadIdx.x * per;
  const int hi = min(K, lo + per);
  // thread-local pass: ok flags + chunk counts
  int64_t my_ok = 0, my_ch = 0;
  for (int k = lo; k < hi; ++k) {
    const float gain = __int_as_float((int)packed[(size_t)k * 6]);
    const long long f = packed[(size_t)k * 6 + 1];
    const bool ok = (gain > 0.0f) && (f >= 0) && isfinite(gain);
    if (ok) {
      ++my_ok;
      my_ch += (counts_ord[k] + PART_CHUNK - 1) / PART_CHUNK;
    }
  }
  s_ok[threadIdx.x] = my_ok;
  s_ch[threadIdx.x] = my_ch;
  __syncthreads();
  // inclusive block scan (Hillis-Steele over 1024)
  for (int off = 1; off < 1024; off <<= 1) {
    int64_t a = 0, b = 0;
    if ((int)threadIdx.x >= off) {
      a = s_ok[threadIdx.x - off];
      b = s_ch[threadIdx.x - off];
    }
    __syncthreads();
    s_ok[threadIdx.x] += a;
    s_ch[threadIdx.x] += b;
    __syncthreads();
  }
  const int64_t n_split = s_ok[1023];
  const int64_t total_chunks = s_ch[1023];
  int64_t pos = s_ok[threadIdx.x] - my_ok;   // exclusive prefixes
  int64_t coff = s_ch[threadIdx.x] - my_ch;
  // meta layout (Ks = n_split): [starts Ks | counts Ks | chunk_off Ks+1
  //  | feat Ks | bin Ks | dl Ks] packed back-to-back at n_split-based
  // offsets; chunk_off tail padded with total_chunks so the kernels'
  // binary search over a BOUND-sized node range never maps a chunk to a
  // phantom node.
  int64_t* m_starts = meta;
  int64_t* m_counts = meta + n_split;
  int64_t* m_coff = meta + 2 * n_split;
  int64_t* m_feat = meta + 3 * n_split + 1;
  int64_t* m_bin = meta + 4 * n_split + 1;
  int64_t* m_dl = meta + 5 * n_split + 1;
  for (int k = lo; k < hi; ++k) {
    const float gain = __int_as_float((int)packed[(size_t)k * 6]);
    const long long f = packed[(size_t)k * 6 + 1];
    const bool ok = (gain > 0.0f) && (f >= 0) && isfinite(gain);
    if (ok) {
      m_starts[pos] = starts_ord[k];
      m_counts[pos] = counts_ord[k];
      m_coff[pos] = coff;
      m_feat[pos] = f;
      m_bin[pos] = packed[(size_t)k * 6 + 2];
      m_dl[pos] = packed[(size_t)k * 6 + 3];
      coff += (counts_ord[k] + PART_CHUNK - 1) / PART_CHUNK;
      ++pos;
    }
  }
  if (threadIdx.x == 1023) m_coff[n_split] = total_chunks;
  if (threadIdx.x == 0) {
    scalars[0] = n_split;
    scalars[1] = total_chunks;
  }
}

// find_splits_reduce_kernel + plan_partition_kernel as ONE single-
// workgroup kernel for K <= 1024 (between them the two launches were a
// serial thread walking F features twice and a 20-barrier block scan).
// Reduce: wave w takes nodes w, w+16, ...; lanes cover the features and
// keep a dl=1 and a dl=0 candidate each (strictly-greater replacement in
// ascending feature order == lowest feature wins ties, start gain -1, a
// NaN gain never compares greater); a butterfly merges the lanes by
// (gain desc, feature asc) - the order the serial loop realizes - and
// the dl=0 winner replaces the dl=1 winner only on strictly greater
// gain. Plan: thread k owns node k (what plan_partition_kernel does at
// K <= 1024), reading the reduce phase's results from LDS; the block
// scan is a wave shuffle scan plus a 16-entry carry.
#define RP_THREADS 1024
#define RP_WAVES (RP_THREADS / WAVE)
__global__ __launch_bounds__(RP_THREADS) void reduce_plan_kernel(
    const double* __restrict__ kf_gain, const int32_t* __restrict__ kf_bin,
    const uint8_t* __restrict__ kf_dl, const long long* __restrict__ kf_lg,
    const long long* __restrict__ kf_lh,
    const int64_t* __restrict__ starts_ord,  // [K] scan-slot order
    const int64_t* __restrict__ counts_ord,  // [K]
    long long* __restrict__ out_packed,      // [K, 6]
    int64_t* __restrict__ meta,     // [6K+1] compacted partition meta
    int64_t* __restrict__ scalars,  // [2]: n_split, total_chunks
    int K, int F,
    // device-limit form (nullptr: off): K = limits[1], starts/counts come
    // from the depth's scan meta (layout: find_splits_kf_kernel). K == 0
    // plans an empty partition.
    const int64_t* __restrict__ limits, const int64_t* __restrict__ dmeta) {
  if (limits != nullptr) {
    K = (int)limits[1];
    starts_ord = dmeta + 2 * (int64_t)K;
    counts_ord = dmeta + 3 * (int64_t)K;
  }
  __shared__ int s_gbits[RP_THREADS];
  __shared__ int s_feat[RP_THREADS];
  __shared__ int s_bin[RP_THREADS];
  __shared__ int s_dl[RP_THREADS];
  __shared__ long long s_wok[RP_WAVES];
  __shared__ long long s_wch[RP_WAVES];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave_id = threadIdx.x / WAVE;

  for (int k = wave_id; k < K; k += RP_WAVES) {
    double g1 = -1.0, g0 = -1.0;
    int f1 = -1, f0 = -1;
    for (int f = lane; f < F; f += WAVE) {
      const int64_t kf = (int64_t)k * F + f;
      const int dl = (int)kf_dl[kf];
      const double g = kf_gain[kf];
      if (dl == 1) {
        if (g > g1) { g1 = g; f1 = f; }
      } else if (dl == 0) {
        if (g > g0) { g0 = g; f0 = f; }
      }
    }
    #pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
      const double og1 = __shfl_xor(g1, off, WAVE);
      const int of1 = __shfl_xor(f1, off, WAVE);
      const double og0 = __shfl_xor(g0, off, WAVE);
      const int of0 = __shfl_xor(f0, off, WAVE);
      // equal gains with a candidate on both sides: lowest feature (an
      // empty side has gain -1, which a held candidate always exceeds)
      if (og1 > g1 || (og1 == g1 && of1 >= 0 && of1 < f1)) { g1 = og1; f1 = of1; }
      if (og0 > g0 || (og0 == g0 && of0 >= 0 && of0 < f0)) { g0 = og0; f0 = of0; }
    }
    if (lane == 0) {
      double bg = g1;
      int bf = f1, bdl = f1 >= 0 ? 1 : 0;
      if (g0 > bg) { bg = g0; bf = f0; bdl = 0; }
      int bb = 0;
      long long blg = 0, blh = 0;
      if (bf >= 0) {
        const int64_t kf = (int64_t)k * F + bf;
        bb = kf_bin[kf];
        blg = kf_lg[kf];
        blh = kf_lh[kf];
      }
      const int gbits = __float_as_int((float)bg);
      long long* row = out_packed + (size_t)k * 6;
      row[0] = (long long)gbits;
      row[1] = bf;
      row[2] = bb;
      row[3] = bdl;
      row[4] = blg;
      row[5] = blh;
      s_gbits[k] = gbits;
      s_feat[k] = bf;
      s_bin[k] = bb;
      s_dl[k] = bdl;
    }
  }
  __syncthreads();

  const int k = threadIdx.x;
  bool ok = false;
  long long cnt = 0, ch = 0;
  if (k < K) {
    const float gain = __int_as_float(s_gbits[k]);
    ok = (gain > 0.0f) && (s_feat[k] >= 0) && isfinite(gain);
    if (ok) {
      cnt = counts_ord[k];
      ch = (cnt + PART_CHUNK - 1) / PART_CHUNK;
    }
  }
  long long iok = ok ? 1 : 0, ich = ch;  // inclusive wave scans
  #pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const long long uo = __shfl_up(iok, d, WAVE);
    const long long uc = __shfl_up(ich, d, WAVE);
    if (lane >= d) {
      iok += uo;
      ich += uc;
    }
  }
  if (lane == WAVE - 1) {
    s_wok[wave_id] = iok;
    s_wch[wave_id] = ich;
  }
  __syncthreads();
  long long ok_off = 0, ch_off = 0, n_split = 0, total_chunks = 0;
  #pragma unroll
  for (int w = 0; w < RP_WAVES; ++w) {
    const long long a = s_wok[w], b = s_wch[w];
    if (w < wave_id) {
      ok_off += a;
      ch_off += b;
    }
    n_split += a;
    total_chunks += b;
  }
  // meta layout: see plan_partition_kernel
  if (ok) {
    const long long pos = ok_off + iok - 1;
    meta[pos] = starts_ord[k];
    meta[n_split + pos] = cnt;
    meta[2 * n_split + pos] = ch_off + ich - ch;
    meta[3 * n_split + 1 + pos] = s_feat[k];
    meta[4 * n_split + 1 + pos] = s_bin[k];
    meta[5 * n_split + 1 + pos] = s_dl[k];
  }
  if (threadIdx.x == 0) {
    meta[3 * n_split] = total_chunks;
    scalars[0] = n_split;
    scalars[1] = total_chunks;
  }
}

// ---------------------------------------------------------------------------
// plan_next_depth: depth d's split results -> depth d+1's launch metadata,
// on device, so the next depth's histogram/scan/plan kernels need nothing
// from the host. The integer transcription of the trainer's child
// bookkeeping: per split node (scan slot k, compact position pos in
// ascending-k order, the order reduce_plan_kernel compacted and the
// partition's left totals are stored in)
//   left  = (start,      lc,         lg,        lh)
//   right = (start + lc, count - lc, sumg - lg, sumh - lh)
// the child with the smaller quantized hessian sum is BUILT (tie: left),
// the other is derived as parent - built. Built children take scan slots
// [0, K'), their siblings [K', 2K') in the same order; K' = n_split.
// Outputs, at true-K' offsets (KK' = 2K'):
//   dmeta_next  [sumg KK' | sumh KK' | starts KK' | counts KK' |
//                pslot K' | spos K']          (pslot = k, spos = pos)
//   hmeta_next  [starts K' | counts K' | chunk_off K'+1]   built nodes
//   limits_next {K', KK', total histogram chunks}
// Single workgroup, thread k owns scan slot k (KK <= 1024); two wave-
// shuffle scans with a 16-entry carry, like reduce_plan_kernel. Integer
// math only. K' = 0 writes zero limits.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(RP_THREADS) void plan_next_depth_kernel(
    const long long* __restrict__ packed,         // depth d [KK, 6]
    const int64_t* __restrict__ dmeta,            // depth d scan meta
    const int64_t* __restrict__ limits,           // depth d {K, KK, chunks}
    const int64_t* __restrict__ node_left_total,  // [n_split] compact order
    int64_t* __restrict__ dmeta_next, int64_t* __restrict__ hmeta_next,
    int64_t* __restrict__ limits_next, int rows_per_wg) {
  __shared__ long long s_wok[RP_WAVES];
  __shared__ long long s_wch[RP_WAVES];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave_id = threadIdx.x / WAVE;
  const int KK = (int)limits[1];
  const int k = threadIdx.x;
  bool ok = false;
  if (k < KK) {
    const float gain = __int_as_float((int)packed[(size_t)k * 6]);
    ok = (gain > 0.0f) && (packed[(size_t)k * 6 + 1] >= 0) && isfinite(gain);
  }
  long long iok = ok ? 1 : 0;  // inclusive wave scan
  #pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const long long u = __shfl_up(iok, d, WAVE);
    if (lane >= d) iok += u;
  }
  if (lane == WAVE - 1) s_wok[wave_id] = iok;
  __syncthreads();
  long long ok_off = 0, n_split = 0;
  #pragma unroll
  for (int w = 0; w < RP_WAVES; ++w) {
    const long long a = s_wok[w];
    if (w < wave_id) ok_off += a;
    n_split += a;
  }
  const long long pos = ok_off + iok - 1;
  long long b_start = 0, b_count = 0, b_g = 0, b_h = 0;
  long long s_start = 0, s_count = 0, s_g = 0, s_h = 0;
  long long ch = 0;
  if (ok) {
    const long long sumg = dmeta[k], sumh = dmeta[KK + k];
    const long long start = dmeta[2 * (int64_t)KK + k];
    const long long count = dmeta[3 * (int64_t)KK + k];
    const long long lg = packed[(size_t)k * 6 + 4];
    const long long lh = packed[(size_t)k * 6 + 5];
    const long long lc = node_left_total[pos];
    const long long rg = sumg - lg, rh = sumh - lh;
    const bool build_left = lh <= rh;
    b_start = build_left ? start : start + lc;
    b_count = build_left ? lc : count - lc;
    b_g = build_left ? lg : rg;
    b_h = build_left ? lh : rh;
    s_start = build_left ? start + lc : start;
    s_count = build_left ? count - lc : lc;
    s_g = build_left ? rg : lg;
    s_h = build_left ? rh : lh;
    ch = (b_count + rows_per_wg - 1) / rows_per_wg;
  }
  long long ich = ch;
  #pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const long long u = __shfl_up(ich, d, WAVE);
    if (lane >= d) ich += u;
  }
  if (lane == WAVE - 1) s_wch[wave_id] = ich;
  __syncthreads();
  long long ch_off = 0, total_chunks = 0;
  #pragma unroll
  for (int w = 0; w < RP_WAVES; ++w) {
    const long long b = s_wch[w];
    if (w < wave_id) ch_off += b;
    total_chunks += b;
  }
  const long long Kn = n_split, KKn = 2 * n_split;
  if (ok) {
    dmeta_next[pos] = b_g;
    dmeta_next[Kn + pos] = s_g;
    dmeta_next[KKn + pos] = b_h;
    dmeta_next[KKn + Kn + pos] = s_h;
    dmeta_next[2 * KKn + pos] = b_start;
    dmeta_next[2 * KKn + Kn + pos] = s_start;
    dmeta_next[3 * KKn + pos] = b_count;
    dmeta_next[3 * KKn + Kn + pos] = s_count;
    dmeta_next[4 * KKn + pos] = k;
    dmeta_next[4 * KKn + Kn + pos] = pos;
    hmeta_next[pos] = b_start;
    hmeta_next[Kn + pos] = b_count;
    hmeta_next[2 * Kn + pos] = ch_off + ich - ch;
  }
  if (threadIdx.x == 0) {
    hmeta_next[3 * Kn] = total_chunks;
    limits_next[0] = Kn;
    limits_next[1] = KKn;
    limits_next[2] = total_chunks;
  }
}

// The root's metadata in the same layouts, from the device-resident
// gradient sums: one node, segment [0, n_local). Also copies the sums to
// `root_out` so they reach the host with the depth-0 pull.
__global__ void plan_root_kernel(const int64_t* __restrict__ root_sum,
                                 int64_t n_local, int rows_per_wg,
                                 int64_t* __restrict__ dmeta,
                                 int64_t* __restrict__ hmeta,
                                 int64_t* __restrict__ limits,
                                 int64_t* __restrict__ root_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t chunks = (n_local + rows_per_wg - 1) / rows_per_wg;
  dmeta[0] = root_sum[0];
  dmeta[1] = root_sum[1];
  dmeta[2] = 0;
  dmeta[3] = n_local;
  hmeta[0] = 0;
  hmeta[1] = n_local;
  hmeta[2] = 0;
  hmeta[3] = chunks;
  limits[0] = 1;
  limits[1] = 1;
  limits[2] = chunks;
  root_out[0] = root_sum[0];
  root_out[1] = root_sum[1];
}

static void launch_plan(torch::Tensor packed, torch::Tensor starts_ord,
                        torch::Tensor counts_ord, torch::Tensor meta,
                        torch::Tensor scalars, int K) {
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(plan_partition_kernel, dim3(1), dim3(1024), 0,
                     stream.stream(),
                     reinterpret_cast<const long long*>(packed.data_ptr<int64_t>()),
                     starts_ord.data_ptr<int64_t>(),
                     counts_ord.data_ptr<int64_t>(),
                     meta.data_ptr<int64_t>(), scalars.data_ptr<int64_t>(),
                     K);
}

static void check_kf(const std::vector<torch::Tensor>& kf,
                     const torch::Tensor& starts_ord,
                     const torch::Tensor& counts_ord, int* K, int* F) {
  TORCH_CHECK(kf.size() == 5, "expected kf_gain, kf_bin, kf_dl, kf_lg, kf_lh");
  *K = (int)starts_ord.numel();
  TORCH_CHECK(*K > 0 && counts_ord.numel() == *K,
              "starts_ord/counts_ord must be non-empty, equal length");
  const int64_t KF = kf[0].numel();
  TORCH_CHECK(KF > 0 && KF % *K == 0, "kf arrays must hold K*F entries");
  *F = (int)(KF / *K);
  TORCH_CHECK(kf[0].scalar_type() == torch::kFloat64 &&
                  kf[1].scalar_type() == torch::kInt32 &&
                  kf[2].scalar_type() == torch::kUInt8 &&
                  kf[3].scalar_type() == torch::kInt64 &&
                  kf[4].scalar_type() == torch::kInt64 &&
                  starts_ord.scalar_type() == torch::kInt64 &&
                  counts_ord.scalar_type() == torch::kInt64,
              "reduce+plan: wrong dtype");
  for (const auto& t : kf)
    TORCH_CHECK(on_gpu(t) && t.is_contiguous() && t.numel() == KF,
                "kf arrays must be contiguous device tensors of K*F entries");
  TORCH_CHECK(on_gpu(starts_ord) && on_gpu(counts_ord) &&
                  starts_ord.is_contiguous() && counts_ord.is_contiguous(),
              "starts_ord/counts_ord must be contiguous device tensors");
}

// Per-node best split + partition plan from the (node, feature) scan
// results. Fused: ONE single-workgroup kernel at K <= 1024 (above that
// the two legacy kernels), into a [7K] device buffer whose first 6K
// entries are `packed` and whose last K the partition fills with the
// left totals - the layout the host pulls in one copy. Returns
// {packed, meta, scalars, pullbuf}.
static std::vector<torch::Tensor> reduce_plan_impl(
    const std::vector<torch::Tensor>& kf, torch::Tensor starts_ord,
    torch::Tensor counts_ord, bool fused) {
  int K = 0, F = 0;
  check_kf(kf, starts_ord, counts_ord, &K, &F);
  auto optsl =
      torch::TensorOptions().dtype(torch::kInt64).device(kf[0].device());
  auto meta = torch::empty({6 * (int64_t)K + 2}, optsl);
  if (!fused) {
    auto packed = torch::empty({K, 6}, optsl);
    auto scalars = torch::zeros({2}, optsl);
    launch_reduce(kf, packed, K, F);
    launch_plan(packed, starts_ord, counts_ord, meta, scalars, K);
    return {packed, meta, scalars, torch::Tensor()};
  }
  auto pullbuf = torch::empty({7 * (int64_t)K}, optsl);
  auto packed = pullbuf.narrow(0, 0, 6 * (int64_t)K).view({K, 6});
  auto scalars = torch::empty({2}, optsl);  // both written by the kernel
  if (K <= RP_THREADS) {
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(reduce_plan_kernel, dim3(1), dim3(RP_THREADS), 0,
                       stream.stream(), kf[0].data_ptr<double>(),
                       kf[1].data_ptr<int32_t>(), kf[2].data_ptr<uint8_t>(),
                       reinterpret_cast<const long long*>(kf[3].data_ptr<int64_t>()),
                       reinterpret_cast<const long long*>(kf[4].data_ptr<int64_t>()),
                       starts_ord.data_ptr<int64_t>(),
                       counts_ord.data_ptr<int64_t>(),
                       reinterpret_cast<long long*>(packed.data_ptr<int64_t>()),
                       meta.data_ptr<int64_t>(), scalars.data_ptr<int64_t>(),
                       K, F, (const int64_t*)nullptr, (const int64_t*)nullptr);
  } else {
    launch_reduce(kf, packed, K, F);
    launch_plan(packed, starts_ord, counts_ord, meta, scalars, K);
  }
  return {packed, meta, scalars, pullbuf};
}

// reduce_plan_kernel in its device-limit form: K_bound (<= 1024) sizes the
// outputs, the true frontier size is limits[1] and the node segments come
// from the scan meta `dmeta`, both device-resident. The outputs keep
// K_bound-based offsets: packed rows at [6k, 6k+6), the left totals at
// pullbuf[6 * K_bound ...). Returns {packed, meta, scalars, pullbuf}.
std::vector<torch::Tensor> reduce_plan_limits(
    torch::Tensor kf_gain, torch::Tensor kf_bin, torch::Tensor kf_dl,
    torch::Tensor kf_lg, torch::Tensor kf_lh, torch::Tensor dmeta,
    torch::Tensor limits, int64_t K_bound) {
  TORCH_CHECK(K_bound >= 1 && K_bound <= RP_THREADS,
              "reduce_plan_limits: frontier bound must be in [1, 1024]");
  const int64_t KF = kf_gain.numel();
  TORCH_CHECK(KF > 0 && KF % K_bound == 0, "kf arrays must hold K_bound*F entries");
  const int F = (int)(KF / K_bound);
  TORCH_CHECK(kf_gain.scalar_type() == torch::kFloat64 &&
                  kf_bin.scalar_type() == torch::kInt32 &&
                  kf_dl.scalar_type() == torch::kUInt8 &&
                  kf_lg.scalar_type() == torch::kInt64 &&
                  kf_lh.scalar_type() == torch::kInt64 &&
                  dmeta.scalar_type() == torch::kInt64 &&
                  limits.scalar_type() == torch::kInt64,
              "reduce_plan_limits: wrong dtype");
  for (const auto& t : {kf_gain, kf_bin, kf_dl, kf_lg, kf_lh})
    TORCH_CHECK(on_gpu(t) && t.is_contiguous() && t.numel() == KF,
                "kf arrays must be contiguous device tensors of K_bound*F entries");
  TORCH_CHECK(on_gpu(dmeta) && on_gpu(limits) && dmeta.is_contiguous() &&
                  limits.numel() >= 3 && dmeta.numel() >= 4 * K_bound,
              "reduce_plan_limits: need device limits[3], dmeta[>= 4K]");
  auto optsl =
      torch::TensorOptions().dtype(torch::kInt64).device(kf_gain.device());
  auto meta = torch::empty({6 * K_bound + 2}, optsl);
  auto pullbuf = torch::empty({7 * K_bound}, optsl);
  auto packed = pullbuf.narrow(0, 0, 6 * K_bound).view({K_bound, 6});
  auto scalars = torch::empty({2}, optsl);
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(reduce_plan_kernel, dim3(1), dim3(RP_THREADS), 0,
                     stream.stream(), kf_gain.data_ptr<double>(),
                     kf_bin.data_ptr<int32_t>(), kf_dl.data_ptr<uint8_t>(),
                     reinterpret_cast<const long long*>(kf_lg.data_ptr<int64_t>()),
                     reinterpret_cast<const long long*>(kf_lh.data_ptr<int64_t>()),
                     (const int64_t*)nullptr, (const int64_t*)nullptr,
                     reinterpret_cast<long long*>(packed.data_ptr<int64_t>()),
                     meta.data_ptr<int64_t>(), scalars.data_ptr<int64_t>(),
                     (int)K_bound, F, limits.data_ptr<int64_t>(),
                     dmeta.data_ptr<int64_t>());
  return {packed, meta, scalars, pullbuf};
}

std::vector<torch::Tensor> reduce_plan_fused(
    torch::Tensor kf_gain, torch::Tensor kf_bin, torch::Tensor kf_dl,
    torch::Tensor kf_lg, torch::Tensor kf_lh, torch::Tensor starts_ord,
    torch::Tensor counts_ord) {
  auto r = reduce_plan_impl({kf_gain, kf_bin, kf_dl, kf_lg, kf_lh},
                            starts_ord, counts_ord, /*fused=*/true);
  return {r[0], r[1], r[2]};
}

std::vector<torch::Tensor> reduce_plan_legacy(
    torch::Tensor kf_gain, torch::Tensor kf_bin, torch::Tensor kf_dl,
    torch::Tensor kf_lg, torch::Tensor kf_lh, torch::Tensor starts_ord,
    torch::Tensor counts_ord) {
  auto r = reduce_plan_impl({kf_gain, kf_bin, kf_dl, kf_lg, kf_lh},
                            starts_ord, counts_ord, /*fused=*/false);
  return {r[0], r[1], r[2]};
}

// count + prefix + pull of a device-planned partition (everything but
// the plan before it and the scatter after it). `pullbuf` ([7K], packed
// in its first 6K) defined: the left totals land in its tail and ONE
// D2H brings both to the host; undefined: two copies. `fused` selects
// the shuffle-scan prefix kernel, which zeroes the unused left totals
// itself (no fill). Returns the list partition_rows_from_packed returns.
static std::vector<torch::Tensor> partition_planned(
    torch::Tensor bins, torch::Tensor ridx, torch::Tensor packed,
    torch::Tensor meta, torch::Tensor scalars, torch::Tensor pullbuf,
    torch::Tensor gseg, torch::Tensor bins_t, int64_t chunk_bound,
    torch::Tensor ridx_dest, bool fused, bool stage_pull = true) {
  const int K = (int)packed.size(0);     // frontier bound (scan-slot count)
  auto dev = bins.device();
  // ping-pong destination: the caller tracks which buffer each leaf
  // segment's rows last landed in (parity) for the margin update, so
  // no full clone is needed (the 44 MB stream-ordered copy per depth
  // serialized the loop like the gseg clone did)
  auto ridx_out = ridx_dest.numel() ? ridx_dest : ridx.clone();
  // gseg needs no clone: the scatter fully rewrites every SPLIT
  // segment, and a leaf segment's gradient pairs are never read again
  // (ridx IS read for the end-of-round leaf margin update, so it keeps
  // the clone). Saves an 88 MB device copy per depth at 11M rows.
  auto gseg_out = torch::empty_like(gseg);
  auto optsl = torch::TensorOptions().dtype(torch::kInt64).device(dev);
  auto stream = c10::hip::getCurrentHIPStream();
  int64_t* mp = meta.data_ptr<int64_t>();
  const int64_t* sc2 = scalars.data_ptr<int64_t>();
  auto block_counts = torch::empty({std::max<int64_t>(chunk_bound, 1)},
      torch::TensorOptions().dtype(torch::kInt32).device(dev));
  auto flags = torch::empty({ridx.size(0)},
      torch::TensorOptions().dtype(torch::kUInt8).device(dev));
  // device-limit form: node/chunk layout pointers are n_split-based
  // inside `meta`, discovered by each kernel from scalars[0]
  hipLaunchKernelGGL(partition_count_kernel,
                     dim3((uint32_t)std::max<int64_t>(chunk_bound, 1)),
                     dim3(PART_THREADS), 0, stream.stream(),
                     bins.data_ptr<uint8_t>(), ridx.data_ptr<int32_t>(),
                     mp, sc2, block_counts.data_ptr<int32_t>(),
                     flags.data_ptr<uint8_t>(), K, bins.stride(0),
                     bins_t.numel() ? bins_t.data_ptr<uint8_t>() : nullptr,
                     bins.size(0));
  auto left_before = torch::empty({std::max<int64_t>(chunk_bound, 1)}, optsl);
  torch::Tensor node_left_total;
  if (pullbuf.defined())
    node_left_total = pullbuf.narrow(0, 6 * (int64_t)K, K);
  else
    node_left_total = fused ? torch::empty({K}, optsl)
                            : torch::zeros({K}, optsl);
  if (fused) {
    hipLaunchKernelGGL(partition_prefix_shfl_kernel,
                       dim3((uint32_t)std::max(K, 1)), dim3(PART_THREADS), 0,
                       stream.stream(),
                       block_counts.data_ptr<int32_t>(), mp, sc2,
                       left_before.data_ptr<int64_t>(),
                       node_left_total.data_ptr<int64_t>(), K);
  } else {
    hipLaunchKernelGGL(partition_prefix_kernel,
                       dim3((uint32_t)std::max(K, 1)), dim3(256), 0,
                       stream.stream(),
                       block_counts.data_ptr<int32_t>(), mp, sc2,
                       left_before.data_ptr<int64_t>(),
                       node_left_total.data_ptr<int64_t>(), K);
  }
  // ONE async pinned D2H of everything the host replay needs -
  // enqueued BEFORE the scatter, so the host's single sync wakes as
  // soon as scan+plan+count+prefix are done and ALL its bookkeeping
  // overlaps the scatter (the first version synced past the scatter,
  // which serialized the bookkeeping after it and measured slower
  // than the 2-sync structure)
  // (stage_pull false: the whole-tree enqueue copies pullbuf into its own
  // per-depth pinned slot instead of this shared one)
  torch::Tensor pull;
  if (stage_pull) {
    static thread_local PinnedStager pull_stager;
    pull = pull_stager.get(7 * (int64_t)K);
    if (pullbuf.defined()) {
      pull.copy_(pullbuf, /*non_blocking=*/true);
    } else {
      pull.narrow(0, 0, 6 * (int64_t)K)
          .copy_(packed.view({-1}), /*non_blocking=*/true);
      pull.narrow(0, 6 * (int64_t)K, K)
          .copy_(node_left_total, /*non_blocking=*/true);
    }
    pull_stager.mark(stream.stream());
  }
  auto cb = torch::full({1}, chunk_bound, torch::kInt64);
  return {ridx_out, gseg_out, pull, meta, scalars, left_before,
          node_left_total, flags, cb};
}

// Fused scan-consume partition: find_splits' packed output feeds the
// partition directly on device; the host gets {packed | left_counts}
// in a pinned D2H it reads after a single stream sync per depth
// (replacing the 2 syncs/depth of the host-planned path). fused_glue
// drops the two zero fills and takes the shuffle-scan prefix kernel.
std::vector<torch::Tensor> partition_rows_from_packed(
    torch::Tensor bins, torch::Tensor ridx, torch::Tensor starts_ord,
    torch::Tensor counts_ord, torch::Tensor packed, torch::Tensor gseg,
    torch::Tensor bins_t, int64_t chunk_bound, torch::Tensor ridx_dest,
    bool fused_glue) {
  const int K = (int)packed.size(0);
  auto optsl =
      torch::TensorOptions().dtype(torch::kInt64).device(bins.device());
  auto meta = torch::empty({6 * (int64_t)K + 2}, optsl);
  // the plan kernel writes both scalars
  auto scalars = fused_glue ? torch::empty({2}, optsl)
                            : torch::zeros({2}, optsl);
  launch_plan(packed, starts_ord, counts_ord, meta, scalars, K);
  return partition_planned(bins, ridx, packed, meta, scalars,
                           torch::Tensor(), gseg, bins_t, chunk_bound,
                           ridx_dest, fused_glue);
}

// The same partition fed by the (node, feature) scan results of
// find_splits_kf: reduce + plan in one kernel, no fills, one pull.
std::vector<torch::Tensor> partition_rows_from_kf(
    torch::Tensor bins, torch::Tensor ridx, torch::Tensor starts_ord,
    torch::Tensor counts_ord, torch::Tensor kf_gain, torch::Tensor kf_bin,
    torch::Tensor kf_dl, torch::Tensor kf_lg, torch::Tensor kf_lh,
    torch::Tensor gseg, torch::Tensor bins_t, int64_t chunk_bound,
    torch::Tensor ridx_dest) {
  auto r = reduce_plan_impl({kf_gain, kf_bin, kf_dl, kf_lg, kf_lh},
                            starts_ord, counts_ord, /*fused=*/true);
  return partition_planned(bins, ridx, r[0], r[1], r[2], r[3], gseg, bins_t,
                           chunk_bound, ridx_dest, /*fused=*/true);
}

// Scatter phase of the device-planned partition: launched AFTER the
// caller records its pull event, so the host's event-wait wakes before
// the scatter and all bookkeeping overlaps it.
void partition_scatter_planned(
    torch::Tensor ridx, torch::Tensor ridx_out, torch::Tensor gseg,
    torch::Tensor gseg_out, torch::Tensor meta, torch::Tensor scalars,
    torch::Tensor left_before, torch::Tensor node_left_total,
    torch::Tensor flags, int64_t chunk_bound) {
  const int K = (int)node_left_total.size(0);
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(partition_scatter_kernel,
                     dim3((uint32_t)std::max<int64_t>(chunk_bound, 1)),
                     dim3(PART_THREADS), 0, stream.stream(),
                     flags.data_ptr<uint8_t>(), ridx.data_ptr<int32_t>(),
                     ridx_out.data_ptr<int32_t>(),
                     gseg.numel() ? (const int2*)gseg.data_ptr<int32_t>()
                                  : nullptr,
                     gseg_out.numel() ? (int2*)gseg_out.data_ptr<int32_t>()
                                      : nullptr,
                     meta.data_ptr<int64_t>(), scalars.data_ptr<int64_t>(),
                     left_before.data_ptr<int64_t>(),
                     node_left_total.data_ptr<int64_t>(), K);
}

void partition_scatter_from_packed(
    torch::Tensor ridx, torch::Tensor ridx_out, torch::Tensor gseg,
    torch::Tensor gseg_out, torch::Tensor meta, torch::Tensor scalars,
    torch::Tensor left_before, torch::Tensor node_left_total,
    torch::Tensor flags, torch::Tensor cb) {
  partition_scatter_planned(ridx, ridx_out, gseg, gseg_out, meta, scalars,
                            left_before, node_left_total, flags,
                            cb.item<int64_t>());
}

// Two-phase partition: `begin` launches count+prefix and returns
// immediately so the caller's host-side tree bookkeeping overlaps those
// kernels; `finish` pulls the per-node left totals (the one host sync)
// and launches the scatter (which the caller's subsequent bookkeeping
// then overlaps). partition_rows keeps the one-call form.
std::vector<torch::Tensor> partition_rows_begin(
    torch::Tensor bins, torch::Tensor ridx, torch::Tensor starts,
    torch::Tensor counts, torch::Tensor split_feat,
    torch::Tensor split_bin, torch::Tensor default_left,
    torch::Tensor gseg, torch::Tensor bins_t, bool gseg_full_rewrite) {
  const int K = (int)starts.size(0);
  auto dev = bins.device();
  auto ridx_out = ridx.clone();
  // Depthwise growth rewrites every still-live gseg segment each depth,
  // so its output needs no clone (see partition_rows_from_packed).
  // Lossguide partitions ONE node per expansion and keeps reading the
  // other candidates''' segments -> it must clone.
  auto gseg_out =
      gseg_full_rewrite ? torch::empty_like(gseg) : gseg.clone();
  auto empty_i64 = torch::zeros({K > 0 ? K : 1}, torch::kInt64);
  if (K == 0)
    return {ridx_out, gseg_out, empty_i64, empty_i64, empty_i64,
            torch::zeros({1}, torch::kInt64)};
  auto starts_cpu = starts.to(torch::kCPU).to(torch::kInt64);
  auto counts_cpu = counts.to(torch::kCPU).to(torch::kInt64);
  int64_t total_chunks = 0;
  auto chunk_off_cpu = torch::zeros({K + 1}, torch::kInt64);
  {
    auto acc = chunk_off_cpu.accessor<int64_t, 1>();
    auto cacc = counts_cpu.accessor<int64_t, 1>();
    for (int k = 0; k < K; ++k)
      acc[k + 1] = acc[k] + (cacc[k] + PART_CHUNK - 1) / PART_CHUNK;
    total_chunks = acc[K];
  }
  if (total_chunks == 0)
    return {ridx_out, gseg_out, empty_i64, empty_i64, empty_i64,
            torch::zeros({1}, torch::kInt64)};
  auto stream0 = c10::hip::getCurrentHIPStream();
  static thread_local PinnedStager part_meta_stager;
  auto meta_cpu = part_meta_stager.get(6 * K + 1);
  cat_into_pinned(meta_cpu, {starts_cpu, counts_cpu, chunk_off_cpu,
                             split_feat.to(torch::kCPU).to(torch::kInt64),
                             split_bin.to(torch::kCPU).to(torch::kInt64),
                             default_left.to(torch::kCPU).to(torch::kInt64)});
  auto meta = meta_cpu.to(dev, /*non_blocking=*/true);
  part_meta_stager.mark(stream0.stream());
  int64_t* mp = meta.data_ptr<int64_t>();

  auto stream = c10::hip::getCurrentHIPStream();
  auto block_counts = torch::empty({total_chunks},
      torch::TensorOptions().dtype(torch::kInt32).device(dev));
  auto flags = torch::empty({ridx.size(0)},
      torch::TensorOptions().dtype(torch::kUInt8).device(dev));
  hipLaunchKernelGGL(partition_count_kernel, dim3((uint32_t)total_chunks),
                     dim3(PART_THREADS), 0, stream.stream(),
                     bins.data_ptr<uint8_t>(), ridx.data_ptr<int32_t>(),
                     mp, (const int64_t*)nullptr,
                     block_counts.data_ptr<int32_t>(),
                     flags.data_ptr<uint8_t>(), K, bins.stride(0),
                     bins_t.numel() ? bins_t.data_ptr<uint8_t>() : nullptr,
                     bins.size(0));
  auto left_before = torch::empty({total_chunks},
      torch::TensorOptions().dtype(torch::kInt64).device(dev));
  auto node_left_total = torch::empty({K},
      torch::TensorOptions().dtype(torch::kInt64).device(dev));
  hipLaunchKernelGGL(partition_prefix_kernel, dim3((uint32_t)K), dim3(256),
                     0, stream0.stream(),
                     block_counts.data_ptr<int32_t>(), mp,
                     (const int64_t*)nullptr,
                     left_before.data_ptr<int64_t>(),
                     node_left_total.data_ptr<int64_t>(), K);
  auto tc = torch::full({1}, total_chunks, torch::kInt64);
  return {ridx_out, gseg_out, meta, left_before, node_left_total, tc,
          flags};
}

std::vector<torch::Tensor> partition_rows_finish(
    torch::Tensor ridx, torch::Tensor ridx_out, torch::Tensor gseg,
    torch::Tensor gseg_out, torch::Tensor meta, torch::Tensor left_before,
    torch::Tensor node_left_total, torch::Tensor tc_t,
    torch::Tensor flags) {
  const int K = (int)node_left_total.size(0);
  const int64_t total_chunks = tc_t.item<int64_t>();
  if (total_chunks == 0)
    return {ridx_out, torch::zeros({K}, torch::kInt64), gseg_out};
  auto stream = c10::hip::getCurrentHIPStream();
  static thread_local PinnedStager nl_stager;
  auto node_left_total_cpu_pin = nl_stager.get(K);
  node_left_total_cpu_pin.copy_(node_left_total);  // sync: host needs it
  auto node_left_total_cpu = node_left_total_cpu_pin.clone();
  int64_t* mp = meta.data_ptr<int64_t>();
  hipLaunchKernelGGL(partition_scatter_kernel, dim3((uint32_t)total_chunks),
                     dim3(PART_THREADS), 0, stream.stream(),
                     flags.data_ptr<uint8_t>(), ridx.data_ptr<int32_t>(),
                     ridx_out.data_ptr<int32_t>(),
                     gseg.numel() ? (const int2*)gseg.data_ptr<int32_t>()
                                  : nullptr,
                     gseg_out.numel() ? (int2*)gseg_out.data_ptr<int32_t>()
                                      : nullptr,
                     mp, (const int64_t*)nullptr,
                     left_before.data_ptr<int64_t>(),
                     node_left_total.data_ptr<int64_t>(), K);
  return {ridx_out, node_left_total_cpu, gseg_out};
}

std::vector<torch::Tensor> partition_rows(torch::Tensor bins, torch::Tensor ridx,
                                          torch::Tensor starts, torch::Tensor counts,
                                          torch::Tensor split_feat,
                                          torch::Tensor split_bin,
                                          torch::Tensor default_left,
                                          torch::Tensor gseg,
                                          torch::Tensor bins_t) {
  auto st = partition_rows_begin(bins, ridx, starts, counts, split_feat,
                                 split_bin, default_left, gseg, bins_t,
                                 /*gseg_full_rewrite=*/false);
  if (st.size() == 6) {  // K==0 / no chunks: nothing to scatter
    return {st[0], torch::zeros({(int64_t)starts.size(0)}, torch::kInt64),
            st[1]};
  }
  return partition_rows_finish(ridx, st[0], gseg, st[1], st[2], st[3],
                               st[4], st[5], st[6]);
}


// ---------------------------------------------------------------------------
// predict_trees_lds: tree-tiled serving walk. Trees are packed into
// contiguous-node TILES (<= PRED_TILE_NODES nodes, 64 KiB) that a block
// stages into LDS once per 2048-row chunk; every node access during the
// walk is then an LDS read instead of a random L1/L2 hit - the plain
// kernel is node-fetch latency bound. Rows' feature reads stay in L1
// (each row re-reads its own 1-2 lines). Falls back to the plain kernel
// for single trees deeper than the tile (host decides).
// ---------------------------------------------------------------------------
#define PRED_TILE_NODES 4096
#define PRED_ROWS_PER_THREAD 8
__global__ __launch_bounds__(256) void predict_trees_lds_kernel(
    const float* __restrict__ X, const uint4* __restrict__ nodes,
    const int32_t* __restrict__ tree_ptr,
    const int32_t* __restrict__ tile_ptr,  // [n_tiles+1] tree indices
    float* __restrict__ out, float tree_weight, int64_t n, int F, int T,
    int n_tiles) {
  __shared__ uint4 lds_nodes[PRED_TILE_NODES];
  const int64_t rows_per_chunk = (int64_t)blockDim.x * PRED_ROWS_PER_THREAD;
  const int64_t n_chunks = (n + rows_per_chunk - 1) / rows_per_chunk;
  for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const int64_t row0 = chunk * rows_per_chunk + threadIdx.x;
    float acc[PRED_ROWS_PER_THREAD];
    #pragma unroll
    for (int r = 0; r < PRED_ROWS_PER_THREAD; ++r) acc[r] = 0.0f;
    for (int tile = 0; tile < n_tiles; ++tile) {
      const int t0 = tile_ptr[tile], t1 = tile_ptr[tile + 1];
      const int nb0 = tree_ptr[t0];
      const int span = tree_ptr[t1] - nb0;
      __syncthreads();  // previous walk done before overwriting LDS
      for (int i = threadIdx.x; i < span; i += blockDim.x)
        lds_nodes[i] = nodes[nb0 + i];
      __syncthreads();
      for (int t = t0; t < t1; ++t) {
        const int rel = tree_ptr[t] - nb0;
        #pragma unroll
        for (int r = 0; r < PRED_ROWS_PER_THREAD; ++r) {
          const int64_t row = row0 + (int64_t)r * blockDim.x;
          if (row >= n) continue;
          uint4 p = lds_nodes[rel];
          while (!(p.x & 0x80000000u)) {
            const float v = X[row * (int64_t)F + (p.x & 0x3FFFFFFFu)];
            const bool goleft =
                isnan(v) ? ((p.x & 0x40000000u) != 0)
                         : (v < __uint_as_float(p.y));
            p = lds_nodes[rel + (int)p.z + (goleft ? 0 : 1)];
          }
          acc[r] += __uint_as_float(p.y);
        }
      }
    }
    #pragma unroll
    for (int r = 0; r < PRED_ROWS_PER_THREAD; ++r) {
      const int64_t row = row0 + (int64_t)r * blockDim.x;
      if (row < n) out[row] += acc[r] * tree_weight;
    }
  }
}

// RXGB_PREDICT_LDS=0 sends every tree walk to its plain (global-node)
// variant, so both variants can be exercised on small forests.
static bool predict_lds_enabled() {
  if (const char* e = getenv("RXGB_PREDICT_LDS")) return atoi(e) != 0;
  return true;
}

// Greedy tiling of a forest for the LDS tree walks: consecutive trees
// whose nodes fit `tile_nodes` share a tile; `tiles` receives the tree
// index each tile starts at (plus T). False when one tree alone exceeds
// a tile - the caller then takes its plain variant.
static bool greedy_tree_tiles(const int32_t* tp, int T, int tile_nodes,
                              std::vector<int32_t>& tiles) {
  tiles.assign(1, 0);
  int t = 0;
  while (t < T) {
    int t_end = t;
    while (t_end < T && tp[t_end + 1] - tp[t] <= tile_nodes) ++t_end;
    if (t_end == t) return false;  // one tree > tile
    tiles.push_back(t_end);
    t = t_end;
  }
  return true;
}

void predict_trees(torch::Tensor X, torch::Tensor feat, torch::Tensor thr,
                   torch::Tensor left, torch::Tensor default_left,
                   torch::Tensor value, torch::Tensor tree_ptr,
                   torch::Tensor out, double tree_weight) {
  int64_t n = X.size(0);
  int F = (int)X.size(1);
  int T = (int)tree_ptr.size(0) - 1;
  if (n == 0 || T <= 0) return;
  auto stream = c10::hip::getCurrentHIPStream();
  int64_t n_nodes = feat.size(0);
  auto packed = torch::empty({n_nodes, 4},
      torch::TensorOptions().dtype(torch::kInt32).device(X.device()));
  hipLaunchKernelGGL(pack_nodes_kernel, dim3((uint32_t)ceil_div(n_nodes, 256)),
                     dim3(256), 0, stream.stream(),
                     feat.data_ptr<int32_t>(), thr.data_ptr<float>(),
                     left.data_ptr<int32_t>(), default_left.data_ptr<uint8_t>(),
                     value.data_ptr<float>(),
                     (uint4*)packed.data_ptr<int32_t>(), n_nodes);
  // tree-tiled LDS path: pack trees into <= PRED_TILE_NODES-node tiles
  // (CPU-side scan over tree_ptr; falls back to the plain kernel when a
  // single tree exceeds the tile or when disabled)
  std::vector<int32_t> tiles;
  bool use_lds = predict_lds_enabled();
  if (use_lds) {
    auto tp_cpu = tree_ptr.to(torch::kCPU).to(torch::kInt32).contiguous();
    use_lds = greedy_tree_tiles(tp_cpu.data_ptr<int32_t>(), T,
                                PRED_TILE_NODES, tiles);
  }
  if (use_lds) {
    auto tile_t = torch::from_blob(
        tiles.data(), {(int64_t)tiles.size()},
        torch::TensorOptions().dtype(torch::kInt32)).clone().to(X.device());
    const int64_t rows_per_chunk = 256 * PRED_ROWS_PER_THREAD;
    int64_t blocks = std::min<int64_t>(
        ceil_div(n, rows_per_chunk), 8192);
    hipLaunchKernelGGL(predict_trees_lds_kernel, dim3((uint32_t)blocks),
                       dim3(256), 0, stream.stream(),
                       X.data_ptr<float>(),
                       (const uint4*)packed.data_ptr<int32_t>(),
                       tree_ptr.data_ptr<int32_t>(),
                       tile_t.data_ptr<int32_t>(),
                       out.data_ptr<float>(), (float)tree_weight, n, F, T,
                       (int)tiles.size() - 1);
    return;
  }
  // measured: R=4 ILP loses to plain TLP here (75.8 vs 94.5 M rows/s on
  // 100 trees x depth 8) - one row per thread with a full grid wins
  int64_t blocks = std::min<int64_t>(ceil_div(n, 256), 8192);
  hipLaunchKernelGGL((predict_trees_kernel<1>), dim3(blocks), dim3(256), 0,
                     stream.stream(), X.data_ptr<float>(),
                     (const uint4*)packed.data_ptr<int32_t>(),
                     tree_ptr.data_ptr<int32_t>(),
                     out.data_ptr<float>(), (float)tree_weight, n, F, T);
}

// ---------------------------------------------------------------------------
// predict_leaf / saabas_contribs: the predict_trees walk with something
// else written per step. Both reuse the packed node (its value slot is
// unused) and the greedy LDS tiling; LDS_NODES = false is the plain variant
// that reads nodes from global memory (one tile spanning the forest).
// tree_ptr arrives on the HOST and the grid covers exactly the rows of the
// launch: no cap, no grid-stride loop (the wrappers bound the rows of a
// launch). One thread owns a row from the first tree to the last, no
// atomics, no cross-lane sums: launches are bitwise repeatable.
// ---------------------------------------------------------------------------
// A forest packed and tiled for the walks: made once per op call
// (walk_pack), used by every row chunk of that call.
struct WalkForest {
  torch::Tensor packed, ptr_d, tile_d;
  int T, n_tiles, tile_nodes;
  bool lds_nodes;
};

// Checks the flat arrays against the host tree_ptr, packs the nodes and
// tiles the forest into tiles of at most `tile_nodes` nodes.
WalkForest walk_pack(torch::Tensor feat, torch::Tensor thr,
                     torch::Tensor left, torch::Tensor default_left,
                     torch::Tensor tree_ptr, int64_t tile_nodes) {
  const char* op = "walk_pack";
  TORCH_CHECK(on_gpu(feat) && on_gpu(thr) && on_gpu(left) &&
              on_gpu(default_left), op, ": tensors must be on the GPU");
  TORCH_CHECK(tile_nodes >= 1 && tile_nodes <= PRED_TILE_NODES, op,
              ": tile_nodes must be in [1, ", PRED_TILE_NODES, "]");
  TORCH_CHECK(!on_gpu(tree_ptr) && tree_ptr.scalar_type() == torch::kInt32 &&
              tree_ptr.dim() == 1 && tree_ptr.size(0) >= 1 &&
              tree_ptr.is_contiguous(),
              op, ": tree_ptr must be a host int32 vector");
  const int64_t n_nodes = feat.numel();
  TORCH_CHECK(feat.scalar_type() == torch::kInt32 && feat.is_contiguous() &&
              thr.scalar_type() == torch::kFloat32 && thr.is_contiguous() &&
              left.scalar_type() == torch::kInt32 && left.is_contiguous() &&
              default_left.scalar_type() == torch::kUInt8 &&
              default_left.is_contiguous() && thr.numel() == n_nodes &&
              left.numel() == n_nodes && default_left.numel() == n_nodes,
              op, ": bad forest arrays");
  const int T = (int)tree_ptr.size(0) - 1;
  const int32_t* tp = tree_ptr.data_ptr<int32_t>();
  TORCH_CHECK(tp[0] == 0 && tp[T] == n_nodes, op,
              ": tree_ptr does not span the node arrays");
  for (int t = 0; t < T; ++t)
    TORCH_CHECK(tp[t + 1] > tp[t], op, ": tree ", t, " has no nodes");
  WalkForest w;
  w.T = T;
  w.tile_nodes = (int)tile_nodes;
  w.lds_nodes = predict_lds_enabled();
  std::vector<int32_t> tiles;
  if (w.lds_nodes)
    w.lds_nodes = greedy_tree_tiles(tp, T, (int)tile_nodes, tiles);
  if (!w.lds_nodes) tiles = {0, (int32_t)T};
  w.n_tiles = (int)tiles.size() - 1;
  auto dev_i32 = [&](const int32_t* src, int64_t len) {
    return torch::from_blob(const_cast<int32_t*>(src), {len},
                            torch::TensorOptions().dtype(torch::kInt32))
        .clone().to(feat.device());
  };
  w.ptr_d = dev_i32(tp, T + 1);
  w.tile_d = dev_i32(tiles.data(), (int64_t)tiles.size());
  w.packed = torch::empty({n_nodes, 4},
      torch::TensorOptions().dtype(torch::kInt32).device(feat.device()));
  if (n_nodes) {
    auto zeros = torch::zeros({n_nodes},
        torch::TensorOptions().dtype(torch::kFloat32).device(feat.device()));
    hipLaunchKernelGGL(pack_nodes_kernel,
                       dim3((uint32_t)ceil_div(n_nodes, 256)), dim3(256), 0,
                       c10::hip::getCurrentHIPStream().stream(),
                       feat.data_ptr<int32_t>(), thr.data_ptr<float>(),
                       left.data_ptr<int32_t>(),
                       default_left.data_ptr<uint8_t>(),
                       zeros.data_ptr<float>(),
                       (uint4*)w.packed.data_ptr<int32_t>(), n_nodes);
  }
  return w;
}

static void walk_check_X(const char* op, const torch::Tensor& X,
                         const WalkForest& w) {
  TORCH_CHECK(on_gpu(X) && X.scalar_type() == torch::kFloat32 &&
              X.dim() == 2 && X.is_contiguous() &&
              X.device() == w.packed.device(),
              op, ": X must be contiguous f32 [n, F] on the forest's GPU");
}

// out[row, t] = node index (relative to the tree's root) of the leaf the
// row reaches in tree t. `out` is addressed through both strides, so the
// same kernel writes row-major [n, T] or a tree-major [T, n] scratch.
template <bool LDS_NODES>
__global__ __launch_bounds__(256) void predict_leaf_kernel(
    const float* __restrict__ X, const uint4* __restrict__ nodes,
    const int32_t* __restrict__ tree_ptr,
    const int32_t* __restrict__ tile_ptr, int32_t* __restrict__ out,
    int64_t row_stride, int64_t tree_stride, int64_t n, int F, int n_tiles) {
  __shared__ uint4 lds_nodes[LDS_NODES ? PRED_TILE_NODES : 1];
  const int64_t row0 =
      (int64_t)blockIdx.x * blockDim.x * PRED_ROWS_PER_THREAD + threadIdx.x;
  for (int tile = 0; tile < n_tiles; ++tile) {
    const int t0 = tile_ptr[tile], t1 = tile_ptr[tile + 1];
    const int nb0 = tree_ptr[t0];
    const uint4* nd = nodes + nb0;
    if (LDS_NODES) {
      const int span = tree_ptr[t1] - nb0;
      __syncthreads();  // previous walk done before overwriting LDS
      for (int i = threadIdx.x; i < span; i += blockDim.x)
        lds_nodes[i] = nodes[nb0 + i];
      __syncthreads();
      nd = lds_nodes;
    }
    for (int t = t0; t < t1; ++t) {
      const int rel = tree_ptr[t] - nb0;
      #pragma unroll
      for (int r = 0; r < PRED_ROWS_PER_THREAD; ++r) {
        const int64_t row = row0 + (int64_t)r * blockDim.x;
        if (row >= n) continue;
        int idx = 0;
        uint4 p = nd[rel];
        while (!(p.x & 0x80000000u)) {
          const float v = X[row * (int64_t)F + (p.x & 0x3FFFFFFFu)];
          const bool goleft =
              isnan(v) ? ((p.x & 0x40000000u) != 0)
                       : (v < __uint_as_float(p.y));
          idx = (int)p.z + (goleft ? 0 : 1);
          p = nd[rel + idx];
        }
        out[row * row_stride + t * tree_stride] = idx;
      }
    }
  }
}

void predict_leaf(torch::Tensor X, const WalkForest& w, torch::Tensor out) {
  walk_check_X("predict_leaf", X, w);
  TORCH_CHECK(!w.lds_nodes || w.tile_nodes <= PRED_TILE_NODES,
              "predict_leaf: forest tiled beyond the LDS tile");
  const int64_t n = X.size(0);
  const int T = w.T;
  TORCH_CHECK(on_gpu(out) && out.scalar_type() == torch::kInt32 &&
              out.dim() == 2 && out.size(0) == n && out.size(1) == T,
              "predict_leaf: out must be int32 [n, T] on the GPU");
  if (n == 0 || T == 0) return;
  const int64_t blocks = ceil_div(n, 256 * PRED_ROWS_PER_THREAD);
  TORCH_CHECK(blocks <= 0x7fffffffLL, "predict_leaf: ", n,
              " rows exceed one launch");
  auto stream = c10::hip::getCurrentHIPStream();
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(256), 0,
                       stream.stream(), X.data_ptr<float>(),
                       (const uint4*)w.packed.data_ptr<int32_t>(),
                       w.ptr_d.data_ptr<int32_t>(),
                       w.tile_d.data_ptr<int32_t>(), out.data_ptr<int32_t>(),
                       out.stride(0), out.stride(1), n, (int)X.size(1),
                       w.n_tiles);
  };
  if (w.lds_nodes) launch(predict_leaf_kernel<true>);
  else launch(predict_leaf_kernel<false>);
  CHECK_HIP(hipGetLastError());
}

// Saabas attributions. Per row and tree, in this order and in float64:
// out[row, F] += mean[root]; then at every split on the walk
// out[row, feat] += mean[child] - mean[node]. The row's F+1 sums start
// from what `out` holds. LDS_ACC keeps them in an LDS column
// [feature][thread] (bank = lane: conflict-free whatever the feature),
// loaded from `out` once and stored once, both coalesced; otherwise every
// add is a read-modify-write of `out` in global memory, in the same order.
// Dynamic LDS: [tile nodes | tile means] if LDS_NODES, then accumulators.
#define SAABAS_LDS_BYTES (160 * 1024)
template <bool LDS_NODES, bool LDS_ACC>
__global__ __launch_bounds__(1024) void saabas_contribs_kernel(
    const float* __restrict__ X, const uint4* __restrict__ nodes,
    const double* __restrict__ node_mean,
    const int32_t* __restrict__ tree_ptr,
    const int32_t* __restrict__ tile_ptr, double* __restrict__ out,
    int64_t out_stride, int64_t n, int F, int n_tiles, int tile_nodes) {
  extern __shared__ __attribute__((aligned(16))) char saabas_smem[];
  uint4* lds_nodes = (uint4*)saabas_smem;
  double* lds_mean = (double*)(saabas_smem + (size_t)tile_nodes * 16);
  double* lds_acc =
      (double*)(saabas_smem + (LDS_NODES ? (size_t)tile_nodes * 24 : 0));
  const int W = F + 1;
  const int64_t row_base = (int64_t)blockIdx.x * blockDim.x;
  const int64_t row = row_base + threadIdx.x;
  const bool valid = row < n;
  const int cells =
      (int)(n - row_base < blockDim.x ? n - row_base : blockDim.x) * W;
  if (LDS_ACC) {
    for (int e = threadIdx.x; e < cells; e += blockDim.x) {
      const int r = e / W, f = e - r * W;
      lds_acc[f * blockDim.x + r] = out[(row_base + r) * out_stride + f];
    }
    __syncthreads();
  }
  // the cell of feature f of this thread's row
  double* acc = LDS_ACC ? lds_acc + threadIdx.x : out + row * out_stride;
  const int64_t acc_stride = LDS_ACC ? (int64_t)blockDim.x : 1;
  for (int tile = 0; tile < n_tiles; ++tile) {
    const int t0 = tile_ptr[tile], t1 = tile_ptr[tile + 1];
    const int nb0 = tree_ptr[t0];
    const uint4* nd = nodes + nb0;
    const double* mn = node_mean + nb0;
    if (LDS_NODES) {
      const int span = tree_ptr[t1] - nb0;
      __syncthreads();  // previous walk done before overwriting LDS
      for (int i = threadIdx.x; i < span; i += blockDim.x) {
        lds_nodes[i] = nodes[nb0 + i];
        lds_mean[i] = node_mean[nb0 + i];
      }
      __syncthreads();
      nd = lds_nodes;
      mn = lds_mean;
    }
    if (!valid) continue;
    for (int t = t0; t < t1; ++t) {
      int cur = tree_ptr[t] - nb0;
      const int rel = cur;
      uint4 p = nd[cur];
      double m = mn[cur];
      acc[F * acc_stride] = acc[F * acc_stride] + m;
      while (!(p.x & 0x80000000u)) {
        const int f = (int)(p.x & 0x3FFFFFFFu);
        const float v = X[row * (int64_t)F + f];
        const bool goleft =
            isnan(v) ? ((p.x & 0x40000000u) != 0)
                     : (v < __uint_as_float(p.y));
        cur = rel + (int)p.z + (goleft ? 0 : 1);
        const double mc = mn[cur];
        acc[f * acc_stride] = acc[f * acc_stride] + (mc - m);
        m = mc;
        p = nd[cur];
      }
    }
  }
  if (LDS_ACC) {
    __syncthreads();
    for (int e = threadIdx.x; e < cells; e += blockDim.x) {
      const int r = e / W, f = e - r * W;
      out[(row_base + r) * out_stride + f] = lds_acc[f * blockDim.x + r];
    }
  }
}

// lds_acc: -1 = LDS accumulators when they fit SAABAS_LDS_BYTES next to the
// node tile, 0 = accumulate in global `out`, 1 = LDS or an error.
// threads (and the forest's tile size): launch geometry, chosen by ops.gpu
// (defaults measured there; benchmarks sweep them).
void saabas_contribs(torch::Tensor X, const WalkForest& w,
                     torch::Tensor node_mean, torch::Tensor out,
                     int64_t lds_acc, int64_t threads) {
  TORCH_CHECK(threads >= 64 && threads <= 1024 && threads % 64 == 0,
              "saabas_contribs: threads must be a multiple of 64 in "
              "[64, 1024]");
  walk_check_X("saabas_contribs", X, w);
  const int64_t tile_nodes = w.tile_nodes;
  const int64_t n = X.size(0);
  const int F = (int)X.size(1);
  const int T = w.T;
  TORCH_CHECK(on_gpu(node_mean) &&
              node_mean.scalar_type() == torch::kFloat64 &&
              node_mean.is_contiguous() && node_mean.numel() == w.packed.size(0),
              "saabas_contribs: node_mean must be f64 [n_nodes] on the GPU");
  TORCH_CHECK(on_gpu(out) && out.scalar_type() == torch::kFloat64 &&
              out.dim() == 2 && out.size(0) == n && out.size(1) == F + 1 &&
              (n == 0 || out.stride(1) == 1) &&
              (n <= 1 || out.stride(0) >= F + 1),
              "saabas_contribs: out must be f64 [n, F+1] on the GPU with "
              "unit column stride");
  if (n == 0 || T == 0) return;
  const size_t node_bytes = w.lds_nodes ? (size_t)tile_nodes * 24 : 0;
  const size_t acc_bytes = (size_t)(F + 1) * 8 * (size_t)threads;
  const bool fits = node_bytes + acc_bytes <= SAABAS_LDS_BYTES;
  TORCH_CHECK(lds_acc != 1 || fits, "saabas_contribs: ", F + 1,
              " accumulators of ", threads, " threads do not fit the LDS");
  const bool use_acc = lds_acc == 0 ? false : fits;
  const size_t lds_bytes = node_bytes + (use_acc ? acc_bytes : 0);
  const int64_t blocks = ceil_div(n, threads);
  TORCH_CHECK(blocks <= 0x7fffffffLL, "saabas_contribs: ", n,
              " rows exceed one launch");
  auto stream = c10::hip::getCurrentHIPStream();
  auto launch = [&](auto kernel, bool& attr_set) {
    if (!attr_set) {
      // dynamic LDS above 64 KiB needs the opt-in attribute (160 KiB/CU)
      CHECK_HIP(hipFuncSetAttribute(
          reinterpret_cast<const void*>(kernel),
          hipFuncAttributeMaxDynamicSharedMemorySize, SAABAS_LDS_BYTES));
      attr_set = true;
    }
    hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks),
                       dim3((uint32_t)threads), lds_bytes, stream.stream(),
                       X.data_ptr<float>(),
                       (const uint4*)w.packed.data_ptr<int32_t>(),
                       node_mean.data_ptr<double>(),
                       w.ptr_d.data_ptr<int32_t>(),
                       w.tile_d.data_ptr<int32_t>(), out.data_ptr<double>(),
                       out.stride(0), n, F, w.n_tiles, (int)tile_nodes);
  };
  static bool attr_set[4] = {false, false, false, false};
  if (w.lds_nodes && use_acc)
    launch(saabas_contribs_kernel<true, true>, attr_set[0]);
  else if (w.lds_nodes)
    launch(saabas_contribs_kernel<true, false>, attr_set[1]);
  else if (use_acc)
    launch(saabas_contribs_kernel<false, true>, attr_set[2]);
  else
    launch(saabas_contribs_kernel<false, false>, attr_set[3]);
  CHECK_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------
// tree_shap: exact TreeSHAP in path form (one root-to-leaf path = one
// independent unit, one element per unique feature; host side:
// ops.cpu.shap_paths). One thread owns one row and walks every path in
// order, so a row's output is written by that thread alone in a fixed
// sequence: no float atomics, bitwise repeatable. All arithmetic is
// float64 in the operation order of ops.cpu.tree_shap (the build keeps
// FMA contraction off).
//
// LDS (dynamic): path elements are staged in tiles of SHAP_TILE_ELEMS,
// as predict_trees_lds stages nodes - every row of the block reads the
// same element, a broadcast. The per-row permutation-weight vector is an
// LDS column laid out [element][thread]: a wave's 64 accesses are 64
// consecutive 8-byte words, conflict-free, and nothing is runtime-indexed
// in registers (no scratch). INTER adds a second column for the weights
// of the path with one element unwound.
// ---------------------------------------------------------------------------
#define SHAP_TILE_ELEMS 1024
#define SHAP_MAX_PATH_LEN 32
#define SHAP_THREADS 128
#define SHAP_INTER_THREADS 64

#define SHAP_RCP_LEN (SHAP_MAX_PATH_LEN + 8)

// a / k for a small positive integer k, given r = RN(1 / k) (the LDS table
// every block fills with true divisions): q = RN(a r), one exact FMA
// remainder, one FMA correction (Markstein's sequence) - the IEEE
// quotient in 3 instructions instead of the ~14 of the generic
// expansion. The divisions by path positions (ln, ln + 1, j + 1) are the
// bulk of the kernel's instruction stream; the ones by a zero_fraction
// stay generic.
__device__ __forceinline__ double shap_div_int(double a, int k,
                                               const double* rcp) {
  const double r = rcp[k];
  const double q = a * r;
  return fma(fma(-q, (double)k, a), r, q);
}

// _tree_shap's unwind_sum over weights w[0..ln] (column stride bs)
__device__ __forceinline__ double shap_unwound_sum(
    const double* w, int bs, int ln, double pz, bool hot,
    const double* rcp) {
  double total = 0.0;
  if (hot) {
    double nxt = w[ln * bs];
    for (int j = ln - 1; j >= 0; --j) {
      const double tmp = shap_div_int(nxt * (double)(ln + 1), j + 1, rcp);
      total += tmp;
      nxt = w[j * bs] -
            shap_div_int(tmp * pz * (double)(ln - j), ln + 1, rcp);
    }
  } else {
    for (int j = 0; j < ln; ++j)
      total += w[j * bs] * (double)(ln + 1) / (pz * (double)(ln - j));
  }
  return total;
}

template <bool INTER>
__global__ void tree_shap_kernel(
    const float* __restrict__ X,
    const int4* __restrict__ elem,      // {feature | miss_ok << 31, lo, hi, 0}
    const double* __restrict__ elem_z,  // zero_fraction
    const int32_t* __restrict__ path_ptr, const double* __restrict__ path_val,
    const int32_t* __restrict__ path_grp,
    const int32_t* __restrict__ tile_ptr,  // [n_tiles+1] path indices
    int n_tiles, double* __restrict__ out, int64_t n, int F, int G,
    int wlen) {  // wlen = longest path + 1 weights per row
  extern __shared__ __align__(16) double shap_lds[];
  double* lds_z = shap_lds;
  int4* lds_e = (int4*)(shap_lds + SHAP_TILE_ELEMS);
  double* rcp = shap_lds + 3 * SHAP_TILE_ELEMS;  // rcp[k] = 1 / k
  const int bs = (int)blockDim.x;
  double* w = rcp + SHAP_RCP_LEN + threadIdx.x;
  double* w2 = w + (size_t)wlen * bs;  // INTER only
  if (threadIdx.x < SHAP_RCP_LEN)  // published by the first tile's barrier
    rcp[threadIdx.x] = 1.0 / (double)(threadIdx.x ? threadIdx.x : 1);
  const int64_t row_stride =
      INTER ? (int64_t)(F + 1) * (F + 1) : (int64_t)G * (F + 1);
  const int64_t n_blocks = (n + bs - 1) / bs;
  for (int64_t rb = blockIdx.x; rb < n_blocks; rb += gridDim.x) {
    const int64_t row = rb * bs + threadIdx.x;
    const bool active = row < n;
    const float* xr = X + (active ? row : 0) * (int64_t)F;
    double* orow = out + (active ? row : 0) * row_stride;
    for (int tile = 0; tile < n_tiles; ++tile) {
      const int p0 = tile_ptr[tile], p1 = tile_ptr[tile + 1];
      const int eb = path_ptr[p0];
      const int span = path_ptr[p1] - eb;
      __syncthreads();  // previous tile's walk done before overwriting
      for (int i = threadIdx.x; i < span; i += bs) {
        lds_e[i] = elem[eb + i];
        lds_z[i] = elem_z[eb + i];
      }
      __syncthreads();
      if (!active) continue;
      for (int p = p0; p < p1; ++p) {
        const int e0 = path_ptr[p] - eb;
        const int m = path_ptr[p + 1] - path_ptr[p];
        if (m == 0 || (INTER && m < 2)) continue;
        // one_fraction of every element, as a bit mask
        uint32_t omask = 0;
        bool dead = false;
        for (int i = 0; i < m; ++i) {
          const int4 e = lds_e[e0 + i];
          const float x = xr[e.x & 0x7FFFFFFF];
          const float lo = __int_as_float(e.y), hi = __int_as_float(e.z);
          const bool o = isnan(x) ? (e.x < 0)
                                  : (x >= lo && (x < hi || hi == INFINITY));
          omask |= (uint32_t)o << i;
          // one == 0 and zero == 0: every subset term vanishes
          dead |= (!o && lds_z[e0 + i] == 0.0);
        }
        if (dead) continue;
        const double v = path_val[p];
        // EXTEND over the dummy root element, then every element
        w[0] = 1.0;
        for (int k = 1; k <= m; ++k) {
          const double pz = lds_z[e0 + k - 1];
          const double po = (omask >> (k - 1)) & 1u ? 1.0 : 0.0;
          double carry = 0.0;
          for (int i = k - 1; i >= 0; --i) {
            const double wi = w[i * bs];
            w[(i + 1) * bs] =
                carry + shap_div_int(po * wi * (double)(i + 1), k + 1, rcp);
            carry = shap_div_int(pz * wi * (double)(k - i), k + 1, rcp);
          }
          w[0] = carry;
        }
        if (!INTER) {
          double* dest = orow + (int64_t)path_grp[p] * (F + 1);
          for (int i = 0; i < m; ++i) {
            const double pz = lds_z[e0 + i];
            const bool hot = (omask >> i) & 1u;
            const double s = shap_unwound_sum(w, bs, m, pz, hot, rcp);
            dest[lds_e[e0 + i].x & 0x7FFFFFFF] +=
                s * ((hot ? 1.0 : 0.0) - pz) * v;
          }
        } else {
          for (int c = 0; c < m; ++c) {
            const double pzc = lds_z[e0 + c];
            const bool hotc = (omask >> c) & 1u;
            // UNWIND element c: w2[0..m-1] are the weights of E \ {c}
            if (hotc) {
              double nxt = w[m * bs];
              for (int j = m - 1; j >= 0; --j) {
                const double tmp =
                    shap_div_int(nxt * (double)(m + 1), j + 1, rcp);
                nxt = w[j * bs] -
                      shap_div_int(tmp * pzc * (double)(m - j), m + 1, rcp);
                w2[j * bs] = tmp;
              }
            } else {
              for (int j = 0; j < m; ++j)
                w2[j * bs] =
                    w[j * bs] * (double)(m + 1) / (pzc * (double)(m - j));
            }
            const double half = ((hotc ? 1.0 : 0.0) - pzc) / 2.0;
            double* dest =
                orow + (int64_t)(lds_e[e0 + c].x & 0x7FFFFFFF) * (F + 1);
            for (int j = 0; j < m; ++j) {
              if (j == c) continue;
              const double pz = lds_z[e0 + j];
              const bool hot = (omask >> j) & 1u;
              const double s = shap_unwound_sum(w2, bs, m - 1, pz, hot, rcp);
              dest[lds_e[e0 + j].x & 0x7FFFFFFF] +=
                  half * s * ((hot ? 1.0 : 0.0) - pz) * v;
            }
          }
        }
      }
    }
  }
}

// path_ptr arrives on the HOST: the tiling (consecutive paths whose
// elements fit SHAP_TILE_ELEMS) is a scan over it, and every index the
// kernel forms from it is checked here before anything is launched.
void tree_shap(torch::Tensor X, torch::Tensor elem, torch::Tensor elem_z,
               torch::Tensor path_ptr, torch::Tensor path_val,
               torch::Tensor path_grp, torch::Tensor out, int64_t n_groups,
               bool interactions) {
  TORCH_CHECK(on_gpu(X) && on_gpu(elem) && on_gpu(elem_z) &&
              on_gpu(path_val) && on_gpu(path_grp) && on_gpu(out),
              "tree_shap: tensors must be on the GPU");
  TORCH_CHECK(!on_gpu(path_ptr) && path_ptr.scalar_type() == torch::kInt32 &&
              path_ptr.dim() == 1 && path_ptr.size(0) >= 1 &&
              path_ptr.is_contiguous(),
              "tree_shap: path_ptr must be a host int32 vector");
  TORCH_CHECK(X.scalar_type() == torch::kFloat32 && X.dim() == 2 &&
              X.is_contiguous(), "tree_shap: X must be contiguous f32 [n, F]");
  TORCH_CHECK(out.scalar_type() == torch::kFloat64 && out.is_contiguous(),
              "tree_shap: out must be contiguous f64");
  TORCH_CHECK(elem.scalar_type() == torch::kInt32 && elem.dim() == 2 &&
              elem.size(1) == 4 && elem.is_contiguous() &&
              elem_z.scalar_type() == torch::kFloat64 &&
              elem_z.is_contiguous() &&
              path_val.scalar_type() == torch::kFloat64 &&
              path_val.is_contiguous() &&
              path_grp.scalar_type() == torch::kInt32 &&
              path_grp.is_contiguous(), "tree_shap: bad path arrays");
  const int64_t n = X.size(0);
  const int F = (int)X.size(1);
  const int64_t P = path_ptr.size(0) - 1;
  const int G = interactions ? 1 : (int)n_groups;
  TORCH_CHECK(G >= 1, "tree_shap: n_groups must be >= 1");
  const int64_t per_row =
      interactions ? (int64_t)(F + 1) * (F + 1) : (int64_t)G * (F + 1);
  TORCH_CHECK(out.numel() == n * per_row, "tree_shap: out has ",
              out.numel(), " elements, expected ", n * per_row);
  TORCH_CHECK(path_val.numel() == P && path_grp.numel() == P,
              "tree_shap: per-path arrays do not match path_ptr");
  const int32_t* pp = path_ptr.data_ptr<int32_t>();
  TORCH_CHECK(pp[0] == 0 && pp[P] == elem.size(0) &&
              elem_z.numel() == elem.size(0),
              "tree_shap: path_ptr does not span the element arrays");
  if (n == 0 || P == 0) return;
  std::vector<int32_t> tiles;
  tiles.push_back(0);
  int max_len = 0;
  int64_t tile_e0 = 0;
  for (int64_t p = 0; p < P; ++p) {
    const int len = pp[p + 1] - pp[p];
    TORCH_CHECK(len >= 0 && len <= SHAP_MAX_PATH_LEN, "tree_shap: path ", p,
                " has ", len, " elements (max ", SHAP_MAX_PATH_LEN, ")");
    if (len > max_len) max_len = len;
    if (pp[p + 1] - tile_e0 > SHAP_TILE_ELEMS) {  // close the tile before p
      tiles.push_back((int32_t)p);
      tile_e0 = pp[p];
    }
  }
  tiles.push_back((int32_t)P);
  auto dev_i32 = [&](const int32_t* src, int64_t len) {
    return torch::from_blob(const_cast<int32_t*>(src), {len},
                            torch::TensorOptions().dtype(torch::kInt32))
        .clone().to(X.device());
  };
  auto ptr_d = dev_i32(pp, P + 1);
  auto tile_d = dev_i32(tiles.data(), (int64_t)tiles.size());
  const int threads = interactions ? SHAP_INTER_THREADS : SHAP_THREADS;
  const int wlen = max_len + 1;
  const size_t lds_bytes =
      (size_t)SHAP_TILE_ELEMS * 24 + SHAP_RCP_LEN * sizeof(double) +
      (size_t)wlen * threads * sizeof(double) * (interactions ? 2 : 1);
  TORCH_CHECK(lds_bytes <= 64 * 1024, "tree_shap: LDS budget exceeded");
  const int64_t blocks = std::min<int64_t>(ceil_div(n, threads), 65536);
  auto stream = c10::hip::getCurrentHIPStream();
  if (interactions) {
    hipLaunchKernelGGL((tree_shap_kernel<true>), dim3((uint32_t)blocks),
                       dim3(threads), lds_bytes, stream.stream(),
                       X.data_ptr<float>(),
                       (const int4*)elem.data_ptr<int32_t>(),
                       elem_z.data_ptr<double>(), ptr_d.data_ptr<int32_t>(),
                       path_val.data_ptr<double>(),
                       path_grp.data_ptr<int32_t>(),
                       tile_d.data_ptr<int32_t>(), (int)tiles.size() - 1,
                       out.data_ptr<double>(), n, F, G, wlen);
  } else {
    hipLaunchKernelGGL((tree_shap_kernel<false>), dim3((uint32_t)blocks),
                       dim3(threads), lds_bytes, stream.stream(),
                       X.data_ptr<float>(),
                       (const int4*)elem.data_ptr<int32_t>(),
                       elem_z.data_ptr<double>(), ptr_d.data_ptr<int32_t>(),
                       path_val.data_ptr<double>(),
                       path_grp.data_ptr<int32_t>(),
                       tile_d.data_ptr<int32_t>(), (int)tiles.size() - 1,
                       out.data_ptr<double>(), n, F, G, wlen);
  }
  CHECK_HIP(hipGetLastError());
}

void update_margins(torch::Tensor margin, torch::Tensor ridx,
                    torch::Tensor starts, torch::Tensor counts,
                    torch::Tensor leaf_vals, torch::Tensor ridx_b,
                    torch::Tensor parity) {
  const int K = (int)starts.size(0);
  if (K == 0) return;
  auto dev = margin.device();
  auto starts_cpu = starts.to(torch::kCPU).to(torch::kInt64);
  auto counts_cpu = counts.to(torch::kCPU).to(torch::kInt64);
  auto chunk_off_cpu = torch::zeros({K + 1}, torch::kInt64);
  int64_t total_chunks = 0;
  {
    auto acc = chunk_off_cpu.accessor<int64_t, 1>();
    auto cacc = counts_cpu.accessor<int64_t, 1>();
    for (int k = 0; k < K; ++k)
      acc[k + 1] = acc[k] + (cacc[k] + MARGIN_CHUNK - 1) / MARGIN_CHUNK;
    total_chunks = acc[K];
  }
  if (total_chunks == 0) return;
  auto stream0 = c10::hip::getCurrentHIPStream();
  static thread_local PinnedStager margin_meta_stager;
  const bool have_parity = parity.numel() > 0;
  auto meta_cpu = margin_meta_stager.get((have_parity ? 4 : 3) * K + 1);
  if (have_parity) {
    cat_into_pinned(meta_cpu, {starts_cpu, counts_cpu, chunk_off_cpu,
                               parity.to(torch::kCPU).to(torch::kInt64)});
  } else {
    cat_into_pinned(meta_cpu, {starts_cpu, counts_cpu, chunk_off_cpu});
  }
  auto meta = meta_cpu.to(dev, /*non_blocking=*/true);
  margin_meta_stager.mark(stream0.stream());
  int64_t* mp = meta.data_ptr<int64_t>();
  // leaf values ride their own pinned stager (fp32; the int64 meta
  // stager cannot carry them without a bitcast)
  static thread_local PinnedStager margin_lv_stager;
  auto lv_cpu = margin_lv_stager.get(K, torch::kFloat32);
  lv_cpu.copy_(leaf_vals.to(torch::kFloat32));
  auto lv = lv_cpu.to(dev, /*non_blocking=*/true);
  margin_lv_stager.mark(stream0.stream());
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(update_margins_kernel, dim3((uint32_t)total_chunks),
                     dim3(PART_THREADS), 0, stream.stream(),
                     margin.data_ptr<float>(), ridx.data_ptr<int32_t>(),
                     ridx_b.numel() ? ridx_b.data_ptr<int32_t>()
                                    : ridx.data_ptr<int32_t>(),
                     mp, mp + 2 * K,
                     have_parity ? mp + 3 * K + 1 : nullptr,
                     lv.data_ptr<float>(), K);
}

template <int NDW, int R>
static void launch_apply_tree_binned(bool lds, int grid, size_t lds_bytes,
                                     hipStream_t s, const uint8_t* bins,
                                     const uint2* nodes, float* margin,
                                     int64_t n, int64_t row_stride,
                                     int64_t margin_stride, int n_nodes) {
  if (lds) {
    hipLaunchKernelGGL((apply_tree_binned_kernel<NDW, R, true>), dim3(grid),
                       dim3(ATB_THREADS), lds_bytes, s, bins, nodes, margin,
                       n, row_stride, margin_stride, n_nodes, n_nodes);
  } else {
    hipLaunchKernelGGL((apply_tree_binned_kernel<NDW, R, false>), dim3(grid),
                       dim3(ATB_THREADS), 0, s, bins, nodes, margin, n,
                       row_stride, margin_stride, n_nodes, n_nodes);
  }
}

// margin[r * margin_stride] += value[leaf of row r] for every row of the
// binned matrix. The tree arrives as HOST arrays (feat < 0 marks a leaf)
// and is packed into ONE pinned H2D; `margin` may be a strided column view.
void apply_tree_binned(torch::Tensor bins, torch::Tensor margin,
                       torch::Tensor feat, torch::Tensor split_bin,
                       torch::Tensor left, torch::Tensor default_left,
                       torch::Tensor value) {
  TORCH_CHECK(on_gpu(bins) && bins.dtype() == torch::kUInt8 &&
                  bins.dim() == 2 && bins.stride(1) == 1,
              "apply_tree_binned: bins must be a GPU uint8 [n, F] matrix");
  TORCH_CHECK(on_gpu(margin) && margin.dtype() == torch::kFloat32 &&
                  margin.dim() == 1,
              "apply_tree_binned: margin must be a GPU f32 vector (view)");
  const int64_t n = bins.size(0);
  const int64_t F = bins.size(1);
  TORCH_CHECK(margin.size(0) == n, "apply_tree_binned: margin has ",
              margin.size(0), " rows, bins ", n);
  const int64_t row_stride = n > 1 ? bins.stride(0) : F;
  const int64_t margin_stride = n > 1 ? margin.stride(0) : 1;
  TORCH_CHECK(row_stride >= F && margin_stride >= 1);
  const int64_t n_nodes = feat.size(0);
  TORCH_CHECK(n_nodes >= 1 && n_nodes < (int64_t)1 << 30);
  auto feat_c = feat.to(torch::kCPU).to(torch::kInt32).contiguous();
  auto sbin_c = split_bin.to(torch::kCPU).to(torch::kInt32).contiguous();
  auto left_c = left.to(torch::kCPU).to(torch::kInt32).contiguous();
  auto dl_c = default_left.to(torch::kCPU).to(torch::kUInt8).contiguous();
  auto val_c = value.to(torch::kCPU).to(torch::kFloat32).contiguous();
  TORCH_CHECK(sbin_c.size(0) == n_nodes && left_c.size(0) == n_nodes &&
                  dl_c.size(0) == n_nodes && val_c.size(0) == n_nodes,
              "apply_tree_binned: tree arrays differ in length");
  if (n == 0) return;
  static thread_local PinnedStager atb_node_stager;
  auto nodes_cpu = atb_node_stager.get(n_nodes);
  {
    const int32_t* fp = feat_c.data_ptr<int32_t>();
    const int32_t* bp = sbin_c.data_ptr<int32_t>();
    const int32_t* lp = left_c.data_ptr<int32_t>();
    const uint8_t* dp = dl_c.data_ptr<uint8_t>();
    const float* vp = val_c.data_ptr<float>();
    uint32_t* np = reinterpret_cast<uint32_t*>(nodes_cpu.data_ptr<int64_t>());
    for (int64_t i = 0; i < n_nodes; ++i) {
      if (fp[i] < 0) {
        np[2 * i] = ATB_LEAF;
        std::memcpy(&np[2 * i + 1], &vp[i], 4);
      } else {
        TORCH_CHECK(fp[i] < F && fp[i] < 65536 && bp[i] >= 0 &&
                        bp[i] <= 255 && lp[i] > 0 && lp[i] + 1 < n_nodes,
                    "apply_tree_binned: malformed node ", i);
        np[2 * i] = (uint32_t)fp[i] | ((uint32_t)bp[i] << 16) |
                    (dp[i] ? (1u << 24) : 0u);
        np[2 * i + 1] = (uint32_t)lp[i];
      }
    }
  }
  auto nodes = nodes_cpu.to(bins.device(), /*non_blocking=*/true);
  auto stream = c10::hip::getCurrentHIPStream();
  atb_node_stager.mark(stream.stream());
  const uint8_t* bptr = bins.data_ptr<uint8_t>();
  const uint2* nptr = reinterpret_cast<const uint2*>(nodes.data_ptr<int64_t>());
  float* mptr = margin.data_ptr<float>();
  const bool lds = n_nodes <= ATB_LDS_NODES;
  const size_t lds_bytes = lds ? (size_t)n_nodes * sizeof(uint2) : 0;
  // whole-row register form: 16 B aligned rows of 4, 8, 12 or 16 dwords
  // whose padding lies inside the allocation
  const int64_t avail =
      (int64_t)bins.storage().nbytes() - bins.storage_offset();
  const bool vec = (reinterpret_cast<uintptr_t>(bptr) % 16 == 0) &&
                   (row_stride % 16 == 0) && row_stride <= 64 &&
                   n * row_stride <= avail;
  const int ndw = vec ? (int)(row_stride / 4) : 0;
  const int R = (ndw == 12 || ndw == 16) ? 4 : 8;
  // one chunk per workgroup while the table is small (<= 16 KB to stage);
  // a big table is staged by a chip-filling grid that strides over chunks
  const int64_t chunks = ceil_div(n, (int64_t)ATB_THREADS * R);
  const int grid = (int)std::min<int64_t>(
      chunks, n_nodes <= 2048 ? (int64_t)1 << 30 : 1024);
  hipStream_t s = stream.stream();
  const int nn = (int)n_nodes;
  switch (ndw) {
    case 4:
      launch_apply_tree_binned<4, 8>(lds, grid, lds_bytes, s, bptr, nptr,
                                     mptr, n, row_stride, margin_stride, nn);
      break;
    case 8:
      launch_apply_tree_binned<8, 8>(lds, grid, lds_bytes, s, bptr, nptr,
                                     mptr, n, row_stride, margin_stride, nn);
      break;
    case 12:
      launch_apply_tree_binned<12, 4>(lds, grid, lds_bytes, s, bptr, nptr,
                                      mptr, n, row_stride, margin_stride, nn);
      break;
    case 16:
      launch_apply_tree_binned<16, 4>(lds, grid, lds_bytes, s, bptr, nptr,
                                      mptr, n, row_stride, margin_stride, nn);
      break;
    default:
      launch_apply_tree_binned<0, 8>(lds, grid, lds_bytes, s, bptr, nptr,
                                     mptr, n, row_stride, margin_stride, nn);
  }
  CHECK_HIP(hipGetLastError());
}

static_assert(LQH_THREADS == 256, "flush maps one thread to one bin");

// One radix-select pass over the leaf segments; accumulates into hist
// (int64 [K,256], device). starts/counts/parity/prefix are host tensors
// staged through one pinned H2D.
void leaf_quantile_hist(torch::Tensor resid, torch::Tensor weight,
                        torch::Tensor ridx, torch::Tensor ridx_b,
                        torch::Tensor starts, torch::Tensor counts,
                        torch::Tensor parity, torch::Tensor prefix,
                        int64_t pass, torch::Tensor hist) {
  const int K = (int)starts.size(0);
  if (K == 0) return;
  TORCH_CHECK(on_gpu(resid) && resid.dtype() == torch::kFloat32 &&
              resid.is_contiguous() && resid.dim() == 1);
  TORCH_CHECK(on_gpu(ridx) && ridx.dtype() == torch::kInt32 &&
              ridx.is_contiguous());
  TORCH_CHECK(on_gpu(hist) && hist.dtype() == torch::kInt64 &&
              hist.is_contiguous() && hist.numel() == (int64_t)K * 256);
  TORCH_CHECK(pass >= 0 && pass < 4, "pass must be 0..3");
  TORCH_CHECK(counts.size(0) == K && prefix.size(0) == K);
  const bool have_w = weight.numel() > 0;
  if (have_w)
    TORCH_CHECK(on_gpu(weight) && weight.dtype() == torch::kInt64 &&
                weight.is_contiguous() &&
                weight.numel() == resid.numel());
  const bool have_b = ridx_b.numel() > 0;
  if (have_b)
    TORCH_CHECK(on_gpu(ridx_b) && ridx_b.dtype() == torch::kInt32 &&
                ridx_b.is_contiguous());
  const bool have_parity = parity.numel() > 0;
  if (have_parity)
    TORCH_CHECK(parity.size(0) == K && have_b,
                "parity needs the second ridx buffer");
  auto starts_cpu = starts.to(torch::kCPU).to(torch::kInt64).contiguous();
  auto counts_cpu = counts.to(torch::kCPU).to(torch::kInt64).contiguous();
  auto prefix_cpu = prefix.to(torch::kCPU).to(torch::kInt64).contiguous();
  auto parity_cpu = have_parity
      ? parity.to(torch::kCPU).to(torch::kInt64).contiguous()
      : torch::zeros({K}, torch::kInt64);
  auto chunk_off_cpu = torch::zeros({K + 1}, torch::kInt64);
  int64_t total_chunks = 0;
  {
    auto acc = chunk_off_cpu.accessor<int64_t, 1>();
    auto cacc = counts_cpu.accessor<int64_t, 1>();
    auto sacc = starts_cpu.accessor<int64_t, 1>();
    auto pacc = parity_cpu.accessor<int64_t, 1>();
    for (int k = 0; k < K; ++k) {
      // every segment must lie inside the buffer it is read from
      const int64_t lim = pacc[k] ? ridx_b.numel() : ridx.numel();
      TORCH_CHECK(sacc[k] >= 0 && cacc[k] >= 0 && sacc[k] + cacc[k] <= lim,
                  "leaf segment ", k, " out of range");
      TORCH_CHECK(pacc[k] == 0 || pacc[k] == 1);
      acc[k + 1] = acc[k] + (cacc[k] + LQH_CHUNK - 1) / LQH_CHUNK;
    }
    total_chunks = acc[K];
  }
  if (total_chunks == 0) return;
  auto stream = c10::hip::getCurrentHIPStream();
  static thread_local PinnedStager lqh_meta_stager;
  auto meta_cpu = lqh_meta_stager.get(5 * K + 1);
  cat_into_pinned(meta_cpu, {starts_cpu, counts_cpu, chunk_off_cpu,
                             parity_cpu, prefix_cpu});
  auto meta = meta_cpu.to(resid.device(), /*non_blocking=*/true);
  lqh_meta_stager.mark(stream.stream());
  int64_t* mp = meta.data_ptr<int64_t>();
  hipLaunchKernelGGL(leaf_quantile_hist_kernel,
                     dim3((uint32_t)total_chunks), dim3(LQH_THREADS), 0,
                     stream.stream(), resid.data_ptr<float>(),
                     have_w ? weight.data_ptr<int64_t>() : nullptr,
                     ridx.data_ptr<int32_t>(),
                     have_b ? ridx_b.data_ptr<int32_t>()
                            : ridx.data_ptr<int32_t>(),
                     mp, mp + 2 * K,
                     have_parity ? mp + 3 * K + 1 : nullptr,
                     mp + 4 * K + 1,
                     (long long*)hist.data_ptr<int64_t>(), K, (int)pass);
}

// -- gradient-based row sampling ---------------------------------------------
static void mvs_check_c(const torch::Tensor& c) {
  TORCH_CHECK(on_gpu(c) && c.dtype() == torch::kUInt32 && c.dim() == 1 &&
                  c.is_contiguous() && c.numel() < (1ll << 31),
              "mvs: c must be a contiguous uint32 device vector, n < 2^31");
}

static void mvs_check_gpair(const torch::Tensor& gpair) {
  TORCH_CHECK(on_gpu(gpair) && gpair.dtype() == torch::kFloat32 &&
                  gpair.dim() == 2 && gpair.size(1) == 2 &&
                  gpair.is_contiguous() && gpair.size(0) < (1ll << 31),
              "mvs: gpair must be contiguous f32 [n, 2] on device, n < 2^31");
}

torch::Tensor mvs_score(torch::Tensor gpair, double sv) {
  mvs_check_gpair(gpair);
  const int64_t n = gpair.size(0);
  auto c = torch::empty({n}, gpair.options().dtype(torch::kUInt32));
  if (n == 0) return c;
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(mvs_score_kernel,
                     dim3((uint32_t)ceil_div(n, MVS_THREADS)),
                     dim3(MVS_THREADS), 0, stream.stream(),
                     (const float2*)gpair.data_ptr<float>(),
                     c.data_ptr<uint32_t>(), sv, n);
  return c;
}

// int64 [3] device: (#{c > 0}, max c, sum c)
torch::Tensor mvs_stats(torch::Tensor c) {
  mvs_check_c(c);
  const int64_t n = c.numel();
  const auto opts = c.options().dtype(torch::kInt64);
  if (n == 0) return torch::zeros({3}, opts);
  auto stats = torch::empty({3}, opts);  // the fold writes all of it
  const int64_t blocks = ceil_div(n, MVS_CHUNK);
  auto partials =
      torch::empty({blocks, 3}, c.options().dtype(torch::kInt64));
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(mvs_stats_kernel, dim3((uint32_t)blocks),
                     dim3(MVS_THREADS), 0, stream.stream(),
                     c.data_ptr<uint32_t>(), n,
                     (unsigned long long*)partials.data_ptr<int64_t>());
  hipLaunchKernelGGL(mvs_stats_fold_kernel, dim3(1), dim3(MVS_THREADS), 0,
                     stream.stream(),
                     (const unsigned long long*)partials.data_ptr<int64_t>(),
                     blocks, (unsigned long long*)stats.data_ptr<int64_t>());
  return stats;
}

// int64 [256, 2] device: per digit (count, sum c) of the rows under prefix
torch::Tensor mvs_hist(torch::Tensor c, int64_t prefix, int64_t pass) {
  mvs_check_c(c);
  TORCH_CHECK(pass >= 0 && pass < 4, "pass must be 0..3");
  TORCH_CHECK(prefix >= 0 && prefix < (1ll << (8 * pass)),
              "prefix must fit the top 8*pass bits");
  const int64_t n = c.numel();
  const auto opts = c.options().dtype(torch::kInt64);
  if (n == 0) return torch::zeros({256, 2}, opts);
  auto hist = torch::empty({256, 2}, opts);  // the fold writes all of it
  const int64_t blocks = ceil_div(n, MVS_CHUNK);
  const int n_slots =
      blocks < MVS_HIST_SLOTS ? (int)blocks : MVS_HIST_SLOTS;
  auto slots =
      torch::zeros({n_slots, 512}, c.options().dtype(torch::kInt64));
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(mvs_hist_kernel, dim3((uint32_t)blocks),
                     dim3(MVS_THREADS), 0, stream.stream(),
                     c.data_ptr<uint32_t>(), n, (uint32_t)prefix, (int)pass,
                     (unsigned long long*)slots.data_ptr<int64_t>(), n_slots);
  hipLaunchKernelGGL(mvs_hist_fold_kernel, dim3(1), dim3(512), 0,
                     stream.stream(),
                     (const unsigned long long*)slots.data_ptr<int64_t>(),
                     n_slots, (unsigned long long*)hist.data_ptr<int64_t>());
  return hist;
}

// (keep uint8 [n], reweighted gpair f32 [n, 2]); key: the uint64 bits
std::vector<torch::Tensor> mvs_sample(torch::Tensor gpair, torch::Tensor c,
                                      int64_t S, int64_t M, int64_t key) {
  mvs_check_gpair(gpair);
  mvs_check_c(c);
  const int64_t n = gpair.size(0);
  TORCH_CHECK(c.numel() == n, "mvs_sample: c must have one value per row");
  // c*M < 2^61 and u*S < 2^93: the kernel's products do not wrap
  TORCH_CHECK(S >= 0 && M >= 0 && S < (1ll << 61) && M < (1ll << 31),
              "mvs_sample: (S, M) out of range");
  auto keep = torch::empty({n}, gpair.options().dtype(torch::kUInt8));
  auto out = torch::empty_like(gpair);
  if (n == 0) return {keep, out};
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(mvs_sample_kernel,
                     dim3((uint32_t)ceil_div(n, MVS_THREADS)),
                     dim3(MVS_THREADS), 0, stream.stream(),
                     (const float2*)gpair.data_ptr<float>(),
                     c.data_ptr<uint32_t>(), (unsigned long long)S,
                     (unsigned long long)M, (unsigned long long)key,
                     keep.data_ptr<uint8_t>(),
                     (float2*)out.data_ptr<float>(), n);
  return {keep, out};
}

torch::Tensor lambdarank_grad(torch::Tensor margin, torch::Tensor label,
                              torch::Tensor group_ptr, torch::Tensor rank,
                              torch::Tensor idcg, bool use_ndcg) {
  const int64_t n = margin.size(0);
  const int G = (int)group_ptr.size(0) - 1;
  auto out = torch::zeros({n, 2},
      torch::TensorOptions().dtype(torch::kFloat32).device(margin.device()));
  if (n == 0 || G <= 0) return out;
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(lambdarank_kernel, dim3(G), dim3(256), 0,
                     stream.stream(), margin.data_ptr<float>(),
                     label.data_ptr<float>(), group_ptr.data_ptr<int64_t>(),
                     rank.data_ptr<int32_t>(),
                     use_ndcg ? idcg.data_ptr<double>() : nullptr,
                     (float2*)out.data_ptr<float>(), use_ndcg ? 1 : 0);
  return out;
}


// ---------------------------------------------------------------------------
// grad_fused: objective gradient + hessian + |g|/|h| max in ONE pass.
// Replaces the 5-kernel torch chain (sigmoid, sub, mul, clamp, stack)
// plus the two abs().max() reduction passes for the hot objectives -
// the margin/label are read once and the fp32 gpair written once.
// The f32 op ORDER replicates torch's eager kernels exactly
// (p = 1/(1+expf(-x)); h = max(p*(1-p), eps); per-factor multiplies in
// the same sequence), so models stay bitwise-identical to the CPU
// oracle. The max reduction is order-free (max is associative) and, like
// torch's abs().max() and clamp(), keeps NaN: fmaxf would drop it, and a
// diverged margin would quantize as if it were finite.
// MODE 0: reg:squarederror (g = m - y, h = 1)
// MODE 1: binary:logistic  (g = p - y, h = max(p(1-p), 1e-16))
// ---------------------------------------------------------------------------
// max(a, b) that returns NaN when either side is NaN
__device__ __forceinline__ float max_keep_nan(float a, float b) {
  return (b > a || b != b) ? b : a;
}

template <int MODE>
__global__ __launch_bounds__(256) void grad_fused_kernel(
    const float* __restrict__ margin, const float* __restrict__ label,
    const float* __restrict__ weight,  // nullable
    float spw, float2* __restrict__ gpair,
    float* __restrict__ block_max,  // [gridDim.x, 2] per-block maxes
    int64_t n) {
  float gmax = 0.0f, hmax = 0.0f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const float x = margin[i];
    const float y = label[i];
    float g, h;
    if constexpr (MODE == 1) {
      const float p = 1.0f / (1.0f + expf(-x));
      g = p - y;
      const float pq = p * (1.0f - p);
      h = pq < 1e-16f ? 1e-16f : pq;  // NaN stays NaN, as torch.clamp
      if (spw != 1.0f) {
        const float w = 1.0f + (spw - 1.0f) * y;
        g *= w;
        h *= w;
      }
    } else {
      g = x - y;
      h = 1.0f;
    }
    if (weight != nullptr) {
      const float w = weight[i];
      g *= w;
      h *= w;
    }
    gpair[i] = {g, h};
    gmax = max_keep_nan(gmax, fabsf(g));
    hmax = max_keep_nan(hmax, fabsf(h));
  }
  // wave reduce -> LDS -> one [2]-float store per BLOCK. A global
  // atomicMax per wave serialized 43k atomics on TWO L2 addresses and
  // cost ~10x the kernel's memory traffic (measured 496 us for 186 MB);
  // per-block maxes + a tiny torch amax reduction have zero contention.
  __shared__ float red[2 * 256 / WAVE];
  #pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    gmax = max_keep_nan(gmax, __shfl_down(gmax, off, WAVE));
    hmax = max_keep_nan(hmax, __shfl_down(hmax, off, WAVE));
  }
  const int wid = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    red[2 * wid] = gmax;
    red[2 * wid + 1] = hmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = blockDim.x / WAVE;
    float g = red[0], h = red[1];
    for (int w = 1; w < nw; ++w) {
      g = max_keep_nan(g, red[2 * w]);
      h = max_keep_nan(h, red[2 * w + 1]);
    }
    block_max[2 * (size_t)blockIdx.x] = g;
    block_max[2 * (size_t)blockIdx.x + 1] = h;
  }
}

std::vector<torch::Tensor> grad_fused(torch::Tensor margin,
                                      torch::Tensor label,
                                      torch::Tensor weight, double spw,
                                      int64_t mode) {
  TORCH_CHECK(on_gpu(margin) && margin.dtype() == torch::kFloat32);
  const int64_t n = margin.numel();
  auto dev = margin.device();
  auto gpair = torch::empty(
      {n, 2}, torch::TensorOptions().dtype(torch::kFloat32).device(dev));
  if (n == 0) {
    return {gpair, torch::zeros({2}, torch::TensorOptions()
                                         .dtype(torch::kFloat32)
                                         .device(dev))};
  }
  auto stream = c10::hip::getCurrentHIPStream();
  const int64_t blocks = std::min<int64_t>(ceil_div(n, 256 * 16), 4096);
  auto block_max = torch::empty(
      {blocks, 2},
      torch::TensorOptions().dtype(torch::kFloat32).device(dev));
  const float* wp =
      weight.numel() ? weight.data_ptr<float>() : nullptr;
  if (mode == 1) {
    hipLaunchKernelGGL((grad_fused_kernel<1>), dim3((uint32_t)blocks),
                       dim3(256), 0, stream.stream(),
                       margin.data_ptr<float>(), label.data_ptr<float>(),
                       wp, (float)spw,
                       (float2*)gpair.data_ptr<float>(),
                       block_max.data_ptr<float>(), n);
  } else {
    hipLaunchKernelGGL((grad_fused_kernel<0>), dim3((uint32_t)blocks),
                       dim3(256), 0, stream.stream(),
                       margin.data_ptr<float>(), label.data_ptr<float>(),
                       wp, (float)spw,
                       (float2*)gpair.data_ptr<float>(),
                       block_max.data_ptr<float>(), n);
  }
  // max is order-free and torch's max keeps NaN, so this equals
  // abs().max() bitwise
  auto absmax = std::get<0>(block_max.max(0));
  return {gpair, absmax};
}


// ---------------------------------------------------------------------------
// Fused eval metrics: ONE pass over [margin, label(, weight)] replaces
// the 4-6 torch f64 elementwise/reduction kernels per metric per round.
// logloss: per-block (sum w*ll, sum w) f64 partials -> torch .sum(0)
// (fixed-order reduction, deterministic). AUC: unweighted int64
// pos/neg score-bin histograms via global atomics (exact).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eval_logloss_kernel(
    const float* __restrict__ margin, const float* __restrict__ label,
    const float* __restrict__ weight,  // nullable
    double* __restrict__ block_out,    // [gridDim.x, 2]
    int64_t n) {
  double ll = 0.0, wsum = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    // same math as metrics.LogLoss: sigmoid in f64, clamped p
    double p = 1.0 / (1.0 + exp(-(double)margin[i]));
    // comparisons, not fmin/fmax: a NaN margin stays NaN (torch.clamp
    // does the same), so a diverged run cannot report a finite loss
    p = p < 1e-16 ? 1e-16 : (p > 1.0 - 1e-16 ? 1.0 - 1e-16 : p);
    const double y = (double)label[i];
    const double w = weight ? (double)weight[i] : 1.0;
    ll += w * -(y * log(p) + (1.0 - y) * log(1.0 - p));
    wsum += w;
  }
  __shared__ double red[2 * 256 / WAVE];
  #pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    ll += __shfl_down(ll, off, WAVE);
    wsum += __shfl_down(wsum, off, WAVE);
  }
  const int wid = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    red[2 * wid] = ll;
    red[2 * wid + 1] = wsum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = blockDim.x / WAVE;
    double a = red[0], b = red[1];
    for (int w = 1; w < nw; ++w) {
      a += red[2 * w];
      b += red[2 * w + 1];
    }
    block_out[2 * (size_t)blockIdx.x] = a;
    block_out[2 * (size_t)blockIdx.x + 1] = b;
  }
}

torch::Tensor eval_logloss(torch::Tensor margin, torch::Tensor label,
                           torch::Tensor weight) {
  const int64_t n = margin.numel();
  auto dev = margin.device();
  const int64_t blocks = std::min<int64_t>(ceil_div(n, 256 * 16), 2048);
  auto block_out = torch::empty(
      {std::max<int64_t>(blocks, 1), 2},
      torch::TensorOptions().dtype(torch::kFloat64).device(dev));
  if (n == 0) return torch::zeros({2}, block_out.options());
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(eval_logloss_kernel, dim3((uint32_t)blocks),
                     dim3(256), 0, stream.stream(),
                     margin.data_ptr<float>(), label.data_ptr<float>(),
                     weight.numel() ? weight.data_ptr<float>() : nullptr,
                     block_out.data_ptr<double>(), n);
  return block_out.sum(0);  // fixed-order torch reduction
}

__global__ __launch_bounds__(256) void eval_auc_hist_kernel(
    const float* __restrict__ margin, const float* __restrict__ label,
    long long* __restrict__ hist,  // [2*B]: neg plane | pos plane
    int B, int64_t n) {
  // Per-WG LDS u32 histogram (2*B*4 = 128 KiB dynamic LDS), merged
  // once with skip-if-zero global atomics. The direct-global version
  // serialized on the few bins a saturated sigmoid concentrates mass
  // into: measured 850 us/round on HIGGS (~30x this kernel's memory
  // cost). Counts per WG stay far below 2^32.
  extern __shared__ unsigned int lds_auc[];
  for (int i = threadIdx.x; i < 2 * B; i += blockDim.x) lds_auc[i] = 0u;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const double p = 1.0 / (1.0 + exp(-(double)margin[i]));
    long long b = (long long)(p * (double)B);  // trunc, matches .long()
    if (b > B - 1) b = B - 1;
    if (b < 0) b = 0;
    const int pos = label[i] > 0.5f ? 1 : 0;
    atomicAdd(&lds_auc[(size_t)pos * B + b], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * B; i += blockDim.x) {
    const unsigned int v = lds_auc[i];
    if (v)
      atomicAdd((unsigned long long*)&hist[i], (unsigned long long)v);
  }
}

torch::Tensor eval_auc_hist(torch::Tensor margin, torch::Tensor label,
                            int64_t n_bins) {
  const int64_t n = margin.numel();
  auto dev = margin.device();
  // two u32 planes of n_bins in dynamic LDS; a larger request fails the
  // launch and would leave the histogram all zero
  constexpr int64_t kAucLdsBytes = 160 * 1024;
  TORCH_CHECK(n_bins >= 1 &&
                  2 * n_bins * (int64_t)sizeof(unsigned int) <= kAucLdsBytes,
              "eval_auc_hist: n_bins must be in [1, ",
              kAucLdsBytes / (2 * (int64_t)sizeof(unsigned int)), "], got ",
              n_bins);
  auto hist = torch::zeros(
      {2 * n_bins},
      torch::TensorOptions().dtype(torch::kInt64).device(dev));
  if (n == 0) return hist;
  auto stream = c10::hip::getCurrentHIPStream();
  const size_t lds = 2 * (size_t)n_bins * sizeof(unsigned int);
  static bool lds_attr_set = false;
  if (!lds_attr_set) {
    // dynamic LDS above 64 KiB needs the opt-in attribute (160 KiB/CU)
    CHECK_HIP(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&eval_auc_hist_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAucLdsBytes));
    lds_attr_set = true;
  }
  const int64_t blocks = std::min<int64_t>(ceil_div(n, 256 * 64), 256);
  hipLaunchKernelGGL(eval_auc_hist_kernel, dim3((uint32_t)blocks),
                     dim3(256), lds, stream.stream(),
                     margin.data_ptr<float>(), label.data_ptr<float>(),
                     reinterpret_cast<long long*>(hist.data_ptr<int64_t>()),
                     (int)n_bins, n);
  CHECK_HIP(hipGetLastError());
  return hist;  // [neg | pos] planes
}


// ---------------------------------------------------------------------------
// depth_step: one C++ call runs a whole depth of the fused single-sync
// loop - stage control data, zero+build the histogram, derive siblings,
// scan, plan+partition, enqueue the pull and record the pull event,
// then launch the scatter. The python loop's ~30 torch/pybind dispatches
// per depth (~100 us of host time each depth) collapse to one call +
// one wait + numpy bookkeeping. Single-GPU only: the distributed path
// keeps the python structure (it interleaves the RCCL allreduce).
// ---------------------------------------------------------------------------
static hipEvent_t g_pull_event = nullptr;

void wait_pull_event() {
  if (g_pull_event) (void)hipEventSynchronize(g_pull_event);
}

std::vector<torch::Tensor> depth_step(
    torch::Tensor bins, torch::Tensor bins_t, torch::Tensor gseg,
    torch::Tensor ridx, torch::Tensor ridx_dest, torch::Tensor prev_hist,
    torch::Tensor hist, torch::Tensor depth_meta_cpu, int64_t KK,
    int64_t nd, int64_t K_built, torch::Tensor starts_cpu,
    torch::Tensor counts_cpu, torch::Tensor fb, double scale_g,
    double scale_h, double lam, double alpha, double gamma, double mcw,
    torch::Tensor mono, torch::Tensor bounds, torch::Tensor allowed,
    int64_t n_bins, int64_t chunk_bound, bool fused_glue) {
  auto dev = bins.device();
  auto stream = c10::hip::getCurrentHIPStream();
  const int F = (int)bins.size(1);

  // ONE pinned H2D for all of this depth's control data
  static thread_local PinnedStager depth_meta_stager;
  auto meta_cpu_pin = depth_meta_stager.get(depth_meta_cpu.numel());
  meta_cpu_pin.copy_(depth_meta_cpu);
  auto dmeta = meta_cpu_pin.to(dev, /*non_blocking=*/true);
  depth_meta_stager.mark(stream.stream());
  // layout: [sumg KK | sumh KK | starts KK | counts KK | pslot nd | sib nd]
  auto pg = dmeta.narrow(0, 0, KK);
  auto ph = dmeta.narrow(0, KK, KK);
  auto d_starts = dmeta.narrow(0, 2 * KK, KK);
  auto d_counts = dmeta.narrow(0, 3 * KK, KK);

  // built block: zero + histogram
  hist.narrow(0, 0, K_built).zero_();
  build_histogram(bins, gseg, ridx, starts_cpu, counts_cpu, n_bins, 0, F,
                  hist, /*pregathered=*/true);
  // sibling = parent - built: inside the scan kernel (fused_glue) or as
  // torch index_select + sub
  OptTensor d_prev, d_pslots, d_spos;
  if (nd > 0) {
    auto pslots = dmeta.narrow(0, 4 * KK, nd);
    auto spos = dmeta.narrow(0, 4 * KK + nd, nd);
    if (fused_glue) {
      d_prev = prev_hist;
      d_pslots = pslots;
      d_spos = spos;
    } else {
      auto derived = hist.narrow(0, K_built, nd);
      torch::sub_out(derived, prev_hist.index_select(0, pslots),
                     hist.index_select(0, spos));
    }
  }
  // scan + device-planned partition (writes into ridx_dest, no clones)
  std::vector<torch::Tensor> st;
  if (fused_glue) {
    auto kf = find_splits_kf(hist, pg, ph, fb, scale_g, scale_h, lam, alpha,
                             gamma, mcw, mono, bounds, allowed, d_prev,
                             d_pslots, d_spos, c10::nullopt, c10::nullopt);
    st = partition_rows_from_kf(bins, ridx, d_starts, d_counts, kf[0], kf[1],
                                kf[2], kf[3], kf[4], gseg, bins_t,
                                chunk_bound, ridx_dest);
  } else {
    auto fs = find_splits(hist, pg, ph, fb, scale_g, scale_h, lam, alpha,
                          gamma, mcw, mono, bounds, allowed,
                          /*pull=*/false, c10::nullopt, c10::nullopt,
                          c10::nullopt);
    st = partition_rows_from_packed(bins, ridx, d_starts, d_counts, fs[0],
                                    gseg, bins_t, chunk_bound, ridx_dest,
                                    /*fused_glue=*/false);
  }
  // record the pull event BETWEEN the pull copies and the scatter
  if (!g_pull_event)
    (void)hipEventCreateWithFlags(&g_pull_event, hipEventDisableTiming);
  (void)hipEventRecord(g_pull_event, stream.stream());
  partition_scatter_planned(ridx, st[0], gseg, st[1], st[3], st[4], st[5],
                            st[6], st[7], chunk_bound);
  return {st[0], st[1], st[2]};
}

// ---------------------------------------------------------------------------
// Whole-tree enqueue: every level of a depthwise tree goes onto the stream
// in one call, with no host round trip between depths. Depth d+1's
// launches read their frontier from what plan_next_depth_kernel wrote at
// depth d; grids are host-known BOUNDS (frontier <= 2^d, histogram chunks
// <= ceil(n / rows_per_wg) + built nodes, partition chunks <=
// ceil(n / PART_CHUNK) + frontier) and excess workgroups exit on the
// device limits. Each depth's {packed | left totals} record is copied to
// its own pinned slot and followed by its own event, so the host replays
// depth d's bookkeeping behind the GPU while deeper levels run. The last
// level runs histogram, scan, reduce and pull only (row-order finish).
// A depth whose frontier emptied runs as empty launches.
// ---------------------------------------------------------------------------
#define TREE_ENQUEUE_MAX_DEPTH 10  // frontier bound 2^9 <= RP_THREADS

struct TreeEnqueueState {
  torch::Tensor pin;            // [2 root sums | depth 0: 7 | depth 1: 14 ..]
  std::vector<hipEvent_t> ev;   // one per depth
};
static thread_local TreeEnqueueState g_tree_enq;

// {histogram flavour has the limits form (0/1), its rows per workgroup}
std::vector<int64_t> tree_enqueue_config(torch::Tensor bins, int64_t n_bins) {
  if (!on_gpu(bins) || bins.dim() != 2) return {0, 0};
  const HistConfig hc = hist_config(bins, n_bins, 0, bins.size(1), 1);
  return {hc.xcd ? 1 : 0, hc.rows_per_wg};
}

// test entry: one plan_next_depth_kernel launch. Outputs are sized for the
// largest next frontier (every node splits) and pre-filled with -1.
std::vector<torch::Tensor> plan_next_depth(torch::Tensor packed,
                                           torch::Tensor dmeta,
                                           torch::Tensor limits,
                                           torch::Tensor node_left_total,
                                           int64_t rows_per_wg) {
  const int64_t KKb = packed.size(0);
  TORCH_CHECK(on_gpu(packed) && on_gpu(dmeta) && on_gpu(limits) &&
                  on_gpu(node_left_total) && packed.is_contiguous() &&
                  dmeta.is_contiguous() && packed.dim() == 2 &&
                  packed.size(1) == 6 && KKb >= 1 && KKb <= RP_THREADS &&
                  packed.scalar_type() == torch::kInt64 &&
                  dmeta.scalar_type() == torch::kInt64 &&
                  limits.scalar_type() == torch::kInt64 &&
                  node_left_total.scalar_type() == torch::kInt64 &&
                  limits.numel() >= 3 && dmeta.numel() >= 4 * KKb &&
                  node_left_total.numel() >= KKb && rows_per_wg >= 1,
              "plan_next_depth: bad arguments");
  auto optsl = torch::TensorOptions().dtype(torch::kInt64).device(packed.device());
  auto dm_n = torch::full({10 * KKb}, -1, optsl);
  auto hm_n = torch::full({3 * KKb + 1}, -1, optsl);
  auto lim_n = torch::full({3}, -1, optsl);
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(plan_next_depth_kernel, dim3(1), dim3(RP_THREADS), 0,
                     stream.stream(),
                     reinterpret_cast<const long long*>(packed.data_ptr<int64_t>()),
                     dmeta.data_ptr<int64_t>(), limits.data_ptr<int64_t>(),
                     node_left_total.data_ptr<int64_t>(),
                     dm_n.data_ptr<int64_t>(), hm_n.data_ptr<int64_t>(),
                     lim_n.data_ptr<int64_t>(), (int)rows_per_wg);
  return {dm_n, hm_n, lim_n};
}

// test entry: the XCD histogram kernel in its device-limit form. hist's
// leading size bounds the built-node count, chunk_bound the row chunks.
torch::Tensor build_histogram_limits(torch::Tensor bins, torch::Tensor gseg,
                                     torch::Tensor ridx, torch::Tensor hmeta,
                                     torch::Tensor limits, int64_t n_bins,
                                     torch::Tensor hist, int64_t chunk_bound) {
  const int F = (int)bins.size(1);
  const int Kb = (int)hist.size(0);
  const HistConfig hc = hist_config(bins, n_bins, 0, F, Kb);
  TORCH_CHECK(hc.xcd, "build_histogram_limits: only the XCD flavour has the "
                      "device-limit form");
  TORCH_CHECK(on_gpu(bins) && on_gpu(gseg) && on_gpu(ridx) && on_gpu(hmeta) &&
                  on_gpu(limits) && on_gpu(hist) && hist.is_contiguous() &&
                  hist.dim() == 4 && hist.size(1) == F &&
                  hist.size(2) == n_bins && hist.size(3) == 2 &&
                  hmeta.scalar_type() == torch::kInt64 &&
                  limits.scalar_type() == torch::kInt64 &&
                  limits.numel() >= 3 && hmeta.numel() >= 3 * (int64_t)Kb + 1 &&
                  gseg.scalar_type() == torch::kInt32 &&
                  ridx.scalar_type() == torch::kInt32 && chunk_bound >= 0,
              "build_histogram_limits: bad arguments");
  auto stream = c10::hip::getCurrentHIPStream();
  launch_hist_xcd(hc, bins, (const int2*)gseg.data_ptr<int32_t>(),
                  ridx.data_ptr<int32_t>(), hmeta.data_ptr<int64_t>(), nullptr,
                  reinterpret_cast<long long*>(hist.data_ptr<int64_t>()), Kb,
                  (int)n_bins, 0, F, chunk_bound, limits.data_ptr<int64_t>(),
                  stream.stream());
  return hist;
}

void tree_enqueue_wait(int64_t depth) {
  TORCH_CHECK(depth >= 0 && depth < (int64_t)g_tree_enq.ev.size(),
              "tree_enqueue_wait: no such depth");
  CHECK_HIP(hipEventSynchronize(g_tree_enq.ev[depth]));
}

// Returns the pinned record buffer: [sumg, sumh of the root | depth 0's
// 7 entries | depth 1's 14 | ...]; depth d's slot starts at
// 2 + 7 * (2^d - 1), holds packed rows at [6k, 6k+6) and the left totals
// (compact split order) from 6 * 2^d on, and is valid once
// tree_enqueue_wait(d) returns. The root sums are valid with depth 0.
torch::Tensor tree_enqueue(
    torch::Tensor bins, torch::Tensor bins_t, torch::Tensor gseg,
    torch::Tensor ridx_a, torch::Tensor ridx_b, torch::Tensor root_sum,
    int64_t max_depth, torch::Tensor fb, double scale_g, double scale_h,
    double lam, double alpha, double gamma, double mcw, int64_t n_bins) {
  const int D = (int)max_depth;
  const int F = (int)bins.size(1);
  const int64_t n_local = ridx_a.numel();
  TORCH_CHECK(D >= 1 && D <= TREE_ENQUEUE_MAX_DEPTH,
              "tree_enqueue: max_depth must be in [1, 10]");
  TORCH_CHECK(on_gpu(bins) && bins.dtype() == torch::kUInt8 &&
                  on_gpu(gseg) && gseg.scalar_type() == torch::kInt32 &&
                  gseg.is_contiguous() && gseg.dim() == 2 &&
                  gseg.size(0) == n_local && gseg.size(1) == 2 &&
                  on_gpu(ridx_a) && on_gpu(ridx_b) &&
                  ridx_a.scalar_type() == torch::kInt32 &&
                  ridx_b.scalar_type() == torch::kInt32 &&
                  ridx_b.numel() == n_local && n_local > 0 &&
                  ridx_a.data_ptr() != ridx_b.data_ptr() &&
                  on_gpu(root_sum) && root_sum.scalar_type() == torch::kInt64 &&
                  root_sum.numel() == 2 && root_sum.is_contiguous() &&
                  on_gpu(fb) && fb.scalar_type() == torch::kInt32 &&
                  fb.numel() == F && fb.is_contiguous(),
              "tree_enqueue: bad arguments");
  const HistConfig hc = hist_config(bins, n_bins, 0, F, 1);
  TORCH_CHECK(hc.xcd, "tree_enqueue: the selected histogram flavour has no "
                      "device-limit form");
  auto dev = bins.device();
  auto stream = c10::hip::getCurrentHIPStream();
  auto optsl = torch::TensorOptions().dtype(torch::kInt64).device(dev);
  const int rows = hc.rows_per_wg;

  auto& S = g_tree_enq;
  const int64_t total = 2 + 7 * (((int64_t)1 << D) - 1);
  if (!S.pin.defined() || S.pin.numel() < total)
    S.pin = torch::empty({total}, torch::TensorOptions()
                                      .dtype(torch::kInt64)
                                      .pinned_memory(true));
  while ((int)S.ev.size() < D) {
    hipEvent_t e = nullptr;
    CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    S.ev.push_back(e);
  }

  // at most two bound-sized histograms live: depth d in buffer d & 1,
  // its parent level in the other
  int64_t hn[2] = {0, 0};
  for (int d = 0; d < D; ++d) hn[d & 1] = (int64_t)1 << d;
  torch::Tensor hb[2];
  for (int p = 0; p < 2; ++p)
    if (hn[p]) hb[p] = torch::empty({hn[p], F, n_bins, 2}, optsl);

  auto e64 = torch::empty({0}, optsl);
  auto mono = torch::empty({0}, optsl.dtype(torch::kInt8));
  auto bounds = torch::empty({0, 2}, optsl.dtype(torch::kFloat64));
  auto allowed = torch::empty({0}, optsl.dtype(torch::kUInt8));

  auto dm = torch::empty({5}, optsl);
  auto hm = torch::empty({4}, optsl);
  auto lim = torch::empty({3}, optsl);
  auto root_out = torch::empty({2}, optsl);
  hipLaunchKernelGGL(plan_root_kernel, dim3(1), dim3(1), 0, stream.stream(),
                     root_sum.data_ptr<int64_t>(), n_local, rows,
                     dm.data_ptr<int64_t>(), hm.data_ptr<int64_t>(),
                     lim.data_ptr<int64_t>(), root_out.data_ptr<int64_t>());
  S.pin.narrow(0, 0, 2).copy_(root_out, /*non_blocking=*/true);

  torch::Tensor cur_r = ridx_a, other_r = ridx_b, cur_g = gseg;
  for (int d = 0; d < D; ++d) {
    const int64_t KKb = (int64_t)1 << d;        // frontier bound
    const int64_t Kb = d ? KKb / 2 : 1;         // built-node bound
    const bool last = d == D - 1;
    auto hist = hb[d & 1].narrow(0, 0, KKb);
    hist.narrow(0, 0, Kb).zero_();  // one fill over the bound
    launch_hist_xcd(hc, bins, (const int2*)cur_g.data_ptr<int32_t>(),
                    cur_r.data_ptr<int32_t>(), hm.data_ptr<int64_t>(), nullptr,
                    reinterpret_cast<long long*>(hist.data_ptr<int64_t>()),
                    (int)Kb, (int)n_bins, 0, F, ceil_div(n_local, rows) + Kb,
                    lim.data_ptr<int64_t>(), stream.stream());
    OptTensor prev;
    if (d) prev = hb[(d - 1) & 1].narrow(0, 0, KKb / 2);
    auto kf = find_splits_kf(hist, e64, e64, fb, scale_g, scale_h, lam, alpha,
                             gamma, mcw, mono, bounds, allowed, prev,
                             c10::nullopt, c10::nullopt, lim, dm);
    auto rp = reduce_plan_limits(kf[0], kf[1], kf[2], kf[3], kf[4], dm, lim,
                                 KKb);
    auto slot = S.pin.narrow(0, 2 + 7 * (KKb - 1), 7 * KKb);
    if (last) {
      slot.narrow(0, 0, 6 * KKb)
          .copy_(rp[3].narrow(0, 0, 6 * KKb), /*non_blocking=*/true);
      CHECK_HIP(hipEventRecord(S.ev[d], stream.stream()));
      break;
    }
    const int64_t cb = ceil_div(n_local, PART_CHUNK) + KKb;
    auto st = partition_planned(bins, cur_r, rp[0], rp[1], rp[2], rp[3], cur_g,
                                bins_t, cb, other_r, /*fused=*/true,
                                /*stage_pull=*/false);
    auto dm_n = torch::empty({10 * KKb}, optsl);
    auto hm_n = torch::empty({3 * KKb + 1}, optsl);
    auto lim_n = torch::empty({3}, optsl);
    hipLaunchKernelGGL(plan_next_depth_kernel, dim3(1), dim3(RP_THREADS), 0,
                       stream.stream(),
                       reinterpret_cast<const long long*>(rp[0].data_ptr<int64_t>()),
                       dm.data_ptr<int64_t>(), lim.data_ptr<int64_t>(),
                       st[6].data_ptr<int64_t>(), dm_n.data_ptr<int64_t>(),
                       hm_n.data_ptr<int64_t>(), lim_n.data_ptr<int64_t>(),
                       rows);
    // the pull and its event go BEFORE the scatter: the host's replay of
    // this depth overlaps it
    slot.copy_(rp[3], /*non_blocking=*/true);
    CHECK_HIP(hipEventRecord(S.ev[d], stream.stream()));
    partition_scatter_planned(cur_r, st[0], cur_g, st[1], st[3], st[4], st[5],
                              st[6], st[7], cb);
    other_r = cur_r;
    cur_r = st[0];
    cur_g = st[1];
    dm = dm_n;
    hm = hm_n;
    lim = lim_n;
  }
  CHECK_HIP(hipGetLastError());
  return S.pin.narrow(0, 0, total);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("quantize_gpair", &quantize_gpair, "quantize gradient pairs");
  m.def("quantize_gpair_sums", &quantize_gpair_sums,
        "quantize gradient pairs, also returning their int64 column sums");
  m.def("apply_tree_binned", &apply_tree_binned,
        "row-order tree walk over the binned matrix, added into the margin");
  m.def("grad_fused", &grad_fused, "fused objective gradient + absmax");
  m.def("eval_logloss", &eval_logloss, "fused logloss eval");
  m.def("eval_auc_hist", &eval_auc_hist, "fused AUC score histograms");
  m.def("bin_matrix", &bin_matrix, "bin feature matrix");
  m.def("build_histogram", &build_histogram, "build gradient histograms");
  m.def("find_splits", &find_splits, "best-split scan", py::arg("hist"),
        py::arg("parent_g"), py::arg("parent_h"), py::arg("feat_bins"),
        py::arg("scale_g"), py::arg("scale_h"), py::arg("lam"),
        py::arg("alpha"), py::arg("gamma"), py::arg("mcw"), py::arg("mono"),
        py::arg("bounds"), py::arg("allowed"), py::arg("pull"),
        py::arg("prev_hist") = py::none(), py::arg("pslots") = py::none(),
        py::arg("spos") = py::none());
  m.def("find_splits_kf", &find_splits_kf,
        "(node, feature) split scan without the per-node reduce",
        py::arg("hist"), py::arg("parent_g"), py::arg("parent_h"),
        py::arg("feat_bins"), py::arg("scale_g"), py::arg("scale_h"),
        py::arg("lam"), py::arg("alpha"), py::arg("gamma"), py::arg("mcw"),
        py::arg("mono"), py::arg("bounds"), py::arg("allowed"),
        py::arg("prev_hist") = py::none(), py::arg("pslots") = py::none(),
        py::arg("spos") = py::none(), py::arg("limits") = py::none(),
        py::arg("dmeta") = py::none());
  m.def("reduce_plan_limits", &reduce_plan_limits,
        "reduce+plan kernel with a device-resident frontier size");
  m.def("build_histogram_limits", &build_histogram_limits,
        "XCD histogram kernel with device-resident node and chunk counts");
  m.def("plan_next_depth", &plan_next_depth,
        "next depth's scan/histogram metadata from this depth's splits");
  m.def("tree_enqueue_config", &tree_enqueue_config,
        "{histogram flavour supports the tree enqueue, rows per workgroup}");
  m.def("tree_enqueue", &tree_enqueue,
        "enqueue every level of a depthwise tree without host round trips");
  m.def("tree_enqueue_wait", &tree_enqueue_wait,
        "host wait for one depth's pull of the last tree_enqueue");
  m.def("reduce_plan_fused", &reduce_plan_fused,
        "per-node best split + partition plan, one kernel at K <= 1024");
  m.def("reduce_plan_legacy", &reduce_plan_legacy,
        "per-node best split + partition plan, the two separate kernels");
  m.def("partition_rows", &partition_rows, "stable row partition");
  m.def("partition_rows_begin", &partition_rows_begin,
        "count+prefix phase (returns before the host sync)");
  m.def("partition_rows_finish", &partition_rows_finish,
        "left-totals pull + scatter phase");
  m.def("partition_rows_from_packed", &partition_rows_from_packed,
        "device-planned partition consuming find_splits packed output",
        py::arg("bins"), py::arg("ridx"), py::arg("starts_ord"),
        py::arg("counts_ord"), py::arg("packed"), py::arg("gseg"),
        py::arg("bins_t"), py::arg("chunk_bound"), py::arg("ridx_dest"),
        py::arg("fused_glue") = false);
  m.def("partition_rows_from_kf", &partition_rows_from_kf,
        "device-planned partition consuming find_splits_kf output");
  m.def("partition_scatter_planned", &partition_scatter_planned,
        "scatter phase of the device-planned partition, integer chunk bound");
  m.def("partition_scatter_from_packed", &partition_scatter_from_packed,
        "scatter phase of the device-planned partition");
  m.def("depth_step", &depth_step,
        "one fused single-sync depth (single-GPU fast path)",
        py::arg("bins"), py::arg("bins_t"), py::arg("gseg"), py::arg("ridx"),
        py::arg("ridx_dest"), py::arg("prev_hist"), py::arg("hist"),
        py::arg("depth_meta_cpu"), py::arg("KK"), py::arg("nd"),
        py::arg("K_built"), py::arg("starts_cpu"), py::arg("counts_cpu"),
        py::arg("fb"), py::arg("scale_g"), py::arg("scale_h"), py::arg("lam"),
        py::arg("alpha"), py::arg("gamma"), py::arg("mcw"), py::arg("mono"),
        py::arg("bounds"), py::arg("allowed"), py::arg("n_bins"),
        py::arg("chunk_bound"), py::arg("fused_glue") = false);
  m.def("wait_pull_event", &wait_pull_event,
        "host wait for the depth_step pull event");
  m.def("predict_trees", &predict_trees, "tree-walk prediction");
  py::class_<WalkForest>(m, "WalkForest")
      .def_readonly("lds_nodes", &WalkForest::lds_nodes)
      .def_readonly("tile_nodes", &WalkForest::tile_nodes);
  m.def("walk_pack", &walk_pack,
        "pack and tile a forest for predict_leaf / saabas_contribs");
  m.def("predict_leaf", &predict_leaf, "tree-walk leaf indices");
  m.def("saabas_contribs", &saabas_contribs,
        "tree-walk Saabas attributions, accumulated into out",
        py::arg("X"), py::arg("forest"), py::arg("node_mean"),
        py::arg("out"), py::arg("lds_acc"), py::arg("threads"));
  m.attr("PRED_TILE_NODES") = PRED_TILE_NODES;
  m.attr("SAABAS_LDS_BYTES") = SAABAS_LDS_BYTES;
  m.def("tree_shap", &tree_shap,
        "path-form exact TreeSHAP (contributions or interactions)");
  m.attr("SHAP_TILE_ELEMS") = SHAP_TILE_ELEMS;
  m.attr("SHAP_MAX_PATH_LEN") = SHAP_MAX_PATH_LEN;
  m.def("update_margins", &update_margins, "leaf margin update");
  m.def("leaf_quantile_hist", &leaf_quantile_hist,
        "per-leaf radix-select digit histogram (one pass)");
  m.def("mvs_score", &mvs_score, "gradient-based sampling: row scores");
  m.def("mvs_stats", &mvs_stats,
        "gradient-based sampling: (#nonzero, max, sum) of the scores");
  m.def("mvs_hist", &mvs_hist,
        "gradient-based sampling: one radix-select pass over the scores");
  m.def("mvs_sample", &mvs_sample,
        "gradient-based sampling: keep mask + reweighted gradient pairs");
  m.def("lambdarank_grad", &lambdarank_grad, "pairwise lambdarank gradients");
}
