// Multiclass AUC / AUCPR score histograms for AMD Instinct MI355X (CDNA4,
// gfx950): one-vs-rest [K, 2, B] histograms of the softmax probabilities of
// an [n, K] margin. Built as its own extension module
// (xgboost_ray_amd._hip_auc_ops), so that adding it leaves the build lines
// and the generated code of the other modules as they were.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <cstdint>
#include <limits>

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
// Contract: docs/parity.md "Multiclass AUC on the device".
//
// The binary eval_auc_hist_kernel keeps two u32 planes of 16384 bins in LDS,
// 128 of the 160 KiB: room for one class. K classes need K such histograms,
// and a workgroup that counted one class straight from the margin would read
// whole [n, K] rows for one value each, K times over. So the work is split:
//
// 1. auc_bin_rows_kernel reads the margin once. A workgroup of R threads owns
//    R consecutive rows, stages them through an odd-pitch float64 LDS tile
//    (consecutive lanes read consecutive addresses; thread r then walks row r
//    with lane = bank), forms each row's softmax once and writes one u16 code
//    per (class, row) into a class-major buffer: bin | positive << 15. For
//    one class a wave stores 64 consecutive codes, 128 contiguous bytes.
// 2. auc_count_kernel has a grid of row segments x classes (x planes when
//    weighted). A workgroup streams its class's codes, 8 to a 16-byte load,
//    counts into an LDS histogram and merges it once into the global
//    [K, 2, B] with skip-if-zero 64-bit atomics.
//
// Every sum is an integer sum, so atomics in any order, any row chunking and
// any sharding give equal bytes.
// ---------------------------------------------------------------------------
#define AUC_CHUNK_CLASSES 16       // classes per LDS chunk of the row kernel
#define AUC_MAX_CHUNK 64
#define AUC_MAX_ROWS 256           // rows (= threads) of a tile
#define AUC_ROWS_LDS_BYTES (64 * 1024)
#define AUC_ROWS_MAX_BLOCKS 4096
#define AUC_MAX_BINS 16384         // 14 bits of a code
#define AUC_POS_BIT 0x8000u
#define AUC_COUNT_THREADS 1024
#define AUC_COUNT_LDS_BYTES (128 * 1024)
#define AUC_CODES_PER_LOAD 8       // u16 codes of one 16-byte load
// Rows of a count workgroup: a multiple of the codes per load, and far below
// 2^32 so that a u32 LDS count cannot wrap.
#define AUC_COUNT_MIN_ROWS (1 << 16)
#define AUC_COUNT_MAX_ROWS (int64_t(1) << 30)
#define AUC_WEIGHT_SCALE 1048576.0  // 2^20

// The class a label names: truncated toward zero as .long() does, -1 (no
// class) outside [0, K) and for NaN. The result is only ever compared.
__device__ __forceinline__ int label_class(float y, int K) {
  return (y > -1.f && y < (float)K) ? (int)y : -1;
}

// Stage classes [c0, c0 + kc) of rows [row0, row0 + R) into tile[r * pitch +
// k]; rows from `rows` on are filled with zeros. Flat element i = r * kc + k
// goes to thread i % T, so a wave reads 64 consecutive elements of the chunk:
// one contiguous run when kc == K, else runs of kc floats. (r, k) advance by
// T without a division per element.
__device__ __forceinline__ void stage_tile(const float* __restrict__ margin,
                                           double* __restrict__ tile,
                                           int64_t row0, int rows, int R,
                                           int K, int c0, int kc, int pitch) {
  const int T = blockDim.x;
  const int dq = T / kc, dr = T % kc;
  int r = threadIdx.x / kc, k = threadIdx.x % kc;
  const int total = R * kc;
#pragma unroll 4
  for (int i = threadIdx.x; i < total; i += T) {
    float v = 0.f;
    if (r < rows) v = margin[(row0 + r) * (int64_t)K + c0 + k];
    tile[r * pitch + k] = (double)v;
    r += dq;
    k += dr;
    if (k >= kc) {
      k -= kc;
      ++r;
    }
  }
}

// bin | positive << 15 of one probability. The comparison keeps NaN (and
// anything below the first inner edge) in bin 0, so no address made from the
// code depends on a NaN.
__device__ __forceinline__ unsigned short auc_code(double p, int B,
                                                   bool positive) {
  const double t = p * (double)B;
  unsigned int b = 0u;
  if (t >= 1.0) {
    const double top = (double)(B - 1);
    b = (unsigned int)(t < top ? t : top);  // trunc
  }
  return (unsigned short)(b | (positive ? AUC_POS_BIT : 0u));
}

__global__ __launch_bounds__(AUC_MAX_ROWS) void auc_bin_rows_kernel(
    const float* __restrict__ margin,    // [n, K]
    const float* __restrict__ label,     // [n]
    unsigned short* __restrict__ codes,  // [K, pitch], pitch >= n
    int64_t n, int64_t pitch, int K, int KC, int B, int64_t ntiles) {
  extern __shared__ double tile[];  // [R][pitch_k]
  const int R = blockDim.x, r = threadIdx.x;
  const int kcw = K < KC ? K : KC;  // widest chunk
  const int pk = kcw | 1;
  const bool single = K <= KC;
  double* my = tile + r * pk;

  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * R;
    const int rows = (int)(n - row0 < R ? n - row0 : R);
    const bool valid = r < rows;
    const int64_t row = row0 + r;
    const int yi = valid ? label_class(label[row], K) : -1;

    float m = -std::numeric_limits<float>::infinity();
    double s = 0.0;
    if (single) {
      stage_tile(margin, tile, row0, rows, R, K, 0, K, pk);
      __syncthreads();
      for (int k = 0; k < K; ++k) {
        const float x = (float)my[k];
        if (x > m) m = x;
      }
      const double md = (double)m;
      for (int k = 0; k < K; ++k) {
        const double e = exp(my[k] - md);
        my[k] = e;
        s += e;
      }
      if (valid) {
        for (int k = 0; k < K; ++k)
          codes[(int64_t)k * pitch + row] = auc_code(my[k] / s, B, k == yi);
      }
    } else {
      // sweep 1 keeps the maximum, sweep 2 forms the plain ascending sum
      // against it (no rescaling: s has the bits of the one-chunk form),
      // sweep 3 the probabilities
      for (int sweep = 0; sweep < 3; ++sweep) {
        const double md = (double)m;
        for (int c0 = 0; c0 < K; c0 += KC) {
          const int kc = K - c0 < KC ? K - c0 : KC;
          __syncthreads();  // the tile's readers are done
          stage_tile(margin, tile, row0, rows, R, K, c0, kc, pk);
          __syncthreads();
          if (sweep == 0) {
            for (int k = 0; k < kc; ++k) {
              const float x = (float)my[k];
              if (x > m) m = x;
            }
          } else if (sweep == 1) {
            for (int k = 0; k < kc; ++k) s += exp(my[k] - md);
          } else if (valid) {
            for (int k = 0; k < kc; ++k)
              codes[(int64_t)(c0 + k) * pitch + row] =
                  auc_code(exp(my[k] - md) / s, B, c0 + k == yi);
          }
        }
      }
    }
    __syncthreads();  // before the next tile is staged over this one
  }
}

// Count one class's codes of rows [blockIdx.x * seg, +seg) into LDS, then
// merge. Unweighted: both u32 planes, [neg | pos]. Weighted: the one u64
// plane that blockIdx.z names, fed W = llrint(w * 2^20).
template <bool WEIGHTED>
__global__ __launch_bounds__(AUC_COUNT_THREADS) void auc_count_kernel(
    const unsigned short* __restrict__ codes,  // [K, pitch]
    const float* __restrict__ weight,          // [n] when WEIGHTED
    unsigned long long* __restrict__ hist,     // [K, 2, B]
    int64_t n, int64_t pitch, int B, int64_t seg) {
  extern __shared__ unsigned int lds_u32[];
  unsigned long long* lds_u64 = (unsigned long long*)lds_u32;
  const int T = blockDim.x;
  const int k = blockIdx.y;
  const unsigned int plane = blockIdx.z;
  const int cells = WEIGHTED ? B : 2 * B;
  for (int i = threadIdx.x; i < cells; i += T) {
    if (WEIGHTED)
      lds_u64[i] = 0ull;
    else
      lds_u32[i] = 0u;
  }
  __syncthreads();

  const int64_t lo = (int64_t)blockIdx.x * seg;
  const int64_t hi = lo + seg < n ? lo + seg : n;
  const unsigned short* c = codes + (int64_t)k * pitch;
  const unsigned int top = (unsigned int)(B - 1);
  // a weight view may start off a 16-byte boundary: scalar loads then
  const bool w_vec = WEIGHTED && ((uintptr_t)weight & 15) == 0;
  // lo and every step are multiples of 8 and pitch is one too, so each load
  // is aligned and stays inside the class's row of the buffer; codes past
  // hi (the pad included) are read but never counted
  for (int64_t i = lo + (int64_t)threadIdx.x * AUC_CODES_PER_LOAD; i < hi;
       i += (int64_t)T * AUC_CODES_PER_LOAD) {
    const uint4 v = *reinterpret_cast<const uint4*>(c + i);
    const unsigned int q[4] = {v.x, v.y, v.z, v.w};
    const int live = (int)(hi - i < AUC_CODES_PER_LOAD ? hi - i
                                                        : AUC_CODES_PER_LOAD);
    float w[AUC_CODES_PER_LOAD];
    if (WEIGHTED) {
      if (w_vec && live == AUC_CODES_PER_LOAD) {
        const float4 a = *reinterpret_cast<const float4*>(weight + i);
        const float4 b = *reinterpret_cast<const float4*>(weight + i + 4);
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
        w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
      } else {
#pragma unroll
        for (int j = 0; j < AUC_CODES_PER_LOAD; ++j)
          w[j] = j < live ? weight[i + j] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < AUC_CODES_PER_LOAD; ++j) {
      if (j >= live) break;
      const unsigned int code = (q[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
      unsigned int b = code & (AUC_POS_BIT - 1u);
      if (b > top) b = top;  // a foreign code cannot leave the planes
      const unsigned int pos = code >> 15;
      if (WEIGHTED) {
        if (pos != plane) continue;
        const long long W = llrint((double)w[j] * AUC_WEIGHT_SCALE);
        if (W != 0)
          atomicAdd(&lds_u64[b], (unsigned long long)W);
      } else {
        atomicAdd(&lds_u32[pos * (unsigned int)B + b], 1u);
      }
    }
  }
  __syncthreads();

  unsigned long long* dst =
      hist + ((int64_t)k * 2 + (WEIGHTED ? plane : 0u)) * (int64_t)B;
  for (int i = threadIdx.x; i < cells; i += T) {
    const unsigned long long v = WEIGHTED ? lds_u64[i]
                                          : (unsigned long long)lds_u32[i];
    if (v) atomicAdd(&dst[i], v);
  }
}

static void check_bins(const char* op, int64_t n_bins) {
  TORCH_CHECK(n_bins >= 1 && n_bins <= AUC_MAX_BINS, op,
              ": n_bins must lie in [1, ", AUC_MAX_BINS, "], got ", n_bins);
}

// Codes int16 [K, pitch] (the u16 bit patterns), pitch = n rounded up to 8.
// chunk / rows override KC and R for the benchmark's sweep (0: the defaults).
torch::Tensor auc_bin_rows(torch::Tensor margin, torch::Tensor label,
                           int64_t n_bins, int64_t chunk, int64_t rows) {
  check_bins("auc_bin_rows", n_bins);
  if (chunk == 0) chunk = AUC_CHUNK_CLASSES;
  if (rows == 0) rows = AUC_MAX_ROWS;
  TORCH_CHECK(on_gpu(margin) && margin.scalar_type() == torch::kFloat32 &&
                  margin.dim() == 2 && margin.is_contiguous(),
              "auc_bin_rows: margin must be a contiguous float32 GPU matrix "
              "[n, K]");
  const int64_t n = margin.size(0), K = margin.size(1);
  TORCH_CHECK(K >= 2 && K <= 65535, "auc_bin_rows: K must lie in [2, 65535], "
              "got ", K);
  TORCH_CHECK(n <= (int64_t(1) << 40), "auc_bin_rows: too many rows: ", n);
  TORCH_CHECK(label.device() == margin.device() &&
                  label.scalar_type() == torch::kFloat32 &&
                  label.is_contiguous() && label.numel() == n,
              "auc_bin_rows: label must be a contiguous float32 [n] on "
              "margin's GPU");
  TORCH_CHECK(chunk >= 1 && chunk <= AUC_MAX_CHUNK,
              "auc_bin_rows: chunk must lie in [1, ", AUC_MAX_CHUNK, "], got ",
              chunk);
  const int kcw = (int)std::min<int64_t>(K, chunk);
  const size_t lds = (size_t)rows * (kcw | 1) * sizeof(double);
  TORCH_CHECK(rows >= WAVE && rows % WAVE == 0 && rows <= AUC_MAX_ROWS &&
                  lds <= AUC_ROWS_LDS_BYTES,
              "auc_bin_rows: tile rows must be a multiple of 64, at most ",
              AUC_MAX_ROWS, ", with a tile inside the LDS budget; got ", rows);
  const int64_t pitch = ceil_div(n, AUC_CODES_PER_LOAD) * AUC_CODES_PER_LOAD;
  auto codes = torch::empty(
      {K, pitch},
      torch::TensorOptions().dtype(torch::kInt16).device(margin.device()));
  if (n == 0) return codes;
  const int64_t ntiles = ceil_div(n, rows);
  const int64_t blocks = std::min<int64_t>(ntiles, AUC_ROWS_MAX_BLOCKS);
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(auc_bin_rows_kernel, dim3((uint32_t)blocks),
                     dim3((uint32_t)rows), lds, stream.stream(),
                     margin.data_ptr<float>(), label.data_ptr<float>(),
                     (unsigned short*)codes.data_ptr<int16_t>(), n, pitch,
                     (int)K, (int)chunk, (int)n_bins, ntiles);
  CHECK_HIP(hipGetLastError());
  return codes;
}

template <bool WEIGHTED>
static void launch_count(const torch::Tensor& codes, const float* weight,
                         torch::Tensor& hist, int64_t n, int64_t pitch, int B,
                         int64_t seg, int threads, dim3 grid) {
  static bool lds_attr_set = false;
  if (!lds_attr_set) {
    // dynamic LDS above 64 KiB needs the opt-in attribute (160 KiB/CU)
    CHECK_HIP(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&auc_count_kernel<WEIGHTED>),
        hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)AUC_COUNT_LDS_BYTES));
    lds_attr_set = true;
  }
  const size_t lds = (size_t)B * 8;  // 2 B u32, or B u64
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(
      auc_count_kernel<WEIGHTED>, grid, dim3((uint32_t)threads), lds,
      stream.stream(), (const unsigned short*)codes.data_ptr<int16_t>(),
      weight, (unsigned long long*)hist.data_ptr<int64_t>(), n, pitch, B, seg);
  CHECK_HIP(hipGetLastError());
}

// hist int64 [K, 2, B], planes [neg | pos], accumulated into: the counts of
// the first n codes of every class row. count_rows / threads override the
// rows and the threads of a workgroup (0: the defaults).
void auc_count(torch::Tensor codes, int64_t n, torch::Tensor weight,
               torch::Tensor hist, int64_t count_rows, int64_t threads) {
  TORCH_CHECK(on_gpu(codes) && codes.scalar_type() == torch::kInt16 &&
                  codes.dim() == 2 && codes.is_contiguous(),
              "auc_count: codes must be a contiguous int16 GPU matrix");
  const int64_t K = codes.size(0), pitch = codes.size(1);
  TORCH_CHECK(K >= 1 && K <= 65535 && n >= 0 && n <= pitch &&
                  pitch % AUC_CODES_PER_LOAD == 0 &&
                  ((uintptr_t)codes.data_ptr<int16_t>() & 15) == 0,
              "auc_count: codes must be what auc_bin_rows returned for n rows");
  TORCH_CHECK(hist.device() == codes.device() &&
                  hist.scalar_type() == torch::kInt64 && hist.dim() == 3 &&
                  hist.is_contiguous() && hist.size(0) == K &&
                  hist.size(1) == 2,
              "auc_count: hist must be a contiguous int64 [K, 2, n_bins] on "
              "the codes' GPU");
  const int64_t B = hist.size(2);
  check_bins("auc_count", B);
  const bool weighted = weight.numel() > 0;
  TORCH_CHECK(!weighted || (weight.device() == codes.device() &&
                            weight.scalar_type() == torch::kFloat32 &&
                            weight.is_contiguous() && weight.numel() == n),
              "auc_count: weight must be empty or a contiguous float32 [n] on "
              "the codes' GPU");
  if (threads == 0) threads = AUC_COUNT_THREADS;
  TORCH_CHECK(threads >= WAVE && threads % WAVE == 0 &&
                  threads <= AUC_COUNT_THREADS,
              "auc_count: threads must be a multiple of 64, at most ",
              AUC_COUNT_THREADS, ", got ", threads);
  if (n == 0) return;
  const int planes = weighted ? 2 : 1;
  int64_t seg = count_rows;
  if (seg == 0) {
    // Clearing and merging its planes is a workgroup's fixed cost (up to
    // 2 B cells and as many global atomics), and at 16384 bins the LDS
    // admits one workgroup per CU: so at most one workgroup per CU in all,
    // in equal segments, measured fastest (docs/parity.md)
    int cus = 0;
    CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                    codes.device().index()));
    const int64_t want = std::max<int64_t>(1, cus / (K * planes));
    seg = std::max<int64_t>(AUC_COUNT_MIN_ROWS, ceil_div(n, want));
  }
  TORCH_CHECK(seg >= AUC_CODES_PER_LOAD,
              "auc_count: count_rows must be at least ", AUC_CODES_PER_LOAD);
  seg = std::min<int64_t>(
      ceil_div(seg, AUC_CODES_PER_LOAD) * AUC_CODES_PER_LOAD,
      AUC_COUNT_MAX_ROWS);
  const int64_t segs = ceil_div(n, seg);
  TORCH_CHECK(segs <= (int64_t(1) << 31) - 1, "auc_count: too many segments");
  const dim3 grid((uint32_t)segs, (uint32_t)K, (uint32_t)planes);
  if (weighted)
    launch_count<true>(codes, weight.data_ptr<float>(), hist, n, pitch, (int)B,
                       seg, (int)threads, grid);
  else
    launch_count<false>(codes, nullptr, hist, n, pitch, (int)B, seg,
                        (int)threads, grid);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("auc_bin_rows", &auc_bin_rows,
        "u16 codes (bin | positive << 15) of a multiclass margin, class-major",
        py::arg("margin"), py::arg("label"), py::arg("n_bins"),
        py::arg("chunk") = 0, py::arg("rows") = 0);
  m.def("auc_count", &auc_count,
        "count class-major codes into int64 [K, 2, n_bins] histograms",
        py::arg("codes"), py::arg("n"), py::arg("weight"), py::arg("hist"),
        py::arg("count_rows") = 0, py::arg("threads") = 0);
  m.attr("AUC_MAX_BINS") = (int)AUC_MAX_BINS;
}
