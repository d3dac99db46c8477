// Multiclass kernels for AMD Instinct MI355X (CDNA4, gfx950): the fused
// softmax gradient with its per-class |g| / |h| maxima, and the mlogloss /
// merror sums. Built as its own extension module
// (xgboost_ray_amd._hip_softmax_ops), so that adding it leaves the build
// lines and the generated code of csrc/kernels.hip and csrc/rank as they were.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <cstdint>
#include <limits>
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
// Multiclass on the device (contract: docs/parity.md "Multiclass on the
// device").
//
// The margin is row-major [n, K] and a row's softmax is a thread's work, but
// a thread that read "its" row from global memory would make every wave load
// touch 64 lines (stride 4K bytes). So a workgroup of R threads owns a tile
// of R consecutive rows and stages it through LDS: consecutive lanes read
// consecutive global addresses (with K <= KC the tile is one contiguous run
// of R*K floats), and the values land in an LDS tile whose row pitch is odd
// (in elements), where thread r then walks row r with lane = bank.
//
// Classes are walked in chunks of at most KC. The gradient tile holds float64:
// with one chunk (K <= KC) e_k = exp(x_k - m) is computed once, kept in the
// tile for the sum and read back for g and h. With several chunks sweep A
// keeps a running (m, s) per row, rescaling s by exp(m_old - m_new) when the
// maximum grows, and sweep B stages every chunk again and forms e_k against
// the final m; that s is no longer the plain ascending sum, so K > KC is held
// to the error bound, not to the bits of the one-chunk form. One K takes one
// route, so equal inputs give equal bytes.
//
// Pairs are stored class-major, out[k][row]: for one k a wave writes 64
// consecutive float2, 512 contiguous bytes. When a thread has stored the
// pair of class k, its tile slot [r][k] (8 bytes) is free and takes
// (|g|, |h|); after the chunk each wave folds its 64 rows by column (lanes
// split into class x row-group, then a xor butterfly over the row groups),
// the waves are folded in wave order and the result is max-ed into this
// workgroup's own [K, 2] row of the partial buffer. Nothing is atomic; the
// partials are reduced by one max(0) afterwards. All maxima keep NaN.
// ---------------------------------------------------------------------------
// Tile constants, measured (docs/parity.md): a small chunk keeps the float64
// tile small and the occupancy high, which pays for the second read of the
// margin that K > KC costs; one-chunk tiles ran fastest with 192 rows,
// several-chunk tiles with 256.
#define SOFTMAX_CHUNK_CLASSES 16
#define SOFTMAX_MAX_CHUNK 64        // a chunk's classes fit one wave's lanes
#define SOFTMAX_MAX_ROWS 256        // rows (= threads) of a tile
#define SOFTMAX_ONE_CHUNK_ROWS 192
#define SOFTMAX_LDS_BYTES (64 * 1024)
#define SOFTMAX_MAX_BLOCKS 2048
#define SOFTMAX_PARTIAL_ELEMS (1 << 21)  // bound on blocks * K of the partials

// max(a, b) that returns NaN when either side is NaN
__device__ __forceinline__ float max_keep_nan(float a, float b) {
  return (b > a || b != b) ? b : a;
}

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
template <typename TT>
__device__ __forceinline__ void stage_tile(const float* __restrict__ margin,
                                           TT* __restrict__ tile,
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
    tile[r * pitch + k] = (TT)v;
    r += dq;
    k += dr;
    if (k >= kc) {
      k -= kc;
      ++r;
    }
  }
}

__global__ __launch_bounds__(SOFTMAX_MAX_ROWS) void softmax_grad_kernel(
    const float* __restrict__ margin,  // [n, K]
    const float* __restrict__ label,   // [n]
    const float* __restrict__ weight,  // [n], nullable
    float2* __restrict__ out,          // [K, n]
    float* __restrict__ part,          // [gridDim.x, K, 2]
    int64_t n, int K, int KC, int64_t ntiles) {
  extern __shared__ double smem[];
  const int R = blockDim.x, r = threadIdx.x;
  const int lane = r & (WAVE - 1), wv = r / WAVE, nw = R / WAVE;
  const int kcw = K < KC ? K : KC;  // widest chunk
  const int pitch = kcw | 1;
  const bool single = K <= KC;
  double* tile = smem;                          // [R][pitch]
  float* wred = (float*)(smem + R * pitch);     // [nw][kcw][2]
  double* my = tile + r * pitch;

  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * R;
    const int rows = (int)(n - row0 < R ? n - row0 : R);
    const bool valid = r < rows;
    const int64_t row = row0 + r;
    const int yi = valid ? label_class(label[row], K) : -1;
    const float w = (valid && weight) ? weight[row] : 1.f;

    // sweep A: running maximum and sum over the chunks
    float m = -std::numeric_limits<float>::infinity();
    double s = 0.0;
    for (int c0 = 0; c0 < K; c0 += KC) {
      const int kc = K - c0 < KC ? K - c0 : KC;
      if (c0 > 0) __syncthreads();  // the tile's readers are done
      stage_tile(margin, tile, row0, rows, R, K, c0, kc, pitch);
      __syncthreads();
      float cm = m;
      for (int k = 0; k < kc; ++k) {
        const float x = (float)my[k];
        if (x > cm) cm = x;
      }
      if (cm > m) {
        if (c0 > 0) s *= exp((double)m - (double)cm);
        m = cm;
      }
      const double md = (double)m;
      for (int k = 0; k < kc; ++k) {
        const double e = exp(my[k] - md);
        if (single) my[k] = e;
        s += e;
      }
    }

    // sweep B: pairs, and the chunk's column maxima
    for (int c0 = 0; c0 < K; c0 += KC) {
      const int kc = K - c0 < KC ? K - c0 : KC;
      if (!single) {
        __syncthreads();
        stage_tile(margin, tile, row0, rows, R, K, c0, kc, pitch);
        __syncthreads();
      }
      const double md = (double)m;
      for (int k = 0; k < kc; ++k) {
        const double e = single ? my[k] : exp(my[k] - md);
        const double p = e / s;
        float g = (float)(p - (c0 + k == yi ? 1.0 : 0.0));
        const double hh = 2.0 * p * (1.0 - p);
        float h = (float)(hh < 1e-16 ? 1e-16 : hh);  // NaN stays NaN
        if (weight != nullptr) {
          g *= w;
          h *= w;
        }
        float2 a = {0.f, 0.f};
        if (valid) {
          out[(int64_t)(c0 + k) * n + row] = {g, h};
          a = {fabsf(g), fabsf(h)};
        }
        ((float2*)my)[k] = a;
      }
      __syncthreads();
      // wave wv folds its 64 rows: lane = (row group, class)
      int kcp = 1;
      while (kcp < kc) kcp <<= 1;
      const int cl = lane & (kcp - 1), rg = lane / kcp, ngr = WAVE / kcp;
      float gm = 0.f, hm = 0.f;
      if (cl < kc) {
        for (int rr = rg; rr < WAVE; rr += ngr) {
          const float2 v =
              ((const float2*)(tile + (wv * WAVE + rr) * pitch))[cl];
          gm = max_keep_nan(gm, v.x);
          hm = max_keep_nan(hm, v.y);
        }
      }
      for (int off = kcp; off < WAVE; off <<= 1) {
        gm = max_keep_nan(gm, __shfl_xor(gm, off, WAVE));
        hm = max_keep_nan(hm, __shfl_xor(hm, off, WAVE));
      }
      if (lane < kc) {
        wred[(wv * kcw + lane) * 2] = gm;
        wred[(wv * kcw + lane) * 2 + 1] = hm;
      }
      __syncthreads();
      if (r < kc) {
        float g = wred[r * 2], h = wred[r * 2 + 1];
        for (int q = 1; q < nw; ++q) {
          g = max_keep_nan(g, wred[(q * kcw + r) * 2]);
          h = max_keep_nan(h, wred[(q * kcw + r) * 2 + 1]);
        }
        float* dst = part + ((int64_t)blockIdx.x * K + c0 + r) * 2;
        if (t != blockIdx.x) {  // a later tile of this workgroup
          g = max_keep_nan(g, dst[0]);
          h = max_keep_nan(h, dst[1]);
        }
        dst[0] = g;
        dst[1] = h;
      }
    }
    __syncthreads();  // before the next tile is staged over this one
  }
}

// mlogloss / merror sums: one sweep with the running (m, s), the lowest index
// of the maximum and the label's margin; the tile holds the float32 margins.
// With one chunk s is the plain ascending sum of the contract.
__global__ __launch_bounds__(SOFTMAX_MAX_ROWS) void eval_multiclass_kernel(
    const float* __restrict__ margin, const float* __restrict__ label,
    const float* __restrict__ weight,  // nullable
    double* __restrict__ block_out,    // [gridDim.x, 3]
    int64_t n, int K, int KC, int64_t ntiles) {
  extern __shared__ double smem[];
  const int R = blockDim.x, r = threadIdx.x;
  const int kcw = K < KC ? K : KC;
  const int pitch = kcw | 1;
  float* tile = (float*)smem;  // [R][pitch]
  const float* my = tile + r * pitch;
  double acc_nll = 0.0, acc_wrong = 0.0, acc_w = 0.0;

  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * R;
    const int rows = (int)(n - row0 < R ? n - row0 : R);
    const bool valid = r < rows;
    const int yi = valid ? label_class(label[row0 + r], K) : -1;
    float m = -std::numeric_limits<float>::infinity(), xy = 0.f;
    int best = 0;
    double s = 0.0;
    for (int c0 = 0; c0 < K; c0 += KC) {
      const int kc = K - c0 < KC ? K - c0 : KC;
      __syncthreads();
      stage_tile(margin, tile, row0, rows, R, K, c0, kc, pitch);
      __syncthreads();
      const float m_old = m;
      for (int k = 0; k < kc; ++k) {
        const float x = my[k];
        if (x > m) {  // strict: the lowest index keeps a tie
          m = x;
          best = c0 + k;
        }
        if (c0 + k == yi) xy = x;
      }
      if (c0 > 0 && m > m_old) s *= exp((double)m_old - (double)m);
      const double md = (double)m;
      for (int k = 0; k < kc; ++k) s += exp((double)my[k] - md);
    }
    if (valid) {
      const double w = weight ? (double)weight[row0 + r] : 1.0;
      const double nll =
          yi >= 0 ? log(s) - ((double)xy - (double)m)
                  : std::numeric_limits<double>::quiet_NaN();
      acc_nll += w * nll;
      acc_wrong += w * (best == yi ? 0.0 : 1.0);
      acc_w += w;
    }
  }
  // thread order inside a lane (above), butterfly inside a wave, wave order
  // across waves
  for (int off = 1; off < WAVE; off <<= 1) {
    acc_nll += __shfl_xor(acc_nll, off, WAVE);
    acc_wrong += __shfl_xor(acc_wrong, off, WAVE);
    acc_w += __shfl_xor(acc_w, off, WAVE);
  }
  __shared__ double red[3 * SOFTMAX_MAX_ROWS / WAVE];
  const int wv = r / WAVE;
  if ((r & (WAVE - 1)) == 0) {
    red[3 * wv] = acc_nll;
    red[3 * wv + 1] = acc_wrong;
    red[3 * wv + 2] = acc_w;
  }
  __syncthreads();
  if (r < 3) {
    double a = red[r];
    for (int q = 1; q < R / WAVE; ++q) a += red[3 * q + r];
    block_out[3 * (int64_t)blockIdx.x + r] = a;
  }
}

// Rows of a tile: the largest multiple of 64, at most SOFTMAX_MAX_ROWS, whose
// tile of `elem`-byte values (odd pitch) plus `extra` bytes per wave fits
// the LDS budget. `rows` overrides (the benchmark's sweep).
static int softmax_tile_rows(int kcw, int elem, int extra_per_wave,
                             int64_t rows) {
  const int per_wave = WAVE * (kcw | 1) * elem + extra_per_wave;
  int R = std::min(SOFTMAX_MAX_ROWS, SOFTMAX_LDS_BYTES / per_wave * WAVE);
  if (rows > 0) {
    TORCH_CHECK(rows % WAVE == 0 && rows <= R,
                "softmax tile rows must be a multiple of 64 and at most ", R,
                " here, got ", rows);
    R = (int)rows;
  }
  TORCH_CHECK(R >= WAVE, "softmax tile does not fit the LDS budget");
  return R;
}

static void softmax_check_inputs(const char* op, const torch::Tensor& margin,
                                 const torch::Tensor& label,
                                 const torch::Tensor& weight, int64_t chunk) {
  TORCH_CHECK(on_gpu(margin) && margin.scalar_type() == torch::kFloat32 &&
                  margin.dim() == 2 && margin.is_contiguous(),
              op, ": margin must be a contiguous float32 GPU matrix [n, K]");
  const int64_t n = margin.size(0), K = margin.size(1);
  TORCH_CHECK(K >= 2 && K <= (1 << 20), op, ": K must lie in [2, 2^20], got ",
              K);
  TORCH_CHECK(n <= (int64_t(1) << 40), op, ": too many rows: ", n);
  TORCH_CHECK(label.device() == margin.device() &&
                  label.scalar_type() == torch::kFloat32 &&
                  label.is_contiguous() && label.numel() == n,
              op, ": label must be a contiguous float32 [n] on margin's GPU");
  TORCH_CHECK(weight.numel() == 0 ||
                  (weight.device() == margin.device() &&
                   weight.scalar_type() == torch::kFloat32 &&
                   weight.is_contiguous() && weight.numel() == n),
              op, ": weight must be empty or a contiguous float32 [n] on "
                  "margin's GPU");
  TORCH_CHECK(chunk >= 1 && chunk <= SOFTMAX_MAX_CHUNK, op,
              ": chunk must lie in [1, ", SOFTMAX_MAX_CHUNK, "], got ", chunk);
}

// (pairs f32 [K, n, 2] class-major, absmax f32 [K, 2]). chunk / rows
// override KC and R for the benchmark's sweep (0: the defaults).
std::vector<torch::Tensor> softmax_grad(torch::Tensor margin,
                                        torch::Tensor label,
                                        torch::Tensor weight, int64_t chunk,
                                        int64_t rows) {
  if (chunk == 0) chunk = SOFTMAX_CHUNK_CLASSES;
  softmax_check_inputs("softmax_grad", margin, label, weight, chunk);
  const int64_t n = margin.size(0);
  const int K = (int)margin.size(1);
  auto opts = torch::TensorOptions().dtype(torch::kFloat32).device(
      margin.device());
  auto out = torch::empty({K, n, 2}, opts);
  if (n == 0) return {out, torch::zeros({K, 2}, opts)};
  const int kcw = (int)std::min<int64_t>(K, chunk);
  int R = softmax_tile_rows(kcw, 8, kcw * 8, rows);
  if (rows == 0 && K <= chunk) R = std::min(R, SOFTMAX_ONE_CHUNK_ROWS);
  const int64_t ntiles = ceil_div(n, R);
  const int64_t blocks = std::min<int64_t>(
      ntiles, std::min<int64_t>(SOFTMAX_MAX_BLOCKS,
                                std::max<int64_t>(64, SOFTMAX_PARTIAL_ELEMS / K)));
  const size_t lds = (size_t)R * (kcw | 1) * 8 + (size_t)(R / WAVE) * kcw * 8;
  TORCH_CHECK(blocks >= 1 && blocks <= SOFTMAX_MAX_BLOCKS &&
                  lds <= SOFTMAX_LDS_BYTES,
              "softmax_grad: bad launch geometry");
  auto part = torch::empty({blocks, K, 2}, opts);
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(softmax_grad_kernel, dim3((uint32_t)blocks), dim3(R), lds,
                     stream.stream(), margin.data_ptr<float>(),
                     label.data_ptr<float>(),
                     weight.numel() ? weight.data_ptr<float>() : nullptr,
                     (float2*)out.data_ptr<float>(), part.data_ptr<float>(),
                     n, K, (int)chunk, ntiles);
  CHECK_HIP(hipGetLastError());
  // max is order-free and torch's max keeps NaN, so this equals the
  // abs().max() of every class slice bitwise
  return {out, std::get<0>(part.max(0))};
}

// f64 [3] = [sum w * nll, sum w * wrong, sum w]
torch::Tensor eval_multiclass(torch::Tensor margin, torch::Tensor label,
                              torch::Tensor weight, int64_t chunk,
                              int64_t rows) {
  if (chunk == 0) chunk = SOFTMAX_CHUNK_CLASSES;
  softmax_check_inputs("eval_multiclass", margin, label, weight, chunk);
  const int64_t n = margin.size(0);
  const int K = (int)margin.size(1);
  auto opts = torch::TensorOptions().dtype(torch::kFloat64).device(
      margin.device());
  if (n == 0) return torch::zeros({3}, opts);
  const int kcw = (int)std::min<int64_t>(K, chunk);
  const int R = softmax_tile_rows(kcw, 4, 0, rows);
  const int64_t ntiles = ceil_div(n, R);
  const int64_t blocks = std::min<int64_t>(ntiles, SOFTMAX_MAX_BLOCKS);
  const size_t lds = (size_t)R * (kcw | 1) * 4;
  TORCH_CHECK(blocks >= 1 && lds <= SOFTMAX_LDS_BYTES,
              "eval_multiclass: bad launch geometry");
  auto block_out = torch::empty({blocks, 3}, opts);
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(eval_multiclass_kernel, dim3((uint32_t)blocks), dim3(R),
                     lds, stream.stream(), margin.data_ptr<float>(),
                     label.data_ptr<float>(),
                     weight.numel() ? weight.data_ptr<float>() : nullptr,
                     block_out.data_ptr<double>(), n, K, (int)chunk, ntiles);
  CHECK_HIP(hipGetLastError());
  return block_out.sum(0);  // fixed-order torch reduction
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("softmax_grad", &softmax_grad,
        "multi:softprob / multi:softmax pairs, class-major, + per-class absmax",
        py::arg("margin"), py::arg("label"), py::arg("weight"),
        py::arg("chunk") = 0, py::arg("rows") = 0);
  m.def("eval_multiclass", &eval_multiclass,
        "[sum w * nll, sum w * wrong, sum w] of a multiclass margin",
        py::arg("margin"), py::arg("label"), py::arg("weight"),
        py::arg("chunk") = 0, py::arg("rows") = 0);
  m.attr("SOFTMAX_CHUNK_CLASSES") = (int)SOFTMAX_CHUNK_CLASSES;
}
