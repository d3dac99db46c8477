// Pointwise regression kernels for AMD Instinct MI355X (CDNA4, gfx950): the
// gradients of reg:absoluteerror, count:poisson, reg:gamma, reg:tweedie,
// reg:squaredlogerror, reg:pseudohubererror, binary:hinge and
// reg:quantileerror with their |g| / |h| maxima, and the one-pass sums of
// rmse, mae, mape, rmsle, mphe, the three nloglik metrics and quantile.
// Built as its own extension module (xgboost_ray_amd._hip_pointwise_ops), so
// that adding it leaves the build lines and the generated code of the other
// modules as they were. Contract: docs/parity.md "Regression on the device".

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
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

#define PW_THREADS 256
#define PW_WAVES (PW_THREADS / WAVE)
#define PW_ROWS_PER_THREAD 4
#define PW_MAX_BLOCKS 4096
#define PW_MAX_TARGETS 16  // quantile targets the tile kernel serves

// max(a, b) that returns NaN when either side is NaN
__device__ __forceinline__ float max_keep_nan(float a, float b) {
  return (b > a || b != b) ? b : a;
}
// torch.clamp(x, min=lo): NaN stays NaN
__device__ __forceinline__ float clamp_minf(float x, float lo) {
  return x < lo ? lo : x;
}
__device__ __forceinline__ double clamp_mind(double x, double lo) {
  return x < lo ? lo : x;
}

// (|g|, |h|) maxima of a workgroup: the caller folded its own rows; here a
// butterfly inside the wave, then the waves in wave order through LDS.
// Thread 0 stores the workgroup's pair. Nothing is atomic.
__device__ __forceinline__ void block_absmax_store(float gm, float hm,
                                                   float* __restrict__ dst) {
  __shared__ float red[2 * PW_WAVES];
  for (int off = 1; off < WAVE; off <<= 1) {
    gm = max_keep_nan(gm, __shfl_xor(gm, off, WAVE));
    hm = max_keep_nan(hm, __shfl_xor(hm, off, WAVE));
  }
  const int wv = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    red[2 * wv] = gm;
    red[2 * wv + 1] = hm;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < PW_WAVES; ++q) {
      gm = max_keep_nan(gm, red[2 * q]);
      hm = max_keep_nan(hm, red[2 * q + 1]);
    }
    dst[0] = gm;
    dst[1] = hm;
  }
}

// Two float64 sums of a workgroup in a fixed order: butterfly inside a wave,
// wave order across waves. Thread 0 stores them.
__device__ __forceinline__ void block_sum2_store(double a, double b,
                                                 double* __restrict__ dst) {
  __shared__ double red[2 * PW_WAVES];
  for (int off = 1; off < WAVE; off <<= 1) {
    a += __shfl_xor(a, off, WAVE);
    b += __shfl_xor(b, off, WAVE);
  }
  const int wv = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    red[2 * wv] = a;
    red[2 * wv + 1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < PW_WAVES; ++q) {
      a += red[2 * q];
      b += red[2 * q + 1];
    }
    dst[0] = a;
    dst[1] = b;
  }
}

// ---------------------------------------------------------------------------
// Gradients. Every formula is the float32 operation order of its objective
// class in engine/objectives.py as torch's eager GPU kernels run it: one
// rounding per torch op (the module is built with -ffp-contract=off), Python
// scalars rounded to float32 first, a division by a Python scalar as the
// product with its float32 reciprocal, 1.0 / t as a reciprocal.
// p0, p1 per kind:
//   tweedie      p0 = f32(1 - rho), p1 = f32(2 - rho)
//   pseudohuber  p0 = 1.0f / f32(huber_slope)
//   quantile     p0 = 1.0f - f32(alpha), p1 = -f32(alpha)
// ---------------------------------------------------------------------------
enum {
  G_ABSOLUTE = 0, G_POISSON, G_GAMMA, G_TWEEDIE, G_SQUAREDLOG, G_PSEUDOHUBER,
  G_HINGE, G_QUANTILE, G_KINDS
};

template <int KIND>
__device__ __forceinline__ void grad_pair(float m, float y, float p0, float p1,
                                          float& g, float& h) {
  if constexpr (KIND == G_ABSOLUTE) {
    const float d = m - y;
    g = (float)((0.f < d) - (d < 0.f));  // torch.sign: 0 for NaN
    h = 1.f;
  } else if constexpr (KIND == G_POISSON) {
    const float mu = expf(m);
    g = mu - y;
    h = mu;
  } else if constexpr (KIND == G_GAMMA) {
    const float ratio = y * expf(-m);
    g = 1.f - ratio;
    h = ratio;
  } else if constexpr (KIND == G_TWEEDIE) {
    const float a = expf(p0 * m), b = expf(p1 * m);
    const float ny = -y;
    g = ny * a + b;
    h = (ny * p0) * a + p1 * b;
  } else if constexpr (KIND == G_SQUAREDLOG) {
    const float q = clamp_minf(m + 1.f, 1e-6f);
    const float d = logf(q) - logf(clamp_minf(y + 1.f, 1e-6f));
    g = d / q;
    h = clamp_minf((1.f - d) / (q * q), 1e-6f);
  } else if constexpr (KIND == G_PSEUDOHUBER) {
    const float r = m - y;
    const float s = r * p0;
    const float z = 1.f + s * s;
    const float sq = sqrtf(z);
    g = r / sq;
    h = clamp_minf(1.f / (z * sq), 1e-16f);
  } else if constexpr (KIND == G_HINGE) {
    const float t = 2.f * y - 1.f;
    const bool active = m * t < 1.f;  // false for NaN
    g = active ? -t : 0.f;
    h = active ? 1.f : 1e-16f;
  } else {
    g = (m - y >= 0.f) ? p0 : p1;  // false for NaN
    h = 1.f;
  }
}

// A thread takes four consecutive rows per step. VEC: margin, label and
// weight as one 16-byte load each (their bases are 16-byte aligned); else
// one by one, for views that start off a 16-byte boundary. The four pairs
// leave as two 16-byte stores either way: out is this module's own
// allocation. The last n mod 4 rows go one by one.
template <int KIND, bool WEIGHTED, bool VEC>
__global__ __launch_bounds__(PW_THREADS) void pointwise_grad_kernel(
    const float* __restrict__ margin, const float* __restrict__ label,
    const float* __restrict__ weight, float* __restrict__ out,  // [n, 2]
    float* __restrict__ part,                                   // [grid, 2]
    int64_t n, float p0, float p1) {
  float gm = 0.f, hm = 0.f;
  const int64_t step = (int64_t)gridDim.x * PW_THREADS * PW_ROWS_PER_THREAD;
  for (int64_t r0 = ((int64_t)blockIdx.x * PW_THREADS + threadIdx.x) *
                    PW_ROWS_PER_THREAD;
       r0 < n; r0 += step) {
    if (r0 + PW_ROWS_PER_THREAD <= n) {
      float m[4], y[4], w[4] = {1.f, 1.f, 1.f, 1.f}, g[4], h[4];
      if constexpr (VEC) {
        const float4 mv = *(const float4*)(margin + r0);
        const float4 yv = *(const float4*)(label + r0);
        m[0] = mv.x, m[1] = mv.y, m[2] = mv.z, m[3] = mv.w;
        y[0] = yv.x, y[1] = yv.y, y[2] = yv.z, y[3] = yv.w;
        if constexpr (WEIGHTED) {
          const float4 wv = *(const float4*)(weight + r0);
          w[0] = wv.x, w[1] = wv.y, w[2] = wv.z, w[3] = wv.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          m[j] = margin[r0 + j];
          y[j] = label[r0 + j];
          if constexpr (WEIGHTED) w[j] = weight[r0 + j];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        grad_pair<KIND>(m[j], y[j], p0, p1, g[j], h[j]);
        if constexpr (WEIGHTED) {
          g[j] *= w[j];
          h[j] *= w[j];
        }
        gm = max_keep_nan(gm, fabsf(g[j]));
        hm = max_keep_nan(hm, fabsf(h[j]));
      }
      float4* dst = (float4*)(out + 2 * r0);
      dst[0] = make_float4(g[0], h[0], g[1], h[1]);
      dst[1] = make_float4(g[2], h[2], g[3], h[3]);
    } else {
      for (int64_t r = r0; r < n; ++r) {
        float g, h;
        grad_pair<KIND>(margin[r], label[r], p0, p1, g, h);
        if constexpr (WEIGHTED) {
          const float w = weight[r];
          g *= w;
          h *= w;
        }
        *(float2*)(out + 2 * r) = make_float2(g, h);
        gm = max_keep_nan(gm, fabsf(g));
        hm = max_keep_nan(hm, fabsf(h));
      }
    }
  }
  block_absmax_store(gm, hm, part + 2 * (int64_t)blockIdx.x);
}

// ---------------------------------------------------------------------------
// reg:quantileerror with K > 1 targets. The margin is row-major [n, K] and
// the pairs leave target-major, out[k][row]. A workgroup owns a tile of
// PW_THREADS consecutive rows: it reads the tile's rows * K floats as one
// contiguous run (consecutive lanes, consecutive addresses) into an LDS tile
// whose row pitch K | 1 is odd, where thread r then walks row r with every
// lane on a bank of its own. For one k a wave stores 64 consecutive float2,
// 512 contiguous bytes. The K maxima pairs stay in registers over all of a
// workgroup's tiles (the k loop is unrolled to PW_MAX_TARGETS, so they are
// never indexed by a variable) and are folded once at the end.
// ---------------------------------------------------------------------------
struct QuantileAlphas {
  float hi[PW_MAX_TARGETS];  // 1 - a_k
  float lo[PW_MAX_TARGETS];  // -a_k
};

template <bool WEIGHTED>
__global__ __launch_bounds__(PW_THREADS) void quantile_grad_kernel(
    const float* __restrict__ margin,  // [n, K]
    const float* __restrict__ label, const float* __restrict__ weight,
    float2* __restrict__ out,   // [K, n]
    float* __restrict__ part,   // [gridDim.x, K, 2]
    int64_t n, int K, int64_t ntiles, QuantileAlphas al) {
  __shared__ float tile[PW_THREADS * (PW_MAX_TARGETS | 1)];
  __shared__ float red[PW_WAVES * PW_MAX_TARGETS * 2];
  const int r = threadIdx.x, pitch = K | 1;
  const int dq = PW_THREADS / K, dr = PW_THREADS % K;
  float gm[PW_MAX_TARGETS], hm[PW_MAX_TARGETS];
#pragma unroll
  for (int k = 0; k < PW_MAX_TARGETS; ++k) gm[k] = 0.f, hm[k] = 0.f;

  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * PW_THREADS;
    const int rows =
        (int)(n - row0 < PW_THREADS ? n - row0 : (int64_t)PW_THREADS);
    // flat element i = rr * K + kk of the tile goes to thread i % T; (rr, kk)
    // advance by T without a division per element
    const int total = rows * K;
    const float* src = margin + row0 * K;
    int rr = r / K, kk = r % K;
    for (int i = r; i < total; i += PW_THREADS) {
      tile[rr * pitch + kk] = src[i];
      rr += dq;
      kk += dr;
      if (kk >= K) {
        kk -= K;
        ++rr;
      }
    }
    __syncthreads();
    if (r < rows) {
      const int64_t row = row0 + r;
      const float y = label[row];
      float w = 1.f;
      if constexpr (WEIGHTED) w = weight[row];
      const float* my = tile + r * pitch;
#pragma unroll
      for (int k = 0; k < PW_MAX_TARGETS; ++k) {
        if (k < K) {
          float g = (my[k] - y >= 0.f) ? al.hi[k] : al.lo[k];
          float h = 1.f;
          if constexpr (WEIGHTED) {
            g *= w;
            h *= w;
          }
          out[(int64_t)k * n + row] = make_float2(g, h);
          gm[k] = max_keep_nan(gm[k], fabsf(g));
          hm[k] = max_keep_nan(hm[k], fabsf(h));
        }
      }
    }
    __syncthreads();  // before the next tile is staged over this one
  }

  const int lane = r & (WAVE - 1), wv = r / WAVE;
#pragma unroll
  for (int k = 0; k < PW_MAX_TARGETS; ++k) {
    if (k < K) {
      float g = gm[k], h = hm[k];
      for (int off = 1; off < WAVE; off <<= 1) {
        g = max_keep_nan(g, __shfl_xor(g, off, WAVE));
        h = max_keep_nan(h, __shfl_xor(h, off, WAVE));
      }
      if (lane == 0) {
        red[(wv * PW_MAX_TARGETS + k) * 2] = g;
        red[(wv * PW_MAX_TARGETS + k) * 2 + 1] = h;
      }
    }
  }
  __syncthreads();
  if (r < K) {
    float g = red[r * 2], h = red[r * 2 + 1];
    for (int q = 1; q < PW_WAVES; ++q) {
      g = max_keep_nan(g, red[(q * PW_MAX_TARGETS + r) * 2]);
      h = max_keep_nan(h, red[(q * PW_MAX_TARGETS + r) * 2 + 1]);
    }
    float* dst = part + ((int64_t)blockIdx.x * K + r) * 2;
    dst[0] = g;
    dst[1] = h;
  }
}

// ---------------------------------------------------------------------------
// Metrics: [sum w * loss, sum w] in float64 from the float32 inputs, the
// formulae of engine/metrics.py with their clamps. TRANSFORM stands in for
// the objective's prediction transform where the metric class applies one.
// ---------------------------------------------------------------------------
enum {
  E_SE = 0, E_AE, E_APE, E_SLE, E_MPHE, E_POISSON, E_GAMMA, E_TWEEDIE,
  E_KINDS
};
enum { T_IDENTITY = 0, T_EXP, T_SIGMOID, T_KINDS };

template <int TRANSFORM>
__device__ __forceinline__ double eval_pred(float m) {
  const double x = (double)m;
  if constexpr (TRANSFORM == T_EXP) return exp(x);
  if constexpr (TRANSFORM == T_SIGMOID) return 1.0 / (1.0 + exp(-x));
  return x;
}

// w * loss of one row; p0 = 1 - rho, p1 = 2 - rho for tweedie
template <int KIND, int TRANSFORM>
__device__ __forceinline__ double eval_term(float m, float yf, double w,
                                            double p0, double p1) {
  const double y = (double)yf;
  if constexpr (KIND == E_SE) {
    const double d = eval_pred<TRANSFORM>(m) - y;
    return w * (d * d);
  } else if constexpr (KIND == E_AE) {
    return w * fabs(eval_pred<TRANSFORM>(m) - y);
  } else if constexpr (KIND == E_APE) {
    return w * (fabs(eval_pred<TRANSFORM>(m) - y) /
                clamp_mind(fabs(y), 1e-10));
  } else if constexpr (KIND == E_SLE) {
    const double p = clamp_mind(eval_pred<TRANSFORM>(m), -1.0 + 1e-6);
    const double d = log1p(p) - log1p(y);
    return w * d * d;
  } else if constexpr (KIND == E_MPHE) {
    const double r = (double)(m - yf);  // the metric subtracts in float32
    return w * (sqrt(1.0 + r * r) - 1.0);
  } else if constexpr (KIND == E_POISSON) {
    const double mu = clamp_mind(exp((double)m), 1e-16);
    return w * (mu - y * log(mu) + lgamma(y + 1.0));
  } else if constexpr (KIND == E_GAMMA) {
    const double mu = clamp_mind(exp((double)m), 1e-16);
    return w * (y / mu + log(mu));
  } else {
    const double x = (double)m;
    return w * (-y * exp(p0 * x) / p0 + exp(p1 * x) / p1);
  }
}

// The gradient kernel's row split; a thread adds its rows in row order.
template <int KIND, int TRANSFORM, bool WEIGHTED, bool VEC>
__global__ __launch_bounds__(PW_THREADS) void eval_pointwise_kernel(
    const float* __restrict__ margin, const float* __restrict__ label,
    const float* __restrict__ weight, double* __restrict__ part,  // [grid, 2]
    int64_t n, double p0, double p1) {
  double acc = 0.0, accw = 0.0;
  const int64_t step = (int64_t)gridDim.x * PW_THREADS * PW_ROWS_PER_THREAD;
  for (int64_t r0 = ((int64_t)blockIdx.x * PW_THREADS + threadIdx.x) *
                    PW_ROWS_PER_THREAD;
       r0 < n; r0 += step) {
    if (VEC && r0 + PW_ROWS_PER_THREAD <= n) {
      const float4 mv = *(const float4*)(margin + r0);
      const float4 yv = *(const float4*)(label + r0);
      float4 wv = {1.f, 1.f, 1.f, 1.f};
      if constexpr (WEIGHTED) wv = *(const float4*)(weight + r0);
      const float m[4] = {mv.x, mv.y, mv.z, mv.w};
      const float y[4] = {yv.x, yv.y, yv.z, yv.w};
      const float w[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double wd = (double)w[j];
        acc += eval_term<KIND, TRANSFORM>(m[j], y[j], wd, p0, p1);
        accw += wd;
      }
    } else {
      const int64_t end = r0 + PW_ROWS_PER_THREAD < n
                              ? r0 + PW_ROWS_PER_THREAD : n;
      for (int64_t r = r0; r < end; ++r) {
        double wd = 1.0;
        if constexpr (WEIGHTED) wd = (double)weight[r];
        acc += eval_term<KIND, TRANSFORM>(margin[r], label[r], wd, p0, p1);
        accw += wd;
      }
    }
  }
  block_sum2_store(acc, accw, part + 2 * (int64_t)blockIdx.x);
}

// Pinball loss over the flat row-major [n, K] margin: element i belongs to
// row i / K and target i % K, so consecutive lanes read consecutive
// addresses with no tile. A row's weight counts once, at its first target.
struct PinballAlphas {
  double a[PW_MAX_TARGETS];
};

template <bool WEIGHTED>
__global__ __launch_bounds__(PW_THREADS) void eval_pinball_kernel(
    const float* __restrict__ margin, const float* __restrict__ label,
    const float* __restrict__ weight, double* __restrict__ part,
    int64_t total, int K, PinballAlphas al) {
  __shared__ double alpha[PW_MAX_TARGETS];
  if ((int)threadIdx.x < PW_MAX_TARGETS) alpha[threadIdx.x] = al.a[threadIdx.x];
  __syncthreads();
  double acc = 0.0, accw = 0.0;
  const int64_t step = (int64_t)gridDim.x * PW_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * PW_THREADS + threadIdx.x; i < total;
       i += step) {
    const int64_t row = i / K;
    const int k = (int)(i - row * K);
    double w = 1.0;
    if constexpr (WEIGHTED) w = (double)weight[row];
    const double d = (double)label[row] - (double)margin[i];
    const double a = alpha[k];
    acc += w * (d >= 0.0 ? a * d : (a - 1.0) * d);
    if (k == 0) accw += w;
  }
  block_sum2_store(acc, accw, part + 2 * (int64_t)blockIdx.x);
}

// --------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------
static inline bool aligned16(const torch::Tensor& t) {
  return (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0;
}

// Checks shared by every op; returns whether the 16-byte loads apply.
static bool check_inputs(const char* op, const torch::Tensor& margin,
                         const torch::Tensor& label,
                         const torch::Tensor& weight, int64_t n) {
  TORCH_CHECK(on_gpu(margin) && margin.scalar_type() == torch::kFloat32 &&
                  margin.is_contiguous(),
              op, ": margin must be a contiguous float32 GPU tensor");
  TORCH_CHECK(label.device() == margin.device() &&
                  label.scalar_type() == torch::kFloat32 &&
                  label.is_contiguous() && label.dim() == 1 &&
                  label.numel() == n,
              op, ": label must be a contiguous float32 [n] on margin's GPU");
  TORCH_CHECK(weight.numel() == 0 ||
                  (weight.device() == margin.device() &&
                   weight.scalar_type() == torch::kFloat32 &&
                   weight.is_contiguous() && weight.dim() == 1 &&
                   weight.numel() == n),
              op, ": weight must be empty or a contiguous float32 [n] on "
                  "margin's GPU");
  return aligned16(margin) && aligned16(label) &&
         (weight.numel() == 0 || aligned16(weight));
}

static int pointwise_blocks(const char* op, int64_t n, int64_t rows_per_block,
                            int64_t max_blocks) {
  TORCH_CHECK(max_blocks >= 0 && max_blocks <= PW_MAX_BLOCKS, op,
              ": max_blocks must lie in [0, ", PW_MAX_BLOCKS, "], got ",
              max_blocks);
  if (max_blocks == 0) max_blocks = PW_MAX_BLOCKS;
  return (int)std::min<int64_t>(ceil_div(n, rows_per_block), max_blocks);
}

template <int KIND>
static void launch_grad(bool weighted, bool vec, int blocks,
                        hipStream_t stream, const float* m, const float* y,
                        const float* w, float* out, float* part, int64_t n,
                        float p0, float p1) {
  auto kernel = weighted
      ? (vec ? pointwise_grad_kernel<KIND, true, true>
             : pointwise_grad_kernel<KIND, true, false>)
      : (vec ? pointwise_grad_kernel<KIND, false, true>
             : pointwise_grad_kernel<KIND, false, false>);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(PW_THREADS), 0, stream, m, y,
                     w, out, part, n, p0, p1);
}

// (pairs f32 [n, 2], absmax f32 [2]); kind as in the G_* list above
std::vector<torch::Tensor> pointwise_grad(torch::Tensor margin,
                                          torch::Tensor label,
                                          torch::Tensor weight, int64_t kind,
                                          double p0, double p1,
                                          int64_t max_blocks) {
  TORCH_CHECK(margin.dim() == 1, "pointwise_grad: margin must be a vector");
  const int64_t n = margin.numel();
  const bool vec = check_inputs("pointwise_grad", margin, label, weight, n);
  TORCH_CHECK(kind >= 0 && kind < G_KINDS, "pointwise_grad: unknown kind ",
              kind);
  auto opts = margin.options();
  auto out = torch::empty({n, 2}, opts);
  if (n == 0) return {out, torch::zeros({2}, opts)};
  const int blocks = pointwise_blocks(
      "pointwise_grad", n, PW_THREADS * PW_ROWS_PER_THREAD, max_blocks);
  auto part = torch::empty({blocks, 2}, opts);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const bool wt = weight.numel() > 0;
  const float* m = margin.data_ptr<float>();
  const float* y = label.data_ptr<float>();
  const float* w = wt ? weight.data_ptr<float>() : nullptr;
  float* o = out.data_ptr<float>();
  float* p = part.data_ptr<float>();
  const float a = (float)p0, b = (float)p1;
  switch (kind) {
#define PW_CASE(K) \
  case K: launch_grad<K>(wt, vec, blocks, stream, m, y, w, o, p, n, a, b); break
    PW_CASE(G_ABSOLUTE);
    PW_CASE(G_POISSON);
    PW_CASE(G_GAMMA);
    PW_CASE(G_TWEEDIE);
    PW_CASE(G_SQUAREDLOG);
    PW_CASE(G_PSEUDOHUBER);
    PW_CASE(G_HINGE);
    PW_CASE(G_QUANTILE);
#undef PW_CASE
  }
  CHECK_HIP(hipGetLastError());
  // max is order-free and torch's max keeps NaN: this equals abs().amax(0)
  return {out, std::get<0>(part.max(0))};
}

// (pairs f32 [K, n, 2] target-major, absmax f32 [K, 2]); hi[k] = 1 - a_k and
// lo[k] = -a_k, both already float32 values
std::vector<torch::Tensor> quantile_grad(torch::Tensor margin,
                                         torch::Tensor label,
                                         torch::Tensor weight,
                                         std::vector<double> hi,
                                         std::vector<double> lo,
                                         int64_t max_blocks) {
  TORCH_CHECK(margin.dim() == 2, "quantile_grad: margin must be [n, K]");
  const int64_t n = margin.size(0);
  const int K = (int)margin.size(1);
  check_inputs("quantile_grad", margin, label, weight, n);
  TORCH_CHECK(K >= 1 && K <= PW_MAX_TARGETS && (int)hi.size() == K &&
                  (int)lo.size() == K,
              "quantile_grad: K must lie in [1, ", PW_MAX_TARGETS,
              "] with one alpha per target");
  auto opts = margin.options();
  auto out = torch::empty({K, n, 2}, opts);
  if (n == 0) return {out, torch::zeros({K, 2}, opts)};
  QuantileAlphas al;
  for (int k = 0; k < PW_MAX_TARGETS; ++k) {
    al.hi[k] = k < K ? (float)hi[k] : 0.f;
    al.lo[k] = k < K ? (float)lo[k] : 0.f;
  }
  const int64_t ntiles = ceil_div(n, PW_THREADS);
  const int blocks =
      pointwise_blocks("quantile_grad", n, PW_THREADS, max_blocks);
  auto part = torch::empty({blocks, K, 2}, opts);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const bool wt = weight.numel() > 0;
  auto kernel = wt ? quantile_grad_kernel<true> : quantile_grad_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(PW_THREADS), 0, stream,
                     margin.data_ptr<float>(), label.data_ptr<float>(),
                     wt ? weight.data_ptr<float>() : nullptr,
                     (float2*)out.data_ptr<float>(), part.data_ptr<float>(), n,
                     K, ntiles, al);
  CHECK_HIP(hipGetLastError());
  return {out, std::get<0>(part.max(0))};
}

template <int KIND, int TRANSFORM>
static void launch_eval(bool weighted, bool vec, int blocks,
                        hipStream_t stream, const float* m, const float* y,
                        const float* w, double* part, int64_t n, double p0,
                        double p1) {
  auto kernel = weighted
      ? (vec ? eval_pointwise_kernel<KIND, TRANSFORM, true, true>
             : eval_pointwise_kernel<KIND, TRANSFORM, true, false>)
      : (vec ? eval_pointwise_kernel<KIND, TRANSFORM, false, true>
             : eval_pointwise_kernel<KIND, TRANSFORM, false, false>);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(PW_THREADS), 0, stream, m, y,
                     w, part, n, p0, p1);
}

// f64 [2] = [sum w * loss, sum w]; kind and transform as in the E_* / T_*
// lists above. mphe and the nloglik kinds are defined on the margin itself
// and take the identity only.
torch::Tensor eval_pointwise(torch::Tensor margin, torch::Tensor label,
                             torch::Tensor weight, int64_t kind,
                             int64_t transform, double p0, double p1,
                             int64_t max_blocks) {
  TORCH_CHECK(margin.dim() == 1, "eval_pointwise: margin must be a vector");
  const int64_t n = margin.numel();
  const bool vec = check_inputs("eval_pointwise", margin, label, weight, n);
  TORCH_CHECK(kind >= 0 && kind < E_KINDS && transform >= 0 &&
                  transform < T_KINDS,
              "eval_pointwise: unknown kind ", kind, " or transform ",
              transform);
  TORCH_CHECK(kind < E_MPHE || transform == T_IDENTITY,
              "eval_pointwise: kind ", kind, " takes the identity transform");
  auto opts = margin.options().dtype(torch::kFloat64);
  if (n == 0) return torch::zeros({2}, opts);
  const int blocks = pointwise_blocks(
      "eval_pointwise", n, PW_THREADS * PW_ROWS_PER_THREAD, max_blocks);
  auto part = torch::empty({blocks, 2}, opts);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const bool wt = weight.numel() > 0;
  const float* m = margin.data_ptr<float>();
  const float* y = label.data_ptr<float>();
  const float* w = wt ? weight.data_ptr<float>() : nullptr;
  double* p = part.data_ptr<double>();
#define PW_EVAL(K, T) \
  launch_eval<K, T>(wt, vec, blocks, stream, m, y, w, p, n, p0, p1)
#define PW_EVAL3(K)                                   \
  case K:                                             \
    if (transform == T_EXP) PW_EVAL(K, T_EXP);        \
    else if (transform == T_SIGMOID) PW_EVAL(K, T_SIGMOID); \
    else PW_EVAL(K, T_IDENTITY);                      \
    break
  switch (kind) {
    PW_EVAL3(E_SE);
    PW_EVAL3(E_AE);
    PW_EVAL3(E_APE);
    PW_EVAL3(E_SLE);
    case E_MPHE: PW_EVAL(E_MPHE, T_IDENTITY); break;
    case E_POISSON: PW_EVAL(E_POISSON, T_IDENTITY); break;
    case E_GAMMA: PW_EVAL(E_GAMMA, T_IDENTITY); break;
    case E_TWEEDIE: PW_EVAL(E_TWEEDIE, T_IDENTITY); break;
  }
#undef PW_EVAL3
#undef PW_EVAL
  CHECK_HIP(hipGetLastError());
  return part.sum(0);  // fixed-order torch reduction
}

// f64 [2] = [sum over rows and targets of w * pinball, sum w]
torch::Tensor eval_pinball(torch::Tensor margin, torch::Tensor label,
                           torch::Tensor weight, std::vector<double> alphas,
                           int64_t max_blocks) {
  TORCH_CHECK(margin.dim() == 2, "eval_pinball: margin must be [n, K]");
  const int64_t n = margin.size(0);
  const int K = (int)margin.size(1);
  check_inputs("eval_pinball", margin, label, weight, n);
  TORCH_CHECK(K >= 1 && K <= PW_MAX_TARGETS && (int)alphas.size() == K,
              "eval_pinball: K must lie in [1, ", PW_MAX_TARGETS,
              "] with one alpha per target");
  auto opts = margin.options().dtype(torch::kFloat64);
  if (n == 0) return torch::zeros({2}, opts);
  PinballAlphas al;
  for (int k = 0; k < PW_MAX_TARGETS; ++k) al.a[k] = k < K ? alphas[k] : 0.0;
  const int64_t total = n * K;
  const int blocks = pointwise_blocks(
      "eval_pinball", total, PW_THREADS * PW_ROWS_PER_THREAD, max_blocks);
  auto part = torch::empty({blocks, 2}, opts);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const bool wt = weight.numel() > 0;
  auto kernel = wt ? eval_pinball_kernel<true> : eval_pinball_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(PW_THREADS), 0, stream,
                     margin.data_ptr<float>(), label.data_ptr<float>(),
                     wt ? weight.data_ptr<float>() : nullptr,
                     part.data_ptr<double>(), total, K, al);
  CHECK_HIP(hipGetLastError());
  return part.sum(0);  // fixed-order torch reduction
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("pointwise_grad", &pointwise_grad, "pointwise pairs + absmax",
        py::arg("margin"), py::arg("label"), py::arg("weight"),
        py::arg("kind"), py::arg("p0"), py::arg("p1"),
        py::arg("max_blocks") = 0);
  m.def("quantile_grad", &quantile_grad,
        "reg:quantileerror pairs, target-major, + per-target absmax",
        py::arg("margin"), py::arg("label"), py::arg("weight"),
        py::arg("hi"), py::arg("lo"), py::arg("max_blocks") = 0);
  m.def("eval_pointwise", &eval_pointwise, "[sum w * loss, sum w]",
        py::arg("margin"), py::arg("label"), py::arg("weight"),
        py::arg("kind"), py::arg("transform"), py::arg("p0"), py::arg("p1"),
        py::arg("max_blocks") = 0);
  m.def("eval_pinball", &eval_pinball,
        "[sum w * pinball over rows and targets, sum w]",
        py::arg("margin"), py::arg("label"), py::arg("weight"),
        py::arg("alphas"), py::arg("max_blocks") = 0);
  m.attr("MAX_TARGETS") = (int)PW_MAX_TARGETS;
}
