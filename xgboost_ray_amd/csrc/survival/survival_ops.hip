// Survival kernels for AMD Instinct MI355X (CDNA4, gfx950): the survival:aft
// gradient and aft-nloglik sums (elementwise, one branch per row), and the
// survival:cox gradient and cox-nloglik sums (a reduce-then-scan in both
// directions over the time-sorted rows). Built as its own extension module
// (xgboost_ray_amd._hip_survival_ops), so that adding it leaves the build
// lines and the generated code of the other modules as they were.
// Contract: docs/parity.md "Survival on the device".

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <cmath>
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

#define SURV_THREADS 256
#define SURV_WAVES (SURV_THREADS / WAVE)

// max(a, b) that returns NaN when either side is NaN
__device__ __forceinline__ float max_keep_nan(float a, float b) {
  return (b > a || b != b) ? b : a;
}
// torch.clamp(x, min=lo): NaN stays NaN
__device__ __forceinline__ double clamp_min(double x, double lo) {
  return x < lo ? lo : x;
}

// (|g|, |h|) maxima of a workgroup: the caller folded its own rows; here a
// butterfly inside the wave, then the waves in wave order through LDS.
// Thread 0 stores the workgroup's pair. Nothing is atomic.
__device__ __forceinline__ void block_absmax_store(float gm, float hm,
                                                   float* __restrict__ dst) {
  __shared__ float red[2 * SURV_WAVES];
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
    for (int q = 1; q < SURV_WAVES; ++q) {
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
  __shared__ double red[2 * SURV_WAVES];
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
    for (int q = 1; q < SURV_WAVES; ++q) {
      a += red[2 * q];
      b += red[2 * q + 1];
    }
    dst[0] = a;
    dst[1] = b;
  }
}

// ---------------------------------------------------------------------------
// AFT. A thread takes four consecutive rows per step: the margins and the
// weights as one 16-byte load each, every row's (lower, upper) as one 8-byte
// load. A row then runs the code of its own censoring kind only; rows that
// share a kind inside a wave share the cost. The distribution is a template
// parameter, so a launch carries one distribution's code.
// ---------------------------------------------------------------------------
enum { AFT_NORMAL = 0, AFT_LOGISTIC = 1, AFT_EXTREME = 2 };
#define AFT_ROWS_PER_THREAD 4
#define AFT_MAX_BLOCKS 4096

__device__ __forceinline__ double sigm(double z) {
  return 1.0 / (1.0 + exp(-z));
}
__device__ __forceinline__ double clamp_z(double z) {
  return z < -15.0 ? -15.0 : (z > 15.0 ? 15.0 : z);  // NaN stays NaN
}
__device__ __forceinline__ double exp_z(double z) {
  return exp(z > 15.0 ? 15.0 : z);
}

// f(z) and dlogf(z)
template <int DIST>
__device__ __forceinline__ void pdf_terms(double z, double& f, double& dlogf) {
  if (DIST == AFT_LOGISTIC) {
    const double s = sigm(z);
    f = s * (1.0 - s);
    dlogf = 1.0 - 2.0 * s;
  } else if (DIST == AFT_EXTREME) {
    const double ez = exp_z(z);
    f = ez * exp(-ez);
    dlogf = 1.0 - ez;
  } else {
    f = exp(-0.5 * z * z) / 2.5066282746310002;  // sqrt(2 pi)
    dlogf = -z;
  }
}

// S(z) = 1 - F(z) without cancellation
template <int DIST>
__device__ __forceinline__ double survival(double z) {
  if (DIST == AFT_LOGISTIC) return sigm(-z);
  if (DIST == AFT_EXTREME) return exp(-exp_z(z));
  return 0.5 * erfc(z * M_SQRT1_2);
}

// F(z) as the metric takes it
template <int DIST>
__device__ __forceinline__ double cdf(double z) {
  if (DIST == AFT_LOGISTIC) return sigm(z);
  if (DIST == AFT_EXTREME) return 1.0 - exp(-exp_z(z));
  return 0.5 * erfc(-z * M_SQRT1_2);
}

__device__ __forceinline__ double log_time(float y) {
  return log(clamp_min((double)y, 1e-16));
}

template <int DIST>
__device__ __forceinline__ void aft_pair(float m, float2 y, double sig,
                                         double& g, double& h) {
  const double md = (double)m, s2 = sig * sig;
  const double zl = clamp_z((log_time(y.x) - md) / sig);
  if (y.x == y.y) {  // uncensored: nll = -log f(zl)
    if (DIST == AFT_LOGISTIC) {
      const double s = sigm(zl);
      g = (1.0 - 2.0 * s) / sig;
      h = 2.0 * s * (1.0 - s) / s2;
    } else if (DIST == AFT_EXTREME) {
      const double ez = exp_z(zl);
      g = (1.0 - ez) / sig;
      h = ez / s2;
    } else {
      g = -zl / sig;
      h = 1.0 / s2;
    }
  } else if (isinf(y.y)) {  // right-censored: hazard f/S at zl
    double hz, dhz;
    if (DIST == AFT_LOGISTIC) {
      hz = sigm(zl);
      dhz = hz * (1.0 - hz);
    } else if (DIST == AFT_EXTREME) {
      hz = exp_z(zl);
      dhz = hz;
    } else {
      double f, d;
      pdf_terms<DIST>(zl, f, d);
      hz = f / clamp_min(survival<DIST>(zl), 1e-300);
      dhz = hz * (hz - zl);
    }
    g = -hz / sig;
    h = dhz / s2;
  } else {
    const double zu = clamp_z((log_time(y.y) - md) / sig);
    if (y.x <= 0.f) {  // left-censored: reversed hazard f/F at zu
      double rh, drh;
      if (DIST == AFT_LOGISTIC) {
        rh = sigm(-zu);
        drh = -rh * (1.0 - rh);
      } else if (DIST == AFT_EXTREME) {
        double f, d;
        pdf_terms<DIST>(zu, f, d);
        rh = f / clamp_min(1.0 - survival<DIST>(zu), 1e-300);
        drh = rh * (d - rh);  // d = 1 - e^z
      } else {
        double f, d;
        pdf_terms<DIST>(zu, f, d);
        rh = f / clamp_min(0.5 * erfc(-zu * M_SQRT1_2), 1e-300);
        drh = rh * (-zu - rh);
      }
      g = rh / sig;
      h = -drh / s2;
    } else {  // interval: nll = -log(F(zu) - F(zl))
      double fl, dl, fu, du;
      pdf_terms<DIST>(zl, fl, dl);
      pdf_terms<DIST>(zu, fu, du);
      const double D =
          clamp_min(survival<DIST>(zl) - survival<DIST>(zu), 1e-300);
      const double df = fu - fl;
      g = df / (sig * D);
      h = (df * df / (D * D) - (fu * du - fl * dl) / D) / s2;
    }
  }
  h = clamp_min(h, 1e-6);
}

template <int DIST>
__device__ __forceinline__ double aft_nll(float m, float2 y, double sig,
                                          double log_sig) {
  const double md = (double)m;
  const double lo = log_time(y.x);
  const double zl = clamp_z((lo - md) / sig);
  if (y.x == y.y) {
    double f, d;
    pdf_terms<DIST>(zl, f, d);
    return -log(clamp_min(f, 1e-12)) + log_sig + lo;
  }
  double D;
  if (isinf(y.y)) {
    D = 1.0 - cdf<DIST>(zl);
  } else {
    const double zu = clamp_z((log_time(y.y) - md) / sig);
    D = y.x <= 0.f ? cdf<DIST>(zu) : cdf<DIST>(zu) - cdf<DIST>(zl);
  }
  return -log(clamp_min(D, 1e-12));
}

// Rows [r0, r0 + 4) of a thread: vector loads when all four exist.
struct AftRows {
  float m[AFT_ROWS_PER_THREAD], w[AFT_ROWS_PER_THREAD];
  float2 y[AFT_ROWS_PER_THREAD];
  int cnt;
};
__device__ __forceinline__ AftRows aft_load(const float* __restrict__ margin,
                                            const float2* __restrict__ label,
                                            const float* __restrict__ weight,
                                            int64_t r0, int64_t n) {
  AftRows a;
  a.cnt = (int)(n - r0 < AFT_ROWS_PER_THREAD ? n - r0 : AFT_ROWS_PER_THREAD);
  if (a.cnt == AFT_ROWS_PER_THREAD) {
    const float4 mv = *(const float4*)(margin + r0);
    a.m[0] = mv.x, a.m[1] = mv.y, a.m[2] = mv.z, a.m[3] = mv.w;
    float4 wv = {1.f, 1.f, 1.f, 1.f};
    if (weight) wv = *(const float4*)(weight + r0);
    a.w[0] = wv.x, a.w[1] = wv.y, a.w[2] = wv.z, a.w[3] = wv.w;
#pragma unroll
    for (int j = 0; j < AFT_ROWS_PER_THREAD; ++j) a.y[j] = label[r0 + j];
  } else {
    for (int j = 0; j < a.cnt; ++j) {
      a.m[j] = margin[r0 + j];
      a.w[j] = weight ? weight[r0 + j] : 1.f;
      a.y[j] = label[r0 + j];
    }
  }
  return a;
}

template <int DIST>
__global__ __launch_bounds__(SURV_THREADS) void aft_grad_kernel(
    const float* __restrict__ margin, const float2* __restrict__ label,
    const float* __restrict__ weight,  // nullable
    float2* __restrict__ out, float* __restrict__ part,  // [gridDim.x, 2]
    int64_t n, double sig) {
  float gm = 0.f, hm = 0.f;
  const int64_t step = (int64_t)gridDim.x * SURV_THREADS * AFT_ROWS_PER_THREAD;
  for (int64_t r0 = ((int64_t)blockIdx.x * SURV_THREADS + threadIdx.x) *
                    AFT_ROWS_PER_THREAD;
       r0 < n; r0 += step) {
    const AftRows a = aft_load(margin, label, weight, r0, n);
    for (int j = 0; j < a.cnt; ++j) {
      double gd, hd;
      aft_pair<DIST>(a.m[j], a.y[j], sig, gd, hd);
      float g = (float)gd, h = (float)hd;
      if (weight != nullptr) {
        g *= a.w[j];
        h *= a.w[j];
      }
      out[r0 + j] = {g, h};
      gm = max_keep_nan(gm, fabsf(g));
      hm = max_keep_nan(hm, fabsf(h));
    }
  }
  block_absmax_store(gm, hm, part + 2 * (int64_t)blockIdx.x);
}

template <int DIST>
__global__ __launch_bounds__(SURV_THREADS) void eval_aft_kernel(
    const float* __restrict__ margin, const float2* __restrict__ label,
    const float* __restrict__ weight,  // nullable
    double* __restrict__ part,         // [gridDim.x, 2]
    int64_t n, double sig, double log_sig) {
  double acc = 0.0, accw = 0.0;
  const int64_t step = (int64_t)gridDim.x * SURV_THREADS * AFT_ROWS_PER_THREAD;
  for (int64_t r0 = ((int64_t)blockIdx.x * SURV_THREADS + threadIdx.x) *
                    AFT_ROWS_PER_THREAD;
       r0 < n; r0 += step) {
    const AftRows a = aft_load(margin, label, weight, r0, n);
    for (int j = 0; j < a.cnt; ++j) {
      const double w = (double)a.w[j];
      acc += w * aft_nll<DIST>(a.m[j], a.y[j], sig, log_sig);
      accw += w;
    }
  }
  block_sum2_store(acc, accw, part + 2 * (int64_t)blockIdx.x);
}

// ---------------------------------------------------------------------------
// Cox. Rows are visited in the layout's order (time descending); position s
// of that order belongs to tile s / COX_TILE_ROWS, and inside a tile thread t
// owns COX_ROWS_PER_THREAD consecutive positions, so a thread's serial sum,
// a wave scan over the threads and the waves in order add up in position
// order. The reverse passes give thread t the mirrored slice and walk it
// backwards, so the same scan code yields suffix sums. Every sum has one
// fixed grouping: equal inputs give equal bytes.
// ---------------------------------------------------------------------------
#ifndef COX_ROWS_PER_THREAD
#define COX_ROWS_PER_THREAD 8
#endif
#define COX_TILE_ROWS (SURV_THREADS * COX_ROWS_PER_THREAD)
#define COX_MAX_PARTS SURV_THREADS  // partial maxima of the margin
#define RPT COX_ROWS_PER_THREAD

// Positions [s0, s0 + RPT) of an int32 array: 16-byte loads when all exist
// (s0 is a multiple of RPT, the base is 16-byte aligned), else one by one,
// `fill` beyond n.
__device__ __forceinline__ void load_i32(const int* __restrict__ p, int64_t s0,
                                         int64_t n, int (&v)[RPT], int fill) {
  if (s0 + RPT <= n) {
#pragma unroll
    for (int q = 0; q < RPT / 4; ++q) {
      const int4 x = *(const int4*)(p + s0 + 4 * q);
      v[4 * q] = x.x, v[4 * q + 1] = x.y, v[4 * q + 2] = x.z,
             v[4 * q + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < RPT; ++j) v[j] = s0 + j < n ? p[s0 + j] : fill;
  }
}
__device__ __forceinline__ void load_u8(const uint8_t* __restrict__ p,
                                        int64_t s0, int64_t n,
                                        int (&v)[RPT]) {
  if (s0 + RPT <= n) {
#pragma unroll
    for (int q = 0; q < RPT / 4; ++q) {
      const uint32_t x = *(const uint32_t*)(p + s0 + 4 * q);
#pragma unroll
      for (int b = 0; b < 4; ++b) v[4 * q + b] = (x >> (8 * b)) & 0xff;
    }
  } else {
#pragma unroll
    for (int j = 0; j < RPT; ++j) v[j] = s0 + j < n ? p[s0 + j] : 0;
  }
}

// The margin's maximum from the per-workgroup partials: every workgroup that
// needs the shift folds these few floats again, so no launch finalises them
// and the host never reads them.
__device__ __forceinline__ float block_shift(const float* __restrict__ pmax,
                                             int nparts) {
  __shared__ float sh[SURV_WAVES];
  float v = (int)threadIdx.x < nparts
                ? pmax[threadIdx.x]
                : -std::numeric_limits<float>::infinity();
  for (int off = 1; off < WAVE; off <<= 1)
    v = max_keep_nan(v, __shfl_xor(v, off, WAVE));
  if ((threadIdx.x & (WAVE - 1)) == 0) sh[threadIdx.x / WAVE] = v;
  __syncthreads();
  v = sh[0];
  for (int q = 1; q < SURV_WAVES; ++q) v = max_keep_nan(v, sh[q]);
  return v;
}

// Exclusive prefix of `tot` over the workgroup's threads in thread order:
// shuffle scan inside a wave, wave totals through LDS. `total` is the
// workgroup's sum.
__device__ __forceinline__ double block_excl_scan(double tot, double& total) {
  __shared__ double wtot[SURV_WAVES];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  double incl = tot;
  for (int off = 1; off < WAVE; off <<= 1) {
    const double t = __shfl_up(incl, off, WAVE);
    if (lane >= off) incl += t;
  }
  double excl = __shfl_up(incl, 1, WAVE);
  if (lane == 0) excl = 0.0;
  __syncthreads();  // wtot's earlier readers are done
  if (lane == WAVE - 1) wtot[wv] = incl;
  __syncthreads();
  double woff = 0.0, all = 0.0;
  for (int q = 0; q < SURV_WAVES; ++q) {
    if (q == wv) woff = all;
    all += wtot[q];
  }
  total = all;
  return woff + excl;
}

__global__ __launch_bounds__(SURV_THREADS) void cox_max_kernel(
    const float* __restrict__ margin, float* __restrict__ pmax, int64_t n) {
  float v = -std::numeric_limits<float>::infinity();
  const int64_t step = (int64_t)gridDim.x * SURV_THREADS * 4;
  for (int64_t r0 = ((int64_t)blockIdx.x * SURV_THREADS + threadIdx.x) * 4;
       r0 < n; r0 += step) {
    if (r0 + 4 <= n) {
      const float4 x = *(const float4*)(margin + r0);
      v = max_keep_nan(max_keep_nan(max_keep_nan(max_keep_nan(v, x.x), x.y),
                                    x.z), x.w);
    } else {
      for (int64_t r = r0; r < n; ++r) v = max_keep_nan(v, margin[r]);
    }
  }
  for (int off = 1; off < WAVE; off <<= 1)
    v = max_keep_nan(v, __shfl_xor(v, off, WAVE));
  __shared__ float sh[SURV_WAVES];
  if ((threadIdx.x & (WAVE - 1)) == 0) sh[threadIdx.x / WAVE] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < SURV_WAVES; ++q) v = max_keep_nan(v, sh[q]);
    pmax[blockIdx.x] = v;
  }
}

// A thread's slice of tile `tile`: forward, thread t owns local positions
// [t * RPT, +RPT) and walks them upwards; reversed, thread t owns the slice
// of thread (T - 1 - t) and walks it downwards.
template <bool REV>
__device__ __forceinline__ int64_t slice_start(int64_t tile) {
  const int t = REV ? SURV_THREADS - 1 - (int)threadIdx.x : (int)threadIdx.x;
  return tile * COX_TILE_ROWS + (int64_t)t * RPT;
}

// eta of a thread's slice (0 beyond n), margins gathered through `order`
__device__ __forceinline__ void slice_eta(const float* __restrict__ margin,
                                          const int (&ord)[RPT], int64_t s0,
                                          int64_t n, float shift,
                                          float (&m)[RPT], double (&eta)[RPT]) {
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    const bool in = s0 + j < n;
    m[j] = in ? margin[ord[j]] : 0.f;
    eta[j] = in ? exp((double)m[j] - (double)shift) : 0.0;
  }
}

// Forward pass over a tile. SUMS: store the tile's eta sum (reduce step).
// Otherwise the tile prefix is known (apply step): WRITE_C stores the
// inclusive prefix C in sorted order, METRIC accumulates the cox-nloglik
// terms of the event rows into this tile's partial.
template <bool SUMS, bool WRITE_C, bool METRIC>
__global__ __launch_bounds__(SURV_THREADS) void cox_forward_kernel(
    const float* __restrict__ margin, const int* __restrict__ order,
    const uint8_t* __restrict__ event, const float* __restrict__ pmax,
    int nparts, double* __restrict__ tile_io,  // sums out / prefixes in
    double* __restrict__ C, double* __restrict__ mpart,  // [ntiles, 2]
    int64_t n) {
  const int64_t tile = blockIdx.x;
  const float shift = block_shift(pmax, nparts);
  const int64_t s0 = slice_start<false>(tile);
  int ord[RPT];
  float m[RPT];
  double eta[RPT];
  load_i32(order, s0, n, ord, 0);
  slice_eta(margin, ord, s0, n, shift, m, eta);
  double run[RPT], tot = 0.0;
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    tot += eta[j];
    run[j] = tot;
  }
  double total;
  const double excl = block_excl_scan(tot, total);
  if (SUMS) {
    if (threadIdx.x == 0) tile_io[tile] = total;
    return;
  }
  const double base = tile_io[tile] + excl;
  double acc = 0.0, nev = 0.0;
  int ev[RPT];
  if (METRIC) load_u8(event, s0, n, ev);
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    if (s0 + j < n) {
      const double c = base + run[j];
      if (WRITE_C) C[s0 + j] = c;
      if (METRIC && ev[j]) {
        // stored negated: the partials sum to -ll
        acc -= (double)m[j] - (double)shift - log(clamp_min(c, 1e-300));
        nev += 1.0;
      }
    }
  }
  if (METRIC) block_sum2_store(acc, nev, mpart + 2 * tile);
}

// Exclusive scan of the tile sums in one workgroup per array (blockIdx.x
// names the array): a thread sums a contiguous chunk serially, the chunk
// totals are scanned across the workgroup, and the thread walks its chunk
// again. REV scans from the last tile down.
template <bool REV>
__global__ __launch_bounds__(SURV_THREADS) void cox_tile_scan_kernel(
    const double* __restrict__ sums, double* __restrict__ prefix,
    int64_t ntiles) {
  sums += (int64_t)blockIdx.x * ntiles;
  prefix += (int64_t)blockIdx.x * ntiles;
  const int64_t chunk = (ntiles + SURV_THREADS - 1) / SURV_THREADS;
  const int64_t lo = threadIdx.x * chunk < ntiles ? threadIdx.x * chunk : ntiles;
  const int64_t hi = lo + chunk < ntiles ? lo + chunk : ntiles;
  double tot = 0.0;
  for (int64_t i = lo; i < hi; ++i) tot += sums[REV ? ntiles - 1 - i : i];
  double total;
  double run = block_excl_scan(tot, total);
  for (int64_t i = lo; i < hi; ++i) {
    const int64_t t = REV ? ntiles - 1 - i : i;
    prefix[t] = run;
    run += sums[t];
  }
}

// Reverse pass over a tile: a = ev / R and b = ev / R^2 with R = C[last(s)],
// two sums side by side. The tile's C is staged in LDS; only a tie block
// that runs past the tile's end reads C from memory, and only event rows
// read it at all. SUMS stores the tile's two sums, otherwise the inclusive
// suffix sums are stored in sorted order.
template <bool SUMS>
__global__ __launch_bounds__(SURV_THREADS) void cox_reverse_kernel(
    const double* __restrict__ C, const int* __restrict__ last,
    const uint8_t* __restrict__ event,
    double* __restrict__ tile_io,  // [2, ntiles] sums out / suffixes in
    double* __restrict__ suf,      // [2, n]
    int64_t n, int64_t ntiles) {
  __shared__ double ctile[COX_TILE_ROWS];
  const int64_t tile = blockIdx.x, t0 = tile * COX_TILE_ROWS;
  for (int i = threadIdx.x; i < COX_TILE_ROWS; i += SURV_THREADS)
    ctile[i] = t0 + i < n ? C[t0 + i] : 0.0;
  __syncthreads();
  const int64_t s0 = slice_start<true>(tile);
  int lst[RPT], ev[RPT];
  load_i32(last, s0, n, lst, 0);
  load_u8(event, s0, n, ev);
  double ra[RPT], rb[RPT], ta = 0.0, tb = 0.0;
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const int j = RPT - 1 - k;
    double a = 0.0, b = 0.0;
    if (s0 + j < n && ev[j]) {
      const int64_t l = lst[j];
      const double R = clamp_min(
          l < t0 + COX_TILE_ROWS ? ctile[l - t0] : C[l], 1e-300);
      a = 1.0 / R;
      b = 1.0 / (R * R);
    }
    ta += a;
    tb += b;
    ra[j] = ta;
    rb[j] = tb;
  }
  double totala, totalb;
  const double ea = block_excl_scan(ta, totala);
  const double eb = block_excl_scan(tb, totalb);
  if (SUMS) {
    if (threadIdx.x == 0) {
      tile_io[tile] = totala;
      tile_io[ntiles + tile] = totalb;
    }
    return;
  }
  const double basea = tile_io[tile] + ea, baseb = tile_io[ntiles + tile] + eb;
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    if (s0 + j < n) {
      suf[s0 + j] = basea + ra[j];
      suf[n + s0 + j] = baseb + rb[j];
    }
  }
}

// The pair of every row: A and B are the suffix sums at first(s), taken from
// the LDS copy of the tile unless the tie block began in an earlier tile;
// stored at order[s], with this tile's (|g|, |h|) maxima.
__global__ __launch_bounds__(SURV_THREADS) void cox_pair_kernel(
    const float* __restrict__ margin, const float* __restrict__ weight,
    const int* __restrict__ order, const int* __restrict__ first,
    const uint8_t* __restrict__ event, const float* __restrict__ pmax,
    int nparts, const double* __restrict__ suf,  // [2, n]
    float2* __restrict__ out, float* __restrict__ part,  // [ntiles, 2]
    int64_t n) {
  __shared__ double sa[COX_TILE_ROWS], sb[COX_TILE_ROWS];
  const int64_t tile = blockIdx.x, t0 = tile * COX_TILE_ROWS;
  for (int i = threadIdx.x; i < COX_TILE_ROWS; i += SURV_THREADS) {
    const bool in = t0 + i < n;
    sa[i] = in ? suf[t0 + i] : 0.0;
    sb[i] = in ? suf[n + t0 + i] : 0.0;
  }
  const float shift = block_shift(pmax, nparts);  // syncs: the tile is staged
  const int64_t s0 = slice_start<false>(tile);
  int ord[RPT], fst[RPT], ev[RPT];
  float m[RPT];
  double eta[RPT];
  load_i32(order, s0, n, ord, 0);
  load_i32(first, s0, n, fst, 0);
  load_u8(event, s0, n, ev);
  slice_eta(margin, ord, s0, n, shift, m, eta);
  float gm = 0.f, hm = 0.f;
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    if (s0 + j < n) {
      const int64_t f = fst[j];
      const double A = f >= t0 ? sa[f - t0] : suf[f];
      const double B = f >= t0 ? sb[f - t0] : suf[n + f];
      const double ea = eta[j] * A;
      float g = (float)(-(double)ev[j] + ea);
      float h = (float)clamp_min(ea - eta[j] * eta[j] * B, 1e-6);
      if (weight != nullptr) {
        const float w = weight[ord[j]];
        g *= w;
        h *= w;
      }
      out[ord[j]] = {g, h};
      gm = max_keep_nan(gm, fabsf(g));
      hm = max_keep_nan(hm, fabsf(h));
    }
  }
  block_absmax_store(gm, hm, part + 2 * tile);
}

// --------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------
static void check_vec(const char* op, const char* what, const torch::Tensor& t,
                      torch::ScalarType ty, int64_t numel,
                      const torch::Tensor& like) {
  TORCH_CHECK(t.device() == like.device() && t.scalar_type() == ty &&
                  t.is_contiguous() && t.numel() == numel &&
                  (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0,
              op, ": ", what, " must be a contiguous, 16-byte aligned tensor "
              "of ", numel, " elements of its type on margin's GPU");
}

static void aft_check(const char* op, const torch::Tensor& margin,
                      const torch::Tensor& label, const torch::Tensor& weight,
                      int64_t dist, double sigma) {
  TORCH_CHECK(on_gpu(margin) && margin.dim() == 1, op,
              ": margin must be a float32 GPU vector");
  const int64_t n = margin.numel();
  check_vec(op, "margin", margin, torch::kFloat32, n, margin);
  TORCH_CHECK(label.dim() == 2 && label.size(1) == 2, op,
              ": label must be [n, 2] (lower, upper)");
  check_vec(op, "label", label, torch::kFloat32, 2 * n, margin);
  if (weight.numel()) check_vec(op, "weight", weight, torch::kFloat32, n,
                                margin);
  TORCH_CHECK(dist >= 0 && dist <= 2, op, ": unknown distribution ", dist);
  TORCH_CHECK(sigma > 0.0, op, ": sigma must be positive");
}

static inline int aft_blocks(int64_t n) {
  return (int)std::min<int64_t>(
      ceil_div(n, SURV_THREADS * AFT_ROWS_PER_THREAD), AFT_MAX_BLOCKS);
}

// (pairs f32 [n, 2], absmax f32 [2]); dist 0 normal, 1 logistic, 2 extreme
std::vector<torch::Tensor> aft_grad(torch::Tensor margin, torch::Tensor label,
                                    torch::Tensor weight, int64_t dist,
                                    double sigma) {
  aft_check("aft_grad", margin, label, weight, dist, sigma);
  const int64_t n = margin.numel();
  auto opts = margin.options();
  auto out = torch::empty({n, 2}, opts);
  if (n == 0) return {out, torch::zeros({2}, opts)};
  const int blocks = aft_blocks(n);
  auto part = torch::empty({blocks, 2}, opts);
  auto stream = c10::hip::getCurrentHIPStream();
  auto kernel = dist == AFT_NORMAL     ? aft_grad_kernel<AFT_NORMAL>
                : dist == AFT_LOGISTIC ? aft_grad_kernel<AFT_LOGISTIC>
                                       : aft_grad_kernel<AFT_EXTREME>;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(SURV_THREADS), 0,
                     stream.stream(), margin.data_ptr<float>(),
                     (const float2*)label.data_ptr<float>(),
                     weight.numel() ? weight.data_ptr<float>() : nullptr,
                     (float2*)out.data_ptr<float>(), part.data_ptr<float>(), n,
                     sigma);
  CHECK_HIP(hipGetLastError());
  // max is order-free and torch's max keeps NaN: this equals abs().max(0)
  return {out, std::get<0>(part.max(0))};
}

// f64 [2] = [sum w * nll, sum w]
torch::Tensor eval_aft(torch::Tensor margin, torch::Tensor label,
                       torch::Tensor weight, int64_t dist, double sigma) {
  aft_check("eval_aft", margin, label, weight, dist, sigma);
  const int64_t n = margin.numel();
  auto opts = margin.options().dtype(torch::kFloat64);
  if (n == 0) return torch::zeros({2}, opts);
  const int blocks = aft_blocks(n);
  auto part = torch::empty({blocks, 2}, opts);
  auto stream = c10::hip::getCurrentHIPStream();
  auto kernel = dist == AFT_NORMAL     ? eval_aft_kernel<AFT_NORMAL>
                : dist == AFT_LOGISTIC ? eval_aft_kernel<AFT_LOGISTIC>
                                       : eval_aft_kernel<AFT_EXTREME>;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(SURV_THREADS), 0,
                     stream.stream(), margin.data_ptr<float>(),
                     (const float2*)label.data_ptr<float>(),
                     weight.numel() ? weight.data_ptr<float>() : nullptr,
                     part.data_ptr<double>(), n, sigma, std::log(sigma));
  CHECK_HIP(hipGetLastError());
  return part.sum(0);  // fixed-order torch reduction
}

struct CoxArgs {
  int64_t n, ntiles;
  int nparts;
  torch::Tensor pmax, tiles;
};

// Checks, the margin maximum's partials, the forward tile sums and their
// exclusive prefixes (steps 1-3, shared by the gradient and the metric).
static CoxArgs cox_begin(const char* op, const torch::Tensor& margin,
                         const torch::Tensor& order,
                         const torch::Tensor& event, hipStream_t stream) {
  TORCH_CHECK(on_gpu(margin) && margin.dim() == 1, op,
              ": margin must be a float32 GPU vector");
  CoxArgs c;
  c.n = margin.numel();
  TORCH_CHECK(c.n > 0 && c.n <= std::numeric_limits<int32_t>::max(), op,
              ": row count must lie in [1, 2^31 - 1], got ", c.n);
  check_vec(op, "margin", margin, torch::kFloat32, c.n, margin);
  check_vec(op, "order", order, torch::kInt32, c.n, margin);
  check_vec(op, "event", event, torch::kUInt8, c.n, margin);
  c.ntiles = ceil_div(c.n, COX_TILE_ROWS);
  c.nparts = (int)std::min<int64_t>(ceil_div(c.n, SURV_THREADS * 16),
                                    COX_MAX_PARTS);
  c.pmax = torch::empty({c.nparts}, margin.options());
  c.tiles = torch::empty({2, c.ntiles},
                         margin.options().dtype(torch::kFloat64));
  const float* m = margin.data_ptr<float>();
  double* sums = c.tiles.data_ptr<double>();
  double* prefix = sums + c.ntiles;
  hipLaunchKernelGGL(cox_max_kernel, dim3(c.nparts), dim3(SURV_THREADS), 0,
                     stream, m, c.pmax.data_ptr<float>(), c.n);
  hipLaunchKernelGGL((cox_forward_kernel<true, false, false>),
                     dim3((uint32_t)c.ntiles), dim3(SURV_THREADS), 0, stream,
                     m, order.data_ptr<int>(), event.data_ptr<uint8_t>(),
                     c.pmax.data_ptr<float>(), c.nparts, sums, nullptr,
                     nullptr, c.n);
  hipLaunchKernelGGL(cox_tile_scan_kernel<false>, dim3(1), dim3(SURV_THREADS),
                     0, stream, sums, prefix, c.ntiles);
  CHECK_HIP(hipGetLastError());
  return c;
}

// (pairs f32 [n, 2] in row order, absmax f32 [2])
std::vector<torch::Tensor> cox_grad(torch::Tensor margin, torch::Tensor order,
                                    torch::Tensor first, torch::Tensor last,
                                    torch::Tensor event,
                                    torch::Tensor weight) {
  auto stream = c10::hip::getCurrentHIPStream().stream();
  CoxArgs c = cox_begin("cox_grad", margin, order, event, stream);
  const int64_t n = c.n, nt = c.ntiles;
  check_vec("cox_grad", "first", first, torch::kInt32, n, margin);
  check_vec("cox_grad", "last", last, torch::kInt32, n, margin);
  if (weight.numel())
    check_vec("cox_grad", "weight", weight, torch::kFloat32, n, margin);
  auto f64 = margin.options().dtype(torch::kFloat64);
  auto C = torch::empty({n}, f64);
  auto suf = torch::empty({2, n}, f64);
  auto rtiles = torch::empty({4, nt}, f64);  // sums a, b; suffixes a, b
  auto out = torch::empty({n, 2}, margin.options());
  auto part = torch::empty({nt, 2}, margin.options());
  const float* m = margin.data_ptr<float>();
  const uint8_t* ev = event.data_ptr<uint8_t>();
  double* rsum = rtiles.data_ptr<double>();
  const dim3 grid((uint32_t)nt), block(SURV_THREADS);
  hipLaunchKernelGGL((cox_forward_kernel<false, true, false>), grid, block, 0,
                     stream, m, order.data_ptr<int>(), ev,
                     c.pmax.data_ptr<float>(), c.nparts,
                     c.tiles.data_ptr<double>() + nt, C.data_ptr<double>(),
                     nullptr, n);
  hipLaunchKernelGGL(cox_reverse_kernel<true>, grid, block, 0, stream,
                     C.data_ptr<double>(), last.data_ptr<int>(), ev, rsum,
                     nullptr, n, nt);
  hipLaunchKernelGGL(cox_tile_scan_kernel<true>, dim3(2), block, 0, stream,
                     rsum, rsum + 2 * nt, nt);
  hipLaunchKernelGGL(cox_reverse_kernel<false>, grid, block, 0, stream,
                     C.data_ptr<double>(), last.data_ptr<int>(), ev,
                     rsum + 2 * nt, suf.data_ptr<double>(), n, nt);
  hipLaunchKernelGGL(cox_pair_kernel, grid, block, 0, stream, m,
                     weight.numel() ? weight.data_ptr<float>() : nullptr,
                     order.data_ptr<int>(), first.data_ptr<int>(), ev,
                     c.pmax.data_ptr<float>(), c.nparts,
                     suf.data_ptr<double>(), (float2*)out.data_ptr<float>(),
                     part.data_ptr<float>(), n);
  CHECK_HIP(hipGetLastError());
  return {out, std::get<0>(part.max(0))};
}

// f64 [2] = [-ll, number of events]
torch::Tensor eval_cox(torch::Tensor margin, torch::Tensor order,
                       torch::Tensor event) {
  auto stream = c10::hip::getCurrentHIPStream().stream();
  CoxArgs c = cox_begin("eval_cox", margin, order, event, stream);
  auto mpart = torch::empty({c.ntiles, 2},
                            margin.options().dtype(torch::kFloat64));
  hipLaunchKernelGGL((cox_forward_kernel<false, false, true>),
                     dim3((uint32_t)c.ntiles), dim3(SURV_THREADS), 0, stream,
                     margin.data_ptr<float>(), order.data_ptr<int>(),
                     event.data_ptr<uint8_t>(), c.pmax.data_ptr<float>(),
                     c.nparts, c.tiles.data_ptr<double>() + c.ntiles, nullptr,
                     mpart.data_ptr<double>(), c.n);
  CHECK_HIP(hipGetLastError());
  return mpart.sum(0);  // fixed-order torch reduction
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("aft_grad", &aft_grad, "survival:aft pairs + absmax",
        py::arg("margin"), py::arg("label"), py::arg("weight"),
        py::arg("dist"), py::arg("sigma"));
  m.def("eval_aft", &eval_aft, "[sum w * nll, sum w] of survival:aft",
        py::arg("margin"), py::arg("label"), py::arg("weight"),
        py::arg("dist"), py::arg("sigma"));
  m.def("cox_grad", &cox_grad, "survival:cox pairs + absmax",
        py::arg("margin"), py::arg("order"), py::arg("first"),
        py::arg("last"), py::arg("event"), py::arg("weight"));
  m.def("eval_cox", &eval_cox, "[-ll, events] of survival:cox",
        py::arg("margin"), py::arg("order"), py::arg("event"));
  m.attr("COX_TILE_ROWS") = (int)COX_TILE_ROWS;
}
