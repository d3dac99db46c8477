// Weighted quantile sketch kernels for AMD Instinct MI355X (CDNA4, gfx950):
// the radix-select passes behind ops.weighted_cuts (tree_method="approx") and
// the re-bin of the raw features into the resident bin matrix.
// Built as its own extension module (xgboost_ray_amd._hip_sketch_ops), so
// that adding it leaves the build lines and the generated code of the other
// modules as they were. Contract: docs/parity.md "Per-tree weighted sketch".
//
// One pass reads X [n, F] once, flat and coalesced: consecutive lanes take
// consecutive addresses (16 bytes per lane where the pointer allows), and
// the feature of an element is its flat index mod F, carried along the
// grid-stride walk as a (row, feature) pair so the loop holds no division.
// Every sum is an int64 atomic add: the order does not matter, equal inputs
// give equal bytes, and the result equals the CPU oracle's.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <cstdint>

#define CHECK_HIP(x)                                                         \
  do {                                                                       \
    hipError_t err = (x);                                                    \
    TORCH_CHECK(err == hipSuccess, "HIP error: ", hipGetErrorString(err));   \
  } while (0)

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// torch spells the ROCm GPU device type with its legacy vendor name in the
// public tensor API; isolate that single spelling here.
static inline bool on_gpu(const torch::Tensor& t) { return t.is_cuda(); }

#define SK_THREADS 256
// Features per workgroup in pass 0: 28 x 256 int64 bins = 56 KiB of LDS, two
// workgroups per CU. A wider matrix is covered by blockIdx.y tiles.
#define SK_FTILE 28
#define SK_PASS0_BLOCKS 512
#define SK_MAX_BLOCKS 4096
#define SK_LDS_LIMIT (64 * 1024)

typedef unsigned long long u64;

// order-preserving uint32 key of ops.cpu.quantile_keys. -0.0 folds into +0.0
// on the bits, so no float add stands between a denormal and its key.
__device__ __forceinline__ uint32_t sk_key(float v) {
  uint32_t u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Flat walk over the n * F elements of X in units of VEC floats. fn(value,
// row, feature) sees every element exactly once per blockIdx.y; the
// total % VEC tail elements go to the first threads of block x == 0.
template <int VEC, typename Fn>
__device__ __forceinline__ void sk_walk(const float* __restrict__ X,
                                        int64_t total, int F, Fn fn) {
  const int64_t units = total / VEC;
  int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ustride = (int64_t)gridDim.x * blockDim.x;
  int64_t row = (u * VEC) / F;
  int f = (int)(u * VEC - row * F);
  const int64_t srow = (ustride * VEC) / F;
  const int sf = (int)(ustride * VEC - srow * F);
  for (; u < units; u += ustride) {
    float v[VEC];
    if constexpr (VEC == 4) {
      const float4 q = reinterpret_cast<const float4*>(X)[u];
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      v[0] = X[u];
    }
    int ff = f;
    int64_t rr = row;
    #pragma unroll
    for (int k = 0; k < VEC; ++k) {
      fn(v[k], rr, ff);
      if (++ff == F) { ff = 0; ++rr; }
    }
    f += sf;
    row += srow;
    if (f >= F) { f -= F; ++row; }
  }
  if (VEC > 1 && blockIdx.x == 0) {
    const int64_t i = units * VEC + threadIdx.x;
    if (i < total) fn(X[i], i / F, (int)(i % F));
  }
}

// ---------------------------------------------------------------------------
// Pass 0: out[f * S * 256 + digit] += W[row], digit = the key's top 8 bits
// (slot 0 of feature f). The digit is sign + 7 exponent bits, so a feature's
// mass falls on a handful of bins: the workgroup keeps [ftile][256] int64
// bins in LDS, takes the contention there and flushes its non-zero bins once.
// ---------------------------------------------------------------------------
template <int VEC, typename WT>
__global__ __launch_bounds__(SK_THREADS) void sketch_pass0_kernel(
    const float* __restrict__ X, const WT* __restrict__ W, int64_t w_stride,
    int64_t total, int F, int S, long long* __restrict__ out) {
  extern __shared__ u64 sk_lds[];
  const int f_lo = blockIdx.y * SK_FTILE;
  const int ftile = min(SK_FTILE, F - f_lo);
  for (int i = threadIdx.x; i < ftile * 256; i += SK_THREADS) sk_lds[i] = 0ull;
  __syncthreads();
  sk_walk<VEC>(X, total, F, [&](float v, int64_t row, int f) {
    const int ft = f - f_lo;
    if (v != v || ft < 0 || ft >= ftile) return;
    const long long w = (long long)W[row * w_stride];
    if (w > 0) atomicAdd(&sk_lds[ft * 256 + (sk_key(v) >> 24)], (u64)w);
  });
  __syncthreads();
  for (int i = threadIdx.x; i < ftile * 256; i += SK_THREADS) {
    const u64 s = sk_lds[i];
    if (s != 0ull)
      atomicAdd((u64*)&out[((size_t)(f_lo + (i >> 8)) * S) * 256 + (i & 255)],
                s);
  }
}

// ---------------------------------------------------------------------------
// Passes 1..3: table[f][0 .. n_slots[f]) holds the feature's active key
// prefixes (the top 8 * pass bits), ascending and distinct. An element whose
// prefix is in the table adds its weight to out[(f * S + slot) * 256 + digit]
// (digit = the next 8 key bits) with a global int64 atomic; W is gathered only
// then. The tables are staged in LDS when F * (S + 1) words fit, else read
// from global memory (they are small and stay in L2).
// ---------------------------------------------------------------------------
template <int VEC, typename WT, bool LDS_TABLE>
__global__ __launch_bounds__(SK_THREADS) void sketch_pass_kernel(
    const float* __restrict__ X, const WT* __restrict__ W, int64_t w_stride,
    int64_t total, int F, int S, const int32_t* __restrict__ table,
    const int32_t* __restrict__ n_slots, int pass,
    long long* __restrict__ out) {
  extern __shared__ int32_t sk_tab[];
  const int32_t* T = table;
  const int32_t* NS = n_slots;
  if (LDS_TABLE) {
    for (int i = threadIdx.x; i < F * S; i += SK_THREADS) sk_tab[i] = table[i];
    for (int i = threadIdx.x; i < F; i += SK_THREADS)
      sk_tab[F * S + i] = n_slots[i];
    __syncthreads();
    T = sk_tab;
    NS = sk_tab + F * S;
  }
  const int hi_shift = 32 - 8 * pass;
  const int lo_shift = 24 - 8 * pass;
  sk_walk<VEC>(X, total, F, [&](float v, int64_t row, int f) {
    if (v != v) return;
    const uint32_t key = sk_key(v);
    const int32_t pfx = (int32_t)(key >> hi_shift);  // at most 24 bits
    const int32_t* tf = T + (size_t)f * S;
    int lo = 0, hi = min(NS[f], S);  // first slot with tf[slot] >= pfx
    const int ns = hi;
    while (lo < hi) {
      const int m = (lo + hi) >> 1;
      if (tf[m] < pfx) lo = m + 1; else hi = m;
    }
    if (lo >= ns || tf[lo] != pfx) return;
    const long long w = (long long)W[row * w_stride];
    if (w > 0)
      atomicAdd((u64*)&out[((size_t)f * S + lo) * 256 +
                           ((key >> lo_shift) & 255u)],
                (u64)w);
  });
}

// ---------------------------------------------------------------------------
// rebin: the bin_matrix rule (bin = number of cuts <= v, clamped to the
// feature's bin count - 1; NaN -> 255; 0 for a feature without cuts) written
// into an existing uint8 matrix of any row stride, on the same flat walk.
// ---------------------------------------------------------------------------
template <int VEC, bool LDS_CUTS>
__global__ __launch_bounds__(SK_THREADS) void rebin_kernel(
    const float* __restrict__ X, int64_t total, int F,
    const float* __restrict__ cuts, const int64_t* __restrict__ cut_ptr,
    int total_cuts, uint8_t* __restrict__ out, int64_t out_stride) {
  extern __shared__ float sk_cuts[];
  const float* C = cuts;
  if (LDS_CUTS) {
    for (int i = threadIdx.x; i < total_cuts; i += SK_THREADS)
      sk_cuts[i] = cuts[i];
    __syncthreads();
    C = sk_cuts;
  }
  sk_walk<VEC>(X, total, F, [&](float v, int64_t row, int f) {
    const int lo = (int)cut_ptr[f];
    const int nb = (int)cut_ptr[f + 1] - lo;
    uint8_t b;
    if (v != v) {
      b = 255;
    } else if (nb == 0) {
      b = 0;
    } else {
      int l = 0, r = nb;  // upper_bound: first cut > v
      while (l < r) {
        const int m = (l + r) >> 1;
        if (C[lo + m] <= v) l = m + 1; else r = m;
      }
      b = (uint8_t)min(l, nb - 1);
    }
    out[row * out_stride + f] = b;
  });
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
static inline bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

template <int VEC, typename WT>
static void launch_pass(const float* X, const WT* W, int64_t w_stride,
                        int64_t total, int F, int S, const int32_t* table,
                        const int32_t* n_slots, int pass, long long* out,
                        hipStream_t stream) {
  const int64_t units = std::max<int64_t>(total / VEC, 1);
  if (pass == 0) {
    const int blocks =
        (int)std::min<int64_t>(ceil_div(units, SK_THREADS), SK_PASS0_BLOCKS);
    const size_t lds = (size_t)std::min(F, SK_FTILE) * 256 * sizeof(u64);
    hipLaunchKernelGGL((sketch_pass0_kernel<VEC, WT>),
                       dim3(blocks, (unsigned)ceil_div(F, SK_FTILE)),
                       dim3(SK_THREADS), lds, stream, X, W, w_stride, total, F,
                       S, out);
  } else {
    const int blocks =
        (int)std::min<int64_t>(ceil_div(units, SK_THREADS), SK_MAX_BLOCKS);
    const size_t lds = ((size_t)F * S + F) * sizeof(int32_t);
    if (lds <= SK_LDS_LIMIT) {
      hipLaunchKernelGGL((sketch_pass_kernel<VEC, WT, true>), dim3(blocks),
                         dim3(SK_THREADS), lds, stream, X, W, w_stride, total,
                         F, S, table, n_slots, pass, out);
    } else {
      hipLaunchKernelGGL((sketch_pass_kernel<VEC, WT, false>), dim3(blocks),
                         dim3(SK_THREADS), 0, stream, X, W, w_stride, total, F,
                         S, table, n_slots, pass, out);
    }
  }
  CHECK_HIP(hipGetLastError());
}

// One radix-select pass, accumulated into out (int64 [F * S, 256]).
// X: f32 [n, F] contiguous, any 4-byte-aligned start; W: int32 or int64 [n],
// any stride; table: int32 [F, S]; n_slots: int32 [F] (both unread in pass 0).
void sketch_pass(torch::Tensor X, torch::Tensor W, torch::Tensor table,
                 torch::Tensor n_slots, int64_t pass, int64_t S,
                 torch::Tensor out) {
  TORCH_CHECK(on_gpu(X) && X.dim() == 2 && X.is_contiguous() &&
              X.scalar_type() == torch::kFloat32,
              "sketch_pass: X must be a contiguous f32 [n, F] GPU tensor");
  const int64_t n = X.size(0), F = X.size(1);
  TORCH_CHECK(on_gpu(W) && W.dim() == 1 && W.size(0) == n &&
              (W.scalar_type() == torch::kInt32 ||
               W.scalar_type() == torch::kInt64),
              "sketch_pass: W must be int32 or int64 [n] on the GPU");
  TORCH_CHECK(pass >= 0 && pass <= 3 && S >= 1 && S <= 254 && F >= 1 &&
              F * S < (1 << 24), "sketch_pass: bad pass / S / F");
  TORCH_CHECK(on_gpu(out) && out.is_contiguous() &&
              out.scalar_type() == torch::kInt64 &&
              out.numel() == F * S * 256,
              "sketch_pass: out must be int64 [F * S, 256]");
  if (pass > 0) {
    TORCH_CHECK(on_gpu(table) && table.is_contiguous() &&
                table.scalar_type() == torch::kInt32 &&
                table.numel() == F * S && on_gpu(n_slots) &&
                n_slots.is_contiguous() &&
                n_slots.scalar_type() == torch::kInt32 &&
                n_slots.numel() == F,
                "sketch_pass: table int32 [F, S], n_slots int32 [F]");
  }
  if (n == 0) return;
  const int64_t total = n * F;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const float* x = X.data_ptr<float>();
  const int32_t* tab = pass > 0 ? table.data_ptr<int32_t>() : nullptr;
  const int32_t* ns = pass > 0 ? n_slots.data_ptr<int32_t>() : nullptr;
  long long* o = reinterpret_cast<long long*>(out.data_ptr<int64_t>());
  const int64_t ws = W.stride(0);
  const bool vec = aligned16(x);
  if (W.scalar_type() == torch::kInt32) {
    const int32_t* w = W.data_ptr<int32_t>();
    if (vec) launch_pass<4>(x, w, ws, total, (int)F, (int)S, tab, ns, (int)pass, o, stream);
    else launch_pass<1>(x, w, ws, total, (int)F, (int)S, tab, ns, (int)pass, o, stream);
  } else {
    const int64_t* w = W.data_ptr<int64_t>();
    if (vec) launch_pass<4>(x, w, ws, total, (int)F, (int)S, tab, ns, (int)pass, o, stream);
    else launch_pass<1>(x, w, ws, total, (int)F, (int)S, tab, ns, (int)pass, o, stream);
  }
}

template <int VEC>
static void launch_rebin(const float* X, int64_t total, int F,
                         const float* cuts, const int64_t* cut_ptr,
                         int total_cuts, uint8_t* out, int64_t out_stride,
                         hipStream_t stream) {
  const int64_t units = std::max<int64_t>(total / VEC, 1);
  const int blocks =
      (int)std::min<int64_t>(ceil_div(units, SK_THREADS), SK_MAX_BLOCKS);
  const size_t lds = (size_t)total_cuts * sizeof(float);
  if (lds <= SK_LDS_LIMIT) {
    hipLaunchKernelGGL((rebin_kernel<VEC, true>), dim3(blocks),
                       dim3(SK_THREADS), lds, stream, X, total, F, cuts,
                       cut_ptr, total_cuts, out, out_stride);
  } else {
    hipLaunchKernelGGL((rebin_kernel<VEC, false>), dim3(blocks),
                       dim3(SK_THREADS), 0, stream, X, total, F, cuts, cut_ptr,
                       total_cuts, out, out_stride);
  }
  CHECK_HIP(hipGetLastError());
}

// Bin X with the given cuts into out (uint8 [n, F], unit column stride, any
// row stride >= F): the storage of the resident bin matrix.
void rebin(torch::Tensor X, torch::Tensor cuts_flat, torch::Tensor cut_ptr,
           torch::Tensor out) {
  TORCH_CHECK(on_gpu(X) && X.dim() == 2 && X.is_contiguous() &&
              X.scalar_type() == torch::kFloat32,
              "rebin: X must be a contiguous f32 [n, F] GPU tensor");
  const int64_t n = X.size(0), F = X.size(1);
  TORCH_CHECK(on_gpu(out) && out.dim() == 2 && out.size(0) == n &&
              out.size(1) == F && out.scalar_type() == torch::kUInt8 &&
              (n <= 1 || out.stride(0) >= F) && (F <= 1 || out.stride(1) == 1),
              "rebin: out must be uint8 [n, F] with unit column stride");
  TORCH_CHECK(on_gpu(cuts_flat) && cuts_flat.is_contiguous() &&
              cuts_flat.scalar_type() == torch::kFloat32 &&
              on_gpu(cut_ptr) && cut_ptr.is_contiguous() &&
              cut_ptr.scalar_type() == torch::kInt64 &&
              cut_ptr.numel() == F + 1,
              "rebin: cuts_flat f32, cut_ptr int64 [F + 1] on the GPU");
  if (n == 0 || F == 0) return;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const float* x = X.data_ptr<float>();
  if (aligned16(x))
    launch_rebin<4>(x, n * F, (int)F, cuts_flat.data_ptr<float>(),
                    cut_ptr.data_ptr<int64_t>(), (int)cuts_flat.numel(),
                    out.data_ptr<uint8_t>(), out.stride(0), stream);
  else
    launch_rebin<1>(x, n * F, (int)F, cuts_flat.data_ptr<float>(),
                    cut_ptr.data_ptr<int64_t>(), (int)cuts_flat.numel(),
                    out.data_ptr<uint8_t>(), out.stride(0), stream);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "xgboost_ray_amd weighted quantile sketch kernels (gfx950)";
  m.attr("MAX_SLOTS") = 254;
  m.def("sketch_pass", &sketch_pass, "one radix-select pass of the sketch");
  m.def("rebin", &rebin, "bin raw features into an existing bin matrix");
}
