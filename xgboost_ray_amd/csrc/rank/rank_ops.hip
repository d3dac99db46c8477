// Ranking kernels for AMD Instinct MI355X (CDNA4, gfx950): the in-LDS group
// sort, ranks + DCG / AP sums, the rank:map pair loop and the LambdaRank
// pair loop with top-k truncation. Built as its own
// extension module (xgboost_ray_amd._hip_rank_ops), so that adding it leaves
// the build line and the generated code of csrc/kernels.hip as they were.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
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

// ---------------------------------------------------------------------------
// Ranking on the device (contract: docs/parity.md "Ranking on the device").
//
// One primitive serves rank:ndcg's preparation, rank:map and the ndcg / map
// metrics: a stable descending sort of the margins inside every query group,
// one launch for all groups. A row's sort key is 64 bits,
//   (~okey(margin) << 32) | local_index,
// with okey the order-preserving uint32 image of a float32 (-0.0 first mapped
// to +0.0, so the two zeros tie). Keys are distinct, so the ASCENDING bitonic
// network - which is not stable - returns the stable DESCENDING margin order.
// Groups are padded to a power of two P >= 64 with all-ones keys, which sort
// last. No address depends on a margin: a key's low half is a local index
// < L by construction and pads are never dereferenced.
//
// The network is split by stride. Strides below 64 exchange through
// __shfl_xor with one element per lane (no LDS traffic, no barrier); strides
// of 64 and more go through LDS with one barrier each. A group of at most 64
// rows therefore sorts entirely in registers, and rank_stats_wave_kernel
// packs one such group per wave. Longer groups take one workgroup each
// (rank_stats_block_kernel, lambdamap_kernel) and pad to the power of two of
// THEIR length, not of the launch's longest group.
//
// Every sum runs in a fixed order (rank order inside a lane, a xor butterfly
// inside a wave, wave order across waves) and nothing is atomic, so two
// launches return the same bytes.
// ---------------------------------------------------------------------------
#define RANK_LDS_MAX_GROUP 2048
#define RANK_MAX_THREADS 256
#define RANK_MAX_WAVES (RANK_MAX_THREADS / WAVE)

__device__ __forceinline__ uint32_t rank_okey(float v) {
  if (v == 0.f) v = 0.f;  // -0.0 -> +0.0
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float rank_okey_inv(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}
__device__ __forceinline__ unsigned long long rank_key(float m, int idx) {
  return ((unsigned long long)(~rank_okey(m)) << 32) | (uint32_t)idx;
}
__device__ __forceinline__ int rank_pad(int len) {
  int P = WAVE;
  while (P < len) P <<= 1;
  return P;
}

// Strides jstart..1 of bitonic stage k for element e (one element per lane,
// the wave holds 64 consecutive elements).
template <typename K>
__device__ __forceinline__ K bitonic_lane_steps(K key, int e, int k,
                                                int jstart) {
  const bool asc = (e & k) == 0;
  for (int j = jstart; j >= 1; j >>= 1) {
    const K o = __shfl_xor(key, j);
    const bool lower = (e & j) == 0;
    const K lo = o < key ? o : key, hi = o < key ? key : o;
    key = (lower == asc) ? lo : hi;
  }
  return key;
}

// 64 elements, one per lane, fully sorted ascending.
template <typename K>
__device__ __forceinline__ K bitonic_wave_sort(K key, int lane) {
  for (int k = 2; k <= WAVE; k <<= 1)
    key = bitonic_lane_steps(key, lane, k, k >> 1);
  return key;
}

// Ascending sort of s[0..P) in LDS, P a power of two >= 64, by the whole
// workgroup (blockDim.x a multiple of 64). TWO sorts a second array in the
// same steps, so both share the barriers.
template <typename KA, typename KB, bool TWO>
__device__ __forceinline__ void bitonic_block_sort(KA* sa, KB* sb, int P) {
  const int T = blockDim.x, tid = threadIdx.x, lane = tid & (WAVE - 1);
  for (int base = tid - lane; base < P; base += T) {
    const int e = base + lane;
    KA ka = sa[e];
    KB kb = TWO ? sb[e] : KB(0);
    for (int k = 2; k <= WAVE; k <<= 1) {
      ka = bitonic_lane_steps(ka, e, k, k >> 1);
      if (TWO) kb = bitonic_lane_steps(kb, e, k, k >> 1);
    }
    sa[e] = ka;
    if (TWO) sb[e] = kb;
  }
  __syncthreads();
  for (int k = 2 * WAVE; k <= P; k <<= 1) {
    for (int j = k >> 1; j >= WAVE; j >>= 1) {
      for (int i = tid; i < (P >> 1); i += T) {
        const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a | j;
        const bool asc = (a & k) == 0;
        const KA xa = sa[a], ya = sa[b];
        if ((xa > ya) == asc) { sa[a] = ya; sa[b] = xa; }
        if (TWO) {
          const KB xb = sb[a], yb = sb[b];
          if ((xb > yb) == asc) { sb[a] = yb; sb[b] = xb; }
        }
      }
      __syncthreads();
    }
    for (int base = tid - lane; base < P; base += T) {
      const int e = base + lane;
      sa[e] = bitonic_lane_steps(sa[e], e, k, WAVE >> 1);
      if (TWO) sb[e] = bitonic_lane_steps(sb[e], e, k, WAVE >> 1);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int o = WAVE >> 1; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int wave_incl_scan_i32(int v, int lane) {
  for (int o = 1; o < WAVE; o <<= 1) {
    const int u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}
__device__ __forceinline__ bool rank_group_ok(int64_t s0, int64_t s1,
                                              int64_t n, int cap) {
  return s0 >= 0 && s1 >= s0 && s1 <= n && s1 - s0 <= cap;
}

// stats[g] = [dcg@k, idcg@k, idcg, ap]; k <= 0 means the whole group.
// Wave per group (L <= 64): sort, ranks and all four sums in registers.
__global__ __launch_bounds__(RANK_MAX_THREADS) void rank_stats_wave_kernel(
    const float* __restrict__ margin, const float* __restrict__ label,
    const int64_t* __restrict__ group_ptr, const double* __restrict__ disc,
    int32_t* __restrict__ rank, double* __restrict__ stats, int G, int64_t n,
    int k) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int g = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  if (g >= G) return;  // wave-uniform
  const int64_t s0 = group_ptr[g], s1 = group_ptr[g + 1];
  if (!rank_group_ok(s0, s1, n, WAVE)) return;
  const int L = (int)(s1 - s0);
  const int kk = (k <= 0 || k > L) ? L : k;
  const bool live = lane < L;
  const float m = live ? margin[s0 + lane] : 0.f;
  const float y = live ? label[s0 + lane] : 0.f;
  unsigned long long key = live ? rank_key(m, lane) : ~0ull;
  uint32_t lkey = live ? ~rank_okey(y) : ~0u;
  key = bitonic_wave_sort(key, lane);
  lkey = bitonic_wave_sort(lkey, lane);
  // lane p now holds rank p
  const int idx = (int)(uint32_t)key & (WAVE - 1);
  const float yr = __shfl(y, idx);
  if (live) rank[s0 + ((uint32_t)key)] = lane;
  const double d = live ? disc[lane] : 0.0;
  const double gain = exp2((double)yr) - 1.0;
  const double igain = exp2((double)rank_okey_inv(~lkey)) - 1.0;
  const int rel = (live && yr > 0.f) ? 1 : 0;
  const int prefix = wave_incl_scan_i32(rel, lane);
  const int R = __shfl(prefix, WAVE - 1);
  const double iterm = live ? igain * d : 0.0;
  const double dcgk = wave_sum_f64(lane < kk ? gain * d : 0.0);
  const double idcgk = wave_sum_f64(lane < kk ? iterm : 0.0);
  const double idcg = wave_sum_f64(iterm);
  const double ap =
      wave_sum_f64(rel ? (double)prefix / (double)(lane + 1) : 0.0);
  if (lane == 0) {
    double* o = stats + (size_t)g * 4;
    o[0] = dcgk;
    o[1] = idcgk;
    o[2] = idcg;
    o[3] = R > 0 ? ap / (double)R : 0.0;
  }
}

// Workgroup per group (L <= RANK_LDS_MAX_GROUP). Dynamic LDS, for the
// launch's longest padded group Pmax: u64 keys [Pmax], f32 labels in row
// order [Pmax], u32 label keys [Pmax] = 16 B per element.
__global__ __launch_bounds__(RANK_MAX_THREADS) void rank_stats_block_kernel(
    const float* __restrict__ margin, const float* __restrict__ label,
    const int64_t* __restrict__ group_ptr, const double* __restrict__ disc,
    int32_t* __restrict__ rank, double* __restrict__ stats, int64_t n, int k,
    int Pmax) {
  extern __shared__ unsigned long long rank_smem[];
  __shared__ double s_red[4][RANK_MAX_WAVES];
  __shared__ int s_cnt[RANK_MAX_WAVES];
  unsigned long long* skey = rank_smem;
  float* slab = (float*)(skey + Pmax);
  uint32_t* lkey = (uint32_t*)(slab + Pmax);
  const int g = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int lane = tid & (WAVE - 1), wv = tid / WAVE, nw = T / WAVE;
  const int64_t s0 = group_ptr[g], s1 = group_ptr[g + 1];
  if (!rank_group_ok(s0, s1, n, Pmax)) return;  // block-uniform
  const int L = (int)(s1 - s0);
  const int P = rank_pad(L);
  const int kk = (k <= 0 || k > L) ? L : k;
  for (int e = tid; e < P; e += T) {
    const bool live = e < L;
    const float y = live ? label[s0 + e] : 0.f;
    skey[e] = live ? rank_key(margin[s0 + e], e) : ~0ull;
    slab[e] = y;
    lkey[e] = live ? ~rank_okey(y) : ~0u;
  }
  __syncthreads();
  bitonic_block_sort<unsigned long long, uint32_t, true>(skey, lkey, P);
  // thread t owns ranks [t*C, (t+1)*C): rank order inside the lane
  const int C = (P + T - 1) / T;
  const int p0 = min(tid * C, L), p1 = min(p0 + C, L);
  int cnt = 0;
  for (int p = p0; p < p1; ++p) cnt += slab[(uint32_t)skey[p]] > 0.f;
  const int incl = wave_incl_scan_i32(cnt, lane);
  if (lane == WAVE - 1) s_cnt[wv] = incl;
  __syncthreads();
  int before = incl - cnt, R = 0;
  for (int w = 0; w < nw; ++w) {
    if (w < wv) before += s_cnt[w];
    R += s_cnt[w];
  }
  double dcgk = 0.0, idcgk = 0.0, idcg = 0.0, ap = 0.0;
  for (int p = p0; p < p1; ++p) {
    const uint32_t idx = (uint32_t)skey[p];
    rank[s0 + idx] = p;
    const float y = slab[idx];
    const double d = disc[p];
    const double it = (exp2((double)rank_okey_inv(~lkey[p])) - 1.0) * d;
    idcg += it;
    if (p < kk) {
      dcgk += (exp2((double)y) - 1.0) * d;
      idcgk += it;
    }
    if (y > 0.f) {
      ++before;
      ap += (double)before / (double)(p + 1);
    }
  }
  dcgk = wave_sum_f64(dcgk);
  idcgk = wave_sum_f64(idcgk);
  idcg = wave_sum_f64(idcg);
  ap = wave_sum_f64(ap);
  if (lane == 0) {
    s_red[0][wv] = dcgk;
    s_red[1][wv] = idcgk;
    s_red[2][wv] = idcg;
    s_red[3][wv] = ap;
  }
  __syncthreads();
  if (tid < 4) {
    double v = s_red[tid][0];
    for (int w = 1; w < nw; ++w) v += s_red[tid][w];
    if (tid == 3) v = R > 0 ? v / (double)R : 0.0;
    stats[(size_t)g * 4 + tid] = v;
  }
}

// rank:map pair kernel, one workgroup per group. After the sort the keys
// are dead and their LDS is reused; per element of the padded group:
//   row order : margin f32, label f32, rank i32           12 B
//   rank order: t f64 (aliases the sort keys), S f64      16 B
// with, for rank p (rel = label > 0),
//   prefix[p] = #rel in ranks 0..p,  t[p] = prefix[p] / (p + 1),
//   S[p] = sum_{q <= p} rel_q / (q + 1)   summed in rank order, so S and
//   every difference S[a] - S[b] are the bits of a sequential cumsum.
// One thread runs that L-step running sum (one add per rank; the divides
// are done by all threads before and after it) rather than a parallel scan,
// whose association would differ: a delta that is exactly 0 in the contract
// must be exactly 0 here. Its share of the kernel's time is not measured;
// the pair loop below has L^2 / T steps with an exp each.
// The pair loop reads LDS only; thread owns rows i = tid, tid + T, ... and
// walks j in row order accumulating in float64 -> fixed order, no atomics.
__global__ __launch_bounds__(RANK_MAX_THREADS) void lambdamap_kernel(
    const float* __restrict__ margin, const float* __restrict__ label,
    const int64_t* __restrict__ group_ptr, float2* __restrict__ out,
    int64_t n, int Pmax) {
  extern __shared__ unsigned long long rank_smem[];
  __shared__ int s_R;
  unsigned long long* skey = rank_smem;
  double* st = (double*)rank_smem;  // alias, live after the sort
  double* sS = st + Pmax;
  float* sm = (float*)(sS + Pmax);
  float* sy = sm + Pmax;
  int* srank = (int*)(sy + Pmax);
  const int g = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int64_t s0 = group_ptr[g], s1 = group_ptr[g + 1];
  if (!rank_group_ok(s0, s1, n, Pmax)) return;  // block-uniform
  const int L = (int)(s1 - s0);
  if (L < 2) return;  // `out` starts zeroed
  const int P = rank_pad(L);
  for (int e = tid; e < P; e += T) {
    const bool live = e < L;
    const float m = live ? margin[s0 + e] : 0.f;
    skey[e] = live ? rank_key(m, e) : ~0ull;
    sm[e] = m;
    sy[e] = live ? label[s0 + e] : 0.f;
  }
  __syncthreads();
  bitonic_block_sort<unsigned long long, uint32_t, false>(skey, nullptr, P);
  for (int p = tid; p < L; p += T) {
    const uint32_t idx = (uint32_t)skey[p];
    srank[idx] = p;
    sS[p] = sy[idx] > 0.f ? 1.0 / (double)(p + 1) : 0.0;
  }
  __syncthreads();  // keys dead from here: st may be written
  if (tid == 0) {
    int cnt = 0;
    double acc = 0.0;
    for (int p = 0; p < L; ++p) {
      const double term = sS[p];
      cnt += term != 0.0;
      acc += term;
      sS[p] = acc;
      st[p] = (double)cnt;
    }
    s_R = cnt;
  }
  __syncthreads();
  const int R = s_R;
  if (R == 0) return;  // block-uniform; zeros stay
  for (int p = tid; p < L; p += T) st[p] = st[p] / (double)(p + 1);
  __syncthreads();
  const double invR = 1.0 / (double)R;
  for (int i = tid; i < L; i += T) {
    const float yi = sy[i], mi = sm[i];
    const int ri = srank[i];
    double gacc = 0.0, hacc = 0.0;
    for (int j = 0; j < L; ++j) {
      const float yj = sy[j];
      if (yj == yi) continue;
      const float mj = sm[j];
      const int rj = srank[j];
      const int lo = min(ri, rj), hi = max(ri, rj);  // hi >= 1
      const double delta =
          fabs(st[hi] - st[lo] - (sS[hi - 1] - sS[lo])) * invR;
      const bool win = yi > yj;
      const double rho =
          1.0 / (1.0 + exp((double)(win ? mi - mj : mj - mi)));
      double hij = rho * (1.0 - rho);
      if (hij < 1e-16) hij = 1e-16;
      gacc += win ? -(rho * delta) : rho * delta;
      hacc += hij * delta;
    }
    out[s0 + i] = make_float2((float)gacc, (float)hacc);
  }
}

// ---------------------------------------------------------------------------
// LambdaRank with top-k pair truncation (rank:pairwise / rank:ndcg,
// lambdarank_pair_method="topk"): a pair (i, j) with label_i > label_j
// counts iff min(rank_i, rank_j) < k. One launch sorts every group, forms
// idcg and runs the pair loop; the loop works in RANK space, so the
// truncation is a loop bound and not a test per pair.
//
// One pair term of row p against partner q (both in rank order). The row
// collects -rho w when it wins the pair and +rho w when it loses it.
template <bool NDCG>
__device__ __forceinline__ void topk_pair(float mp, float yp, double gp,
                                          double dp, float mq, float yq,
                                          double gq, double dq, double inv,
                                          double& g, double& h) {
  if (yq == yp) return;
  const bool win = yp > yq;
  const double rho = 1.0 / (1.0 + exp((double)(win ? mp - mq : mq - mp)));
  double hij = rho * (1.0 - rho);
  if (hij < 1e-16) hij = 1e-16;
  if (NDCG) {
    const double w = fabs((gp - gq) * (dp - dq)) * inv;
    g += win ? -(rho * w) : rho * w;
    h += hij * w;
  } else {
    g += win ? -rho : rho;
    h += hij;
  }
}

// Workgroup per group (L <= RANK_LDS_MAX_GROUP). Dynamic LDS per element of
// the launch's largest padded group Pmax, all of it indexed by rank p once
// the sort is done:
//   u64 sort key [Pmax]   8 B  low word = row index inside the group (kept),
//                              high word rewritten in place to the margin
//                              f32: okey is invertible, so the sorted key
//                              IS the rank-ordered margin (-0.0 comes back
//                              as +0.0; every difference keeps its value)
//   f32 label, row order  4 B  dead after the gather; then the wave sums
//   u32 label key [Pmax]  4 B  sorted with the margins for idcg; element p
//                              is read, then overwritten by label-at-rank-p
//   f64 gain, f64 disc   16 B  ndcg only, one exp2 per element
// = 32 B (ndcg: 64 KiB at P = 2048, two workgroups per 160 KiB CU) or 16 B
// (pairwise: 32 KiB, five per CU by LDS). No static LDS, so the largest
// launch is exactly 64 KiB.
// Pair loop, LDS reads only, kk = min(k, L):
//   head rows p < kk have L - 1 partners: one WAVE per row, lane l takes
//     q = l, l + 64, ... ascending; xor butterfly; lane 0 stores.
//   tail rows p >= kk have kk partners: one THREAD per row, q = 0 .. kk-1
//     ascending (every lane reads the same q: an LDS broadcast).
// Both halves cost about kk * L / 64 wave steps. Sums are float64 in that
// fixed order, one float32 store per row, no atomics.
template <bool NDCG>
__global__ __launch_bounds__(RANK_MAX_THREADS) void lambdarank_topk_kernel(
    const float* __restrict__ margin, const float* __restrict__ label,
    const int64_t* __restrict__ group_ptr, const double* __restrict__ disc,
    float2* __restrict__ out, int64_t n, int k, int Pmax) {
  extern __shared__ unsigned long long rank_smem[];
  unsigned long long* skey = rank_smem;
  const uint32_t* sidx = (const uint32_t*)rank_smem;  // word 2p, after sort
  float* smar = (float*)rank_smem;                    // word 2p + 1
  float* slab = (float*)(skey + Pmax);
  uint32_t* lkey = (uint32_t*)(slab + Pmax);
  float* sy = (float*)lkey;
  double* sgain = (double*)(lkey + Pmax);
  double* sdisc = sgain + Pmax;
  double* sred = (double*)slab;  // Pmax >= 64 floats: room for every wave
  const int g = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int lane = tid & (WAVE - 1), wv = tid / WAVE, nw = T / WAVE;
  const int64_t s0 = group_ptr[g], s1 = group_ptr[g + 1];
  if (!rank_group_ok(s0, s1, n, Pmax)) return;  // block-uniform
  const int L = (int)(s1 - s0);
  if (L < 2) return;  // `out` starts zeroed
  const int P = rank_pad(L);
  for (int e = tid; e < P; e += T) {
    const bool live = e < L;
    const float y = live ? label[s0 + e] : 0.f;
    skey[e] = live ? rank_key(margin[s0 + e], e) : ~0ull;
    slab[e] = y;
    if (NDCG) lkey[e] = live ? ~rank_okey(y) : ~0u;
  }
  __syncthreads();
  bitonic_block_sort<unsigned long long, uint32_t, NDCG>(skey, lkey, P);
  double part = 0.0;
  for (int p = tid; p < L; p += T) {
    const unsigned long long key = skey[p];
    const float y = slab[(uint32_t)key];  // < L: pads sort last
    if (NDCG) {
      const double d = disc[p];
      part += (exp2((double)rank_okey_inv(~lkey[p])) - 1.0) * d;
      sgain[p] = exp2((double)y) - 1.0;
      sdisc[p] = d;
    }
    smar[2 * p + 1] = rank_okey_inv(~(uint32_t)(key >> 32));
    sy[p] = y;
  }
  __syncthreads();  // rank-ordered arrays complete, slab dead
  double inv = 1.0;
  if (NDCG) {
    part = wave_sum_f64(part);
    if (lane == 0) sred[wv] = part;
    __syncthreads();
    double idcg = sred[0];
    for (int w = 1; w < nw; ++w) idcg += sred[w];
    if (!(idcg > 0.0)) return;  // block-uniform; zeros stay
    inv = 1.0 / idcg;
  }
  const int kk = min(k, L);
  for (int p = wv; p < kk; p += nw) {  // head rows: wave-uniform
    const float mp = smar[2 * p + 1], yp = sy[p];
    const double gp = NDCG ? sgain[p] : 0.0, dp = NDCG ? sdisc[p] : 0.0;
    double gacc = 0.0, hacc = 0.0;
    for (int q = lane; q < L; q += WAVE)
      topk_pair<NDCG>(mp, yp, gp, dp, smar[2 * q + 1], sy[q],
                      NDCG ? sgain[q] : 0.0, NDCG ? sdisc[q] : 0.0, inv, gacc,
                      hacc);
    gacc = wave_sum_f64(gacc);
    hacc = wave_sum_f64(hacc);
    if (lane == 0)
      out[s0 + sidx[2 * p]] = make_float2((float)gacc, (float)hacc);
  }
  for (int p = kk + tid; p < L; p += T) {  // tail rows
    const float mp = smar[2 * p + 1], yp = sy[p];
    const double gp = NDCG ? sgain[p] : 0.0, dp = NDCG ? sdisc[p] : 0.0;
    double gacc = 0.0, hacc = 0.0;
    for (int q = 0; q < kk; ++q)
      topk_pair<NDCG>(mp, yp, gp, dp, smar[2 * q + 1], sy[q],
                      NDCG ? sgain[q] : 0.0, NDCG ? sdisc[q] : 0.0, inv, gacc,
                      hacc);
    out[s0 + sidx[2 * p]] = make_float2((float)gacc, (float)hacc);
  }
}

// Wave per group (L <= 64), four groups per 256-thread workgroup: sort,
// idcg and the rank-ordered values stay in registers; a partner's values
// come from lane q by __shfl with a wave-uniform q. Lane p walks
// q = 0 .. L-1 ascending and takes the pairs with p < kk or q < kk.
template <bool NDCG>
__global__ __launch_bounds__(RANK_MAX_THREADS)
void lambdarank_topk_wave_kernel(
    const float* __restrict__ margin, const float* __restrict__ label,
    const int64_t* __restrict__ group_ptr, const double* __restrict__ disc,
    float2* __restrict__ out, int G, int64_t n, int k) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int g = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  if (g >= G) return;  // wave-uniform
  const int64_t s0 = group_ptr[g], s1 = group_ptr[g + 1];
  if (!rank_group_ok(s0, s1, n, WAVE)) return;
  const int L = (int)(s1 - s0);
  if (L < 2) return;
  const bool live = lane < L;
  const float m = live ? margin[s0 + lane] : 0.f;
  const float y = live ? label[s0 + lane] : 0.f;
  unsigned long long key = live ? rank_key(m, lane) : ~0ull;
  key = bitonic_wave_sort(key, lane);
  // lane p now holds rank p
  const int idx = (int)(uint32_t)key & (WAVE - 1);
  const float mr = rank_okey_inv(~(uint32_t)(key >> 32));
  const float yr = __shfl(y, idx);
  double gain = 0.0, d = 0.0, inv = 1.0;
  if (NDCG) {
    uint32_t lkey = live ? ~rank_okey(y) : ~0u;
    lkey = bitonic_wave_sort(lkey, lane);
    d = live ? disc[lane] : 0.0;
    gain = exp2((double)yr) - 1.0;
    const double idcg = wave_sum_f64(
        live ? (exp2((double)rank_okey_inv(~lkey)) - 1.0) * d : 0.0);
    if (!(idcg > 0.0)) return;  // wave-uniform
    inv = 1.0 / idcg;
  }
  const int kk = min(k, L);
  double gacc = 0.0, hacc = 0.0;
  for (int q = 0; q < L; ++q) {
    const float mq = __shfl(mr, q), yq = __shfl(yr, q);
    const double gq = NDCG ? __shfl(gain, q) : 0.0;
    const double dq = NDCG ? __shfl(d, q) : 0.0;
    if (live && (lane < kk || q < kk))
      topk_pair<NDCG>(mr, yr, gain, d, mq, yq, gq, dq, inv, gacc, hacc);
  }
  if (live) out[s0 + idx] = make_float2((float)gacc, (float)hacc);
}

static int rank_pad_host(int64_t len) {
  int P = WAVE;
  while (P < len) P <<= 1;
  return P;
}

// Workgroup size: `block` > 0 (benchmark sweeps) if valid, else `dflt`.
static int rank_threads(int64_t block, int dflt) {
  TORCH_CHECK(block <= 0 || (block % WAVE == 0 && block <= RANK_MAX_THREADS),
              "rank ops: block must be a multiple of 64, at most ",
              RANK_MAX_THREADS);
  return block > 0 ? (int)block : dflt;
}

// Default of the workgroup-per-group kernels: two elements per lane, within
// [64, RANK_MAX_THREADS] (measured: docs/parity.md).
static int rank_block_threads(int Pmax, int64_t block) {
  return rank_threads(block,
                      std::min(std::max(Pmax / 2, WAVE), RANK_MAX_THREADS));
}

static void rank_check_inputs(const char* op, const torch::Tensor& margin,
                              const torch::Tensor& label,
                              const torch::Tensor& group_ptr,
                              int64_t max_len) {
  TORCH_CHECK(on_gpu(margin) && label.device() == margin.device() &&
                  group_ptr.device() == margin.device(),
              op, ": tensors must be on one GPU");
  TORCH_CHECK(margin.scalar_type() == torch::kFloat32 &&
                  label.scalar_type() == torch::kFloat32 &&
                  group_ptr.scalar_type() == torch::kInt64,
              op, ": margin/label must be float32, group_ptr int64");
  TORCH_CHECK(margin.dim() == 1 && margin.is_contiguous() &&
                  label.is_contiguous() && group_ptr.is_contiguous() &&
                  label.numel() == margin.numel() && group_ptr.dim() == 1 &&
                  group_ptr.numel() >= 1,
              op, ": margin/label must be contiguous vectors of one length");
  TORCH_CHECK(max_len >= 0 && max_len <= RANK_LDS_MAX_GROUP, op,
              ": longest group ", max_len, " exceeds RANK_LDS_MAX_GROUP = ",
              RANK_LDS_MAX_GROUP);
}

// -> (rank i32 [n], stats f64 [G, 4]). max_len is the longest group of
// group_ptr (a longer group is left untouched, never indexed); variant:
// 0 picks by max_len, 1 forces wave-per-group, 2 workgroup-per-group.
std::vector<torch::Tensor> rank_group_stats(
    torch::Tensor margin, torch::Tensor label, torch::Tensor group_ptr,
    torch::Tensor disc, int64_t k, int64_t max_len, int64_t variant,
    int64_t block) {
  rank_check_inputs("rank_group_stats", margin, label, group_ptr, max_len);
  TORCH_CHECK(disc.device() == margin.device() &&
                  disc.scalar_type() == torch::kFloat64 &&
                  disc.is_contiguous() &&
                  disc.numel() >= rank_pad_host(max_len),
              "rank_group_stats: disc must be a float64 GPU table that "
              "covers the longest group padded to a power of two");
  const int64_t n = margin.numel();
  const int64_t G = group_ptr.numel() - 1;
  auto dev = margin.device();
  auto rank = torch::zeros(
      {n}, torch::TensorOptions().dtype(torch::kInt32).device(dev));
  auto stats = torch::zeros(
      {G, 4}, torch::TensorOptions().dtype(torch::kFloat64).device(dev));
  if (n == 0 || G <= 0) return {rank, stats};
  TORCH_CHECK(variant >= 0 && variant <= 2 &&
                  (variant != 1 || max_len <= WAVE),
              "rank_group_stats: the wave variant serves groups of at most "
              "64 rows");
  auto stream = c10::hip::getCurrentHIPStream();
  const bool wave = variant == 1 || (variant == 0 && max_len <= WAVE);
  if (wave) {
    // four groups per workgroup unless overridden
    const int T = rank_threads(block, RANK_MAX_THREADS);
    hipLaunchKernelGGL(rank_stats_wave_kernel,
                       dim3((uint32_t)ceil_div(G, T / WAVE)), dim3(T), 0,
                       stream.stream(), margin.data_ptr<float>(),
                       label.data_ptr<float>(),
                       group_ptr.data_ptr<int64_t>(), disc.data_ptr<double>(),
                       rank.data_ptr<int32_t>(), stats.data_ptr<double>(),
                       (int)G, n, (int)std::min<int64_t>(k, 1 << 30));
  } else {
    const int Pmax = rank_pad_host(max_len);
    const int T = rank_block_threads(Pmax, block);
    hipLaunchKernelGGL(rank_stats_block_kernel, dim3((uint32_t)G), dim3(T),
                       (size_t)Pmax * 16, stream.stream(),
                       margin.data_ptr<float>(), label.data_ptr<float>(),
                       group_ptr.data_ptr<int64_t>(), disc.data_ptr<double>(),
                       rank.data_ptr<int32_t>(), stats.data_ptr<double>(), n,
                       (int)std::min<int64_t>(k, 1 << 30), Pmax);
  }
  CHECK_HIP(hipGetLastError());
  return {rank, stats};
}

// rank:map gradient pairs f32 [n, 2]; max_len / block as above.
torch::Tensor lambdamap_grad(torch::Tensor margin, torch::Tensor label,
                             torch::Tensor group_ptr, int64_t max_len,
                             int64_t block) {
  rank_check_inputs("lambdamap_grad", margin, label, group_ptr, max_len);
  const int64_t n = margin.numel();
  const int64_t G = group_ptr.numel() - 1;
  auto out = torch::zeros({n, 2},
      torch::TensorOptions().dtype(torch::kFloat32).device(margin.device()));
  if (n == 0 || G <= 0) return out;
  const int Pmax = rank_pad_host(max_len);
  const int T = rank_block_threads(Pmax, block);
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(lambdamap_kernel, dim3((uint32_t)G), dim3(T),
                     (size_t)Pmax * 28, stream.stream(),
                     margin.data_ptr<float>(), label.data_ptr<float>(),
                     group_ptr.data_ptr<int64_t>(),
                     (float2*)out.data_ptr<float>(), n, Pmax);
  CHECK_HIP(hipGetLastError());
  return out;
}

template <bool NDCG>
static void launch_lambdarank_topk(const torch::Tensor& margin,
                                   const torch::Tensor& label,
                                   const torch::Tensor& group_ptr,
                                   const torch::Tensor& disc,
                                   torch::Tensor& out, int k, int64_t max_len,
                                   int64_t block, bool wave) {
  const int64_t n = margin.numel();
  const int64_t G = group_ptr.numel() - 1;
  auto stream = c10::hip::getCurrentHIPStream();
  if (wave) {
    const int T = rank_threads(block, RANK_MAX_THREADS);
    hipLaunchKernelGGL(lambdarank_topk_wave_kernel<NDCG>,
                       dim3((uint32_t)ceil_div(G, T / WAVE)), dim3(T), 0,
                       stream.stream(), margin.data_ptr<float>(),
                       label.data_ptr<float>(),
                       group_ptr.data_ptr<int64_t>(), disc.data_ptr<double>(),
                       (float2*)out.data_ptr<float>(), (int)G, n, k);
  } else {
    const int Pmax = rank_pad_host(max_len);
    const int T = rank_block_threads(Pmax, block);
    hipLaunchKernelGGL(lambdarank_topk_kernel<NDCG>, dim3((uint32_t)G),
                       dim3(T), (size_t)Pmax * (NDCG ? 32 : 16),
                       stream.stream(), margin.data_ptr<float>(),
                       label.data_ptr<float>(),
                       group_ptr.data_ptr<int64_t>(), disc.data_ptr<double>(),
                       (float2*)out.data_ptr<float>(), n, k, Pmax);
  }
  CHECK_HIP(hipGetLastError());
}

// rank:pairwise / rank:ndcg gradient pairs f32 [n, 2] over the pairs with
// min(rank_i, rank_j) < k; max_len / block as above; variant: 1 forces
// wave-per-group (max_len <= 64), 2 workgroup-per-group, 0 picks: the wave
// kernel always walks all L partners, so it wins only from about k = 32 on
// (measured: docs/parity.md) and serves max_len <= 64 with k >= 32.
torch::Tensor lambdarank_topk_grad(torch::Tensor margin, torch::Tensor label,
                                   torch::Tensor group_ptr,
                                   torch::Tensor disc, int64_t k, bool ndcg,
                                   int64_t max_len, int64_t block,
                                   int64_t variant) {
  rank_check_inputs("lambdarank_topk_grad", margin, label, group_ptr,
                    max_len);
  TORCH_CHECK(k >= 1, "lambdarank_topk_grad: k must be at least 1, got ", k);
  TORCH_CHECK(disc.device() == margin.device() &&
                  disc.scalar_type() == torch::kFloat64 &&
                  disc.is_contiguous() &&
                  disc.numel() >= rank_pad_host(max_len),
              "lambdarank_topk_grad: disc must be a float64 GPU table that "
              "covers the longest group padded to a power of two");
  TORCH_CHECK(variant >= 0 && variant <= 2 &&
                  (variant != 1 || max_len <= WAVE),
              "lambdarank_topk_grad: the wave variant serves groups of at "
              "most 64 rows");
  const int64_t n = margin.numel();
  const int64_t G = group_ptr.numel() - 1;
  auto out = torch::zeros({n, 2},
      torch::TensorOptions().dtype(torch::kFloat32).device(margin.device()));
  if (n == 0 || G <= 0) return out;
  const int kk = (int)std::min<int64_t>(k, 1 << 30);
  const bool wave =
      variant == 1 || (variant == 0 && max_len <= WAVE && k >= 32);
  if (ndcg)
    launch_lambdarank_topk<true>(margin, label, group_ptr, disc, out, kk,
                                 max_len, block, wave);
  else
    launch_lambdarank_topk<false>(margin, label, group_ptr, disc, out, kk,
                                  max_len, block, wave);
  return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("lambdarank_topk_grad", &lambdarank_topk_grad,
        "rank:pairwise / rank:ndcg pair gradients, top-k pair truncation",
        py::arg("margin"), py::arg("label"), py::arg("group_ptr"),
        py::arg("disc"), py::arg("k"), py::arg("ndcg"), py::arg("max_len"),
        py::arg("block") = 0, py::arg("variant") = 0);
  m.def("rank_group_stats", &rank_group_stats,
        "per-group stable descending ranks + [dcg@k, idcg@k, idcg, ap]",
        py::arg("margin"), py::arg("label"), py::arg("group_ptr"),
        py::arg("disc"), py::arg("k"), py::arg("max_len"),
        py::arg("variant") = 0, py::arg("block") = 0);
  m.def("lambdamap_grad", &lambdamap_grad, "rank:map pair gradients",
        py::arg("margin"), py::arg("label"), py::arg("group_ptr"),
        py::arg("max_len"), py::arg("block") = 0);
  m.attr("RANK_LDS_MAX_GROUP") = (int)RANK_LDS_MAX_GROUP;
}
