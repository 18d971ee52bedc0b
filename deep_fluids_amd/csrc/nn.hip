// The latent-space integrator (include/deepfluids_hip_nn.h holds the definitions, summation orders included): what stands between the
// three linear layers of the reference's `NN`, the window step of its training graph, the windowed MSE, and the rollout of `test_nn`.
//   bn_fwd_kernel / bn_bwd_kernel   one workgroup per 32 columns of [B,N], 32 row threads per column: the column sums, the element
//                                   pass and the moving averages in one launch; the dropout mask is a hash, recomputed in backward
//   bn_infer_kernel                 elementwise, moving statistics
//   advance_* / rows_copy_kernel    elementwise
//   mse_kernel / mse_final_kernel   one pass + one workgroup
//   rollout_kernel                  one workgroup per scene loops over the frames; activations in LDS, weights from L2
// No atomics; fp32 per thread, fp64 across threads, a fixed combine.
#include "df_common.hpp"

#include "../../include/deepfluids_hip_nn.h"

namespace {

using df::ceil_div;
constexpr int kCols = 32;                   // columns per workgroup of the bn kernels
constexpr int kRowT = 32;                   // row threads per column
constexpr int kBnThreads = kCols * kRowT;   // 1024
constexpr int kThreads = 256;               // elementwise and mse kernels
constexpr int kMsePerThread = 4;
constexpr int kMsePerBlock = kThreads * kMsePerThread;
constexpr int kRoll = 1024;                 // threads of a rollout workgroup (and columns per chunk of its matrix-vector products)
constexpr int64_t kIndexLimit = int64_t(1) << 31;

__host__ __device__ __forceinline__ uint32_t mix(uint32_t h) {
  h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
  return h;
}
__host__ __device__ __forceinline__ uint32_t mask_key(uint32_t seed, uint32_t step, uint32_t window, uint32_t layer) {
  return mix(seed ^ (step * 0x8DA6B343u) ^ (window * 0xD8163841u) ^ (layer * 0xCB1AB31Fu));
}
__device__ __forceinline__ bool kept(uint32_t key, uint32_t row, uint32_t col, float keep_prob) {
  const uint32_t h = mix(key ^ (row * 0x8DA6B343u) ^ (col * 0xD8163841u));
  return static_cast<float>(h >> 8) * 5.9604644775390625e-8f < keep_prob;      // 2^-24
}
// elu of the header: exp(y) - 1 for y <= 0 in plain fp32 steps (no library call), so that the twin repeats it bit for bit
__device__ __forceinline__ float elu(float y) {
  if (y > 0.f) return y;
  if (y < -17.5f) return -1.f;
  const float n = rintf(y * 1.44269502f);
  const float r = (y - n * 0.693359375f) - n * -2.12194440e-4f;
  float q = 2.48015873e-5f;
  q = q * r + 1.98412698e-4f;
  q = q * r + 1.38888889e-3f;
  q = q * r + 8.33333333e-3f;
  q = q * r + 4.16666667e-2f;
  q = q * r + 1.66666667e-1f;
  q = q * r + 0.5f;
  const float p = r + (r * r) * q;
  const float s = ldexpf(1.0f, static_cast<int>(n));
  return s * p + (s - 1.0f);
}
__device__ __forceinline__ float rstd_of(float var, float eps) {
  return static_cast<float>(1.0 / sqrt(static_cast<double>(var) + static_cast<double>(eps)));
}

// S(.) of the header: the 32 row threads' accumulators of a column, fp64, ascending; every thread of the column gets the same total
__device__ __forceinline__ double column_sum(double (*part)[kCols], float acc, int q, int cl) {
  part[q][cl] = static_cast<double>(acc);
  __syncthreads();
  double tot = 0.0;
#pragma unroll 8
  for (int i = 0; i < kRowT; ++i) tot = tot + part[i][cl];
  __syncthreads();
  return tot;
}

struct BnArgs {
  int B, N;
  float eps, decay, keep_prob, inv, bessel, inv_b;
  uint32_t key;
};

__global__ __launch_bounds__(kBnThreads) void bn_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ moving_mean,
                                                            float* __restrict__ moving_var, float* __restrict__ act, float* __restrict__ out,
                                                            float* __restrict__ mean_out, float* __restrict__ rstd_out, BnArgs a) {
  __shared__ double part[kRowT][kCols];
  const int cl = threadIdx.x & (kCols - 1), q = threadIdx.x >> 5;
  const int c = blockIdx.x * kCols + cl;
  const bool valid = c < a.N;
  float s = 0.f;
  if (valid)
    for (int r = q; r < a.B; r += kRowT) s += x[static_cast<int64_t>(r) * a.N + c];
  const float mean = static_cast<float>(column_sum(part, s, q, cl) / static_cast<double>(a.B));
  float v = 0.f;
  if (valid)
    for (int r = q; r < a.B; r += kRowT) {
      const float d = x[static_cast<int64_t>(r) * a.N + c] - mean;
      v += d * d;
    }
  const float var = static_cast<float>(column_sum(part, v, q, cl) / static_cast<double>(a.B));
  if (!valid) return;      // (no barrier follows)
  const float rstd = rstd_of(var, a.eps);
  const float g = gamma[c], bt = beta[c];
  for (int r = q; r < a.B; r += kRowT) {
    const int64_t i = static_cast<int64_t>(r) * a.N + c;
    const float xh = (x[i] - mean) * rstd;
    const float e = elu(xh * g + bt);
    act[i] = e;
    out[i] = kept(a.key, static_cast<uint32_t>(r), static_cast<uint32_t>(c), a.keep_prob) ? e * a.inv : 0.f;
  }
  if (q == 0) {
    mean_out[c] = mean;
    rstd_out[c] = rstd;
    const float omd = 1.0f - a.decay;
    moving_mean[c] = moving_mean[c] * a.decay + mean * omd;
    moving_var[c] = moving_var[c] * a.decay + (var * a.bessel) * omd;
  }
}

__device__ __forceinline__ float bn_dy(const BnArgs& a, float e, float go, int r, int c) {
  const float gd = kept(a.key, static_cast<uint32_t>(r), static_cast<uint32_t>(c), a.keep_prob) ? go * a.inv : 0.f;
  return e < 0.f ? gd * (e + 1.0f) : gd;
}

__global__ __launch_bounds__(kBnThreads) void bn_bwd_kernel(const float* __restrict__ x, const float* __restrict__ act,
                                                            const float* __restrict__ gout, const float* __restrict__ gamma,
                                                            const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                            float* __restrict__ gx, float* __restrict__ ggamma, float* __restrict__ gbeta,
                                                            BnArgs a) {
  __shared__ double part[kRowT][kCols];
  const int cl = threadIdx.x & (kCols - 1), q = threadIdx.x >> 5;
  const int c = blockIdx.x * kCols + cl;
  const bool valid = c < a.N;
  const float mean = valid ? mean_in[c] : 0.f, rstd = valid ? rstd_in[c] : 0.f;
  float s1 = 0.f, s2 = 0.f;
  if (valid)
    for (int r = q; r < a.B; r += kRowT) {
      const int64_t i = static_cast<int64_t>(r) * a.N + c;
      const float dy = bn_dy(a, act[i], gout[i], r, c);
      const float xh = (x[i] - mean) * rstd;
      s1 += dy;
      s2 += dy * xh;
    }
  const float db = static_cast<float>(column_sum(part, s1, q, cl));
  const float dg = static_cast<float>(column_sum(part, s2, q, cl));
  if (!valid) return;
  const float k = gamma[c] * rstd, mb = db * a.inv_b, mg = dg * a.inv_b;
  for (int r = q; r < a.B; r += kRowT) {
    const int64_t i = static_cast<int64_t>(r) * a.N + c;
    const float dy = bn_dy(a, act[i], gout[i], r, c);
    const float xh = (x[i] - mean) * rstd;
    gx[i] = k * ((dy - mb) - xh * mg);
  }
  if (q == 0) {
    gbeta[c] = db;
    ggamma[c] = dg;
  }
}

// grid (column blocks of 256, up to 1024 row strides)
__global__ __launch_bounds__(kThreads) void bn_infer_kernel(const float* x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ mm, const float* __restrict__ mv, float* out, int B, int N,
                                                            float eps) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= N) return;
  const float rstd = rstd_of(mv[c], eps), m = mm[c], g = gamma[c], bt = beta[c];
  for (int r = blockIdx.y; r < B; r += gridDim.y) {
    const int64_t i = static_cast<int64_t>(r) * N + c;
    out[i] = elu(((x[i] - m) * rstd) * g + bt);
  }
}

__global__ __launch_bounds__(kThreads) void advance_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const float* __restrict__ xw, float* __restrict__ xn, int64_t total, int W, int Z,
                                                               int P, int i, float ratio) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= total) return;
  const int K = Z + P;
  const int64_t b = e / K;
  const int j = static_cast<int>(e - b * K);
  xn[e] = j < Z ? x[e] + y[b * Z + j] * ratio : xw[(b * W + i + 1) * K + j];
}

__global__ __launch_bounds__(kThreads) void advance_bwd_kernel(const float* __restrict__ gxn, float* __restrict__ gx, float* __restrict__ gy,
                                                               int64_t total, int Z, int P, float ratio) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= total) return;
  const int K = Z + P;
  const int64_t b = e / K;
  const int j = static_cast<int>(e - b * K);
  const float g = gxn[e];
  if (gx) gx[e] = j < Z ? g : 0.f;
  if (gy && j < Z) gy[b * Z + j] = g * ratio;
}

__global__ __launch_bounds__(kThreads) void rows_copy_kernel(const float* __restrict__ src, int64_t ss, float* __restrict__ dst, int64_t ds,
                                                             int64_t total, int Z) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= total) return;
  const int64_t b = e / Z;
  const int j = static_cast<int>(e - b * Z);
  dst[b * ds + j] = src[b * ss + j];
}

// the tree of the header (as metrics.hip); the result is valid in thread 0
__device__ __forceinline__ double block_tree(double a) {
  __shared__ double wave[kThreads / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a = a + __shfl_down(a, off, 64);
  if ((threadIdx.x & 63) == 0) wave[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kThreads / 64; ++w) a = a + wave[w];
  return a;
}

__global__ __launch_bounds__(kThreads) void mse_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                       double* __restrict__ partial) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kMsePerThread; ++i) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kMsePerBlock + i * kThreads + threadIdx.x;
    if (e < n) {
      const float d = a[e] - b[e];
      s += d * d;
    }
  }
  const double t = block_tree(static_cast<double>(s));
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ __launch_bounds__(kThreads) void mse_final_kernel(const double* __restrict__ partial, int64_t nblk, int64_t n, float* __restrict__ out) {
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < nblk; i += kThreads) s = s + partial[i];
  const double t = block_tree(s);
  if (threadIdx.x == 0) out[0] = static_cast<float>(t / static_cast<double>(n));
}

__global__ __launch_bounds__(kThreads) void mse_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ gout,
                                                           float* __restrict__ ga, int64_t n, float two_over_n) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= n) return;
  ga[e] = (gout[0] * two_over_n) * (a[e] - b[e]);
}

// ---- rollout ---------------------------------------------------------------------------------------------------------------------------
struct Layer {
  const float *w, *b, *gamma, *beta, *mm;      // gamma == nullptr: the last layer (no bn, no elu)
};
struct Roll {
  const float *x_test, *y_test, *mv1, *mv2;
  Layer l1, l2, l3;
  float* z_out;
  int F, Z, P, N1, N2;
  float eps, code_std, out_std;
};

// dst[n] = epilogue(v . w[:,n] + b[n]) for all N columns; v, dst, rs and part are LDS; every thread of the workgroup calls it
__device__ __forceinline__ void matvec(const float* v, int K, const Layer& l, const float* rs, int N, float* part, float* dst) {
  const int t = threadIdx.x;
  for (int n0 = 0; n0 < N; n0 += kRoll) {
    const int nb = N - n0 < kRoll ? N - n0 : kRoll;
    const int sk = kRoll / nb;
    const int q = t / nb, cl = t - q * nb;
    if (q < sk) {
      float acc = 0.f;
      const float* wc = l.w + n0 + cl;
      for (int k = q; k < K; k += sk) acc += v[k] * wc[static_cast<int64_t>(k) * N];
      part[t] = acc;
    }
    __syncthreads();
    if (t < nb) {
      double tot = 0.0;
      for (int i = 0; i < sk; ++i) tot = tot + static_cast<double>(part[i * nb + t]);
      const int n = n0 + t;
      float y = static_cast<float>(tot) + l.b[n];
      if (l.gamma) y = elu(((y - l.mm[n]) * rs[n]) * l.gamma[n] + l.beta[n]);
      dst[n] = y;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kRoll) void rollout_kernel(Roll a) {
  extern __shared__ float lds[];
  const int K0 = a.Z + a.P, t = threadIdx.x;
  float* xin = lds;                  // [K0]
  float* h1 = xin + K0;              // [N1]
  float* h2 = h1 + a.N1;             // [N2]
  float* yv = h2 + a.N2;             // [Z]
  float* rs1 = yv + a.Z;             // [N1]
  float* rs2 = rs1 + a.N1;           // [N2]
  float* part = rs2 + a.N2;          // [kRoll]
  const int64_t s = blockIdx.x;
  const int64_t row0 = s * (a.F - 1);
  for (int n = t; n < a.N1; n += kRoll) rs1[n] = rstd_of(a.mv1[n], a.eps);
  for (int n = t; n < a.N2; n += kRoll) rs2[n] = rstd_of(a.mv2[n], a.eps);
  for (int j = t; j < K0; j += kRoll) xin[j] = a.x_test[row0 * K0 + j];
  __syncthreads();
  float* zo = a.z_out + s * a.F * a.Z;
  for (int j = t; j < a.Z; j += kRoll) zo[j] = xin[j] * a.code_std;
  for (int f = 0; f < a.F - 1; ++f) {
    matvec(xin, K0, a.l1, rs1, a.N1, part, h1);
    matvec(h1, a.N1, a.l2, rs2, a.N2, part, h2);
    matvec(h2, a.N2, a.l3, nullptr, a.Z, part, yv);
    const int64_t r = row0 + f;
    // (Z may exceed the workgroup: a thread's entries j = t, t + 1024, ... are its own in both phases, so one barrier between reading
    //  and overwriting xin is enough for the OTHER threads' reads in the next matvec)
    for (int j = t; j < a.Z; j += kRoll) {
      float pred = yv[j] * a.out_std + xin[j] * a.code_std;
      if (j >= a.Z - a.P) pred = a.y_test[r * a.Z + j] * a.out_std + a.x_test[r * K0 + j] * a.code_std;
      zo[static_cast<int64_t>(f + 1) * a.Z + j] = pred;
      xin[j] = pred / a.code_std;
    }
    if (f < a.F - 2)
      for (int j = t; j < a.P; j += kRoll) xin[a.Z + j] = a.x_test[(r + 1) * K0 + a.Z + j];
    __syncthreads();
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
inline bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
inline bool aligned4(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (!aligned(p, 4)) return false;
  return true;
}
inline unsigned blocks_of(int64_t n) { return static_cast<unsigned>(ceil_div(n, kThreads)); }

int bn_extents(const char* fn, int64_t B, int64_t N) {
  DF_REQUIRE(B > 0 && N > 0, DF_EINVAL, "%s: non-positive extent (B %lld, N %lld)", fn, (long long)B, (long long)N);
  DF_REQUIRE(B < kIndexLimit && N < kIndexLimit && B * N < kIndexLimit, DF_ESHAPE, "%s: %lld x %lld elements do not fit the int32 row and column index",
             fn, (long long)B, (long long)N);
  return DF_OK;
}

int mask_args(const char* fn, float keep_prob) {
  DF_REQUIRE(keep_prob > 0.f && keep_prob <= 1.f, DF_EINVAL, "%s: keep_prob must be in (0, 1], got %g", fn, (double)keep_prob);
  return DF_OK;
}

}  // namespace

extern "C" {

int df_nn_bn_elu_dropout_fwd(const float* x, const float* gamma, const float* beta, float* moving_mean, float* moving_var, float* act,
                             float* out, float* mean, float* rstd, int64_t B, int64_t N, float eps, float decay, float keep_prob,
                             uint32_t seed, uint32_t step, uint32_t window, uint32_t layer, df_stream_t stream) {
  const char* fn = "df_nn_bn_elu_dropout_fwd";
  DF_REQUIRE(x && gamma && beta && moving_mean && moving_var && act && out && mean && rstd, DF_EINVAL, "%s: null pointer", fn);
  if (int e = bn_extents(fn, B, N)) return e;
  if (int e = mask_args(fn, keep_prob)) return e;
  DF_REQUIRE(eps > 0.f, DF_EINVAL, "%s: eps must be positive, got %g", fn, (double)eps);
  DF_REQUIRE(decay >= 0.f && decay <= 1.f, DF_EINVAL, "%s: decay must be in [0, 1], got %g", fn, (double)decay);
  DF_REQUIRE(aligned4({x, gamma, beta, moving_mean, moving_var, act, out, mean, rstd}), DF_EALIGN, "%s: every buffer must be 4-byte aligned", fn);
  BnArgs a{(int)B, (int)N, eps, decay, keep_prob, 1.0f / keep_prob, static_cast<float>(B) / static_cast<float>(B > 1 ? B - 1 : 1),
           1.0f / static_cast<float>(B), mask_key(seed, step, window, layer)};
  hipLaunchKernelGGL(bn_fwd_kernel, dim3((unsigned)ceil_div(N, kCols)), dim3(kBnThreads), 0, df::as_stream(stream), x, gamma, beta,
                     moving_mean, moving_var, act, out, mean, rstd, a);
  return df::launched(fn);
}

int df_nn_bn_elu_dropout_bwd(const float* x, const float* act, const float* gout, const float* gamma, const float* mean,
                             const float* rstd, float* gx, float* ggamma, float* gbeta, int64_t B, int64_t N, float keep_prob,
                             uint32_t seed, uint32_t step, uint32_t window, uint32_t layer, df_stream_t stream) {
  const char* fn = "df_nn_bn_elu_dropout_bwd";
  DF_REQUIRE(x && act && gout && gamma && mean && rstd && gx && ggamma && gbeta, DF_EINVAL, "%s: null pointer", fn);
  if (int e = bn_extents(fn, B, N)) return e;
  if (int e = mask_args(fn, keep_prob)) return e;
  DF_REQUIRE(aligned4({x, act, gout, gamma, mean, rstd, gx, ggamma, gbeta}), DF_EALIGN, "%s: every buffer must be 4-byte aligned", fn);
  BnArgs a{(int)B, (int)N, 0.f, 0.f, keep_prob, 1.0f / keep_prob, 0.f, 1.0f / static_cast<float>(B), mask_key(seed, step, window, layer)};
  hipLaunchKernelGGL(bn_bwd_kernel, dim3((unsigned)ceil_div(N, kCols)), dim3(kBnThreads), 0, df::as_stream(stream), x, act, gout, gamma,
                     mean, rstd, gx, ggamma, gbeta, a);
  return df::launched(fn);
}

int df_nn_bn_elu_infer(const float* x, const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                       float* out, int64_t B, int64_t N, float eps, df_stream_t stream) {
  const char* fn = "df_nn_bn_elu_infer";
  DF_REQUIRE(x && gamma && beta && moving_mean && moving_var && out, DF_EINVAL, "%s: null pointer", fn);
  if (int e = bn_extents(fn, B, N)) return e;
  DF_REQUIRE(eps > 0.f, DF_EINVAL, "%s: eps must be positive, got %g", fn, (double)eps);
  DF_REQUIRE(aligned4({x, gamma, beta, moving_mean, moving_var, out}), DF_EALIGN, "%s: every buffer must be 4-byte aligned", fn);
  hipLaunchKernelGGL(bn_infer_kernel, dim3((unsigned)ceil_div(N, kThreads), (unsigned)(B < 1024 ? B : 1024)), dim3(kThreads), 0,
                     df::as_stream(stream), x, gamma, beta, moving_mean, moving_var, out, (int)B, (int)N, eps);
  return df::launched(fn);
}

int df_nn_window_advance_fwd(const float* x, const float* y, const float* xw, float* x_next, int64_t B, int64_t W, int64_t Z, int64_t P,
                             int64_t i, float ratio, df_stream_t stream) {
  const char* fn = "df_nn_window_advance_fwd";
  DF_REQUIRE(x && y && xw && x_next, DF_EINVAL, "%s: null pointer", fn);
  DF_REQUIRE(B > 0 && W > 0 && Z > 0 && P > 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(i >= 0 && i < W - 1, DF_EINVAL, "%s: window entry %lld has no successor among %lld", fn, (long long)i, (long long)W);
  DF_REQUIRE(P <= Z, DF_ESHAPE, "%s: %lld parameters in a code of %lld", fn, (long long)P, (long long)Z);
  DF_REQUIRE(B < kIndexLimit && W < kIndexLimit && Z < kIndexLimit && B * W < kIndexLimit && B * W * (Z + P) < kIndexLimit, DF_ESHAPE,
             "%s: %lld x %lld x %lld elements are more than one launch holds", fn, (long long)B, (long long)W, (long long)(Z + P));
  DF_REQUIRE(aligned4({x, y, xw, x_next}), DF_EALIGN, "%s: every buffer must be 4-byte aligned", fn);
  const int64_t total = B * (Z + P);
  hipLaunchKernelGGL(advance_fwd_kernel, dim3(blocks_of(total)), dim3(kThreads), 0, df::as_stream(stream), x, y, xw, x_next, total, (int)W,
                     (int)Z, (int)P, (int)i, ratio);
  return df::launched(fn);
}

int df_nn_window_advance_bwd(const float* gx_next, float* gx, float* gy, int64_t B, int64_t Z, int64_t P, float ratio, df_stream_t stream) {
  const char* fn = "df_nn_window_advance_bwd";
  DF_REQUIRE(gx_next, DF_EINVAL, "%s: null pointer", fn);
  DF_REQUIRE(B > 0 && Z > 0 && P > 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(P <= Z, DF_ESHAPE, "%s: %lld parameters in a code of %lld", fn, (long long)P, (long long)Z);
  DF_REQUIRE(B < kIndexLimit && Z < kIndexLimit && B * (Z + P) < kIndexLimit, DF_ESHAPE, "%s: %lld x %lld elements are more than one launch holds", fn,
             (long long)B, (long long)(Z + P));
  DF_REQUIRE(aligned4({gx_next, gx, gy}), DF_EALIGN, "%s: every buffer must be 4-byte aligned", fn);
  if (!gx && !gy) return DF_OK;
  const int64_t total = B * (Z + P);
  hipLaunchKernelGGL(advance_bwd_kernel, dim3(blocks_of(total)), dim3(kThreads), 0, df::as_stream(stream), gx_next, gx, gy, total, (int)Z, (int)P,
                     ratio);
  return df::launched(fn);
}

int df_nn_rows_copy(const float* src, int64_t src_stride, float* dst, int64_t dst_stride, int64_t B, int64_t Z, df_stream_t stream) {
  const char* fn = "df_nn_rows_copy";
  DF_REQUIRE(src && dst, DF_EINVAL, "%s: null pointer", fn);
  DF_REQUIRE(B > 0 && Z > 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(src_stride >= Z && dst_stride >= Z, DF_ESHAPE, "%s: a row stride (%lld, %lld) below the row length %lld", fn, (long long)src_stride,
             (long long)dst_stride, (long long)Z);
  DF_REQUIRE(B < kIndexLimit && Z < kIndexLimit && src_stride < kIndexLimit && dst_stride < kIndexLimit && B * src_stride < kIndexLimit &&
                 B * dst_stride < kIndexLimit,
             DF_ESHAPE, "%s: %lld rows of stride %lld / %lld are more than one launch holds", fn, (long long)B, (long long)src_stride,
             (long long)dst_stride);
  DF_REQUIRE(aligned4({src, dst}), DF_EALIGN, "%s: every buffer must be 4-byte aligned", fn);
  const int64_t total = B * Z;
  hipLaunchKernelGGL(rows_copy_kernel, dim3(blocks_of(total)), dim3(kThreads), 0, df::as_stream(stream), src, src_stride, dst, dst_stride, total,
                     (int)Z);
  return df::launched(fn);
}

int64_t df_nn_mse_workspace_bytes(int64_t n) {
  if (n <= 0 || n >= kIndexLimit * kMsePerBlock) return -1;
  return ceil_div(n, kMsePerBlock) * static_cast<int64_t>(sizeof(double));
}

int df_nn_mse_fwd(const float* a, const float* b, int64_t n, float* out, void* ws, int64_t ws_bytes, df_stream_t stream) {
  const char* fn = "df_nn_mse_fwd";
  DF_REQUIRE(a && b && out && ws, DF_EINVAL, "%s: null pointer", fn);
  DF_REQUIRE(n > 0, DF_EINVAL, "%s: non-positive element count %lld", fn, (long long)n);
  const int64_t need = df_nn_mse_workspace_bytes(n);
  DF_REQUIRE(need > 0, DF_ESHAPE, "%s: %lld elements are more than one launch holds", fn, (long long)n);
  DF_REQUIRE(aligned4({a, b, out}), DF_EALIGN, "%s: a, b and out must be 4-byte aligned", fn);
  DF_REQUIRE(aligned(ws, 8), DF_EALIGN, "%s: the workspace must be 8-byte aligned", fn);
  DF_REQUIRE(ws_bytes >= need, DF_EWORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn, (long long)ws_bytes, (long long)need);
  const int64_t nblk = need / 8;
  hipStream_t s = df::as_stream(stream);
  hipLaunchKernelGGL(mse_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, s, a, b, n, static_cast<double*>(ws));
  if (int e = df::launched(fn)) return e;
  hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(kThreads), 0, s, static_cast<const double*>(ws), nblk, n, out);
  return df::launched(fn);
}

int df_nn_mse_bwd(const float* a, const float* b, const float* gout, float* ga, int64_t n, df_stream_t stream) {
  const char* fn = "df_nn_mse_bwd";
  DF_REQUIRE(a && b && gout && ga, DF_EINVAL, "%s: null pointer", fn);
  DF_REQUIRE(n > 0, DF_EINVAL, "%s: non-positive element count %lld", fn, (long long)n);
  DF_REQUIRE(n < kIndexLimit * kThreads, DF_ESHAPE, "%s: %lld elements are more than one launch holds", fn, (long long)n);
  DF_REQUIRE(aligned4({a, b, gout, ga}), DF_EALIGN, "%s: every buffer must be 4-byte aligned", fn);
  hipLaunchKernelGGL(mse_bwd_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, df::as_stream(stream), a, b, gout, ga, n, 2.0f / static_cast<float>(n));
  return df::launched(fn);
}

int df_nn_rollout(const float* x_test, const float* y_test, const float* w1, const float* b1, const float* gamma1, const float* beta1,
                  const float* mm1, const float* mv1, const float* w2, const float* b2, const float* gamma2, const float* beta2,
                  const float* mm2, const float* mv2, const float* w3, const float* b3, float* z_out, int64_t S, int64_t F, int64_t Z,
                  int64_t P, int64_t N1, int64_t N2, float eps, float code_std, float out_std, df_stream_t stream) {
  const char* fn = "df_nn_rollout";
  DF_REQUIRE(x_test && y_test && w1 && b1 && gamma1 && beta1 && mm1 && mv1 && w2 && b2 && gamma2 && beta2 && mm2 && mv2 && w3 && b3 && z_out,
             DF_EINVAL, "%s: null pointer", fn);
  DF_REQUIRE(S > 0 && F > 0 && Z > 0 && P > 0 && N1 > 0 && N2 > 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(eps > 0.f && code_std > 0.f, DF_EINVAL, "%s: eps and code_std must be positive (got %g, %g)", fn, (double)eps, (double)code_std);
  DF_REQUIRE(F >= 2, DF_ESHAPE, "%s: a scene of %lld frame has no step", fn, (long long)F);
  DF_REQUIRE(P <= Z, DF_ESHAPE, "%s: %lld parameters in a code of %lld", fn, (long long)P, (long long)Z);
  const int64_t kLds = 64 * 1024;
  DF_REQUIRE(Z < kLds && N1 < kLds && N2 < kLds, DF_ESHAPE, "%s: the activations (%lld, %lld, %lld) do not fit the LDS", fn, (long long)Z,
             (long long)N1, (long long)N2);
  const int64_t lds = 4 * (Z + P + 2 * N1 + 2 * N2 + Z + kRoll);
  DF_REQUIRE(lds <= kLds, DF_ESHAPE, "%s: the activations need %lld bytes of LDS, 65536 at most", fn, (long long)lds);
  DF_REQUIRE(S < kIndexLimit && F < kIndexLimit && S * F < kIndexLimit && S * F * (Z + P) < kIndexLimit, DF_ESHAPE,
             "%s: %lld scenes of %lld frames are more than one launch holds", fn, (long long)S, (long long)F);
  DF_REQUIRE(aligned4({x_test, y_test, w1, b1, gamma1, beta1, mm1, mv1, w2, b2, gamma2, beta2, mm2, mv2, w3, b3, z_out}), DF_EALIGN,
             "%s: every buffer must be 4-byte aligned", fn);
  Roll a{x_test, y_test, mv1, mv2, Layer{w1, b1, gamma1, beta1, mm1}, Layer{w2, b2, gamma2, beta2, mm2}, Layer{w3, b3, nullptr, nullptr, nullptr},
         z_out, (int)F, (int)Z, (int)P, (int)N1, (int)N2, eps, code_std, out_std};
  hipLaunchKernelGGL(rollout_kernel, dim3((unsigned)S), dim3(kRoll), (size_t)lds, df::as_stream(stream), a);
  return df::launched(fn);
}

}  // extern "C"
