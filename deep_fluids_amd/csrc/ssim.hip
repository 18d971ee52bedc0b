// Structural similarity of two image batches (include/deepfluids_hip_ssim.h holds the definition, tap, operation and summation order
// included): the reference's ssim / one level of its ms_ssim as ONE pass.  HBM-bound: a workgroup owns one 32x32 output tile of one
// image, loads tile + (S-1) halo of both images once as 2x2 pixel quads (the halo of a neighbour tile is an L2 hit), writes the pooled
// quads it owns for the next MS-SSIM level from those registers, keeps the five channel-summed planes in LDS, filters them rows first
// into a second LDS buffer and columns second into registers, and reduces the two values of its pixels.
//   ssim_kernel<C>          one workgroup per tile of ONE image -> maps, pooled images, one (ssim, cs) tile sum
//   ssim_final_kernel       one workgroup per image: its tile sums in a fixed order -> the 8 output words
//   ssim_group_mean_kernel  one workgroup per group of images: their totals in a fixed order -> two fp64 means
// No atomics; fp32 per thread (<= 4 pixels), fp64 across threads and workgroups.
// LDS pitches: the row pass has lane (xq, r) read tile[r][4 xq + k] -- with a pitch of 43 (11 mod 32) four consecutive rows fall on
// banks 0, 11, 22, 1 (distinct mod 4) and the eight xq on multiples of 4: conflict-free -- and write hbuf[r][4 xq + i], conflict-free at a
// pitch of 33; the column pass reads hbuf[r][x] with x on the lane.
#include "df_common.hpp"

#include <cmath>

#include "../../include/deepfluids_hip_ssim.h"

namespace {

using df::ceil_div;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = DF_SSIM_TILE;                      // 32 x 32 output pixels
constexpr int kMaxSize = DF_SSIM_MAX_SIZE;               // 11 taps
constexpr int kStage = kTile + kMaxSize - 1;             // 42 staged rows and columns
constexpr int kPitch = 43, kHPitch = 33;
constexpr int kPlanes = 5;
constexpr int kPerThread = 4;                            // output rows of a thread (and output columns of a row-pass item)
static_assert(kStage % 2 == 0, "a staged tile is whole 2x2 quads");
static_assert(kThreads == kTile * kTile / kPerThread, "one thread per column and four rows");

struct Args {
  const float* a;
  const float* b;
  float* smap;
  float* cmap;
  float* pa;
  float* pb;
  double* partial;      // [N, tiles, 2]
  int H, W, S, OH, OW, nty, ntx, PH, PW;
  float lo, range, inv_c2, c1, c2;
  float taps[kMaxSize];
};

template <int C>
struct Rec {
  float v[C];
};
template <int C>
__device__ __forceinline__ Rec<C> ld(const float* __restrict__ p) {
  return *reinterpret_cast<const Rec<C>*>(p);
}

// the tree of step 2 of the header, for the pair (ssim, cs); the result is valid in thread 0
__device__ __forceinline__ void block_reduce(double& s, double& c) {
  __shared__ double part[kWaves][2];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s = s + __shfl_down(s, off, 64);      // lanes >= off combine with values the tree no longer reads
    c = c + __shfl_down(c, off, 64);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { part[wid][0] = s; part[wid][1] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) { s = s + part[w][0]; c = c + part[w][1]; }
  }
}

template <int C>
__global__ __launch_bounds__(kThreads) void ssim_kernel(Args g) {
  __shared__ float tile[kPlanes][kStage][kPitch];
  __shared__ float hbuf[kPlanes][kStage][kHPitch];
  __shared__ float tp[16];
  const int tid = threadIdx.x;
  const int tiles = g.nty * g.ntx;
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const int ty = t / g.ntx, tx = t - ty * g.ntx;
  const int y0 = ty * kTile, x0 = tx * kTile;
  const int S = g.S, TS = kTile + S - 1, NQ = (TS + 1) >> 1;      // staged extent, in pixels and in quads (<= 21)
  const int64_t img = static_cast<int64_t>(n) * g.H * g.W * C;
  const float* ia = g.a + img;
  const float* ib = g.b + img;
  if (tid < S) tp[tid] = g.taps[tid];

  // ---- stage: 2x2 quads of both images -> the five planes (0 outside the image), and the pooled quads this tile owns
  const bool last_y = ty == g.nty - 1, last_x = tx == g.ntx - 1;
  for (int item = tid; item < NQ * NQ; item += kThreads) {
    const int qy = item / NQ, qx = item - qy * NQ;
    Rec<C> ra[2][2], rb[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int r = 2 * qy + dy, c = 2 * qx + dx, gy = y0 + r, gx = x0 + c;
        const bool in = gy < g.H && gx < g.W;
        float P[kPlanes] = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (in) {
          const int at = (gy * g.W + gx) * C;
          ra[dy][dx] = ld<C>(ia + at);
          rb[dy][dx] = ld<C>(ib + at);
#pragma unroll
          for (int k = 0; k < C; ++k) {
            const float p = (ra[dy][dx].v[k] - g.lo) / g.range, q = (rb[dy][dx].v[k] - g.lo) / g.range;
            const float pp = p * p, qq = q * q, pq = p * q;
            if (k == 0) { P[0] = p; P[1] = q; P[2] = pp; P[3] = qq; P[4] = pq; }
            else { P[0] = P[0] + p; P[1] = P[1] + q; P[2] = P[2] + pp; P[3] = P[3] + qq; P[4] = P[4] + pq; }
          }
        } else {
#pragma unroll
          for (int k = 0; k < C; ++k) { ra[dy][dx].v[k] = 0.f; rb[dy][dx].v[k] = 0.f; }
        }
#pragma unroll
        for (int k = 0; k < kPlanes; ++k) tile[k][r][c] = P[k];      // r, c <= 2 * 20 + 1 = 41
      }
    }
    const int gy = y0 + 2 * qy, gx = x0 + 2 * qx;
    if (g.pa && (qy < kTile / 2 || last_y) && (qx < kTile / 2 || last_x) && gy < g.H && gx < g.W) {
      const bool two_x = gx + 1 < g.W, two_y = gy + 1 < g.H;
      const float w = two_x ? (two_y ? 0.25f : 0.5f) : (two_y ? 0.5f : 1.f);
      Rec<C> oa, ob;
#pragma unroll
      for (int k = 0; k < C; ++k) {
        float sa = ra[0][0].v[k], sb = rb[0][0].v[k];
        if (two_x) { sa = sa + ra[0][1].v[k]; sb = sb + rb[0][1].v[k]; }
        if (two_y) {
          sa = sa + ra[1][0].v[k]; sb = sb + rb[1][0].v[k];
          if (two_x) { sa = sa + ra[1][1].v[k]; sb = sb + rb[1][1].v[k]; }
        }
        oa.v[k] = sa * w; ob.v[k] = sb * w;
      }
      const int64_t at = ((static_cast<int64_t>(n) * g.PH + (gy >> 1)) * g.PW + (gx >> 1)) * C;      // gy/2 < PH, gx/2 < PW
      *reinterpret_cast<Rec<C>*>(g.pa + at) = oa;
      *reinterpret_cast<Rec<C>*>(g.pb + at) = ob;
    }
  }
  __syncthreads();

  // ---- rows: an item is four neighbouring outputs of one row of one plane, its S + 3 inputs read once
  for (int item = tid; item < kPlanes * TS * (kTile / kPerThread); item += kThreads) {
    const int xq = item & (kTile / kPerThread - 1), rr = item >> 3;
    const int pl = rr / TS, r = rr - pl * TS;
    const float* row = &tile[pl][r][kPerThread * xq];      // reads up to column 28 + S + 2 = TS - 1
    float acc[kPerThread] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < S + kPerThread - 1; ++k) {
      const float v = row[k];
#pragma unroll
      for (int i = 0; i < kPerThread; ++i) {
        const int j = k - i;
        if (j >= 0 && j < S) acc[i] = acc[i] + tp[j] * v;
      }
    }
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) hbuf[pl][r][kPerThread * xq + i] = acc[i];
  }
  __syncthreads();

  // ---- columns: a thread's four outputs of every plane, its S + 3 row results read once
  const int x = tid & (kTile - 1), yq = tid >> 5;
  float F[kPlanes][kPerThread];
#pragma unroll
  for (int k = 0; k < kPlanes; ++k)
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) F[k][i] = 0.f;
  for (int k = 0; k < S + kPerThread - 1; ++k) {
    const int r = kPerThread * yq + k;                       // <= 28 + S + 2 = TS - 1
    float h[kPlanes];
#pragma unroll
    for (int p = 0; p < kPlanes; ++p) h[p] = hbuf[p][r][x];
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const int j = k - i;
      if (j >= 0 && j < S) {
        const float w = tp[j];
#pragma unroll
        for (int p = 0; p < kPlanes; ++p) F[p][i] = F[p][i] + w * h[p];
      }
    }
  }

  const int oh = min(kTile, g.OH - y0), ow = min(kTile, g.OW - x0);
  float ssum = 0.f, csum = 0.f;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int y = kPerThread * yq + i;
    if (y < oh && x < ow) {
      const float mu1 = F[0][i] * g.inv_c2, mu2 = F[1][i] * g.inv_c2;
      const float e11 = F[2][i] * g.inv_c2, e22 = F[3][i] * g.inv_c2, e12 = F[4][i] * g.inv_c2;
      const float mu11 = mu1 * mu1, mu22 = mu2 * mu2, mu12 = mu1 * mu2;
      const float s11 = e11 - mu11, s22 = e22 - mu22, s12 = e12 - mu12;
      const float v1 = 2.f * s12 + g.c2, v2 = (s11 + s22) + g.c2;
      const float val = ((2.f * mu12 + g.c1) * v1) / (((mu11 + mu22) + g.c1) * v2);
      const float cs = v1 / v2;
      ssum += val; csum += cs;
      if (g.smap) {
        const int64_t at = (static_cast<int64_t>(n) * g.OH + (y0 + y)) * g.OW + (x0 + x);
        g.smap[at] = val; g.cmap[at] = cs;
      }
    }
  }
  double ds = static_cast<double>(ssum), dc = static_cast<double>(csum);
  block_reduce(ds, dc);
  if (tid == 0) {
    g.partial[2 * static_cast<int64_t>(blockIdx.x)] = ds;
    g.partial[2 * static_cast<int64_t>(blockIdx.x) + 1] = dc;
  }
}

__global__ __launch_bounds__(kThreads) void ssim_final_kernel(const double* __restrict__ partial, int tiles, int count, int32_t* __restrict__ out) {
  const double* pe = partial + 2 * static_cast<int64_t>(blockIdx.x) * tiles;
  double s = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < tiles; i += kThreads) { s = s + pe[2 * i]; c = c + pe[2 * i + 1]; }
  block_reduce(s, c);
  if (threadIdx.x == 0) {
    int32_t* o = out + static_cast<int64_t>(blockIdx.x) * DF_SSIM_WORDS;
    o[DF_SSIM_COUNT] = count;
    reinterpret_cast<float*>(o)[DF_SSIM_MEAN] = static_cast<float>(s / static_cast<double>(count));
    reinterpret_cast<float*>(o)[DF_SSIM_MEAN_CS] = static_cast<float>(c / static_cast<double>(count));
    o[3] = 0;
    *reinterpret_cast<double*>(o + DF_SSIM_SUM) = s;
    *reinterpret_cast<double*>(o + DF_SSIM_SUM_CS) = c;
  }
}

__global__ __launch_bounds__(kThreads) void ssim_group_mean_kernel(const int32_t* __restrict__ out, int M, double* __restrict__ mean) {
  const int32_t* rows = out + static_cast<int64_t>(blockIdx.x) * M * DF_SSIM_WORDS;
  double s = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < M; i += kThreads) {
    const int32_t* o = rows + static_cast<int64_t>(i) * DF_SSIM_WORDS;
    s = s + *reinterpret_cast<const double*>(o + DF_SSIM_SUM);
    c = c + *reinterpret_cast<const double*>(o + DF_SSIM_SUM_CS);
  }
  block_reduce(s, c);
  if (threadIdx.x == 0) {
    const double cells = static_cast<double>(M) * static_cast<double>(rows[DF_SSIM_COUNT]);
    mean[2 * static_cast<int64_t>(blockIdx.x)] = s / cells;
    mean[2 * static_cast<int64_t>(blockIdx.x) + 1] = c / cells;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
constexpr int64_t kIndexLimit = int64_t(1) << 31;

struct Geo {
  int S, OH, OW, nty, ntx, PH, PW;
  int64_t tiles;
};

// the derived extents, or a DF_E* code; fn == nullptr: no message (the size query)
int geometry(const char* fn, int64_t N, int64_t H, int64_t W, int filter_size, Geo* geo) {
  if (!(N > 0 && H > 0 && W > 0)) return fn ? df::fail(DF_EINVAL, "%s: non-positive extent", fn) : DF_EINVAL;
  if (filter_size < 1) return fn ? df::fail(DF_EINVAL, "%s: filter_size must be >= 1, got %d", fn, filter_size) : DF_EINVAL;
  const int64_t S = filter_size < H ? (filter_size < W ? filter_size : W) : (H < W ? H : W);
  if (S > kMaxSize) return fn ? df::fail(DF_ESHAPE, "%s: a window of %lld taps; the staged tile holds at most %d", fn, (long long)S, kMaxSize) : DF_ESHAPE;
  // (each factor is below 2^31 once the product of the earlier ones is: no overflow)
  const bool big = H >= kIndexLimit || W >= kIndexLimit || H * W >= kIndexLimit || H * W * DF_SSIM_MAX_CHANNELS >= kIndexLimit;
  if (big) return fn ? df::fail(DF_ESHAPE, "%s: %lld x %lld pixels per image do not fit the int32 index", fn, (long long)H, (long long)W) : DF_ESHAPE;
  const int64_t OH = H - S + 1, OW = W - S + 1, nty = ceil_div(OH, kTile), ntx = ceil_div(OW, kTile), tiles = nty * ntx;
  if (N >= kIndexLimit || N * tiles >= kIndexLimit) return fn ? df::fail(DF_ESHAPE, "%s: %lld images of %lld workgroups are more than one launch holds", fn, (long long)N, (long long)tiles) : DF_ESHAPE;
  *geo = Geo{(int)S, (int)OH, (int)OW, (int)nty, (int)ntx, (int)((H + 1) / 2), (int)((W + 1) / 2), tiles};
  return DF_OK;
}

inline bool apart(const void* p, int64_t np, const void* q, int64_t nq) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a + static_cast<uintptr_t>(np) <= b || b + static_cast<uintptr_t>(nq) <= a;
}
inline bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

struct Buf {
  const void* p;
  int64_t bytes;
  const char* name;
  bool written;
};

template <int C>
void launch(const Args& args, unsigned blocks, hipStream_t s) {
  hipLaunchKernelGGL((ssim_kernel<C>), dim3(blocks), dim3(kThreads), 0, s, args);
}

}  // namespace

extern "C" {

int64_t df_ssim_workspace_bytes(int64_t N, int64_t H, int64_t W, int filter_size) {
  Geo geo;
  if (geometry(nullptr, N, H, W, filter_size, &geo) != DF_OK) return -1;
  return N * geo.tiles * 2 * static_cast<int64_t>(sizeof(double));
}

int df_ssim(const float* a, const float* b, const float* taps, float* ssim_map, float* cs_map, float* pool_a, float* pool_b, void* out,
            void* ws, int64_t ws_bytes, int64_t N, int64_t H, int64_t W, int C, int filter_size, float k1, float k2, float min_val,
            float max_val, df_stream_t stream) {
  const char* fn = "df_ssim";
  DF_REQUIRE(a && b, DF_EINVAL, "%s: null image", fn);
  DF_REQUIRE(taps, DF_EINVAL, "%s: null taps", fn);
  DF_REQUIRE(out, DF_EINVAL, "%s: null out", fn);
  DF_REQUIRE(ws, DF_EINVAL, "%s: null workspace", fn);
  DF_REQUIRE((ssim_map != nullptr) == (cs_map != nullptr), DF_EINVAL, "%s: ssim_map and cs_map go together", fn);
  DF_REQUIRE((pool_a != nullptr) == (pool_b != nullptr), DF_EINVAL, "%s: pool_a and pool_b go together", fn);
  DF_REQUIRE(C >= 1 && C <= DF_SSIM_MAX_CHANNELS, DF_EINVAL, "%s: C must be in 1..%d, got %d", fn, DF_SSIM_MAX_CHANNELS, C);
  Geo geo;
  if (int e = geometry(fn, N, H, W, filter_size, &geo)) return e;
  DF_REQUIRE(std::isfinite(min_val) && std::isfinite(max_val) && max_val != min_val, DF_EINVAL,
             "%s: min_val and max_val must be finite and differ (got %g, %g)", fn, (double)min_val, (double)max_val);
  DF_REQUIRE(aligned(a, 4) && aligned(b, 4) && aligned(ssim_map, 4) && aligned(cs_map, 4) && aligned(pool_a, 4) && aligned(pool_b, 4), DF_EALIGN,
             "%s: images, maps and pooled images must be 4-byte aligned", fn);
  DF_REQUIRE(aligned(out, 8) && aligned(ws, 8), DF_EALIGN, "%s: out and the workspace must be 8-byte aligned", fn);
  const int64_t need = N * geo.tiles * 2 * static_cast<int64_t>(sizeof(double));
  DF_REQUIRE(ws_bytes >= need, DF_EWORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn, (long long)ws_bytes, (long long)need);
  const int64_t ibytes = 4 * N * H * W * C, mbytes = 4 * N * geo.OH * geo.OW, pbytes = 4 * N * geo.PH * geo.PW * C;
  const Buf bufs[] = {{a, ibytes, "a", false},          {b, ibytes, "b", false},          {out, 4 * N * DF_SSIM_WORDS, "out", true},
                      {ws, need, "the workspace", true}, {ssim_map, mbytes, "ssim_map", true}, {cs_map, mbytes, "cs_map", true},
                      {pool_a, pbytes, "pool_a", true},  {pool_b, pbytes, "pool_b", true}};
  constexpr int nb = sizeof(bufs) / sizeof(bufs[0]);
  for (int i = 0; i < nb; ++i)
    for (int j = i + 1; j < nb; ++j)
      if (bufs[i].p && bufs[j].p && (bufs[i].written || bufs[j].written))
        DF_REQUIRE(apart(bufs[i].p, bufs[i].bytes, bufs[j].p, bufs[j].bytes), DF_EINVAL, "%s: %s overlaps %s", fn, bufs[j].name, bufs[i].name);
  Args args;
  args.a = a; args.b = b; args.smap = ssim_map; args.cmap = cs_map; args.pa = pool_a; args.pb = pool_b;
  args.partial = static_cast<double*>(ws);
  args.H = (int)H; args.W = (int)W; args.S = geo.S; args.OH = geo.OH; args.OW = geo.OW; args.nty = geo.nty; args.ntx = geo.ntx;
  args.PH = geo.PH; args.PW = geo.PW;
  args.lo = min_val; args.range = max_val - min_val;
  args.inv_c2 = static_cast<float>(1.0 / static_cast<double>(C * C));
  args.c1 = k1 * k1; args.c2 = k2 * k2;
  for (int i = 0; i < kMaxSize; ++i) args.taps[i] = i < geo.S ? taps[i] : 0.f;
  hipStream_t s = df::as_stream(stream);
  const unsigned blocks = static_cast<unsigned>(N * geo.tiles);
  switch (C) {
    case 1: launch<1>(args, blocks, s); break;
    case 2: launch<2>(args, blocks, s); break;
    case 3: launch<3>(args, blocks, s); break;
    default: launch<4>(args, blocks, s); break;
  }
  if (int e = df::launched(fn)) return e;
  hipLaunchKernelGGL(ssim_final_kernel, dim3((unsigned)N), dim3(kThreads), 0, s, static_cast<const double*>(ws), (int)geo.tiles,
                     geo.OH * geo.OW, static_cast<int32_t*>(out));
  return df::launched(fn);
}

int df_ssim_group_mean(const void* out, void* mean, int64_t G, int64_t M, df_stream_t stream) {
  const char* fn = "df_ssim_group_mean";
  DF_REQUIRE(out, DF_EINVAL, "%s: null out", fn);
  DF_REQUIRE(mean, DF_EINVAL, "%s: null mean", fn);
  DF_REQUIRE(G > 0 && M > 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(G < kIndexLimit && M < kIndexLimit, DF_ESHAPE, "%s: %lld groups of %lld images are more than one launch holds", fn, (long long)G, (long long)M);
  DF_REQUIRE(aligned(out, 8) && aligned(mean, 8), DF_EALIGN, "%s: out and mean must be 8-byte aligned", fn);
  DF_REQUIRE(apart(out, 4 * G * M * DF_SSIM_WORDS, mean, 16 * G), DF_EINVAL, "%s: mean overlaps out", fn);
  hipLaunchKernelGGL(ssim_group_mean_kernel, dim3((unsigned)G), dim3(kThreads), 0, df::as_stream(stream), static_cast<const int32_t*>(out),
                     (int)M, static_cast<double*>(mean));
  return df::launched(fn);
}

}  // extern "C"
