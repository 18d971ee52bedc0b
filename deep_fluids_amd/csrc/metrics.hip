// Fused field metrics (include/deepfluids_hip_metrics.h holds the definition, summation order included): how far a generated velocity
// field g is from the ground truth x, per batch entry, in one pass.  HBM-bound: a lane owns one cell at a time and reads its record
// and the records of its forward (on a far face: backward) neighbours as 8- / 12-byte loads -- the 64 records of a wave are one
// contiguous span, the neighbours are some other lane's own records and come from L1 / L2 -- so HBM sees g, x and the mask once.
// The composition of existing ops this replaces (two Jacobians, two divergences, differences, |.| and eight torch reductions) moves
// more than ten times the bytes and allocates two 9-channel tensors.
//   field_metrics_kernel<D>   one workgroup per 1024 cells of ONE entry (so an entry's sums do not depend on B) -> one Partial
//   field_metrics_final_kernel  one workgroup per entry: its Partials in a fixed order -> the 16 output words
// No atomics; fp32 per thread (<= 4 cells), fp64 across threads and workgroups, rounded to fp32 once.
#include "df_common.hpp"
#include "stencil_common.hpp"

#include "../../include/deepfluids_hip_metrics.h"

namespace {

using df::ceil_div;
constexpr int kThreads = 256;
constexpr int kCellsPerThread = 4;
constexpr int kCellsPerBlock = kThreads * kCellsPerThread;      // 1024
constexpr int kWaves = kThreads / 64;

enum { S_ABS = 0, S_SQ, S_ABS_X, S_SQ_X, S_JAC, S_DIV_G, S_DIV_X, NSUM };

// what a workgroup hands to the final kernel (and the type every reduction step combines)
struct Partial {
  double s[NSUM];
  float m, mdg, mdx;      // max m (-1: nothing counted yet), max |div g|, max |div x|
  int idx, cnt, dcnt;     // cell of max m (-1: none), counted cells, counted cells that hold a divergence
};
static_assert(sizeof(Partial) == 80, "Partial is 7 doubles + 6 words");

struct Geo {
  int64_t ncell;      // cells per entry (< 2^31)
  int Z, Y, X;
  int nblk;           // workgroups per entry
  int per_entry;      // mask [B,N] (1) or [N] (0)
};

template <int D>
struct Rec {
  float v[D];
};
template <int D>
__device__ __forceinline__ Rec<D> ld(const float* __restrict__ p) {
  return *reinterpret_cast<const Rec<D>*>(p);
}

// a (the earlier one: lower lanes, lower workgroups) combined with b
__device__ __forceinline__ void combine(Partial& a, const Partial& b) {
#pragma unroll
  for (int k = 0; k < NSUM; ++k) a.s[k] = a.s[k] + b.s[k];
  if (b.m > a.m || (b.m == a.m && b.idx < a.idx)) { a.m = b.m; a.idx = b.idx; }
  a.mdg = fmaxf(a.mdg, b.mdg);
  a.mdx = fmaxf(a.mdx, b.mdx);
  a.cnt += b.cnt;
  a.dcnt += b.dcnt;
}

// the tree of step 2 of the header; the result is valid in thread 0
__device__ __forceinline__ void block_reduce(Partial& a) {
  __shared__ Partial part[kWaves];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Partial b;
#pragma unroll
    for (int k = 0; k < NSUM; ++k) b.s[k] = __shfl_down(a.s[k], off, 64);
    b.m = __shfl_down(a.m, off, 64); b.mdg = __shfl_down(a.mdg, off, 64); b.mdx = __shfl_down(a.mdx, off, 64);
    b.idx = __shfl_down(a.idx, off, 64); b.cnt = __shfl_down(a.cnt, off, 64); b.dcnt = __shfl_down(a.dcnt, off, 64);
    combine(a, b);      // lanes >= off combine with values the tree no longer reads
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) part[wid] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) combine(a, part[w]);
  }
}

template <int D>
__global__ __launch_bounds__(kThreads) void field_metrics_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                 const uint8_t* __restrict__ mask, Partial* __restrict__ partial, Geo geo,
                                                                 int nblk_total) {
  // XCD-contiguous numbering (speed only: the z neighbours of a workgroup's cells are then in the L2 of its own XCD); the slot a
  // workgroup writes is that of its LOGICAL number
  const int64_t wg = dfst::xcd_block(blockIdx.x, nblk_total, 0);
  const int e = static_cast<int>(wg / geo.nblk), w = static_cast<int>(wg - static_cast<int64_t>(e) * geo.nblk);
  const int64_t base = static_cast<int64_t>(e) * geo.ncell;      // first cell of the entry
  const uint8_t* mk = mask ? mask + (geo.per_entry ? base : 0) : nullptr;
  const int n[3] = {geo.X, geo.Y, geo.Z};
  const int st[3] = {1, geo.X, geo.X * geo.Y};
  float s[NSUM];
#pragma unroll
  for (int k = 0; k < NSUM; ++k) s[k] = 0.f;
  float m = -1.f, mdg = 0.f, mdx = 0.f;
  int idx = -1, cnt = 0, dcnt = 0;
#pragma unroll
  for (int i = 0; i < kCellsPerThread; ++i) {
    const int64_t c64 = static_cast<int64_t>(w) * kCellsPerBlock + i * kThreads + threadIdx.x;
    if (c64 >= geo.ncell) continue;
    const int c = static_cast<int>(c64);
    if (mk && mk[c] == 0) continue;
    const int row = c / geo.X;
    int co[3];
    co[0] = c - row * geo.X;
    co[2] = D == 3 ? row / geo.Y : 0;
    co[1] = row - co[2] * geo.Y;
    const int64_t v = base + c;
    const Rec<D> og = ld<D>(g + v * D), ox = ld<D>(x + v * D);
    float aj = 0.f, dg = 0.f, dx = 0.f;
    bool inner = true;
#pragma unroll
    for (int a = 0; a < D; ++a) {
      const bool last = co[a] == n[a] - 1;
      const int64_t nb = last ? v - st[a] : v + st[a];      // inside the entry: every extent is >= 2
      const Rec<D> ng = ld<D>(g + nb * D), nx = ld<D>(x + nb * D);
      inner = inner && !last;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const float jg = last ? og.v[k] - ng.v[k] : ng.v[k] - og.v[k];
        const float jx = last ? ox.v[k] - nx.v[k] : nx.v[k] - ox.v[k];
        aj += fabsf(jg - jx);
        if (k == a) { dg = a == 0 ? jg : dg + jg; dx = a == 0 ? jx : dx + jx; }
      }
    }
    float d[D];
#pragma unroll
    for (int k = 0; k < D; ++k) d[k] = og.v[k] - ox.v[k];
    float a1 = fabsf(d[0]) + fabsf(d[1]), a2 = d[0] * d[0] + d[1] * d[1], mm = fmaxf(fabsf(d[0]), fabsf(d[1]));
    float x1 = fabsf(ox.v[0]) + fabsf(ox.v[1]), x2 = ox.v[0] * ox.v[0] + ox.v[1] * ox.v[1];
    if (D == 3) {
      a1 = a1 + fabsf(d[D - 1]); a2 = a2 + d[D - 1] * d[D - 1]; mm = fmaxf(mm, fabsf(d[D - 1]));
      x1 = x1 + fabsf(ox.v[D - 1]); x2 = x2 + ox.v[D - 1] * ox.v[D - 1];
    }
    s[S_ABS] += a1; s[S_SQ] += a2; s[S_ABS_X] += x1; s[S_SQ_X] += x2; s[S_JAC] += aj;
    if (mm > m) { m = mm; idx = c; }      // the thread's cells ascend: the first of equals stays
    ++cnt;
    if (inner) {
      const float adg = fabsf(dg), adx = fabsf(dx);
      s[S_DIV_G] += adg; s[S_DIV_X] += adx;
      mdg = fmaxf(mdg, adg); mdx = fmaxf(mdx, adx);
      ++dcnt;
    }
  }
  Partial p;
#pragma unroll
  for (int k = 0; k < NSUM; ++k) p.s[k] = static_cast<double>(s[k]);
  p.m = m; p.mdg = mdg; p.mdx = mdx; p.idx = idx; p.cnt = cnt; p.dcnt = dcnt;
  block_reduce(p);
  if (threadIdx.x == 0) partial[wg] = p;
}

__global__ __launch_bounds__(kThreads) void field_metrics_final_kernel(const Partial* __restrict__ partial, int nblk, int32_t* __restrict__ out) {
  const Partial* pe = partial + static_cast<int64_t>(blockIdx.x) * nblk;
  Partial a;
#pragma unroll
  for (int k = 0; k < NSUM; ++k) a.s[k] = 0.0;
  a.m = -1.f; a.mdg = 0.f; a.mdx = 0.f; a.idx = -1; a.cnt = 0; a.dcnt = 0;
  for (int i = threadIdx.x; i < nblk; i += kThreads) combine(a, pe[i]);
  block_reduce(a);
  if (threadIdx.x == 0) {
    int32_t* o = out + static_cast<int64_t>(blockIdx.x) * DF_FM_WORDS;
    float* f = reinterpret_cast<float*>(o);
#pragma unroll
    for (int k = 0; k < DF_FM_WORDS; ++k) o[k] = 0;
    o[DF_FM_COUNT] = a.cnt; o[DF_FM_DIV_COUNT] = a.dcnt; o[DF_FM_ARGMAX] = a.idx;
    f[DF_FM_SUM_ABS] = static_cast<float>(a.s[S_ABS]);
    f[DF_FM_SUM_SQ] = static_cast<float>(a.s[S_SQ]);
    f[DF_FM_MAX_ABS] = a.cnt > 0 ? a.m : 0.f;
    f[DF_FM_SUM_ABS_X] = static_cast<float>(a.s[S_ABS_X]);
    f[DF_FM_SUM_SQ_X] = static_cast<float>(a.s[S_SQ_X]);
    f[DF_FM_SUM_ABS_JAC] = static_cast<float>(a.s[S_JAC]);
    f[DF_FM_SUM_ABS_DIV_G] = static_cast<float>(a.s[S_DIV_G]);
    f[DF_FM_MAX_ABS_DIV_G] = a.mdg;
    f[DF_FM_SUM_ABS_DIV_X] = static_cast<float>(a.s[S_DIV_X]);
    f[DF_FM_MAX_ABS_DIV_X] = a.mdx;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
constexpr int64_t kIndexLimit = int64_t(1) << 31;

// cells and workgroups per entry, or a DF_E* code; fn == nullptr: no message (the size query)
int geometry(const char* fn, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, Geo* geo) {
  const bool pos = B > 0 && Z > 0 && Y > 0 && X > 0;
  if (!pos) return fn ? df::fail(DF_EINVAL, "%s: non-positive extent", fn) : DF_EINVAL;
  const bool small = Y < 2 || X < 2 || (dim == 3 ? Z < 2 : Z != 1);
  if (small) return fn ? df::fail(DF_ESHAPE, "%s: the forward differences need every extent >= 2 (got %lld,%lld,%lld)", fn, (long long)Z, (long long)Y, (long long)X) : DF_ESHAPE;
  // (each factor is below 2^31 once the product of the earlier ones is: no overflow)
  const bool big = Z >= kIndexLimit || Y >= kIndexLimit || X >= kIndexLimit || Z * Y >= kIndexLimit || Z * Y * X >= kIndexLimit;
  if (big) return fn ? df::fail(DF_ESHAPE, "%s: %lld x %lld x %lld cells per entry do not fit the int32 cell index", fn, (long long)Z, (long long)Y, (long long)X) : DF_ESHAPE;
  const int64_t ncell = Z * Y * X, nblk = ceil_div(ncell, kCellsPerBlock);
  if (B >= kIndexLimit || B * nblk >= kIndexLimit) return fn ? df::fail(DF_ESHAPE, "%s: %lld entries of %lld workgroups are more than one launch holds", fn, (long long)B, (long long)nblk) : DF_ESHAPE;
  *geo = Geo{ncell, (int)Z, (int)Y, (int)X, (int)nblk, 0};
  return DF_OK;
}

inline bool apart(const void* p, int64_t np, const void* q, int64_t nq) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a + static_cast<uintptr_t>(np) <= b || b + static_cast<uintptr_t>(nq) <= a;
}
inline bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

template <int D>
int field_metrics(const char* fn, const float* g, const float* x, const uint8_t* mask, int mask_per_entry, void* out, void* ws, int64_t ws_bytes,
                  int64_t B, int64_t Z, int64_t Y, int64_t X, df_stream_t stream) {
  DF_REQUIRE(g && x, DF_EINVAL, "%s: null field", fn);
  DF_REQUIRE(out, DF_EINVAL, "%s: null out", fn);
  DF_REQUIRE(ws, DF_EINVAL, "%s: null workspace", fn);
  DF_REQUIRE(mask_per_entry == 0 || mask_per_entry == 1, DF_EINVAL, "%s: mask_per_entry must be 0 or 1, got %d", fn, mask_per_entry);
  Geo geo;
  if (int e = geometry(fn, D, B, Z, Y, X, &geo)) return e;
  geo.per_entry = mask_per_entry;
  DF_REQUIRE(aligned(g, 4) && aligned(x, 4) && aligned(out, 4), DF_EALIGN, "%s: g, x and out must be 4-byte aligned", fn);
  DF_REQUIRE(aligned(ws, 8), DF_EALIGN, "%s: the workspace must be 8-byte aligned", fn);
  const int64_t need = B * geo.nblk * static_cast<int64_t>(sizeof(Partial));
  DF_REQUIRE(ws_bytes >= need, DF_EWORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn, (long long)ws_bytes, (long long)need);
  const int64_t fbytes = 4 * B * geo.ncell * D, obytes = 4 * B * DF_FM_WORDS, mbytes = mask ? (mask_per_entry ? B : 1) * geo.ncell : 0;
  DF_REQUIRE(apart(out, obytes, ws, need), DF_EINVAL, "%s: out overlaps the workspace", fn);
  DF_REQUIRE(apart(out, obytes, g, fbytes) && apart(out, obytes, x, fbytes) && (!mask || apart(out, obytes, mask, mbytes)), DF_EINVAL,
             "%s: out overlaps an input", fn);
  DF_REQUIRE(apart(ws, need, g, fbytes) && apart(ws, need, x, fbytes) && (!mask || apart(ws, need, mask, mbytes)), DF_EINVAL,
             "%s: the workspace overlaps an input", fn);
  hipStream_t s = df::as_stream(stream);
  const int total = static_cast<int>(B * geo.nblk);
  hipLaunchKernelGGL((field_metrics_kernel<D>), dim3((unsigned)total), dim3(kThreads), 0, s, g, x, mask, static_cast<Partial*>(ws), geo, total);
  if (int e = df::launched(fn)) return e;
  hipLaunchKernelGGL(field_metrics_final_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, static_cast<const Partial*>(ws), geo.nblk,
                     static_cast<int32_t*>(out));
  return df::launched(fn);
}

}  // namespace

extern "C" {

int64_t df_field_metrics_workspace_bytes(int dim, int64_t B, int64_t Z, int64_t Y, int64_t X) {
  Geo geo;
  if ((dim != 2 && dim != 3) || geometry(nullptr, dim, B, Z, Y, X, &geo) != DF_OK) return -1;
  return B * geo.nblk * static_cast<int64_t>(sizeof(Partial));
}

int df_field_metrics2d(const float* g, const float* x, const uint8_t* mask, int mask_per_entry, void* out, void* ws, int64_t ws_bytes,
                       int64_t B, int64_t Y, int64_t X, df_stream_t stream) {
  return field_metrics<2>("df_field_metrics2d", g, x, mask, mask_per_entry, out, ws, ws_bytes, B, 1, Y, X, stream);
}

int df_field_metrics3d(const float* g, const float* x, const uint8_t* mask, int mask_per_entry, void* out, void* ws, int64_t ws_bytes,
                       int64_t B, int64_t Z, int64_t Y, int64_t X, df_stream_t stream) {
  return field_metrics<3>("df_field_metrics3d", g, x, mask, mask_per_entry, out, ws, ws_bytes, B, Z, Y, X, stream);
}

}  // extern "C"
