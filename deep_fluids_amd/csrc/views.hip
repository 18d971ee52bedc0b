// uint8 image views of a velocity field for the sample sheets written during training (reference ops.py:154-188, trainer3.py:22-25),
// written for gfx950: one pass over the fp32 field, only the B*(Y*X + Y*Z)*C bytes of each view leave the GPU.
//
//   plane_view(x, xy_plane, project):  xy = mean_z x,  zy = (mean_x x)^T,  xym = x[:, Z/2],  zym = (x[:, :, :, X/2])^T
//   every value -> uint8(clip((v + 1) * 127.5, 0, 255)), fp32 arithmetic throughout (no contraction: -ffp-contract=off)
//
// Data layout: channels-last fp32 [B,Z,Y,X,C], x fastest.  Every output element with a given (b, y) depends on the (b, y) row-plane
// [Z][X*C] only, so ONE workgroup owns one (b, y): it walks z in chunks of ZT rows, stages a chunk in LDS with lane-consecutive
// 16-byte loads, and takes from the staged rows
//   - per element (x, c): the running z sum (a register inside a chunk, an LDS word between chunks) and the Z/2 slice,
//   - per (z, c): the x sum, in ascending x like the z sum in ascending z (the order of a plain sequential mean), and the X/2 slice.
// No atomics, no second pass, no dependence on the launch geometry: two launches are bitwise equal.  The four uint8 rows are collected in
// LDS and leave as 32-bit words where the row offset allows.  The staged row stride is padded to 4 (mod 32) dwords: 16-byte LDS writes stay
// aligned and the per-(z, c) readers of a 32-lane group (bank = 4 z + c) collide two-way at worst.
//
// velocity_views3d adds the same four views of curl(u) without ever writing the curl: the chunk is staged with one extra z row, the
// x+1 / z+1 neighbours come from LDS, the y+1 row from L1/L2 (it is the neighbouring workgroup's own row-plane; the XCD-aware block
// remap keeps neighbours on one L2), and the differences are formed exactly as in jacobian3d_fwd_kernel (stencil.hip) -- replicated
// last difference, c = (dwdy-dvdz, dudz-dwdx, dvdx-dudy) -- so the views equal those of df_jacobian3d_fwd's c bit for bit.
#include "df_common.hpp"
#include "stencil_common.hpp"

namespace {

using df::ceil_div;
using dfst::f32x4;
using dfst::kThreads;
using dfst::xcd_block;

constexpr int kMaxZT = 16;                 // z rows staged per chunk (29 KB of LDS at 64x96x64x3 with the curl: five workgroups per CU)
constexpr int64_t kLdsLimit = 64 * 1024;   // dynamic LDS a workgroup gets without opting in

struct ViewDims {
  int B, Z, Y, X, C;
  int RC;    // X*C: floats per row
  int RCp;   // staged row stride (floats)
  int ZT;    // rows per chunk
};

struct Views {      // four device outputs of one field; any may be null
  uint8_t *xy, *zy, *xym, *zym;
};

struct FieldLds {   // per-field LDS state of a workgroup
  float* zacc;      // [RC] running z sums between chunks
  uint8_t *xy, *xym, *zy, *zym;      // [RC], [RC], [Z*C], [Z*C] bytes of this (b, y) row
};

__device__ __forceinline__ uint8_t denorm(float v) {
  const float s = (v + 1.0f) * 127.5f;
  return static_cast<uint8_t>(static_cast<int>(fminf(fmaxf(s, 0.0f), 255.0f)));
}

__host__ __device__ inline int round4(int n) { return (n + 3) & ~3; }

__device__ __forceinline__ FieldLds carve_field(float*& fp, uint8_t*& bp, const ViewDims& d) {
  FieldLds f;
  f.zacc = fp; fp += d.RC;
  f.xy = bp; bp += round4(d.RC);
  f.xym = bp; bp += round4(d.RC);
  f.zy = bp; bp += round4(d.Z * d.C);
  f.zym = bp; bp += round4(d.Z * d.C);
  return f;
}

// rows i = 0..nrows-1 of the (b, y) row-plane into tile[i][RCp]; row i holds z = zrow(i)
template <bool VEC, typename ZR>
__device__ __forceinline__ void stage_rows(const float* __restrict__ x, float* tile, int64_t b, int y, int nrows, const ViewDims& d,
                                           int tid, const ZR& zrow) {
  if (VEC) {
    const int Q = d.RC >> 2;
    for (int q = tid; q < nrows * Q; q += kThreads) {
      const int i = q / Q, k = q - i * Q;
      const f32x4* src = reinterpret_cast<const f32x4*>(x + ((b * d.Z + zrow(i)) * d.Y + y) * d.RC);
      *reinterpret_cast<f32x4*>(tile + i * d.RCp + 4 * k) = src[k];
    }
  } else {
    for (int q = tid; q < nrows * d.RC; q += kThreads) {
      const int i = q / d.RC, k = q - i * d.RC;
      tile[i * d.RCp + k] = x[((b * d.Z + zrow(i)) * d.Y + y) * d.RC + k];
    }
  }
}

// the four views' share of the staged rows z0 .. z0+n-1
__device__ __forceinline__ void views_of_tile(const float* tile, int z0, int n, const ViewDims& d, const FieldLds& f, const Views& o,
                                              int tid) {
  const int zm = d.Z / 2, xm = d.X / 2;
  if (o.xy || o.xym) {
    for (int e = tid; e < d.RC; e += kThreads) {
      if (o.xy) {
        float a = z0 == 0 ? tile[e] : f.zacc[e];
        for (int i = z0 == 0 ? 1 : 0; i < n; ++i) a += tile[i * d.RCp + e];
        if (z0 + n == d.Z) f.xy[e] = denorm(a / static_cast<float>(d.Z));
        else f.zacc[e] = a;
      }
      if (o.xym && zm >= z0 && zm < z0 + n) f.xym[e] = denorm(tile[(zm - z0) * d.RCp + e]);
    }
  }
  if (o.zy || o.zym) {
    for (int p = tid; p < n * d.C; p += kThreads) {
      const int i = p / d.C, c = p - i * d.C;
      const float* row = tile + i * d.RCp + c;
      if (o.zy) {
        float s = row[0];
        for (int xx = 1; xx < d.X; ++xx) s += row[xx * d.C];
        f.zy[(z0 + i) * d.C + c] = denorm(s / static_cast<float>(d.X));
      }
      if (o.zym) f.zym[(z0 + i) * d.C + c] = denorm(row[xm * d.C]);
    }
  }
}

// one uint8 row from LDS (4-byte aligned) to global: 32-bit words where the destination allows, bytes otherwise and for the tail
__device__ __forceinline__ void flush_row(const uint8_t* s, uint8_t* g, int len, int tid) {
  if (g == nullptr) return;
  int done = 0;
  if ((reinterpret_cast<uintptr_t>(g) & 3u) == 0) {
    const int nw = len >> 2;
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
    uint32_t* g4 = reinterpret_cast<uint32_t*>(g);
    for (int w = tid; w < nw; w += kThreads) g4[w] = s4[w];
    done = nw << 2;
  }
  for (int k = done + tid; k < len; k += kThreads) g[k] = s[k];
}

__device__ __forceinline__ void flush_field(const FieldLds& f, const Views& o, int64_t blk, const ViewDims& d, int tid) {
  const int zc = d.Z * d.C;
  flush_row(f.xy, o.xy ? o.xy + blk * d.RC : nullptr, d.RC, tid);
  flush_row(f.xym, o.xym ? o.xym + blk * d.RC : nullptr, d.RC, tid);
  flush_row(f.zy, o.zy ? o.zy + blk * zc : nullptr, zc, tid);
  flush_row(f.zym, o.zym ? o.zym + blk * zc : nullptr, zc, tid);
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void plane_views3d_kernel(const float* __restrict__ x, Views o, ViewDims d) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  float* tile = smem;                                   // [ZT][RCp]
  float* fp = tile + d.ZT * d.RCp;
  uint8_t* bp = reinterpret_cast<uint8_t*>(fp + d.RC);
  const FieldLds f = carve_field(fp, bp, d);
  const int64_t blk = xcd_block(blockIdx.x, gridDim.x, 0);      // (b, y)
  const int64_t b = blk / d.Y;
  const int y = static_cast<int>(blk - b * d.Y);
  for (int z0 = 0; z0 < d.Z; z0 += d.ZT) {
    const int n = d.Z - z0 < d.ZT ? d.Z - z0 : d.ZT;
    stage_rows<VEC>(x, tile, b, y, n, d, tid, [&](int i) { return z0 + i; });
    __syncthreads();
    views_of_tile(tile, z0, n, d, f, o, tid);
    __syncthreads();                                    // the next chunk overwrites the rows just read
  }
  flush_field(f, o, blk, d, tid);
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void velocity_views3d_kernel(const float* __restrict__ u, Views ou, Views oc, ViewDims d) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  float* tu = smem;                                     // [ZT + 1][RCp]: the chunk of u and its z+1 row
  float* tc = tu + (d.ZT + 1) * d.RCp;                  // [ZT][RCp]: curl(u) of the chunk
  float* fp = tc + d.ZT * d.RCp;
  uint8_t* bp = reinterpret_cast<uint8_t*>(fp + 2 * d.RC);
  const FieldLds fu = carve_field(fp, bp, d);
  const FieldLds fc = carve_field(fp, bp, d);
  const int64_t blk = xcd_block(blockIdx.x, gridDim.x, 0);
  const int64_t b = blk / d.Y;
  const int y = static_cast<int>(blk - b * d.Y);
  const bool ly = y == d.Y - 1;
  const int yn = ly ? y - 1 : y + 1;                    // the row the y difference reaches for
  for (int z0 = 0; z0 < d.Z; z0 += d.ZT) {
    const int n = d.Z - z0 < d.ZT ? d.Z - z0 : d.ZT;
    // row n is the z neighbour of row n-1: z0+n, or behind the last slice Z-2 (the replicated difference looks back)
    stage_rows<VEC>(u, tu, b, y, n + 1, d, tid, [&](int i) { return z0 + i < d.Z ? z0 + i : d.Z - 2; });
    __syncthreads();
    for (int v = tid; v < n * d.X; v += kThreads) {
      const int i = v / d.X, xx = v - i * d.X;
      const int z = z0 + i;
      const bool lx = xx == d.X - 1, lz = z == d.Z - 1;
      const float* po = tu + i * d.RCp + xx * 3;
      const float* px = lx ? po - 3 : po + 3;
      const float* pz = po + d.RCp;
      const float* py = u + (((b * d.Z + z) * d.Y + yn) * d.X + xx) * 3;
      float dx[3], dy[3], dz[3];
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) {
        const float own = po[cc], nx = px[cc], ny = py[cc], nz = pz[cc];
        dx[cc] = lx ? own - nx : nx - own;
        dy[cc] = ly ? own - ny : ny - own;
        dz[cc] = lz ? own - nz : nz - own;
      }
      float* q = tc + i * d.RCp + xx * 3;               // (dwdy-dvdz, dudz-dwdx, dvdx-dudy)
      q[0] = dy[2] - dz[1];
      q[1] = dz[0] - dx[2];
      q[2] = dx[1] - dy[0];
    }
    views_of_tile(tu, z0, n, d, fu, ou, tid);
    __syncthreads();                                    // curl rows complete; every reader of tu is done
    views_of_tile(tc, z0, n, d, fc, oc, tid);           // (the next chunk's barrier separates these reads from the next curl writes)
  }
  __syncthreads();
  flush_field(fu, ou, blk, d, tid);
  flush_field(fc, oc, blk, d, tid);
}

// ---- 2-D: denorm_img (ops.py:154-161) --------------------------------------------------------------------------------------------
// x [B,H,W,C] (or [B,C,H,W]) -> uint8 [B,H,W,Co]; Co = 3 for C = 2 (a zero channel is appended BEFORE the mapping: it shows as 127) and
// for C > 3 (the first three are kept), else C.  One thread = four consecutive output bytes = one 32-bit store.
__global__ __launch_bounds__(kThreads) void denorm_img2d_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, int64_t nbytes,
                                                                int64_t HW, int C, int Co, int nchw, int words) {
  const int64_t o0 = 4 * (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x);
  if (o0 >= nbytes) return;
  uint32_t r[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t o = o0 + j;
    if (o < nbytes) {
      const int64_t pix = o / Co;
      const int ch = static_cast<int>(o - pix * Co);
      float v = 0.0f;
      if (ch < C) {
        if (nchw) {
          const int64_t bb = pix / HW;
          v = x[(bb * C + ch) * HW + (pix - bb * HW)];
        } else {
          v = x[pix * C + ch];
        }
      }
      r[j] = denorm(v);
    }
  }
  if (words && o0 + 4 <= nbytes) {
    *reinterpret_cast<uint32_t*>(out + o0) = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (o0 + j < nbytes) out[o0 + j] = static_cast<uint8_t>(r[j]);
  }
}

// geometry shared by the two 3-D entry points: `fields` = 1 (views of x) | 2 (views of u and of curl u, one extra staged row)
int plan3(const void* in, int64_t B, int64_t Z, int64_t Y, int64_t X, int64_t C, int fields, const char* fn, ViewDims* d, size_t* lds) {
  DF_REQUIRE(in != nullptr, DF_EINVAL, "%s: null input", fn);
  DF_REQUIRE(B > 0 && Z > 0 && Y > 0 && X > 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(C >= 1 && C <= 4, DF_ESHAPE, "%s: channel count must be 1..4 (got %lld)", fn, (long long)C);
  if (fields == 2)
    DF_REQUIRE(Z >= 2 && Y >= 2 && X >= 2, DF_ESHAPE, "%s: forward difference needs every extent >= 2 (got %lld,%lld,%lld)", fn,
               (long long)Z, (long long)Y, (long long)X);
  DF_REQUIRE(Z < (1 << 30) && Y < (1 << 30) && X < (1 << 30) && B * Y < (1ll << 31), DF_ESHAPE, "%s: extent too large", fn);
  DF_REQUIRE((reinterpret_cast<uintptr_t>(in) & 3u) == 0, DF_EALIGN, "%s: input must be 4-byte aligned", fn);
  const int64_t RC = X * C;
  const int64_t RCp = RC + ((4 - RC % 32) + 32) % 32;
  const int64_t fixed = fields * (RC * 4 + 2 * ((RC + 3) & ~3ll) + 2 * ((Z * C + 3) & ~3ll));
  // rows staged for a chunk of zt slices: zt (+ zt curl rows + the z+1 row)
  auto bytes = [&](int64_t zt) { return fixed + (fields == 2 ? 2 * zt + 1 : zt) * RCp * 4; };
  int64_t zt = Z < kMaxZT ? Z : kMaxZT;
  while (zt > 1 && bytes(zt) > kLdsLimit) --zt;
  DF_REQUIRE(bytes(zt) <= kLdsLimit, DF_ESHAPE, "%s: a row-plane of %lld x %lld x %lld values does not fit the workgroup's LDS", fn,
             (long long)Z, (long long)X, (long long)C);
  *d = ViewDims{(int)B, (int)Z, (int)Y, (int)X, (int)C, (int)RC, (int)RCp, (int)zt};
  *lds = static_cast<size_t>(bytes(zt));
  return DF_OK;
}

}  // namespace

extern "C" {

int df_plane_views3d(const float* x, uint8_t* xy, uint8_t* zy, uint8_t* xym, uint8_t* zym, int64_t B, int64_t Z, int64_t Y, int64_t X,
                     int64_t C, df_stream_t stream) {
  ViewDims d;
  size_t lds;
  if (int e = plan3(x, B, Z, Y, X, C, 1, "df_plane_views3d", &d, &lds)) return e;
  DF_REQUIRE(xy || zy || xym || zym, DF_EINVAL, "df_plane_views3d: every output null");
  const Views o{xy, zy, xym, zym};
  dim3 grid((unsigned)(B * Y)), block(kThreads);
  hipStream_t s = df::as_stream(stream);
  if (d.RC % 4 == 0 && df::aligned16(x)) hipLaunchKernelGGL((plane_views3d_kernel<true>), grid, block, lds, s, x, o, d);
  else hipLaunchKernelGGL((plane_views3d_kernel<false>), grid, block, lds, s, x, o, d);
  return df::launched("df_plane_views3d");
}

int df_velocity_views3d(const float* u, uint8_t* xy, uint8_t* zy, uint8_t* xym, uint8_t* zym, uint8_t* cxy, uint8_t* czy, uint8_t* cxym,
                        uint8_t* czym, int64_t B, int64_t Z, int64_t Y, int64_t X, df_stream_t stream) {
  ViewDims d;
  size_t lds;
  if (int e = plan3(u, B, Z, Y, X, 3, 2, "df_velocity_views3d", &d, &lds)) return e;
  DF_REQUIRE(xy || zy || xym || zym || cxy || czy || cxym || czym, DF_EINVAL, "df_velocity_views3d: every output null");
  const Views ou{xy, zy, xym, zym}, oc{cxy, czy, cxym, czym};
  dim3 grid((unsigned)(B * Y)), block(kThreads);
  hipStream_t s = df::as_stream(stream);
  if (d.RC % 4 == 0 && df::aligned16(u)) hipLaunchKernelGGL((velocity_views3d_kernel<true>), grid, block, lds, s, u, ou, oc, d);
  else hipLaunchKernelGGL((velocity_views3d_kernel<false>), grid, block, lds, s, u, ou, oc, d);
  return df::launched("df_velocity_views3d");
}

int df_denorm_img2d(const float* x, uint8_t* out, int64_t B, int64_t H, int64_t W, int64_t C, int nchw, df_stream_t stream) {
  DF_REQUIRE(x != nullptr && out != nullptr, DF_EINVAL, "df_denorm_img2d: null %s", x ? "output" : "input");
  DF_REQUIRE(B > 0 && H > 0 && W > 0, DF_EINVAL, "df_denorm_img2d: non-positive extent");
  DF_REQUIRE(C >= 1 && C < (1 << 20), DF_ESHAPE, "df_denorm_img2d: channel count must be >= 1 (got %lld)", (long long)C);
  DF_REQUIRE(H < (1 << 30) && W < (1 << 30), DF_ESHAPE, "df_denorm_img2d: extent too large");
  DF_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3u) == 0, DF_EALIGN, "df_denorm_img2d: input must be 4-byte aligned");
  const int Co = (C == 2 || C > 3) ? 3 : (int)C;
  const int64_t nbytes = B * H * W * Co;
  const int64_t nblk = ceil_div(ceil_div(nbytes, 4), kThreads);
  DF_REQUIRE(nblk < (1ll << 31), DF_ESHAPE, "df_denorm_img2d: extent too large");
  const int words = (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
  hipLaunchKernelGGL(denorm_img2d_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, df::as_stream(stream), x, out, nbytes, H * W, (int)C,
                     Co, nchw ? 1 : 0, words);
  return df::launched("df_denorm_img2d");
}

}  // extern "C"
