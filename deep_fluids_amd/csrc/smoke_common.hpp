// What the pressure solves of smoke.hip and the multigrid preconditioner of multigrid.hip share: the grid of a solve (workgroups that
// never straddle batch entries), the per-entry state words, the fixed-order reductions and the carving of the workspace.  Moved here from
// smoke.hip word for word; every translation unit gets its own copy (anonymous namespace), as before.
#pragma once
#include "advect_common.hpp"
#include "df_common.hpp"
#include "stencil_common.hpp"

namespace {

using dfadv::kFluid;
using dfst::kThreads;
using dfst::xcd_block;

struct PDims {
  int64_t n;       // cells of one batch entry
  int nblk;        // workgroups of one batch entry
  int B, Z, Y, X, bnd;
};

struct CgState {   // per batch entry, 32 bytes
  float rr, maxr, alpha, beta, pq;
  int active, iters, pad;
};

struct PCell {
  int64_t cell;    // index inside the entry
  int e;           // batch entry
  int j;           // workgroup inside the entry
  int p[3];
  bool interior;   // MASKED: fluid
  unsigned fl;     // MASKED: the flags byte of a fluid cell, else 0
};

template <int D, bool MASKED = false>
__device__ __forceinline__ PCell pdecode(const PDims& d, const uint8_t* __restrict__ flags = nullptr) {
  PCell c;
  const int64_t logical = xcd_block(blockIdx.x, gridDim.x, 0);
  c.e = static_cast<int>(logical / d.nblk);
  c.j = static_cast<int>(logical - static_cast<int64_t>(c.e) * d.nblk);
  c.cell = static_cast<int64_t>(c.j) * kThreads + threadIdx.x;
  const int64_t row = c.cell / d.X;
  c.p[0] = static_cast<int>(c.cell - row * d.X);
  c.p[1] = static_cast<int>(row % d.Y);
  c.p[2] = D == 3 ? static_cast<int>(row / d.Y) : 0;
  c.interior = c.cell < d.n && c.p[0] >= d.bnd && c.p[0] < d.X - d.bnd && c.p[1] >= d.bnd && c.p[1] < d.Y - d.bnd &&
               (D == 2 || (c.p[2] >= d.bnd && c.p[2] < d.Z - d.bnd));
  c.fl = 0u;
  if (MASKED) {
    if (c.interior) c.fl = flags[static_cast<int64_t>(c.e) * d.n + c.cell];
    c.interior = (c.fl & kFluid) != 0u;
    if (!c.interior) c.fl = 0u;
  }
  return c;
}

// Fixed-order reductions over the workgroup: xor butterfly inside a wave (every lane ends with the same bits: a + b == b + a), then the
// four wave results in ascending order.  Every thread returns the total.  `lds` holds 4 floats and is free again after the call.
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* lds) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float o = __shfl_xor(v, m);
    v = MAX ? fmaxf(v, o) : v + o;
  }
  __syncthreads();                                      // the previous use of lds is over
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return MAX ? fmaxf(fmaxf(fmaxf(lds[0], lds[1]), lds[2]), lds[3]) : ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// the nblk partials of one entry, combined by every workgroup of the entry in the same order
template <bool MAX>
__device__ __forceinline__ float entry_reduce(const float* __restrict__ part, int nblk, float* lds) {
  float a = 0.0f;
  for (int t = threadIdx.x; t < nblk; t += kThreads) a = MAX ? fmaxf(a, part[t]) : a + part[t];
  return block_reduce<MAX>(a, lds);
}

struct PWs {
  float *r, *p[2], *q, *pq_part, *rr_part, *mx_part;
  CgState* state[2];
};

int64_t ws_floats(int64_t B, int64_t n, int64_t nblk) { return 4 * B * n + 3 * B * nblk + 2 * B * (int64_t)(sizeof(CgState) / 4); }

PWs carve(void* ws, int64_t B, int64_t n, int64_t nblk) {
  PWs w;
  float* f = static_cast<float*>(ws);
  const int64_t N = B * n, P = B * nblk;
  w.r = f; w.p[0] = f + N; w.p[1] = f + 2 * N; w.q = f + 3 * N;
  w.pq_part = f + 4 * N; w.rr_part = w.pq_part + P; w.mx_part = w.rr_part + P;
  w.state[0] = reinterpret_cast<CgState*>(w.mx_part + P);
  w.state[1] = w.state[0] + B;
  return w;
}

}  // namespace
