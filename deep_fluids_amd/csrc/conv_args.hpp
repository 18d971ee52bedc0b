// Shared argument block / constants of the convolution kernels (conv.hip, conv_small.hip).
#pragma once
#include "df_common.hpp"

namespace dfconv {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int CK = 16;          // input channels per LDS chunk
constexpr int LDS_STRIDE = 20;  // floats per staged voxel (16 + 4 pad)

struct ConvArgs {
  const float* x;
  const f32x4* wp;
  const float* bias;
  const float* residual;
  const float* mask_src;
  float* y;
  int B, D, H, W, Cin, Cout;   // D,H,W: OUTPUT extents
  int Di, Hi, Wi;              // LOGICAL input extents the taps slide over (== output for stride 1; 2x for stride 2)
  // generalisation used by the up-sampling-aware first conv of a generator block (conv on the NN-upsampled
  // input == 8 parity-class 2x2x2-tap convs on the coarse grid) and its dgrad; identity values for a plain conv:
  int pz, py, px;              // logical input coordinate of tap 0 = out*S - p   (plain k=3: 1; stride 2: 0)
  int is, iz, iy, ix;          // physical input voxel  = logical*is + i?  (gather stride / offset)
  int xD, xH, xW;              // physical extents of the x tensor (addressing)
  int os, oz, oy, ox;          // physical output voxel = logical*os + o?  (scatter stride / offset)
  int yD, yH, yW;              // physical extents of y / residual / mask_src
  int nclass;                  // > 1: blockIdx.z = parity class c; p = 1 - bit(c), o = bit(c), weights += c*wclass
  int64_t wclass;              // packed-weight stride between classes (float4 units)
  int Kpad, Npad;       // padded K (multiple of 16) and N (multiple of the N tile) of the packed weights
  int nz, ny, nx;       // tiles per axis
  int ntiles;
  int flags;
  float leak;
};


// XCD-aware, bijective workgroup -> tile mapping (workgroup b runs on XCD b % 8; speed only)
__device__ __forceinline__ int xcd_tile(int bid, int ntiles) {
  const int q = ntiles >> 3, rem = ntiles & 7;
  const int xcd = bid & 7, idx = bid >> 3;
  return (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + idx;
}

// Grid of the persistent 3-D Winograd kernels (conv_wino.hip: WinoArgs, conv_wino43.hip: W43Args): one workgroup per CU (a workgroup owns a
// CU's whole register file and most of its LDS), fewer when there are fewer (tile block, cout slice) items.  Sets a.spx = cout slices per XCD.
template <class Args>
inline int64_t wino_grid(Args& a, int64_t ntb) {
  int64_t grid = df::kCUs;
  a.spx = 1;
  if (8 % a.ncs == 0) {      // the slice count divides the 8 XCDs: an XCD only ever sees spx slices (their weights stay L2-resident)
    a.spx = a.ncs % 2 == 0 ? 2 : 1;
    const int xpg = a.ncs / a.spx, ngroups = 8 / xpg;
    const int64_t need = df::ceil_div(ntb, ngroups) * a.spx * 8;      // workers that get at least one tile block
    if (need < grid) grid = need;
    if ((grid >> 3) % a.spx) grid = ((grid >> 3) / a.spx + 1) * a.spx * 8;
    if (grid > df::kCUs) grid = df::kCUs;
  } else {
    grid = (grid / a.ncs) * a.ncs;
    if (ntb * a.ncs < grid) grid = ntb * a.ncs;
  }
  return grid;
}

// The generic mapping above (and its twins wino2d_grid of conv_wino2d.hip and w2_grid of conv_wino2d43.hip) gives every cout slice the same
// number of workers out of the one-workgroup-per-CU grid: (kCUs / ncs) * ncs workgroups, which is an EMPTY grid from kCUs + 1 slices on.  Every
// Winograd conv entry point of the four files refuses such a call here (ncs = the kernel's cout slices of 32 channels), before it computes a grid.
constexpr int kWinoMaxSlices = df::kCUs;
inline int wino_slices_check(const char* name, int64_t ncs) {
  DF_REQUIRE(ncs <= kWinoMaxSlices, DF_ESHAPE, "%s: %lld cout slices of 32 channels, the persistent grid serves at most %d (%d output channels)", name,
             static_cast<long long>(ncs), kWinoMaxSlices, 32 * kWinoMaxSlices);
  return DF_OK;
}

// VALU kernels for the generator's last layer (conv_small.hip); return DF_OK or an error
int launch_small_n(const ConvArgs& a, int kz, hipStream_t s);   // Cout <= 4  (128 -> 3 | 1)
int launch_small_k(const ConvArgs& a, int kz, hipStream_t s);   // Cin  <= 4  (dgrad of the last layer; 3 -> F)

// bf16x3 split-precision MFMA path (conv_bf16.hip)
bool bf16x3_supported(const ConvArgs& a);
int64_t bf16x3_kpad(int64_t K);
int launch_bf16x3(const ConvArgs& a, int kz, int kt, hipStream_t s);
int pack_bf16x3(const float* w, void* wp, int taps, int cin, int cout, int Kpad, int Npad, int mode, hipStream_t s);
int upconv_pack_bf16x3(const float* w, void* wp, int kz, int cin, int cout, int Kpad, int Npad, int mode, hipStream_t s);

}  // namespace dfconv
