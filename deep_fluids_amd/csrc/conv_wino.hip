// 3x3x3 SAME stride-1 convolution as Winograd F(2x2x2, 3x3x3) on the fp32 matrix cores
// (reference: slim.conv3d behind ops.py:12-16, called from model.py:68,84 -- the 128->128 layers of GeneratorBE3).
//
//   Y = A^T [ sum_cin (G g G^T) .* (B^T d B) ] A        per 2x2x2 output tile / 4x4x4 input tile, 64 transform points xi
// = 64 independent GEMMs  M_xi[tile][cout] = sum_cin V_xi[tile][cin] * U_xi[cin][cout]:   8 MFMA MACs per output voxel
// and (cin,cout) pair instead of 27 -> 3.375x fewer matrix-core FLOPs than the direct kernel (conv.hip); all arithmetic
// stays fp32 (v_mfma_f32_16x16x4_f32 + exact +-1 / 0.5 transform factors), results differ from the direct sum only by
// fp32 rounding order (tests: same tolerance as the direct kernel against the fp64 oracle).
//
// Persistent workgroup = 8 waves (two per SIMD: measured on gfx950, a wave's own VALU / LDS / VMEM instructions do NOT
// overlap its own MFMAs -- a second wave on the SIMD is what keeps the matrix pipe busy) = one block of 2x4x4 tiles
// (4x8x8 output voxels) x 32 output channels at a time.  Wave (xi_z, tz) owns the 16 transform points with that xi_z
// for the 16 tiles of z-row tz: 32 MFMA 16x16x4 per k-step (4 input channels), 128 accumulator registers.
//   * input: the 6x10x10 halo block of a 16-channel chunk is staged in LDS channel-major ([c][z*144 + y*12 + x], the
//     pitches make every wave-wide ds_read2_b64 below bank-conflict free), double buffered, one barrier per chunk;
//     the next tile block's first chunk is staged during the last chunk of the current one.
//   * A operand: lane = (tile, cin%4) reads the 2 z-planes x 4 x 4 inputs of its tile that xi_z needs (8 ds_read2_b64),
//     runs the separable B^T transform in registers (24 packed-fp32 VALU ops) and so produces the 16 A values of one
//     k-step directly in MFMA A layout -- the transformed input never touches memory.
//   * B operand: transformed weights U are packed [cout/32][xi_z][cin/4][cout/16%2][xi_y][cin%4][cout%16][xi_x] so that
//     a lane needs 8 coalesced 16-byte global loads per k-step (L2 / L1 hits: the two tz waves read the same words).
//   * epilogue: inverse transform in y,x in registers, the four xi_z partial planes are combined through the idle LDS
//     buffer, then bias / lrelu / residual / lrelu-mask as in conv.hip.  The dgrad is the same kernel on mode-1 weights.
//
// wino3d_kernel<FL, MODE>: FL = the epilogue (compile-time flags, -1 = run-time a.flags), MODE = 0 plain | 2 pooled adjoint | 3 up-sampling-aware
// forward with the coarse halo block staged.  The library instantiates the 12 pairs listed in wino_launch below, nothing else.
//
// The kernel is one fp32 path: a chunk is staged by buffer loads (offsets: set_offs) and stage_store_all into one of two alternating LDS buffers,
// raw_read + transform make the A operands of a k-step, reload_row fetches a xi_y row's weights behind its MFMAs.  (History: until commit
// 2f63d5b it also carried the experiments of rounds 2-5 as template switches DBG / PREC / XS; what they were, their numbers and how they
// were removed is in profiles/LAB_NOTES.md, "Winograd 3-D convs: experiment switches ..." and "wino3d_kernel: the dead DBG / PREC / XS paths".)
#include <type_traits>
#include "df_common.hpp"
#include "conv_args.hpp"

namespace {

using df::ceil_div;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kT = 512;                   // 8 waves: (xi_z, tile z-row)
constexpr int kPackT = 256;
constexpr int CKW = 16;                   // input channels per LDS chunk (4 k-steps)
constexpr int PY = 12, PZ = 144;          // LDS pitches (dwords) of a channel plane: 6 z x 10 y x 10 x, padded
constexpr int CP = 866;                   // dwords per channel plane (6*144 = 864, +2: staging writes spread over banks)
constexpr int HY = 10, HX = 10, HV = 600; // halo block 6 x 10 x 10
constexpr int NLOAD = 5;                  // ceil(600 * 4 float4 pieces / 512 threads)
// MODE 3 (round 5): the up-sampling-aware forward stages the COARSE halo block itself -- 4 x 6 x 6 coarse voxels instead of the 6 x 10 x 10
// fine positions that repeat them (4.2x fewer staging loads) -- and builds the 27 live transform points from the 3 x 3 coarse patch per
// plane a tile sees.  A coarse row (pz, py) of a channel is stored as FOUR 16-byte windows, window t = (c[t], c[t+1], c[t+2], -) = the three
// columns tile column tx = t needs, so a lane fetches a patch row with ONE aligned ds_read_b128 (the 16 (ty, tx) lanes of a channel read 64
// consecutive dwords: conflict-free).  Staging is by WINDOW: thread = (window t of row (pz, py), channel quad) loads the three coarse voxels
// px = t, t+1, t+2 (16 bytes = its 4 channels each; neighbours' loads hit the same lines) and writes its four channels' windows with four
// ds_write_b128 (16 lanes = 4 quads x 4 windows cover 64 banks: conflict-free): 4 x 6 x 4 windows x 4 quads = 384 threads (waves 0-5).
// (First version: every thread staged one voxel and scattered it to its <= 3 windows with 12 ds_write_b32 -- all lanes of an instruction on
//  banks = k (mod 4), >= 4-way conflicts, 10 % of the kernel; profiles/r05_probes.md.)
constexpr int UPY = 16, UPZ = 6 * UPY, UCP = 4 * UPZ + 4;
constexpr int UWIN = 4 * 6 * 4;           // windows of the coarse halo block: 4 planes x 6 rows x 4 windows
constexpr int NLU = 2;                    // loads per staging thread: the window's outer voxels t and t + 2; the middle one comes from the
                                          // neighbouring window's thread by DPP (the 16 lanes of a DPP row = 4 quads x the 4 windows of a row)
// internal epilogue flags (beyond the public DF_CONV_*), part of the compile-time FL of the specialised instantiations:
//   kSignBits: also emit the sign pattern of the output, one byte per lane and cout block holding the signs of the lane's 8 outputs
//              (what a later masked dgrad of the same geometry needs of it: 1/32 of the activation's bytes);
//   kMaskBits: DF_CONV_MASK reads those bytes (2 byte loads per lane and tile block) instead of 16 fp32 activations per lane.
constexpr int kSignBits = 64, kMaskBits = 128;
constexpr int kNoPrimary = 256;            // with DF_CONV_ADDUP + kSignBits: y (the pre-add activation) is NOT written -- its sign bits are all
                                           // the backward pass needs of it (df_wino_conv_fwd_addup_bits / df_lrelu_bits_bwd_pool2x)
constexpr int kBitBytesPerBlock = 1024;    // 8 waves x 2 cout blocks x 64 lanes, per (tile block, cout slice)
constexpr int kZeroFloats = 1024;         // zeroed tail of the packed weights: SAME padding reads it, one 64-byte step per chunk

struct WinoArgs {
  const float* x;
  const f32x4* wp;
  const float* zeros;
  const float* bias;
  const float* residual;
  const float* mask_src;
  float* y;
  float* y2;           // DF_CONV_ADDUP: second output  y2 = y + nearest_up2x(residual)  (residual = the COARSE tensor)
  unsigned char* bits_out;        // kSignBits: sign pattern of y, one byte per (tile block, cout slice, wave, cout block, lane): bit s = output s
  const unsigned char* bits_in;   // kMaskBits: the lrelu mask of DF_CONV_MASK as such bytes instead of mask_src
  int B, D, H, W, Cin, Cout;
  int nbz, nby, nbx, ntb, ncs;
  int flags;
  float leak;
  int spx;             // cout slices per XCD (wino_grid)
  int reserved = 0;    // padding that keeps the argument block at its size: always zero, never read
};

// ---- weight transform + packing ------------------------------------------------------------------------------------------
// mode 0: g[tap][k][n] = w[tap][k][n]          (K = cin,  N = cout)
// mode 1: g[tap][k][n] = w[26 - tap][n][k]     (K = cout, N = cin; taps mirrored)  -> dgrad operand
// Up[cs][xz][k4][nb][xy][kq][j][xx] = sum_taps G[xz][tz] G[xy][ty] G[xx][tx] g[tap][4 k4 + kq][32 cs + 16 nb + j]
// thread = one (k, n) filter: its 27 taps are read once and all 64 transform points come out of the separable G transform in fp64
// (3 -> 4 points per axis), written as 16 float4 (the four xi_x of a (xi_z, xi_y)); the float4 of consecutive n are contiguous.
__global__ __launch_bounds__(kPackT) void wino_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int cin, int cout,
                                                           int mode, int64_t total) {
  const int K = mode == 0 ? cin : cout, N = mode == 0 ? cout : cin;
  const int64_t nfil = static_cast<int64_t>(K) * N;
  for (int64_t f = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; f < nfil; f += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int n = static_cast<int>(f % N), k = static_cast<int>(f / N);
    double g[27];
#pragma unroll
    for (int tap = 0; tap < 27; ++tap)
      g[tap] = static_cast<double>(mode == 0 ? w[(static_cast<int64_t>(tap) * cin + k) * cout + n]
                                             : w[(static_cast<int64_t>(26 - tap) * cin + n) * cout + k]);
    // x: [tz][ty][3] -> [tz][ty][4]
    double gx[9][4];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      const double a = g[r * 3], b = g[r * 3 + 1], c = g[r * 3 + 2];
      gx[r][0] = a; gx[r][1] = 0.5 * (a + b + c); gx[r][2] = 0.5 * (a - b + c); gx[r][3] = c;
    }
    const int cs = n >> 5, nb = (n >> 4) & 1, j = n & 15, k4 = k >> 2, kq = k & 3;
#pragma unroll
    for (int xz = 0; xz < 4; ++xz) {
      double gz[3][4];      // z combined: [ty][xx]
#pragma unroll
      for (int ty = 0; ty < 3; ++ty)
#pragma unroll
        for (int xx = 0; xx < 4; ++xx) {
          const double a = gx[ty][xx], b = gx[3 + ty][xx], c = gx[6 + ty][xx];
          gz[ty][xx] = xz == 0 ? a : xz == 3 ? c : xz == 1 ? 0.5 * (a + b + c) : 0.5 * (a - b + c);
        }
#pragma unroll
      for (int xy = 0; xy < 4; ++xy) {
        f32x4 o;
#pragma unroll
        for (int xx = 0; xx < 4; ++xx) {
          const double a = gz[0][xx], b = gz[1][xx], c = gz[2][xx];
          o[xx] = static_cast<float>(xy == 0 ? a : xy == 3 ? c : xy == 1 ? 0.5 * (a + b + c) : 0.5 * (a - b + c));
        }
        const int64_t idx = ((((((static_cast<int64_t>(cs) * 4 + xz) * (K / 4) + k4) * 2 + nb) * 4 + xy) * 4 + kq) * 16 + j) * 4;
        *reinterpret_cast<f32x4*>(wp + idx) = o;
      }
    }
  }
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < kZeroFloats; i += static_cast<int64_t>(gridDim.x) * blockDim.x)
    wp[total + i] = 0.f;
}

// ---- packed-fp32 helpers (VOP3P): one instruction = two lanes of the separable B^T transform --------------------------------
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) {
  f32x2 d;
  asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ f32x2 pk_add(f32x2 a, f32x2 b) {
  f32x2 d;
  asm("v_pk_add_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) {
  f32x2 d;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
// P = (x0,x1), Q = (x2,x3):  (x0 - x2, x1 + x2)
__device__ __forceinline__ f32x2 pk_bt01(f32x2 p, f32x2 q) {
  f32x2 d;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,0]" : "=v"(d) : "v"(p), "v"(q));
  return d;
}
// (x2 - x1, x1 - x3)
__device__ __forceinline__ f32x2 pk_bt23(f32x2 p, f32x2 q) {
  f32x2 d;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1] neg_lo:[1,0] neg_hi:[0,1]" : "=v"(d) : "v"(p), "v"(q));
  return d;
}

// MODE 3 x stage on a coarse row (c0, c1 | c2, -):  P = (c0, c1) -> (c0 - c1, c1 + c1);  P, Q = (c2, -) -> (-, c1 - c2).  Packed results on
// purpose: a single-register temporary gets allocated into the never-read xi_x = 2 word of a weight quad whose load is still in flight
// (27-point modes), and its write then waits on vmcnt.
__device__ __forceinline__ f32x2 pk_x01(f32x2 p) {
  f32x2 d;
  asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,0]" : "=v"(d) : "v"(p));
  return d;
}
__device__ __forceinline__ f32x2 pk_x3(f32x2 p, f32x2 q) {
  f32x2 d;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0] neg_lo:[0,0] neg_hi:[0,1]" : "=v"(d) : "v"(p), "v"(q));
  return d;
}

struct BlockInfo {
  const float* xb;     // &x[b][0][0][0][0]
  int hoff;            // element offset of the block's halo origin (z0-1, y0-1, x0-1) inside the batch volume (may be < 0)
  int b, z0, y0, x0;
  int id;              // tile block index (for the sign-bit words)
};

// raw buffer descriptor (gfx9 data format word): out-of-range offsets read as zero -- the SAME padding of the staging loads
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_srd(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 buf_load16(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

// Barrier that orders LDS traffic only.  __syncthreads() is a full fence: its s_waitcnt vmcnt(0) also waits for the acknowledgement of
// every global STORE issued before it -- in the epilogue that exposed two HBM write round trips per tile block.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// FL >= 0: the epilogue flags are the compile-time constant FL (no per-element flag tests); FL < 0: run-time a.flags
// UPC (MODE 3): the input is the COARSE tensor of an up-sampling-aware conv (x = nearest_up2x(xc) is never materialised): the staging reads
// xc[g >> 1] for fine halo coordinate g, and because every 2x2x2 tile then sees each coarse value twice, the transform points with
// index 2 in any axis are identically zero (B^T d = (c-1 - c0, 2 c0, 0, c0 - c1)): only 27 of the 64 points are multiplied
// (no wave takes xi_z = 2 and the xi_y|xi_x = 2 MFMAs are skipped) -- the 27-product form of the parity-class convolution.
// POOL (MODE 2): the adjoint case -- the output is the 2x2x2 sum-pool of the convolution (d/d(xc) of the up-sampling-aware conv: x is
// the fine gradient, y the COARSE tensor [B, D/2, H/2, W/2, Cout], accumulated into).  The pooled inverse transform is
// (A^T row 0 + row 1) = (1, 2, 0, -1) per axis, so the same 27 points are the only ones needed and a tile block writes 32 voxels, not 256.
template <int FL, int MODE>
__global__ __launch_bounds__(kT, 1) void wino3d_kernel(const WinoArgs a) {
  constexpr bool UPC = MODE == 3;                    // UP with the coarse halo block staged as such (see UPY / UCP above)
  constexpr bool POOL = MODE == 2, P27 = MODE != 0;
  constexpr int PZk = UPC ? UPZ : PZ, CPk = UPC ? UCP : CP;      // pitches INSIDE a buffer; the buffer stride below keeps the plain size (the
                                                                // epilogue's 32 KB exchange area lives in the idle buffer)
  constexpr int NL = UPC ? NLU : NLOAD;              // staging pieces per thread and chunk
  constexpr int BUFF = CKW * CP;                     // floats per LDS buffer
  __shared__ __attribute__((aligned(16))) float sIn[2 * BUFF];
  __shared__ float sBias[32];        // this worker's cout slice of the bias (the slice is fixed for the worker's whole life)
  __shared__ float sMs[16 * kT];     // lrelu-mask operands of a tile block's outputs, fetched by LDS-DMA loads (no registers)

  const int eflags = FL >= 0 ? FL : a.flags;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int xz = wave & 3, th = wave >> 2;      // xi_z; tile z-row
  const int tl = lane & 15, kq = lane >> 4;     // tile within the row block (ty = tl >> 2, tx = tl & 3); cin % 4

  // ---- persistent worker -> (cout slice, sequence of tile blocks) ------------------------------------------------------------
  // Workgroup g runs on XCD g % 8.  When the slice count divides 8 an XCD only ever sees ONE slice (its 1 MB of transformed
  // weights stays L2-resident), its 32 workers walk 32 neighbouring tile blocks at a time (shared halos hit the L2) and the
  // other slices of those blocks run at the same time on the neighbouring XCDs (Infinity Cache serves the repeats).
  int cs, tb, tstride;
  {
    const int g = blockIdx.x, G = gridDim.x;
    if ((8 % a.ncs) == 0 && (G & 7) == 0) {
      // spx slices per XCD (spx | ncs): the XCD's weights are spx MB, and the spx workgroups of a tile block that share its L2
      // run at the same time on neighbouring CUs, so that block's input is fetched from the fabric once per XCD, not per slice
      const int spx = a.spx, xpg = a.ncs / spx;            // XCDs per group (a group covers all slices of its tile blocks)
      const int xcd = g & 7, slot = g >> 3, wx = G >> 3;   // wx workers per XCD
      const int ngroups = 8 / xpg, tw = wx / spx;          // tile workers per XCD
      cs = (xcd % xpg) * spx + slot % spx;
      tb = (xcd / xpg) * tw + slot / spx;
      tstride = ngroups * tw;
      if (slot / spx >= tw) return;
    } else {
      const int nw = G / a.ncs;
      cs = g % a.ncs;
      tb = g / a.ncs;
      tstride = nw;
      if (tb >= nw) return;
    }
  }
  if (tb >= a.ntb) return;
  const int n0 = cs * 32;
  if (tid < 32) sBias[tid] = (eflags & DF_CONV_BIAS) ? a.bias[n0 + tid] : 0.f;      // visible after the prologue's barrier
  const int tb0 = tb;
  const int niter = (a.ntb - tb0 + tstride - 1) / tstride;
  auto seq = [&](int k) -> int { return tb0 + k * tstride; };

  auto decode = [&](int t) -> BlockInfo {
    BlockInfo bi;
    bi.id = t;
    const int bx = t % a.nbx;
    int t2 = t / a.nbx;
    const int by = t2 % a.nby; t2 /= a.nby;
    const int bz = t2 % a.nbz;
    bi.b = t2 / a.nbz;
    bi.z0 = bz * 4; bi.y0 = by * 8; bi.x0 = bx * 8;
    bi.xb = a.x + static_cast<int64_t>(bi.b) * (UPC ? (a.D >> 1) * (a.H >> 1) * (a.W >> 1) : a.D * a.H * a.W) * a.Cin;
    bi.hoff = (((bi.z0 - 1) * a.H + (bi.y0 - 1)) * a.W + (bi.x0 - 1)) * a.Cin;
    return bi;
  };

  // ---- staging plan (per thread: 5 float4 pieces of the 600-voxel x 16-channel halo block) ---------------------------------
  // so[it] = byte offset of piece `it` inside the batch volume, or an out-of-range offset for halo voxels outside the tensor:
  // the buffer load's range check then returns the zeros of the SAME padding.  Set once per tile block; a staging pass adds
  // only the chunk's scalar offset.
  int ldst[NLOAD];
  unsigned so[NLOAD];
#pragma unroll
  for (int it = 0; it < NL; ++it) {
    int p = it * kT + tid;
    if (UPC) {      // thread tid < 384 = (window w = tid >> 2, channel quad tid & 3); the three loads share one LDS destination (its window)
      const int wq = tid < UWIN * 4 ? tid : UWIN * 4 - 1, q4 = wq & 3, w = wq >> 2;
      const int t = w & 3, py = (w >> 2) % 6, pz = w / 24;
      ldst[it] = ((q4 * 4) * UCP + pz * UPZ + py * UPY + t * 4) * 4;
      continue;
    }
    if (p > HV * 4 - 1) p = HV * 4 - 1;     // the tail threads of the last pass duplicate the last piece (same data, same slot)
    const int hv = p >> 2, q4 = p & 3;
    const int hx = hv % HX, hy = (hv / HX) % HY, hz = hv / (HX * HY);
    ldst[it] = ((q4 * 4) * CPk + hz * PZk + hy * PY + hx) * 4;        // bytes, buffer 0
  }
  // pass `it` of the staging is taken by every wave, except the coarse block's second pass (64 pieces: wave 0) -- wave-uniform
  auto stage_pass = [&](int) -> bool { return !UPC || wave < UWIN * 4 / 64; };      // MODE 3: waves 0-5 stage (wave-uniform)
  const unsigned vol_bytes = static_cast<unsigned>(UPC ? (a.D >> 1) * (a.H >> 1) * (a.W >> 1) : a.D * a.H * a.W) * a.Cin * 4u;
  auto set_offs = [&](const BlockInfo& bi) {
    // [r6] opaque thread id: LLVM otherwise hoists the five pieces' (hz, hy, hx, roff) out of the block loop -- 20 registers that it then spills
    // (37-56 spilled VGPRs in the plain instantiations, 15 in the pooled adjoint), and the reloads sit in the main loop behind `s_waitcnt vmcnt(0)`
    int tido = tid;
    asm volatile("" : "+v"(tido));
#pragma unroll
    for (int it = 0; it < NL; ++it) {
      int p = it * kT + tido;
      if (UPC) {      // coarse voxel (pz, py, px = t + it) of the 4 x 6 x 6 block whose origin is the coarse voxel under fine (z0 - 1, y0 - 1, x0 - 1)
        const int wq = tid < UWIN * 4 ? tid : UWIN * 4 - 1, q4 = wq & 3, w = wq >> 2;
        const int px = (w & 3) + 2 * it, py = (w >> 2) % 6, pz = w / 24;
        const int Dc = a.D >> 1, Hc = a.H >> 1, Wc = a.W >> 1;
        const int cz = (bi.z0 >> 1) - 1 + pz, cy = (bi.y0 >> 1) - 1 + py, cx = (bi.x0 >> 1) - 1 + px;
        const bool ok = static_cast<unsigned>(cz) < static_cast<unsigned>(Dc) && static_cast<unsigned>(cy) < static_cast<unsigned>(Hc) &&
                  static_cast<unsigned>(cx) < static_cast<unsigned>(Wc);      // fine g in range <=> coarse g >> 1 in range (even extents)
        so[it] = ok ? static_cast<unsigned>(((cz * Hc + cy) * Wc + cx) * a.Cin + q4 * 4) * 4u : 0x80000000u;
        continue;
      }
      if (p > HV * 4 - 1) p = HV * 4 - 1;
      const int hv = p >> 2, q4 = p & 3;
      const int hx = hv % HX, hy = (hv / HX) % HY, hz = hv / (HX * HY);
      const int roff = ((hz * a.H + hy) * a.W + hx) * a.Cin + q4 * 4;
      const int gz = bi.z0 - 1 + hz, gy = bi.y0 - 1 + hy, gx = bi.x0 - 1 + hx;
      const bool ok = static_cast<unsigned>(gz) < static_cast<unsigned>(a.D) && static_cast<unsigned>(gy) < static_cast<unsigned>(a.H) &&
                static_cast<unsigned>(gx) < static_cast<unsigned>(a.W);
      so[it] = ok ? static_cast<unsigned>(bi.hoff + roff) * 4u : 0x80000000u;
    }
  };
  char* sInB = reinterpret_cast<char*>(sIn);
  auto stage_store = [&](int it, int bufbytes, const f32x4& v) {
    float* d = reinterpret_cast<float*>(sInB + (ldst[it] + bufbytes));
    d[0] = v[0]; d[CPk] = v[1]; d[2 * CPk] = v[2]; d[3 * CPk] = v[3];
  };
  // all pieces of a thread; MODE 3: the three loaded voxels (c0, c1, c2) x 4 channels -> the window (c0, c1, c2, -) of each channel
  auto stage_store_all = [&](int bufbytes, const auto& v) {
    if constexpr (UPC) {
      if (!stage_pass(0)) return;
      char* d = sInB + (ldst[0] + bufbytes);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // lane = quad + 4 t inside a 16-lane DPP row: voxel t + 1 = first voxel of lane + 4 (row_shl:4); lanes 12-15 (t = 3) have no lane + 4 and
        // keep `old` = the second voxel (t + 2 = 4) of lane - 4 (row_shr:4)
        const float f0 = v[0][e], f2 = v[1][e];      // (bit_cast of a vector-ELEMENT lvalue reads element 0: copy to scalars first)
        const int c0 = __builtin_bit_cast(int, f0), c2 = __builtin_bit_cast(int, f2);
        const int fromlo = __builtin_amdgcn_update_dpp(0, c2, 0x114, 0xF, 0xF, false);            // row_shr:4
        const int c1 = __builtin_amdgcn_update_dpp(fromlo, c0, 0x104, 0xF, 0xF, false);           // row_shl:4, out-of-row lanes keep fromlo
        *reinterpret_cast<f32x4*>(d + e * UCP * 4) = f32x4{v[0][e], __builtin_bit_cast(float, c1), v[1][e], 0.f};
      }
    } else {
#pragma unroll
      for (int it = 0; it < NLOAD; ++it) stage_store(it, bufbytes, v[it]);
    }
  };

  // ---- A operand: this lane's tile, planes (za, zb) of xi_z ---------------------------------------------------------------
  const int tx = tl & 3, ty = tl >> 2;
  // main-loop role (mz = xi_z, mth = tile z-row).  Plain conv: the wave's (xz, th).  27-point modes: only xi_z in {0, 1, 3} is
  // multiplied, 6 (xi_z, z-row) roles of 2 x 9 MFMAs per k-step: waves 0-3 take (xi_z in {0, 1}) x (z-row) with both 16-cout blocks,
  // waves 4-7 split the two xi_z = 3 roles by cout block (hnb) -- every SIMD (wave & 3) then issues 27 MFMAs per k-step.
  const bool half = P27 && wave >= 4;
  const int mz = !P27 ? xz : (wave < 4 ? (wave >> 1) : 3);
  const int mth = !P27 ? th : (wave < 4 ? (wave & 1) : ((wave >> 1) & 1));
  const int hnb = half ? (wave & 1) : 0;
  const int za = mz == 0 ? 0 : mz == 2 ? 2 : 1;
  const int zb = mz == 0 ? 2 : mz == 1 ? 2 : mz == 2 ? 1 : 3;
  const float qs = mz == 1 ? 1.f : -1.f;
  const f32x2 qs2 = {qs, qs};
  const int abase = kq * CPk + (2 * mth) * PZk + (2 * ty) * PY + 2 * tx;
  const int offA = abase + za * PZk, offB = abase + zb * PZk;

  // MODE 3: the tile's fine planes 2 mth + {0..3} repeat the coarse planes mth + {0, 1, 1, 2} (fine halo index h <-> coarse (h + 1) >> 1), its
  // fine rows / columns the coarse rows ty + {0, 1, 1, 2} / columns tx + {0, 1, 1, 2}: the lane reads the 3 x 3 patch of the two coarse planes
  // its xi_z combines and applies the SAME operations to the same values as the fine-grid transform (bit-identical operands):
  //   per axis  (d0 - d2, d1 + d2, -, d1 - d3)  with  d = (c0, c1, c1, c2)   ->   (c0 - c1, c1 + c1, -, c1 - c2)
  const int uoffA = (kq * UCP + (mth + ((za + 1) >> 1)) * UPZ + ty * UPY + tx * 4) * 4;      // bytes: window tx of coarse row ty
  const int uoffB = (kq * UCP + (mth + ((zb + 1) >> 1)) * UPZ + ty * UPY + tx * 4) * 4;
  f32x4 ua[3], ub[3];      // [coarse row]: (c0, c1, c2, -)
  f32x2 ra[8], rb[8];      // raw inputs [y][x pair] of planes za / zb
  f32x2 T[8], U[8];        // after the z / y transform
  f32x2 A2[8];             // A operands of a k-step: A2[xi_y*2 + h] = (xi_x = 2h, 2h+1)
  const int offAb = offA * 4, offBb = offB * 4;      // bytes (multiples of 8)
  auto raw_read_up = [&](int idxbytes) {      // idxbytes: LDS byte offset of channel plane 4 ks (+ buffer)
    int ia = idxbytes + uoffA, ib = idxbytes + uoffB;
    asm volatile("" : "+v"(ia), "+v"(ib));
    __builtin_assume((ia & 15) == 0);
    __builtin_assume((ib & 15) == 0);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      ua[r] = *reinterpret_cast<const f32x4*>(sInB + ia + r * UPY * 4);
      ub[r] = *reinterpret_cast<const f32x4*>(sInB + ib + r * UPY * 4);
    }
  };
  auto raw_read = [&](int idxbytes) {   // idxbytes: LDS byte offset of plane 4 ks (+ buffer), without this lane's offset
    if constexpr (UPC) { raw_read_up(idxbytes); return; }
    int ia = idxbytes + offAb, ib = idxbytes + offBb;
    asm volatile("" : "+v"(ia), "+v"(ib));     // opaque: the 16 row reads become 8 ds_read2_b64 with small immediate offsets
    __builtin_assume((ia & 7) == 0);
    __builtin_assume((ib & 7) == 0);
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      ra[y * 2 + 0] = *reinterpret_cast<const f32x2*>(sInB + ia + (y * PY) * 4);
      ra[y * 2 + 1] = *reinterpret_cast<const f32x2*>(sInB + ia + (y * PY + 2) * 4);
      rb[y * 2 + 0] = *reinterpret_cast<const f32x2*>(sInB + ib + (y * PY) * 4);
      rb[y * 2 + 1] = *reinterpret_cast<const f32x2*>(sInB + ib + (y * PY + 2) * 4);
    }
  };
  auto transform_up = [&]() {
    f32x2 tl2[3], th2[3];      // z: rows as (c0, c1) and (c2, -)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      tl2[r] = pk_fma(f32x2{ub[r][0], ub[r][1]}, qs2, f32x2{ua[r][0], ua[r][1]});
      th2[r] = pk_fma(f32x2{ub[r][2], ub[r][3]}, qs2, f32x2{ua[r][2], ua[r][3]});
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k == 2) { A2[4] = f32x2{0.f, 0.f}; A2[5] = f32x2{0.f, 0.f}; continue; }      // xi_y = 2 is never multiplied
      const f32x2 ul = k == 0 ? pk_sub(tl2[0], tl2[1]) : k == 1 ? pk_add(tl2[1], tl2[1]) : pk_sub(tl2[1], tl2[2]);      // y
      const f32x2 uh = k == 0 ? pk_sub(th2[0], th2[1]) : k == 1 ? pk_add(th2[1], th2[1]) : pk_sub(th2[1], th2[2]);
      A2[k * 2 + 0] = pk_x01(ul);                                                       // x: xi_x = 0, 1: (c0 - c1, c1 + c1)
      A2[k * 2 + 1] = pk_x3(ul, uh);                                                    // xi_x = (2), 3: (-, c1 - c2)
    }
  };
  auto transform = [&]() {
    if constexpr (UPC) { transform_up(); return; }
#pragma unroll
    for (int j = 0; j < 8; ++j) T[j] = pk_fma(rb[j], qs2, ra[j]);          // z
#pragma unroll
    for (int h = 0; h < 2; ++h) {                                           // y
      U[0 + h] = pk_sub(T[0 + h], T[4 + h]);
      U[2 + h] = pk_add(T[2 + h], T[4 + h]);
      U[4 + h] = pk_sub(T[4 + h], T[2 + h]);
      U[6 + h] = pk_sub(T[2 + h], T[6 + h]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                           // x
      A2[k * 2 + 0] = pk_bt01(U[k * 2], U[k * 2 + 1]);
      A2[k * 2 + 1] = pk_bt23(U[k * 2], U[k * 2 + 1]);
    }
  };

  // ---- B operand ------------------------------------------------------------------------------------------------------------
  const int nk4 = a.Cin >> 2;
  f32x4 bq[2][4];          // [cout 16-block][xi_y] = (xi_x 0..3)
  const unsigned laneb = static_cast<unsigned>(lane) * 16u;
  const __amdgpu_buffer_rsrc_t wsrd = make_srd(a.wp, static_cast<unsigned>(a.Cin) * a.Cout * 256u);
  const unsigned wbase_b = static_cast<unsigned>((cs * 4 + mz) * nk4) * 8192u + static_cast<unsigned>(hnb) * 4096u;
  auto issue_bq = [&](int nb, int k4) {
    const int kl = k4 < nk4 ? k4 : 0;        // wraps to the first k-step of the next tile block
    const unsigned sb = wbase_b + static_cast<unsigned>(kl) * 8192u + nb * 4096u;      // wave-uniform
#pragma unroll
    for (int q = 0; q < 4; ++q) bq[nb][q] = buf_load16(wsrd, laneb + q * 1024u, sb);
  };

  f32x4 acc[2][16];
  const int nchunk = a.Cin / CKW;

  // ---- prologue: first block's chunk 0 -> buffer 0 ------------------------------------------------------------------------------
  BlockInfo cur = decode(seq(0));
  {
    set_offs(cur);
    const __amdgpu_buffer_rsrc_t srd0 = make_srd(cur.xb, vol_bytes);
    f32x4 stg[NLOAD];
#pragma unroll
    for (int it = 0; it < NL; ++it) if (stage_pass(it)) stg[it] = buf_load16(srd0, so[it], 0u);
    stage_store_all(0, stg);
  }
  __syncthreads();

  int pb = 0;          // buffer parity of the block's chunk 0
  for (int it = 0; it < niter; ++it) {
    const BlockInfo nxt = decode(seq(it + 1 < niter ? it + 1 : it));
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[nb][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    // first raw inputs of this block (and, for the worker's first block, the weights of k-step 0)
    raw_read(pb * BUFF * 4);
    // [r3] the weights of k-step 0 are the same for every tile block of the worker and the last k-step of a block has already reloaded
    // them (issue_bq / reload_row wrap around): they stay in their registers across the epilogue (16.13 -> 16.05 ms per top-level
    // launch; tuning variant 65536 = reloaded at every block start)
    if (it == 0) {
      issue_bq(0, 0);
      if (!half) issue_bq(1, 0);
    }

    // The 16 lrelu-mask operands of this lane's outputs go global -> LDS by DMA loads (in registers hipcc spills each one to scratch
    // behind its own vmcnt(0): 14 serial HBM round trips).  Issued at the top of the epilogue and read back after the first combine
    // (issuing them inside the last chunk costs more than it hides: +20 % kernel time); every thread reads only what it requested.
    auto mask_dma = [&]() {
      typedef __attribute__((address_space(3))) void* lds_ptr;
      const int oz0 = cur.z0 + 2 * th, oy0 = cur.y0 + 2 * kq, ox0 = cur.x0 + 2 * xz;
      const int sW = a.Cout, sH = a.W * a.Cout, sD = sH * a.H;
      const __amdgpu_buffer_rsrc_t msrd = make_srd(a.mask_src + static_cast<int64_t>(cur.b) * a.D * a.H * a.W * a.Cout,
                                                   static_cast<unsigned>(a.D) * a.H * a.W * a.Cout * 4u);
      const unsigned mv = static_cast<unsigned>(((oz0 * a.H + oy0) * a.W + ox0) * a.Cout + n0 + tl) * 4u;
#pragma unroll
      for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const unsigned so_ = static_cast<unsigned>(n2 * 16 + (s >> 2) * sD + ((s >> 1) & 1) * sH + (s & 1) * sW) * 4u;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(msrd, (lds_ptr)(sMs + (n2 * 8 + s) * kT + wave * 64), 4, mv, so_, 0, 0);
        }
    };
    auto main_loop = [&](auto half_c) {
    constexpr bool HALF = decltype(half_c)::value;      // this wave owns one 16-cout block only (acc[0], weights of block hnb)
    for (int chunk = 0; chunk < nchunk; ++chunk) {
      const int bo = ((chunk + pb) & 1) * BUFF * 4, bn = BUFF * 4 - bo;      // byte offsets of this / the next chunk's buffer
      const bool lastc = chunk + 1 == nchunk;
      if (lastc) set_offs(nxt);                    // the last chunk stages the next tile block's first chunk
      const __amdgpu_buffer_rsrc_t ssrd = make_srd(lastc ? nxt.xb : cur.xb, vol_bytes);
      const unsigned schunk = static_cast<unsigned>(lastc ? 0 : chunk + 1) * (CKW * 4u);
      f32x4 stg[NLOAD];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        // -- A operands of this k-step (its raw inputs were requested during the previous one) --
        transform();
        __builtin_amdgcn_sched_barrier(0);
        if (ks == 2) {
          stage_store_all(bn, stg);
        }
        // next chunk staged by everyone; everyone is done reading the planes it overwrote.  [r3] An LDS-only barrier: the staged data was
        // already waited for at the LDS writes of ks == 2, and __syncthreads()' vmcnt(0) drained the weight loads in flight (this and the
        // two epilogue barriers: 16.21 -> 16.05 ms per top-level launch, round 3)
        if (ks == 3) lds_barrier();
        raw_read(ks < 3 ? bo + (ks + 1) * 16 * CPk : bn);      // raw inputs of the next k-step
        __builtin_amdgcn_sched_barrier(0);
        // [r3] a xi_y row's weight registers are reloaded right after its 4 MFMAs, not after the cout block's 16: every weight load is in
        // flight up to 12 MFMAs longer before the next k-step needs it (16.52 -> 16.27 ms per top-level launch; tuning variant 196608 = the
        // old order)
        auto reload_row = [&](int nb, int q) {
          if (P27 && q == 2) return;
          const int k4 = chunk * 4 + ks + 1;
          const int kl = k4 < nk4 ? k4 : k4 - nk4;      // wraps to the first k-step(s) of the next tile block
          const unsigned sb = wbase_b + static_cast<unsigned>(kl) * 8192u + nb * 4096u;
          bq[nb][q] = buf_load16(wsrd, laneb + q * 1024u, sb);
        };
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if (!P27 || ((i >> 2) != 2 && (i & 3) != 2))
            acc[0][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(A2[i >> 1][i & 1], bq[0][i >> 2][i & 3], acc[0][i], 0, 0, 0);
          if ((i & 3) == 3) {
            __builtin_amdgcn_sched_barrier(0);
            reload_row(0, i >> 2);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_sched_barrier(0);
        if (!HALF) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            if (!P27 || ((i >> 2) != 2 && (i & 3) != 2))
              acc[1][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(A2[i >> 1][i & 1], bq[1][i >> 2][i & 3], acc[1][i], 0, 0, 0);
            if ((i & 3) == 3) {
              __builtin_amdgcn_sched_barrier(0);
              reload_row(1, i >> 2);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        if (ks == 0) {     // staging loads of the next chunk, right behind a weight batch: vmcnt retires in order, so
                                         // the first wait that covers them is the one for the NEXT weight batch (1.5 k-steps away)
#pragma unroll
          for (int it = 0; it < NL; ++it)
            if (stage_pass(it)) stg[it] = buf_load16(ssrd, so[it], schunk);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    };
    if (half) main_loop(std::true_type{}); else main_loop(std::false_type{});

    // ---- epilogue: inverse transform in x, y per accumulator element; z across the waves through the idle LDS buffer ---------
    // (the buffer of the last chunk is free since that chunk's barrier; the other one holds the next block's chunk 0)
    if constexpr (POOL) {
      const int lb = ((nchunk - 1 + pb) & 1) * BUFF;
      float* sP = sIn + lb;      // [xi_z][tz][e][lane]: the (y, x)-pooled value of accumulator element e
      const int Dc = a.D >> 1, Hc = a.H >> 1, Wc = a.W >> 1;
      const int cz = (cur.z0 >> 1) + th, cy = (cur.y0 >> 1) + kq, cx = (cur.x0 >> 1) + xz;      // this wave combines e = xz of its z-row
      const bool inb = cz < Dc && cy < Hc && cx < Wc;
      float* yo = a.y + (((static_cast<int64_t>(cur.b) * Dc + cz) * Hc + cy) * Wc + cx) * a.Cout + n0 + tl;
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const float prev = inb ? yo[nb * 16] : 0.f;
        auto emit = [&](const f32x4 (&c)[16]) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float py[4];
#pragma unroll
            for (int yy = 0; yy < 4; ++yy)
              py[yy] = yy == 2 ? 0.f : c[yy * 4 + 0][e] + 2.f * c[yy * 4 + 1][e] - c[yy * 4 + 3][e];
            sP[((mz * 2 + mth) * 4 + e) * 64 + lane] = py[0] + 2.f * py[1] - py[3];
          }
        };
        if (!half) emit(acc[nb]);
        else if (nb == hnb) emit(acc[0]);
        lds_barrier();
        const float m0 = sP[((0 * 2 + th) * 4 + xz) * 64 + lane], m1 = sP[((1 * 2 + th) * 4 + xz) * 64 + lane];
        const float m3 = sP[((3 * 2 + th) * 4 + xz) * 64 + lane];
        if (inb) yo[nb * 16] = prev + (m0 + 2.f * m1 - m3);
        lds_barrier();
      }
    } else {
      const int lb = ((nchunk - 1 + pb) & 1) * BUFF;
      f32x4* sO = reinterpret_cast<f32x4*>(sIn + lb);      // [xi_z][tz][e][lane] float4 = (oy0ox0, oy0ox1, oy1ox0, oy1ox1)
      // this wave combines accumulator element e = xi_z of its own z-row:  tile (ty = lane>>4, tx = e), cout = lane & 15
      const int oz0 = cur.z0 + 2 * th, oy0 = cur.y0 + 2 * kq, ox0 = cur.x0 + 2 * xz;
      const int64_t sW = a.Cout, sH = static_cast<int64_t>(a.W) * a.Cout, sD = sH * a.H;
      const int64_t obase = (((static_cast<int64_t>(cur.b) * a.D + oz0) * a.H + oy0) * a.W + ox0) * a.Cout + n0 + tl;
      const bool full = cur.z0 + 4 <= a.D && cur.y0 + 8 <= a.H && cur.x0 + 8 <= a.W;
      const unsigned lane_off = static_cast<unsigned>(((oz0 * a.H + oy0) * a.W + ox0) * a.Cout + n0 + tl) * 4u;      // bytes within the batch volume
      constexpr bool SB = FL >= 0 && (FL & kSignBits) != 0, MB = FL >= 0 && (FL & kMaskBits) != 0, NOY = FL >= 0 && (FL & kNoPrimary) != 0;
      if (full && (eflags & DF_CONV_MASK) && !MB) mask_dma();
      // the fp32-mask DMA path counts on vmcnt(8) with nothing but its own loads outstanding: keep the draining barriers there
      const bool full_bar = (eflags & DF_CONV_MASK) && !MB;
      const int64_t wbase = (static_cast<int64_t>(cur.id) * a.ncs + cs) * kBitBytesPerBlock + wave * 128 + lane;
      float rres[2][8];
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const float bv = sBias[nb * 16 + tl];
        unsigned mbyte = 0u, sbyte = 0u;      // kMaskBits: this lane's 8 mask bits of the cout block (one byte load, used after the combine)
        if (MB) mbyte = a.bits_in[wbase + nb * 64];
        auto emit = [&](const f32x4 (&c)[16]) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            f32x2 px[4];
#pragma unroll
            for (int yy = 0; yy < 4; ++yy) {
              if (P27) {      // the xi = 2 points were never multiplied
                px[yy][0] = c[yy * 4 + 0][e] + c[yy * 4 + 1][e];
                px[yy][1] = c[yy * 4 + 1][e] - c[yy * 4 + 3][e];
              } else {
                px[yy][0] = c[yy * 4 + 0][e] + c[yy * 4 + 1][e] + c[yy * 4 + 2][e];
                px[yy][1] = c[yy * 4 + 1][e] - c[yy * 4 + 2][e] - c[yy * 4 + 3][e];
              }
            }
            const f32x2 o01 = P27 ? px[0] + px[1] : px[0] + px[1] + px[2], o23 = P27 ? px[1] - px[3] : px[1] - px[2] - px[3];
            sO[((mz * 2 + mth) * 4 + e) * 64 + lane] = f32x4{o01[0], o01[1], o23[0], o23[1]};
          }
        };
        if (!half) emit(acc[nb]);
        else if (nb == hnb) emit(acc[0]);
        if (nb == 0 && full && (eflags & DF_CONV_RESIDUAL)) {
#pragma unroll
          for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
            for (int s = 0; s < 8; ++s)
              rres[n2][s] = a.residual[obase + n2 * 16 + (s >> 2) * sD + ((s >> 1) & 1) * sH + (s & 1) * sW];
        }
        if (full_bar) __syncthreads(); else lds_barrier();      // (the combine below reads LDS only; the residual loads are waited for at their use)
        const f32x4 m0 = sO[((0 * 2 + th) * 4 + xz) * 64 + lane], m1 = sO[((1 * 2 + th) * 4 + xz) * 64 + lane];
        const f32x4 m3 = sO[((3 * 2 + th) * 4 + xz) * 64 + lane];
        f32x4 lo = m0 + m1, hi = m1 - m3;
        if (!P27) {
          const f32x4 m2 = sO[((2 * 2 + th) * 4 + xz) * 64 + lane];
          lo += m2; hi -= m2;
        }
        // mask DMA of THIS cout block landed: the 16 loads were issued block 0 first and vmcnt retires in order, so "at most 8
        // outstanding" covers block 0 while block 1's eight are still in flight, and block 1 while block 0's eight stores are
        if (full && (eflags & DF_CONV_MASK) && !MB) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        float rup = 0.f;      // DF_CONV_ADDUP: the 2x2x2 outputs of this lane's tile share ONE coarse voxel of the skip tensor
        if ((eflags & DF_CONV_ADDUP) && oz0 < a.D && oy0 < a.H && ox0 < a.W)
          rup = a.residual[(((static_cast<int64_t>(cur.b) * (a.D >> 1) + (oz0 >> 1)) * (a.H >> 1) + (oy0 >> 1)) * (a.W >> 1) + (ox0 >> 1)) * a.Cout +
                           n0 + nb * 16 + tl];
        // Full blocks of the variants without a per-output operand (bias / lrelu / sign bits only: the 27-point up-sampling-aware forward and the plain
        // forward): the stores go through the 4 x 4 lane-quad transpose of conv_wino43.hip -- 2 float4 stores per lane and cout block instead of 8 scalar
        // ones; bias, lrelu and the sign bits stay in the accumulator layout (the sign-byte layout is unchanged).  Bit-identical.
        const bool wide = full && !(eflags & (DF_CONV_RESIDUAL | DF_CONV_MASK | DF_CONV_ADDUP)) && !NOY;
        if (wide) {
          f32x4 vz[2];
#pragma unroll
          for (int s = 0; s < 8; ++s) {
            float v = (s < 4 ? lo[s & 3] : hi[s & 3]) + bv;
            if (eflags & DF_CONV_LRELU) v = fmaxf(v, a.leak * v);
            if (SB) sbyte |= v > 0.f ? (1u << s) : 0u;
            vz[s >> 2][s & 3] = v;
          }
          const int qi = tl & 3;
          const bool odd1 = (qi & 1) != 0, odd2 = (qi & 2) != 0;
          auto quad_t = [&](const f32x4& v) -> f32x4 {
            auto dpp1 = [](float x) { return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0xB1, 0xf, 0xf, true)); };
            auto dpp2 = [](float x) { return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x4E, 0xf, 0xf, true)); };
            const float p0 = dpp1(v[0]), p1 = dpp1(v[1]), p2 = dpp1(v[2]), p3 = dpp1(v[3]);
            const f32x4 a1 = {odd1 ? p1 : v[0], odd1 ? v[1] : p0, odd1 ? p3 : v[2], odd1 ? v[3] : p2};
            const float r0 = dpp2(a1[0]), r1 = dpp2(a1[1]), r2 = dpp2(a1[2]), r3 = dpp2(a1[3]);
            return f32x4{odd2 ? r2 : a1[0], odd2 ? r3 : a1[1], odd2 ? a1[2] : r0, odd2 ? a1[3] : r1};
          };
          const int64_t o4 = obase - tl + 4 * (tl >> 2) + nb * 16 + (qi >> 1) * sH + (qi & 1) * sW;
          *reinterpret_cast<f32x4*>(a.y + o4) = quad_t(vz[0]);
          *reinterpret_cast<f32x4*>(a.y + o4 + sD) = quad_t(vz[1]);
        } else
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          float v = (s < 4 ? lo[s & 3] : hi[s & 3]) + bv;
          if (eflags & DF_CONV_LRELU) v = fmaxf(v, a.leak * v);
          const int64_t o = obase + nb * 16 + (s >> 2) * sD + ((s >> 1) & 1) * sH + (s & 1) * sW;
          if (SB) sbyte |= v > 0.f ? (1u << s) : 0u;      // (outputs outside the tensor carry don't-care bits)
          const bool mpos = !MB || ((mbyte >> s) & 1u) != 0u;
          if (full) {
            if (eflags & DF_CONV_RESIDUAL) v += rres[nb][s];
            if (eflags & DF_CONV_MASK) v = (MB ? mpos : sMs[(nb * 8 + s) * kT + tid] > 0.f) ? v : a.leak * v;
            // wave-uniform base (batch volume + this output's scalar offset) + 32-bit lane offset: no 64-bit address per output
            char* yb = reinterpret_cast<char*>(a.y + static_cast<int64_t>(cur.b) * a.D * a.H * a.W * a.Cout +
                                               ((s >> 2) * sD + ((s >> 1) & 1) * sH + (s & 1) * sW) + nb * 16);
            if (!NOY) *reinterpret_cast<float*>(yb + lane_off) = v;
            if (eflags & DF_CONV_ADDUP) {
              char* yb2 = reinterpret_cast<char*>(a.y2 + static_cast<int64_t>(cur.b) * a.D * a.H * a.W * a.Cout +
                                                  ((s >> 2) * sD + ((s >> 1) & 1) * sH + (s & 1) * sW) + nb * 16);
              *reinterpret_cast<float*>(yb2 + lane_off) = v + rup;
            }
          } else if (oz0 + (s >> 2) < a.D && oy0 + ((s >> 1) & 1) < a.H && ox0 + (s & 1) < a.W) {
            if (eflags & DF_CONV_RESIDUAL) v += a.residual[o];
            if (eflags & DF_CONV_MASK) v = (MB ? mpos : a.mask_src[o] > 0.f) ? v : a.leak * v;
            if (!NOY) a.y[o] = v;
            if (eflags & DF_CONV_ADDUP) a.y2[o] = v + rup;
          }
        }
        if (SB) a.bits_out[wbase + nb * 64] = static_cast<unsigned char>(sbyte);
        if (full_bar) __syncthreads(); else lds_barrier();      // (the output stores drain behind the next cout block's exchange / the next tile block)
      }
    }
    pb = (pb + nchunk) & 1;
    cur = nxt;
  }
}

// The backward tail of an up-sampling generator block from the SIGN BITS of its last conv (kSignBits of wino3d_kernel):
//   gx = gy * (bit ? 1 : leak),   gpool = 2x2x2 sum-pool of gy.
// One thread = one coarse voxel x 4 channels.  The 8 fine voxels under a coarse voxel are exactly the 8 outputs of ONE lane of the
// producing kernel's epilogue (oz0 = z0 + 2 th, oy0 = y0 + 2 kq, ox0 = x0 + 2 xi_z; bit s = (dz, dy, dx)), so the 8 signs of a channel
// are one byte and the thread's 4 channels one aligned 32-bit word.  Summation order (dz, dy, dx) ascending as upsample_bwd_kernel.
__global__ __launch_bounds__(256) void lrelu_bits_bwd_pool_kernel(const float4* __restrict__ gy, const unsigned* __restrict__ bits,
                                                                  float4* __restrict__ gx, float4* __restrict__ gpool, float leak,
                                                                  int64_t nsrc4, int Dc, int Hc, int Wc, int C4, int nbz, int nby, int nbx,
                                                                  int ncs) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= nsrc4) return;
  const int c4 = static_cast<int>(i % C4);
  int64_t r = i / C4;
  const int xc = static_cast<int>(r % Wc); r /= Wc;
  const int yc = static_cast<int>(r % Hc); r /= Hc;
  const int zc = static_cast<int>(r % Dc);
  const int64_t b = r / Dc;
  const int64_t id = ((b * nbz + (zc >> 1)) * nby + (yc >> 2)) * nbx + (xc >> 2);
  const int wave = (zc & 1) * 4 + (xc & 3), kq = yc & 3;
  const int cs = c4 >> 3, nb = (c4 >> 2) & 1, tl = (c4 & 3) * 4;
  const unsigned word = bits[((id * ncs + cs) * kBitBytesPerBlock + wave * 128 + nb * 64 + kq * 16 + tl) >> 2];
  const int64_t W2 = 2 * Wc, H2 = 2 * Hc, D2 = 2 * Dc;
  float4 g[8];
  int64_t idx[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int dz = k >> 2, dy = (k >> 1) & 1, dx = k & 1;
    idx[k] = (((b * D2 + (2 * zc + dz)) * H2 + (2 * yc + dy)) * W2 + (2 * xc + dx)) * C4 + c4;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) g[k] = gy[idx[k]];
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    acc.x += g[k].x; acc.y += g[k].y; acc.z += g[k].z; acc.w += g[k].w;
    float4 o;
    o.x = ((word >> k) & 1u) ? g[k].x : leak * g[k].x;
    o.y = ((word >> (8 + k)) & 1u) ? g[k].y : leak * g[k].y;
    o.z = ((word >> (16 + k)) & 1u) ? g[k].z : leak * g[k].z;
    o.w = ((word >> (24 + k)) & 1u) ? g[k].w : leak * g[k].w;
    gx[idx[k]] = o;
  }
  gpool[i] = acc;
}

// ---- host side: one argument check, one launch -------------------------------------------------------------------------------------
// The operands of a launch as the kernel sees them: the pointer fields of WinoArgs in its order.  Bit i of the masks below = field i.
struct WinoOps {
  const float *x, *wp, *bias, *residual, *mask_src;
  float *y, *y2;
  void* bits_out;
  const void* bits_in;
};
enum : unsigned { kX = 1, kWp = 2, kBias = 4, kResidual = 8, kMaskSrc = 16, kY = 32, kY2 = 64, kBitsOut = 128, kBitsIn = 256 };

// What differs between the argument checks of the seven entry points (everything else is wino_check itself):
struct WinoEntry {
  const char* name;
  unsigned need;          // operands that must not be null
  unsigned aligned;       // operands that must be 16-byte aligned: x, the packed weights, the bit words, and y where every instantiation
                          // the entry point reaches may store it 16 bytes at a time (a null operand counts as aligned)
  bool coarse;            // B, D, H, W are the COARSE extents of an up-sampling form: the kernel runs on twice each
  bool up_fwd_volume;     // the 2 GiB bound is on 8 v Cout and v Cin (v = coarse volume: y is fine, x coarse), not on the kernel's volume x max(Cin, Cout)
  bool even;              // extents must be even (the output of a 2x up-sampling block)
  bool flags_first;       // the flag / operand check comes before the volume bound, not behind it
};
//                                  name                            need                                          aligned                          coarse upvol  even   flags first
constexpr WinoEntry kFwd =        {"df_wino_conv_fwd",            kX | kWp | kY,                                  kX | kWp | kY,                     false, false, false, false};
constexpr WinoEntry kFwdBits =    {"df_wino_conv_fwd_bits",       kX | kWp | kY,                                  kX | kWp | kY | kBitsIn | kBitsOut, false, false, false, false};
constexpr WinoEntry kAddup =      {"df_wino_conv_fwd_addup",      kX | kWp | kBias | kResidual | kY | kY2,        kX | kWp,                          false, false, true,  false};
constexpr WinoEntry kAddupBits =  {"df_wino_conv_fwd_addup_bits", kX | kWp | kBias | kResidual | kY2 | kBitsOut,  kX | kWp | kBitsOut,               false, false, true,  false};
constexpr WinoEntry kUpFwd =      {"df_wino_upconv_fwd",          kX | kWp | kY,                                  kX | kWp | kY,                     true,  true,  false, true};
constexpr WinoEntry kUpFwdBits =  {"df_wino_upconv_fwd_bits",     kX | kWp | kY | kBias | kBitsOut,               kX | kWp | kY | kBitsOut,          true,  true,  false, false};
constexpr WinoEntry kUpDgrad =    {"df_wino_upconv_dgrad",        kX | kWp | kY,                                  kX | kWp,                          true,  false, false, false};

// B, D, H, W, Cin, Cout as the entry point received them; flags_ok = the entry point's own rule for its flags and their operands
int wino_check(const WinoEntry& e, const WinoOps& o, int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, bool flags_ok,
               const char* flags_rule) {
  const void* const p[9] = {o.x, o.wp, o.bias, o.residual, o.mask_src, o.y, o.y2, o.bits_out, o.bits_in};
  bool present = true, aligned = true;
  for (int i = 0; i < 9; ++i) {
    if ((e.need >> i) & 1u) present = present && p[i] != nullptr;
    if ((e.aligned >> i) & 1u) aligned = aligned && df::aligned16(p[i]);
  }
  DF_REQUIRE(present, DF_EINVAL, "%s: null pointer", e.name);
  DF_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, DF_EINVAL, "%s: non-positive extent", e.name);
  DF_REQUIRE(!e.even || (D % 2 == 0 && H % 2 == 0 && W % 2 == 0), DF_EINVAL, "%s: extents must be even (the output of a 2x up-sampling block)", e.name);
  DF_REQUIRE(Cin > 0 && Cout > 0 && Cin % 32 == 0 && Cout % 32 == 0, DF_ESHAPE, "%s: Cin, Cout must be multiples of 32", e.name);
  if (e.flags_first) DF_REQUIRE(flags_ok, DF_EINVAL, "%s: %s", e.name, flags_rule);
  // (staging goes through 32-bit byte offsets into one batch volume, with 0x80000000 as the out-of-range sentinel)
  const int64_t v = D * H * W, cmax = Cin > Cout ? Cin : Cout;
  const bool fits = e.up_fwd_volume ? 8 * v * Cout <= (1LL << 29) && v * Cin <= (1LL << 29) : (e.coarse ? 8 : 1) * v * cmax <= (1LL << 29);
  DF_REQUIRE(fits && Cin * Cout <= (1LL << 24), DF_ESHAPE, "%s: one batch volume must stay below 2 GiB, Cin * Cout below 16 Mi", e.name);
  if (!e.flags_first) DF_REQUIRE(flags_ok, DF_EINVAL, "%s: %s", e.name, flags_rule);
  DF_REQUIRE(aligned, DF_EALIGN, "%s: x, the packed weights, the bit words and a y stored 16 bytes at a time must be 16-byte aligned", e.name);
  return DF_OK;
}

// D, H, W = the OUTPUT extents of the underlying convolution, Cin / Cout = the kernel's; (fl, mode) must be one of the pairs listed here
int wino_launch(const char* name, int fl, int mode, const WinoOps& o, int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                int flags, float leak, df_stream_t stream) {
  WinoArgs a;
  a.x = o.x; a.wp = reinterpret_cast<const f32x4*>(o.wp); a.zeros = o.wp + 64 * Cin * Cout;
  a.bias = o.bias; a.residual = o.residual; a.mask_src = o.mask_src; a.y = o.y; a.y2 = o.y2;
  a.bits_out = static_cast<unsigned char*>(o.bits_out); a.bits_in = static_cast<const unsigned char*>(o.bits_in);
  a.B = (int)B; a.D = (int)D; a.H = (int)H; a.W = (int)W; a.Cin = (int)Cin; a.Cout = (int)Cout;
  a.nbz = (int)ceil_div(D, 4); a.nby = (int)ceil_div(H, 8); a.nbx = (int)ceil_div(W, 8);
  const int64_t ntb = B * a.nbz * a.nby * a.nbx;
  a.ncs = (int)(Cout / 32);
  if (const int rc = dfconv::wino_slices_check(name, Cout / 32)) return rc;
  DF_REQUIRE(ntb * a.ncs < (1LL << 31), DF_ESHAPE, "%s: too many workgroups", name);
  a.ntb = (int)ntb;
  a.flags = flags; a.leak = leak;
  const dim3 grid((unsigned)dfconv::wino_grid(a, ntb));
  hipStream_t s = df::as_stream(stream);
#define DF_WINO(F, M) \
  if (fl == (F) && mode == (M)) { hipLaunchKernelGGL((wino3d_kernel<F, M>), grid, dim3(kT), 0, s, a); return df::launched(name); }
  DF_WINO(-1, 0)
  DF_WINO(0, 0)
  DF_WINO(DF_CONV_RESIDUAL, 0)
  DF_WINO(DF_CONV_MASK, 0)
  DF_WINO(DF_CONV_MASK | kMaskBits, 0)
  DF_WINO(DF_CONV_BIAS | DF_CONV_LRELU, 0)
  DF_WINO(DF_CONV_BIAS | DF_CONV_LRELU | kSignBits, 0)
  DF_WINO(DF_CONV_BIAS | DF_CONV_LRELU | DF_CONV_ADDUP, 0)
  DF_WINO(DF_CONV_BIAS | DF_CONV_LRELU | DF_CONV_ADDUP | kSignBits | kNoPrimary, 0)
  DF_WINO(0, 2)
  DF_WINO(DF_CONV_BIAS | DF_CONV_LRELU, 3)
  DF_WINO(DF_CONV_BIAS | DF_CONV_LRELU | kSignBits, 3)
#undef DF_WINO
  return df::fail(DF_EINVAL, "%s: wino3d_kernel<%d, %d> is not instantiated", name, fl, mode);
}

}  // namespace

extern "C" {

int64_t df_wino_packed_elems(int64_t cin, int64_t cout, int mode) {
  (void)mode;
  return 64 * cin * cout + kZeroFloats;
}

int df_wino_pack_weights(const float* w, float* wp, int64_t cin, int64_t cout, int mode, df_stream_t stream) {
  DF_REQUIRE(w && wp, DF_EINVAL, "df_wino_pack_weights: null pointer");
  DF_REQUIRE(cin > 0 && cout > 0 && cin % 32 == 0 && cout % 32 == 0 && (mode == 0 || mode == 1), DF_ESHAPE,
             "df_wino_pack_weights: cin, cout must be multiples of 32; mode 0|1");
  const int64_t total = 64 * cin * cout;
  int64_t g = ceil_div(cin * cout, 64);      // one wave per workgroup: 16 K filters still cover all 256 CUs
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(wino_pack_kernel, dim3((unsigned)g), dim3(64), 0, df::as_stream(stream), w, wp, (int)cin, (int)cout, mode,
                     total);
  return df::launched("df_wino_pack_weights");
}

int64_t df_wino_signbits_bytes(int64_t B, int64_t D, int64_t H, int64_t W, int64_t C) {
  if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 32) return 0;
  return B * ceil_div(D, 4) * ceil_div(H, 8) * ceil_div(W, 8) * (C / 32) * kBitBytesPerBlock;
}

int df_wino_conv_fwd(const float* x, const float* wp, const float* bias, const float* residual, const float* mask_src,
                     float* y, int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int flags, float leak,
                     df_stream_t stream) {
  const WinoOps o = {x, wp, bias, residual, mask_src, y, nullptr, nullptr, nullptr};
  const bool ok = !(flags & DF_CONV_ADDUP) && (!(flags & DF_CONV_BIAS) || bias) && (!(flags & DF_CONV_RESIDUAL) || residual) &&
                  (!(flags & DF_CONV_MASK) || mask_src);
  if (const int rc = wino_check(kFwd, o, B, D, H, W, Cin, Cout, ok,
                                "DF_CONV_BIAS / RESIDUAL / MASK need bias / residual / mask_src; DF_CONV_ADDUP needs df_wino_conv_fwd_addup"))
    return rc;
  // the flag combinations with an epilogue of their own; every other one runs the kernel that tests a.flags per element
  const bool special = flags == (DF_CONV_BIAS | DF_CONV_LRELU) || flags == DF_CONV_MASK || flags == DF_CONV_RESIDUAL || flags == 0;
  return wino_launch(kFwd.name, special ? flags : -1, 0, o, B, D, H, W, Cin, Cout, flags, leak, stream);
}

int df_wino_conv_fwd_bits(const float* x, const float* wp, const float* bias, const void* mask_bits, float* y, void* sign_bits, int64_t B,
                          int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int flags, float leak, df_stream_t stream) {
  const WinoOps o = {x, wp, bias, nullptr, nullptr, y, nullptr, sign_bits, mask_bits};
  const bool fwd = flags == (DF_CONV_BIAS | DF_CONV_LRELU) && bias && sign_bits && !mask_bits;
  const bool dgr = flags == DF_CONV_MASK && mask_bits && !sign_bits;
  if (const int rc = wino_check(kFwdBits, o, B, D, H, W, Cin, Cout, fwd || dgr, "either (BIAS|LRELU, bias, sign_bits out) or (MASK, mask_bits in)"))
    return rc;
  return wino_launch(kFwdBits.name, fwd ? flags | kSignBits : flags | kMaskBits, 0, o, B, D, H, W, Cin, Cout, flags, leak, stream);
}

int df_wino_conv_fwd_addup(const float* x, const float* wp, const float* bias, const float* xc, float* y, float* y2, int64_t B,
                           int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, float leak, df_stream_t stream) {
  const WinoOps o = {x, wp, bias, xc, nullptr, y, y2, nullptr, nullptr};
  if (const int rc = wino_check(kAddup, o, B, D, H, W, Cin, Cout, true, "")) return rc;
  constexpr int F = DF_CONV_BIAS | DF_CONV_LRELU | DF_CONV_ADDUP;
  return wino_launch(kAddup.name, F, 0, o, B, D, H, W, Cin, Cout, F, leak, stream);
}

int df_wino_conv_fwd_addup_bits(const float* x, const float* wp, const float* bias, const float* xc, float* y2, void* sign_bits,
                                int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, float leak, df_stream_t stream) {
  const WinoOps o = {x, wp, bias, xc, nullptr, nullptr, y2, sign_bits, nullptr};
  if (const int rc = wino_check(kAddupBits, o, B, D, H, W, Cin, Cout, true, "")) return rc;
  constexpr int F = DF_CONV_BIAS | DF_CONV_LRELU | DF_CONV_ADDUP;
  return wino_launch(kAddupBits.name, F | kSignBits | kNoPrimary, 0, o, B, D, H, W, Cin, Cout, F, leak, stream);
}

int df_wino_upconv_fwd(const float* xc, const float* wp, const float* bias, float* y, int64_t B, int64_t Dc, int64_t Hc,
                       int64_t Wc, int64_t Cin, int64_t Cout, int flags, float leak, df_stream_t stream) {
  const WinoOps o = {xc, wp, bias, nullptr, nullptr, y, nullptr, nullptr, nullptr};
  if (const int rc = wino_check(kUpFwd, o, B, Dc, Hc, Wc, Cin, Cout, flags == (DF_CONV_BIAS | DF_CONV_LRELU) && bias,
                                "flags must be DF_CONV_BIAS | DF_CONV_LRELU, with bias"))
    return rc;
  return wino_launch(kUpFwd.name, flags, 3, o, B, 2 * Dc, 2 * Hc, 2 * Wc, Cin, Cout, flags, leak, stream);
}

int df_wino_upconv_fwd_bits(const float* xc, const float* wp, const float* bias, float* y, void* sign_bits, int64_t B, int64_t Dc,
                            int64_t Hc, int64_t Wc, int64_t Cin, int64_t Cout, float leak, df_stream_t stream) {
  const WinoOps o = {xc, wp, bias, nullptr, nullptr, y, nullptr, sign_bits, nullptr};
  if (const int rc = wino_check(kUpFwdBits, o, B, Dc, Hc, Wc, Cin, Cout, true, "")) return rc;
  constexpr int F = DF_CONV_BIAS | DF_CONV_LRELU;
  return wino_launch(kUpFwdBits.name, F | kSignBits, 3, o, B, 2 * Dc, 2 * Hc, 2 * Wc, Cin, Cout, F, leak, stream);
}

int df_wino_upconv_dgrad(const float* g, const float* wp, float* acc, int64_t B, int64_t Dc, int64_t Hc, int64_t Wc, int64_t Cin,
                         int64_t Cout, df_stream_t stream) {
  const WinoOps o = {g, wp, nullptr, nullptr, nullptr, acc, nullptr, nullptr, nullptr};
  if (const int rc = wino_check(kUpDgrad, o, B, Dc, Hc, Wc, Cin, Cout, true, "")) return rc;
  // the adjoint conv reads g (Cout channels, fine grid) and produces Cin channels: the kernel's Cin / Cout are the entry point's Cout / Cin
  return wino_launch(kUpDgrad.name, 0, 2, o, B, 2 * Dc, 2 * Hc, 2 * Wc, Cout, Cin, 0, 0.f, stream);
}

int df_lrelu_bits_bwd_pool2x(const float* gy, const void* mask_bits, float* gx, float* gpool, float leak, int64_t B, int64_t Dc, int64_t Hc,
                             int64_t Wc, int64_t C, df_stream_t stream) {
  DF_REQUIRE(gy && mask_bits && gx && gpool, DF_EINVAL, "df_lrelu_bits_bwd_pool2x: null pointer");
  DF_REQUIRE(B > 0 && Dc > 0 && Hc > 0 && Wc > 0, DF_EINVAL, "df_lrelu_bits_bwd_pool2x: non-positive extent");
  DF_REQUIRE(C > 0 && C % 32 == 0, DF_ESHAPE, "df_lrelu_bits_bwd_pool2x: C must be a multiple of 32 (the sign bits' cout slices)");
  DF_REQUIRE(df::aligned16(gy) && df::aligned16(gx) && df::aligned16(gpool) && df::aligned16(mask_bits), DF_EALIGN,
             "df_lrelu_bits_bwd_pool2x: 16-byte alignment");
  const int64_t n4 = B * Dc * Hc * Wc * (C / 4);
  DF_REQUIRE(ceil_div(n4, 256) < (1LL << 31), DF_ESHAPE, "df_lrelu_bits_bwd_pool2x: tensor too large");
  hipLaunchKernelGGL(lrelu_bits_bwd_pool_kernel, dim3((unsigned)ceil_div(n4, 256)), dim3(256), 0, df::as_stream(stream),
                     reinterpret_cast<const float4*>(gy), static_cast<const unsigned*>(mask_bits), reinterpret_cast<float4*>(gx),
                     reinterpret_cast<float4*>(gpool), leak, n4, (int)Dc, (int)Hc, (int)Wc, (int)(C / 4), (int)ceil_div(2 * Dc, 4),
                     (int)ceil_div(2 * Hc, 8), (int)ceil_div(2 * Wc, 8), (int)(C / 32));
  return df::launched("df_lrelu_bits_bwd_pool2x");
}

}  // extern "C"
