// Launch recorder of tests/test_wgrad_launches_host.py, tests/test_wino_launches_host.py, tests/test_conv_cases_host.py and
// tests/test_wino_cases_host.py: calls the weight-gradient, the 3-D and 2-D Winograd and the direct conv (forward / input-gradient)
// entry points of libdeepfluids_hip.so WITHOUT a GPU and prints what they would have launched.  No HIP header, no device: this executable itself defines every HIP runtime call the host path of
// csrc/conv_wgrad.hip makes (df_common.hpp, core.hip), and a symbol defined in the executable wins over the shared runtime's when the
// library's calls are bound.  A launch arrives as hipLaunchKernel(kernel handle, grid, block, argument pointers, LDS bytes, stream);
// handle - load base of the library = the symbol's value in the library's `nm -C` listing, which names the instantiation.
//
//   wgrad_launch_recorder <symbols> <rows>
//     symbols  lines "<hex value> <demangled name>" (the library's nm -C listing, address and name columns)
//     rows     lines "id entry B D H W Cin Cout kz algo bias xoff goff"; entry as in tests/wgrad_cases.py, algo -1 = the entry point
//              without an algo argument
//              | "id entry B D H W Cin Cout flags present misaligned" with entry = wino_fwd | wino_fwd_bits | wino_fwd_addup | wino_fwd_addup_bits |
//              wino_upconv_fwd | wino_upconv_fwd_bits | wino_upconv_dgrad | wino43 | wino_bits_bwd (df_lrelu_bits_bwd_pool2x: C = Cin); present /
//              misaligned = bit masks over the operand slots x (gy) 1, wp 2, bias 4, residual (xc of the add-up forms) 8, mask_src 16,
//              mask_bits 32, y (acc, gx) 64, y2 (gpool) 128, sign_bits 256: a slot not present is passed as NULL, a misaligned one 4 bytes behind
//              its address; leak = 0.2
//              | "id entry B H W Cin Cout flags present misaligned" (tests/wino_cases.py, tests/test_wino_cases_host.py), the same slots, with entry =
//              w2_fwd df_wino2d_conv_fwd | w2_up_fwd | w2_up_dgrad | w2_43 df_wino2d43_conv | w2_43_bits | w2_43_addup_bits | w2_words_bwd
//              df_lrelu_words2d_bwd_pool2x (C = Cin) | w2_pack df_wino2d_pack_weights | w2_43_pack (w = slot x, mode = flags) | the queries
//              w2_packed_elems | w2_43_packed_elems (mode = flags) | w2_43_signbits_bytes (C = Cin), whose value is printed as ws
//              | "id entry B D H W Cin Cout kz flags present ox owp obias ores omask oy" with entry = dc_fwd | dc_fwd_bf16x3 | dc_s2_fwd |
//              dc_s2_dgrad | dc_up_fwd | dc_up_fwd_bf16x3 | dc_up_dgrad | dc_up_dgrad_bf16x3 (tests/conv_cases.py): present = bit mask over
//              the slots x (gy / g of the dgrads) 1, wp 2, bias 4, residual 8, mask_src 16, y (gx / acc) 32; o* = the slot's payload offset
//              in floats; leak = 0.2
//   per row:   "row <id>", one line per runtime call in order --
//              "  launch <kernel> grid x y z block x lds <bytes> args <hex bytes>" | "  funcattr <kernel> <attribute> <value>" --
//              then "end <id> rc <return code> ws <the workspace bytes the entry point's query asked for, and the call got>"
// Operands sit at fixed fake addresses (never dereferenced on the host) plus the row's payload offsets; the LDS opt-in query is answered
// with 160 KB (an unpartitioned MI355X).
#include <dlfcn.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "deepfluids_hip.h"

namespace {

struct dim3 { unsigned x, y, z; };      // layout of HIP's dim3

std::map<uintptr_t, std::string> g_names;      // symbol value -> demangled name
dim3 g_grid, g_block;
size_t g_lds;
void* g_stream;

std::string kernel_name(const void* f) {
  Dl_info di;
  if (!dladdr(f, &di) || !di.dli_fbase) return "?";
  const auto it = g_names.find(reinterpret_cast<uintptr_t>(f) - reinterpret_cast<uintptr_t>(di.dli_fbase));
  return it == g_names.end() ? "?" : it->second;
}

// Argument bytes of each kernel the weight-gradient host code launches: the sizes of its parameters in order.  The kernels that take one
// argument struct list its size WITHOUT tail padding (WxyzArgs: 140 of 144, SmallWgradArgs: 84 of 88), which is not initialised.
// hole_at / hole_len: padding bytes inside the one argument struct (never initialised by the host code), printed as 00.
struct Layout { const char* prefix; int n; int size[14]; int hole_at, hole_len; };
const Layout kLayouts[] = {
    {"(anonymous namespace)::wgrad_kernel<", 1, {128}},
    {"(anonymous namespace)::wgrad_s2_kernel<", 1, {128}},
    {"(anonymous namespace)::wgrad_up2_kernel<", 1, {128}},
    {"(anonymous namespace)::wgrad_wx_kernel<", 1, {128}},
    {"(anonymous namespace)::wgrad_bf16x3_kernel<", 1, {128}},
    {"(anonymous namespace)::wgrad_wxy_kernel<", 1, {136}},
    {"(anonymous namespace)::wgrad_wxyz_kernel<", 1, {140}},
    {"(anonymous namespace)::wgrad_wxyz_fused_kernel<", 1, {140}},
    {"(anonymous namespace)::wgrad_wxyz_up_fused_kernel<", 1, {140}},
    {"(anonymous namespace)::wgrad_wxyz_staged_kernel<", 1, {140}},
    {"(anonymous namespace)::wgrad_small_n_kernel<", 1, {84}},
    {"(anonymous namespace)::wgrad_thin_mfma_kernel<", 1, {72}},
    {"(anonymous namespace)::wgrad_reduce_kernel(", 10, {8, 8, 8, 8, 4, 4, 4, 4, 4, 4}},
    {"(anonymous namespace)::wgrad_wx_reduce_kernel(", 10, {8, 8, 8, 8, 4, 4, 4, 4, 4, 4}},
    {"(anonymous namespace)::wgrad_wxy_reduce_kernel(", 10, {8, 8, 8, 8, 4, 4, 4, 4, 4, 4}},
    {"(anonymous namespace)::wgrad_wxyz_reduce_kernel(", 10, {8, 8, 8, 8, 4, 4, 4, 4, 4, 4}},
    {"(anonymous namespace)::wgrad_up_reduce_kernel(", 10, {8, 8, 8, 8, 4, 4, 4, 4, 4, 4}},
    {"(anonymous namespace)::wgrad_small_reduce_kernel(", 8, {8, 8, 8, 8, 4, 8, 4, 4}},
    {"(anonymous namespace)::wgrad_thin_reduce_kernel(", 9, {8, 8, 8, 8, 4, 4, 4, 4, 4}},
    {"(anonymous namespace)::pad_rows_kernel(", 6, {8, 8, 8, 4, 4, 4}},
    {"df::zero_words_kernel(", 2, {8, 8}},
    // WinoArgs up to and including spx (the experiment field that once followed it was never set by these entry points); W43Args whole
    {"(anonymous namespace)::wino3d_kernel<", 1, {136}},
    {"(anonymous namespace)::wino43_kernel<", 1, {128}},
    // the 2-D Winograd families: Wino2dArgs and W2Args whole
    {"(anonymous namespace)::wino2d_kernel<", 1, {96}},
    {"(anonymous namespace)::wino2d43_kernel<", 1, {120}},
    {"(anonymous namespace)::wino2d_pack_kernel(", 6, {8, 8, 4, 4, 4, 8}},
    {"(anonymous namespace)::wino2d43_pack_kernel(", 5, {8, 8, 4, 4, 4}},
    {"(anonymous namespace)::lrelu_words2d_bwd_pool_kernel(", 11, {8, 8, 8, 8, 4, 4, 4, 4, 4, 4, 4}},
    {"(anonymous namespace)::lrelu_bits_bwd_pool_kernel(", 14, {8, 8, 8, 8, 4, 8, 4, 4, 4, 4, 4, 4, 4, 4}},
    // the direct convs: ConvArgs whole (200 bytes, 4 of padding in front of wclass); ThinKArgs without its tail padding (84 of 88); ThinNArgs
    {"(anonymous namespace)::conv_mfma_kernel<", 1, {200}, 156, 4},
    {"(anonymous namespace)::conv_tiny2d_kernel(", 1, {200}, 156, 4},
    {"dfconv::(anonymous namespace)::conv_bf16x3_kernel<", 1, {200}, 156, 4},
    {"dfconv::(anonymous namespace)::conv_small_n_kernel<", 1, {200}, 156, 4},
    {"dfconv::(anonymous namespace)::conv_small_k_kernel<", 2, {200, 4}, 156, 4},
    {"dfconv::(anonymous namespace)::conv_thin_k_mfma_kernel<", 1, {84}},
    {"dfconv::(anonymous namespace)::conv_thin_n_mfma_kernel<", 1, {72}},
    {"(anonymous namespace)::pack_kernel(", 8, {8, 8, 4, 4, 4, 4, 4, 4}},
    {"(anonymous namespace)::upconv_pack_kernel(", 8, {8, 8, 4, 4, 4, 4, 4, 4}},
    {"dfconv::(anonymous namespace)::pack_bf16x3_kernel(", 8, {8, 8, 4, 4, 4, 4, 4, 4}},
    {"dfconv::(anonymous namespace)::upconv_pack_bf16x3_kernel(", 8, {8, 8, 4, 4, 4, 4, 4, 4}},
};

}  // namespace

extern "C" {

int __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, void* stream) {
  g_grid = grid; g_block = block; g_lds = lds; g_stream = stream;
  return 0;
}
int __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, void** stream) {
  *grid = g_grid; *block = g_block; *lds = g_lds; *stream = g_stream;
  return 0;
}
int hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t lds, void* stream) {
  (void)stream;
  const std::string name = kernel_name(f);
  printf("  launch %s grid %u %u %u block %u lds %zu args ", name.c_str(), grid.x, grid.y, grid.z, block.x, lds);
  const Layout* lay = nullptr;
  for (const Layout& l : kLayouts)
    if (name.compare(0, strlen(l.prefix), l.prefix) == 0) lay = &l;
  if (!lay) { printf("?\n"); return 0; }
  for (int i = 0; i < lay->n; ++i) {
    const unsigned char* p = static_cast<const unsigned char*>(args[i]);
    for (int b = 0; b < lay->size[i]; ++b) printf("%02x", i == 0 && b >= lay->hole_at && b < lay->hole_at + lay->hole_len ? 0 : p[b]);
    if (i + 1 < lay->n) printf(".");
  }
  printf("\n");
  return 0;
}
int hipGetLastError(void) { return 0; }
int hipPeekAtLastError(void) { return 0; }
const char* hipGetErrorString(int) { return "no error (launch recorder)"; }
int hipFuncSetAttribute(const void* f, int attr, int value) {
  printf("  funcattr %s %d %d\n", kernel_name(f).c_str(), attr, value);
  return 0;
}
int hipGetDevice(int* dev) { *dev = 0; return 0; }
int hipDeviceGetAttribute(int* v, int attr, int dev) {
  (void)attr; (void)dev;
  *v = 160 * 1024;
  return 0;
}
int hipMemsetAsync(void* p, int value, size_t bytes, void* stream) {
  (void)stream;
  printf("  memset %p %d %zu\n", p, value, bytes);
  return 0;
}

}  // extern "C"

// one row of tests/test_wino_launches_host.py: operand slot i sits at (i + 1) << 44
static int wino_row(const std::string& e, long long B, long long D, long long H, long long W, long long Cin, long long Cout, int flags,
                    int present, int mis) {
  auto slot = [&](int i) -> char* {
    if (!((present >> i) & 1)) return nullptr;
    return reinterpret_cast<char*>((static_cast<uintptr_t>(i + 1) << 44) + (((mis >> i) & 1) ? 4 : 0));
  };
  auto f = [&](int i) { return reinterpret_cast<float*>(slot(i)); };
  const float leak = 0.2f;
  if (e == "wino_fwd") return df_wino_conv_fwd(f(0), f(1), f(2), f(3), f(4), f(6), B, D, H, W, Cin, Cout, flags, leak, nullptr);
  if (e == "wino_fwd_bits") return df_wino_conv_fwd_bits(f(0), f(1), f(2), slot(5), f(6), slot(8), B, D, H, W, Cin, Cout, flags, leak, nullptr);
  if (e == "wino_fwd_addup") return df_wino_conv_fwd_addup(f(0), f(1), f(2), f(3), f(6), f(7), B, D, H, W, Cin, Cout, leak, nullptr);
  if (e == "wino_fwd_addup_bits") return df_wino_conv_fwd_addup_bits(f(0), f(1), f(2), f(3), f(7), slot(8), B, D, H, W, Cin, Cout, leak, nullptr);
  if (e == "wino_upconv_fwd") return df_wino_upconv_fwd(f(0), f(1), f(2), f(6), B, D, H, W, Cin, Cout, flags, leak, nullptr);
  if (e == "wino_upconv_fwd_bits") return df_wino_upconv_fwd_bits(f(0), f(1), f(2), f(6), slot(8), B, D, H, W, Cin, Cout, leak, nullptr);
  if (e == "wino_upconv_dgrad") return df_wino_upconv_dgrad(f(0), f(1), f(6), B, D, H, W, Cin, Cout, nullptr);
  if (e == "wino43") return df_wino43_conv(f(0), f(1), f(2), f(3), f(4), slot(5), f(6), f(7), slot(8), B, D, H, W, Cin, Cout, flags, leak, nullptr);
  if (e == "wino_bits_bwd") return df_lrelu_bits_bwd_pool2x(f(0), slot(5), f(6), f(7), leak, B, D, H, W, Cin, nullptr);
  return -1000;
}

// one row of the 2-D entry points (tests/wino_cases.py, tests/test_wino_cases_host.py): the slots and addresses of wino_row; *value = a query's answer
static int wino2d_row(const std::string& e, long long B, long long H, long long W, long long Cin, long long Cout, int flags, int present, int mis,
                      long long* value) {
  auto slot = [&](int i) -> char* {
    if (!((present >> i) & 1)) return nullptr;
    return reinterpret_cast<char*>((static_cast<uintptr_t>(i + 1) << 44) + (((mis >> i) & 1) ? 4 : 0));
  };
  auto f = [&](int i) { return reinterpret_cast<float*>(slot(i)); };
  const float leak = 0.2f;
  if (e == "w2_fwd") return df_wino2d_conv_fwd(f(0), f(1), f(2), f(3), f(4), f(6), B, H, W, Cin, Cout, flags, leak, nullptr);
  if (e == "w2_up_fwd") return df_wino2d_upconv_fwd(f(0), f(1), f(2), f(6), B, H, W, Cin, Cout, flags, leak, nullptr);
  if (e == "w2_up_dgrad") return df_wino2d_upconv_dgrad(f(0), f(1), f(6), B, H, W, Cin, Cout, nullptr);
  if (e == "w2_43") return df_wino2d43_conv(f(0), f(1), f(2), f(3), f(4), f(6), B, H, W, Cin, Cout, flags, leak, nullptr);
  if (e == "w2_43_bits") return df_wino2d43_conv_bits(f(0), f(1), f(2), slot(5), f(6), slot(8), B, H, W, Cin, Cout, flags, leak, nullptr);
  if (e == "w2_43_addup_bits") return df_wino2d43_conv_addup_bits(f(0), f(1), f(2), f(3), f(7), slot(8), B, H, W, Cin, Cout, leak, nullptr);
  if (e == "w2_words_bwd") return df_lrelu_words2d_bwd_pool2x(f(0), slot(5), f(6), f(7), leak, B, H, W, Cin, nullptr);
  if (e == "w2_pack") return df_wino2d_pack_weights(f(0), f(1), Cin, Cout, flags, nullptr);
  if (e == "w2_43_pack") return df_wino2d43_pack_weights(f(0), f(1), Cin, Cout, flags, nullptr);
  if (e == "w2_packed_elems") { *value = df_wino2d_packed_elems(Cin, Cout, flags); return 0; }
  if (e == "w2_43_packed_elems") { *value = df_wino2d43_packed_elems(Cin, Cout, flags); return 0; }
  if (e == "w2_43_signbits_bytes") { *value = df_wino2d43_signbits_bytes(B, H, W, Cin); return 0; }
  return -1000;
}

// one row of tests/conv_cases.py: operand slot i sits at (i + 1) << 44, plus the row's offset in floats
static int dc_row(const std::string& e, long long B, long long D, long long H, long long W, long long Cin, long long Cout, int kz, int flags,
                  int present, const int* off) {
  auto f = [&](int i) -> float* {
    if (!((present >> i) & 1)) return nullptr;
    return reinterpret_cast<float*>(static_cast<uintptr_t>(i + 1) << 44) + off[i];
  };
  const float leak = 0.2f;
  if (e == "dc_fwd") return df_conv_fwd(f(0), f(1), f(2), f(3), f(4), f(5), B, D, H, W, Cin, Cout, kz, flags, leak, nullptr);
  if (e == "dc_fwd_bf16x3") return df_conv_fwd_bf16x3(f(0), f(1), f(2), f(3), f(4), f(5), B, D, H, W, Cin, Cout, kz, flags, leak, nullptr);
  if (e == "dc_s2_fwd") return df_conv_s2_fwd(f(0), f(1), f(2), f(5), B, D, H, W, Cin, Cout, kz, flags, leak, nullptr);
  if (e == "dc_s2_dgrad") return df_conv_s2_dgrad(f(0), f(1), f(5), B, D, H, W, Cin, Cout, kz, nullptr);
  if (e == "dc_up_fwd") return df_upconv_fwd(f(0), f(1), f(2), f(5), B, D, H, W, Cin, Cout, kz, flags, leak, nullptr);
  if (e == "dc_up_fwd_bf16x3") return df_upconv_fwd_bf16x3(f(0), f(1), f(2), f(5), B, D, H, W, Cin, Cout, kz, flags, leak, nullptr);
  if (e == "dc_up_dgrad") return df_upconv_dgrad(f(0), f(1), f(5), B, D, H, W, Cin, Cout, kz, nullptr);
  if (e == "dc_up_dgrad_bf16x3") return df_upconv_dgrad_bf16x3(f(0), f(1), f(5), B, D, H, W, Cin, Cout, kz, nullptr);
  return -1000;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <symbols> <rows>\n", argv[0]); return 2; }
  FILE* fs = fopen(argv[1], "r");
  FILE* fr = fopen(argv[2], "r");
  if (!fs || !fr) { fprintf(stderr, "cannot open %s\n", fs ? argv[2] : argv[1]); return 2; }
  char line[4096];
  while (fgets(line, sizeof line, fs)) {
    char* end = nullptr;
    const uintptr_t v = strtoull(line, &end, 16);
    if (end == line || *end != ' ') continue;
    std::string name(end + 1);
    while (!name.empty() && (name.back() == '\n' || name.back() == ' ')) name.pop_back();
    if (name.compare(0, 5, "void ") == 0) name.erase(0, 5);      // (function templates are listed with their return type)
    g_names[v] = name;
  }
  fclose(fs);
  float* const X = reinterpret_cast<float*>(0x100000000000ull);
  float* const G = reinterpret_cast<float*>(0x200000000000ull);
  float* const GW = reinterpret_cast<float*>(0x300000000000ull);
  float* const GB = reinterpret_cast<float*>(0x400000000000ull);
  void* const WS = reinterpret_cast<void*>(0x500000000000ull);
  char id[128], entry[32];
  long long B, D, H, W, Cin, Cout;
  int kz, algo, bias, xoff, goff;
  while (fgets(line, sizeof line, fr)) {
    int flags, present, mis;
    int off[6];
    if (sscanf(line, "%127s %31s %lld %lld %lld %lld %lld %lld %d %d %d %d %d %d %d %d %d", id, entry, &B, &D, &H, &W, &Cin, &Cout, &kz, &flags,
               &present, &off[0], &off[1], &off[2], &off[3], &off[4], &off[5]) == 17 && strncmp(entry, "dc_", 3) == 0) {
      printf("row %s\n", id);
      printf("end %s rc %d ws 0\n", id, dc_row(entry, B, D, H, W, Cin, Cout, kz, flags, present, off));
      continue;
    }
    if (sscanf(line, "%127s %31s %lld %lld %lld %lld %lld %lld %d %d %d", id, entry, &B, &D, &H, &W, &Cin, &Cout, &flags, &present, &mis) == 11 &&
        strncmp(entry, "wino", 4) == 0) {
      printf("row %s\n", id);
      printf("end %s rc %d ws 0\n", id, wino_row(entry, B, D, H, W, Cin, Cout, flags, present, mis));
      continue;
    }
    if (sscanf(line, "%127s %31s %lld %lld %lld %lld %lld %d %d %d", id, entry, &B, &H, &W, &Cin, &Cout, &flags, &present, &mis) == 10 &&
        strncmp(entry, "w2_", 3) == 0) {
      long long value = 0;
      printf("row %s\n", id);
      const int rc2 = wino2d_row(entry, B, H, W, Cin, Cout, flags, present, mis, &value);
      printf("end %s rc %d ws %lld\n", id, rc2, value);
      continue;
    }
    if (sscanf(line, "%127s %31s %lld %lld %lld %lld %lld %lld %d %d %d %d %d", id, entry, &B, &D, &H, &W, &Cin, &Cout, &kz, &algo, &bias,
               &xoff, &goff) != 13)
      continue;
    const float* x = X + xoff;
    const float* g = G + goff;
    float* gb = bias ? GB : nullptr;
    const std::string e(entry);
    int64_t ws = 0;
    int rc = -1000;
    printf("row %s", id);
    fflush(stdout);
    if (e == "conv" || e == "conv_bf16x3") {
      ws = df_conv_wgrad_workspace_bytes(B, D, H, W, Cin, Cout, kz);
      printf("\n");
      if (e == "conv_bf16x3") rc = df_conv_wgrad_bf16x3(x, g, GW, gb, B, D, H, W, Cin, Cout, kz, WS, ws, nullptr);
      else if (algo < 0) rc = df_conv_wgrad(x, g, GW, gb, B, D, H, W, Cin, Cout, kz, WS, ws, nullptr);
      else rc = df_conv_wgrad_algo(x, g, GW, gb, B, D, H, W, Cin, Cout, kz, WS, ws, algo, nullptr);
    } else if (e == "up" || e == "up_bf16x3") {
      ws = df_upconv_wgrad_workspace_bytes(B, D, H, W, Cin, Cout, kz);
      printf("\n");
      if (e == "up_bf16x3") rc = df_upconv_wgrad_bf16x3(x, g, GW, gb, B, D, H, W, Cin, Cout, kz, WS, ws, nullptr);
      else if (algo < 0) rc = df_upconv_wgrad(x, g, GW, gb, B, D, H, W, Cin, Cout, kz, WS, ws, nullptr);
      else rc = df_upconv_wgrad_algo(x, g, GW, gb, B, D, H, W, Cin, Cout, kz, WS, ws, algo, nullptr);
    } else if (e == "s2") {
      ws = df_conv_s2_wgrad_workspace_bytes(B, D, H, W, Cin, Cout, kz);
      printf("\n");
      rc = df_conv_s2_wgrad(x, g, GW, gb, B, D, H, W, Cin, Cout, kz, WS, ws, nullptr);
    } else {
      printf("\n");
    }
    printf("end %s rc %d ws %lld\n", id, rc, static_cast<long long>(ws));
  }
  fclose(fr);
  return 0;
}
