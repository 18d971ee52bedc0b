/*
 * deepfluids_hip_debug.h -- tuning / instrumentation entry points of the TUNING build of the library
 * (`make -C deep_fluids_amd/csrc tuning` -> libdeepfluids_hip_tuning.so, compiled with -DDF_TUNING).
 *
 * NOT part of the drop-in boundary: the release library (libdeepfluids_hip.so) does not export these symbols and has
 * no mutable global state.  They exist for the probes under tools/ (stencil and fused-tail launch knobs, timing
 * variants of conv_bf16x3_kernel).  Everything here is process-global and thread-unsafe by design.
 */
#ifndef DEEPFLUIDS_HIP_DEBUG_H
#define DEEPFLUIDS_HIP_DEBUG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* jacobian3d_fwd launch knobs: non-temporal stores on/off; XCD run length of the block remap */
void df_debug_set_stencil_nt(int v);
void df_debug_set_stencil_group(int v);
void df_debug_set_stencil_lds(int v);      /* 0: register-only adjoints (jacobian3d_bwd_vec_kernel) even where the LDS-staged kernel applies */
/* fused-tail kernel choice: 0 default dispatch, 1 16-byte quad kernels, 2 record-per-lane (12-byte load) kernels */
void df_debug_set_tail(int v);

/* conv_bf16x3_kernel (the direct split-operand conv) timing-only variants, results wrong by construction: 1 staging loads replaced by zeros,
 * 2 no weight loads, 4 no LDS operand reads, 8 no staging at all (+ sums 3, 6, 10, 14); 0 = production */
void df_debug_set_conv_bf16(int v);

#ifdef __cplusplus
}
#endif
#endif
