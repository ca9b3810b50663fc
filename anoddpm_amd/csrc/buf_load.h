// Raw buffer addressing of the streaming kernels: one resource per tensor, then per access a 32-bit per-lane byte offset (VGPR) plus
// a wave-uniform byte offset (SGPR) -- no 64-bit vector address arithmetic in the loops.  The launchers check that a tensor stays
// below 2 GB.  All address arithmetic that changes inside a K loop is then scalar: VALU instructions are NOT hidden by the fp32 MFMA
// on gfx950, 64-bit VALU pointer adds would come straight out of the matrix issue time.
// Resource words: stride 0, 0x7ffffffe bytes addressable, raw 32-bit data format.
#pragma once
#include <hip/hip_runtime.h>

namespace anoddpm {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void *base)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, 0x7ffffffe, 0x00020000);
}

// 16 bytes per lane; AUX = cache policy bits of the instruction (0: default, 2: nt, 16: sc1)
template <int AUX = 0>
__device__ __forceinline__ f32x4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned lane_bytes, unsigned wave_bytes)
{
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)lane_bytes, (int)wave_bytes, AUX));
}

}  // namespace anoddpm
