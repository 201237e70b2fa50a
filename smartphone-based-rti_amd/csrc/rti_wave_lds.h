// rti_wave_lds.h -- the fence between the phases of a wave's private LDS slab, for the kernels in which a wave
// stages its own rows through LDS and no other wave reads them (rti_lane4.h, rti_hsh_px.h).
#pragma once

#include <hip/hip_runtime.h>

namespace rti {
namespace lds {

// what the wave wrote to its slab is visible to its other lanes; no workgroup barrier
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace lds
}  // namespace rti
