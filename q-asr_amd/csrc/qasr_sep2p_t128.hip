// k_sep2p: the paired form of the plain 512 -> 512 layers at 128 frames (see qasr_sep2_impl.h)
#include "qasr_sep2_impl.h"

namespace qasr {
// flag words back to zero (16-byte granules): a kernel node of its own in front of the forward's first kernel
__global__ void __launch_bounds__(256) k_pair_zero(v4u* __restrict__ w, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) w[i] = (v4u){0u, 0u, 0u, 0u};
}
int launch_pair_zero(hipStream_t s, unsigned* flags, size_t bytes) {
  if (!flags || bytes == 0 || bytes % 16 || ((uintptr_t)flags & 15)) return QASR_ERR_ARG;
  const int n = (int)(bytes / 16);
  hipLaunchKernelGGL(k_pair_zero, dim3((n + 255) / 256), dim3(256), 0, s, (v4u*)flags, n);
  return QASR_OK;
}

int launch_sep2_pair(hipStream_t s, const SepP& p) {
  if (!sep2_pair_shape(p)) return QASR_ERR_UNSUPPORTED;
  return p.K == 51 ? launch_sep2_pair_v<51>(s, p) : p.K == 63 ? launch_sep2_pair_v<63>(s, p) : launch_sep2_pair_v<75>(s, p);
}
}  // namespace qasr
