// k_sep2s instantiations with 32-frame tiles: k_sep2's production kernels with the mask-skip rule (see qasr_sep2_impl.h)
#include "qasr_sep2_impl.h"

namespace qasr {
template int launch_sep2_inst<32, false, true>(hipStream_t, const SepP&);
}  // namespace qasr
