// Instantiations of the fused row-streaming pass for the Op5P operator policy (see fused_kernel.h): a constant 5-point
// operator plus a per-point diagonal, weighted Jacobi and red-black, every mode of launch_variant (plain, zero-in,
// restrict, no-store, prolong, recompute).
#include "fused_kernel.h"

namespace mgcmt {

void launch_fused_op5p(hipStream_t s, const fused::FusedArgs& a, int multicolour, int nsweep, int flags, int k) {
  using namespace fused;
  if (multicolour) {
    if (nsweep == 1) launch_variant<Op5P, kRedBlack, 1>(s, a, flags, k);
    else launch_variant<Op5P, kRedBlack, 2>(s, a, flags, k);
  } else {
    if (nsweep == 1) launch_variant<Op5P, kJacobi, 1>(s, a, flags, k);
    else launch_variant<Op5P, kJacobi, 2>(s, a, flags, k);
  }
}

}  // namespace mgcmt
