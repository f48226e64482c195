// impc_fov_est.hip — the FoV controller's IMPC launch in the estimate form
// (mpccbf_set_fov_estimates): impc_fov_kernel<SLACK, true> (impc_fov.hpp) reads every neighbour
// position and the slack order's covariances from the per-pair buffers ImpcArgs::est_xy / est_cov.
// A translation unit of its own: see impc_fov.hpp.
#include "impc_fov.hpp"

namespace mpccbf {

hipError_t launch_impc_fov_est(ImpcKernel k, int blocks, int block_size, const DevOps& op, const double* buf,
                               const ImpcArgs& a, hipStream_t s) {
    switch (k) {
        case IMPC_FOV_SLACK_EST:
            return launch_kernel(dev::impc_fov_kernel<true, true>, blocks, block_size, 0, s, op, buf, a);
        case IMPC_FOV_EST:
            return launch_kernel(dev::impc_fov_kernel<false, true>, blocks, block_size, 0, s, op, buf, a);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mpccbf
