// impc_store.hip — the launches of the active-set store's kernels (impc_sep_store_kernel:
// impc_sep.hpp; impc_wide_store_kernel: impc_wide_kernels.hpp), instantiated in a translation unit
// of their own, so that the object code of the kernels launched without a store does not depend on
// them ("Why separate translation units").
#include "impc_sep.hpp"
#include "impc_wide_kernels.hpp"
#include "launch_plan.hpp"

namespace mpccbf {

hipError_t launch_impc_store(ImpcKernel k, int blocks, int block_size, const DevOps& op, const double* buf,
                             const ImpcArgs& a, const StoreArgs& st, hipStream_t s) {
    auto go = [&](auto kernel) { return launch_kernel(kernel, blocks, block_size, 0, s, op, buf, a, st); };
    switch (k) {
        case IMPC_SEP_STORE: return go(dev::impc_sep_store_kernel<1, 256, false>);
        case IMPC_QUEUE1_STORE: return go(dev::impc_sep_store_kernel<1, 64, true>);
        case IMPC_QUEUE8_STORE: return go(dev::impc_sep_store_kernel<8, 64, true>);
        case IMPC_WIDE_STORE: return go(dev::impc_wide_store_kernel<256>);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mpccbf
