// impc_store.hip — the active-set store's kernels (impc_sep_store_kernel, impc_wide_store_kernel:
// impc_kernel.hip) and their launches, a translation unit of their own, so that the object code of
// the kernels launched without a store does not depend on them.
#define MPCCBF_STORE_TU
#include "impc_kernel.hip"
