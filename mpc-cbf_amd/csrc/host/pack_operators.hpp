// pack_operators.hpp — the operators as the kernels read them: one buffer of doubles and the
// DevOps that holds every offset into it (launch_plan.hip; no HIP runtime call, so the CPU tests
// reach it through mpccbf_host_launch_plan).
#pragma once

#include <vector>

#include "../../../include/mpccbf.h"
#include "../kernels/impc.hpp"
#include "operators.hpp"

namespace mpccbf {

struct PackedOps {
    DevOps dev;               // wide_max is the caller's (it depends on the device)
    int32_t o_EB2;            // the second-derivative basis' offset (the cap audit's)
    std::vector<double> buf;  // [0, dev.hot): the separable collision kernels' operators
};

PackedOps pack_operators(const Operators& o, const mpccbf_params& p, const mpccbf_options& opt);

}  // namespace mpccbf
