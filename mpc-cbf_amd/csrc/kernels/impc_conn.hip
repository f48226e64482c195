// impc_conn.hip — the batched IMPC with connectivity-maintenance rows (mpccbf_set_connectivity):
// the per-team spectrum launch (team_spectrum_kernel) and the IMPC launch that stages the rows
// (impc_sep_conn_kernel: impc_sep.hpp, conn_rows_dev.hpp). A translation unit of its own, as
// impc_store.hip, so that the object code of the kernels launched without connectivity does not
// depend on it ("Why separate translation units").
#include "impc_sep.hpp"
#include "conn_spectrum.hpp"
#include "launch_plan.hpp"

namespace mpccbf {
namespace dev {

// One wave64 per team: the weighted Laplacian of the team's planar positions in LDS, diagonalised
// by team_lambda2's parallel cyclic Jacobi; lambda2, the mode and the Fiedler entry of every state
// row of the team into the context's tables (ConnArgs) and the caller's outputs.
__global__ void __launch_bounds__(64) team_spectrum_kernel(const SpectrumArgs a) {
    const int lane = threadIdx.x;
    const int team = blockIdx.x;
    if (team >= a.num_teams) return;
    __shared__ ConnLds L;
    const int r0 = a.team_ptr[team], n = a.team_ptr[team + 1] - r0;
    if (n <= 0 || r0 + n <= a.first || r0 >= a.first + a.count) return;  // no agent of this launch
    const bool cap_ok = n <= CC_MAX;
    const int base = a.team_ptr[0];
    if (!cap_ok) {  // more than 16 members: its agents report ERROR (stage_conn_rows)
        if (lane == 0) {
            a.team_l2[team] = __builtin_nan("");
            a.team_mode[team] = -1;
            if (a.out_l2) a.out_l2[team] = __builtin_nan("");
        }
        for (int i = lane; i < n; i += 64) {
            a.fiedler[r0 + i] = __builtin_nan("");
            if (a.out_fiedler) a.out_fiedler[r0 - base + i] = __builtin_nan("");
        }
        return;
    }
    const lds_vptr<double> pos = lds_vol(&L.pos[0][0]);
    if (lane < CC_MAX) {
        pos[2 * lane] = lane < n ? a.states[(size_t)(r0 + lane) * 6] : 0.0;
        pos[2 * lane + 1] = lane < n ? a.states[(size_t)(r0 + lane) * 6 + 1] : 0.0;
    }
    wave_lds_sync();
    team_lambda2<26>(L, n, a.dmax, lane);
    const double l2 = *lds_vol(&L.l2);
    if (lane == 0) {
        a.team_l2[team] = l2;
        a.team_mode[team] = l2 > a.l2_switch ? 1 : 0;
        if (a.out_l2) a.out_l2[team] = l2;
    }
    if (lane < n) {
        const double v = lds_vol(&L.ev[0])[lane];
        a.fiedler[r0 + lane] = v;
        if (a.out_fiedler) a.out_fiedler[r0 - base + lane] = v;
    }
}

}  // namespace dev

hipError_t launch_team_spectrum(const SpectrumArgs& a, hipStream_t s) {
    if (a.num_teams <= 0 || a.count <= 0) return hipSuccess;
    hipLaunchKernelGGL(dev::team_spectrum_kernel, dim3(a.num_teams), dim3(64), 0, s, a);
    return hipGetLastError();
}

// (4 CBF row slots per lane: a full team of 16 at cbf_horizon 2 has 30 safety and 30 CLF rows)
hipError_t launch_impc_conn(ImpcKernel k, int blocks, int block_size, const DevOps& op, const double* buf,
                            const ImpcArgs& a, const ConnArgs& cn, hipStream_t s) {
    if (k != IMPC_CONN) return hipErrorInvalidValue;
    return launch_kernel(dev::impc_sep_conn_kernel<4, 64>, blocks, block_size, 0, s, op, buf, a, cn);
}

}  // namespace mpccbf
