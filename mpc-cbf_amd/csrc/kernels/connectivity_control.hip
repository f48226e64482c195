// connectivity_control.hip — ConnectivityControl::optimize (cbf/src/controller/ConnectivityControl.cpp:22-99)
// for a batch of robot teams: one wavefront per team (<= 16 robots).
//
// Phase 1 (per team, all 64 lanes): the weighted Laplacian of the team's planar positions
// (ConnectivityCBF::getLambda2, ConnectivityCBF.cpp:375-414: A_ij = exp((Rs^2 - d^2)^2 / sigma) - 1
// within Rs = d_max, sigma = d_max^4 / ln 2) in LDS, diagonalised by a parallel cyclic Jacobi
// sweep (round-robin pairing: the N/2 rotations of a round touch disjoint rows / columns, so a
// round is two passes over (pair, column) tasks) to machine precision; lambda2 and the unit
// Fiedler vector are what every robot's connectivity row needs.
// Phase 2 (per robot, one 16-lane group each, 4 robots at a time): the CBF-only QP over u (3) of
// conn_robot_qp.hpp (row formation, the PDIP calls and the status logic, shared with
// formation_rollout.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "cbf_control.hpp"
#include "conn_robot_qp.hpp"
#include "conn_spectrum.hpp"

namespace mpccbf {
namespace dev {

template <bool SLACK>
__global__ void __launch_bounds__(64) connectivity_control_kernel(const ConnControlArgs a) {
    constexpr int G = 16, NZ = 3;
    const int lane = threadIdx.x;
    const int team = blockIdx.x;
    if (team >= a.num_teams) return;
    __shared__ ConnLds L;
    const int r0 = a.team_ptr[team], n = a.team_ptr[team + 1] - r0;
    const bool cap_ok = n >= 1 && n <= CC_MAX;
    if (lane < CC_MAX) {
        L.pos[lane][0] = (cap_ok && lane < n) ? a.states[(size_t)(r0 + lane) * 6] : 0.0;
        L.pos[lane][1] = (cap_ok && lane < n) ? a.states[(size_t)(r0 + lane) * 6 + 1] : 0.0;
    }
    wave_lds_sync();
    if (cap_ok) team_lambda2(L, n, a.qp.dmax, lane);
    const double l2 = cap_ok ? L.l2 : 0.0;
    if (lane == 0 && a.lambda2) a.lambda2[team] = cap_ok ? l2 : __builtin_nan("");
    const int gi = lane / G, gl = lane & (G - 1);
    for (int pass = 0; pass < CC_MAX / 4; pass++) {
        const int self = gi + 4 * pass;
        if (!cap_ok || self >= n) continue;  // group-uniform
        const size_t ri = (size_t)(r0 + self);
        double y[NZ];
        const ConnQpOut qo = conn_robot_qp<SLACK>(a.qp, a.states, r0, L.ev, l2, n, self, gl, a.desired_u + ri * 3, y);
        const int status = qo.status, iters = qo.iters;
        const double vcost = qo.vcost;
        const bool ok = status == ST_OPTIMAL;
        if (gl < NZ) {
            double uv = __builtin_nan("");
#pragma unroll
            for (int d = 0; d < NZ; d++)
                if (d == gl && ok) uv = y[d];
            a.u[ri * 3 + gl] = uv;
        }
        if (gl == 0) {
            if (a.status) a.status[ri] = status;
            if (a.iters) a.iters[ri] = iters;
            if (a.obj) {
                double o = 0.0;
#pragma unroll
                for (int d = 0; d < NZ; d++) {
                    const double e = y[d] - a.desired_u[ri * 3 + d];
                    o = fma(e, e, o);
                }
                a.obj[ri] = ok ? o + vcost : __builtin_nan("");
            }
        }
    }
    if (!cap_ok) {  // team size out of range: every robot of it ERROR
        for (int i = lane; i < n; i += 64) {
            const size_t ri = (size_t)(r0 + i);
            if (a.status) a.status[ri] = ST_ERROR;
            if (a.iters) a.iters[ri] = 0;
            if (a.obj) a.obj[ri] = __builtin_nan("");
            for (int d = 0; d < NZ; d++) a.u[ri * 3 + d] = __builtin_nan("");
        }
    }
}

}  // namespace dev

hipError_t launch_connectivity_control(const ConnControlArgs& a, hipStream_t s) {
    if (a.num_teams <= 0) return hipSuccess;
    if (a.qp.slack_mode)
        hipLaunchKernelGGL(dev::connectivity_control_kernel<true>, dim3(a.num_teams), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL(dev::connectivity_control_kernel<false>, dim3(a.num_teams), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace mpccbf
