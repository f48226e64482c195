// conn_robot_qp.hpp — one robot's QP of ConnectivityControl::optimize
// (cbf/src/controller/ConnectivityControl.cpp:22-99) on a 16-lane group: row formation, the PDIP
// calls and the status logic, once for the batched solve (connectivity_control.hip: four robots of
// a team per pass, the table in global memory) and the rollout (formation_rollout.hip: one robot
// per turn, the table in LDS).
//
//   min ||u - u_des||^2  s.t.  safety rows vs every other robot (:49-55, cubic alpha, gamma 5),
//   velocity CBFs (:58-59), and either the lambda2 connectivity row (lambda2 > 0.1, :70-71,
//   ConnectivityQPGenerator.cpp:13-44) or the per-neighbour CLF rows (:72-82; :47-69); u is free
//   (addControlBoundConstraint is commented out, :60). Lane l holds neighbour l's safety row and
//   CLF row; the connectivity row's gradient and Hessian terms are summed over the lanes.
//   Slack mode: lane l's slack relaxes its safety and CLF rows, lane N-1's the connectivity
//   row, weights slack_cost * decay^l (:31-38) — solved by pdip_slack_lane.hpp; without slack
//   by the group PDIP of pdip.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "cbf_control.hpp"
#include "group.hpp"
#include "impc_common.hpp"
#include "pdip.hpp"
#include "pdip_slack_lane.hpp"

namespace mpccbf {
namespace dev {

struct ConnQpOut {
    int status, iters;
    double vcost;  // slack mode: the slack variables' cost at the solution
};

// Robot `self` of a team of n (2 <= n <= 16, or 1: velocity rows alone) on the group's 16 lanes (gl
// = the lane in its group; every lane of the group calls with the same other arguments).
// tab: a state table (rows x 6) whose rows row0 .. row0 + n - 1 are the team as this robot sees it;
// ev / l2: the unit Fiedler vector and lambda2 of the team's positions (team_lambda2); udes: the
// desired control (3). y: the solution (meaningful when the status is ST_OPTIMAL).
template <bool SLACK>
__device__ __forceinline__ ConnQpOut conn_robot_qp(const ConnQpParams& a, const double* tab, int row0,
                                                   const double* ev, double l2, int n, int self, int gl,
                                                   const double* udes, double (&y)[3]) {
    constexpr int G = 16, NZ = 3;
    const bool conn = l2 > 0.1;  // ConnectivityControl.cpp:69 (threshold 0.1)
    const double Rs2 = a.dmax * a.dmax, sigma = Rs2 * Rs2 / 0.69314718055994530942;
    const size_t ri = (size_t)(row0 + self);
    double st[6];
#pragma unroll
    for (int k = 0; k < 6; k++) st[k] = tab[ri * 6 + k];
    // neighbour l of this lane (the reference's order: other robots by index, :49-55)
    const bool has_nb = gl < n - 1;
    const int j = gl + (gl >= self ? 1 : 0);
    double nb[6] = {0, 0, 0, 0, 0, 0};
    if (has_nb) {
#pragma unroll
        for (int k = 0; k < 6; k++) nb[k] = tab[(size_t)(row0 + j) * 6 + k];
    }
    // safety row: -Ac u <= Bc
    double sa[3] = {0, 0, 0}, sb = 1.0;
    if (has_nb) {
        double ac[3], bc;
        safety_cbf(st, nb[0], nb[1], nb[3], nb[4], a.dmin, ac, bc);
        sa[0] = -ac[0];
        sa[1] = -ac[1];
        sa[2] = -ac[2];
        sb = bc;
    }
    // connectivity row (grad / Hessian of lambda2 over the self position, summed over the
    // lanes: lane gl takes robot j, ConnectivityCBF.cpp:430-512) or this lane's CLF row
    double ca[3] = {0, 0, 0}, cb = 1.0;
    bool clive = false;
    if (conn) {
        double t[5] = {0, 0, 0, 0, 0};
        if (has_nb) {
            const double dx = st[0] - nb[0], dy = st[1] - nb[1];
            const double diff = Rs2 - (dx * dx + dy * dy);
            const double E = exp(diff * diff / sigma);
            const double dev = ev[self] - ev[j];
            const double k = -4.0 * dev * dev / sigma;
            t[0] = k * E * diff * dx;
            t[1] = k * E * diff * dy;
            t[2] = k * (-4.0 * E * diff * diff * dx * dx / sigma - 2.0 * E * dx * dx + E * diff);
            t[3] = k * (-4.0 * E * diff * diff * dx * dy / sigma - 2.0 * E * dx * dy);
            t[4] = k * (-4.0 * E * diff * diff * dy * dy / sigma - 2.0 * E * dy * dy + E * diff);
        }
        grp_sum_vec<G, 5>(t);
        const double vx = st[3], vy = st[4];
        const double lfh = t[0] * vx + t[1] * vy;
        const double lf2h = vx * (t[2] * vx + t[3] * vy) + vy * (t[3] * vx + t[4] * vy);
        const double hh = l2 - 0.1;
        const int owner = SLACK ? n - 1 : 0;  // slack mode: the last slack variable
        if (gl == owner) {
            ca[0] = -t[0];
            ca[1] = -t[1];
            cb = lf2h + 5.0 * lfh + 5.0 * (lfh + 5.0 * hh);
            clive = true;
        }
    } else if (has_nb) {  // CLF: +Ac u <= -Bc
        const double dx = st[0] - nb[0], dy = st[1] - nb[1];
        const double dist = sqrt(dx * dx + dy * dy), e = dist - 2.0;
        const double gx = 2.0 * e * dx / dist, gy = 2.0 * e * dy / dist;
        const double vx = st[3], vy = st[4];
        const double lfv = gx * vx + gy * vy, dv = (dx * vx + dy * vy) / dist;
        const double lf2v = 2.0 * dv * dv + 2.0 * e * (vx * vx + vy * vy - dv * dv) / dist;
        ca[0] = gx;
        ca[1] = gy;
        cb = -(lf2v + 5.0 * lfv + 2.0 * e * e);
        clive = true;
    }
    // velocity CBF row of lanes 0..5: -u_d <= v_d - vmin_d, u_d <= vmax_d - v_d
    double og[3] = {0, 0, 0}, ohi = 1.0, olo = -1.0, oml = 1.0;
    if (gl < 3) {
        og[gl] = -1.0;
        ohi = st[3 + gl] - a.vmin[gl];
        olo = 0.0;
        oml = 0.0;
    } else if (gl < 6) {
        og[gl - 3] = 1.0;
        ohi = a.vmax[gl - 3] - st[gl];
        olo = 0.0;
        oml = 0.0;
    }
    double q[NZ];
#pragma unroll
    for (int d = 0; d < NZ; d++) {
        y[d] = 0.0;
        q[d] = -2.0 * udes[d];
    }
    const PdipCfg cfg{a.maxit, a.tol};
    ConnQpOut out{ST_UNKNOWN, 0, 0.0};
    if constexpr (SLACK) {
        double g[2][3], h[2], live[2];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            g[0][d] = sa[d];
            g[1][d] = ca[d];
        }
        h[0] = sb;
        h[1] = cb;
        live[0] = has_nb ? 1.0 : 0.0;
        live[1] = clive ? 1.0 : 0.0;
        if (!clive) {
            g[1][0] = g[1][1] = g[1][2] = 0.0;
            h[1] = 1.0;
        }
        const bool son = gl < n;  // N slack variables (CBFQPGeneratorBase.cpp:20-27)
        const double w = son ? a.slack_cost * pow(a.slack_decay, (double)gl) : 0.0;
        Rows<NZ, 1> orw;
#pragma unroll
        for (int d = 0; d < 3; d++) orw.g[0][d] = og[d];
        orw.lo[0] = olo;
        orw.hi[0] = ohi;
        orw.ml[0] = oml;
        orw.mu[0] = 1.0;
        const SlackLaneOut so = pdip_slack_lane<2, G>(g, h, live, son, w, orw, q, y, cfg, a.feas_tol);
        out.status = so.status;
        out.iters = so.iters;
        out.vcost = so.vcost;
    } else {
        Rows<NZ, 3> rw;
#pragma unroll
        for (int d = 0; d < 3; d++) {
            rw.g[0][d] = has_nb ? sa[d] : 0.0;
            rw.g[1][d] = clive ? ca[d] : 0.0;
            rw.g[2][d] = og[d];
        }
        rw.lo[0] = has_nb ? 0.0 : -1.0;
        rw.hi[0] = has_nb ? sb : 1.0;
        rw.ml[0] = has_nb ? 0.0 : 1.0;
        rw.mu[0] = 1.0;
        rw.lo[1] = clive ? 0.0 : -1.0;
        rw.hi[1] = clive ? cb : 1.0;
        rw.ml[1] = clive ? 0.0 : 1.0;
        rw.mu[1] = 1.0;
        rw.lo[2] = olo;
        rw.hi[2] = ohi;
        rw.ml[2] = oml;
        rw.mu[2] = 1.0;
        const double LP[9] = {1.4142135623730951, 0, 0, 0, 1.4142135623730951, 0, 0, 0, 1.4142135623730951};
        const double P[9] = {2, 0, 0, 0, 2, 0, 0, 0, 2};
        const PdipOut po = pdip_solve<NZ, G, 3>(rw, P, LP, q, y, cfg);
        out.status = po.status;
        out.iters = po.iters;
        if (out.status != ST_OPTIMAL) {
            const double tstar = pdip_phase1<NZ, G, 3>(rw, cfg);
            out.status = (tstar > a.feas_tol && tstar < 1e300) ? ST_INFEASIBLE : ST_UNKNOWN;
        }
    }
    return out;
}

}  // namespace dev
}  // namespace mpccbf
