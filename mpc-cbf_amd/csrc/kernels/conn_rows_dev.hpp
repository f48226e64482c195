// conn_rows_dev.hpp — the device half of the connectivity-maintenance rows (conn_rows.hpp: the
// rows' definition and the kernel arguments): stage_conn_rows, which impc_sep_agent<.., CONN>
// calls to stage a team's rows behind the agent's safety rows.
#pragma once

#include "conn_rows.hpp"
#include "impc_common.hpp"

namespace mpccbf {
namespace dev {

// One planar row c^T (US_k s0 + UZ_k y) <= bb against the acceleration box at sample k: whether it
// is kept (the box does not imply it) and whether no acceleration satisfies it (the safety rows'
// rule, stage_cbf_rows).
__device__ __forceinline__ bool conn_row_keep(const DevOps& op, double c0, double c1, double bb, bool& infeasible) {
    const double x1 = c0 * op.a_lo[0], x2 = c0 * op.a_hi[0], y1 = c1 * op.a_lo[1], y2 = c1 * op.a_hi[1];
    const double bmax = fmax(x1, x2) + fmax(y1, y2), bmin = fmin(x1, x2) + fmin(y1, y2);
    if (bb < bmin - op.feas_tol) infeasible = true;
    return !(op.cbf_filter && bb >= bmax);
}

template <int NZ>
__device__ __forceinline__ void conn_row_write(lds_vptr<double> dst, const double* UZk, const double (&us)[3], double c0,
                                               double c1, double bb) {
#pragma unroll
    for (int jz = 0; jz < NZ; jz++) dst[jz] = c0 * UZk[jz] + c1 * UZk[NZ + jz];
    dst[NZ] = bb - (c0 * us[0] + c1 * us[1]);
}

// The connectivity rows of state row `self` for IMPC iteration `it`, appended to the `count` safety
// rows already staged (16-lane group; lane l takes member l of the team). Returns the new count
// (cap + 1 for a team beyond 16 members: the agent reports ERROR); *infeasible is or-ed.
template <int NZ>
__device__ int stage_conn_rows(const DevOps& op, const double* buf, const ImpcArgs& args, const ConnArgs& cn, int self,
                               int it, const double (&s0)[6], const double (&y)[NZ], double* stage, int cap, int count,
                               int gl, bool* infeasible) {
    constexpr int G = 16;
    const int team = cn.row_team[self];
    if (team < 0) return count;  // (group-uniform)
    const int mode = cn.team_mode[team];
    if (mode < 0) return cap + 1;
    const int r0 = cn.team_ptr[team], n = cn.team_ptr[team + 1] - r0;
    const bool has = gl < n && r0 + gl != self;
    double px = 0.0, py = 0.0, evj = 0.0;
    if (has) {
        px = args.states[(size_t)(r0 + gl) * 6];
        py = args.states[(size_t)(r0 + gl) * 6 + 1];
        evj = cn.fiedler[r0 + gl];
    }
    const double evs = cn.fiedler[self], l2 = cn.team_l2[team];
    const double Rs2 = cn.dmax * cn.dmax, sigma = Rs2 * Rs2 / 0.69314718055994530942;
    const double* UZ = opp(buf, op.o_UZ);
    const double* US = opp(buf, op.o_US);
    const int nk = (it == 0) ? 1 : op.cbf_h;
    bool row_infeasible = false;
    for (int k = 0; k < nk; k++) {
        double e[6];
        cbf_ego_state<NZ>(op, buf, it, k, s0, y, e);
        const double* UZk = UZ + (size_t)k * 3 * NZ;
        const double* USk = US + (size_t)k * 18;
        double us[3];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            double v = 0.0;
#pragma unroll
            for (int s = 0; s < 6; s++) v = fma(USk[d * 6 + s], s0[s], v);
            us[d] = v;
        }
        const double dx = e[0] - px, dy = e[1] - py, vx = e[3], vy = e[4];
        if (mode == 1) {
            // gradient and Hessian of lambda2 over the ego position, Fiedler entries held fixed,
            // summed over every other member (ConnectivityCBF.cpp:430-512)
            double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            if (has) {
                const double diff = Rs2 - (dx * dx + dy * dy);
                const double E = exp(diff * diff / sigma);
                const double dev = evs - evj;
                const double kk = -4.0 * dev * dev / sigma;
                t[0] = kk * E * diff * dx;
                t[1] = kk * E * diff * dy;
                t[2] = kk * (-4.0 * E * diff * diff * dx * dx / sigma - 2.0 * E * dx * dx + E * diff);
                t[3] = kk * (-4.0 * E * diff * diff * dx * dy / sigma - 2.0 * E * dx * dy);
                t[4] = kk * (-4.0 * E * diff * diff * dy * dy / sigma - 2.0 * E * dy * dy + E * diff);
            }
            grp_sum_vec<G, 5>(t);
            const double lfh = t[0] * vx + t[1] * vy;
            const double lf2h = vx * (t[2] * vx + t[3] * vy) + vy * (t[3] * vx + t[4] * vy);
            const double b = lf2h + 5.0 * lfh + 5.0 * (lfh + 5.0 * (l2 - cn.l2_min));
            // row: -g^T U_k x <= b
            const bool keep = conn_row_keep(op, -t[0], -t[1], b, row_infeasible);
            if (keep && count < cap && gl == 0)
                conn_row_write<NZ>(lds_vol(stage) + count * (NZ + 1), UZk, us, -t[0], -t[1], b);
            count += keep ? 1 : 0;
        } else {
            // CLF row of this lane's member: V = (|p - p_j| - 2)^2, +grad V^T U_k x <= -B
            bool keep = false;
            double gx = 0.0, gy = 0.0, bb = 0.0;
            if (has) {
                const double dist = sqrt(dx * dx + dy * dy), ee = dist - 2.0;
                gx = 2.0 * ee * dx / dist;
                gy = 2.0 * ee * dy / dist;
                const double lfv = gx * vx + gy * vy, dv = (dx * vx + dy * vy) / dist;
                const double lf2v = 2.0 * dv * dv + 2.0 * ee * (vx * vx + vy * vy - dv * dv) / dist;
                bb = -(lf2v + 5.0 * lfv + 2.0 * ee * ee);
                keep = conn_row_keep(op, gx, gy, bb, row_infeasible);
            }
            const unsigned long long msk = grp_ballot<G>(keep);
            const int slot = count + __popcll(msk & ((1ull << gl) - 1ull));
            if (keep && slot < cap) conn_row_write<NZ>(lds_vol(stage) + slot * (NZ + 1), UZk, us, gx, gy, bb);
            count += __popcll(msk);
        }
    }
    if (grp_ballot<G>(row_infeasible) != 0ull) *infeasible = true;
    wave_lds_sync();
    return count;
}

}  // namespace dev
}  // namespace mpccbf
