// formation_rollout.hip — CBFFormationControl_example.cpp:136-187 for a batch of independent teams,
// in the example's order: one wavefront per team (<= 16 robots), the team's state table in LDS for
// the whole launch.
//
// Per step, per robot i in index order (Gauss-Seidel: robots < i have already moved, :146-177):
//   desired_u = k (target - pos) - 2 sqrt(k) vel        (criticallyDampedSpringControl, Controls.h:18-27)
//   lambda2 / Fiedler vector of the table as it stands  (team_lambda2, all 64 lanes)
//   robot i's QP                                        (conn_robot_qp.hpp; the four 16-lane groups
//                                                        solve the same QP, lane l of each holds row l)
//   u = 0 unless OPTIMAL (:168-172); pos += Ts vel + Ts^2 u / 2, vel += Ts u
//   (DoubleIntegratorXYYaw.cpp:14-20); + pos_std / vel_std normal_sample(team seed, absolute step, i,
//   component) (:176); the row goes back into the table before robot i + 1 plans (:177).
// After the last robot the table is sample step_first + s: it goes to the trace and is scored as
// collision_check.py scores a states.json (first arrival per robot, first colliding pair under the
// box test, smallest squared pair distance), so a Monte-Carlo run needs no trace.
//
// Lanes: every lane runs every turn (n, i and the statuses are wave-uniform). Lane c < 6 integrates
// component c of robot i's row; lane r < n holds robot r's arrival sample; the pair scan spreads the
// 16 x 16 index pairs over the lanes. Teams share nothing: no barrier beyond the wave's own, no
// atomics, every loop bounded by its argument (steps, robots, the spectrum's sweeps, max_pdip_iters).
//
// Two waves per SIMD (__launch_bounds__(64, 2)): a turn is one latency-bound chain, so a second
// resident wave nearly doubles the throughput once the batch exceeds one wave per SIMD (4,096 teams
// of 8: 4.1 against 6.3 ms a step), for 400 - 448 bytes a lane of scratch and 2 % at smaller batches
// (DESIGN section 4).
#include <hip/hip_runtime.h>

#include <cmath>

#include "cbf_control.hpp"
#include "conn_robot_qp.hpp"
#include "conn_spectrum.hpp"

namespace mpccbf {
namespace dev {

struct FormationLds {
    ConnLds conn;
    double tab[CC_MAX * 6];  // the team's state table
    double tgt[CC_MAX * 3];
};

// a team of more than CC_MAX robots: no decision is taken. Every one reports ERROR, its states stay
// and its trace rows copy them
__device__ void formation_oversize(const FormationArgs& a, size_t robots, int r0, int n, int team, int lane) {
    const double nan = __builtin_nan("");
    const double k = a.spring, c = 2.0 * sqrt(a.spring);
    for (int s = 0; s < a.num_steps; s++) {
        const size_t row0 = (size_t)(a.record_first + s) * robots + (size_t)r0;
        for (int i = lane; i < n; i += 64) {
            const size_t ri = (size_t)(r0 + i), ro = row0 + i;
            if (a.status) a.status[ro] = ST_ERROR;
            if (a.iters) a.iters[ro] = 0;
            if (a.lambda2) a.lambda2[ro] = nan;
            for (int d = 0; d < 3; d++) {
                if (a.cbf_u) a.cbf_u[ro * 3 + d] = nan;
                if (a.desired_u)
                    a.desired_u[ro * 3 + d] = k * (a.targets[ri * 3 + d] - a.states[ri * 6 + d]) - c * a.states[ri * 6 + 3 + d];
            }
            if (a.trace)
                for (int d = 0; d < 6; d++) a.trace[ro * 6 + d] = a.states[ri * 6 + d];
        }
    }
    if (lane == 0 && a.fail_count) a.fail_count[team] += n * a.num_steps;
}

template <bool SLACK>
__global__ void __launch_bounds__(64, 2) formation_rollout_kernel(const FormationArgs a) {
    constexpr int G = 16, NZ = 3;
    const int lane = threadIdx.x;
    const int team = blockIdx.x;
    if (team >= a.num_teams) return;
    const int r0 = a.team_ptr[team], n = a.team_ptr[team + 1] - r0;
    if (n <= 0) return;  // an empty team writes nothing
    const size_t robots = (size_t)a.team_ptr[a.num_teams];  // rows of one sample of the records
    if (n > CC_MAX) {
        formation_oversize(a, robots, r0, n, team, lane);
        return;
    }
    __shared__ FormationLds L;
    for (int e = lane; e < n * 6; e += 64) L.tab[e] = a.states[(size_t)r0 * 6 + e];
    for (int e = lane; e < n * 3; e += 64) L.tgt[e] = a.targets[(size_t)r0 * 3 + e];
    wave_lds_sync();
    const int gl = lane & (G - 1);
    const uint64_t seed = a.team_seed[team];
    const double spring_k = a.spring, spring_c = 2.0 * sqrt(a.spring);
    // the summary so far (calls chain): robot `lane`'s arrival in its lane, the rest wave-uniform
    int arrival = (a.arrival_sample && lane < n) ? a.arrival_sample[r0 + lane] : -1;
    int fc_s = a.first_collision ? a.first_collision[team * 3] : -1;
    int fc_i = a.first_collision ? a.first_collision[team * 3 + 1] : -1;
    int fc_j = a.first_collision ? a.first_collision[team * 3 + 2] : -1;
    double min_d2 = a.min_d2 ? a.min_d2[team] : __builtin_inf();
    int fails = a.fail_count ? a.fail_count[team] : 0;
    const double goal_r = a.goal_radius;
    const bool pairs = a.first_collision || a.min_d2;  // the pair scan's outputs
    const double hx = a.half_x / 2, hy = a.half_y / 2, wx = 2 * a.half_x, wy = 2 * a.half_y;

    for (int s = 0; s < a.num_steps; s++) {
        const int64_t step = a.step_first + s;
        const size_t row0 = (size_t)(a.record_first + s) * robots + (size_t)r0;
        for (int i = 0; i < n; i++) {
            if (lane < CC_MAX) {
                L.conn.pos[lane][0] = lane < n ? L.tab[lane * 6] : 0.0;
                L.conn.pos[lane][1] = lane < n ? L.tab[lane * 6 + 1] : 0.0;
            }
            wave_lds_sync();
            team_lambda2(L.conn, n, a.qp.dmax, lane);
            const double l2 = L.conn.l2;
            double udes[NZ], y[NZ];
#pragma unroll
            for (int d = 0; d < NZ; d++)
                udes[d] = spring_k * (L.tgt[i * 3 + d] - L.tab[i * 6 + d]) - spring_c * L.tab[i * 6 + 3 + d];
            const ConnQpOut qo = conn_robot_qp<SLACK>(a.qp, L.tab, 0, L.conn.ev, l2, n, i, gl, udes, y);
            const bool ok = qo.status == ST_OPTIMAL;
            fails += ok ? 0 : 1;
            // lane c < 6: component c of the row (c < 3 position, else velocity) and its control
            double uc = 0.0, dc = 0.0;
#pragma unroll
            for (int d = 0; d < NZ; d++)
                if (d == lane || d + 3 == lane) {
                    uc = ok ? y[d] : 0.0;
                    dc = udes[d];
                }
            double v = 0.0;
            if (lane < 6) {
                v = L.tab[i * 6 + lane];
                if (lane < 3)
                    v = v + a.Ts * L.tab[i * 6 + 3 + lane] + 0.5 * a.Ts * a.Ts * uc;
                else
                    v = v + a.Ts * uc;
                const double sd = lane < 3 ? a.pos_std : a.vel_std;
                if (sd > 0.0) v = v + sd * normal_sample(seed, step, i, lane);
            }
            wave_lds_sync();  // every lane has read the table it planned from
            if (lane < 6) L.tab[i * 6 + lane] = v;
            wave_lds_sync();
            const size_t ro = row0 + i;
            if (lane < 3) {
                if (a.cbf_u) a.cbf_u[ro * 3 + lane] = uc;
                if (a.desired_u) a.desired_u[ro * 3 + lane] = dc;
            }
            if (lane == 0) {
                if (a.status) a.status[ro] = qo.status;
                if (a.iters) a.iters[ro] = qo.iters;
                if (a.lambda2) a.lambda2[ro] = l2;
            }
        }
        // the table is sample `step`
        if (a.trace)
            for (int e = lane; e < n * 6; e += 64) a.trace[row0 * 6 + e] = L.tab[e];
        // goal area (collision_check.py:44-46: the planar norm, products and sum rounded one by one)
        if (a.arrival_sample && lane < n && arrival < 0) {
            const double dx = L.tab[lane * 6] - L.tgt[lane * 3], dy = L.tab[lane * 6 + 1] - L.tgt[lane * 3 + 1];
            if (sqrt(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy))) <= goal_r) arrival = (int)step;
        }
        if (!pairs) continue;  // (launch-uniform: neither pair output is asked for)
        // pairs p < q: the script's box test (:11-20, 28-39: corner = centre - half / 2, extent 2 half,
        // strict comparisons) and the squared distance
        unsigned hit = 0u;  // 256 - (p * 16 + q) of this lane's first colliding pair, 0 = none
        double d2min = __builtin_inf();
        for (int e = lane; e < CC_MAX * CC_MAX; e += 64) {
            const int p = e / CC_MAX, q = e % CC_MAX;
            if (p < q && q < n) {
                const double x1 = L.tab[p * 6], y1 = L.tab[p * 6 + 1], x2 = L.tab[q * 6], y2 = L.tab[q * 6 + 1];
                const double xa = x1 - hx, ya = y1 - hy, xb = x2 - hx, yb = y2 - hy;
                const bool c = (xa < xb + wx) && (xa + wx > xb) && (ya < yb + wy) && (ya + wy > yb);
                if (c) hit = max(hit, (unsigned)(CC_MAX * CC_MAX - e));
                const double dx = x1 - x2, dy = y1 - y2;
                d2min = fmin(d2min, __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
            }
        }
        hit = wave_max_u32(hit);
        min_d2 = fmin(min_d2, grp_min<64>(d2min));
        if (hit != 0u && fc_s < 0) {
            const int e = CC_MAX * CC_MAX - (int)hit;
            fc_s = (int)step;
            fc_i = e / CC_MAX;
            fc_j = e % CC_MAX;
        }
    }
    for (int e = lane; e < n * 6; e += 64) a.states[(size_t)r0 * 6 + e] = L.tab[e];
    if (a.arrival_sample && lane < n) a.arrival_sample[r0 + lane] = arrival;
    if (lane == 0) {
        if (a.first_collision) {
            a.first_collision[team * 3] = fc_s;
            a.first_collision[team * 3 + 1] = fc_i;
            a.first_collision[team * 3 + 2] = fc_j;
        }
        if (a.min_d2) a.min_d2[team] = min_d2;
        if (a.fail_count) a.fail_count[team] = fails;
    }
}

}  // namespace dev

hipError_t launch_formation_rollout(const FormationArgs& a, hipStream_t s) {
    if (a.num_teams <= 0 || a.num_steps <= 0) return hipSuccess;
    if (a.qp.slack_mode)
        hipLaunchKernelGGL(dev::formation_rollout_kernel<true>, dim3(a.num_teams), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL(dev::formation_rollout_kernel<false>, dim3(a.num_teams), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace mpccbf
