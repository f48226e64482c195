// team_rollout.hip — MPCCBFFormationControl_example.cpp:131-231 for a batch of independent teams, in
// the example's order: one wavefront per team (<= 16 robots), the grid over teams.
//
// Per step, per robot i in index order (Gauss-Seidel: robots < i have already moved, :140, :201) the
// wave runs one agent of the dense 64 x 4 layout (impc_dense_agent<6, 64, 4>, the body of
// impc_kernel<6,64,4>): robot i against every other robot of the team, read from the team's table as
// it stands; both IMPC iterations; then write_agent_outputs' simulator semantics (kept curve, traj_t,
// the sub-steps, the hold-position fallback, the counter-based noise keyed by the team's seed, the
// absolute step and the robot's index in its team). The agent is handed a per-turn ImpcArgs whose
// pointers select the team's rows, so it is the code of the per-robot launch, not a copy.
//
// The table is the team's rows of `states` in global memory: robot i's new row is written in place
// by lanes 0 .. 5 and read by all lanes at the next turn, the kept curve and traj_t likewise by other
// lanes of a later step. Every such hand-over stays inside the one wave (one CU, one L1): team_sync()
// (a workgroup-scope release, the wave barrier, a workgroup-scope acquire) waits for the stores and
// keeps the compiler from moving a load above them. The operators (`buf`) are never written: they
// alone are __restrict__ and may take the scalar path.
//
// After the last robot of a step the step's nsub sub-step samples of every robot (the rows the
// example writes to states.json, sample step * nsub + k) are scored as collision_check.py scores a
// states.json, with formation_rollout.hip's comparisons: first arrival per robot, first colliding
// pair under the box test, smallest squared pair distance. Teams share nothing: no atomics, every
// loop bounded by an argument (steps, robots, nsub, impc_iter, max_pdip_iters).
#include <hip/hip_runtime.h>

#include <cmath>

#include "impc_dense.hpp"
#include "team_rollout.hpp"

namespace mpccbf {
namespace dev {

// what one lane stored to global memory, visible to the other lanes of the wave
__device__ __forceinline__ void team_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// a team of more than TEAM_MAX robots: no decision is taken. Every one reports ERROR (later
// iterations UNKNOWN, as after any failed iteration), its states stay, its sub-step and trace rows
// copy them
__device__ void team_oversize(const DevOps& op, const TeamRolloutArgs& a, size_t robots, int r0, int n, int team,
                              int lane) {
    const double nan = __builtin_nan("");
    for (int s = 0; s < a.num_steps; s++) {
        const size_t row0 = (size_t)(a.record_first + s) * robots + (size_t)r0;
        for (int i = lane; i < n; i += 64) {
            const size_t ri = (size_t)(r0 + i), ro = row0 + i;
            for (int it = 0; it < op.impc_iter; it++) {
                if (a.status) a.status[ro * op.impc_iter + it] = it == 0 ? ST_ERROR : ST_UNKNOWN;
                if (a.obj) a.obj[ro * op.impc_iter + it] = nan;
                if (a.iters) a.iters[ro * op.impc_iter + it] = 0;
            }
            if (a.x)
                for (int e = 0; e < op.n; e++) a.x[ro * op.n + e] = a.x_keep[ri * op.n + e];
            if (a.traj_t0) a.traj_t0[ro] = a.traj_t[ri];
            if (a.substeps)
                for (int k = 0; k < op.nsub; k++)
                    for (int d = 0; d < 6; d++) a.substeps[(ro * op.nsub + k) * 6 + d] = a.states[ri * 6 + d];
            if (a.trace)
                for (int d = 0; d < 6; d++) a.trace[ro * 6 + d] = a.states[ri * 6 + d];
        }
    }
    if (lane == 0 && a.fail_count) a.fail_count[team] += n * a.num_steps;
}

__global__ void __launch_bounds__(64) team_rollout_kernel(const DevOps op, const double* __restrict__ buf,
                                                           const TeamRolloutArgs a) {
    constexpr int NZ = 6, G = 64, R = 4;
    const int lane = threadIdx.x;
    const int team = blockIdx.x;
    if (team >= a.num_teams) return;
    const int r0 = a.team_ptr[team], n = a.team_ptr[team + 1] - r0;
    if (n <= 0) return;  // an empty team writes nothing
    const size_t robots = (size_t)a.team_ptr[a.num_teams];  // rows of one sample of the records
    if (n > TEAM_MAX) {
        team_oversize(op, a, robots, r0, n, team, lane);
        return;
    }
    extern __shared__ double lds_stage[];   // one agent's CBF row staging
    __shared__ NbScratch nbs;               // (the grid query's: the lists are CSR, never touched)
    __shared__ double sxy[TEAM_MAX][2];     // one sample's planar positions

    const int nsub = op.nsub;
    // (the summary stays in its in/out buffers between steps: loaded, updated and stored by the
    // step's scoring, so that nothing of it is live in registers across the solves)
    const bool pairs = a.first_collision || a.min_d2;  // the pair scan's outputs
    const bool scored = pairs || a.arrival_sample;

    // the agent's arguments: the team's table as the state table, the team's own lists, the team's
    // seed; the per-turn fields are set in the loop
    ImpcArgs t = {};
    t.num_states = n;
    t.states = a.states + (size_t)r0 * 6;
    t.num_agents = 1;
    t.nb_col = a.nb_col;
    t.pos_std = a.pos_std;
    t.vel_std = a.vel_std;
    t.noise_seed = a.team_seed[team];

    for (int s = 0; s < a.num_steps; s++) {
        const int64_t step = a.step_first + s;
        const size_t row0 = (size_t)(a.record_first + s) * robots + (size_t)r0;
        // the step's sub-step samples: the record's rows, or the work rows
        double* const sub = a.substeps ? a.substeps + row0 * nsub * 6 : a.work + (size_t)team * TEAM_MAX * nsub * 6;
        t.step_index = step;
        int fails = 0;  // this step's decisions without a curve
        for (int i = 0; i < n; i++) {
            const size_t ri = (size_t)(r0 + i), ro = row0 + i;
            t.agent_first = i;
            t.targets = a.targets + ri * 3;
            t.nb_row_ptr = a.nb_row + n * TEAM_ROW + i;
            __builtin_assume(t.nb_row_ptr != nullptr);
            t.x = a.x_keep + ri * op.n;
            t.traj_t = a.traj_t + ri;
            t.next_states = a.states + ri * 6;
            t.substeps = sub + (size_t)i * nsub * 6;
            t.status = a.status ? a.status + ro * op.impc_iter : nullptr;
            t.obj = a.obj ? a.obj + ro * op.impc_iter : nullptr;
            t.iters = a.iters ? a.iters + ro * op.impc_iter : nullptr;
            if (a.traj_t0 && lane == 0) a.traj_t0[ro] = a.traj_t[ri];
            // (the operators through an offset the compiler cannot see is zero, and the lane through a
            // copy it cannot see is the lane: what a turn loads of the operators — the shared rows, 48
            // registers a lane — and the lane's row addresses are otherwise hoisted out of the turn
            // loop as invariant and held across the solves: 108 bytes a lane of scratch with the
            // offset alone, none with both)
            int zero = 0, gl = lane;
            asm volatile("" : "+s"(zero), "+v"(gl));
            const bool have_curve = impc_dense_agent<NZ, G, R>(op, buf + zero, t, 0, gl, lds_stage, nbs);
            fails += have_curve ? 0 : 1;
            team_sync();  // robot i's row, curve and traj_t are in place before robot i + 1 plans
            if (a.x)
                for (int e = lane; e < op.n; e += 64) a.x[ro * op.n + e] = a.x_keep[ri * op.n + e];
        }
        // the table is the state after step `step`
        if (a.trace)
            for (int e = lane; e < n * 6; e += 64) a.trace[row0 * 6 + e] = a.states[(size_t)r0 * 6 + e];
        if (a.fail_count && lane == 0) a.fail_count[team] += fails;
        if (!scored) continue;  // (launch-uniform: no summary is asked for)
        // robot `lane`'s arrival and goal in its lane, the rest wave-uniform
        int arrival = (a.arrival_sample && lane < n) ? a.arrival_sample[r0 + lane] : -1;
        int fc_s = a.first_collision ? a.first_collision[team * 3] : -1, fc_i = -1, fc_j = -1;
        double min_d2 = a.min_d2 ? a.min_d2[team] : __builtin_inf();
        const bool had_collision = fc_s >= 0;
        const double goal_r = a.goal_radius;
        const double hx = a.half_x / 2, hy = a.half_y / 2, wx = 2 * a.half_x, wy = 2 * a.half_y;
        double tgx = 0.0, tgy = 0.0;
        if (lane < n) {
            tgx = a.targets[(size_t)(r0 + lane) * 3];
            tgy = a.targets[(size_t)(r0 + lane) * 3 + 1];
        }
        for (int k = 0; k < nsub; k++) {
            const int sample = (int)(step * nsub + k);
            if (lane < 2 * n) sxy[lane >> 1][lane & 1] = sub[((size_t)(lane >> 1) * nsub + k) * 6 + (lane & 1)];
            wave_lds_sync();
            // goal area (collision_check.py:44-46: the planar norm, products and sum rounded one by one)
            if (a.arrival_sample && lane < n && arrival < 0) {
                const double dx = sxy[lane][0] - tgx, dy = sxy[lane][1] - tgy;
                if (sqrt(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy))) <= goal_r) arrival = sample;
            }
            if (pairs) {
                // pairs p < q: the script's box test (:11-20, 28-39: corner = centre - half / 2, extent
                // 2 half, strict comparisons) and the squared distance
                unsigned hit = 0u;  // 256 - (p * 16 + q) of this lane's first colliding pair, 0 = none
                double d2min = __builtin_inf();
                for (int e = lane; e < TEAM_MAX * TEAM_MAX; e += 64) {
                    const int p = e / TEAM_MAX, q = e % TEAM_MAX;
                    if (p < q && q < n) {
                        const double x1 = sxy[p][0], y1 = sxy[p][1], x2 = sxy[q][0], y2 = sxy[q][1];
                        const double xa = x1 - hx, ya = y1 - hy, xb = x2 - hx, yb = y2 - hy;
                        const bool c = (xa < xb + wx) && (xa + wx > xb) && (ya < yb + wy) && (ya + wy > yb);
                        if (c) hit = max(hit, (unsigned)(TEAM_MAX * TEAM_MAX - e));
                        const double dx = x1 - x2, dy = y1 - y2;
                        d2min = fmin(d2min, __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
                    }
                }
                hit = wave_max_u32(hit);
                min_d2 = fmin(min_d2, grp_min<64>(d2min));
                if (hit != 0u && fc_s < 0) {
                    const int e = TEAM_MAX * TEAM_MAX - (int)hit;
                    fc_s = sample;
                    fc_i = e / TEAM_MAX;
                    fc_j = e % TEAM_MAX;
                }
            }
            wave_lds_sync();  // the sample is rewritten by the next one
        }
        if (a.arrival_sample && lane < n) a.arrival_sample[r0 + lane] = arrival;
        if (lane == 0) {
            if (a.first_collision && !had_collision && fc_s >= 0) {
                a.first_collision[team * 3] = fc_s;
                a.first_collision[team * 3 + 1] = fc_i;
                a.first_collision[team * 3 + 2] = fc_j;
            }
            if (a.min_d2) a.min_d2[team] = min_d2;
        }
    }
}

}  // namespace dev

hipError_t launch_team_rollout(const DevOps& op, const double* buf, const TeamRolloutArgs& a, hipStream_t s) {
    if (a.num_teams <= 0 || a.num_steps <= 0) return hipSuccess;
    const size_t lds = (size_t)(4 * 64 - op.m) * (6 + 1) * sizeof(double);
    hipLaunchKernelGGL(dev::team_rollout_kernel, dim3(a.num_teams), dim3(64), lds, s, op, buf, a);
    return hipGetLastError();
}

}  // namespace mpccbf
