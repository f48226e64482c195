// team_rollout.hpp — arguments and launcher of the MPC-CBF team rollout (team_rollout.hip,
// mpccbf_team_rollout in include/mpccbf.h). Host and device.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "impc.hpp"

namespace mpccbf {

constexpr int TEAM_MAX = 16;  // robots per team

// "Every other robot of the team, in index order" for every team size 1 .. TEAM_MAX as CSR lists the
// agent body reads like a caller's: robot i of a team of n has the list
// col[row[n * TEAM_ROW + i] .. row[n * TEAM_ROW + i + 1]) of indices into the team's table.
constexpr int TEAM_ROW = TEAM_MAX + 1;                      // row offsets per team size
constexpr int TEAM_ROWS = (TEAM_MAX + 1) * TEAM_ROW;        // int32 entries of `row`
constexpr int TEAM_COLS = (TEAM_MAX - 1) * TEAM_MAX * (TEAM_MAX + 1) / 3;  // sum of n (n - 1), n <= TEAM_MAX
// fills row[TEAM_ROWS] and col[TEAM_COLS] (host)
inline void team_lists(int32_t* row, int32_t* col) {
    int32_t e = 0;
    for (int n = 0; n <= TEAM_MAX; n++) {
        for (int i = 0; i < TEAM_ROW; i++) {
            row[n * TEAM_ROW + i] = e;
            if (i < n)
                for (int j = 0; j < n; j++)
                    if (j != i) col[e++] = j;
        }
    }
}

struct TeamRolloutArgs {
    int32_t num_teams;
    const int32_t* team_ptr;    // num_teams + 1
    const double* targets;      // robots x 3
    const uint64_t* team_seed;  // num_teams
    int64_t step_first;         // absolute index of this launch's first step
    int32_t num_steps;
    int32_t record_first;       // this launch's first step in the records (team_ptr[num_teams] rows each)
    // carried between steps, launches and calls
    double* states;             // robots x 6: the teams' tables
    double* x_keep;             // robots x n: the kept curves (NaN: none)
    double* traj_t;             // robots: the kept curve's evaluation time (-1: none)
    // per-decision records of the whole call, or nullptr
    int32_t* status;            // [steps][robots][impc_iter]
    double* obj;                // [steps][robots][impc_iter]
    int32_t* iters;             // [steps][robots][impc_iter]
    double* x;                  // [steps][robots][n]
    double* traj_t0;            // [steps][robots]
    double* substeps;           // [steps][robots][nsub][6]
    double* trace;              // [steps][robots][6]
    // one step's sub-step samples when `substeps` is not recorded: num_teams x TEAM_MAX x nsub x 6
    // (by team, so the host need not know the robot count, which is in device memory)
    double* work;
    // per-team summary, in/out, or nullptr
    int32_t* arrival_sample;    // robots
    int32_t* first_collision;   // num_teams x 3
    double* min_d2;             // num_teams
    int32_t* fail_count;        // num_teams
    const int32_t* nb_row;      // team_lists (device)
    const int32_t* nb_col;
    double pos_std, vel_std;
    double half_x, half_y, goal_radius;
};

// one wavefront per team; lds: the CBF row staging of one agent of the dense 64 x 4 layout
hipError_t launch_team_rollout(const DevOps& op, const double* buf, const TeamRolloutArgs& a, hipStream_t s);

}  // namespace mpccbf
