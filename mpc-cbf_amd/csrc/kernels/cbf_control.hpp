// cbf_control.hpp — arguments of the batched CBF-only controller kernel (cbf_control.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mpccbf {

struct FovControlArgs {
    int32_t num_agents;
    const double* states;       // num_agents x 6
    const double* desired_u;    // num_agents x 3
    const int32_t* nb_row_ptr;  // num_agents + 1
    const double* nb_xy;        // observed neighbour positions, nb_row_ptr[num_agents] x 2
    double* u;                  // num_agents x 3 (NaN rows: not OPTIMAL)
    int32_t* status;
    double* obj;
    int32_t* iters;
    double fov, Ds, Rs;
    double vmin[3], vmax[3], umin[3], umax[3];
    int32_t maxit;
    double tol, feas_tol;
    double P[9], LP[9];  // 2 I and its Cholesky factor (objective 1/2 u^T P u + q^T u)
    // slack mode (FovControl.cpp:25-62): one slack per observed neighbour (<= 16)
    int32_t slack_mode;
    double slack_cost, slack_decay;
    const double* nb_cov;  // per observed neighbour (cxx, cxy, cyy), or nullptr (unknown)
};

// one robot's QP of ConnectivityControl::optimize (conn_robot_qp.hpp): what it takes besides the table
struct ConnQpParams {
    double dmin, dmax;
    double vmin[3], vmax[3];
    int32_t maxit;
    double tol, feas_tol;
    int32_t slack_mode;  // (the kernels are instantiated per mode: the launch reads it)
    double slack_cost, slack_decay;
};

// ConnectivityControl::optimize for a batch of teams (connectivity_control.hip)
struct ConnControlArgs {
    int32_t num_teams;
    const int32_t* team_ptr;    // num_teams + 1
    const double* states;       // robots x 6
    const double* desired_u;    // robots x 3
    double* u;                  // robots x 3 (NaN rows: not OPTIMAL)
    int32_t* status;
    double* obj;
    int32_t* iters;
    double* lambda2;            // num_teams, or nullptr
    ConnQpParams qp;
};

hipError_t launch_connectivity_control(const ConnControlArgs& a, hipStream_t s);

// CBFFormationControl_example.cpp:136-187 for a batch of teams, robots in index order
// (formation_rollout.hip); steps [step_first, step_first + num_steps) of one launch
struct FormationArgs {
    int32_t num_teams;
    const int32_t* team_ptr;    // num_teams + 1
    double* states;             // robots x 6, in/out
    const double* targets;      // robots x 3
    const uint64_t* team_seed;  // num_teams
    int64_t step_first;         // absolute index of this launch's first step
    int32_t num_steps;
    int32_t record_first;       // this launch's first step in the records (team_ptr[num_teams] rows each)
    // per-decision records of the whole call, or nullptr
    double* trace;              // [steps][robots][6]
    double* cbf_u;              // [steps][robots][3]
    double* desired_u;          // [steps][robots][3]
    int32_t* status;            // [steps][robots]
    double* lambda2;            // [steps][robots]
    int32_t* iters;             // [steps][robots]
    // per-team summary, in/out, or nullptr
    int32_t* arrival_sample;    // robots
    int32_t* first_collision;   // num_teams x 3
    double* min_d2;             // num_teams
    int32_t* fail_count;        // num_teams
    ConnQpParams qp;
    double Ts, spring, pos_std, vel_std;
    double half_x, half_y, goal_radius;  // collision_check.py's box and goal area
};

hipError_t launch_formation_rollout(const FormationArgs& a, hipStream_t s);

constexpr int FOV_CONTROL_ROW_CAP = 4 * 16;  // rows per agent (R = 4 slots x 16 lanes)

hipError_t launch_fov_control(const FovControlArgs& a, hipStream_t s);

}  // namespace mpccbf
