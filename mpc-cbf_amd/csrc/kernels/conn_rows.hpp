// conn_rows.hpp — the connectivity-maintenance rows of the batched IMPC: per team
// the lambda2 connectivity CBF row (ConnectivityMPCCBFQPOperations.cpp:44-86, 111-151) when the
// team's graph is well connected, else one CLF row per other member (:153-173, in
// ConnectivityControl.cpp:72-82's live sign convention), as inequalities on the acceleration at
// the horizon samples. Every row is planar and has the safety rows' form c^T U_k x <= b, so it is
// staged behind them in the same (NZ + 1)-double layout.
#pragma once

#include "impc.hpp"

namespace mpccbf {

// mpccbf_set_connectivity as the kernels see it: an argument of its own of the connectivity
// kernels (as StoreArgs: the kernels launched without it keep their argument layout). Filled per
// step by team_spectrum_kernel from the table the step reads.
struct ConnArgs {
    const int32_t* row_team;   // num_states: the row's team (2 or more members), -1: none
    const int32_t* team_ptr;   // num_teams + 1 offsets into the state rows
    const int32_t* team_mode;  // num_teams: 1 connectivity row, 0 CLF rows, -1 more than 16 members
    const double* team_l2;     // num_teams: lambda2 (NaN: more than 16 members)
    const double* fiedler;     // num_states: the row's entry of its team's unit Fiedler vector
    double dmax, l2_min;
};

// The per-team spectrum launch (team_spectrum_kernel): teams that intersect the agent range
// [first, first + count) of the state table.
struct SpectrumArgs {
    int32_t num_teams;
    const int32_t* team_ptr;
    const double* states;
    int32_t first, count;
    double dmax, l2_switch;
    double* team_l2;     // context-owned, as ConnArgs
    int32_t* team_mode;
    double* fiedler;
    double* out_l2;       // the caller's outputs (mpccbf_connectivity), or nullptr
    double* out_fiedler;  // indexed by state row - team_ptr[0]
};

}  // namespace mpccbf
