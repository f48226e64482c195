// cap_audit.hpp — arguments of the neighbour-cap audit (mpccbf_cap_audit_run, cap_audit.hip).
#pragma once

#include <stdint.h>

namespace mpccbf {

// The audit kernel keeps one membership bitmap over the state table per wave in LDS (4 waves per
// block, num_states bits each): 65,536 states are 8 KB per wave, 32 KB per block.
constexpr int AUDIT_MAX_STATES = 65536;
constexpr int AUDIT_WORDS = 8;    // int32 words per agent in mpccbf_cap_audit::counts
constexpr int AUDIT_LIVE_NB = 8;  // entries per agent in mpccbf_cap_audit::live_nb

struct AuditArgs {
    int32_t num_states;
    const double* states;
    int32_t agent_first;
    int32_t num_agents;
    const int32_t* nb_row_ptr;  // CSR lists (NULL: nb_list)
    const int32_t* nb_col;
    const int32_t* nb_list;     // num_agents x 16, -1 after the last entry (the solve's nb_out)
    const double* x;            // the solve's x (iteration 1's curve where status[1] is OPTIMAL)
    const int32_t* status;      // the solve's statuses, num_agents x impc_iter
    const double* x0;           // iteration 0's curves, num_agents x n (NaN: none)
    int32_t impc_iter;          // of the solve (1 or 2)
    int32_t o_EB2;              // C x C monomials of the Bernstein basis' second derivative
    double h;                   // CBF sample k is at curve parameter h k
    double tol;
    int32_t* counts;            // num_agents x AUDIT_WORDS
    double* excess;             // num_agents x 2, or NULL
    int32_t* live_nb;           // num_agents x AUDIT_LIVE_NB, or NULL
};

}  // namespace mpccbf
