// grid_rotation.hpp — which of grid mode's three neighbour tables a step reads, fills and zeroes,
// and what one mpccbf_run_steps call leaves for the next to continue (mpccbf_run::continue_tables).
// Decisions only: no HIP call, no allocation. The owner of the tables' buffer (capi_ctx.hpp, GridTables)
// makes the device calls these decisions ask for; tools/host_state_check.cpp drives the same class
// against a model of the tables' contents (tests/test_host_state.py).
//
// The rule. A neighbour table holds copies of the states it was filled from, so a call may pick the
// rotation up only where nothing can have changed those states or the tables since a grid-mode
// mpccbf_run_steps call enqueued its last step. The record is therefore valid from run_finished
// until the next event of any kind, and nothing but run_finished makes it valid.
#pragma once

#include <cstddef>

namespace mpccbf {

// What a grid-mode call asks of the tables: a continuation needs every field unchanged
struct GridQuery {
    const double* states;  // the state table of the call's first step
    int ns, first, count, k;
    double radius;
};

// The tables of one IMPC step (indices 0 .. 2; -1: the step has none in that role)
struct GridRoles {
    int read;  // holds the step's states
    int fill;  // zeroed before the step: its kernel inserts the states it writes
    int zero;  // zeroed by the step's kernel, for the step after next to fill
};

class GridRotation {
  public:
    // ---- events: each ends what a later call could have continued --------------------------------
    // A step outside a rotation (mpccbf_impc_solve, the cap audit's launch, the CSR steps of
    // mpccbf_run_steps): it may write the recorded state table. In grid mode it reads table 0,
    // which its caller rebuilds from the step's own states first.
    GridRoles foreign_step() {
        rec_.valid = false;
        return GridRoles{0, -1, -1};
    }
    // An mpccbf_run_steps call that leaves no rotation (CSR lists, zero steps, zero agents): its
    // steps, or the caller around a call that ran none, may have rewritten the recorded state table.
    void no_rotation() { rec_.valid = false; }
    // The buffer holds `have` bytes and the tables need `need`. true: it is reallocated, and the
    // tables a continuation would read go with it.
    bool reallocates(size_t need, size_t have) {
        if (need <= have) return false;
        rec_.valid = false;
        return true;
    }

    // ---- a grid-mode mpccbf_run_steps call of at least one step -----------------------------------
    // Does a call with this query continue the recorded rotation? The table its first step reads
    // (filled by the recorded call's last step, the one after it zeroed), or -1: rebuild.
    int continues(const GridQuery& q, bool continue_tables) const {
        const bool same = rec_.q.states == q.states && rec_.q.ns == q.ns && rec_.q.first == q.first &&
                          rec_.q.count == q.count && rec_.q.k == q.k && rec_.q.radius == q.radius;
        return continue_tables && rec_.valid && same ? rec_.next : -1;
    }
    // The call starts (after the tables were reserved). Returns continues(): at -1 the caller builds
    // table 0 from q.states and zeroes table 1, and the rotation starts at table 0. Nothing can be
    // continued until run_finished: a call that fails half way leaves no record.
    int run_started(const GridQuery& q, bool continue_tables) {
        const int base = continues(q, continue_tables);
        rec_.valid = false;
        rec_.q = q;
        rec_.next = base < 0 ? 0 : base;
        return base;
    }
    // Step s of the call started
    GridRoles step(int s) const {
        const int t = (rec_.next + s) % 3;
        return GridRoles{t, (t + 1) % 3, (t + 2) % 3};
    }
    // Every one of the call's `steps` steps is enqueued; the last one wrote final_states.
    void run_finished(const double* final_states, int steps) {
        rec_.q.states = final_states;
        rec_.next = (rec_.next + steps) % 3;
        rec_.valid = true;
    }

  private:
    struct {
        bool valid = false;
        GridQuery q{};
        int next = 0;  // valid: the table the next step reads; during a call: its first step's
    } rec_;
};

}  // namespace mpccbf
