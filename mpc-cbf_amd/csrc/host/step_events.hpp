// step_events.hpp — the timing events of one mpccbf_run_steps call: which event of the context's
// pool plays which role, which of them the call records, which one it waits for, and which pairs
// mpccbf_run::step_ms and solve_ms are read from. Decisions only, no HIP: the run loop
// (capi_run.hip) records and reads the events this plan names, out of the pool that owns them
// (capi_ctx.hpp, EventPool); tools/run_owners_check.cpp checks the plan over every small call
// (tests/test_run_owners.py).
//
// The layout: event 0 is the call's start, and step s has three, solve begin / solve end (around
// its IMPC kernel alone) and step end. A step's interval starts where the step before ended.
#pragma once

#include <algorithm>

namespace mpccbf {

class StepEvents {
  public:
    // the fields of mpccbf_run; step_ms / solve_ms: the array is given
    StepEvents(int num_steps, int reserve_steps, int solve_stride, bool step_ms, bool solve_ms)
        : steps_(num_steps), reserve_(reserve_steps), stride_(solve_stride), step_ms_(step_ms), solve_ms_(solve_ms) {}

    // The pool's size before the first step: a call prepared with reserve_steps creates no event
    // in a later, timed call of up to that many steps.
    int needed() const { return 3 * std::max(steps_, reserve_) + 1; }
    bool timing() const { return step_ms_ || solve_ms_; }

    // ---- the roles --------------------------------------------------------------------------------
    int start() const { return 0; }
    int solve_begin(int s) const { return 3 * s + 1; }
    int solve_end(int s) const { return 3 * s + 2; }
    int step_end(int s) const { return 3 * s + 3; }

    // ---- what the call records and waits for ------------------------------------------------------
    bool records_start() const { return timing(); }
    // step s records solve_begin / solve_end around its IMPC kernel (solve_stride <= 1: every step)
    bool times_solve(int s) const { return solve_ms_ && (stride_ <= 1 || s % stride_ == 0); }
    // step s records step_end (without step_ms the last step alone: the event to wait for)
    bool records_end(int s) const { return step_ms_ || (timing() && s == steps_ - 1); }
    // the event the call synchronises on before it reads, or -1: nothing to read
    int waits_for() const { return timing() && steps_ > 0 ? step_end(steps_ - 1) : -1; }

    // ---- what the outputs are read from -----------------------------------------------------------
    struct Pair {
        int from, to;  // from < 0: no interval, the slot is -1
    };
    // step_ms[s] (step_ms given)
    Pair step_slot(int s) const { return Pair{s == 0 ? start() : step_end(s - 1), step_end(s)}; }
    // solve_ms[s] (solve_ms given)
    Pair solve_slot(int s) const { return times_solve(s) ? Pair{solve_begin(s), solve_end(s)} : Pair{-1, -1}; }

  private:
    int steps_, reserve_, stride_;
    bool step_ms_, solve_ms_;
};

}  // namespace mpccbf
