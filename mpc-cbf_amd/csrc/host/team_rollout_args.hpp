// team_rollout_args.hpp — the host-side rules of mpccbf_team_rollout (include/mpccbf.h): what the call
// refuses and how it splits its steps into launches. Decisions only, no HIP: capi_rollout.hip calls
// them before any device call; tools/team_rollout_args_check.cpp drives the same functions on the
// host (tests/test_team_rollout_api.py).
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/mpccbf.h"

namespace mpccbf {

constexpr int TEAM_ROLLOUT_MAX = 16;         // robots per team (TEAM_MAX, team_rollout.hpp)
constexpr int TEAM_ROLLOUT_ROWS = 256;       // row slots of the dense 64 x 4 layout
constexpr int TEAM_ROLLOUT_NZ = 6;           // its reduced dimension

// What the call needs to know of its context: the operators' sizes and what is attached to it
struct TeamRolloutContext {
    int32_t cbf_mode;     // 1: the FoV controller
    int32_t slack_mode;
    int32_t nz, m;        // reduced dimension, shared rows
    int32_t cbf_horizon;
    int32_t nsub;         // control sub-steps per step, int(h / Ts)
    int32_t connectivity; // connectivity rows attached (mpccbf_set_connectivity)
    int32_t ranks;        // ranks of the communicator the context is bound to (1: none)
};

// What mpccbf_team_rollout refuses of its context ("" = accepted)
inline std::string team_rollout_context_error(const TeamRolloutContext& c) {
    if (c.cbf_mode == 1) return "team rollout: the FoV controller is not supported";
    if (c.slack_mode) return "team rollout: slack mode is not supported";
    if (c.nz != TEAM_ROLLOUT_NZ || c.m >= TEAM_ROLLOUT_ROWS)
        return "team rollout: the operators do not fit the dense 64 x 4 layout (nz != 6 or m >= 256)";
    // a full team's CBF rows in iteration 1: (TEAM_ROLLOUT_MAX - 1) neighbours x cbf_horizon samples
    if ((int64_t)(TEAM_ROLLOUT_MAX - 1) * c.cbf_horizon > TEAM_ROLLOUT_ROWS - c.m)
        return "team rollout: 15 * cbf_horizon CBF rows exceed the 256 - m free row slots";
    if (c.nsub < 1) return "team rollout: h / Ts gives no control sub-step";
    if (c.connectivity) return "team rollout: a context with connectivity rows attached is not supported";
    if (c.ranks > 1) return "team rollout: a context bound to a multi-rank communicator is not supported";
    return "";
}

// What mpccbf_team_rollout refuses of its arguments ("" = accepted). nsub: control sub-steps per step
// (the sample numbers of the summary are step * nsub + k)
inline std::string team_rollout_args_error(const mpccbf_team_rollout_params* p, const mpccbf_team_batch* b,
                                           int32_t nsub) {
    if (!p || !b) return "team rollout: null argument";
    auto nonneg = [](double v) { return v >= 0.0 && std::isfinite(v); };
    auto pos = [](double v) { return v > 0.0 && std::isfinite(v); };
    if (!nonneg(p->pos_std) || !nonneg(p->vel_std)) return "team rollout: pos_std and vel_std must be >= 0 and finite";
    if (!pos(p->shape_half[0]) || !pos(p->shape_half[1]))
        return "team rollout: the box's half extents must be positive and finite";
    if (!nonneg(p->goal_radius)) return "team rollout: goal_radius must be >= 0 and finite";
    if (p->steps_per_launch < 0) return "team rollout: steps_per_launch < 0";
    if (b->num_teams < 0 || b->num_steps < 0 || b->step_first < 0) return "team rollout: negative count";
    if (b->step_first > (int64_t)INT32_MAX - b->num_steps)  // (no sum: step_first may be near INT64_MAX)
        return "team rollout: step_first + num_steps exceeds 2^31 - 1";
    // the summary's sample numbers are int32: the last one, (step_first + num_steps) * nsub - 1, must fit
    if ((b->arrival_sample || b->first_collision) && nsub > 1 &&
        (b->step_first + b->num_steps) > (int64_t)INT32_MAX / nsub)
        return "team rollout: the summary's sample numbers (step * nsub + k) exceed 2^31 - 1";
    if (b->num_teams > 0 && b->num_steps > 0 &&
        (!b->team_ptr || !b->states || !b->targets || !b->team_seed || !b->x_keep || !b->traj_t))
        return "team rollout: team_ptr, states, targets, team_seed, x_keep and traj_t are required";
    return "";
}

// steps of one launch (steps_per_launch with its default applied)
inline int32_t team_steps_per_launch(const mpccbf_team_rollout_params& p) {
    return p.steps_per_launch > 0 ? p.steps_per_launch : MPCCBF_TEAM_STEPS_PER_LAUNCH;
}

// launch k of a call over num_steps steps: its first step within the call and its step count
// (count 0: past the last launch)
struct TeamLaunch {
    int32_t first, count;
};
inline TeamLaunch team_launch(int32_t num_steps, int32_t per_launch, int32_t k) {
    const int64_t first = (int64_t)k * per_launch;
    if (first >= num_steps) return {num_steps, 0};
    const int64_t left = num_steps - first;
    return {(int32_t)first, (int32_t)(left < per_launch ? left : per_launch)};
}

}  // namespace mpccbf
