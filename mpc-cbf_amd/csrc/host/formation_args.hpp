// formation_args.hpp — the host-side rules of mpccbf_formation_rollout (include/mpccbf.h): what the
// call refuses and how it splits its steps into launches. Decisions only, no HIP: capi_control.hip
// calls them before any device call; tools/formation_args_check.cpp drives the same functions on the
// host (tests/test_formation_rollout_api.py).
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/mpccbf.h"

namespace mpccbf {

// What mpccbf_connectivity_control_solve and mpccbf_formation_rollout refuse in the controller's
// parameters ("" = accepted)
inline std::string conn_control_params_error(const mpccbf_connectivity_control_params& p) {
    if (!(p.d_min > 0.0) || !(p.d_max > 0.0)) return "d_min and d_max must be positive";
    for (int d = 0; d < 3; d++)
        if (!(p.v_min[d] <= p.v_max[d])) return "v_min must not exceed v_max";
    if (p.slack_mode && !(p.slack_cost > 0.0)) return "Slack cost must be positive when slack_mode is enabled";
    if (p.slack_mode && !(p.slack_decay_rate > 0.0 && p.slack_decay_rate <= 1.0))
        return "Slack decay rate must be in (0,1] when slack_mode is enabled";
    return "";
}

// What mpccbf_formation_rollout refuses ("" = accepted)
inline std::string formation_args_error(const mpccbf_connectivity_control_params* p, const mpccbf_formation_params* f,
                                        const mpccbf_formation_batch* b) {
    if (!p || !f || !b) return "formation rollout: null argument";
    const std::string perr = conn_control_params_error(*p);
    if (!perr.empty()) return "formation rollout: " + perr;
    auto nonneg = [](double v) { return v >= 0.0 && std::isfinite(v); };
    auto pos = [](double v) { return v > 0.0 && std::isfinite(v); };
    if (!pos(f->Ts)) return "formation rollout: Ts must be positive and finite";
    if (!nonneg(f->spring_constant)) return "formation rollout: spring_constant must be >= 0 and finite";
    if (!nonneg(f->pos_std) || !nonneg(f->vel_std)) return "formation rollout: pos_std and vel_std must be >= 0 and finite";
    if (!pos(f->shape_half[0]) || !pos(f->shape_half[1]))
        return "formation rollout: the box's half extents must be positive and finite";
    if (!nonneg(f->goal_radius)) return "formation rollout: goal_radius must be >= 0 and finite";
    if (f->steps_per_launch < 0) return "formation rollout: steps_per_launch < 0";
    if (b->num_teams < 0 || b->num_steps < 0 || b->step_first < 0) return "formation rollout: negative count";
    if (b->step_first > (int64_t)INT32_MAX - b->num_steps)  // (no sum: step_first may be near INT64_MAX)
        return "formation rollout: step_first + num_steps exceeds 2^31 - 1";
    if (b->num_teams > 0 && b->num_steps > 0 && (!b->team_ptr || !b->states || !b->targets || !b->team_seed))
        return "formation rollout: team_ptr, states, targets and team_seed are required";
    return "";
}

// steps of one launch (steps_per_launch with its default applied)
inline int32_t formation_steps_per_launch(const mpccbf_formation_params& f) {
    return f.steps_per_launch > 0 ? f.steps_per_launch : MPCCBF_FORMATION_STEPS_PER_LAUNCH;
}

// launch k of a call over num_steps steps: its first step within the call and its step count
// (count 0: past the last launch)
struct FormationLaunch {
    int32_t first, count;
};
inline FormationLaunch formation_launch(int32_t num_steps, int32_t per_launch, int32_t k) {
    const int64_t first = (int64_t)k * per_launch;
    if (first >= num_steps) return {num_steps, 0};
    const int64_t left = num_steps - first;
    return {(int32_t)first, (int32_t)(left < per_launch ? left : per_launch)};
}

}  // namespace mpccbf
