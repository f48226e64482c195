// team_rollout_args_check.cpp — the host rules of mpccbf_team_rollout (csrc/host/team_rollout_args.hpp)
// driven without a device: what the call refuses of its context and of its arguments, what it
// accepts at the edges, and how it splits its steps into launches (every step exactly once, in
// order, no launch above the cap). Plain C++, no HIP, no library; built as
// build/team_rollout_args_check and run by tests/test_team_rollout_api.py.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

#include "team_rollout_args.hpp"

using namespace mpccbf;

static long checks = 0, failures = 0;

static void expect(bool ok, const char* what) {
    checks++;
    if (!ok) {
        failures++;
        std::printf("FAIL %s\n", what);
    }
}

static bool refused(const std::string& err, const char* word) {
    return err.rfind("team rollout:", 0) == 0 && err.find(word) != std::string::npos;
}

// base_config.json: 6 reduced variables, 51 shared rows, cbf_horizon 2, h / Ts = 10
static TeamRolloutContext good_context() {
    TeamRolloutContext c{};
    c.nz = 6;
    c.m = 51;
    c.cbf_horizon = 2;
    c.nsub = 10;
    c.ranks = 1;
    return c;
}

static mpccbf_team_rollout_params good_params() {
    mpccbf_team_rollout_params p{};
    p.pos_std = 0.001;
    p.vel_std = 0.01;
    p.shape_half[0] = p.shape_half[1] = 0.2;
    p.goal_radius = 1.0;
    return p;
}

int main() {
    int32_t team_ptr[2] = {0, 2};
    double states[12] = {}, targets[6] = {}, x_keep[2 * 36] = {}, traj_t[2] = {-1.0, -1.0};
    uint64_t seeds[1] = {7};
    int32_t arrival[2] = {-1, -1}, collision[3] = {-1, -1, -1};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

    const TeamRolloutContext c = good_context();
    const mpccbf_team_rollout_params p = good_params();
    mpccbf_team_batch b{};
    b.num_teams = 1;
    b.team_ptr = team_ptr;
    b.states = states;
    b.targets = targets;
    b.team_seed = seeds;
    b.x_keep = x_keep;
    b.traj_t = traj_t;
    b.num_steps = 5;

    // ---- the context
    expect(team_rollout_context_error(c).empty(), "the base configuration's context: accepted");
    {
        TeamRolloutContext d = c;
        d.cbf_mode = 1;
        expect(refused(team_rollout_context_error(d), "FoV"), "a FoV context: refused");
        d = c;
        d.slack_mode = 1;
        expect(refused(team_rollout_context_error(d), "slack"), "slack mode: refused");
        for (int nz : {1, 2, 3, 5, 7, 8}) {
            d = c;
            d.nz = nz;
            expect(refused(team_rollout_context_error(d), "nz != 6"), "a reduced dimension other than 6: refused");
        }
        d = c;
        d.m = 256;
        expect(refused(team_rollout_context_error(d), "m >= 256"), "256 shared rows: refused");
        d.m = 300;
        expect(refused(team_rollout_context_error(d), "m >= 256"), "more than 256 shared rows: refused");
        // a full team's CBF rows against the free slots, at every row count and horizon
        for (int m = 0; m < 256; m++) {
            for (int h = 1; h <= 8; h++) {
                d = c;
                d.m = m;
                d.cbf_horizon = h;
                const bool fits = 15 * h <= 256 - m;
                expect(team_rollout_context_error(d).empty() == fits, "15 * cbf_horizon against 256 - m");
                if (!fits) expect(refused(team_rollout_context_error(d), "cbf_horizon"), "names the row capacity");
            }
        }
        d = c;
        d.m = 226;  // 30 free slots = 15 x 2: the last context that fits
        expect(team_rollout_context_error(d).empty(), "15 * 2 rows in exactly 30 free slots: accepted");
        d.m = 227;
        expect(!team_rollout_context_error(d).empty(), "15 * 2 rows in 29 free slots: refused");
        d = c;
        d.connectivity = 1;
        expect(refused(team_rollout_context_error(d), "connectivity"), "connectivity rows attached: refused");
        d = c;
        d.ranks = 2;
        expect(refused(team_rollout_context_error(d), "multi-rank"), "a multi-rank communicator: refused");
        d = c;
        d.nsub = 0;
        expect(!team_rollout_context_error(d).empty(), "no control sub-step: refused");
    }

    // ---- the arguments
    expect(team_rollout_args_error(&p, &b, 10).empty(), "the example's parameters, no record, no summary: accepted");
    expect(refused(team_rollout_args_error(nullptr, &b, 10), "null"), "NULL parameters: refused");
    expect(refused(team_rollout_args_error(&p, nullptr, 10), "null"), "NULL batch: refused");
    // required pointers
    for (int miss = 0; miss < 6; miss++) {
        mpccbf_team_batch d = b;
        if (miss == 0) d.team_ptr = nullptr;
        if (miss == 1) d.states = nullptr;
        if (miss == 2) d.targets = nullptr;
        if (miss == 3) d.team_seed = nullptr;
        if (miss == 4) d.x_keep = nullptr;
        if (miss == 5) d.traj_t = nullptr;
        expect(refused(team_rollout_args_error(&p, &d, 10), "required"), "a missing required pointer: refused");
        d.num_steps = 0;
        expect(team_rollout_args_error(&p, &d, 10).empty(), "no steps: nothing is read, accepted");
        d.num_steps = 5;
        d.num_teams = 0;
        expect(team_rollout_args_error(&p, &d, 10).empty(), "no teams: nothing is read, accepted");
    }
    // counts
    {
        mpccbf_team_batch d = b;
        d.num_teams = -1;
        expect(refused(team_rollout_args_error(&p, &d, 10), "negative"), "num_teams < 0: refused");
        d = b;
        d.num_steps = -1;
        expect(refused(team_rollout_args_error(&p, &d, 10), "negative"), "num_steps < 0: refused");
        d = b;
        d.step_first = -1;
        expect(refused(team_rollout_args_error(&p, &d, 10), "negative"), "step_first < 0: refused");
        d = b;
        d.num_teams = 0;
        expect(team_rollout_args_error(&p, &d, 10).empty(), "0 teams: accepted");
        d = b;
        d.num_steps = 0;
        expect(team_rollout_args_error(&p, &d, 10).empty(), "0 steps: accepted");
        d = b;
        d.step_first = (int64_t)INT32_MAX - 5;
        expect(team_rollout_args_error(&p, &d, 10).empty(), "step_first + num_steps = 2^31 - 1: accepted");
        d.step_first = (int64_t)INT32_MAX - 4;
        expect(refused(team_rollout_args_error(&p, &d, 10), "2^31 - 1"), "step_first + num_steps = 2^31: refused");
        d.step_first = std::numeric_limits<int64_t>::max();
        expect(!team_rollout_args_error(&p, &d, 10).empty(), "step_first at INT64_MAX: refused, without overflow");
        d.step_first = std::numeric_limits<int64_t>::max() - 2;
        expect(!team_rollout_args_error(&p, &d, 10).empty(), "step_first + num_steps past INT64_MAX: refused");
        // the summary's int32 sample numbers, step * nsub + k
        for (int which = 0; which < 2; which++) {
            d = b;
            (which == 0 ? d.arrival_sample : d.first_collision) = which == 0 ? arrival : collision;
            d.step_first = (int64_t)INT32_MAX / 10 - 5;
            expect(team_rollout_args_error(&p, &d, 10).empty(), "the last sample number below 2^31: accepted");
            d.step_first += 1;
            expect(refused(team_rollout_args_error(&p, &d, 10), "sample numbers"), "a sample number past 2^31 - 1: refused");
            d.step_first = (int64_t)INT32_MAX - 5;
            expect(team_rollout_args_error(&p, &d, 1).empty(), "one sub-step: samples are steps, the edge is accepted");
        }
    }
    // parameters
    for (double bad : {nan, inf, -inf, 0.0, -0.01}) {
        mpccbf_team_rollout_params g = p;
        g.shape_half[0] = bad;
        expect(refused(team_rollout_args_error(&g, &b, 10), "half extents"), "a half extent not positive and finite: refused");
        g = p;
        g.shape_half[1] = bad;
        expect(refused(team_rollout_args_error(&g, &b, 10), "half extents"), "a half extent not positive and finite: refused");
    }
    for (double bad : {nan, inf, -inf, -1.0}) {
        for (int field = 0; field < 3; field++) {
            mpccbf_team_rollout_params g = p;
            if (field == 0) g.pos_std = bad;
            if (field == 1) g.vel_std = bad;
            if (field == 2) g.goal_radius = bad;
            expect(!team_rollout_args_error(&g, &b, 10).empty(), "a negative or non-finite parameter: refused");
        }
    }
    {
        mpccbf_team_rollout_params g = p;
        g.pos_std = g.vel_std = 0.0;
        g.goal_radius = 0.0;
        expect(team_rollout_args_error(&g, &b, 10).empty(), "no noise, a goal radius of zero: accepted");
        g.steps_per_launch = -1;
        expect(refused(team_rollout_args_error(&g, &b, 10), "steps_per_launch"), "steps_per_launch < 0: refused");
        g.steps_per_launch = 0;
        expect(team_steps_per_launch(g) == MPCCBF_TEAM_STEPS_PER_LAUNCH, "steps_per_launch 0: the default");
        g.steps_per_launch = 7;
        expect(team_steps_per_launch(g) == 7, "steps_per_launch 7");
    }
    // the split: every step once, in order, no launch above the cap, for every small call
    for (int32_t steps = 0; steps <= 40; steps++) {
        for (int32_t per = 1; per <= 20; per++) {
            int32_t next = 0, launches = 0;
            bool ok = true;
            for (int32_t k = 0; k < 64; k++) {
                const TeamLaunch l = team_launch(steps, per, k);
                if (l.count == 0) break;
                ok = ok && l.first == next && l.count >= 1 && l.count <= per;
                next += l.count;
                launches++;
            }
            expect(ok && next == steps && launches == (steps + per - 1) / per, "split covers the steps once, in order");
        }
    }
    {
        const TeamLaunch l = team_launch(INT32_MAX, INT32_MAX, 0);
        expect(l.first == 0 && l.count == INT32_MAX, "one launch of 2^31 - 1 steps");
        const TeamLaunch m = team_launch(INT32_MAX, 1 << 30, 1);
        expect(m.first == (1 << 30) && m.count == INT32_MAX - (1 << 30), "the second launch at 2^30: no overflow");
        expect(team_launch(INT32_MAX, INT32_MAX, 1).count == 0, "past the last launch");
    }

    std::printf("team_rollout_args_check: %ld checks, %ld failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
