// formation_args_check.cpp — the host rules of mpccbf_formation_rollout (csrc/host/formation_args.hpp)
// driven without a device: what the call accepts and refuses, and how it splits its steps into
// launches (every step exactly once, in order, no launch above the cap). Plain C++, no HIP, no
// library; built as build/formation_args_check and run by tests/test_formation_rollout_api.py.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

#include "formation_args.hpp"

using namespace mpccbf;

static long checks = 0, failures = 0;

static void expect(bool ok, const char* what) {
    checks++;
    if (!ok) {
        failures++;
        std::printf("FAIL %s\n", what);
    }
}

static mpccbf_connectivity_control_params good_params() {
    mpccbf_connectivity_control_params p{};
    p.d_min = 0.8;
    p.d_max = 3.0;
    for (int d = 0; d < 3; d++) {
        p.v_min[d] = -1.0;
        p.v_max[d] = 1.0;
    }
    p.slack_cost = 1e5;
    p.slack_decay_rate = 0.1;
    return p;
}

static mpccbf_formation_params good_formation() {
    mpccbf_formation_params f{};
    f.Ts = 0.01;
    f.spring_constant = 0.5;
    f.pos_std = 0.001;
    f.vel_std = 0.01;
    f.shape_half[0] = f.shape_half[1] = 0.2;
    f.goal_radius = 1.0;
    return f;
}

int main() {
    int32_t team_ptr[2] = {0, 2};
    double states[12] = {}, targets[6] = {};
    uint64_t seeds[1] = {7};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

    const mpccbf_connectivity_control_params p = good_params();
    const mpccbf_formation_params f = good_formation();
    mpccbf_formation_batch b{};
    b.num_teams = 1;
    b.team_ptr = team_ptr;
    b.states = states;
    b.targets = targets;
    b.team_seed = seeds;
    b.num_steps = 5;

    expect(formation_args_error(&p, &f, &b).empty(), "the example's parameters, no record: accepted");
    expect(!formation_args_error(nullptr, &f, &b).empty(), "NULL controller parameters: refused");
    expect(!formation_args_error(&p, nullptr, &b).empty(), "NULL formation parameters: refused");
    expect(!formation_args_error(&p, &f, nullptr).empty(), "NULL batch: refused");

    // required pointers
    for (int miss = 0; miss < 4; miss++) {
        mpccbf_formation_batch c = b;
        if (miss == 0) c.team_ptr = nullptr;
        if (miss == 1) c.states = nullptr;
        if (miss == 2) c.targets = nullptr;
        if (miss == 3) c.team_seed = nullptr;
        expect(!formation_args_error(&p, &f, &c).empty(), "a missing required pointer: refused");
        c.num_steps = 0;
        expect(formation_args_error(&p, &f, &c).empty(), "no steps: nothing is read, accepted");
        c.num_steps = 5;
        c.num_teams = 0;
        expect(formation_args_error(&p, &f, &c).empty(), "no teams: nothing is read, accepted");
    }
    // counts
    {
        mpccbf_formation_batch c = b;
        c.num_teams = -1;
        expect(!formation_args_error(&p, &f, &c).empty(), "num_teams < 0: refused");
        c = b;
        c.num_steps = -1;
        expect(!formation_args_error(&p, &f, &c).empty(), "num_steps < 0: refused");
        c = b;
        c.step_first = -1;
        expect(!formation_args_error(&p, &f, &c).empty(), "step_first < 0: refused");
        c = b;
        c.step_first = (int64_t)INT32_MAX - 5;
        expect(formation_args_error(&p, &f, &c).empty(), "the last sample at 2^31 - 2: accepted");
        c.step_first = (int64_t)INT32_MAX - 4;
        expect(!formation_args_error(&p, &f, &c).empty(), "samples beyond int32: refused");
        c.step_first = std::numeric_limits<int64_t>::max();
        expect(!formation_args_error(&p, &f, &c).empty(), "step_first at INT64_MAX: refused, without overflow");
        c.step_first = std::numeric_limits<int64_t>::max() - 2;
        expect(!formation_args_error(&p, &f, &c).empty(), "step_first + num_steps past INT64_MAX: refused");
    }
    // formation parameters
    for (double bad : {nan, inf, -inf, 0.0, -0.01}) {
        mpccbf_formation_params g = f;
        g.Ts = bad;
        expect(!formation_args_error(&p, &g, &b).empty(), "Ts not positive and finite: refused");
        g = f;
        g.shape_half[1] = bad;
        expect(!formation_args_error(&p, &g, &b).empty(), "a half extent not positive and finite: refused");
    }
    for (double bad : {nan, inf, -1.0}) {
        for (int field = 0; field < 4; field++) {
            mpccbf_formation_params g = f;
            if (field == 0) g.spring_constant = bad;
            if (field == 1) g.pos_std = bad;
            if (field == 2) g.vel_std = bad;
            if (field == 3) g.goal_radius = bad;
            expect(!formation_args_error(&p, &g, &b).empty(), "a negative or non-finite parameter: refused");
        }
    }
    {
        mpccbf_formation_params g = f;
        g.pos_std = g.vel_std = 0.0;
        g.goal_radius = 0.0;
        expect(formation_args_error(&p, &g, &b).empty(), "no noise, a goal radius of zero: accepted");
        g.steps_per_launch = -1;
        expect(!formation_args_error(&p, &g, &b).empty(), "steps_per_launch < 0: refused");
        g.steps_per_launch = 0;
        expect(formation_steps_per_launch(g) == MPCCBF_FORMATION_STEPS_PER_LAUNCH, "steps_per_launch 0: the default");
        g.steps_per_launch = 7;
        expect(formation_steps_per_launch(g) == 7, "steps_per_launch 7");
    }
    // the controller's parameters
    {
        mpccbf_connectivity_control_params q = p;
        q.d_min = 0.0;
        expect(!formation_args_error(&q, &f, &b).empty(), "d_min 0: refused");
        q = p;
        q.d_max = nan;
        expect(!formation_args_error(&q, &f, &b).empty(), "d_max NaN: refused");
        q = p;
        q.v_min[1] = 2.0;
        expect(!formation_args_error(&q, &f, &b).empty(), "v_min > v_max: refused");
        q = p;
        q.slack_mode = 1;
        expect(formation_args_error(&q, &f, &b).empty(), "slack mode with its cost and decay: accepted");
        q.slack_cost = 0.0;
        expect(!formation_args_error(&q, &f, &b).empty(), "slack mode without a cost: refused");
        q = p;
        q.slack_mode = 1;
        q.slack_decay_rate = 1.5;
        expect(!formation_args_error(&q, &f, &b).empty(), "slack decay above 1: refused");
    }
    // the split: every step once, in order, no launch above the cap, for every small call
    for (int32_t steps = 0; steps <= 40; steps++) {
        for (int32_t per = 1; per <= 20; per++) {
            int32_t next = 0, launches = 0;
            bool ok = true;
            for (int32_t k = 0; k < 64; k++) {
                const FormationLaunch l = formation_launch(steps, per, k);
                if (l.count == 0) break;
                ok = ok && l.first == next && l.count >= 1 && l.count <= per;
                next += l.count;
                launches++;
            }
            expect(ok && next == steps && launches == (steps + per - 1) / per, "split covers the steps once, in order");
        }
    }
    {
        const FormationLaunch l = formation_launch(INT32_MAX, INT32_MAX, 0);
        expect(l.first == 0 && l.count == INT32_MAX, "one launch of 2^31 - 1 steps");
        const FormationLaunch m = formation_launch(INT32_MAX, 1 << 30, 1);
        expect(m.first == (1 << 30) && m.count == INT32_MAX - (1 << 30), "the second launch at 2^30: no overflow");
        expect(formation_launch(INT32_MAX, INT32_MAX, 1).count == 0, "past the last launch");
    }

    std::printf("formation_args_check: %ld checks, %ld failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
