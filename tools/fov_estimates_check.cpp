// fov_estimates_check.cpp — the host rules of mpccbf_set_fov_estimates (csrc/host/fov_estimates.hpp)
// driven without a device: what an attach accepts and refuses, what a solve refuses while estimates
// are attached, and the filter parameters mpccbf_pf_step refuses. Plain C++, no HIP, no library;
// built as build/fov_estimates_check and run by tests/test_fov_estimate_inputs.py.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

#include "fov_estimates.hpp"

using namespace mpccbf;

static long checks = 0, failures = 0;

static void expect(bool ok, const char* what) {
    checks++;
    if (!ok) {
        failures++;
        std::printf("FAIL %s\n", what);
    }
}

static mpccbf_pf_params good_pf() {
    mpccbf_pf_params p{};
    p.num_particles = 100;
    p.init_cov[0] = p.init_cov[2] = 1.0;
    p.process[0] = p.process[3] = 0.25;
    p.meas_cov[0] = p.meas_cov[2] = 0.05;
    p.dt = 0.2;
    p.fov = 2.0;
    p.Rs = 6.0;
    p.weight_reduction = 10.0;
    return p;
}

int main() {
    double xy[4] = {}, cov[6] = {}, parts[8] = {}, w[4] = {}, other[4] = {};
    int32_t flags[2] = {};
    const double nan = std::numeric_limits<double>::quiet_NaN();

    // caller's estimates
    mpccbf_fov_estimates e{};
    e.num_pairs = 2;
    e.nb_xy = xy;
    e.nb_cov = cov;
    expect(fov_estimates_attach_error(1, e).empty(), "fov controller, xy + cov: accepted");
    e.nb_cov = nullptr;
    expect(fov_estimates_attach_error(1, e).empty(), "unknown covariances: accepted");
    expect(!fov_estimates_attach_error(0, e).empty(), "collision controller: refused");
    e.num_pairs = -1;
    expect(!fov_estimates_attach_error(1, e).empty(), "num_pairs < 0: refused");
    e.num_pairs = 2;
    e.nb_xy = nullptr;
    expect(!fov_estimates_attach_error(1, e).empty(), "NULL nb_xy with pairs: refused");
    e.num_pairs = 0;
    expect(fov_estimates_attach_error(1, e).empty(), "no pairs, no buffer: accepted");
    // (the filter's buffers without pf are the caller's business: not read)
    e.num_pairs = 2;
    e.nb_xy = xy;
    e.particles = parts;
    expect(fov_estimates_attach_error(1, e).empty(), "pf NULL: the filter buffers are ignored");

    // the filter in the loop
    mpccbf_pf_params pf = good_pf();
    mpccbf_fov_estimates f{};
    f.num_pairs = 2;
    f.nb_xy = xy;
    f.nb_cov = cov;
    f.pf = &pf;
    f.particles = parts;
    f.weights = w;
    f.est_xy = xy;
    f.est_cov = cov;
    f.flags = flags;
    expect(fov_estimates_attach_error(1, f).empty(), "filter with every buffer: accepted");
    expect(!fov_estimates_attach_error(0, f).empty(), "filter on the collision controller: refused");
    f.flags = nullptr;
    expect(fov_estimates_attach_error(1, f).empty(), "flags are optional");
    f.nb_cov = nullptr;
    expect(fov_estimates_attach_error(1, f).empty(), "filter with unknown covariances in the slack order: accepted");
    f.nb_cov = cov;
    for (int miss = 0; miss < 4; miss++) {
        mpccbf_fov_estimates g = f;
        if (miss == 0) g.particles = nullptr;
        if (miss == 1) g.weights = nullptr;
        if (miss == 2) g.est_xy = nullptr;
        if (miss == 3) g.est_cov = nullptr;
        expect(!fov_estimates_attach_error(1, g).empty(), "filter with a missing buffer: refused");
    }
    {
        mpccbf_fov_estimates g = f;
        g.est_xy = other;
        expect(!fov_estimates_attach_error(1, g).empty(), "est_xy != nb_xy: refused");
        g = f;
        g.est_cov = other;
        expect(!fov_estimates_attach_error(1, g).empty(), "est_cov != nb_cov: refused");
    }
    // parameters mpccbf_pf_step refuses
    expect(pf_params_error(pf).empty(), "the example's filter parameters: accepted");
    for (int bad = 0; bad < 8; bad++) {
        mpccbf_pf_params q = good_pf();
        if (bad == 0) q.num_particles = 1;
        if (bad == 1) q.num_particles = 1025;
        if (bad == 2) q.init_cov[0] = 0.0;
        if (bad == 3) q.init_cov[1] = 1.0;  // (singular)
        if (bad == 4) q.meas_cov[2] = -1.0;
        if (bad == 5) q.meas_cov[0] = nan;
        if (bad == 6) q.weight_reduction = 0.0;
        if (bad == 7) q.weight_reduction = nan;
        expect(!pf_params_error(q).empty(), "bad filter parameters: refused by the step");
        mpccbf_fov_estimates g = f;
        g.pf = &q;
        expect(!fov_estimates_attach_error(1, g).empty(), "bad filter parameters: refused by the attach");
    }
    {
        mpccbf_pf_params q = good_pf();
        q.num_particles = 2;
        expect(pf_params_error(q).empty(), "2 particles: accepted");
        q.num_particles = 1024;
        expect(pf_params_error(q).empty(), "1024 particles: accepted");
    }

    // solves while attached
    expect(fov_estimates_solve_error(false, true, 4).empty(), "nothing attached: every solve as before");
    expect(fov_estimates_solve_error(true, false, 1).empty(), "attached, CSR lists, one rank: accepted");
    expect(!fov_estimates_solve_error(true, true, 1).empty(), "attached, grid mode: refused");
    expect(!fov_estimates_solve_error(true, false, 2).empty(), "attached, two ranks: refused");

    std::printf("fov_estimates_check: %ld checks, %ld failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
