// fov_estimates.hpp — the host-side rules of mpccbf_set_fov_estimates (include/mpccbf.h): what an
// attach refuses, what a solve refuses while estimates are attached, and the parameter checks the
// attach shares with mpccbf_pf_init / mpccbf_pf_step. Decisions only, no HIP: capi.hip and
// capi_control.hip call them before any device call; tools/fov_estimates_check.cpp drives the same
// functions on the host (tests/test_fov_estimate_inputs.py).
#pragma once

#include <cmath>
#include <string>

#include "../../../include/mpccbf.h"

namespace mpccbf {

constexpr int PF_PARTICLES_MIN = 2;
constexpr int PF_PARTICLES_MAX = 1024;  // (PF_MAX_PARTICLES, pf_fov.hpp: 4 P doubles of LDS per pair)

// What mpccbf_pf_init / mpccbf_pf_step refuse in the parameters ("" = accepted)
inline std::string pf_params_error(const mpccbf_pf_params& p) {
    if (p.num_particles < PF_PARTICLES_MIN || p.num_particles > PF_PARTICLES_MAX)
        return "num_particles must be in 2 .. 1024";
    auto pos_def = [](const double* c) {
        return c[0] > 0.0 && c[0] * c[2] - c[1] * c[1] > 0.0 && std::isfinite(c[0]) && std::isfinite(c[1]) &&
               std::isfinite(c[2]);
    };
    if (!pos_def(p.init_cov)) return "init_cov must be positive definite";
    if (!pos_def(p.meas_cov)) return "meas_cov must be positive definite";
    if (!(p.weight_reduction > 0.0)) return "weight_reduction must be positive";
    return "";
}

// What an attach refuses ("" = accepted). cbf_mode: the context's controller (1 = FoV). e != NULL
// (a detach is always accepted).
inline std::string fov_estimates_attach_error(int cbf_mode, const mpccbf_fov_estimates& e) {
    if (cbf_mode != 1) return "fov estimates: the FoV controller (cbf_mode 1) only";
    if (e.num_pairs < 0) return "fov estimates: num_pairs < 0";
    if (!e.nb_xy && e.num_pairs > 0) return "fov estimates: nb_xy is required";
    if (!e.pf) return "";  // (the estimates are the caller's: the filter buffers are not read)
    if (!e.particles || !e.weights || !e.est_xy || !e.est_cov)
        return "fov estimates: pf needs particles, weights, est_xy and est_cov";
    if (e.est_xy != e.nb_xy) return "fov estimates: pf needs est_xy == nb_xy";
    // (nb_cov NULL: the filter still runs, the slack order takes every covariance as unknown)
    if (e.nb_cov && e.est_cov != e.nb_cov) return "fov estimates: pf needs est_cov == nb_cov (or nb_cov NULL)";
    const std::string pe = pf_params_error(*e.pf);
    if (!pe.empty()) return "fov estimates: pf: " + pe;
    return "";
}

// What a solve refuses while estimates are attached ("" = accepted). grid: the batch gives no CSR
// lists (nb_row_ptr NULL); nranks: the ranks of the run's communicator (1: none).
inline std::string fov_estimates_solve_error(bool attached, bool grid, int nranks) {
    if (!attached) return "";
    if (grid) return "fov estimates: grid mode is not supported while estimates are attached (give CSR lists)";
    if (nranks > 1) return "fov estimates: a communicator of more than one rank is not supported";
    return "";
}

}  // namespace mpccbf
