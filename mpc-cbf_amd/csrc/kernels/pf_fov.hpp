// pf_fov.hpp — arguments of the batched FoV particle filter kernels (pf_fov.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

struct mpccbf_pf_params;
struct mpccbf_pf_batch;

namespace mpccbf {

constexpr int PF_MIN_PARTICLES = 2;
constexpr int PF_MAX_PARTICLES = 1024;  // 4 P doubles of LDS per pair: 32 KB

struct PfArgs {
    int32_t num_particles;
    int32_t num_states;
    const double* states;       // num_states x 6
    int32_t agent_first, num_agents;
    const int32_t* nb_row_ptr;  // num_agents + 1; pair e = CSR entry e (nb_row_ptr[0] may be nonzero)
    const int32_t* nb_col;
    int32_t num_pairs;          // blocks of the launch: pairs nb_row_ptr[0] .. nb_row_ptr[0] + num_pairs - 1
    const double* input;        // pairs x 2, or nullptr (zero)
    const double* init_xy;      // pairs x 2, or nullptr (the neighbour's true position); init only
    double* particles;          // pairs x 2 x P (x then y)
    double* weights;            // pairs x P
    double* est_xy;             // pairs x 2
    double* est_cov;            // pairs x 3 (cxx, cxy, cyy)
    int32_t* flags;             // pairs, or nullptr
    int32_t* ancestors;         // pairs x P, or nullptr
    int64_t step_index;
    uint64_t seed;
    double init_cov[3];         // (cxx, cxy, cyy)
    double init_chol[3];        // its Cholesky factor (l00, l10, l11)
    double process[4];          // W, row-major (a plain multiplier: particle_filter.cpp:73)
    double meas_inv[3];         // R^-1 (ixx, ixy, iyy)
    double dt, fov, Rs, weight_reduction;
    int32_t pair_rows;          // > 0: rows of the per-pair buffers, a pair e >= pair_rows is skipped
};

hipError_t launch_pf_init(const PfArgs& a, hipStream_t s);
hipError_t launch_pf_step(const PfArgs& a, hipStream_t s);

// The body of mpccbf_pf_init / mpccbf_pf_step (capi_control.hip): checks, arguments, one launch
int pf_enqueue(const mpccbf_pf_params* p, const mpccbf_pf_batch* b, int32_t device, void* stream, bool init,
               int32_t pair_rows);

}  // namespace mpccbf
