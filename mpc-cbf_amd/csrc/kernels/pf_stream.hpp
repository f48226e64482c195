// pf_stream.hpp — the particle filter's counter-based random stream (pf_fov.hip; restated in
// tests/pf_ref.py). The reference draws from an unseeded std::mt19937 (particle_filter.h), which no
// two runs share; here every draw is a pure function of
//   (seed, step_index, observer's global row, neighbour's global row, particle, component)
// by the project's construction (impc_common.hpp, mix64 / normal_sample): the splitmix64 mixer
// chained over the key words. Keyed on global rows, not on the CSR position, so a pair's draws do
// not depend on how the observers are split over calls or ranks.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mpccbf {
namespace pf {

// components of a particle's draws
constexpr int PF_COMP_X = 0;        // predict: the x normal
constexpr int PF_COMP_Y = 1;        // predict: the y normal
constexpr int PF_COMP_RESAMPLE = 2; // resampling uniform
constexpr int PF_COMP_INIT_X = 3;   // init: the x normal (its own components, so that an init and a
constexpr int PF_COMP_INIT_Y = 4;   // step with the same step_index do not share their normals)

__host__ __device__ __forceinline__ uint64_t pf_mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the part of the key that a pair's particles share
__host__ __device__ __forceinline__ uint64_t pf_pair_key(uint64_t seed, int64_t step, int64_t observer,
                                                         int64_t neighbour) {
    uint64_t k = pf_mix64(seed);
    k = pf_mix64(k ^ (uint64_t)step);
    k = pf_mix64(k ^ (uint64_t)observer);
    return pf_mix64(k ^ (uint64_t)neighbour);
}

__host__ __device__ __forceinline__ uint64_t pf_key(uint64_t pair_key, int particle, int comp) {
    return pf_mix64(pair_key ^ ((uint64_t)particle * 8u + (uint64_t)comp));
}

// u in [0, 1)
__host__ __device__ __forceinline__ double pf_uniform(uint64_t key) {
    return (double)(key >> 11) * 0x1.0p-53;
}

#ifdef __HIPCC__
// Box-Muller: u1 in (0, 1] from the key, u2 in [0, 1) from the key mixed once more
__device__ __forceinline__ double pf_normal(uint64_t key) {
    const double u1 = (double)((key >> 11) + 1) * 0x1.0p-53;
    const double u2 = (double)(pf_mix64(key) >> 11) * 0x1.0p-53;
    return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}
#endif

}  // namespace pf
}  // namespace mpccbf
