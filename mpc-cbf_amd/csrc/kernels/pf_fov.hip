// pf_fov.hip — batched particle filters of the FoV controllers' neighbour estimates: one filter per
// (observer, neighbour) pair, one wave64 (a block of 64) per pair, FP64 throughout.
//
//   pf_init_kernel   ParticleFilter::init               particle_filter.cpp:12-56
//   pf_step_kernel   PFApplications::processFovUpdate   pf_applications.cpp:6-44
//
// The per-pair state lives in HBM and belongs to the caller: particles[pair][2][P] (x then y) and
// weights[pair][P]. A step stages the predicted particles, their weights and the cumulative weights
// in dynamic LDS (4 P doubles, 32 KB at P = 1024): resampling gathers from the pre-resampling
// particles, so they cannot be overwritten in place. Global loads and stores are strided by lane
// (coalesced); the weight sums and the cumulative sum run over the LDS image with a contiguous run
// of ceil(P / 64) particles per lane: a serial pass per lane plus one wave scan of the lane totals.
// Every random draw is counter-based (pf_stream.hpp), so a pair's result does not depend on the
// launch it is part of.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pf_fov.hpp"
#include "pf_stream.hpp"

namespace mpccbf {
namespace dev {

using namespace mpccbf::pf;

// every byte of LDS is dynamic, so the base keeps its 16-byte alignment
extern __shared__ __attribute__((aligned(16))) char pf_smem[];

__device__ __forceinline__ double pf_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;  // the same bits in every lane (the butterfly adds the same pairs everywhere)
}

// The pair of this block: CSR entry e, its observer's and its neighbour's rows of the state table.
// False (for the whole block) when the block is past the last pair (of the lists, or of the buffers
// where pair_rows gives their rows) or the neighbour index is not a row of the table.
__device__ __forceinline__ bool pf_locate(const PfArgs& a, int& e, int& obs, int& nb) {
    e = a.nb_row_ptr[0] + (int)blockIdx.x;
    if (e >= a.nb_row_ptr[a.num_agents] || (a.pair_rows > 0 && e >= a.pair_rows)) return false;
    int lo = 0, hi = a.num_agents;  // nb_row_ptr[lo] <= e < nb_row_ptr[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.nb_row_ptr[mid] <= e) lo = mid; else hi = mid;
    }
    obs = a.agent_first + lo;
    nb = a.nb_col[e];
    return nb >= 0 && nb < a.num_states;
}

// math::insideFOV (math/src/Geometry.cpp:59-73): the target in the observer's frame (rotation
// [[cos, sin], [-sin, cos]]), inside iff |atan2(ly, lx)| <= fov / 2 and its norm <= range
__device__ __forceinline__ bool pf_inside_fov(double ex, double ey, double cy, double sy, double px,
                                              double py, double half_fov, double Rs) {
    const double dx = px - ex, dy = py - ey;
    const double lx = cy * dx + sy * dy, ly = -sy * dx + cy * dy;
    const double dist = sqrt(lx * lx + ly * ly);
    const double angle = fabs(atan2(ly, lx));
    return angle <= half_fov && dist <= Rs;
}

// ParticleFilter::init (particle_filter.cpp:12-56): particles = x0 + chol(init_cov) z, weights 1 / P,
// state = x0, distribution = init_cov
__global__ void __launch_bounds__(64) pf_init_kernel(const PfArgs a) {
    int e, obs, nb;
    if (!pf_locate(a, e, obs, nb)) return;
    const int P = a.num_particles;
    const int lane = threadIdx.x;
    double x0, y0;
    if (a.init_xy) {
        x0 = a.init_xy[(size_t)e * 2];
        y0 = a.init_xy[(size_t)e * 2 + 1];
    } else {  // CBFControl_example.cpp:163-165: the neighbour's position
        x0 = a.states[(size_t)nb * 6];
        y0 = a.states[(size_t)nb * 6 + 1];
    }
    const uint64_t pk = pf_pair_key(a.seed, a.step_index, obs, nb);
    double* gx = a.particles + (size_t)e * 2 * P;
    double* gy = gx + P;
    double* gw = a.weights + (size_t)e * P;
    const double w0 = 1.0 / (double)P;
    for (int i = lane; i < P; i += 64) {
        const double z0 = pf_normal(pf_key(pk, i, PF_COMP_INIT_X));
        const double z1 = pf_normal(pf_key(pk, i, PF_COMP_INIT_Y));
        gx[i] = x0 + a.init_chol[0] * z0;
        gy[i] = y0 + (a.init_chol[1] * z0 + a.init_chol[2] * z1);
        gw[i] = w0;
    }
    if (lane == 0) {
        a.est_xy[(size_t)e * 2] = x0;
        a.est_xy[(size_t)e * 2 + 1] = y0;
        a.est_cov[(size_t)e * 3] = a.init_cov[0];
        a.est_cov[(size_t)e * 3 + 1] = a.init_cov[1];
        a.est_cov[(size_t)e * 3 + 2] = a.init_cov[2];
        if (a.flags) a.flags[e] = 0;
    }
}

__global__ void __launch_bounds__(64) pf_step_kernel(const PfArgs a) {
    int e, obs, nb;
    if (!pf_locate(a, e, obs, nb)) return;
    const int P = a.num_particles;
    const int lane = threadIdx.x;
    double* ox = reinterpret_cast<double*>(pf_smem);  // predicted particles
    double* oy = ox + P;
    double* ow = oy + P;  // their weights
    double* cw = ow + P;  // cumulative weights over the total

    const double* so = a.states + (size_t)obs * 6;
    const double ex = so[0], ey = so[1];
    double sy, cy;
    sincos(so[2], &sy, &cy);
    const double tx = a.states[(size_t)nb * 6], ty = a.states[(size_t)nb * 6 + 1];
    const double half_fov = 0.5 * a.fov;
    // pf_applications.cpp:29-33: the measurement update runs only for a visible neighbour
    const bool measured = pf_inside_fov(ex, ey, cy, sy, tx, ty, half_fov, a.Rs);
    const double ux = a.input ? a.input[(size_t)e * 2] : 0.0;
    const double uy = a.input ? a.input[(size_t)e * 2 + 1] : 0.0;
    const uint64_t pk = pf_pair_key(a.seed, a.step_index, obs, nb);
    double* gx = a.particles + (size_t)e * 2 * P;
    double* gy = gx + P;
    double* gw = a.weights + (size_t)e * P;

    // predict (particle_filter.cpp:63-75: p += input dt + W z, W a plain multiplier), negative
    // information (pf_applications.cpp:19-26: w /= reduction inside the FoV) and, for a visible
    // neighbour, the measurement weights exp(-1/2 d^T R^-1 d) that replace them
    // (particle_filter.cpp:95-98)
    double s2 = 0.0;
    for (int i = lane; i < P; i += 64) {
        const double z0 = pf_normal(pf_key(pk, i, PF_COMP_X));
        const double z1 = pf_normal(pf_key(pk, i, PF_COMP_Y));
        const double x = (gx[i] + ux * a.dt) + (a.process[0] * z0 + a.process[1] * z1);
        const double y = (gy[i] + uy * a.dt) + (a.process[2] * z0 + a.process[3] * z1);
        double w = gw[i];
        if (pf_inside_fov(ex, ey, cy, sy, x, y, half_fov, a.Rs)) w /= a.weight_reduction;
        s2 += w;
        if (measured) {
            const double dx = x - tx, dy = y - ty;
            const double q = a.meas_inv[0] * dx * dx + 2.0 * a.meas_inv[1] * dx * dy + a.meas_inv[2] * dy * dy;
            w = exp(-0.5 * q);
        }
        ox[i] = x;
        oy[i] = y;
        ow[i] = w;
    }
    s2 = pf_wave_sum(s2);
    // the reference divides by a zero sum / resamples over NaN weights (undefined); here a weight
    // sum that is 0 or not finite resets the weights to 1 / P and sets bit 1 of the flag word
    bool degenerate = !(s2 > 0.0 && s2 < INFINITY);
    bool uniform = degenerate && !measured;
    __syncthreads();

    const int run_len = (P + 63) >> 6;
    const int b0 = min(lane * run_len, P), b1 = min(b0 + run_len, P);
    if (measured) {  // particle_filter.cpp:99: w /= w.sum()
        double s3 = 0.0;
        for (int j = b0; j < b1; j++) s3 += ow[j];
        s3 = pf_wave_sum(s3);
        if (s3 > 0.0 && s3 < INFINITY) {
            for (int j = b0; j < b1; j++) ow[j] /= s3;
        } else {
            degenerate = true;
            uniform = true;
        }
    }
    if (uniform) {
        const double w0 = 1.0 / (double)P;
        for (int j = b0; j < b1; j++) ow[j] = w0;
    }

    // cumulative weights C_j = (sum_{i <= j} w_i) / sum w: the lane's running sums, then a wave scan
    // of the lane totals
    double run = 0.0;
    for (int j = b0; j < b1; j++) {
        run += ow[j];
        cw[j] = run;
    }
    double incl = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    double excl = __shfl_up(incl, 1);
    if (lane == 0) excl = 0.0;
    const double total = __shfl(incl, 63);
    for (int j = b0; j < b1; j++) cw[j] = (excl + cw[j]) / total;
    __syncthreads();

    // resample (particle_filter.cpp:106-118, std::discrete_distribution's inverse-CDF rule):
    // ancestor = the first j with u < C_j, clamped to P - 1; the new particle and its weight are the
    // ancestor's, the weights not renormalised
    int32_t* anc = a.ancestors ? a.ancestors + (size_t)e * P : nullptr;
    double sx = 0.0, syy = 0.0;
    for (int i = lane; i < P; i += 64) {
        const double u = pf_uniform(pf_key(pk, i, PF_COMP_RESAMPLE));
        int lo = 0, hi = P - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (u < cw[mid]) hi = mid; else lo = mid + 1;
        }
        const double x = ox[lo], y = oy[lo];
        gx[i] = x;
        gy[i] = y;
        gw[i] = ow[lo];
        if (anc) anc[i] = lo;
        sx += x;
        syy += y;
    }

    // estimate (particle_filter.cpp:120-124, 153-171): the plain mean and sum (p - mean)(p - mean)^T
    // / (P - 1) of the resampled particles (each lane reads back the particles it just stored)
    const double mx = pf_wave_sum(sx) / (double)P, my = pf_wave_sum(syy) / (double)P;
    double cxx = 0.0, cxy = 0.0, cyy = 0.0;
    for (int i = lane; i < P; i += 64) {
        const double dx = gx[i] - mx, dy = gy[i] - my;
        cxx += dx * dx;
        cxy += dx * dy;
        cyy += dy * dy;
    }
    const double inv = 1.0 / (double)(P - 1);
    cxx = pf_wave_sum(cxx);
    cxy = pf_wave_sum(cxy);
    cyy = pf_wave_sum(cyy);
    if (lane == 0) {
        a.est_xy[(size_t)e * 2] = mx;
        a.est_xy[(size_t)e * 2 + 1] = my;
        a.est_cov[(size_t)e * 3] = cxx * inv;
        a.est_cov[(size_t)e * 3 + 1] = cxy * inv;
        a.est_cov[(size_t)e * 3 + 2] = cyy * inv;
        if (a.flags) a.flags[e] = (measured ? 1 : 0) | (degenerate ? 2 : 0);
    }
}

}  // namespace dev

hipError_t launch_pf_init(const PfArgs& a, hipStream_t s) {
    if (a.num_pairs <= 0 || a.num_agents <= 0) return hipSuccess;
    hipLaunchKernelGGL(dev::pf_init_kernel, dim3(a.num_pairs), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pf_step(const PfArgs& a, hipStream_t s) {
    if (a.num_pairs <= 0 || a.num_agents <= 0) return hipSuccess;
    const size_t lds = (size_t)a.num_particles * 4 * sizeof(double);  // a multiple of 16
    hipLaunchKernelGGL(dev::pf_step_kernel, dim3(a.num_pairs), dim3(64), lds, s, a);
    return hipGetLastError();
}

}  // namespace mpccbf
