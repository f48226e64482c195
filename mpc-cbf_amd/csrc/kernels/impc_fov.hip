// impc_fov.hip — the FoV controller's IMPC launch on the state table's neighbour positions
// (impc_fov_kernel<SLACK>, impc_fov.hpp; the estimate form: impc_fov_est.hip) and the per-neighbour
// row evaluation of mpccbf_fov_rows_eval.
#include "impc_fov.hpp"

namespace mpccbf {
namespace dev {

// The FoV controller's per-neighbour rows for `count` (ego, neighbour) pairs, evaluated by the same
// device functions the IMPC kernel uses (mpccbf_fov_rows_eval): Voronoi (nx, ny, 0, off) and the
// four FoV HOCBF rows (a0, a1, a2, b; safety, left, right, range; b = DBL_MAX when absent).
__global__ void __launch_bounds__(64) fov_rows_eval_kernel(int count, const double* __restrict__ ego,
                                                           const double* __restrict__ nb, double fov, double Ds,
                                                           double Rs, double bbx, double bby,
                                                           double* __restrict__ vor, double* __restrict__ rows) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    double e[6];
#pragma unroll
    for (int k = 0; k < 6; k++) e[k] = ego[(size_t)i * 6 + k];
    const double ox = nb[(size_t)i * 2], oy = nb[(size_t)i * 2 + 1];
    if (vor) {
        double nx, ny, off;
        voronoi_row(e[0], e[1], ox, oy, bbx, bby, nx, ny, off);
        vor[(size_t)i * 4 + 0] = nx;
        vor[(size_t)i * 4 + 1] = ny;
        vor[(size_t)i * 4 + 2] = 0.0;
        vor[(size_t)i * 4 + 3] = off;
    }
    if (rows) {
        for (int kind = 0; kind < 4; kind++) {
            double a[3], b;
            bool present;
            fov_cbf_row(kind, e, ox, oy, fov, Ds, Rs, a, b, present);
            double* r = rows + ((size_t)i * 4 + kind) * 4;
            r[0] = a[0];
            r[1] = a[1];
            r[2] = a[2];
            r[3] = b;
        }
    }
}

}  // namespace dev

hipError_t launch_fov_rows_eval(int count, const double* ego, const double* nb, double fov, double Ds, double Rs,
                                double bbx, double bby, double* vor, double* rows, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(dev::fov_rows_eval_kernel, dim3((count + 63) / 64), dim3(64), 0, s, count, ego, nb, fov, Ds,
                       Rs, bbx, bby, vor, rows);
    return hipGetLastError();
}

const int IMPC_FOV_ROWS_MAX = dev::WROWS;

hipError_t launch_impc_fov(ImpcKernel k, int blocks, int block_size, const DevOps& op, const double* buf,
                           const ImpcArgs& a, hipStream_t s) {
    switch (k) {  // (<true> first, as the instantiations have always stood: see launch_impc, impc_kernel.hip)
        case IMPC_FOV_SLACK: return launch_kernel(dev::impc_fov_kernel<true>, blocks, block_size, 0, s, op, buf, a);
        case IMPC_FOV: return launch_kernel(dev::impc_fov_kernel<false>, blocks, block_size, 0, s, op, buf, a);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mpccbf
