// impc_dense.hpp — the dense-layout IMPC kernel (any operators): rows spread over G lanes x R slots
// per agent, dense NZ x NZ normal matrix (pdip.hpp). Steps 1-4 of impc_kernel.hip's mapping.
// Instantiated and launched by impc_kernel.hip (launch_impc_dense).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "impc.hpp"
#include "impc_common.hpp"
#include "pdip.hpp"

namespace mpccbf {
namespace dev {

// One agent of the dense layout on its group of G lanes (gl: the lane in the group), from the state
// load through write_agent_outputs: what impc_kernel runs per group and team_rollout_kernel
// (team_rollout.hip) per robot turn. stage: the group's cap * (NZ + 1) doubles of LDS for the CBF
// rows, cap = R * G - op.m; nbs: the group's scratch of the grid query. Returns whether the agent
// has a new curve (an OPTIMAL iteration).
template <int NZ, int G, int R>
__device__ __forceinline__ bool impc_dense_agent(const DevOps& op, const double* buf, const ImpcArgs& args,
                                                 int ai, int gl, double* stage, NbScratch& nbs) {
    const int cap = R * G - op.m;  // CBF row slots per agent
    const int self = args.agent_first + ai;
    double s0[6];
#pragma unroll
    for (int i = 0; i < 6; i++) s0[i] = args.states[(size_t)self * 6 + i];
    double q[NZ], kconst;
    agent_linear_term<NZ>(op, buf, args, ai, s0, q, kconst);

    // ---- shared rows into register slots
    Rows<NZ, R> rw;
    {
        const double* Gm = opp(buf, op.o_G);
        const double* Gs = opp(buf, op.o_Gs);
        const double* lo = opp(buf, op.o_lo);
        const double* hi = opp(buf, op.o_hi);
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int slot = r * G + gl;
            const bool on = slot < op.m;
            const int si = on ? slot : 0;
            double sh = 0.0;
#pragma unroll
            for (int s = 0; s < 6; s++) sh = fma(Gs[si * 6 + s], s0[s], sh);
#pragma unroll
            for (int j = 0; j < NZ; j++) rw.g[r][j] = on ? Gm[si * NZ + j] : 0.0;
            const double l = lo[si], h = hi[si];
            const bool hl = on && l > -1e300, hu = on && h < 1e300;
            rw.ml[r] = hl ? 1.0 : 0.0;
            rw.mu[r] = hu ? 1.0 : 0.0;
            rw.lo[r] = hl ? l - sh : 0.0;
            rw.hi[r] = hu ? h - sh : 0.0;
        }
    }
    const bool infeasible = constant_rows_infeasible<G>(op, buf, s0, gl);
    stamp(args, ai, gl, 1);

    // ---- neighbours: CSR (caller-provided, e.g. all N-1 others as the reference does) or the
    // k nearest within the radius from the spatial hash (3 x 3 cells around the agent)
    const bool grid_mode = args.nb_row_ptr == nullptr;
    int nb0 = 0, nnb = 0;
    if (!grid_mode) {
        nb0 = args.nb_row_ptr[ai];
        nnb = args.nb_row_ptr[ai + 1] - nb0;
    } else {
        nnb = grid_neighbors<G>(args, self, s0[0], s0[1], nbs, gl);
    }
    const bool nb_overflow = nnb < 0;
    if (nb_overflow) nnb = 0;
    write_nb_out(args, ai, gl, grid_mode, nbs, nb0, nnb);
    stamp(args, ai, gl, 2);

    double y[NZ], ykeep[NZ];
#pragma unroll
    for (int i = 0; i < NZ; i++) y[i] = ykeep[i] = 0.0;
    bool have_curve = false, success = true;
    const PdipCfg cfg{op.maxit, op.tol};

    for (int it = 0; it < op.impc_iter; it++) {
        const size_t oi = (size_t)ai * op.impc_iter + it;
        if (!success) {  // the reference breaks out of the IMPC loop (:208-211)
            write_iteration(args, oi, gl, ST_UNKNOWN, __builtin_nan(""), 0);
            continue;
        }
        bool row_infeasible = false;
        const int count = stage_cbf_rows<NZ, G>(op, buf, args, it, s0, y, grid_mode, &nbs,
                                                nb0, nnb, stage, cap, gl, &row_infeasible);
        if (it < 2) stamp(args, ai, gl, 3 + 2 * it);
        // ---- CBF rows into the free slots (previous iteration's CBF rows are replaced)
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int slot = r * G + gl;
            if (slot >= op.m) {
                const int ci = slot - op.m;
                const bool on = ci < count && ci < cap;
                const double* src = stage + (size_t)(on ? ci : 0) * (NZ + 1);
#pragma unroll
                for (int jz = 0; jz < NZ; jz++) rw.g[r][jz] = on ? src[jz] : 0.0;
                rw.ml[r] = 0.0;
                rw.mu[r] = on ? 1.0 : 0.0;
                rw.lo[r] = 0.0;
                rw.hi[r] = on ? src[NZ] : 0.0;
            }
        }
        int st;
        int nit = 0;
        double prs = __builtin_nan(""), drs = __builtin_nan("");
        bool nfin = false;  // non-finite data: not solved, ERROR (see impc_sep_agent)
#pragma unroll
        for (int j = 0; j < NZ; j++) nfin = nfin || !isfinite(q[j]);
#pragma unroll
        for (int r = 0; r < R; r++) {
            nfin = nfin || !isfinite(rw.lo[r]) || !isfinite(rw.hi[r]);
#pragma unroll
            for (int j = 0; j < NZ; j++) nfin = nfin || !isfinite(rw.g[r][j]);
        }
        if (count > cap || nb_overflow || grp_ballot<G>(nfin) != 0ull) {
            st = ST_ERROR;  // capacity (CBF rows beyond this instantiation's slots) / non-finite data
        } else if (infeasible || row_infeasible) {
            st = ST_INFEASIBLE;
        } else {
            const PdipOut po =
                pdip_solve<NZ, G, R>(rw, opp(buf, op.o_Pr), opp(buf, op.o_LPr), q, y, cfg);
            st = po.status;
            nit = po.iters;
            prs = po.rp;
            drs = po.rd;
            if (st != ST_OPTIMAL) {
                // certify: minimal uniform row violation above the feasibility tolerance
                const double tstar = pdip_phase1<NZ, G, R>(rw, cfg);
                if (tstar > op.feas_tol && tstar < 1e300) {  // (1e300: phase 1 failed, the PDIP decides)
                    st = ST_INFEASIBLE;
                    prs = tstar;
                }
            }
        }
        double objv = __builtin_nan("");
        if (st == ST_OPTIMAL) {
            objv = reduced_objective<NZ>(op, buf, q, y, kconst);
#pragma unroll
            for (int i = 0; i < NZ; i++) ykeep[i] = y[i];
            have_curve = true;
        } else {
            success = false;
        }
        write_iteration(args, oi, gl, st, objv, nit, prs, drs);
        if (it < 2) stamp(args, ai, gl, 4 + 2 * it);
        wave_lds_sync();  // staging is rewritten by the next iteration
    }
    write_agent_outputs<NZ, G>(op, buf, args, ai, gl, s0, ykeep, have_curve);
    stamp(args, ai, gl, 7);
    return have_curve;
}

template <int NZ, int G, int R>
__global__ void __launch_bounds__(256) impc_kernel(const DevOps op, const double* __restrict__ buf,
                                                    const ImpcArgs args) {
    constexpr int GPB = 256 / G;
    const int gl = threadIdx.x & (G - 1);
    const int gib = threadIdx.x / G;
    const int ai = blockIdx.x * GPB + gib;  // agent index within the batch
    grid_clear<256>(args);
    if (ai >= args.num_agents) return;      // whole group leaves together
    stamp(args, ai, gl, 0);

    extern __shared__ double lds_stage[];
    __shared__ NbScratch nb_scratch[GPB];
    double* stage = lds_stage + (size_t)gib * (R * G - op.m) * (NZ + 1);
    impc_dense_agent<NZ, G, R>(op, buf, args, ai, gl, stage, nb_scratch[gib]);
}

}  // namespace dev
}  // namespace mpccbf
