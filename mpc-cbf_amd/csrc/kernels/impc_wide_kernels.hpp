// impc_wide_kernels.hpp — the one-agent-per-wave IMPC kernels: the agent pipeline (impc_wide_agent,
// on impc_wide.hpp's lane layout and solver) and its two __global__ wrappers: plain
// (impc_wide_kernel, instantiated by impc_kernel.hip) and with the active-set store
// (impc_wide_store_kernel, impc_store.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "impc.hpp"
#include "impc_common.hpp"
#include "impc_wide.hpp"
#include "active_store.hpp"

namespace mpccbf {
namespace dev {

__device__ __forceinline__ void wide_defer(const ImpcArgs& args, int ai, int gl) {
    if (gl == 0) {
        const int slot = atomicAdd(&args.defer[0], 1);
        args.defer[2 + slot] = ai;
    }
}

// STORE: as impc_sep_agent's (astore: this wave's LDS, the staged CBF rows' keys then the record).
template <bool STORE>
__device__ void impc_wide_agent(const DevOps& op, const double* __restrict__ buf, const ImpcArgs& args, const int ai,
                                WideLds& L, int32_t* astore = nullptr, const StoreArgs store = StoreArgs{nullptr, 0}) {
    constexpr int NZ = SEP_NZ;
    const int gl = (int)(threadIdx.x & 63u);
    stamp(args, ai, gl, 0);
    const int self = args.agent_first + ai;
    // (the record's load goes first: it has arrived when the state, issued after it, has)
    int rec_in = 0;
    if constexpr (STORE)
        if (gl < AS_WORDS) rec_in = store.records[(size_t)self * AS_WORDS + gl];
    const lds_vptr<int32_t> tags = lds_vol(astore);
    const lds_vptr<int32_t> rec = lds_vol(astore + (STORE ? W_CBF : 0));
    double s0[6];
#pragma unroll
    for (int i = 0; i < 6; i++) s0[i] = args.states[(size_t)self * 6 + i];
    early_noise(args, ai, gl, L.noise);  // (while the state is in flight)
    const bool grid_mode = args.nb_row_ptr == nullptr;
    WideQuery gq;
    WideCells gc;
    if (grid_mode) wn_issue(args, s0[0], s0[1], gl, gq);
    // linear term: lane i < 6 forms q_i, the constant's terms summed over the first 16-lane row
    // (agent_linear_term_lanes; lanes >= 9 contribute 0, so the row total is the whole sum)
    double kconst;
    const double qlane = agent_linear_term_lanes<NZ, 16>(op, buf, args, ai, s0, gl, kconst);
    // this lane's box row: channel d = gl / 16, slot gl % 16 (host layout [channel][16][SEP_ROW])
    WRow rw;
    {
        const int lb = gl < W_BOX ? gl : 0;
        const double* r = opp(buf, op.o_Gsep) + (size_t)lb * SEP_ROW;
        double rv[SEP_ROW];
#pragma unroll
        for (int i = 0; i < SEP_ROW; i++) rv[i] = r[i];
        double sh = 0.0;
#pragma unroll
        for (int s = 0; s < 6; s++) sh = fma(rv[2 + s], s0[s], sh);
        const int d = gl >> 4;
#pragma unroll
        for (int j = 0; j < NZ; j++) rw.g[j] = 0.0;
        if (gl < W_BOX) {
#pragma unroll
            for (int dd = 0; dd < SEP_D; dd++)
                if (dd == d) {
                    rw.g[2 * dd] = rv[0];
                    rw.g[2 * dd + 1] = rv[1];
                }
        }
        rw.lo = gl < W_BOX ? rv[8] - sh : -1e300;
        rw.hi = gl < W_BOX ? rv[9] - sh : 1.0;
        const double* pd = opp(buf, op.o_Pinv) + 3 * (d < SEP_D ? d : 0);
        rw.w = wide_weight(wide_n2(pd[0], pd[1], pd[2], rv[0], rv[1]));
        rw.sl = rcp(1.0 + fabs(rw.lo));
        rw.su = rcp(1.0 + fabs(rw.hi));
    }
    wide_sample_us(op, buf, s0, L, gl);
    if constexpr (STORE)
        if (gl < AS_WORDS) rec[gl] = rec_in;
    if (grid_mode) wn_cells(args, gq, gc);
    const bool infeasible = constant_rows_infeasible<64>(op, buf, s0, gl);
    stamp(args, ai, gl, 1);

    int nb0 = 0, nnb = 0;
    if (!grid_mode) {
        nb0 = args.nb_row_ptr[ai];
        nnb = args.nb_row_ptr[ai + 1] - nb0;
    } else {
        nnb = wn_finish(args, self, s0[0], s0[1], gc, gq, L, gl);
    }
    nnb = uni_i(nnb);
    if (args.nb_out && gl < 16)  // diagnostics: the list the rows are built from
        args.nb_out[(size_t)ai * 16 + gl] = gl < nnb ? (grid_mode ? L.nbi[gl] : args.nb_col[nb0 + gl]) : -1;
    const bool nb_overflow = nnb < 0;
    if (nb_overflow) nnb = 0;
    stamp(args, ai, gl, 2);

    double q[NZ], yu[NZ];
#pragma unroll
    for (int j = 0; j < NZ; j++) q[j] = lane_of(qlane, j);
    kconst = uni(kconst);
    const double* Pinv = opp(buf, op.o_Pinv);
#pragma unroll
    for (int d = 0; d < SEP_D; d++) {  // the unconstrained minimiser -P^-1 q (both IMPC iterations)
        const int o = 2 * d;
        yu[o] = -fma(Pinv[3 * d], q[o], Pinv[3 * d + 1] * q[o + 1]);
        yu[o + 1] = -fma(Pinv[3 * d + 1], q[o], Pinv[3 * d + 2] * q[o + 1]);
    }
    // non-finite data (a NaN / Inf state, target or neighbour state): such a model is not solved
    // (CPLEX rejects non-finite coefficients), ERROR; the linear term and the box rows are checked
    // here, the CBF rows per iteration
    bool nfin_fixed;
    {
        bool nf = gl < W_BOX && (!isfinite(rw.lo) || !isfinite(rw.hi));
#pragma unroll
        for (int j = 0; j < NZ; j++) nf = nf || !isfinite(q[j]);
        nfin_fixed = __ballot(nf) != 0ull;
    }
#ifdef MPCCBF_PDIP_STAMPS
    long long* wdbg = args.stamps ? (long long*)args.stamps + (size_t)args.num_agents * NSTAMP + (size_t)ai * 16 : nullptr;
#else
    long long* wdbg = nullptr;
#endif
    double y[NZ], yk[NZ];
#pragma unroll
    for (int j = 0; j < NZ; j++) y[j] = yk[j] = 0.0;
    bool have_curve = false, success = true;
    if (gl == 0) L.act[POL_K] = 0.0;
    int steps0 = 0;
    int k0_off = 0, rec_out = 0;  // STORE: the sides iteration 0 was offered; this lane's record word
    // per-iteration results, written together after the loop (impc_iter <= 2 here; more iterations
    // are written as they finish)
    int st_w0 = ST_UNKNOWN, st_w1 = ST_UNKNOWN, nit_w0 = 0, nit_w1 = 0;
    double obj_w0 = __builtin_nan(""), obj_w1 = __builtin_nan(""), prs_w0 = obj_w0, prs_w1 = obj_w0,
           drs_w0 = obj_w0, drs_w1 = obj_w0;
    const bool want_rp = args.primal_res != nullptr;

    for (int it = 0; it < op.impc_iter; it++) {
        const size_t oi = (size_t)ai * op.impc_iter + it;
        if (!success) {  // the reference breaks out of the IMPC loop (:208-211)
            if (it >= 2) write_iteration(args, oi, gl, ST_UNKNOWN, __builtin_nan(""), 0);
            continue;
        }
        bool row_infeasible = false;
        long long* wd = it == 0 ? wdbg : nullptr;
        const int count =
            uni_i(wide_cbf_rows<STORE>(op, buf, args, it, s0, y, grid_mode, L, nb0, nnb, gl, row_infeasible, wd, astore));
        bool nfin = false;
        if (gl >= W_BOX) {  // this iteration's CBF rows into the CBF lanes (unused: inert 0 <= 1)
            const int c = gl - W_BOX;
            const bool on = c < count;
            const double* src = L.stage + (on ? c : 0) * W_ROW;
#pragma unroll
            for (int j = 0; j < 4; j++) rw.g[j] = on ? src[j] : 0.0;
            rw.hi = on ? src[4] : 1.0;
            rw.w = wide_weight(wide_n2(Pinv[0], Pinv[1], Pinv[2], rw.g[0], rw.g[1]) +
                               wide_n2(Pinv[3], Pinv[4], Pinv[5], rw.g[2], rw.g[3]));
            rw.su = rcp(1.0 + fabs(rw.hi));
            nfin = !isfinite(rw.hi) || !isfinite(rw.g[0]) || !isfinite(rw.g[1]) || !isfinite(rw.g[2]) ||
                   !isfinite(rw.g[3]);
        }
        {
            long long* wdbg = wd;
            (void)wdbg;
            WST(4);
        }
        if (it < 2) stamp(args, ai, gl, 3 + 2 * it);
        if (count > W_CBF) {  // beyond the 16 CBF lanes: the fallback launch (8 slots per lane)
            if (args.defer) {
                wide_defer(args, ai, gl);
                return;
            }
        }
        const bool nonfinite = nfin_fixed || __ballot(nfin) != 0ull;
        int st, nit = 0;
        double prs = __builtin_nan(""), drs = __builtin_nan("");
        if (count > W_CBF || nb_overflow || nonfinite) {
            st = ST_ERROR;
        } else if (infeasible || row_infeasible) {
            st = ST_INFEASIBLE;
        } else {
            int k0 = 0;
            if constexpr (STORE) {
                // (as impc_sep_agent's warm_count)
                wave_lds_sync();
                if (it == 0) {
                    k0 = as_map_wide(rec, tags, count, op.sep_rows_per_dim, store.min_steps, gl, L.act);
                } else if (op.das_warm > 0) {
                    const int kf = (int)L.act[POL_K];
                    if (kf > 0 && (steps0 >= op.das_warm || (k0_off > 0 && kf >= 2))) k0 = kf;
                }
                k0 = uni_i(k0);
                wave_lds_sync();
                if (gl == 0) L.act[POL_K] = -1.0;
                k0_off = k0;
            } else if (it > 0 && op.das_warm > 0 && steps0 >= op.das_warm) {
                wave_lds_sync();
                k0 = uni_i((int)L.act[POL_K]);
            }
            double tl = 0.0;
            const int r = wide_dual_as(rw, opp(buf, op.o_Pr), Pinv, q, yu, op.tol, op.dual_as, L.pol, y, prs, drs,
                                       nit, tl, k0, L.act, (STORE || it == 0) ? L.act : nullptr, want_rp, wd);
            if (r > 0) {
                st = ST_OPTIMAL;
                if (!want_rp) prs = __builtin_nan("");
            } else if (r < 0 && tl > 10.0 * op.feas_tol) {
                st = ST_INFEASIBLE;
                prs = tl;
                drs = __builtin_nan("");
            } else {
                if (args.defer) {
                    wide_defer(args, ai, gl);
                    return;
                }
                st = ST_UNKNOWN;
            }
        }
        double objv = __builtin_nan("");
        if (st == ST_OPTIMAL) {
            // 1/2 y^T P y + q^T y + k (reduced_objective) on the first 16-lane row: lane i < 6 row i
            const double* Pr = opp(buf, op.o_Pr) + (size_t)(gl < NZ ? gl : 0) * NZ;
            double pr[NZ], pyi = 0.0, yi = y[0], qi = q[0];
#pragma unroll
            for (int j = 0; j < NZ; j++) pr[j] = Pr[j];
#pragma unroll
            for (int j = 1; j < NZ; j++) {
                yi = gl == j ? y[j] : yi;
                qi = gl == j ? q[j] : qi;
            }
#pragma unroll
            for (int j = 0; j < NZ; j++) pyi = fma(pr[j], y[j], pyi);
            objv = grp_sum<16>(gl < NZ ? yi * (0.5 * pyi + qi) : (gl == NZ ? kconst : 0.0));
#pragma unroll
            for (int i = 0; i < NZ; i++) yk[i] = y[i];
            have_curve = true;
            if constexpr (STORE) {
                wave_lds_sync();
                rec_out = as_word_wide(L.act, tags, nit + k0_off, it, gl);
            }
        } else {
            success = false;
        }
        {
            long long* wdbg = wd;
            (void)wdbg;
            WST(12);
        }
        if (it == 0) {
            st_w0 = st, nit_w0 = nit, obj_w0 = objv, prs_w0 = prs, drs_w0 = drs;
        } else if (it == 1) {
            st_w1 = st, nit_w1 = nit, obj_w1 = objv, prs_w1 = prs, drs_w1 = drs;
        } else {
            write_iteration(args, oi, gl, st, objv, nit, prs, drs);
        }
        if (it == 0) steps0 = nit;
        if (it < 2) stamp(args, ai, gl, 4 + 2 * it);
    }
    write_iteration(args, (size_t)ai * op.impc_iter, gl, st_w0, obj_w0, nit_w0, prs_w0, drs_w0);
    if (op.impc_iter > 1) write_iteration(args, (size_t)ai * op.impc_iter + 1, gl, st_w1, obj_w1, nit_w1, prs_w1, drs_w1);
    write_agent_outputs<NZ, 64>(op, buf, args, ai, gl, s0, yk, have_curve, L.noise);
    if constexpr (STORE)
        if (gl < AS_WORDS) store.records[(size_t)self * AS_WORDS + gl] = rec_out;
    stamp(args, ai, gl, 7);
}

// The operators (the buffer's hot prefix, DevOps::hot doubles) are staged into LDS once per block,
// while the agents' state loads are in flight: every operator read of the agent chain is then an
// LDS read (~100 cycles) instead of a scalar / vector memory round trip (~1,000 cycles under load).
template <int BS>
__global__ void __launch_bounds__(BS) impc_wide_kernel(const DevOps op, const double* __restrict__ buf,
                                                        const ImpcArgs args) {
    constexpr int WPB = BS / 64;
    constexpr int PER = WIDE_OPS / BS;
    __shared__ WideLds lds_all[WPB];
    __shared__ double ops[WIDE_OPS];
    lds_poison();
    kclock_start(args);
    {
        double v[PER];
#pragma unroll
        for (int r = 0; r < PER; r++) {
            const int i = r * BS + (int)threadIdx.x;
            v[r] = i < op.hot ? buf[i] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < PER; r++) ops[r * BS + threadIdx.x] = v[r];
    }
    grid_clear<BS>(args);
    __syncthreads();
    const int wv = uni_i((int)(threadIdx.x >> 6));
    const int ai = xcd_block((int)blockIdx.x, (int)gridDim.x) * WPB + wv;
    if (ai >= args.num_agents) return;
    impc_wide_agent<false>(op, ops, args, ai, lds_all[wv]);
    kclock_end<BS>(args);
}

// impc_wide_kernel with the active-set store attached (a kernel of its own, as impc_sep_store_kernel)
template <int BS>
__global__ void __launch_bounds__(BS) impc_wide_store_kernel(const DevOps op, const double* __restrict__ buf,
                                                              const ImpcArgs args, const StoreArgs store) {
    constexpr int WPB = BS / 64;
    constexpr int PER = WIDE_OPS / BS;
    __shared__ WideLds lds_all[WPB];
    __shared__ double ops[WIDE_OPS];
    __shared__ int32_t astore_all[WPB][W_CBF + AS_WORDS];  // the staged CBF rows' keys, then the agent's record
    lds_poison();
    kclock_start(args);
    {
        double v[PER];
#pragma unroll
        for (int r = 0; r < PER; r++) {
            const int i = r * BS + (int)threadIdx.x;
            v[r] = i < op.hot ? buf[i] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < PER; r++) ops[r * BS + threadIdx.x] = v[r];
    }
    grid_clear<BS>(args);
    __syncthreads();
    const int wv = uni_i((int)(threadIdx.x >> 6));
    const int ai = xcd_block((int)blockIdx.x, (int)gridDim.x) * WPB + wv;
    if (ai >= args.num_agents) return;
    impc_wide_agent<true>(op, ops, args, ai, lds_all[wv], astore_all[wv], store);
    kclock_end<BS>(args);
}

}  // namespace dev
}  // namespace mpccbf
