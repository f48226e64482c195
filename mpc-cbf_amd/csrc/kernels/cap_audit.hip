// cap_audit.hip — neighbour-cap audit (mpccbf_cap_audit_run): for every agent of a solved batch, the
// CBF rows of every state row its capped neighbour list dropped, evaluated at the capped QPs' optima.
//
// The QPs are strictly convex in the reduced variables, so the optimum of the capped QP that also
// satisfies every dropped row is the unique optimum of the all-others QP (the reference's lists,
// ConnectivityIMPCCBF.cpp:59-67). A dropped row the acceleration box already implies (b >= bmax, the
// drop rule of stage_cbf_rows) holds at every feasible point, so only the live dropped rows count.
//
// Layout: one agent per wave64, four agents per 256-thread block. The block streams the state table
// through LDS in tiles of 256 rows (px, py, vx, vy), read once per block; the lanes of a wave stride
// over a tile's candidates in ascending index. Membership in the agent's list is a per-wave bitmap
// over the state table in LDS, so lists of any length, order and multiplicity audit alike. The ego
// states and accelerations at the CBF samples come from the full control points (piece lookup and
// monomial Bernstein basis, as curve_component), not from the reduced operators: the audit does
// not depend on the solver's layout. Counts and the (excess, index, sample) maximum are reduced
// across the lanes by shuffles; the live neighbours are compacted by ballot and popcount per
// 64-candidate chunk, so their order is by index. Outputs are deterministic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../../include/mpccbf.h"
#include "cap_audit.hpp"
#include "impc_common.hpp"

namespace mpccbf {
namespace dev {

constexpr int AUDIT_BS = 256;               // threads per block
constexpr int AUDIT_WPB = AUDIT_BS / 64;    // agents (waves) per block
constexpr int AUDIT_TILE = 256;             // state rows per LDS tile
constexpr int AUDIT_SLOTS = 1 + MAX_CBF_H;  // (iteration, sample) pairs: iteration 0's one + iteration 1's

// Component dim of the d-th derivative (EB: the C x C monomials of that derivative's Bernstein
// basis) of the piecewise Bezier curve with control points xr at parameter t
// (SingleParameterPiecewiseCurve::eval: the first piece whose cumulative parameter reaches t, the
// local parameter clamped to the piece).
__device__ double audit_curve(const DevOps& op, const double* buf, const double* EB, const double* xr, double t,
                              int dim) {
    const double* cum = opp(buf, op.o_cum);
    int piece = 0;
    while (piece < op.P - 1 && cum[piece] < t) piece++;
    const double par = piece == 0 ? fmin(cum[0], t) : fmin(cum[0], t - cum[piece - 1]);
    const int C = op.C;
    double v = 0.0;
    for (int cp = 0; cp < C; cp++) {
        double b = 0.0, tp = 1.0;
        for (int j = 0; j < C; j++, tp *= par) b = fma(EB[cp * C + j], tp, b);
        v = fma(xr[piece * 3 * C + dim * C + cp], b, v);
    }
    return v;
}

// (a, ja, ka) before (b, jb, kb): the larger scaled excess, ties to the smaller index, then the
// smaller sample; j < 0 = none
__device__ __forceinline__ bool audit_before(double a, int ja, int ka, double b, int jb, int kb) {
    if (ja < 0) return false;
    if (jb < 0) return true;
    return a > b || (a == b && (ja < jb || (ja == jb && ka < kb)));
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(AUDIT_BS) void cap_audit_kernel(const DevOps op, const double* __restrict__ buf,
                                                             const AuditArgs a) {
    extern __shared__ double audit_lds[];
    // [4][AUDIT_TILE] state planes | [AUDIT_WPB][AUDIT_SLOTS][6] samples | [AUDIT_WPB][words] bitmaps
    double* tile = audit_lds;
    double* smp_all = tile + 4 * AUDIT_TILE;
    uint32_t* bits_all = reinterpret_cast<uint32_t*>(smp_all + AUDIT_WPB * AUDIT_SLOTS * 6);
    const int words = (a.num_states + 31) >> 5;
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int ai = (int)blockIdx.x * AUDIT_WPB + wave;
    const bool active = ai < a.num_agents;
    const int self = a.agent_first + ai;
    const int ns = a.num_states;
    double* smp = smp_all + wave * AUDIT_SLOTS * 6;
    uint32_t* bits = bits_all + (size_t)wave * words;

    int st0 = MPCCBF_UNKNOWN, st1 = MPCCBF_UNKNOWN;
    if (active) {
        st0 = a.status[(size_t)ai * a.impc_iter];
        if (a.impc_iter > 1) st1 = a.status[(size_t)ai * a.impc_iter + 1];
    }
    const bool has1 = a.impc_iter > 1 && st0 == MPCCBF_OPTIMAL;  // iteration 1 had a QP
    const bool solved0 = st0 == MPCCBF_OPTIMAL, solved1 = has1 && st1 == MPCCBF_OPTIMAL;
    const int nk1 = has1 ? op.cbf_h : 0;

    // membership bitmap: the agent itself and its list
    if (active)
        for (int w = lane; w < words; w += 64) bits[w] = 0u;
    __syncthreads();
    bool bad = false;  // a non-finite ego or listed state: the QP's data is not finite
    if (active) {
        if (lane == 0) atomicOr(&bits[self >> 5], 1u << (self & 31));
        if (lane < 6) bad = !isfinite(a.states[(size_t)self * 6 + lane]);
        if (a.nb_row_ptr) {
            const int r0 = a.nb_row_ptr[ai], r1 = a.nb_row_ptr[ai + 1];
            for (int p = r0 + lane; p < r1; p += 64) {
                const int j = a.nb_col[p];
                if (j < 0 || j >= ns) continue;
                atomicOr(&bits[j >> 5], 1u << (j & 31));
                const double* s = a.states + (size_t)j * 6;
                bad = bad || !(isfinite(s[0]) && isfinite(s[1]) && isfinite(s[3]) && isfinite(s[4]));
            }
        } else {
            const int j = lane < 16 ? a.nb_list[(size_t)ai * 16 + lane] : -1;
            // (-1 after the last entry: nothing follows the first -1)
            const unsigned long long neg = __ballot(lane < 16 && j < 0);
            const int cnt = neg ? __ffsll((long long)neg) - 1 : 16;
            if (lane < cnt && j >= 0 && j < ns) {
                atomicOr(&bits[j >> 5], 1u << (j & 31));
                const double* s = a.states + (size_t)j * 6;
                bad = bad || !(isfinite(s[0]) && isfinite(s[1]) && isfinite(s[3]) && isfinite(s[4]));
            }
        }
        // ego states and accelerations at the samples: lane 6 s + c holds component c of slot s,
        // c = px, py, vx, vy, ax, ay; slot 0 is iteration 0 (the agent's state, the iteration-0
        // curve's acceleration at 0), slot 1 + k is iteration 1's sample k (the iteration-0 curve at
        // h k, the iteration-1 curve's acceleration there)
        const int slot = lane / 6, c = lane % 6;
        if (slot < 1 + nk1) {
            const double* x0r = a.x0 + (size_t)ai * op.n;
            const double* x1r = a.x + (size_t)ai * op.n;
            const double* EB2 = opp(buf, a.o_EB2);
            double v = __builtin_nan("");
            if (slot == 0) {
                if (c < 4) v = a.states[(size_t)self * 6 + (c < 2 ? c : c + 1)];
                else if (solved0) v = audit_curve(op, buf, EB2, x0r, 0.0, c - 4);
            } else {
                const double t = a.h * (double)(slot - 1);
                if (c < 2) v = audit_curve(op, buf, opp(buf, op.o_EB0), x0r, t, c);
                else if (c < 4) v = audit_curve(op, buf, opp(buf, op.o_EB1), x0r, t, c - 2);
                else if (solved1) v = audit_curve(op, buf, EB2, x1r, t, c - 4);
            }
            smp[slot * 6 + c] = v;
        }
    }
    bad = __ballot(bad) != 0ull;
    __syncthreads();

    int in_list = 0;
    if (active)
        for (int w = lane; w < words; w += 64) in_list += __popc(bits[w]);
    in_list = wave_sum(in_list);  // (the agent itself included)

    int nlive[2] = {0, 0}, nviol[2] = {0, 0};
    double best[2] = {0.0, 0.0};
    int bj[2] = {-1, -1}, bk[2] = {0, 0};
    int nout = 0;  // live neighbours written so far (wave-uniform)
    const double tol = a.tol;

    for (int t0 = 0; t0 < ns; t0 += AUDIT_TILE) {
        __syncthreads();  // (the previous tile is read)
        {
            const int j = t0 + (int)threadIdx.x;
            double px = 0.0, py = 0.0, vx = 0.0, vy = 0.0;
            if (j < ns) {
                const double* s = a.states + (size_t)j * 6;
                px = s[0];
                py = s[1];
                vx = s[3];
                vy = s[4];
            }
            tile[0 * AUDIT_TILE + threadIdx.x] = px;
            tile[1 * AUDIT_TILE + threadIdx.x] = py;
            tile[2 * AUDIT_TILE + threadIdx.x] = vx;
            tile[3 * AUDIT_TILE + threadIdx.x] = vy;
        }
        __syncthreads();
        if (!active || bad) continue;
        for (int cb = 0; cb < AUDIT_TILE; cb += 64) {
            if (t0 + cb >= ns) break;
            const int tl = cb + lane, j = t0 + tl;
            bool dropped = false;
            if (j < ns) dropped = ((bits[j >> 5] >> (j & 31)) & 1u) == 0u;
            bool any_live = false;
            if (dropped) {
                const double npx = tile[tl], npy = tile[AUDIT_TILE + tl];
                const double nvx = tile[2 * AUDIT_TILE + tl], nvy = tile[3 * AUDIT_TILE + tl];
                for (int s = 0; s < 1 + nk1; s++) {
                    const double* q = smp + s * 6;
                    const double e[6] = {q[0], q[1], 0.0, q[2], q[3], 0.0};
                    double ar[3], b;
                    safety_cbf(e, npx, npy, nvx, nvy, op.d_min, ar, b);
                    double bmax = 0.0;
#pragma unroll
                    for (int d = 0; d < 3; d++) bmax += fmax(-ar[d] * op.a_lo[d], -ar[d] * op.a_hi[d]);
                    if (!(isfinite(b) && isfinite(bmax)) || b >= bmax) continue;  // not live
                    const int it = s == 0 ? 0 : 1, k = s == 0 ? 0 : s - 1;
                    any_live = true;
                    nlive[it]++;
                    if (!(it == 0 ? solved0 : solved1)) continue;
                    const double v = -(ar[0] * q[4] + ar[1] * q[5]) - b;
                    const double sc = v / (1.0 + fabs(b));
                    if (sc > tol) nviol[it]++;
                    if (audit_before(sc, j, k, best[it], bj[it], bk[it])) {
                        best[it] = sc;
                        bj[it] = j;
                        bk[it] = k;
                    }
                }
            }
            const unsigned long long m = __ballot(any_live);
            if (a.live_nb && any_live) {
                const int pos = nout + __popcll(m & ((1ull << lane) - 1ull));
                if (pos < AUDIT_LIVE_NB) a.live_nb[(size_t)ai * AUDIT_LIVE_NB + pos] = j;
            }
            nout += __popcll(m);
        }
    }
    if (!active) return;

#pragma unroll
    for (int it = 0; it < 2; it++) {
        nlive[it] = wave_sum(nlive[it]);
        nviol[it] = wave_sum(nviol[it]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best[it], o, 64);
            const int oj = __shfl_xor(bj[it], o, 64), ok = __shfl_xor(bk[it], o, 64);
            if (audit_before(ob, oj, ok, best[it], bj[it], bk[it])) {
                best[it] = ob;
                bj[it] = oj;
                bk[it] = ok;
            }
        }
    }
    if (a.live_nb && lane < AUDIT_LIVE_NB && lane >= nout) a.live_nb[(size_t)ai * AUDIT_LIVE_NB + lane] = -1;
    if (lane != 0) return;
    const bool no1 = !has1;
    int bitsw = 0;
    if (!bad) {
        const bool c0 = (solved0 && nviol[0] == 0) || st0 == MPCCBF_INFEASIBLE;
        const bool c1 = c0 && (no1 || (st1 == MPCCBF_OPTIMAL && nviol[1] == 0) || st1 == MPCCBF_INFEASIBLE);
        bitsw = (c0 ? 1 : 0) | (c1 ? 2 : 0);
    }
    int32_t* cw = a.counts + (size_t)ai * AUDIT_WORDS;
    cw[0] = nlive[0];
    cw[1] = nviol[0];
    cw[2] = no1 ? -1 : nlive[1];
    cw[3] = no1 ? -1 : nviol[1];
    cw[4] = bj[0];
    cw[5] = no1 ? -1 : bj[1];
    cw[6] = ns - in_list;
    cw[7] = bitsw;
    if (a.excess) {
        a.excess[(size_t)ai * 2] = bj[0] >= 0 ? best[0] : __builtin_nan("");
        a.excess[(size_t)ai * 2 + 1] = (!no1 && bj[1] >= 0) ? best[1] : __builtin_nan("");
    }
}

}  // namespace dev

size_t cap_audit_lds_bytes(int num_states) {
    const size_t words = ((size_t)num_states + 31) >> 5;
    return (size_t)(4 * dev::AUDIT_TILE + dev::AUDIT_WPB * dev::AUDIT_SLOTS * 6) * sizeof(double) +
           (size_t)dev::AUDIT_WPB * words * sizeof(uint32_t);
}

hipError_t launch_cap_audit(const DevOps& op, const double* buf, const AuditArgs& a, hipStream_t s) {
    if (a.num_agents <= 0) return hipSuccess;
    if (a.num_states > AUDIT_MAX_STATES) return hipErrorInvalidValue;
    const int blocks = (a.num_agents + dev::AUDIT_WPB - 1) / dev::AUDIT_WPB;
    hipLaunchKernelGGL(dev::cap_audit_kernel, dim3(blocks), dim3(dev::AUDIT_BS), cap_audit_lds_bytes(a.num_states), s,
                       op, buf, a);
    return hipGetLastError();
}

}  // namespace mpccbf
