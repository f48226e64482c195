// impc_sep.hpp — the separable-layout IMPC kernels (x / y / yaw channels, 2 reduced variables each;
// pdip_sep.hpp): one agent per 16-lane group, lane l holds box row l of each channel and CBF row l.
// The agent pipeline (impc_sep_agent) and its three __global__ wrappers: plain (impc_sep_kernel,
// instantiated by impc_kernel.hip), with the active-set store (impc_sep_store_kernel,
// impc_store.hip) and with connectivity rows (impc_sep_conn_kernel, impc_conn.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "impc.hpp"
#include "impc_common.hpp"
#include "active_store.hpp"
#include "pdip.hpp"
#include "pdip_sep.hpp"
#include "conn_rows_dev.hpp"

namespace mpccbf {
namespace dev {

// Slack mode: a lane builds the CBF rows of its neighbour (list position jn, -1: none) itself
// (slot k = sample k), so all rows of one slack variable live in the lane that owns it. Filtered
// rows stay inert (ccv = 0). Returns whether some row of this lane is live.
template <int SB, int CB>
__device__ bool lane_cbf_rows(const DevOps& op, const double* buf, const ImpcArgs& args, int it,
                              const double (&s0)[6], const double (&y)[SEP_NZ], bool grid_mode,
                              const int32_t* nbl, int nb0, int jn, SepRows<SB, CB>& rw) {
    const double* UZ = opp(buf, op.o_UZ);
    const double* US = opp(buf, op.o_US);
    const int nk = (it == 0) ? 1 : op.cbf_h;
    bool live = false;
#pragma unroll
    for (int k = 0; k < CB; k++) {
#pragma unroll
        for (int j = 0; j < 4; j++) rw.cg[k][j] = 0.0;
        rw.chi[k] = 1.0;
        rw.ccv[k] = 0.0;
        if (k < nk && jn >= 0) {
            double e[6];
            cbf_ego_state<SEP_NZ>(op, buf, it, k, s0, y, e);
            const int nbi = grid_mode ? nbl[jn] : args.nb_col[nb0 + jn];
            const double* ns = args.states + (size_t)nbi * 6;
            double a[3], b;
            safety_cbf(e, ns[0], ns[1], ns[3], ns[4], op.d_min, a, b);
            double bmax = 0.0;
#pragma unroll
            for (int d = 0; d < 3; d++) bmax += fmax(-a[d] * op.a_lo[d], -a[d] * op.a_hi[d]);
            if (!(op.cbf_filter && b >= bmax)) {  // implied by the acceleration box: drop
                const double* UZk = UZ + (size_t)k * 3 * SEP_NZ;
                const double* USk = US + (size_t)k * 18;
                double us = 0.0;
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    double v = 0.0;
#pragma unroll
                    for (int s = 0; s < 6; s++) v = fma(USk[d * 6 + s], s0[s], v);
                    us = fma(a[d], v, us);
                }
#pragma unroll
                for (int j = 0; j < 4; j++)
                    rw.cg[k][j] = -(a[0] * UZk[j] + a[1] * UZk[SEP_NZ + j] + a[2] * UZk[2 * SEP_NZ + j]);
                rw.chi[k] = b + us;
                rw.ccv[k] = 1.0;
                live = true;
            }
        }
    }
    return live;
}

// Whether neighbour jn (-1: none) has a CBF row the acceleration box does not imply (the filter of
// lane_cbf_rows without the row coefficients).
__device__ bool lane_cbf_live(const DevOps& op, const double* buf, const ImpcArgs& args, int it,
                              const double (&s0)[6], const double (&y)[SEP_NZ], bool grid_mode,
                              const int32_t* nbl, int nb0, int jn) {
    if (jn < 0) return false;
    const int nk = (it == 0) ? 1 : op.cbf_h;
    const int nbi = grid_mode ? nbl[jn] : args.nb_col[nb0 + jn];
    const double* ns = args.states + (size_t)nbi * 6;
    bool live = false;
    for (int k = 0; k < nk; k++) {
        double e[6], a[3], b;
        cbf_ego_state<SEP_NZ>(op, buf, it, k, s0, y, e);
        safety_cbf(e, ns[0], ns[1], ns[3], ns[4], op.d_min, a, b);
        double bmax = 0.0;
#pragma unroll
        for (int d = 0; d < 3; d++) bmax += fmax(-a[d] * op.a_lo[d], -a[d] * op.a_hi[d]);
        live = live || !(op.cbf_filter && b >= bmax);
    }
    return live;
}

template <int G>
__device__ double lane_slack_weight(const DevOps& op, const ImpcArgs& args, const double (&s0)[6],
                                    bool grid_mode, const int32_t* nbl, int nb0, int nnb, int jn);

// Slack mode with more than G neighbours: the ones with a live row in IMPC iteration `it` are
// compacted into the lanes (lane l takes the l-th: jn, its weight); returns their count (more than
// G: capacity exceeded, jn = -1). State and kept solution from LDS.
template <int G>
__device__ int slack_compact(const DevOps& op, const double* buf, const ImpcArgs& args, int it,
                                          const double* s0k, const double* ykeep, bool grid_mode,
                                          const int32_t* nbl, int nb0, int nnb, int gl, int& jn,
                                          double& wslack) {
    double sx[6], y[SEP_NZ];
#pragma unroll
    for (int i = 0; i < 6; i++) sx[i] = s0k[i];
#pragma unroll
    for (int i = 0; i < SEP_NZ; i++) y[i] = ykeep[16 * i];
    int nlive = 0;
    jn = -1;
    for (int base = 0; base < nnb; base += G) {
        const bool lv = lane_cbf_live(op, buf, args, it, sx, y, grid_mode, nbl, nb0, base + gl < nnb ? base + gl : -1);
        const unsigned long long msk = grp_ballot<G>(lv);
        const int want = gl - nlive;
        int c = 0;
        for (int b = 0; b < G; b++) {
            if ((msk >> b) & 1ull) {
                if (c == want) jn = base + b;
                c++;
            }
        }
        nlive += c;
    }
    if (nlive > G) jn = -1;
    wslack = lane_slack_weight<G>(op, args, sx, grid_mode, nbl, nb0, nnb, jn);
    return nlive;
}

// Slack weight of the lane's neighbour (list position jn, -1: none): slack_cost * decay^rank,
// rank by planar distance among all nnb neighbours (ConnectivityIMPCCBF.cpp:73-100; ties by list
// position — the reference's std::sort leaves them unspecified). Lanes without a neighbour get
// cost 1 (their slack has no rows: v -> 0). Up to G neighbours by lane shuffles, beyond by a
// scan of the whole list.
template <int G>
__device__ double lane_slack_weight(const DevOps& op, const ImpcArgs& args, const double (&s0)[6],
                                    bool grid_mode, const int32_t* nbl, int nb0, int nnb, int jn) {
    auto dist_of = [&](int j) {
        const int nbi = grid_mode ? nbl[j] : args.nb_col[nb0 + j];
        const double dx = args.states[(size_t)nbi * 6] - s0[0], dy = args.states[(size_t)nbi * 6 + 1] - s0[1];
        return sqrt(dx * dx + dy * dy);
    };
    const double dist = jn >= 0 ? dist_of(jn) : 0.0;
    int rank = 0;
    if (nnb <= G) {  // (jn = this lane's index)
        for (int k = 0; k < nnb; k++) {
            const double dk = __shfl(dist, k, G);
            rank += (dk < dist || (dk == dist && k < jn)) ? 1 : 0;
        }
    } else {
        for (int k = 0; k < nnb; k++) {
            const double dk = dist_of(k);
            rank += (dk < dist || (dk == dist && k < jn)) ? 1 : 0;
        }
    }
    return jn >= 0 ? op.slack_cost * pow(op.slack_decay, (double)rank) : 1.0;
}

// Slack-pattern active set of the collision slack mode (ConnectivityIMPCCBF.cpp:73-119,
// MPCCBFQPGeneratorBase.cpp:28-130; the FoV kernel's run_patterns on the separable layout). Lane l
// owns neighbour l's slack v_l >= 0 (cost w) and its CBF rows g_c y - v_l <= h_c (slots c with
// ccv = 1). A pattern fixes per lane either v_l = 0 (lead = -1: its rows hard, g_c y <= h_c) or a
// leader slot l with v_l = g_l y - h_l >= 0: w g_l joins the linear term, the other rows become
// (g_c - g_l) y <= h_c - h_l and the leader's own row the bound -g_l y <= -h_l. Each pattern is a
// strictly convex QP in y alone, solved exactly by sep_dual_as; it is the slack QP's optimum when
// every lane's multipliers are consistent — v_l = 0: the rows' multipliers sum to at most w
// (stationarity in v, the bound's multiplier w - sum >= 0); led: the leader row's implied
// multiplier w - sum(others) - mu >= 0 (mu: the bound's). Otherwise a lane over its cost takes its
// largest-multiplier row as leader, a led lane with a negative leader multiplier its other active
// row; a pattern without a feasible point lets the unreachable candidate's row lead when that is a
// CBF row of a lane without a leader. lead: per lane, in (the first pattern) and out. Returns 1 with
// yo, vo (this lane's slack), the residuals and the summed steps; 0: no consistent pattern found
// (the caller's PDIP solves). mult: 16 doubles of the group's LDS (sep_dual_as's multipliers).
template <int G, int SB, int CB>
__device__ int sep_slack_patterns(const SepRows<SB, CB>& rw, double w, int& lead, const double* __restrict__ P,
                                  const double* __restrict__ Pinv, const double (&q)[SEP_NZ], double tol,
                                  int maxstep, int npat, double* pol, double* mult, double (&yo)[SEP_NZ], double& vo,
                                  double& rp_out, double& rd_out, int& steps) {
    const int gl = lane_bits_opaque<G - 1>();
    constexpr int SCBF = 2 * SEP_D * SB;  // first CBF side index (sep_stage_side)
    steps = 0;
    for (int pat = 0; pat < npat; pat++) {
        double g4[4] = {0.0, 0.0, 0.0, 0.0}, hl = 0.0;
#pragma unroll
        for (int c = 0; c < CB; c++) {
            if (c != lead) continue;
#pragma unroll
            for (int j = 0; j < 4; j++) g4[j] = rw.cg[c][j];
            hl = rw.chi[c];
        }
        SepRows<SB, CB> rp = rw;
#pragma unroll
        for (int c = 0; c < CB; c++) {
            if (lead < 0 || rw.ccv[c] == 0.0) continue;  // (inert slots stay inert)
            const double keep = c == lead ? 0.0 : 1.0;  // leader: -g_l; others: g_c - g_l
#pragma unroll
            for (int j = 0; j < 4; j++) rp.cg[c][j] = fma(keep, rw.cg[c][j], -g4[j]);
            rp.chi[c] = fma(keep, rw.chi[c], -hl);
        }
        double qa[4];
#pragma unroll
        for (int j = 0; j < 4; j++) qa[j] = lead >= 0 ? w * g4[j] : 0.0;
        grp_sum_vec<G, 4>(qa);
        double qp[SEP_NZ], yu[SEP_NZ], yg[SEP_NZ], rpg = 0.0, rdg = 0.0, tl = 0.0;
#pragma unroll
        for (int j = 0; j < SEP_NZ; j++) qp[j] = j < 4 ? q[j] + qa[j] : q[j];
#pragma unroll
        for (int d = 0; d < SEP_D; d++) {
            const int o = 2 * d;
            yu[o] = -fma(Pinv[3 * d], qp[o], Pinv[3 * d + 1] * qp[o + 1]);
            yu[o + 1] = -fma(Pinv[3 * d + 1], qp[o], Pinv[3 * d + 2] * qp[o + 1]);
        }
        int st = 0;
        const int r = sep_dual_as<G, SB, CB>(rp, true, P, Pinv, qp, yu, tol, maxstep, pol, yg, rpg, rdg, st, nullptr,
                                             true, tl, nullptr, 0, nullptr, nullptr, mult);
        steps += st;
        if (r == 0) return 0;
        if (r < 0) {
            // no feasible point with this pattern: the unreachable candidate's row leads its lane
            const int id = (int)pol[POL_K * 16 + POL_ID];
            const int s = id >> 4, ln = id & 15;
            if (s < SCBF || __shfl(lead, ln, G) >= 0) return 0;
            wave_lds_sync();
            if (gl == ln) lead = s - SCBF;
            continue;
        }
        // per lane: multipliers of its rows (lam) and of its leader's bound (mu)
        const int k = (int)mult[7];
        double lam = 0.0, mu = 0.0, best = -1.0;
        int pick = -1;
        for (int a = 0; a < k; a++) {
            const int id = (int)mult[8 + a];
            const int s = id >> 4;
            if ((id & 15) != gl || s < SCBF) continue;
            const int c = s - SCBF;
            const double ua = mult[a];
            if (c == lead) {
                mu += ua;
            } else {
                lam += ua;
                if (ua > best) best = ua, pick = c;
            }
        }
        const bool bad = lead < 0 ? !(lam <= w) : !(w - lam - mu >= 0.0);
        wave_lds_sync();  // (mult is rewritten by the next pattern)
        if (grp_ballot<G>(bad) == 0ull) {
#pragma unroll
            for (int j = 0; j < SEP_NZ; j++) yo[j] = yg[j];
            double t = -hl;
#pragma unroll
            for (int j = 0; j < 4; j++) t = fma(g4[j], yg[j], t);
            vo = lead >= 0 ? fmax(t, 0.0) : 0.0;
            rp_out = rpg;
            rd_out = rdg;
            return 1;
        }
        if (grp_ballot<G>(bad && pick < 0) != 0ull) return 0;
        if (bad) lead = pick;
    }
    return 0;
}

// state row `row` of the batch (re-read where needed instead of held in registers)
__device__ __forceinline__ void load_state_lds(const double* s0k, double (&s)[6]) {
    wave_lds_sync();  // (written by lanes 0..5 of the group)
#pragma unroll
    for (int i = 0; i < 6; i++) s[i] = s0k[i];
}

// Hand agent ai to the fallback launch (lane 0 appends it to args.defer: [count, -, agents...]).
__device__ __forceinline__ void defer_agent(const ImpcArgs& args, int ai, int gl) {
    if (gl == 0) {
        const int slot = atomicAdd(&args.defer[0], 1);
        args.defer[2 + slot] = ai;
    }
}

// One agent's IMPC step on the separable layout (the body of impc_sep_kernel). stage / red / nbs:
// this group's LDS (CBF-row staging, Newton-sum all-reduce, neighbour query).
// The (non-slack) fallback launch keeps a lane's rows (SepRows, e.g. 8 CBF slots: 60 doubles) in
// LDS instead of registers: its occupancy is one wave per SIMD either way, and in registers they
// spilled (1236 -> 424 B/lane for 8 slots, 44 -> 0 for 1). Padded to an odd number of doubles per
// lane (bank spread of the per-lane struct reads). The slack fallback too since round 4 (156 -> 0
// B/lane; round 3 had kept them in registers because in LDS one all-neighbour slack QP of the
// stress line flipped to UNKNOWN in the last bits — with the slack-pattern active set the 1000-step
// stress line stays at 0 UNKNOWN either way, `profiles/r04_slack_fallback_lds.log`).
template <int SB, int CB>
struct SepRowsLds {
    SepRows<SB, CB> r;
    double pad[(sizeof(SepRows<SB, CB>) / 8) % 2 == 0 ? 1 : 2];
};

// LDS of the separable pipeline per agent (doubles): CBF-row staging / the dual active set's
// scratch, and the kept solution | warm duals | state | warm-start side ids | linear term
template <int SB, int CB, bool SLACK>
constexpr int sep_stage_doubles() {
    return SLACK ? sep_pol_doubles<SB, CB>() + 16
                 : (CB * 16 * (SEP_NZ + 1) > sep_pol_doubles<SB, CB>() ? CB * 16 * (SEP_NZ + 1)
                                                                      : sep_pol_doubles<SB, CB>());
}
template <int SB, bool SLACK, bool LEAN>
constexpr int sep_keep_doubles() {
    return 16 * (SEP_NZ + (LEAN ? 0 : 2 * SEP_D * SB)) + 8 + (SLACK ? 0 : POL_K + 1) + 10 + 6;
}

// (lds: this group's 16 entries, one per lane)
template <bool LDS, int SB, int CB>
__device__ __forceinline__ SepRows<SB, CB>& pick_rows(SepRows<SB, CB>& reg, SepRowsLds<SB, CB>* lds) {
    if constexpr (LDS) return lds[threadIdx.x & 15u].r;
    else return reg;
}

// (force-inlined: instantiated by two kernels, an out-of-line call would copy the kernel arguments
// to the stack at every launch's start)
// STORE (a store is attached, mpccbf_set_active_store; never in slack mode): the agent's record
// starts iteration 0's solve and the returned curve's final active set is written back (astore:
// this group's LDS for the staged CBF rows' keys; active_store.hpp).
// CONN (connectivity attached, mpccbf_set_connectivity; impc_conn.hip alone instantiates it): the
// team's connectivity rows are staged behind the safety rows of every iteration (conn_rows.hpp);
// rows in LDS as the capacity launch keeps them.
// HANDOVER (with LEAN: the main launch that completes in-kernel, impc_sep_complete): a QP the lean
// pipeline does not settle makes the agent set *handed and return instead of deferring it — nothing
// but per-iteration outputs, the neighbour list and stamps has been written by then, all of which the
// full pipeline's run from scratch rewrites with the same values. (A flag, not a return value: the
// other instantiations' code stays what it was, tools/code_sizes.py.)
// FORM (LaunchForm, impc.hpp; the loop form only for the handing-over lean pipeline): what is known
// at compile time about the launch-uniform options. Only the tests change with it: every
// expression on a path the form keeps is the generic form's.
template <int SB, int CB, bool SLACK, bool QUEUE, bool LEAN = false, bool STORE = false, bool CONN = false,
          bool HANDOVER = false, int FORM = FORM_GENERIC>
__device__ __forceinline__ void impc_sep_agent(const DevOps& op, const double* __restrict__ buf, const ImpcArgs& args,
                               const int ai, const int gl, double* stage, double* red, NbScratch& nbs,
                               double* keep, SepRowsLds<SB, CB>* rows_lds = nullptr, double* bconst = nullptr,
                               int32_t* astore = nullptr, const StoreArgs store = StoreArgs{nullptr, 0},
                               const ConnArgs conn = ConnArgs{}, bool* handed = nullptr) {
    static_assert(!(STORE && SLACK), "the active-set store is not built for slack mode");
    static_assert(!CONN || (!SLACK && !STORE && !LEAN), "connectivity rows: the full non-slack pipeline");
    static_assert(!HANDOVER || (LEAN && !STORE), "only the lean pipeline hands an agent over");
    static_assert(FORM == FORM_GENERIC || (HANDOVER && !SLACK && !QUEUE), "the loop form: the main launch's lean agent");
    using LF = FormOf<FORM>;
    constexpr int G = 16;
    constexpr int NZ = SEP_NZ;
    constexpr int cap = CB * G;  // CBF rows per agent
    stamp(args, ai, gl, 0);

    const int self = args.agent_first + ai;
    // (the record's load goes first: it has arrived when the state, issued after it, has)
    int rec_in = 0;
    if constexpr (STORE)
        if (gl < AS_WORDS) rec_in = store.records[(size_t)self * AS_WORDS + gl];
    double s0[6];
#pragma unroll
    for (int i = 0; i < 6; i++) s0[i] = args.states[(size_t)self * 6 + i];
    // the next state's noise draws, while the state is in flight (the keep area's last 6 doubles)
    double* const noise0 = keep + sep_keep_doubles<SB, SLACK, LEAN>() - 6;
    early_noise<FORM>(args, ai, gl, noise0);
    // grid mode: the neighbour query's loads are staged between the setup's (gq_*)
    const bool grid_mode = LF::loop || args.nb_row_ptr == nullptr;
    GridQuery<G> gq;
    // (the state arrives before the branch: waited for only on one side, the join would wait for
    // every load in flight, the query's included)
    asm volatile("" ::"v"(s0[0]), "v"(s0[1]), "v"(s0[2]), "v"(s0[3]), "v"(s0[4]), "v"(s0[5]));
    if (grid_mode) gq_begin<G>(args, s0[0], s0[1], gq);
    // (LDS pointers by type, as lds_vol's other users: the accesses do not depend on inlining to be
    // LDS accesses)
    const lds_vptr<int32_t> tags = lds_vol(astore);
    // (the record waits in the Newton sums' area, which only the interior-point solver uses, after
    // iteration 0's start has been mapped: the main launch's LDS has no 32 bytes per group left)
    const lds_vptr<int32_t> rec = lds_vol((int32_t*)red);
    if constexpr (STORE)
        if (gl < AS_WORDS) rec[gl] = rec_in;
    // the linear term and constant, group-uniform: kept in LDS (qk, after the warm-start ids) and
    // read back inside each IMPC iteration, so they are not live in registers across the loop
    double* qk = keep + 16 * (SEP_NZ + (LEAN ? 0 : 2 * SEP_D * SB)) + 8 + (SLACK ? 0 : POL_K + 1);
    {
        double kc0;
        const double q0 = agent_linear_term_lanes<NZ, G, FORM>(op, buf, args, ai, s0, gl, kc0);
        if (gl < NZ) qk[gl] = q0;
        if (gl == 0) {
            qk[NZ] = kc0;
            *(int*)(qk + NZ + 1) = ai;
        }
    }
    // the agent index and the returned point's residuals, re-read from LDS where they are used
    // (held in registers across the solves they were the main launch's last spills)
    auto agent = [&]() -> int { return *lds_vol((int*)(qk + NZ + 1)); };
    lds_vptr<double> res = lds_vol(qk + NZ + 2);

    // ---- box rows: channel d, slot k -> row k * G + gl of that channel (packed by the host:
    // per row [g0, g1, Gs(6), lo, hi], two-sided; unused rows inert: g = 0, Gs = 0, [-1, 1])
    if (grid_mode) gq_slots<G>(args, gq, gl);
    SepRows<SB, CB> rw_reg;  // (the fallback launch: rows in LDS)
    // (rows in LDS: the fallback launch, and two box slots per lane, where in registers they spill)
    SepRows<SB, CB>& rw = pick_rows<QUEUE || CONN || (SB > 1)>(rw_reg, rows_lds);
    {
        const double* B = opp(buf, op.o_Gsep);
#pragma unroll
        for (int d = 0; d < SEP_D; d++)
#pragma unroll
            for (int k = 0; k < SB; k++) {
                const double* r = B + ((size_t)(d * SB + k) * G + gl) * SEP_ROW;
                double sh = 0.0;
#pragma unroll
                for (int s = 0; s < 6; s++) sh = fma(r[2 + s], s0[s], sh);
                rw.bg[d][k][0] = r[0];
                rw.bg[d][k][1] = r[1];
                rw.blo[d][k] = r[8] - sh;
                rw.bhi[d][k] = r[9] - sh;
            }
    }
    if (grid_mode) gq_states<G>(args, gq, gl);
    const bool infeasible = constant_rows_infeasible<G>(op, buf, s0, gl);
    // the box rows' violation scales and candidate weights, formed once for both IMPC iterations'
    // active-set solves (bconst: [2 SEP_D SB sides][16] doubles, then [SEP_D SB rows][16] floats)
    double* bsc = nullptr;
    float* bw = nullptr;
    if (!SLACK && bconst != nullptr) {
        bsc = bconst;
        bw = (float*)(bconst + 16 * 2 * SEP_D * SB);
        sep_box_consts<SB, CB>(rw, opp(buf, op.o_Pinv), bsc, bw);
    }
    stamp(args, ai, gl, 1);

    int nb0 = 0, nnb = 0;
    if (!grid_mode) {
        nb0 = args.nb_row_ptr[ai];
        nnb = args.nb_row_ptr[ai + 1] - nb0;
    } else {
        nnb = grid_neighbors_finish<G, FORM>(args, self, s0[0], s0[1], nbs, gl, 0.0, gq);
    }
    write_nb_out<FORM>(args, ai, gl, grid_mode, nbs, nb0, nnb);
    if (SLACK && !QUEUE && nnb > G && args.defer) {  // slack mode: beyond one lane per neighbour
        defer_agent(args, agent(), gl);
        return;
    }
    const bool nb_overflow = nnb < 0 || (SLACK && !QUEUE && nnb > G);
    if (nb_overflow) nnb = 0;
    double wslack = 0.0, vslack = 0.0;
    // slack mode: one lane per neighbour; with more than G neighbours (the fallback launch), per
    // IMPC iteration the ones with a live row (a slack without rows is 0 at the optimum)
    if constexpr (SLACK)
        if (nnb <= G) wslack = lane_slack_weight<G>(op, args, s0, grid_mode, nbs.idx, nb0, nnb, gl < nnb ? gl : -1);
    stamp(args, ai, gl, 2);

    // the kept solution and the warm-start duals live in per-lane LDS slots (keep: [ykeep 6 x 16 |
    // warm 2 x 3 x SB x 16]), not registers: they are touched once per IMPC iteration
    double y[NZ];
    double* ykeep = keep + gl;  // ykeep[16 * i]
#pragma unroll
    for (int i = 0; i < NZ; i++) y[i] = ykeep[16 * i] = 0.0;
    // the agent's state, kept for the CBF rows and the outputs (group-uniform: LDS broadcast reads
    // instead of further global round trips)
    double* s0k = keep + 16 * (SEP_NZ + (LEAN ? 0 : 2 * SEP_D * SB));
    {
        double v = s0[0];
#pragma unroll
        for (int i = 1; i < 6; i++) v = gl == i ? s0[i] : v;
        if (gl < 6) s0k[gl] = v;
    }
    bool have_curve = false, success = true;
    const PdipCfg cfg{op.maxit, op.tol};
    SepWarm<SB> warm{keep + 16 * NZ};  // box duals of the previous OPTIMAL solve (iteration 1 warm start)
    const double warm_delta = SLACK ? 0.0 : op.warm_delta;
    // the dual active set's warm start: iteration 0's final active set (side ids, their count at
    // act[POL_K]) starts iteration 1's solve (same box rows and cost, sample-0 CBF rows) when
    // iteration 0 took at least op.das_warm steps. Measured on the bench swarm: after a long
    // iteration-0 solve (a transient: several sides) iteration 1 then takes 0 steps where a cold
    // start repeats them; after a 1-2 step solve (steady state: one CBF side, which iteration 1's
    // sample-1 row usually replaces) the warm set costs a step more than the cold start.
    double* act = s0k + 8;  // (no such area in slack mode: never touched there)
    if (!SLACK && gl == 0) act[POL_K] = 0.0;
    int steps0 = 0;  // iteration 0's solver steps
    // STORE: the sides this iteration's solve was offered (iteration 0: the record's, mapped onto
    // the staged rows), the staged row count, and this lane's word of the record to write
    int k0_off = 0, cbf_count = 0, rec_out = 0;
    auto warm_count = [&](int it) -> int {
        if constexpr (STORE) {
            // iteration 1 carries iteration 0's set when that took das_warm steps, or when it was
            // itself warm-started (then few steps say nothing) and ended with several sides.
            // act[POL_K] < 0 afterwards: no solve of this iteration has saved a set
            wave_lds_sync();
            int k0 = 0;
            if (it == 0) {
                k0 = as_map_sep<CB>(rec, tags, cbf_count, op.sep_rows_per_dim, store.min_steps, gl, act);
            } else if (op.das_warm > 0) {
                const int kf = (int)act[POL_K];
                if (kf > 0 && (steps0 >= op.das_warm || (k0_off > 0 && kf >= 2))) k0 = kf;
            }
            wave_lds_sync();
            if (gl == 0) act[POL_K] = -1.0;
            k0_off = k0;
            return k0;
        } else {
            if (SLACK || it == 0 || op.das_warm <= 0 || steps0 < op.das_warm) return 0;
            wave_lds_sync();
            return (int)act[POL_K];
        }
    };

    for (int it = 0; it < op.impc_iter; it++) {
        const size_t oi = (size_t)agent() * op.impc_iter + it;
        if (!success) {
            write_iteration<FORM>(args, oi, gl, ST_UNKNOWN, __builtin_nan(""), 0);
            continue;
        }
        bool row_infeasible = false;
        int count = 0;
        bool live = false;
        bool slack_overflow = false;
        wave_lds_sync();
        asm volatile("" ::: "memory");  // (the reads below stay inside the iteration)
        double q[NZ];
#pragma unroll
        for (int j = 0; j < NZ; j++) q[j] = qk[j];
        if constexpr (SLACK) {
            // slack mode: rows stay in their neighbour's lane; a slack row is never infeasible
            double sx[6];  // the state again (not kept in registers across the solves)
            load_state_lds(s0k, sx);
            int jn = gl < nnb ? gl : -1;
            if (QUEUE && nnb > G) {
                const int nlive = slack_compact<G>(op, buf, args, it, s0k, ykeep, grid_mode, nbs.idx, nb0, nnb,
                                                   gl, jn, wslack);
                slack_overflow = nlive > G;
            }
            live = grp_ballot<G>(lane_cbf_rows<SB, CB>(op, buf, args, it, sx, y, grid_mode, nbs.idx, nb0, jn, rw)) != 0ull;
        } else {
            double sx[6];  // the state again (not kept in registers across the solves)
            load_state_lds(s0k, sx);
            // (the staging area's tail beyond the cap rows holds the samples' terms when it has
            // room: the dual active set's scratch is larger than 16 rows)
            constexpr int STG = CB * 16 * (SEP_NZ + 1) > sep_pol_doubles<SB, CB>() ? CB * 16 * (SEP_NZ + 1)
                                                                                   : sep_pol_doubles<SB, CB>();
            if (STG - cap * (NZ + 1) >= 27 && it > 0)
                count = stage_cbf_rows_pairs<NZ, STORE, FORM>(op, buf, args, it, sx, y, grid_mode, &nbs, nb0, nnb, stage, cap,
                                                        gl, &row_infeasible, stage + cap * (NZ + 1), astore);
            else
                count = stage_cbf_rows<NZ, G, STORE, FORM>(op, buf, args, it, sx, y, grid_mode, &nbs,
                                                     nb0, nnb, stage, cap, gl, &row_infeasible, astore);
            if constexpr (CONN)
                count = stage_conn_rows<NZ>(op, buf, args, conn, args.agent_first + agent(), it, sx, y,
                                            stage, cap, count, gl, &row_infeasible);
            live = count > 0;
            if constexpr (STORE) cbf_count = count;
#pragma unroll
            for (int c = 0; c < CB; c++) {
                const int ci = c * G + gl;
                const bool on = ci < count && ci < cap;
                const double* src = stage + (size_t)(on ? ci : 0) * (NZ + 1);
#pragma unroll
                for (int j = 0; j < 4; j++) rw.cg[c][j] = on ? src[j] : 0.0;  // yaw columns are 0
                rw.chi[c] = on ? src[NZ] : 1.0;  // unused slot: inert row 0 <= 1
                rw.ccv[c] = 0.0;
            }
        }
        if (it < 2) stamp(args, ai, gl, 3 + 2 * it);
        if (count > cap && args.defer) {  // beyond this instantiation: the fallback launch solves it
            defer_agent(args, agent(), gl);
            return;
        }
#ifdef MPCCBF_PDIP_STAMPS  // (profiling build: the solve phase's parts around the solver, slots 16 ..)
        long long* const dbgs = (args.stamps && it == 0)
                                    ? (long long*)args.stamps + (size_t)args.num_agents * NSTAMP + (size_t)ai * 32
                                    : nullptr;
#define SSTAMP(k)                                                                \
    do {                                                                         \
        if (dbgs) dbgs[k] = (long long)__builtin_amdgcn_s_memtime();             \
    } while (0)
#else
#define SSTAMP(k) \
    do {          \
    } while (0)
#endif
        SSTAMP(16);
        int st;
        int nit = 0;
        if (gl == 0) res[0] = res[1] = __builtin_nan("");
        // non-finite data (a NaN / Inf state, target or neighbour state): such a model is not
        // solved (CPLEX rejects non-finite coefficients); reported as ERROR
        bool nfin = false;
#pragma unroll
        for (int j = 0; j < NZ; j++) nfin = nfin || !isfinite(q[j]);
#pragma unroll
        for (int d = 0; d < SEP_D; d++)
#pragma unroll
            for (int k = 0; k < SB; k++) nfin = nfin || !isfinite(rw.blo[d][k]) || !isfinite(rw.bhi[d][k]);
#pragma unroll
        for (int c = 0; c < CB; c++)
            nfin = nfin || !isfinite(rw.chi[c]) || !isfinite(rw.cg[c][0]) || !isfinite(rw.cg[c][1]) ||
                   !isfinite(rw.cg[c][2]) || !isfinite(rw.cg[c][3]);
        const bool nonfinite = grp_ballot<G>(nfin) != 0ull;
        SSTAMP(17);
        if (count > cap || nb_overflow || slack_overflow || nonfinite) {
            st = ST_ERROR;
        } else if (infeasible || row_infeasible) {
            st = ST_INFEASIBLE;
        } else if constexpr (LEAN) {
            // lean main launch: the fast start and the dual active set only. A QP that needs more
            // (the active set gives up, or no feasible point without a certificate well above the
            // tolerance: phase 1) defers the whole agent to the fallback launch (HANDOVER: returns
            // it to the wrapper for the in-kernel completion), which runs the
            // full pipeline (PDIP attempts, phase 1) on the same inputs — so the main kernel's
            // registers are those of the active-set path, not the interior-point solver's.
            const double* Pi = opp(buf, op.o_Pinv);
            double yu[NZ];
#pragma unroll
            for (int d = 0; d < SEP_D; d++) {
                const int o = 2 * d;
                yu[o] = -fma(Pi[3 * d], q[o], Pi[3 * d + 1] * q[o + 1]);
                yu[o + 1] = -fma(Pi[3 * d + 1], q[o], Pi[3 * d + 2] * q[o + 1]);
            }
            double tl = 0.0, prs = __builtin_nan(""), drs = __builtin_nan("");
            const int k0 = warm_count(it);
            const int r = sep_dual_as<G, SB, CB>(rw, live, opp(buf, op.o_Pr), Pi, q, yu, op.tol, op.dual_as, stage, y,
                                                 prs, drs, nit, nullptr, HANDOVER ? !LF::loop && args.dual_res != nullptr : true, tl,
                                                 nullptr, k0, act,
                                                 (STORE || it == 0) ? act : nullptr, nullptr, bsc, bw);
            if (r > 0) {
                st = ST_OPTIMAL;
            } else if (r < 0 && tl > 10.0 * op.feas_tol) {
                st = ST_INFEASIBLE;
                prs = tl;
                drs = __builtin_nan("");
            } else if constexpr (HANDOVER) {
                *handed = true;
                return;
            } else {
                defer_agent(args, agent(), gl);
                return;
            }
            if (gl == 0) res[0] = prs, res[1] = drs;
        } else {
#ifdef MPCCBF_PDIP_STAMPS
            long long* dbg = (args.stamps && it == 0)
                                 ? (long long*)args.stamps + (size_t)args.num_agents * NSTAMP + (size_t)agent() * 32
                                 : nullptr;
#elif defined(MPCCBF_SOLVE_TRACE)  // per-step (rp, mu, alpha, rd) of the first solve + phase 1
            long long* dbg = args.stamps ? (long long*)args.stamps + (size_t)args.num_agents * NSTAMP +
                                               ((size_t)agent() * 2 + it) * 256
                                         : nullptr;
#else
            long long* dbg = nullptr;
#endif
            // Attempts (group-uniform; one call site): 0 = warm start (IMPC iteration 1) or cold,
            // with the divergence test; 1 = cold to the iteration limit; 2 = cold with the shifted
            // Newton matrix. Before any retry, phase 1 certifies feasibility (minimal uniform row
            // violation above the tolerance, from the failed solve's last iterate), so an
            // infeasible QP needs no retry and statuses never depend on the first attempt's
            // warm start or divergence test.
            // (with the dual active-set solve first, the PDIP runs cold: no warm-start duals kept)
            const bool warm_try = it > 0 && warm_delta > 0.0 && op.dual_as <= 0;
            int tr_warm = 0, tr_cold = 0, tr_p1 = 0;  // per kind (MPCCBF_SOLVE_TRACE); phase-1 steps
            int attempt = 0, total = 0;
            bool certified = false, infeas = false;
            double tstar = 0.0;
            PdipOut po{ST_UNKNOWN, 0};
            // slack mode: the slack-pattern active set first (every slack at zero, then leader
            // rows); the PDIP below only when it finds no consistent pattern
            bool pattern_done = false;
            double* pat_mult = SLACK ? stage + sep_pol_doubles<SB, CB>() : nullptr;
            if constexpr (SLACK) {
                if (op.dual_as > 0 && live) {
                    int lead = -1, pst = 0;
                    double yg[NZ], vg = 0.0, rpg = 0.0, rdg = 0.0;
                    if (sep_slack_patterns<G, SB, CB>(rw, wslack, lead, opp(buf, op.o_Pr), opp(buf, op.o_Pinv), q,
                                                      op.tol, 2 * op.dual_as, 8, stage, pat_mult, yg, vg, rpg, rdg,
                                                      pst)) {
#pragma unroll
                        for (int j = 0; j < NZ; j++) y[j] = yg[j];
                        vslack = vg;
                        po = PdipOut{ST_OPTIMAL, 0};
                        po.rp = rpg;
                        po.rd = rdg;
                        pattern_done = true;
                    }
                    total += pst;
                }
            }
            for (; !pattern_done;) {
                PdipCfg ca = cfg;
                ca.early_it = attempt == 0 ? op.early_it : 0;
                ca.fast_start = op.fast_start != 0;
                ca.robust = attempt == 2;
                ca.dual_as = attempt == 0 ? op.dual_as : 0;
                ca.want_rd = args.dual_res != nullptr;
                const int k0 = attempt == 0 ? warm_count(it) : 0;
                po = pdip_solve_sep<G, SB, CB, SLACK>(rw, live, opp(buf, op.o_Pr), opp(buf, op.o_Pinv), q, y,
                                                      ca, dbg, wslack, &vslack, red, &warm,
                                                      (attempt == 0 && warm_try) ? warm_delta : 0.0,
                                                      SLACK ? nullptr : stage, k0, SLACK ? nullptr : act,
                                                      (!SLACK && attempt == 0 && (STORE || it == 0)) ? act : nullptr,
                                                      bsc, bw);
                total += po.iters;
                ((attempt == 0 && warm_try) ? tr_warm : tr_cold) += po.iters;
                if (po.status == ST_OPTIMAL) break;
                if (!certified && po.tlow > 10.0 * op.feas_tol) {
                    // the dual active set's infeasibility certificate bounds t* from below: no
                    // phase 1 needed (a bound within 10x of the tolerance still goes to phase 1)
                    tstar = po.tlow;
                    infeas = true;
                    certified = true;
                }
                if (!certified) {
                    SepRows<SB, CB> rp1 = rw;
                    if constexpr (SLACK) {  // slack rows are always satisfiable: certify the box rows
#pragma unroll
                        for (int c = 0; c < CB; c++) {
#pragma unroll
                            for (int j = 0; j < 4; j++) rp1.cg[c][j] = 0.0;
                            rp1.chi[c] = 1.0;
                        }
                    }
                    tstar = pdip_phase1_sep<G, SB, CB>(rp1, cfg, op.feas_tol, y, red, &tr_p1, dbg);
                    infeas = tstar > op.feas_tol && tstar < 1e300;  // 1e300: phase 1 failed
                    certified = true;
#ifdef MPCCBF_DEBUG_EXIT
                    total += tstar >= 1e300 ? 10000 : 0;
#endif
                }
                if (infeas) {
                    po.status = ST_INFEASIBLE;
                    break;
                }
                if (attempt == 0 && (warm_try || po.early)) attempt = 1;
                else if (attempt < 2) attempt = 2;
                else break;
            }
            if constexpr (SLACK) {
                // the slack PDIP's point fixes a pattern — a lane with v > 0 leads with its row of
                // largest excess g y - h — and one active-set solve of it (plus one exchange)
                // returns the exact optimum, which replaces the interior point's when consistent
                // (also a PDIP that stalled short of its tolerance: round 3's UNKNOWN all-neighbour
                // slack QPs)
                if (!pattern_done && !infeas && op.dual_as > 0 && live) {
                    int lead = -1;
                    double best = -1e300;
#pragma unroll
                    for (int c = 0; c < CB; c++) {
                        double t = -rw.chi[c];
#pragma unroll
                        for (int j = 0; j < 4; j++) t = fma(rw.cg[c][j], y[j], t);
                        if (rw.ccv[c] != 0.0 && t > best) best = t, lead = c;
                    }
                    if (!(vslack > 1e-9)) lead = -1;
                    int pst = 0;
                    double yg[NZ], vg = 0.0, rpg = 0.0, rdg = 0.0;
                    if (sep_slack_patterns<G, SB, CB>(rw, wslack, lead, opp(buf, op.o_Pr), opp(buf, op.o_Pinv), q,
                                                      op.tol, 2 * op.dual_as, 2, stage, pat_mult, yg, vg, rpg, rdg,
                                                      pst)) {
#pragma unroll
                        for (int j = 0; j < NZ; j++) y[j] = yg[j];
                        vslack = vg;
                        po.status = ST_OPTIMAL;
                        po.rp = rpg;
                        po.rd = rdg;
                    }
                    total += pst;
                }
            }
            st = po.status;
            // active-set and PDIP steps. Phase 1's steps are not counted (include/mpccbf.h): it
            // starts from the failed solve's last iterate and stops as soon as its decision is
            // settled, so its count depends on that iterate's last bits — the in-kernel completion
            // and the fallback launch, two code objects of this source, took 7 and 9 steps to the
            // same t* (test_gpu_feasibility.py, test_lean_step_counts).
            nit = total;
            if (gl == 0) res[0] = st == ST_INFEASIBLE ? tstar : po.rp, res[1] = po.rd;
#ifdef MPCCBF_SOLVE_TRACE  // diagnostics build: warm + 100 cold + 10000 phase-1 iterations
            nit = tr_warm + 100 * tr_cold + 10000 * tr_p1;
#else
            (void)tr_warm, (void)tr_cold;
#endif
        }
        SSTAMP(18);
        double objv = __builtin_nan("");
        if (st == ST_OPTIMAL) {
            objv = sep_objective(opp(buf, op.o_Pr), q, y, qk[NZ]);
            if constexpr (SLACK) objv += grp_sum<G>(live ? wslack * vslack : 0.0);  // + w^T v
            SSTAMP(19);
#pragma unroll
            for (int i = 0; i < NZ; i++) ykeep[16 * i] = y[i];
            have_curve = true;
            // the record of the curve kept so far: this solve's final set (steps: its own plus one
            // per side a warm start offered, so that a set that converged at once stays eligible)
            if constexpr (STORE) {
                wave_lds_sync();
                rec_out = as_word_sep(act, tags, nit + k0_off, it, gl);
            }
        } else {
            success = false;
        }
        SSTAMP(20);
        write_iteration<FORM>(args, oi, gl, st, objv, nit, res[0], res[1]);
        SSTAMP(21);
        if (it == 0) steps0 = nit;
        if (it < 2) stamp(args, ai, gl, 4 + 2 * it);
        wave_lds_sync();
#undef SSTAMP
    }
    double yk[NZ], sx[6];
#pragma unroll
    for (int i = 0; i < NZ; i++) yk[i] = ykeep[16 * i];
    load_state_lds(s0k, sx);
    write_agent_outputs<NZ, G, true, true, FORM>(op, buf, args, agent(), gl, sx, yk, have_curve, noise0);
    if constexpr (STORE)
        if (gl < AS_WORDS) store.records[(size_t)(args.agent_first + agent()) * AS_WORDS + gl] = rec_out;
    stamp(args, ai, gl, 7);
}

// The kernel-argument segment of impc_sep_kernel as a struct: each argument at its natural alignment
// in declaration order (the hidden arguments follow the last one).
struct SepKernargs {
    DevOps op;
    const double* buf;
    ImpcArgs args;
};
static_assert(offsetof(SepKernargs, buf) == ((sizeof(DevOps) + 7) & ~size_t(7)) &&
                  offsetof(SepKernargs, args) == offsetof(SepKernargs, buf) + 8 && alignof(ImpcArgs) <= 8 &&
                  alignof(DevOps) <= 8,
              "SepKernargs mirrors the kernel-argument layout");

template <class T>
using lds_ptr = __attribute__((address_space(3))) T*;

// In-kernel completion of the 16-lane main launch: the full pipeline (PDIP attempts, phase 1) from
// scratch for an agent the lean pipeline handed over (impc_sep_agent's HANDOVER), on the group's own
// LDS slices. Out of line, so that the main kernel's hot path is the lean pipeline's code and
// registers; it takes nothing from the caller but the agent index, the slices as LDS-typed pointers
// and the address of the kernel-argument segment (ka_lo, ka_hi: as a value, made wave-uniform again
// here — the segment-pointer intrinsic itself is null outside a kernel): the operators and the launch
// arguments are re-read from the segment with scalar loads (as arguments by reference they were copied
// to the stack at every launch's start). Internal linkage and never a tail call: the caller then
// knows which registers the callee leaves alone and the callee saves none (inter-procedural register
// allocation), which keeps its frame at its own spills (40 B/lane; 1,368 with the saves).
template <int SB, int CB>
static __device__ __attribute__((noinline, not_tail_called)) void impc_sep_complete(
    const int ai, const unsigned ka_lo, const unsigned ka_hi, lds_ptr<double> stage, lds_ptr<double> red,
    lds_ptr<NbScratch> nbs, lds_ptr<double> keep, lds_ptr<double> bconst) {
    const unsigned long long kp = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)ka_hi) << 32) |
                                  (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)ka_lo);
    const SepKernargs* ka = (const SepKernargs*)(const __attribute__((address_space(4))) SepKernargs*)kp;
    impc_sep_agent<SB, CB, false, false>(ka->op, ka->buf, ka->args, ai, (int)(threadIdx.x & 15u), (double*)stage,
                                         (double*)red, *(NbScratch*)nbs, (double*)keep, nullptr, (double*)bconst);
}

// QUEUE = false: one agent per 16-lane group. QUEUE = true (fallback launch): the agents the main
// launch deferred (args.queue: [count, blocks done, agents...]), one per group (the grid covers
// every agent of the batch); the last block to finish empties the queue for the next step.
// The plain main launch (no slack, not LEAN) runs the lean pipeline — fast start and dual active set
// — inline and finishes the agents it does not settle with a call of impc_sep_complete once the
// wave's four groups have come back: one launch, the hot path without the interior-point solver's
// code. LEAN is the two-launch form of the same split (the unsettled agents go to the queue).
// FORM (LaunchForm): the launch form of the plain main launch's lean agent; the completion it calls
// is the generic one in either form (one function, the same call).
template <int SB, int CB, bool SLACK, int BS, bool QUEUE = false, bool LEAN = false, int FORM = FORM_GENERIC>
__global__ void __launch_bounds__(BS) impc_sep_kernel(const DevOps op, const double* __restrict__ buf,
                                                       const ImpcArgs args) {
    static_assert(FORM == FORM_GENERIC || (!SLACK && !QUEUE && !LEAN), "the loop form: the plain main launch");
    constexpr int GPB = BS / 16;
    // CBF-row staging, reused as the dual active set's scratch (sep_pol_doubles)
    // (slack mode: the slack-pattern active set's scratch + its multipliers, sep_slack_patterns)
    __shared__ double stage_all[GPB][sep_stage_doubles<SB, CB, SLACK>()];
    __shared__ double red_all[GPB][LEAN ? 1 : 16 * (A_N + 1)];  // LDS all-reduce of the Newton sums
    __shared__ NbScratch nb_scratch[GPB];
    // kept solution | warm-start duals (not in the lean launch) | the agent's state | the dual active
    // set's warm-start side ids and their count (not in slack mode) | linear term and constant, the
    // agent index, the residuals
    __shared__ double keep_all[GPB][sep_keep_doubles<SB, SLACK, LEAN>()];
    constexpr bool rows_lds_per_lane = QUEUE || SB > 1;
    __shared__ SepRowsLds<SB, CB> rows_lds[rows_lds_per_lane ? BS : 1];
    // the box rows' constants per agent (sep_box_consts; not in slack mode)
    __shared__ double bconst_all[SLACK ? 1 : GPB][SLACK ? 1 : 16 * 2 * SEP_D * SB + 8 * SEP_D * SB];
    const int gl = threadIdx.x & 15;
    const int gib = threadIdx.x / 16;
    lds_poison();
    if constexpr (!QUEUE) {
        kclock_start(args);
        grid_clear<BS>(args);
        const int ai = xcd_block((int)blockIdx.x, (int)gridDim.x) * GPB + gib;
        if (ai >= args.num_agents) return;
        if constexpr (!SLACK && !LEAN) {
            static_assert(!rows_lds_per_lane, "the completion keeps its rows in registers");
            // (the lean agent uses a prefix of the full pipeline's keep area; without the dual active
            // set — the PDIP-only diagnostic setting — every agent takes the completion)
            bool left = op.dual_as <= 0;
            if (!left)
                impc_sep_agent<SB, CB, false, false, true, false, false, true, FORM>(
                    op, buf, args, ai, gl, stage_all[gib], red_all[gib], nb_scratch[gib], keep_all[gib], nullptr,
                    bconst_all[gib], nullptr, StoreArgs{nullptr, 0}, ConnArgs{}, &left);
            const unsigned long long kp = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
            if (left)
                impc_sep_complete<SB, CB>(ai, (unsigned)kp, (unsigned)(kp >> 32), (lds_ptr<double>)stage_all[gib],
                                          (lds_ptr<double>)red_all[gib],
                                          (lds_ptr<NbScratch>)&nb_scratch[gib], (lds_ptr<double>)keep_all[gib],
                                          (lds_ptr<double>)bconst_all[gib]);
        } else {
            impc_sep_agent<SB, CB, SLACK, false, LEAN>(op, buf, args, ai, gl, stage_all[gib], red_all[gib],
                                                       nb_scratch[gib], keep_all[gib],
                                                       rows_lds + (rows_lds_per_lane ? gib * 16 : 0),
                                                       SLACK ? nullptr : bconst_all[SLACK ? 0 : gib]);
        }
        kclock_end<BS>(args);
    } else {
        // one queue entry per group (no grid-stride loop: carried across iterations the agent's
        // state spills, 0 -> 372 B/lane, and a 16-block grid saved 0.2 us of the empty launch,
        // r06d); groups beyond the queue's length leave at once. The queue's header is zeroed by
        // the main launch after next (the queues alternate by step parity), so no block has to
        // find out that it is the last one
        const int k = blockIdx.x * GPB + gib;
        if (k < args.queue[0])
            impc_sep_agent<SB, CB, SLACK, true>(op, buf, args, args.queue[2 + k], gl, stage_all[gib], red_all[gib],
                                                nb_scratch[gib], keep_all[gib],
                                                rows_lds + (rows_lds_per_lane ? gib * 16 : 0),
                                                SLACK ? nullptr : bconst_all[SLACK ? 0 : gib]);
    }
}

// impc_sep_kernel (no slack mode, full pipeline) with the active-set store attached: a kernel of
// its own with the store as a further argument, so that the kernels launched without a store are
// the code they were — neither their body nor their argument layout knows of the store.
template <int CB, int BS, bool QUEUE>
__global__ void __launch_bounds__(BS) impc_sep_store_kernel(const DevOps op, const double* __restrict__ buf,
                                                             const ImpcArgs args, const StoreArgs store) {
    constexpr int SB = 1, GPB = BS / 16;
    __shared__ double stage_all[GPB][sep_stage_doubles<SB, CB, false>()];
    __shared__ double red_all[GPB][16 * (A_N + 1)];  // (also where the agent's record waits)
    __shared__ NbScratch nb_scratch[GPB];
    __shared__ double keep_all[GPB][sep_keep_doubles<SB, false, false>()];
    __shared__ SepRowsLds<SB, CB> rows_lds[QUEUE ? BS : 1];
    __shared__ double bconst_all[GPB][16 * 2 * SEP_D * SB + 8 * SEP_D * SB];
    __shared__ int32_t tags_all[GPB][CB * 16];  // the staged CBF rows' keys
    const int gl = threadIdx.x & 15;
    const int gib = threadIdx.x / 16;
    lds_poison();
    if constexpr (!QUEUE) {
        kclock_start(args);
        grid_clear<BS>(args);
        const int ai = xcd_block((int)blockIdx.x, (int)gridDim.x) * GPB + gib;
        if (ai >= args.num_agents) return;
        impc_sep_agent<SB, CB, false, false, false, true>(op, buf, args, ai, gl, stage_all[gib], red_all[gib],
                                                          nb_scratch[gib], keep_all[gib], rows_lds, bconst_all[gib],
                                                          tags_all[gib], store);
        kclock_end<BS>(args);
    } else {
        const int k = blockIdx.x * GPB + gib;
        if (k < args.queue[0])
            impc_sep_agent<SB, CB, false, true, false, true>(op, buf, args, args.queue[2 + k], gl, stage_all[gib],
                                                             red_all[gib], nb_scratch[gib], keep_all[gib],
                                                             rows_lds + gib * 16, bconst_all[gib], tags_all[gib], store);
    }
}

// impc_sep_kernel (no slack mode, full pipeline) with connectivity attached: a kernel of its own
// with the connectivity tables as a further argument (as impc_sep_store_kernel). One agent per
// 16-lane group, CB CBF row slots per lane with the rows in LDS; an agent beyond CB * 16 staged
// rows reports ERROR (no capacity launch behind it).
template <int CB, int BS>
__global__ void __launch_bounds__(BS) impc_sep_conn_kernel(const DevOps op, const double* __restrict__ buf,
                                                            const ImpcArgs args, const ConnArgs conn) {
    constexpr int SB = 1, GPB = BS / 16;
    __shared__ double stage_all[GPB][sep_stage_doubles<SB, CB, false>()];
    __shared__ double red_all[GPB][16 * (A_N + 1)];
    __shared__ NbScratch nb_scratch[GPB];
    __shared__ double keep_all[GPB][sep_keep_doubles<SB, false, false>()];
    __shared__ SepRowsLds<SB, CB> rows_lds[BS];
    __shared__ double bconst_all[GPB][16 * 2 * SEP_D * SB + 8 * SEP_D * SB];
    const int gl = threadIdx.x & 15;
    const int gib = threadIdx.x / 16;
    lds_poison();
    kclock_start(args);
    grid_clear<BS>(args);
    const int ai = xcd_block((int)blockIdx.x, (int)gridDim.x) * GPB + gib;
    if (ai >= args.num_agents) return;
    impc_sep_agent<SB, CB, false, false, false, false, true>(op, buf, args, ai, gl, stage_all[gib], red_all[gib],
                                                             nb_scratch[gib], keep_all[gib], rows_lds + gib * 16,
                                                             bconst_all[gib], nullptr, StoreArgs{nullptr, 0}, conn);
    kclock_end<BS>(args);
}

}  // namespace dev
}  // namespace mpccbf
