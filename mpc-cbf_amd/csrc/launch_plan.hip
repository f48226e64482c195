// launch_plan.hip — the host side of an IMPC step that needs no device: the launch plan
// (launch_plan.hpp), the operator packing (pack_operators.hpp) and the host-only export that shows
// both to the CPU tests (mpccbf_host_launch_plan). No HIP runtime call in this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>

#include "host/errors.hpp"
#include "host/pack_operators.hpp"
#include "kernels/fov_cbf.hpp"
#include "kernels/launch_plan.hpp"

namespace mpccbf {

namespace {

struct KernelShape {
    const char* name;
    int block_size, agents_per_block;
    bool clock;  // the kernel calls kclock_end
};

// indexed by ImpcKernel
const KernelShape SHAPES[] = {
    {"", 64, 1, false},
    {"impc_kernel<6,16,4>", 256, 16, false},
    {"impc_kernel<6,64,1>", 256, 4, false},
    {"impc_kernel<6,64,4>", 256, 4, false},
    {"impc_sep_kernel<1,1,false,256>", 256, 16, true},
    {"impc_sep_kernel<1,1,false,256,false,true>", 256, 16, true},
    {"impc_sep_kernel<1,2,true,256>", 256, 16, true},
    {"impc_sep_kernel<2,2,true,128>", 128, 8, true},
    {"impc_wide_kernel<256>", 256, 4, true},
    {"impc_sep_kernel<1,1,false,64,true>", 64, 4, false},
    {"impc_sep_kernel<1,8,false,64,true>", 64, 4, false},
    {"impc_sep_kernel<1,2,true,64,true>", 64, 4, false},
    {"impc_sep_kernel<2,2,true,64,true>", 64, 4, false},
    {"impc_sep_store_kernel<1,256,false>", 256, 16, true},
    {"impc_wide_store_kernel<256>", 256, 4, true},
    {"impc_sep_store_kernel<1,64,true>", 64, 4, false},
    {"impc_sep_store_kernel<8,64,true>", 64, 4, false},
    {"impc_sep_conn_kernel<4,64>", 64, 4, true},
    {"impc_fov_kernel<false>", 64, 1, false},
    {"impc_fov_kernel<true>", 64, 1, false},
    {"impc_sep_kernel<1,1,false,256>", 256, 16, true},  // (the loop form: IMPC_SEP's name)
    {"impc_fov_kernel<false,true>", 64, 1, false},
    {"impc_fov_kernel<true,true>", 64, 1, false},
};
static_assert(sizeof(SHAPES) / sizeof(SHAPES[0]) == IMPC_FOV_SLACK_EST + 1, "one shape per ImpcKernel");

constexpr int VARIANT_SEP16 = 4, VARIANT_WIDE = 5;

}  // namespace

const char* launch_form_name(LaunchForm f) { return f == FORM_LOOP ? "loop" : "generic"; }

// The facts a caller gives as a bit set of MPCCBF_FACT_* (mpccbf_host_launch_form)
static LaunchFacts launch_facts_of_bits(uint32_t bits) {
    auto on = [&](int bit) { return ((bits >> bit) & 1u) != 0; };
    LaunchFacts f{};
    f.targets = on(MPCCBF_FACT_TARGETS);
    f.traj_t = on(MPCCBF_FACT_TRAJ_T);
    f.substeps = on(MPCCBF_FACT_SUBSTEPS);
    f.cov = on(MPCCBF_FACT_COV);
    f.nb_out = on(MPCCBF_FACT_NB_OUT);
    f.primal_res = on(MPCCBF_FACT_PRIMAL_RES);
    f.dual_res = on(MPCCBF_FACT_DUAL_RES);
    f.cone = on(MPCCBF_FACT_CONE);
    f.x = on(MPCCBF_FACT_X);
    f.status = on(MPCCBF_FACT_STATUS);
    f.obj = on(MPCCBF_FACT_OBJ);
    f.iters = on(MPCCBF_FACT_ITERS);
    f.next_states = on(MPCCBF_FACT_NEXT_STATES);
    f.insert = on(MPCCBF_FACT_INSERT);
    f.est = on(MPCCBF_FACT_EST);
    return f;
}

LaunchPlan impc_launch_plan(const DevOps& op, int variant, int n, bool csr, int knn_k, bool store, bool conn,
                            const LaunchFacts& f) {
    // the separable layout with one row slot per lane and channel (up to 16 box rows per channel)
    const bool sep = op.sep && op.nzd == SEP_NZD_HOST;
    const bool sep16 = sep && op.sep_rows_per_dim <= 16;
    const bool slack = op.slack_mode != 0;
    // row slots per lane and channel of the separable slack kernel (2: up to 32 rows per channel,
    // e.g. K = 16 as in the reference's instance files); 0: no slack instantiation fits
    const int slack_sb = !(sep && op.cbf_h <= 2) ? 0 : (op.sep_rows_per_dim <= 16 ? 1 : (op.sep_rows_per_dim <= 32 ? 2 : 0));
    // the one-agent-per-wave kernel: no slack variables, the dual active set on, the operators
    // within its LDS stage; share-adaptive (variant 0) up to one agent per SIMD of the device
    // (the collision controller's: cbf_mode is 0 or 1, validate_params, and 1 takes the FoV branch)
    const bool wide = !slack && sep16 && op.dual_as > 0 && op.cbf_h <= MAX_CBF_H && op.hot > 0 &&
                      op.hot <= IMPC_WIDE_OPS_MAX &&
                      (variant == VARIANT_WIDE || (variant == 0 && n <= op.wide_max));
    const bool sep_variant = variant == 0 || variant == VARIANT_SEP16;
    // the lean main launch (fast start + dual active set; everything else deferred) has no store
    // instantiation: while a store is attached the 16-lane layout runs its full kernel
    const bool lean = sep_variant && !wide && !slack && sep16 && op.lean && !store && op.dual_as > 0;
    const bool full16 = sep_variant && sep16;
    // some agent can exceed the 16 CBF row slots (caller lists, or k nearest x CBF samples > 16)
    const bool exceed = csr || knn_k * op.cbf_h > 16;
    // the dense 16-lane instantiation has 64 - m CBF row slots and no capacity launch (beyond them
    // a QP reports ERROR): the default variant takes it only when no agent can exceed them (grid
    // lists: at most knn_k neighbours x cbf_h samples), else the 64-lane one with 256 - m slots
    const bool dense16 = op.m < 64 && (variant == 3 || (variant == 0 && !csr && knn_k * op.cbf_h <= 64 - op.m));

    // the loop form (FORM_LOOP, impc.hpp): every launch-uniform option as that form fixes it
    const bool loop = !csr && f.targets && f.traj_t && !f.substeps && !f.cov && !f.cone && !f.nb_out && !f.est &&
                      !f.primal_res && !f.dual_res && f.x && f.status && f.obj && f.iters && f.next_states && f.insert;

    LaunchPlan p{};
    p.capacity = IMPC_NONE;
    p.form = FORM_GENERIC;
    if (conn) {
        p.kernel = op.cbf_mode == 0 && !slack && sep16 ? IMPC_CONN : IMPC_NONE;
        p.name = SHAPES[IMPC_CONN].name;
    } else if (op.cbf_mode == 1) {
        // (slack mode: 4 kinds x cbf_h rows per 8-lane segment)
        const bool ok = op.nz == 15 && op.m <= IMPC_FOV_ROWS_MAX && (!slack || op.cbf_h <= 2);
        // (the estimate form: the same kernel reading the per-pair buffers, mpccbf_set_fov_estimates)
        const ImpcKernel k = f.est ? (slack ? IMPC_FOV_SLACK_EST : IMPC_FOV_EST) : (slack ? IMPC_FOV_SLACK : IMPC_FOV);
        p.kernel = !ok ? IMPC_NONE : k;
        p.name = SHAPES[k].name;
    } else {
        p.store = store && !slack && (wide || full16);
        if (slack) {
            p.kernel = slack_sb == 1 ? IMPC_SLACK1 : (slack_sb == 2 ? IMPC_SLACK2 : IMPC_NONE);
            // (more than 16 neighbours only from caller lists: grid mode takes knn_k <= 16)
            p.defer = slack_sb > 0 && csr;
            p.capacity = slack_sb == 2 ? IMPC_QUEUE_SLACK2 : IMPC_QUEUE_SLACK1;
        } else {
            if (wide) p.kernel = p.store ? IMPC_WIDE_STORE : IMPC_WIDE;
            else if (lean) p.kernel = IMPC_SEP_LEAN;
            else if (full16) p.kernel = p.store ? IMPC_SEP_STORE : IMPC_SEP;
            else if (op.nz == 6 && dense16) p.kernel = IMPC_DENSE_16_4;
            else if (op.nz == 6 && variant == 1 && op.m < 64) p.kernel = IMPC_DENSE_64_1;
            else if (op.nz == 6 && op.m < 256) p.kernel = IMPC_DENSE_64_4;
            else p.kernel = IMPC_NONE;
            // the lean and the wide main launches always may defer; the full 16-lane kernel when
            // its 16 CBF row slots can be exceeded
            p.defer = wide || lean || (full16 && exceed);
            p.capacity = p.store ? (exceed ? IMPC_QUEUE8_STORE : IMPC_QUEUE1_STORE) : (exceed ? IMPC_QUEUE8 : IMPC_QUEUE1);
        }
        if (!p.defer) p.capacity = IMPC_NONE;
        if (p.kernel == IMPC_SEP && loop) {
            p.kernel = IMPC_SEP_LOOP;
            p.form = FORM_LOOP;
        }
        p.name = SHAPES[p.kernel].name;
    }
    const KernelShape& sh = SHAPES[p.kernel != IMPC_NONE ? p.kernel : (conn ? IMPC_CONN : IMPC_NONE)];
    p.block_size = sh.block_size;
    p.agents_per_block = sh.agents_per_block;
    p.clock_waves = (n > 0 && sh.clock) ? plan_blocks(p, n) * (sh.block_size / 64) : 0;
    return p;
}

static void pack(std::vector<double>& v, int32_t& off, const Mat& m) {
    off = (int32_t)v.size();
    v.insert(v.end(), m.a.begin(), m.a.end());
}
static void pack(std::vector<double>& v, int32_t& off, const std::vector<double>& m) {
    off = (int32_t)v.size();
    v.insert(v.end(), m.begin(), m.end());
}
static void pack(std::vector<double>& v, int32_t& off, const std::vector<Mat>& ms) {
    off = (int32_t)v.size();
    for (const Mat& m : ms) v.insert(v.end(), m.a.begin(), m.a.end());
}

PackedOps pack_operators(const Operators& o, const mpccbf_params& prm, const mpccbf_options& so) {
    const mpccbf_params* p = &prm;
    PackedOps out;
    DevOps& d = out.dev;
    std::vector<double>& v = out.buf;
    std::memset(&d, 0, sizeof(d));
    d.n = o.n;
    d.nz = o.nz;
    d.m = o.G.r;
    d.mc = o.Cs.r;
    d.K = o.K;
    d.spd_f = o.spd_f;
    d.cbf_h = o.cbf_h;
    d.impc_iter = p->impc_iter;
    // operator buffer: the operators of the separable kernels first (the "hot" prefix the
    // one-agent-per-wave kernel stages in LDS, DevOps::hot), then the rest
    // separable layout: box rows regrouped by channel, 16 per channel (lanes of a group)
    d.sep = 0;
    d.o_Gsep = 0;
    if (o.sep && o.nzd == SEP_NZD_HOST) {
        int per[DIM] = {0, 0, 0};
        bool ok = true;
        for (int i = 0; i < o.G.r; i++) {
            if (o.row_dim[i] < 0 || o.row_dim[i] >= DIM) ok = false;
            else per[o.row_dim[i]]++;
            if (!(o.lo[i] > -1e300 && o.hi[i] < 1e300)) ok = false;  // the layout is two-sided only
        }
        const int rpd = std::max(per[0], std::max(per[1], per[2]));
        const int sb = (rpd + 15) / 16;  // row slots per lane and channel
        if (ok && sb <= 2) {
            std::vector<double> B((size_t)DIM * sb * 16 * SEP_ROW, 0.0);
            for (size_t r = 0; r < (size_t)DIM * sb * 16; r++) {
                B[r * SEP_ROW + 8] = -1.0;  // inert row: 0 in [-1, 1]
                B[r * SEP_ROW + 9] = 1.0;
            }
            int fill[DIM] = {0, 0, 0};
            for (int i = 0; i < o.G.r; i++) {
                const int dd = o.row_dim[i], f = fill[dd]++;
                // slot f / 16, lane f % 16 (sb = 1: row f of the channel in lane f)
                double* r = &B[((size_t)(dd * sb + f / 16) * 16 + f % 16) * SEP_ROW];
                r[0] = o.G(i, dd * o.nzd);
                r[1] = o.G(i, dd * o.nzd + 1);
                for (int s = 0; s < SD; s++) r[2 + s] = o.Gs(i, s);
                r[8] = o.lo[i];
                r[9] = o.hi[i];
            }
            pack(v, d.o_Gsep, B);
            std::vector<double> Pi((size_t)DIM * 3, 0.0);  // [[a b] [b c]]^-1 per channel
            for (int dd = 0; dd < DIM; dd++) {
                const int r0 = dd * o.nzd;
                const double a = o.Pr(r0, r0), b = o.Pr(r0, r0 + 1), cc = o.Pr(r0 + 1, r0 + 1);
                const double det = a * cc - b * b;
                Pi[dd * 3 + 0] = cc / det;
                Pi[dd * 3 + 1] = -b / det;
                Pi[dd * 3 + 2] = a / det;
            }
            pack(v, d.o_Pinv, Pi);
            d.sep = 1;
            d.nzd = o.nzd;
            d.sep_rows_per_dim = rpd;
            d.sep_sb = sb;
        }
    }
    pack(v, d.o_Z, o.Z);
    pack(v, d.o_Xs, o.Xs);
    pack(v, d.o_Pr, o.Pr);
    pack(v, d.o_Qs, o.Qs);
    pack(v, d.o_Qt, o.Qt);
    pack(v, d.o_Qr, o.Qr);
    pack(v, d.o_Ks, o.Ks);
    pack(v, d.o_Kt, o.Kt);
    pack(v, d.o_Kr, o.Kr);
    pack(v, d.o_Cs, o.Cs);
    pack(v, d.o_clo, o.clo);
    pack(v, d.o_chi, o.chi);
    pack(v, d.o_UZ, o.UZ);
    pack(v, d.o_US, o.US);
    pack(v, d.o_PZ, o.PZ);
    pack(v, d.o_PS, o.PS);
    pack(v, d.o_AZ, o.AZ);
    pack(v, d.o_AS, o.AS);
    d.P = p->num_pieces;
    d.slack_mode = p->slack_mode ? 1 : 0;
    d.slack_cost = p->slack_cost;
    d.slack_decay = p->slack_decay_rate;
    pack(v, d.o_EB0, o.EB0);
    pack(v, d.o_EB1, o.EB1);
    pack(v, d.o_cum, o.cum);
    d.hot = (int32_t)v.size();
    pack(v, d.o_LPr, o.LPr);
    pack(v, d.o_G, o.G);
    pack(v, d.o_Gs, o.Gs);
    pack(v, d.o_lo, o.lo);
    pack(v, d.o_hi, o.hi);
    d.eval_step = o.eval_step;
    {
        const double tend = o.cum.empty() ? 0.0 : o.cum.back();
        d.az_at_eval = (!o.cum.empty() && std::min(o.eval_step, tend) == std::min(p->h, tend)) ? 1 : 0;
    }
    d.Ts = p->Ts;
    d.nsub = (int)(p->h / p->Ts);
    // FoV controller: Voronoi operators, dense 16-wide box rows, P / LP padded to 16 x 16
    d.cbf_mode = p->cbf_mode;
    d.C = p->num_control_points;
    d.fov_beta = p->fov_beta;
    {
        const dev::FovBorder fb = dev::fov_border(p->fov_beta);
        d.fov_kap = fb.kap;
        d.fov_sig = fb.sig_left;
        d.fov_none = fb.none ? 1 : 0;
    }
    d.fov_Ds = p->fov_Ds;
    d.fov_Rs = p->fov_Rs;
    for (int k = 0; k < 3; k++) d.bbox[k] = p->bbox[k];
    if (p->cbf_mode == 1 && o.nz <= 15) {
        pack(v, d.o_VZ, o.VZ);
        pack(v, d.o_VS, o.VS);
        std::vector<double> W((size_t)o.G.r * WBOX_ROW, 0.0);
        for (int i = 0; i < o.G.r; i++) {
            double* r = &W[(size_t)i * WBOX_ROW];
            for (int j = 0; j < o.nz; j++) r[j] = o.G(i, j);
            for (int s2 = 0; s2 < SD; s2++) r[16 + s2] = o.Gs(i, s2);
            r[22] = o.lo[i];
            r[23] = o.hi[i];
        }
        pack(v, d.o_Wbox, W);
        std::vector<double> P16(256, 0.0), L16(256, 0.0);
        for (int a = 0; a < 16; a++)
            for (int b = 0; b < 16; b++) {
                const bool in = a < o.nz && b < o.nz;
                P16[a * 16 + b] = in ? o.Pr(a, b) : (a == b ? 1.0 : 0.0);
                L16[a * 16 + b] = in ? o.LPr(a, b) : (a == b ? 1.0 : 0.0);
            }
        pack(v, d.o_P16, P16);
        pack(v, d.o_LP16, L16);
        // P^-1 (padded with the identity) for the dual active-set solve: columns of
        // L^-T L^-1 e_b by forward / backward substitution with the factor L = LPr
        std::vector<double> Pi16(256, 0.0);
        for (int b = 0; b < 16; b++) {
            if (b >= o.nz) {
                Pi16[b * 16 + b] = 1.0;
                continue;
            }
            std::vector<double> x(o.nz, 0.0);
            for (int a = 0; a < o.nz; a++) {  // L x = e_b
                double s = a == b ? 1.0 : 0.0;
                for (int k = 0; k < a; k++) s -= o.LPr(a, k) * x[k];
                x[a] = s / o.LPr(a, a);
            }
            for (int a = o.nz - 1; a >= 0; a--) {  // L^T x = x
                double s = x[a];
                for (int k = a + 1; k < o.nz; k++) s -= o.LPr(k, a) * x[k];
                x[a] = s / o.LPr(a, a);
            }
            for (int a = 0; a < o.nz; a++) Pi16[a * 16 + b] = x[a];
        }
        pack(v, d.o_Pinv16, Pi16);
        std::vector<double> wb(o.G.r, 0.0);  // the box rows' weights in the active-set candidate rule
        for (int i = 0; i < o.G.r; i++) {
            double n2 = 0.0;
            for (int a = 0; a < o.nz; a++)
                for (int b = 0; b < o.nz; b++) n2 += o.G(i, a) * Pi16[a * 16 + b] * o.G(i, b);
            wb[i] = 1.0 / std::sqrt(std::max(n2, 1e-30));
        }
        pack(v, d.o_wbox, wb);
        auto pgram = [&](const Mat& A, int i, int j) {  // A_i P^-1 A_j^T
            double g = 0.0;
            for (int a = 0; a < o.nz; a++)
                for (int b = 0; b < o.nz; b++) g += A(i, a) * Pi16[a * 16 + b] * A(j, b);
            return g;
        };
        std::vector<double> wv, wf;
        for (const Mat& V : o.VZ) {
            wv.push_back(pgram(V, 0, 0));
            wv.push_back(pgram(V, 0, 1));
            wv.push_back(pgram(V, 1, 1));
        }
        for (const Mat& U : o.UZ)
            for (int i = 0; i < 3; i++)
                for (int j = i; j < 3; j++) wf.push_back(pgram(U, i, j));
        pack(v, d.o_wvor, wv);
        pack(v, d.o_wfov, wf);
    }
    pack(v, out.o_EB2, o.EB2);  // (after every operator of the solve kernels: their offsets stay)
    v.push_back(0.0);  // keep every offset addressable even for empty operators
    for (int i = 0; i < 3; i++) {
        d.a_lo[i] = o.a_lo[i];
        d.a_hi[i] = o.a_hi[i];
    }
    d.d_min = p->d_min;
    d.cbf_filter = so.no_cbf_filter ? 0 : 1;
    d.maxit = so.max_pdip_iters > 0 ? so.max_pdip_iters : 60;
    d.tol = so.tolerance > 0 ? so.tolerance : 1e-9;
    // solver pipeline: from mpccbf_options only (zero = default)
    d.warm_delta = so.warm_delta == 0.0 ? 0.3 : (so.warm_delta > 0.0 ? so.warm_delta : 0.0);
    d.feas_tol = 1e-6;  // CPLEX default feasibility tolerance
    d.early_it = so.early_it == 0 ? 10 : (so.early_it > 0 ? so.early_it : 0);
    d.fast_start = so.no_fast_start ? 0 : 1;
    d.dual_as = so.dual_as_steps == 0 ? 24 : (so.dual_as_steps > 0 ? so.dual_as_steps : 0);
    d.lean = so.lean ? 1 : 0;  // measured no faster at occupancy 1
    d.das_warm = so.das_warm_steps == 0 ? 3 : (so.das_warm_steps > 0 ? so.das_warm_steps : 0);
#ifdef MPCCBF_DIAG_ENV
    {  // diagnostics build only (make diag): tuning overrides from the environment
        const char* e = getenv("MPCCBF_EARLY_IT");
        if (e) d.early_it = atoi(e);
        const char* f = getenv("MPCCBF_FAST_START");
        if (f) d.fast_start = atoi(f);
        const char* g = getenv("MPCCBF_DUAL_AS");
        if (g) d.dual_as = atoi(g);
        const char* l = getenv("MPCCBF_LEAN");
        if (l) d.lean = atoi(l);
        const char* w = getenv("MPCCBF_DAS_WARM");
        if (w) d.das_warm = atoi(w);
        const char* wd = getenv("MPCCBF_WARM_DELTA");
        if (wd) d.warm_delta = std::max(0.0, std::strtod(wd, nullptr));
    }
#endif
    return out;
}

}  // namespace mpccbf

extern "C" int mpccbf_host_launch_form(const mpccbf_params* p, const mpccbf_options* opt, int32_t variant,
                                       int32_t num_agents, int32_t csr, int32_t knn_k, int32_t store,
                                       int32_t connectivity, int32_t wide_max, uint32_t facts, int32_t* kernel_id,
                                       const char** kernel_name, const char** form) {
    using namespace mpccbf;
    if (!p) return set_host_error(MPCCBF_ERR_INVALID_ARGUMENT, "null argument");
    const std::string verr = validate_params(*p);
    if (!verr.empty()) return set_host_error(MPCCBF_ERR_INVALID_ARGUMENT, verr);
    mpccbf_options o;
    if (opt) o = *opt; else std::memset(&o, 0, sizeof(o));
    try {
        PackedOps po = pack_operators(build_operators(*p, o.keep_redundant != 0), *p, o);
        po.dev.wide_max = wide_max;
        const LaunchPlan pl = impc_launch_plan(po.dev, variant, num_agents, csr != 0, knn_k, store != 0,
                                               connectivity != 0, launch_facts_of_bits(facts));
        if (kernel_id) *kernel_id = pl.kernel;
        if (kernel_name) *kernel_name = pl.name;
        if (form) *form = launch_form_name(pl.form);
        return MPCCBF_OK;
    } catch (const std::exception& e) {
        return set_host_error(MPCCBF_ERR_INVALID_ARGUMENT, e.what());
    }
}

extern "C" int mpccbf_host_launch_plan(const mpccbf_params* p, const mpccbf_options* opt, int32_t variant,
                                       int32_t num_agents, int32_t csr, int32_t knn_k, int32_t store,
                                       int32_t connectivity, int32_t wide_max, mpccbf_host_plan* out) {
    using namespace mpccbf;
    if (!p || !out) return set_host_error(MPCCBF_ERR_INVALID_ARGUMENT, "null argument");
    const std::string verr = validate_params(*p);
    if (!verr.empty()) return set_host_error(MPCCBF_ERR_INVALID_ARGUMENT, verr);
    mpccbf_options o;
    if (opt) o = *opt; else std::memset(&o, 0, sizeof(o));
    try {
        PackedOps po = pack_operators(build_operators(*p, o.keep_redundant != 0), *p, o);
        DevOps& d = po.dev;
        d.wide_max = wide_max;
        const LaunchPlan pl = impc_launch_plan(d, variant, num_agents, csr != 0, knn_k, store != 0, connectivity != 0);
        out->kernel_name = pl.name;
        out->capacity_name = SHAPES[pl.capacity].name;
        out->block_size = pl.block_size;
        out->agents_per_block = pl.agents_per_block;
        out->clock_waves = pl.clock_waves;
        out->store = pl.store;
        out->defers = pl.defer;
        out->hot = d.hot;
        out->total = (int32_t)po.buf.size();
        out->wide_capacity = IMPC_WIDE_OPS_MAX;
        out->sep = d.sep;
        out->sep_rows_per_dim = d.sep_rows_per_dim;
        out->sep_sb = d.sep_sb;
        out->o_Gsep = d.o_Gsep;
        const int32_t offs[] = {d.o_Z,    d.o_Xs,   d.o_Pr,  d.o_LPr,  d.o_Qs,     d.o_Qt,   d.o_Qr,   d.o_Ks,
                                d.o_Kt,   d.o_Kr,   d.o_G,   d.o_Gs,   d.o_lo,     d.o_hi,   d.o_Cs,   d.o_clo,
                                d.o_chi,  d.o_UZ,   d.o_US,  d.o_PZ,   d.o_PS,     d.o_AZ,   d.o_AS,   d.o_Gsep,
                                d.o_Pinv, d.o_VZ,   d.o_VS,  d.o_Wbox, d.o_P16,    d.o_LP16, d.o_Pinv16, d.o_wbox,
                                d.o_wvor, d.o_wfov, d.o_EB0, d.o_EB1,  d.o_cum,    po.o_EB2};
        static_assert(sizeof(offs) / sizeof(offs[0]) == MPCCBF_HOST_PLAN_OFFSETS, "mpccbf_host_plan::offsets");
        std::memcpy(out->offsets, offs, sizeof(offs));
        if (out->buf) std::memcpy(out->buf, po.buf.data(), std::min<size_t>(po.buf.size(), (size_t)std::max(out->buf_capacity, 0)) * sizeof(double));
        return MPCCBF_OK;
    } catch (const std::exception& e) {
        return set_host_error(MPCCBF_ERR_INVALID_ARGUMENT, e.what());
    }
}
