// capi.hip — the C ABI of include/mpccbf.h for a context: its lifetime, operator upload, setters and
// single launches, and impc_enqueue, the one IMPC step that every launch path goes through
// (the communicators and mpccbf_run_steps: capi_run.hip, which shares capi_ctx.hpp with this
// unit; the entry points that hold no context: capi_control.hip). No exception crosses this
// boundary (the reference's std::invalid_argument / runtime_error become
// MPCCBF_ERR_INVALID_ARGUMENT plus a thread-local message).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_ctx.hpp"
#include "host/fov_estimates.hpp"
#include "host/pack_operators.hpp"
#include "kernels/cap_audit.hpp"
#include "kernels/conn_rows.hpp"
#include "kernels/monitor.hpp"

namespace mpccbf {

static thread_local std::string g_err;

int set_error(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

}  // namespace mpccbf

using namespace mpccbf;

// Warm-start threshold when mpccbf_set_active_store is given min_steps = 0
constexpr int STORE_MIN_STEPS_DEFAULT = 3;

static void conn_free(mpccbf_ctx* c) {
    auto& k = c->conn;
    for (DevBuf* b : {&k.d_team_ptr, &k.d_team_mode, &k.d_row_team, &k.d_team_l2, &k.d_fiedler}) b->release();
    k.rows = 0;
}

// The connectivity tables for a state table of num_states rows (grown on demand; the team offsets
// and the rows' teams are uploaded here, the rest is written by every step's spectrum launch).
static int conn_tables(mpccbf_ctx* c, int num_states) {
    auto& k = c->conn;
    if (k.d_team_ptr.p && k.rows >= num_states) return MPCCBF_OK;
    conn_free(c);
    const size_t nt = k.team_ptr.size() - 1, rows = (size_t)std::max(num_states, 1);
    HIP_TRY(k.d_team_ptr.reserve((nt + 1) * sizeof(int32_t)));
    HIP_TRY(k.d_team_mode.reserve(std::max<size_t>(nt, 1) * sizeof(int32_t)));
    HIP_TRY(k.d_team_l2.reserve(std::max<size_t>(nt, 1) * sizeof(double)));
    HIP_TRY(k.d_row_team.reserve(rows * sizeof(int32_t)));
    HIP_TRY(k.d_fiedler.reserve(rows * sizeof(double)));
    std::vector<int32_t> row_team(rows, -1);
    for (size_t t = 0; t < nt; t++)
        if (k.team_ptr[t + 1] - k.team_ptr[t] >= 2)  // (teams of one: no rows)
            for (int32_t r = k.team_ptr[t]; r < k.team_ptr[t + 1] && r < num_states; r++) row_team[r] = (int32_t)t;
    HIP_TRY(hipMemcpy(k.d_team_ptr.p, k.team_ptr.data(), (nt + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(k.d_row_team.p, row_team.data(), rows * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(k.d_team_mode.p, 0, k.d_team_mode.bytes));
    HIP_TRY(hipMemset(k.d_team_l2.p, 0, k.d_team_l2.bytes));
    HIP_TRY(hipMemset(k.d_fiedler.p, 0, k.d_fiedler.bytes));
    k.rows = (int)rows;
    return MPCCBF_OK;
}

// ---- the steps of impc_enqueue, in its order ---------------------------------------------------

int mpccbf::check_agent_range(const mpccbf_batch* b) {
    if (b->num_agents < 0 || b->agent_first < 0 || b->agent_first + b->num_agents > b->num_states)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "agent range outside states");
    return MPCCBF_OK;
}

int mpccbf::check_grid_query(const mpccbf_batch* b) {
    if (b->knn_k < 1 || !(b->knn_radius > 0))
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "grid neighbours need knn_k >= 1 and knn_radius > 0");
    return MPCCBF_OK;
}

// a batch of at least one agent
static int check_batch(const mpccbf_ctx* c, const mpccbf_batch* b, bool grid, const int32_t* store) {
    if (!b->states || (!grid && !b->nb_col && b->num_states > 1))
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "states / neighbour CSR missing");
    const int grc = grid ? check_grid_query(b) : MPCCBF_OK;
    if (grc != MPCCBF_OK) return grc;
    if (grid && b->knn_k > NB_MAX)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "grid neighbours: knn_k > 16 not supported (give CSR lists)");
    if (!b->targets && !b->refs) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "targets or refs required");
    if (b->traj_t && !b->x)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "traj_t (closed-loop fallback) needs the persistent x buffer");
    if (!(b->pos_std >= 0.0) || !(b->vel_std >= 0.0))
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "noise standard deviations must be >= 0");
    const std::string est_err = fov_estimates_solve_error(c->est.on, grid, 1);
    if (!est_err.empty()) return fail(MPCCBF_ERR_INVALID_ARGUMENT, est_err);
    if (store && c->store_rows < b->num_states)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "active store: rows (" + std::to_string(c->store_rows) +
                                                     ") < num_states (" + std::to_string(b->num_states) + ")");
    if (c->conn.on && c->conn.team_ptr.back() > b->num_states)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "connectivity: team_ptr ends at row " +
                                                     std::to_string(c->conn.team_ptr.back()) + " > num_states (" +
                                                     std::to_string(b->num_states) + ")");
    return MPCCBF_OK;
}

// This step's team spectra, ahead of the IMPC launch on the same stream, from the state table it
// reads; cn: what the IMPC launch takes from them.
static int enqueue_spectrum(mpccbf_ctx* c, const mpccbf_batch* b, hipStream_t stream, ConnArgs& cn) {
    const int rc = conn_tables(c, b->num_states);
    if (rc != MPCCBF_OK) return rc;
    const auto& k = c->conn;
    SpectrumArgs sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.num_teams = (int32_t)k.team_ptr.size() - 1;
    sp.team_ptr = k.d_team_ptr.as<int32_t>();
    sp.states = b->states;
    sp.first = b->agent_first;
    sp.count = b->num_agents;
    sp.dmax = k.dmax;
    sp.l2_switch = k.l2_switch;
    sp.team_l2 = k.d_team_l2.as<double>();
    sp.team_mode = k.d_team_mode.as<int32_t>();
    sp.fiedler = k.d_fiedler.as<double>();
    sp.out_l2 = k.out_l2;
    sp.out_fiedler = k.out_fiedler;
    HIP_TRY(launch_team_spectrum(sp, stream));
    cn.row_team = k.d_row_team.as<int32_t>();
    cn.team_ptr = sp.team_ptr;
    cn.team_mode = sp.team_mode;
    cn.team_l2 = sp.team_l2;
    cn.fiedler = sp.fiedler;
    cn.dmax = k.dmax;
    cn.l2_min = k.l2_min;
    return MPCCBF_OK;
}

// The step's neighbour tables in their roles. A step outside a rotation (roles.fill < 0) has the
// table it reads built from b->states first (memset + insert kernel) and fills none.
static int grid_args(mpccbf_ctx* c, const mpccbf_batch* b, const DevOps& ops, const GridRoles& roles,
                     hipStream_t stream, GridArgs& g) {
    GridTables& t = c->grid;
    const int rc = t.carve(b->num_states);
    if (rc != MPCCBF_OK) return rc;
    if (roles.fill < 0) {
        const int rb = t.rebuild(b->states, b->num_states, b->knn_radius, false, stream);
        if (rb != MPCCBF_OK) return rb;
    } else {
        g.ins_cnt = t.cnt[roles.fill];
        g.ins_slots = t.slots[roles.fill];
        g.ins_sst = t.sst[roles.fill];
        g.clr_cnt = t.cnt[roles.zero];
    }
    g.cnt = t.cnt[roles.read];
    g.slots = t.slots[roles.read];
    g.sst = t.sst[roles.read];
    g.mask = grid_table_size(b->num_states) - 1;
    g.inv_cell = grid_inv_cell(b->knn_radius);  // (as launch_grid_insert's)
    g.radius = b->knn_radius;
    g.k = b->knn_k;
    // FoV controller: only agents inside the field of view are observed neighbours
    g.cone = (ops.cbf_mode == 1 && ops.fov_beta < 2.0 * M_PI - 1e-9) ? 0.5 * ops.fov_beta : 0.0;
    return MPCCBF_OK;
}

static void batch_args(const mpccbf_batch* b, unsigned long long* kclock, ImpcArgs& a) {
    a.num_states = b->num_states;
    a.states = b->states;
    a.agent_first = b->agent_first;
    a.num_agents = b->num_agents;
    a.targets = b->targets;
    a.refs = b->targets ? nullptr : b->refs;
    a.nb_row_ptr = b->nb_row_ptr;
    a.nb_col = b->nb_col;
    a.x = b->x;
    a.status = b->status;
    a.obj = b->obj;
    a.iters = b->iters;
    a.next_states = b->next_states;
    a.stamps = b->stamps;
    a.traj_t = b->traj_t;
    a.pos_std = b->pos_std;
    a.vel_std = b->vel_std;
    a.noise_seed = b->noise_seed;
    a.step_index = b->step_index;
    a.cov = b->cov;
    a.primal_res = b->primal_res;
    a.dual_res = b->dual_res;
    a.substeps = b->substeps;
    a.nb_out = b->nb_out;
    a.kclock = kclock;
}

// The queue the main launch appends to and the one whose header it zeroes, each with room for
// every agent of the batch (growth: the whole buffer zeroed on the stream)
static int defer_args(mpccbf_ctx* c, int num_agents, hipStream_t stream, ImpcArgs& a) {
    const int rc = c->queues.ensure(num_agents, [&](size_t bytes) -> int {
        HIP_TRY(c->defer.reserve(bytes));
        HIP_TRY(hipMemsetAsync(c->defer.p, 0, bytes, stream));
        return MPCCBF_OK;
    });
    if (rc != MPCCBF_OK) return rc;
    a.defer = c->defer.as<int32_t>() + c->queues.current();
    a.defer_clear = c->defer.as<int32_t>() + c->queues.other();
    return MPCCBF_OK;
}

// One IMPC step for a batch (the arguments: capi_ctx.hpp)
int mpccbf::impc_enqueue(mpccbf_ctx* c, const mpccbf_batch* b, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1,
                         const DevOps& ops, int32_t* store, int run_step, unsigned long long* kclock) {
    if (!c || !b) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null argument");
    const GridRoles roles = run_step < 0 ? c->grid.rot.foreign_step() : c->grid.rot.step(run_step);
    // validate
    int rc = check_agent_range(b);
    if (rc != MPCCBF_OK || b->num_agents == 0) return rc;
    const bool grid = b->nb_row_ptr == nullptr, conn = c->conn.on;
    if ((rc = check_batch(c, b, grid, store)) != MPCCBF_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // spectrum, grid arguments, the batch's fields
    ImpcArgs a;
    std::memset(&a, 0, sizeof(a));
    ConnArgs cn;
    std::memset(&cn, 0, sizeof(cn));
    if (conn && (rc = enqueue_spectrum(c, b, stream, cn)) != MPCCBF_OK) return rc;
    if (grid && (rc = grid_args(c, b, ops, roles, stream, a.grid)) != MPCCBF_OK) return rc;
    batch_args(b, kclock, a);
    // (attached only to contexts of the FoV controller, whose launches alone read them)
    if (c->est.on && ops.cbf_mode == 1) {
        a.est_xy = c->est.e.nb_xy;
        a.est_cov = c->est.e.nb_cov;
        a.est_pairs = c->est.e.num_pairs;
        // (no pair: no list can reach one; a non-null pointer keeps the estimate form, which reads nothing)
        if (!a.est_xy) a.est_xy = b->states;
    }
    // facts and plan
    const LaunchPlan plan = impc_launch_plan(ops, c->variant, b->num_agents, !grid, b->knn_k, store != nullptr, conn,
                                             launch_facts(a));
    if (b->substeps && !b->traj_t)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "substeps (closed-loop records) needs traj_t");
    // store reset: the store is read and written by the kernels that support it; any other launch
    // leaves its agents' records zero (no record), so a record never outlives the solve it describes
    const StoreArgs st{store, c->store_min_steps};
    if (store && !plan.store)
        HIP_TRY(hipMemsetAsync(store + (size_t)b->agent_first * AS_WORDS, 0,
                               (size_t)b->num_agents * AS_WORDS * sizeof(int32_t), stream));
    c->last = LastLaunch{b->num_agents, !grid, b->knn_k, plan.form};
    // queues: agents the main launch defers (the lean launch: QPs that need the PDIP or phase 1;
    // beyond the separable kernel's 16 CBF row slots) are solved by a second launch of the full
    // separable pipeline (128 slots when the 16 can be exceeded)
    // (the connectivity launch has no capacity launch behind it: beyond its rows, ERROR)
    if (plan.defer && (rc = defer_args(c, b->num_agents, stream, a)) != MPCCBF_OK) return rc;
    // main launch
    if (ev0) HIP_TRY(hipEventRecord(ev0, stream));
    const double* buf = c->dbuf.as<double>();
    // one launcher per translation unit that instantiates IMPC kernels (launch_plan.hpp)
    auto launch = [&](ImpcKernel k, int bs, int per_block, const ImpcArgs& ia) {
        const int blocks = (ia.num_agents + per_block - 1) / per_block;
        if (k == IMPC_CONN) return launch_impc_conn(k, blocks, bs, ops, buf, ia, cn, stream);
        if (k == IMPC_FOV || k == IMPC_FOV_SLACK) return launch_impc_fov(k, blocks, bs, ops, buf, ia, stream);
        if (k == IMPC_FOV_EST || k == IMPC_FOV_SLACK_EST)
            return launch_impc_fov_est(k, blocks, bs, ops, buf, ia, stream);
        if (plan.store) return launch_impc_store(k, blocks, bs, ops, buf, ia, st, stream);
        return launch_impc(k, blocks, bs, ops, buf, ia, stream);
    };
    hipError_t e = launch(plan.kernel, plan.block_size, plan.agents_per_block, a);
    if (plan.defer) c->queues.advance(e == hipSuccess);
    // capacity launch
    if (e == hipSuccess && plan.defer) {
        ImpcArgs f = a;
        f.defer = nullptr;
        f.defer_clear = nullptr;
        f.kclock = nullptr;  // (the clock is the main launch's)
        f.queue = a.defer;
        e = launch(plan.capacity, IMPC_QUEUE_BLOCK, IMPC_QUEUE_AGENTS, f);
        // (a queue the fallback never read is zeroed by the main launch after next)
    }
    // events
    if (e == hipSuccess && ev1) e = hipEventRecord(ev1, stream);
    if (e == hipErrorInvalidValue)
        return fail(MPCCBF_ERR_CAPACITY, "no kernel instantiation for this reduced dimension / row count");
    HIP_TRY(e);
    return MPCCBF_OK;
}

// ---- the attached monitor around a step (capi_ctx.hpp) ------------------------------------------

int mpccbf::monitor_step_check(const mpccbf_ctx* c, const mpccbf_batch* b) {
    if (!c->mon.on || b->num_agents <= 0) return MPCCBF_OK;
    const mpccbf_monitor& m = c->mon.m;
    if (b->num_states > m.rows || b->num_states > MONITOR_MAX_ROWS)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "monitor: rows (" + std::to_string(m.rows) + ") < num_states (" +
                                                     std::to_string(b->num_states) + ")");
    if (monitor_scratch_bytes(b->num_states, b->substeps ? c->dev.nsub : 1) > m.scratch_bytes)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "monitor: scratch too small for this step's samples");
    return MPCCBF_OK;
}

int mpccbf::monitor_after_step(mpccbf_ctx* c, const mpccbf_batch* b, hipStream_t stream) {
    if (!c->mon.on || !b->next_states || b->num_agents <= 0) return MPCCBF_OK;
    const bool sub = b->substeps != nullptr;
    const int nsub = c->dev.nsub;
    return monitor_enqueue(&c->mon.m, sub ? b->substeps : b->next_states, sub ? nsub : 1, 6, sub ? (int64_t)nsub * 6 : 6,
                           b->agent_first, b->num_agents, b->states, b->num_states, b->targets, -1, c->device, stream);
}

extern "C" {

int mpccbf_abi_version(void) { return MPCCBF_ABI_VERSION; }

const char* mpccbf_last_error(void) { return g_err.c_str(); }

const char* mpccbf_status_string(int32_t s) {
    switch (s) {
        case MPCCBF_OPTIMAL: return "OPTIMAL";
        case MPCCBF_FEASIBLE: return "FEASIBLE";
        case MPCCBF_UNBOUNDED: return "UNBOUNDED";
        case MPCCBF_INFEASIBLE: return "INFEASIBLE";
        case MPCCBF_ERROR: return "ERROR";
        case MPCCBF_UNKNOWN: return "UNKNOWN";
        case MPCCBF_INFEASIBLEORUNBOUNDED: return "INFEASIBLEORUNBOUNDED";
        default: return "";
    }
}

int mpccbf_create(const mpccbf_params* p, const mpccbf_options* opt, mpccbf_ctx** out) {
    if (!p || !out) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    const std::string verr = validate_params(*p);
    if (!verr.empty()) return fail(MPCCBF_ERR_INVALID_ARGUMENT, verr);
    if (p->cbf_horizon > MAX_CBF_H) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "cbf_horizon > 8 not supported");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(MPCCBF_ERR_NO_DEVICE, "no HIP device visible");
    mpccbf_ctx* c = new mpccbf_ctx();
    c->p = *p;
    if (opt) c->opt = *opt; else std::memset(&c->opt, 0, sizeof(c->opt));
    c->device = c->opt.device;
    try {
        c->ops = build_operators(*p, c->opt.keep_redundant != 0);
    } catch (const std::exception& e) {
        delete c;
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, e.what());
    }
    const PackedOps packed = pack_operators(c->ops, *p, c->opt);
    c->dev = packed.dev;
    c->o_EB2 = packed.o_EB2;
    c->variant = 0;
    hipError_t e = hipSetDevice(c->device);
    c->dev.wide_max = 1024;
    if (e == hipSuccess) {
        // share-adaptive layout: one agent per wave up to one agent per SIMD (4 per CU) of this
        // context's device (kept in the context: no process-wide state shared by contexts)
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0)
            c->dev.wide_max = 4 * prop.multiProcessorCount;
    }
    const size_t bytes = packed.buf.size() * sizeof(double);
    if (e == hipSuccess) e = c->dbuf.reserve(bytes);
    if (e == hipSuccess) e = hipMemcpy(c->dbuf.p, packed.buf.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        delete c;
        return fail(MPCCBF_ERR_HIP, std::string("operator upload: ") + hipGetErrorString(e));
    }
    *out = c;
    return MPCCBF_OK;
}

void mpccbf_destroy(mpccbf_ctx* c) {
    if (!c) return;
    delete c;  // (its device buffers and timing events with it)
}

int mpccbf_num_vars(const mpccbf_ctx* c) { return c ? c->ops.n : -1; }
int mpccbf_reduced_dim(const mpccbf_ctx* c) { return c ? c->ops.nz : -1; }
int mpccbf_num_shared_rows(const mpccbf_ctx* c) { return c ? c->ops.G.r : -1; }

int mpccbf_impc_solve(mpccbf_ctx* c, const mpccbf_batch* b, void* stream) {
    if (!c) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null argument");
    if (b && b->next_states) {
        const int mrc = monitor_step_check(c, b);
        if (mrc != MPCCBF_OK) return mrc;
    }
    const int rc = impc_enqueue(c, b, (hipStream_t)stream, nullptr, nullptr, c->dev, c->store);
    if (rc != MPCCBF_OK || !b) return rc;
    return monitor_after_step(c, b, (hipStream_t)stream);
}

// (the clock waves do not depend on where the neighbour lists come from: the dense layouts, whose
// choice does, write no clock)
int32_t mpccbf_impc_launch_waves(const mpccbf_ctx* c, int32_t num_agents) {
    return c ? ctx_plan(c, num_agents, false, 0, c->store != nullptr).clock_waves : 0;
}

const char* mpccbf_kernel_name(const mpccbf_ctx* c) {
    return c ? ctx_plan(c, c->last.n, c->last.csr, c->last.knn, c->store != nullptr).name : "";
}

const char* mpccbf_launch_form(const mpccbf_ctx* c) { return launch_form_name(c ? c->last.form : FORM_GENERIC); }

int mpccbf_set_active_store(mpccbf_ctx* c, int32_t* store, int32_t rows, int32_t min_steps) {
    if (rows < 0) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "active store: rows must be >= 0");
    if (store != nullptr && rows == 0)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "active store: a buffer needs rows >= 1");
    if (!c) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null context");
    c->store = store;
    c->store_rows = store ? rows : 0;
    c->store_min_steps = min_steps == 0 ? STORE_MIN_STEPS_DEFAULT : min_steps;
    return MPCCBF_OK;
}

int mpccbf_set_connectivity(mpccbf_ctx* c, const mpccbf_connectivity* k) {
    // the checks that need no context first, then the context's
    if (k) {
        if (!(k->d_max > 0.0) || !std::isfinite(k->d_max))
            return fail(MPCCBF_ERR_INVALID_ARGUMENT, "connectivity: d_max must be positive and finite");
        if (!(k->lambda2_min >= 0.0) || !std::isfinite(k->lambda2_min) || !(k->lambda2_switch >= 0.0) ||
            !std::isfinite(k->lambda2_switch))
            return fail(MPCCBF_ERR_INVALID_ARGUMENT, "connectivity: lambda2_min and lambda2_switch must be >= 0 and finite");
        if (k->num_teams < 0) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "connectivity: num_teams < 0");
        if (!k->team_ptr) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "connectivity: team_ptr is required");
        if (k->team_ptr[0] < 0) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "connectivity: team_ptr[0] < 0");
        for (int32_t t = 0; t < k->num_teams; t++)
            if (k->team_ptr[t + 1] < k->team_ptr[t])
                return fail(MPCCBF_ERR_INVALID_ARGUMENT, "connectivity: team_ptr decreases at team " + std::to_string(t));
    }
    if (!c) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null context");
    if (!k) {
        // (the device tables are freed: kernels in flight finish first, hipFree waits for the device)
        (void)hipSetDevice(c->device);
        conn_free(c);
        c->conn.on = false;
        c->conn.team_ptr.clear();
        c->conn.out_l2 = c->conn.out_fiedler = nullptr;
        return MPCCBF_OK;
    }
    if (c->dev.slack_mode) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "connectivity: slack mode is not supported");
    if (c->dev.cbf_mode == 1) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "connectivity: the FoV controller is not supported");
    if (!(k->d_max > c->p.d_min)) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "connectivity: d_max must exceed d_min");
    if (impc_launch_plan(c->dev, c->variant, 1, false, 0, false, true).kernel != IMPC_CONN)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "connectivity: the separable collision controller only");
    (void)hipSetDevice(c->device);
    conn_free(c);
    auto& d = c->conn;
    d.on = true;
    d.dmax = k->d_max;
    d.l2_min = k->lambda2_min == 0.0 ? 0.1 : k->lambda2_min;
    d.l2_switch = k->lambda2_switch == 0.0 ? 0.1 : k->lambda2_switch;
    d.team_ptr.assign(k->team_ptr, k->team_ptr + k->num_teams + 1);
    d.out_l2 = k->lambda2;
    d.out_fiedler = k->fiedler;
    return MPCCBF_OK;
}

int mpccbf_set_fov_estimates(mpccbf_ctx* c, const mpccbf_fov_estimates* e) {
    if (!c) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null context");
    if (!e) {
        c->est.on = false;
        c->est.e = mpccbf_fov_estimates{};
        return MPCCBF_OK;
    }
    const std::string err = fov_estimates_attach_error(c->dev.cbf_mode, *e);
    if (!err.empty()) return fail(MPCCBF_ERR_INVALID_ARGUMENT, err);
    c->est.on = true;
    c->est.e = *e;
    if (e->pf) {
        c->est.pf = *e->pf;
        c->est.e.pf = &c->est.pf;
    }
    return MPCCBF_OK;
}

int mpccbf_set_monitor(mpccbf_ctx* c, const mpccbf_monitor* m) {
    // the checks that need no context first
    if (m) {
        const std::string err = monitor_attach_error(m);
        if (!err.empty()) return fail(MPCCBF_ERR_INVALID_ARGUMENT, err);
    }
    if (!c) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null context");
    c->mon.on = m != nullptr;
    c->mon.m = m ? *m : mpccbf_monitor{};
    return MPCCBF_OK;
}

int mpccbf_cap_audit_run(mpccbf_ctx* c, const mpccbf_batch* b, const mpccbf_cap_audit* au, void* stream_) {
    // the checks that need no device first, then the context's
    if (!b) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "cap audit: null batch");
    if (!au) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "cap audit: null audit");
    if (!au->counts) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "cap audit: counts is required");
    if (!b->x || !b->status)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "cap audit: the solve's x and status are required");
    const bool grid = b->nb_row_ptr == nullptr;
    if (grid && !b->nb_out)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "cap audit: grid mode needs the solve's nb_out");
    if (b->num_agents < 0 || b->agent_first < 0 || b->agent_first + b->num_agents > b->num_states)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "cap audit: agent range outside states");
    if (!(au->tol >= 0.0)) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "cap audit: tol must be >= 0");
    if (!c) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null context");
    if (c->conn.on)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "cap audit: not supported while connectivity is attached");
    if (c->dev.slack_mode) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "cap audit: slack mode is not supported");
    if (c->dev.cbf_mode == 1) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "cap audit: the FoV controller is not supported");
    // (the layouts whose launches can take a store: the separable ones)
    if (!ctx_plan(c, b->num_agents > 0 ? b->num_agents : 1, !grid, b->knn_k, true).store)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "cap audit: the separable layouts only (variants 0, 4, 5)");
    if (c->p.impc_iter > 2) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "cap audit: impc_iter > 2 is not supported");
    if (b->num_agents == 0) return MPCCBF_OK;
    if (!b->states || (!grid && !b->nb_col && b->num_states > 1))
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "cap audit: states / neighbour CSR missing");
    if (b->num_states > AUDIT_MAX_STATES)
        return fail(MPCCBF_ERR_CAPACITY, "cap audit: num_states (" + std::to_string(b->num_states) + ") > " +
                                             std::to_string(AUDIT_MAX_STATES));
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    const size_t xbytes = (size_t)b->num_agents * c->ops.n * sizeof(double);
    const size_t need = xbytes + (size_t)b->num_agents * sizeof(int32_t);
    HIP_TRY(c->audit_scratch.reserve(need));
    double* x0 = c->audit_scratch.as<double>();
    int32_t* st0 = (int32_t*)(c->audit_scratch.as<char>() + xbytes);
    // iteration 0's solutions: the context's own IMPC launch once more on the same batch with one
    // iteration, every output into scratch, no closed-loop state, no diagnostics, no active store
    // (grid mode: a step outside a rotation rebuilds the table from b->states, so the lists are the
    // solve's)
    {
        mpccbf_batch sb = *b;
        sb.x = x0;
        sb.status = st0;
        sb.obj = nullptr;
        sb.iters = nullptr;
        sb.next_states = nullptr;
        sb.stamps = nullptr;
        sb.traj_t = nullptr;
        sb.pos_std = sb.vel_std = 0.0;
        sb.primal_res = sb.dual_res = nullptr;
        sb.substeps = nullptr;
        sb.nb_out = nullptr;
        DevOps one = c->dev;
        one.impc_iter = 1;
        const int rc = impc_enqueue(c, &sb, stream, nullptr, nullptr, one, nullptr);
        if (rc != MPCCBF_OK) return rc;
    }
    AuditArgs a;
    std::memset(&a, 0, sizeof(a));
    a.num_states = b->num_states;
    a.states = b->states;
    a.agent_first = b->agent_first;
    a.num_agents = b->num_agents;
    a.nb_row_ptr = b->nb_row_ptr;
    a.nb_col = b->nb_col;
    a.nb_list = grid ? b->nb_out : nullptr;
    a.x = b->x;
    a.status = b->status;
    a.x0 = x0;
    a.impc_iter = c->p.impc_iter;
    a.o_EB2 = c->o_EB2;
    a.h = c->p.h;
    a.tol = au->tol > 0.0 ? au->tol : 1e-6;
    a.counts = au->counts;
    a.excess = au->excess;
    a.live_nb = au->live_nb;
    HIP_TRY(launch_cap_audit(c->dev, c->dbuf.as<double>(), a, stream));
    if (au->x0_out) HIP_TRY(hipMemcpyAsync(au->x0_out, x0, xbytes, hipMemcpyDeviceToDevice, stream));
    return MPCCBF_OK;
}

int mpccbf_set_variant(mpccbf_ctx* c, int variant) {
    if (!c) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null argument");
    c->variant = variant;
    return MPCCBF_OK;
}

int mpccbf_build_neighbors(mpccbf_ctx* c, const double* states, int32_t num_states,
                           int32_t first, int32_t num_agents, int32_t k, double radius,
                           int32_t* row_ptr, int32_t* col, void* stream) {
    if (!c || !states || !row_ptr) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null argument");
    if (first < 0 || num_agents < 0 || first + num_agents > num_states)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "agent range outside states");
    if (k > 16) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "k > 16 not supported (use k <= 0 for all)");
    if (k > 0 && !(radius > 0)) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "radius must be positive");
    HIP_TRY(hipSetDevice(c->device));
    const size_t need = neighbors_scratch_bytes(num_states, num_agents, k);
    HIP_TRY(c->scratch.reserve(need));
    const int rc = launch_neighbors(states, num_states, first, num_agents, k, radius, row_ptr, col,
                                    c->scratch.p, c->scratch.bytes, (hipStream_t)stream);
    if (rc != 0) return fail(MPCCBF_ERR_HIP, std::string("neighbour kernels: ") + hipGetErrorString((hipError_t)rc));
    return MPCCBF_OK;
}

}  // extern "C"
