// capi.hip — the C ABI of include/mpccbf.h: context lifetime, operator upload, launches (the entry
// points that hold no context: capi_control.hip). No exception crosses this boundary (the
// reference's std::invalid_argument / runtime_error become MPCCBF_ERR_INVALID_ARGUMENT plus a
// thread-local message).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mpccbf.h"
#include "host/defer_queues.hpp"
#include "host/fov_estimates.hpp"
#include "host/grid_rotation.hpp"
#include "host/hip_host.hpp"
#include "host/operators.hpp"
#include "host/pack_operators.hpp"
#include "kernels/impc.hpp"
#include "kernels/cap_audit.hpp"
#include "kernels/conn_rows.hpp"
#include "kernels/launch_plan.hpp"
#include "kernels/monitor.hpp"
#include "kernels/pf_fov.hpp"

namespace mpccbf {

static thread_local std::string g_err;

int set_error(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// Grid mode's three neighbour tables (GridArgs) in one buffer grown on demand, with the rotation
// that says which of them a step uses and what a later call may continue (grid_rotation.hpp). The
// device calls are here; every decision, and the only writes of the continuation record, are rot's.
struct GridTables {
    DevBuf buf;
    GridRotation rot;
    uint32_t *cnt[3] = {}, *slots[3] = {};
    double* sst[3] = {};

    // the tables of a state table of num_states rows
    int carve(int num_states) {
        const size_t tb = grid_table_bytes(num_states);
        rot.reallocates(3 * tb, buf.bytes);
        HIP_TRY(buf.reserve(3 * tb));
        for (int t = 0; t < 3; t++)
            grid_table_carve(buf.as<char>() + t * tb, num_states, &cnt[t], &slots[t], &sst[t]);
        return MPCCBF_OK;
    }
    // table 0 from these states; zero_fill: table 1 zeroed for the inserts of the step that reads it
    int rebuild(const double* states, int num_states, double radius, bool zero_fill, hipStream_t stream) {
        const size_t cb = (size_t)grid_table_size(num_states) * 4;
        HIP_TRY(hipMemsetAsync(cnt[0], 0, cb, stream));
        if (zero_fill) HIP_TRY(hipMemsetAsync(cnt[1], 0, cb, stream));
        HIP_TRY(launch_grid_insert(states, num_states, 0, 0, radius, cnt[0], slots[0], sst[0], stream));
        return MPCCBF_OK;
    }
};

// What the last IMPC launch was, for the calls that report it (mpccbf_kernel_name: the name is
// share-adaptive in the agents, and the default variant's dense layout depends on where the
// neighbour lists come from; mpccbf_launch_form)
struct LastLaunch {
    int n = 0;
    bool csr = false;
    int knn = 0;
    LaunchForm form = FORM_GENERIC;
};

}  // namespace mpccbf

struct mpccbf_ctx {
    std::vector<hipEvent_t> events;  // timing events of mpccbf_run_steps (grown on demand)
    mpccbf_params p;
    mpccbf_options opt;
    mpccbf::Operators ops;
    mpccbf::DevOps dev;
    int device = 0;
    mpccbf::DevBuf dbuf;          // the packed operators (pack_operators)
    mpccbf::DevBuf scratch;       // mpccbf_build_neighbors
    mpccbf::GridTables grid;      // grid mode's neighbour tables and their rotation
    // the two deferral queues (defer_queues.hpp: offsets into defer)
    mpccbf::DevBuf defer;
    mpccbf::DeferQueues queues;
    int variant = 0;
    mpccbf::LastLaunch last;
    // active-set store (mpccbf_set_active_store): the caller's device buffer of store_rows records,
    // or nullptr; store_min_steps as the kernels take it (>= 1, or < 0: export only)
    int32_t* store = nullptr;
    int store_rows = 0;
    int store_min_steps = 0;
    // neighbour-cap audit (mpccbf_cap_audit_run): the second-derivative basis' offset in dbuf, and
    // the scratch its iteration-0 launch writes (x0: agents x n doubles, then their statuses)
    int32_t o_EB2 = 0;
    mpccbf::DevBuf audit_scratch;
    // connectivity rows (mpccbf_set_connectivity): the teams (host copy), the caller's outputs, and
    // the device tables the spectrum launch fills per step and the IMPC launch reads (ConnArgs;
    // allocated at the first solve, rows: the state rows they cover)
    struct {
        bool on = false;
        double dmax = 0.0, l2_min = 0.1, l2_switch = 0.1;
        std::vector<int32_t> team_ptr;
        double* out_l2 = nullptr;
        double* out_fiedler = nullptr;
        int rows = 0;
        mpccbf::DevBuf d_team_ptr, d_team_mode, d_row_team;  // int32
        mpccbf::DevBuf d_team_l2, d_fiedler;                 // double
    } conn;
    // per-pair neighbour estimates (mpccbf_set_fov_estimates): the caller's buffers as attached
    // (e.pf: null, or &pf, the copied filter parameters mpccbf_run_steps steps the filter with)
    struct {
        bool on = false;
        mpccbf_fov_estimates e{};
        mpccbf_pf_params pf{};
    } est;
    // safety monitor (mpccbf_set_monitor): the caller's monitor as attached (its buffers stay the
    // caller's); every step's samples are scored after the step's IMPC launch (monitor_after_step)
    struct {
        bool on = false;
        mpccbf_monitor m{};
    } mon;
};

using namespace mpccbf;

// The launch plan of the context's next IMPC step for n agents (launch_plan.hpp)
static LaunchPlan ctx_plan(const mpccbf_ctx* c, int n, bool csr, int knn_k, bool store) {
    LaunchFacts f{};
    f.est = c->est.on;
    return impc_launch_plan(c->dev, c->variant, n, csr, knn_k, store, c->conn.on, f);
}

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

static int check_agent_range(const mpccbf_batch* b) {
    if (b->num_agents < 0 || b->agent_first < 0 || b->agent_first + b->num_agents > b->num_states)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "agent range outside states");
    return MPCCBF_OK;
}

// a batch of at least one agent
static int check_batch(const mpccbf_ctx* c, const mpccbf_batch* b, bool grid, const int32_t* store) {
    if (!b->states || (!grid && !b->nb_col && b->num_states > 1))
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "states / neighbour CSR missing");
    if (grid && (b->knn_k < 1 || !(b->knn_radius > 0)))
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "grid neighbours need knn_k >= 1 and knn_radius > 0");
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

// One IMPC step for a batch, enqueued on `stream`; ev0 / ev1 (optional) are recorded around the
// IMPC kernel alone. run_step >= 0: step run_step of the grid-mode mpccbf_run_steps call that
// started the rotation (GridRotation::step); < 0: a step outside a rotation (foreign_step).
// ops / store: the context's (c->dev, c->store), or what the cap audit puts in their place.
int impc_enqueue(mpccbf_ctx* c, const mpccbf_batch* b, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1,
                 const DevOps& ops, int32_t* store, int run_step = -1, unsigned long long* kclock = nullptr) {
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


// The attached monitor's score of the step `b` just enqueued, behind its IMPC launch on the same
// stream: the step's sub-step records when the batch gives them, else its one next-state sample.
// The rows outside the agent range are those of the table the step read. The IMPC launch itself is
// untouched (nothing here is an argument of it).
// What the attached monitor refuses of a batch, ahead of the step's launches
static int monitor_step_check(const mpccbf_ctx* c, const mpccbf_batch* b) {
    if (!c->mon.on || b->num_agents <= 0) return MPCCBF_OK;
    const mpccbf_monitor& m = c->mon.m;
    if (b->num_states > m.rows || b->num_states > MONITOR_MAX_ROWS)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "monitor: rows (" + std::to_string(m.rows) + ") < num_states (" +
                                                     std::to_string(b->num_states) + ")");
    if (monitor_scratch_bytes(b->num_states, b->substeps ? c->dev.nsub : 1) > m.scratch_bytes)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "monitor: scratch too small for this step's samples");
    return MPCCBF_OK;
}

static int monitor_after_step(mpccbf_ctx* c, const mpccbf_batch* b, hipStream_t stream) {
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
    for (hipEvent_t e : c->events) (void)hipEventDestroy(e);
    delete c;  // (its device buffers with it)
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


// ---------------------------------------------------------------------------------------------
// Closed-loop stepping + RCCL exchange
// ---------------------------------------------------------------------------------------------
// In-process communicator group (mpccbf_comm_create_local): the ranks are host threads of one
// process on one device; the per-step all-gather becomes device copies between their state
// tables, ordered by one event per rank and step and a host barrier, so mpccbf_run_steps runs its
// N-rank data flow (own block written by the IMPC kernel, exchange, the other blocks inserted
// into the next neighbour table) on a single GPU.
struct LocalGroup {
    int nranks = 0;
    std::mutex m;
    std::condition_variable cv;
    int arrived = 0;
    long long gen = 0;
    std::vector<double*> table[2];     // [step & 1][rank]: the table that rank wrote this step
    std::vector<hipEvent_t> ev[2];     // [step & 1][rank]: that rank's IMPC kernel of the step done
    // (double-buffered by step parity: a rank rewrites slot s & 1 only after the barrier of step
    // s + 1, which every peer reaches after enqueueing its step-s copies)
    std::vector<int> nsteps;           // [rank]: num_steps of the current mpccbf_run_steps call
    bool aborted = false;              // a rank left early: every barrier fails from then on
    // false: a rank aborted (the group cannot be used again; destroy and recreate it)
    bool barrier() {
        std::unique_lock<std::mutex> lk(m);
        if (aborted) return false;
        const long long g = gen;
        if (++arrived == nranks) {
            arrived = 0;
            gen++;
            cv.notify_all();
            return true;
        }
        cv.wait(lk, [&] { return gen != g || aborted; });
        return gen != g;
    }
    void abort() {
        std::lock_guard<std::mutex> lk(m);
        aborted = true;
        cv.notify_all();
    }
};

// Aborts the rank's in-process group when mpccbf_run_steps leaves before its last barrier, so the
// peers' barriers return an error instead of waiting forever.
struct GroupAbortGuard {
    LocalGroup* g = nullptr;
    ~GroupAbortGuard() {
        if (g) g->abort();
    }
};

struct mpccbf_comm {
    ncclComm_t nccl = nullptr;
    int nranks = 1, rank = 0, device = 0;
    std::shared_ptr<LocalGroup> local;  // set: in-process group (no RCCL)
};

extern "C" {

int mpccbf_comm_unique_id(char id_out[MPCCBF_COMM_ID_BYTES]) {
    if (!id_out) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null argument");
    static_assert(sizeof(ncclUniqueId) == MPCCBF_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    const ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(MPCCBF_ERR_HIP, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    std::memcpy(id_out, &id, sizeof(id));
    return MPCCBF_OK;
}

int mpccbf_comm_create(const char id[MPCCBF_COMM_ID_BYTES], int32_t nranks, int32_t rank, int32_t device,
                       mpccbf_comm** out) {
    if (!id || !out || nranks < 1 || rank < 0 || rank >= nranks)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "bad communicator arguments");
    *out = nullptr;
    HIP_TRY(hipSetDevice(device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    mpccbf_comm* cm = new mpccbf_comm();
    cm->nranks = nranks;
    cm->rank = rank;
    cm->device = device;
    const ncclResult_t r = ncclCommInitRank(&cm->nccl, nranks, uid, rank);
    if (r != ncclSuccess) {
        delete cm;
        return fail(MPCCBF_ERR_HIP, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    }
    *out = cm;
    return MPCCBF_OK;
}

int mpccbf_comm_create_local(int32_t nranks, int32_t device, mpccbf_comm** out) {
    if (!out || nranks < 1) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "bad communicator arguments");
    HIP_TRY(hipSetDevice(device));
    auto g = std::make_shared<LocalGroup>();
    g->nranks = nranks;
    for (int p = 0; p < 2; p++) {
        g->table[p].assign(nranks, nullptr);
        g->ev[p].assign(nranks, nullptr);
        for (int r = 0; r < nranks; r++) HIP_TRY(hipEventCreateWithFlags(&g->ev[p][r], hipEventDisableTiming));
    }
    g->nsteps.assign(nranks, 0);
    for (int r = 0; r < nranks; r++) {
        out[r] = new mpccbf_comm();
        out[r]->nranks = nranks;
        out[r]->rank = r;
        out[r]->device = device;
        out[r]->local = g;
    }
    return MPCCBF_OK;
}

void mpccbf_comm_destroy(mpccbf_comm* cm) {
    if (!cm) return;
    if (cm->nccl) (void)ncclCommDestroy(cm->nccl);
    if (cm->local && cm->local.use_count() == 1)
        for (int p = 0; p < 2; p++)
            for (hipEvent_t e : cm->local->ev[p]) (void)hipEventDestroy(e);
    delete cm;
}

int mpccbf_run_steps(mpccbf_ctx* c, const mpccbf_batch* b, mpccbf_run* r, void* stream_) {
    if (!c || !b || !r) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null argument");
    // (before the group's first barrier: a refused rank never joins it)
    if (c->mon.on && r->comm && r->comm->nranks > 1)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "monitor: a communicator of more than one rank is not supported");
    // in-process group: any return before the last step's barrier aborts the group (the peers
    // get an error), and every rank must run the same number of steps
    LocalGroup* lg = (r->comm && r->comm->nranks > 1 && r->comm->local) ? r->comm->local.get() : nullptr;
    GroupAbortGuard guard{lg};
    if (lg) {
        {
            std::lock_guard<std::mutex> lk(lg->m);
            lg->nsteps[r->comm->rank] = r->num_steps;
        }
        if (!lg->barrier()) return fail(MPCCBF_ERR_HIP, "run: a rank of the in-process group aborted");
        bool same = true;
        {
            std::lock_guard<std::mutex> lk(lg->m);
            for (int v : lg->nsteps) same = same && v == r->num_steps;
        }
        // (every rank reads the counts before any rank can overwrite them at its next call's
        // entry: that write follows this call's step barriers, or the abort below)
        if (!same) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "run: ranks of the in-process group differ in num_steps");
        if (r->num_steps == 0) {
            c->grid.rot.no_rotation();
            if (!lg->barrier()) return fail(MPCCBF_ERR_HIP, "run: a rank of the in-process group aborted");
            guard.g = nullptr;
            return MPCCBF_OK;
        }
    }
    if (r->num_steps < 0 || !r->states_alt || !b->states)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "run: num_steps < 0 or missing state tables");
    const int first = b->agent_first, count = b->num_agents, ns = b->num_states;
    if (first < 0 || count < 0 || first + count > ns) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "agent range outside states");
    if (r->comm && (ns != r->comm->nranks * count || first != r->comm->rank * count))
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "run: ranks must own equal contiguous agent blocks");
    {
        const std::string est_err = fov_estimates_solve_error(c->est.on, false, r->comm ? r->comm->nranks : 1);
        if (!est_err.empty()) return fail(MPCCBF_ERR_INVALID_ARGUMENT, est_err);
    }
    if (r->num_steps > 0) {
        const int mrc = monitor_step_check(c, b);
        if (mrc != MPCCBF_OK) return mrc;
    }
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    const bool timing = r->step_ms || r->solve_ms;
    const int kcw = mpccbf_impc_launch_waves(c, count);  // (pairs per step)
    if (r->kernel_clock && r->kernel_clock_waves < kcw)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "run: kernel_clock_waves < mpccbf_impc_launch_waves (" +
                                                     std::to_string(kcw) + ")");
    if (r->kernel_clock && r->num_steps > 0)
        HIP_TRY(hipMemsetAsync(r->kernel_clock, 0,
                               2 * sizeof(uint64_t) * (size_t)r->kernel_clock_waves * (size_t)r->num_steps, stream));
    const int need = 3 * std::max(r->num_steps, r->reserve_steps) + 1;
    while ((int)c->events.size() < need) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        c->events.push_back(e);
    }
    double* tables[2] = {const_cast<double*>(b->states), r->states_alt};
    const size_t per_log = (size_t)count * c->p.impc_iter;
    mpccbf_batch sb = *b;
    hipEvent_t* ev = c->events.data();
    if (timing) HIP_TRY(hipEventRecord(ev[0], stream));
    // grid mode: the rotation of the previous call continued, or neighbour table 0 from the initial
    // states and table 1 zeroed for step 0's inserts (each IMPC launch zeroes the table two steps
    // ahead). Only a grid-mode call that runs at least one step leaves a rotation to continue.
    const bool gtab = b->nb_row_ptr == nullptr && count > 0 && r->num_steps > 0;
    GridTables& gt = c->grid;
    if (!gtab) gt.rot.no_rotation();
    if (gtab) {
        if (b->knn_k < 1 || !(b->knn_radius > 0))
            return fail(MPCCBF_ERR_INVALID_ARGUMENT, "grid neighbours need knn_k >= 1 and knn_radius > 0");
        int rc = gt.carve(ns);
        if (rc != MPCCBF_OK) return rc;
        const GridQuery q{b->states, ns, first, count, b->knn_k, b->knn_radius};
        if (gt.rot.run_started(q, r->continue_tables != 0) < 0 &&
            (rc = gt.rebuild(b->states, ns, b->knn_radius, true, stream)) != MPCCBF_OK)
            return rc;
    }
    for (int s = 0; s < r->num_steps; s++) {
        double* cur = tables[s & 1];
        double* nxt = tables[(s & 1) ^ 1];
        sb.states = cur;
        sb.next_states = nxt + (size_t)first * 6;
        sb.step_index = b->step_index + s;
        if (r->status_log) sb.status = r->status_log + (size_t)s * per_log;
        if (r->iters_log) sb.iters = r->iters_log + (size_t)s * per_log;
        if (!r->comm) {  // rows this batch does not solve (static agents) carry over
            if (first > 0)
                HIP_TRY(hipMemcpyAsync(nxt, cur, (size_t)first * 6 * sizeof(double), hipMemcpyDeviceToDevice, stream));
            const int tail = ns - first - count;
            if (tail > 0)
                HIP_TRY(hipMemcpyAsync(nxt + (size_t)(first + count) * 6, cur + (size_t)(first + count) * 6,
                                       (size_t)tail * 6 * sizeof(double), hipMemcpyDeviceToDevice, stream));
        }
        // the attached filter's step against the table this step reads, ahead of the IMPC launch:
        // mpccbf_pf_step over the batch's lists (pairs beyond the attached rows are skipped)
        if (c->est.on && c->est.e.pf && b->nb_row_ptr && count > 0) {
            const auto& e = c->est.e;
            mpccbf_pf_batch pb;
            std::memset(&pb, 0, sizeof(pb));
            pb.num_states = ns;
            pb.states = cur;
            pb.agent_first = first;
            pb.num_agents = count;
            pb.nb_row_ptr = b->nb_row_ptr;
            pb.nb_col = b->nb_col;
            pb.num_pairs = e.num_pairs;  // (blocks; past the lists' end they leave at once)
            pb.particles = e.particles;
            pb.weights = e.weights;
            pb.est_xy = e.est_xy;
            pb.est_cov = e.est_cov;
            pb.flags = e.flags;
            pb.step_index = b->step_index + s;
            const int prc = pf_enqueue(e.pf, &pb, c->device, stream, false, e.num_pairs);
            if (prc != MPCCBF_OK) return prc;
        }
        const bool tk = r->solve_ms && (r->solve_stride <= 1 || s % r->solve_stride == 0);
        const int rc = impc_enqueue(c, &sb, stream, tk ? ev[3 * s + 1] : nullptr, tk ? ev[3 * s + 2] : nullptr,
                                    c->dev, c->store, gtab ? s : -1,
                                    r->kernel_clock ? (unsigned long long*)r->kernel_clock +
                                                          2 * (size_t)r->kernel_clock_waves * s
                                                    : nullptr);
        if (rc != MPCCBF_OK) return rc;
        // (a single rank: the table of the next step is complete behind the IMPC launch)
        const int mrc = monitor_after_step(c, &sb, stream);
        if (mrc != MPCCBF_OK) return mrc;
        if (r->comm && r->comm->nranks > 1 && r->comm->local) {
            // in-process group: every rank's block of this step copied into this rank's table
            LocalGroup& g = *r->comm->local;
            const int me = r->comm->rank;
            g.table[s & 1][me] = nxt;
            HIP_TRY(hipEventRecord(g.ev[s & 1][me], stream));
            if (!g.barrier()) return fail(MPCCBF_ERR_HIP, "run: a rank of the in-process group aborted");
            for (int p = 0; p < g.nranks; p++) {
                if (p == me) continue;
                HIP_TRY(hipStreamWaitEvent(stream, g.ev[s & 1][p], 0));
                HIP_TRY(hipMemcpyAsync(nxt + (size_t)p * count * 6, g.table[s & 1][p] + (size_t)p * count * 6,
                                       (size_t)count * 6 * sizeof(double), hipMemcpyDeviceToDevice, stream));
            }
        } else if (r->comm && r->comm->nranks > 1) {
            const ncclResult_t nr = ncclAllGather(nxt + (size_t)first * 6, nxt, (size_t)count * 6, ncclDouble,
                                                  r->comm->nccl, stream);
            if (nr != ncclSuccess) return fail(MPCCBF_ERR_HIP, std::string("ncclAllGather: ") + ncclGetErrorString(nr));
        }
        // the rows the kernel did not insert (static rows / the other ranks' rows) join the table
        // of the next step
        if (gtab && count < ns) {
            const int t = gt.rot.step(s).fill;
            HIP_TRY(launch_grid_insert(nxt, ns, first, first + count, b->knn_radius, gt.cnt[t], gt.slots[t],
                                       gt.sst[t], stream));
        }
        if (r->step_ms || (timing && s == r->num_steps - 1)) HIP_TRY(hipEventRecord(ev[3 * s + 3], stream));
    }
    guard.g = nullptr;  // every barrier of the call passed: the peers no longer wait on this rank
    r->final_table = r->num_steps & 1;
    // where a continuing call picks the rotation up (mpccbf_run::continue_tables)
    if (gtab) gt.rot.run_finished(tables[r->num_steps & 1], r->num_steps);
    if (timing && r->num_steps > 0) {
        HIP_TRY(hipEventSynchronize(ev[3 * (r->num_steps - 1) + 3]));
        for (int s = 0; s < r->num_steps; s++) {
            float ms = 0.f;
            if (r->step_ms) {
                HIP_TRY(hipEventElapsedTime(&ms, ev[s == 0 ? 0 : 3 * (s - 1) + 3], ev[3 * s + 3]));
                r->step_ms[s] = ms;
            }
            if (r->solve_ms) {
                if (r->solve_stride <= 1 || s % r->solve_stride == 0) {
                    HIP_TRY(hipEventElapsedTime(&ms, ev[3 * s + 1], ev[3 * s + 2]));
                    r->solve_ms[s] = ms;
                } else {
                    r->solve_ms[s] = -1.f;
                }
            }
        }
    }
    return MPCCBF_OK;
}

}  // extern "C"
