// capi_run.hip — closed-loop stepping and the exchange between ranks: the communicators
// (mpccbf_comm_*) and mpccbf_run_steps, a list of named steps around impc_enqueue (capi.hip). What
// a call decides without a device has an owner in csrc/host/: the in-process group's barrier,
// abort rule and num_steps agreement (group_sync.hpp), the timing events' layout
// (step_events.hpp), the neighbour-table rotation (grid_rotation.hpp).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "capi_ctx.hpp"
#include "host/fov_estimates.hpp"
#include "host/group_sync.hpp"
#include "host/step_events.hpp"
#include "kernels/pf_fov.hpp"

namespace mpccbf {

// In-process communicator group (mpccbf_comm_create_local): the ranks are host threads of one
// process on one device; the per-step all-gather becomes device copies between their state
// tables, ordered by one event per rank and step and a host barrier, so mpccbf_run_steps runs its
// N-rank data flow (own block written by the IMPC kernel, exchange, the other blocks inserted
// into the next neighbour table) on a single GPU.
// The slots are double-buffered by step parity: a rank rewrites slot s & 1 only after the barrier
// of step s + 1, which every peer reaches after enqueueing its step-s copies.
// The group owns its events: the last of the communicators that share it destroys them with it.
struct LocalGroup {
    GroupSync sync;
    std::vector<double*> table[2];  // [step & 1][rank]: the table that rank wrote this step
    std::vector<hipEvent_t> ev[2];  // [step & 1][rank]: that rank's IMPC kernel of the step done

    explicit LocalGroup(int nranks) : sync(nranks) {
        for (int p = 0; p < 2; p++) {
            table[p].assign(nranks, nullptr);
            ev[p].assign(nranks, nullptr);
        }
    }
    LocalGroup(const LocalGroup&) = delete;
    LocalGroup& operator=(const LocalGroup&) = delete;
    ~LocalGroup() {
        for (int p = 0; p < 2; p++)
            for (hipEvent_t e : ev[p])
                if (e) (void)hipEventDestroy(e);
    }
    // (after a failure the destructor releases the events created so far)
    int create_events() {
        for (int p = 0; p < 2; p++)
            for (hipEvent_t& e : ev[p]) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return MPCCBF_OK;
    }
};

}  // namespace mpccbf

using namespace mpccbf;

struct mpccbf_comm {
    ncclComm_t nccl = nullptr;
    int nranks = 1, rank = 0, device = 0;
    std::shared_ptr<LocalGroup> local;  // set: in-process group (no RCCL)
};

// ---- the steps of mpccbf_run_steps, in its order -------------------------------------------------

static int group_aborted() { return fail(MPCCBF_ERR_HIP, "run: a rank of the in-process group aborted"); }

// The in-process group at the call's entry: every rank must run the same number of steps.
static int group_handshake(GroupSync& g, int rank, int num_steps) {
    switch (g.agree(rank, num_steps)) {
        case GroupSync::ABORTED: return group_aborted();
        case GroupSync::DIFFERS:
            return fail(MPCCBF_ERR_INVALID_ARGUMENT, "run: ranks of the in-process group differ in num_steps");
        default: return MPCCBF_OK;
    }
}

static int check_run(const mpccbf_ctx* c, const mpccbf_batch* b, const mpccbf_run* r) {
    if (r->num_steps < 0 || !r->states_alt || !b->states)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "run: num_steps < 0 or missing state tables");
    int rc = check_agent_range(b);
    if (rc != MPCCBF_OK) return rc;
    if (r->comm && (b->num_states != r->comm->nranks * b->num_agents || b->agent_first != r->comm->rank * b->num_agents))
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "run: ranks must own equal contiguous agent blocks");
    const std::string est_err = fov_estimates_solve_error(c->est.on, false, r->comm ? r->comm->nranks : 1);
    if (!est_err.empty()) return fail(MPCCBF_ERR_INVALID_ARGUMENT, est_err);
    if (r->num_steps > 0 && (rc = monitor_step_check(c, b)) != MPCCBF_OK) return rc;
    return MPCCBF_OK;
}

// The launch clock of the call's steps, zeroed (mpccbf_run::kernel_clock)
static int clear_kernel_clock(const mpccbf_ctx* c, int count, const mpccbf_run* r, hipStream_t stream) {
    const int kcw = mpccbf_impc_launch_waves(c, count);  // (pairs per step)
    if (r->kernel_clock && r->kernel_clock_waves < kcw)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "run: kernel_clock_waves < mpccbf_impc_launch_waves (" +
                                                     std::to_string(kcw) + ")");
    if (r->kernel_clock && r->num_steps > 0)
        HIP_TRY(hipMemsetAsync(r->kernel_clock, 0,
                               2 * sizeof(uint64_t) * (size_t)r->kernel_clock_waves * (size_t)r->num_steps, stream));
    return MPCCBF_OK;
}
// step s's slice of it
static unsigned long long* kernel_clock_of(const mpccbf_run* r, int s) {
    return r->kernel_clock ? (unsigned long long*)r->kernel_clock + 2 * (size_t)r->kernel_clock_waves * s : nullptr;
}

// Every event the call can need exists before its first step; the start event
static int start_timing(EventPool& events, const StepEvents& plan, hipStream_t stream) {
    const int rc = events.ensure(plan.needed());
    if (rc != MPCCBF_OK) return rc;
    if (plan.records_start()) HIP_TRY(hipEventRecord(events[plan.start()], stream));
    return MPCCBF_OK;
}

// Grid mode: the rotation of the previous call continued, or neighbour table 0 from the initial
// states and table 1 zeroed for step 0's inserts (each IMPC launch zeroes the table two steps ahead).
static int start_rotation(GridTables& gt, const mpccbf_batch* b, bool continue_tables, hipStream_t stream) {
    int rc = check_grid_query(b);
    if (rc != MPCCBF_OK || (rc = gt.carve(b->num_states)) != MPCCBF_OK) return rc;
    const GridQuery q{b->states, b->num_states, b->agent_first, b->num_agents, b->knn_k, b->knn_radius};
    if (gt.rot.run_started(q, continue_tables) < 0)
        return gt.rebuild(b->states, b->num_states, b->knn_radius, true, stream);
    return MPCCBF_OK;
}

// The rows this batch does not solve (static agents) carry over to the next table
static int carry_over_rows(const mpccbf_batch* b, const double* cur, double* nxt, hipStream_t stream) {
    const int first = b->agent_first, end = b->agent_first + b->num_agents, tail = b->num_states - end;
    if (first > 0)
        HIP_TRY(hipMemcpyAsync(nxt, cur, (size_t)first * 6 * sizeof(double), hipMemcpyDeviceToDevice, stream));
    if (tail > 0)
        HIP_TRY(hipMemcpyAsync(nxt + (size_t)end * 6, cur + (size_t)end * 6, (size_t)tail * 6 * sizeof(double),
                               hipMemcpyDeviceToDevice, stream));
    return MPCCBF_OK;
}

// mpccbf_pf_step's batch over the IMPC batch's lists, against the table the step reads
static mpccbf_pf_batch pf_batch(const mpccbf_fov_estimates& e, const mpccbf_batch* b, const double* cur,
                                int64_t step_index) {
    mpccbf_pf_batch pb;
    std::memset(&pb, 0, sizeof(pb));
    pb.num_states = b->num_states;
    pb.states = cur;
    pb.agent_first = b->agent_first;
    pb.num_agents = b->num_agents;
    pb.nb_row_ptr = b->nb_row_ptr;
    pb.nb_col = b->nb_col;
    pb.num_pairs = e.num_pairs;  // (blocks; past the lists' end they leave at once)
    pb.particles = e.particles;
    pb.weights = e.weights;
    pb.est_xy = e.est_xy;
    pb.est_cov = e.est_cov;
    pb.flags = e.flags;
    pb.step_index = step_index;
    return pb;
}

// The attached filter's step, ahead of the IMPC launch (pairs beyond the attached rows are skipped)
static int filter_step(const mpccbf_ctx* c, const mpccbf_batch* b, const double* cur, int64_t step_index,
                       hipStream_t stream) {
    if (!(c->est.on && c->est.e.pf && b->nb_row_ptr && b->num_agents > 0)) return MPCCBF_OK;
    const auto& e = c->est.e;
    const mpccbf_pf_batch pb = pf_batch(e, b, cur, step_index);
    return pf_enqueue(e.pf, &pb, c->device, stream, false, e.num_pairs);
}

// In-process group: every rank's block of step s copied into this rank's table
static int exchange_local(LocalGroup& g, int me, int s, double* nxt, int count, hipStream_t stream) {
    g.table[s & 1][me] = nxt;
    HIP_TRY(hipEventRecord(g.ev[s & 1][me], stream));
    if (!g.sync.barrier()) return group_aborted();
    for (int p = 0; p < g.sync.nranks(); p++) {
        if (p == me) continue;
        HIP_TRY(hipStreamWaitEvent(stream, g.ev[s & 1][p], 0));
        HIP_TRY(hipMemcpyAsync(nxt + (size_t)p * count * 6, g.table[s & 1][p] + (size_t)p * count * 6,
                               (size_t)count * 6 * sizeof(double), hipMemcpyDeviceToDevice, stream));
    }
    return MPCCBF_OK;
}

// Step s's states of every rank into nxt, whose block [first, first + count) this rank wrote
// (a single rank: the table of the next step is complete behind the IMPC launch)
static int exchange(const mpccbf_comm* cm, int s, double* nxt, int first, int count, hipStream_t stream) {
    if (!cm || cm->nranks <= 1) return MPCCBF_OK;
    if (cm->local) return exchange_local(*cm->local, cm->rank, s, nxt, count, stream);
    const ncclResult_t nr = ncclAllGather(nxt + (size_t)first * 6, nxt, (size_t)count * 6, ncclDouble, cm->nccl, stream);
    if (nr != ncclSuccess) return fail(MPCCBF_ERR_HIP, std::string("ncclAllGather: ") + ncclGetErrorString(nr));
    return MPCCBF_OK;
}

// The rows the kernel did not insert (static rows / the other ranks' rows) join the neighbour
// table of the next step
static int insert_foreign_rows(const GridTables& gt, int s, const mpccbf_batch* b, const double* nxt,
                               hipStream_t stream) {
    const int t = gt.rot.step(s).fill;
    HIP_TRY(launch_grid_insert(nxt, b->num_states, b->agent_first, b->agent_first + b->num_agents, b->knn_radius,
                               gt.cnt[t], gt.slots[t], gt.sst[t], stream));
    return MPCCBF_OK;
}

// step_ms and solve_ms, once the call's last event has passed
static int read_timings(const EventPool& events, const StepEvents& plan, const mpccbf_run* r) {
    if (plan.waits_for() < 0) return MPCCBF_OK;
    HIP_TRY(hipEventSynchronize(events[plan.waits_for()]));
    for (int s = 0; s < r->num_steps; s++) {
        float ms = 0.f;
        if (r->step_ms) {
            const StepEvents::Pair p = plan.step_slot(s);
            HIP_TRY(hipEventElapsedTime(&ms, events[p.from], events[p.to]));
            r->step_ms[s] = ms;
        }
        if (r->solve_ms) {
            const StepEvents::Pair p = plan.solve_slot(s);
            if (p.from >= 0) HIP_TRY(hipEventElapsedTime(&ms, events[p.from], events[p.to]));
            r->solve_ms[s] = p.from >= 0 ? ms : -1.f;
        }
    }
    return MPCCBF_OK;
}

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
    auto g = std::make_shared<LocalGroup>(nranks);
    const int rc = g->create_events();
    if (rc != MPCCBF_OK) return rc;
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
    delete cm;  // (the last communicator of an in-process group: the group and its events with it)
}

int mpccbf_run_steps(mpccbf_ctx* c, const mpccbf_batch* b, mpccbf_run* r, void* stream_) {
    if (!c || !b || !r) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null argument");
    // (before the group's first barrier: a refused rank never joins it)
    if (c->mon.on && r->comm && r->comm->nranks > 1)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "monitor: a communicator of more than one rank is not supported");
    int rc;
    // handshake: from here any return before the last step's barrier aborts the in-process group
    // (the peers get an error)
    GroupSync* group = (r->comm && r->comm->nranks > 1 && r->comm->local) ? &r->comm->local->sync : nullptr;
    GroupAbortGuard guard(group);
    if (group) {
        if ((rc = group_handshake(*group, r->comm->rank, r->num_steps)) != MPCCBF_OK) return rc;
        if (r->num_steps == 0) {
            c->grid.rot.no_rotation();
            if (!group->barrier()) return group_aborted();
            guard.disarm();
            return MPCCBF_OK;
        }
    }
    // validate
    if ((rc = check_run(c, b, r)) != MPCCBF_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(c->device));
    const int first = b->agent_first, count = b->num_agents, ns = b->num_states;
    if ((rc = clear_kernel_clock(c, count, r, stream)) != MPCCBF_OK) return rc;
    // timing
    const StepEvents plan(r->num_steps, r->reserve_steps, r->solve_stride, r->step_ms != nullptr,
                          r->solve_ms != nullptr);
    EventPool& events = c->events;
    if ((rc = start_timing(events, plan, stream)) != MPCCBF_OK) return rc;
    // rotation: only a grid-mode call that runs at least one step leaves one to continue
    const bool gtab = b->nb_row_ptr == nullptr && count > 0 && r->num_steps > 0;
    GridTables& gt = c->grid;
    if (!gtab) gt.rot.no_rotation();
    if (gtab && (rc = start_rotation(gt, b, r->continue_tables != 0, stream)) != MPCCBF_OK) return rc;
    // steps
    double* tables[2] = {const_cast<double*>(b->states), r->states_alt};
    const size_t per_log = (size_t)count * c->p.impc_iter;
    mpccbf_batch sb = *b;
    for (int s = 0; s < r->num_steps; s++) {
        double* cur = tables[s & 1];
        double* nxt = tables[(s & 1) ^ 1];
        sb.states = cur;
        sb.next_states = nxt + (size_t)first * 6;
        sb.step_index = b->step_index + s;
        if (r->status_log) sb.status = r->status_log + (size_t)s * per_log;
        if (r->iters_log) sb.iters = r->iters_log + (size_t)s * per_log;
        if (!r->comm && (rc = carry_over_rows(b, cur, nxt, stream)) != MPCCBF_OK) return rc;
        if ((rc = filter_step(c, b, cur, sb.step_index, stream)) != MPCCBF_OK) return rc;
        const bool tk = plan.times_solve(s);
        rc = impc_enqueue(c, &sb, stream, tk ? events[plan.solve_begin(s)] : nullptr,
                          tk ? events[plan.solve_end(s)] : nullptr, c->dev, c->store, gtab ? s : -1,
                          kernel_clock_of(r, s));
        if (rc != MPCCBF_OK) return rc;
        if ((rc = monitor_after_step(c, &sb, stream)) != MPCCBF_OK) return rc;
        if ((rc = exchange(r->comm, s, nxt, first, count, stream)) != MPCCBF_OK) return rc;
        if (gtab && count < ns && (rc = insert_foreign_rows(gt, s, b, nxt, stream)) != MPCCBF_OK) return rc;
        if (plan.records_end(s)) HIP_TRY(hipEventRecord(events[plan.step_end(s)], stream));
    }
    guard.disarm();  // every barrier of the call passed: the peers no longer wait on this rank
    r->final_table = r->num_steps & 1;
    // where a continuing call picks the rotation up (mpccbf_run::continue_tables)
    if (gtab) gt.rot.run_finished(tables[r->num_steps & 1], r->num_steps);
    return read_timings(events, plan, r);
}

}  // extern "C"
