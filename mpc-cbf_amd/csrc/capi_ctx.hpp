// capi_ctx.hpp — what the two translation units of the context's C ABI share: the context itself
// with the owners of what it carries from call to call, and the steps of one IMPC launch that the
// run loop calls. capi.hip: context lifetime, setters, single launches, and the definitions of the
// functions declared here; capi_run.hip: the communicators and mpccbf_run_steps. Private to csrc/.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mpccbf.h"
#include "host/defer_queues.hpp"
#include "host/grid_rotation.hpp"
#include "host/hip_host.hpp"
#include "host/operators.hpp"
#include "kernels/impc.hpp"
#include "kernels/launch_plan.hpp"

namespace mpccbf {

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

// The timing events of mpccbf_run_steps (step_events.hpp says which is which): created on demand,
// outside the steps, and destroyed with the context.
struct EventPool {
    std::vector<hipEvent_t> ev;
    EventPool() = default;
    EventPool(const EventPool&) = delete;
    EventPool& operator=(const EventPool&) = delete;
    ~EventPool() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    // at least `need` events
    int ensure(int need) {
        while ((int)ev.size() < need) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            ev.push_back(e);
        }
        return MPCCBF_OK;
    }
    hipEvent_t operator[](int i) const { return ev[i]; }
};

}  // namespace mpccbf

struct mpccbf_ctx {
    mpccbf::EventPool events;     // timing events of mpccbf_run_steps
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
    // team rollouts (mpccbf_team_rollout): the all-others lists of every team size (team_lists,
    // uploaded at the first call) and, for calls that do not record the sub-steps, one step's rows
    mpccbf::DevBuf team_lists, team_work;
};

namespace mpccbf {

// The launch plan of the context's next IMPC step for n agents (launch_plan.hpp)
inline LaunchPlan ctx_plan(const mpccbf_ctx* c, int n, bool csr, int knn_k, bool store) {
    LaunchFacts f{};
    f.est = c->est.on;
    return impc_launch_plan(c->dev, c->variant, n, csr, knn_k, store, c->conn.on, f);
}

// ---- argument checks that more than one entry point makes ---------------------------------------
int check_agent_range(const mpccbf_batch* b);
// what a batch whose neighbours come from the grid must give
int check_grid_query(const mpccbf_batch* b);

// One IMPC step for a batch, enqueued on `stream`; ev0 / ev1 (optional) are recorded around the
// IMPC kernel alone. run_step >= 0: step run_step of the grid-mode mpccbf_run_steps call that
// started the rotation (GridRotation::step); < 0: a step outside a rotation (foreign_step).
// ops / store: the context's (c->dev, c->store), or what the cap audit puts in their place.
int impc_enqueue(mpccbf_ctx* c, const mpccbf_batch* b, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1,
                 const DevOps& ops, int32_t* store, int run_step = -1, unsigned long long* kclock = nullptr);

// What the attached monitor refuses of a batch, ahead of the step's launches
int monitor_step_check(const mpccbf_ctx* c, const mpccbf_batch* b);
// The attached monitor's score of the step `b` just enqueued, behind its IMPC launch on the same
// stream: the step's sub-step records when the batch gives them, else its one next-state sample.
// The rows outside the agent range are those of the table the step read. The IMPC launch itself is
// untouched (nothing here is an argument of it).
int monitor_after_step(mpccbf_ctx* c, const mpccbf_batch* b, hipStream_t stream);

}  // namespace mpccbf
