// capi_rollout.hip — mpccbf_team_rollout: the MPC-CBF example's closed loop for a batch of teams with
// the context's operators. The argument and context rules are team_rollout_args.hpp's (host only);
// this file fills the kernel's arguments and enqueues the launches (kernels/team_rollout.hip).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "capi_ctx.hpp"
#include "host/team_rollout_args.hpp"
#include "kernels/team_rollout.hpp"

using namespace mpccbf;

static_assert(TEAM_ROLLOUT_MAX == TEAM_MAX, "one team size limit on the host and on the device");

extern "C" {

int mpccbf_team_rollout(mpccbf_ctx* c, const mpccbf_team_rollout_params* p, const mpccbf_team_batch* b,
                        void* stream) {
    if (!c) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "team rollout: null argument");
    TeamRolloutContext tc{};
    tc.cbf_mode = c->dev.cbf_mode;
    tc.slack_mode = c->dev.slack_mode;
    tc.nz = c->dev.nz;
    tc.m = c->dev.m;
    tc.cbf_horizon = c->dev.cbf_h;
    tc.nsub = c->dev.nsub;
    tc.connectivity = c->conn.on ? 1 : 0;
    tc.ranks = 1;  // (a context holds no communicator: mpccbf_run_steps alone takes one)
    std::string err = team_rollout_context_error(tc);
    if (err.empty()) err = team_rollout_args_error(p, b, c->dev.nsub);
    if (!err.empty()) return fail(MPCCBF_ERR_INVALID_ARGUMENT, err);
    if (b->num_teams == 0 || b->num_steps == 0) return MPCCBF_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (c->team_lists.bytes == 0) {
        std::vector<int32_t> lists(TEAM_ROWS + TEAM_COLS);
        team_lists(lists.data(), lists.data() + TEAM_ROWS);
        HIP_TRY(c->team_lists.reserve(lists.size() * sizeof(int32_t)));
        const hipError_t e = hipMemcpy(c->team_lists.p, lists.data(), lists.size() * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            c->team_lists.release();
            return fail(MPCCBF_ERR_HIP, std::string("team rollout: list upload: ") + hipGetErrorString(e));
        }
    }
    if (!b->substeps)
        HIP_TRY(c->team_work.reserve((size_t)b->num_teams * TEAM_MAX * c->dev.nsub * 6 * sizeof(double)));
    TeamRolloutArgs a;
    std::memset(&a, 0, sizeof(a));
    a.num_teams = b->num_teams;
    a.team_ptr = b->team_ptr;
    a.targets = b->targets;
    a.team_seed = b->team_seed;
    a.states = b->states;
    a.x_keep = b->x_keep;
    a.traj_t = b->traj_t;
    a.status = b->status;
    a.obj = b->obj;
    a.iters = b->iters;
    a.x = b->x;
    a.traj_t0 = b->traj_t0;
    a.substeps = b->substeps;
    a.trace = b->trace;
    a.work = b->substeps ? nullptr : c->team_work.as<double>();
    a.arrival_sample = b->arrival_sample;
    a.first_collision = b->first_collision;
    a.min_d2 = b->min_d2;
    a.fail_count = b->fail_count;
    a.nb_row = c->team_lists.as<int32_t>();
    a.nb_col = c->team_lists.as<int32_t>() + TEAM_ROWS;
    a.pos_std = p->pos_std;
    a.vel_std = p->vel_std;
    a.half_x = p->shape_half[0];
    a.half_y = p->shape_half[1];
    a.goal_radius = p->goal_radius;
    // the steps in launches of at most steps_per_launch on the one stream: each continues from the
    // tables, the kept curves and the summary the one before it left
    const int32_t per = team_steps_per_launch(*p);
    for (int32_t k = 0;; k++) {
        const TeamLaunch l = team_launch(b->num_steps, per, k);
        if (l.count == 0) break;
        a.step_first = b->step_first + l.first;
        a.record_first = l.first;
        a.num_steps = l.count;
        HIP_TRY(launch_team_rollout(c->dev, c->dbuf.as<double>(), a, (hipStream_t)stream));
    }
    return MPCCBF_OK;
}

}  // extern "C"
