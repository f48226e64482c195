// capi_control.hip — the C ABI's entry points that hold no context: the CBF-only controllers
// (mpccbf_connectivity_control_solve, mpccbf_formation_rollout, mpccbf_fov_rows_eval,
// mpccbf_fov_control_solve) and the FoV
// particle filter (mpccbf_pf_init, mpccbf_pf_step) and the safety monitor (mpccbf_monitor_reset,
// mpccbf_monitor_score). Each checks its arguments on the host, fills the kernel's argument struct
// and enqueues its launches.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../include/mpccbf.h"
#include "host/formation_args.hpp"
#include "host/fov_estimates.hpp"
#include "host/hip_host.hpp"
#include "kernels/cbf_control.hpp"
#include "kernels/impc.hpp"
#include "kernels/launch_plan.hpp"
#include "kernels/monitor.hpp"
#include "kernels/pf_fov.hpp"

using namespace mpccbf;

// the per-robot QP's parameters with the defaults applied (both connectivity entry points)
static ConnQpParams conn_qp_params(const mpccbf_connectivity_control_params& p) {
    ConnQpParams q;
    std::memset(&q, 0, sizeof(q));
    q.dmin = p.d_min;
    q.dmax = p.d_max;
    for (int d = 0; d < 3; d++) {
        q.vmin[d] = p.v_min[d];
        q.vmax[d] = p.v_max[d];
    }
    q.maxit = p.max_pdip_iters > 0 ? p.max_pdip_iters : 60;
    q.tol = p.tolerance > 0.0 ? p.tolerance : 1e-9;
    q.feas_tol = 1e-6;
    q.slack_mode = p.slack_mode ? 1 : 0;
    q.slack_cost = p.slack_cost;
    q.slack_decay = p.slack_decay_rate;
    return q;
}

extern "C" {

int mpccbf_connectivity_control_solve(const mpccbf_connectivity_control_params* p,
                                      const mpccbf_connectivity_control_batch* b, int32_t device,
                                      void* stream) {
    if (!p || !b) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null argument");
    const std::string perr = conn_control_params_error(*p);
    if (!perr.empty()) return fail(MPCCBF_ERR_INVALID_ARGUMENT, perr);
    if (b->num_teams < 0) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "num_teams < 0");
    if (b->num_teams == 0) return MPCCBF_OK;
    if (!b->team_ptr || !b->states || !b->desired_u || !b->u)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "team_ptr, states, desired_u and u are required");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(MPCCBF_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    ConnControlArgs a;
    std::memset(&a, 0, sizeof(a));
    a.num_teams = b->num_teams;
    a.team_ptr = b->team_ptr;
    a.states = b->states;
    a.desired_u = b->desired_u;
    a.u = b->u;
    a.status = b->status;
    a.obj = b->obj;
    a.iters = b->iters;
    a.lambda2 = b->lambda2;
    a.qp = conn_qp_params(*p);
    HIP_TRY(launch_connectivity_control(a, (hipStream_t)stream));
    return MPCCBF_OK;
}

int mpccbf_formation_rollout(const mpccbf_connectivity_control_params* p, const mpccbf_formation_params* f,
                             const mpccbf_formation_batch* b, int32_t device, void* stream) {
    const std::string err = formation_args_error(p, f, b);
    if (!err.empty()) return fail(MPCCBF_ERR_INVALID_ARGUMENT, err);
    if (b->num_teams == 0 || b->num_steps == 0) return MPCCBF_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(MPCCBF_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    FormationArgs a;
    std::memset(&a, 0, sizeof(a));
    a.num_teams = b->num_teams;
    a.team_ptr = b->team_ptr;
    a.states = b->states;
    a.targets = b->targets;
    a.team_seed = b->team_seed;
    a.trace = b->trace;
    a.cbf_u = b->cbf_u;
    a.desired_u = b->desired_u;
    a.status = b->status;
    a.lambda2 = b->lambda2;
    a.iters = b->iters;
    a.arrival_sample = b->arrival_sample;
    a.first_collision = b->first_collision;
    a.min_d2 = b->min_d2;
    a.fail_count = b->fail_count;
    a.qp = conn_qp_params(*p);
    a.Ts = f->Ts;
    a.spring = f->spring_constant;
    a.pos_std = f->pos_std;
    a.vel_std = f->vel_std;
    a.half_x = f->shape_half[0];
    a.half_y = f->shape_half[1];
    a.goal_radius = f->goal_radius;
    // the steps in launches of at most steps_per_launch on the one stream: each continues from the
    // table and the summary the one before it left
    const int32_t per = formation_steps_per_launch(*f);
    for (int32_t k = 0;; k++) {
        const FormationLaunch l = formation_launch(b->num_steps, per, k);
        if (l.count == 0) break;
        a.step_first = b->step_first + l.first;
        a.record_first = l.first;
        a.num_steps = l.count;
        HIP_TRY(launch_formation_rollout(a, (hipStream_t)stream));
    }
    return MPCCBF_OK;
}

int mpccbf_fov_rows_eval(int32_t count, const double* ego, const double* nb_xy, double fov, double Ds,
                         double Rs, const double* bbox, double* voronoi, double* fov_rows, void* stream) {
    if (count < 0 || (count > 0 && (!ego || !nb_xy))) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "bad arguments");
    if (count == 0) return MPCCBF_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(MPCCBF_ERR_NO_DEVICE, "no HIP device visible");
    const double bbx = bbox ? bbox[0] : 0.0, bby = bbox ? bbox[1] : 0.0;
    HIP_TRY(launch_fov_rows_eval(count, ego, nb_xy, fov, Ds, Rs, bbx, bby, voronoi, fov_rows, (hipStream_t)stream));
    return MPCCBF_OK;
}

int mpccbf_fov_control_solve(const mpccbf_fov_control_params* p, const mpccbf_fov_control_batch* b,
                             int32_t device, void* stream) {
    if (!p || !b) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null argument");
    if (p->slack_mode && !(p->slack_cost > 0.0))
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "Slack cost must be positive when slack_mode is enabled");
    if (p->slack_mode && !(p->slack_decay_rate > 0.0 && p->slack_decay_rate <= 1.0))
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "Slack decay rate must be in (0,1] when slack_mode is enabled");
    if (!(p->fov > 0.0) || !(p->Rs > 0.0))
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "fov and Rs must be positive");
    for (int d = 0; d < 3; d++)
        if (!(p->u_min[d] <= p->u_max[d]) || !(p->v_min[d] <= p->v_max[d]))
            return fail(MPCCBF_ERR_INVALID_ARGUMENT, "bounds: min must not exceed max");
    if (b->num_agents < 0) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "num_agents < 0");
    if (b->num_agents == 0) return MPCCBF_OK;
    if (!b->states || !b->desired_u || !b->nb_row_ptr || !b->u)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "states, desired_u, nb_row_ptr and u are required");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(MPCCBF_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    FovControlArgs a;
    std::memset(&a, 0, sizeof(a));
    a.num_agents = b->num_agents;
    a.states = b->states;
    a.desired_u = b->desired_u;
    a.nb_row_ptr = b->nb_row_ptr;
    a.nb_xy = b->nb_xy;
    a.u = b->u;
    a.status = b->status;
    a.obj = b->obj;
    a.iters = b->iters;
    a.fov = p->fov;
    a.Ds = p->Ds;
    a.Rs = p->Rs;
    for (int d = 0; d < 3; d++) {
        a.vmin[d] = p->v_min[d];
        a.vmax[d] = p->v_max[d];
        a.umin[d] = p->u_min[d];
        a.umax[d] = p->u_max[d];
    }
    a.maxit = p->max_pdip_iters > 0 ? p->max_pdip_iters : 60;
    a.tol = p->tolerance > 0.0 ? p->tolerance : 1e-9;
    a.feas_tol = 1e-6;  // CPLEX's default feasibility tolerance
    for (int i = 0; i < 9; i++) {
        a.P[i] = (i % 4 == 0) ? 2.0 : 0.0;  // ||u - u_des||^2 = 1/2 u^T (2 I) u - 2 u_des^T u + c
        a.LP[i] = (i % 4 == 0) ? std::sqrt(2.0) : 0.0;
    }
    a.slack_mode = p->slack_mode ? 1 : 0;
    a.slack_cost = p->slack_cost;
    a.slack_decay = p->slack_decay_rate;
    a.nb_cov = b->nb_cov;
    HIP_TRY(launch_fov_control(a, (hipStream_t)stream));
    return MPCCBF_OK;
}

static_assert(PF_PARTICLES_MIN == PF_MIN_PARTICLES && PF_PARTICLES_MAX == PF_MAX_PARTICLES,
              "fov_estimates.hpp's particle bounds are the kernels'");

}  // extern "C"

// mpccbf_pf_init / mpccbf_pf_step: every argument check runs on the host before any device call.
// pair_rows > 0 (the filter mpccbf_run_steps drives): rows of the per-pair buffers, pairs beyond
// them are skipped.
int mpccbf::pf_enqueue(const mpccbf_pf_params* p, const mpccbf_pf_batch* b, int32_t device, void* stream, bool init,
                       int32_t pair_rows) {
    if (!p || !b) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "null argument");
    const std::string perr = pf_params_error(*p);
    if (!perr.empty()) return fail(MPCCBF_ERR_INVALID_ARGUMENT, perr);
    if (b->num_states < 0 || b->num_agents < 0 || b->num_pairs < 0 || b->agent_first < 0)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "negative count");
    if ((int64_t)b->agent_first + b->num_agents > b->num_states)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "agent_first + num_agents exceeds num_states");
    if (b->num_pairs == 0 || b->num_agents == 0) return MPCCBF_OK;
    if (!b->states || !b->nb_row_ptr || !b->nb_col || !b->particles || !b->weights || !b->est_xy || !b->est_cov)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT,
                    "states, nb_row_ptr, nb_col, particles, weights, est_xy and est_cov are required");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(MPCCBF_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    PfArgs a;
    std::memset(&a, 0, sizeof(a));
    a.num_particles = p->num_particles;
    a.num_states = b->num_states;
    a.states = b->states;
    a.agent_first = b->agent_first;
    a.num_agents = b->num_agents;
    a.nb_row_ptr = b->nb_row_ptr;
    a.nb_col = b->nb_col;
    a.num_pairs = b->num_pairs;
    a.input = b->input;
    a.init_xy = b->init_xy;
    a.particles = b->particles;
    a.weights = b->weights;
    a.est_xy = b->est_xy;
    a.est_cov = b->est_cov;
    a.flags = b->flags;
    a.ancestors = b->ancestors;
    a.step_index = b->step_index;
    a.seed = p->seed;
    for (int i = 0; i < 3; i++) a.init_cov[i] = p->init_cov[i];
    // Eigen::LLT of init_cov (particle_filter.cpp:38-39)
    a.init_chol[0] = std::sqrt(p->init_cov[0]);
    a.init_chol[1] = p->init_cov[1] / a.init_chol[0];
    a.init_chol[2] = std::sqrt(p->init_cov[2] - a.init_chol[1] * a.init_chol[1]);
    for (int i = 0; i < 4; i++) a.process[i] = p->process[i];
    // cov.inverse() of the measurement covariance (particle_filter.cpp:96)
    const double det = p->meas_cov[0] * p->meas_cov[2] - p->meas_cov[1] * p->meas_cov[1];
    a.meas_inv[0] = p->meas_cov[2] / det;
    a.meas_inv[1] = -p->meas_cov[1] / det;
    a.meas_inv[2] = p->meas_cov[0] / det;
    a.dt = p->dt;
    a.fov = p->fov;
    a.Rs = p->Rs;
    a.weight_reduction = p->weight_reduction;
    a.pair_rows = pair_rows;
    HIP_TRY(init ? launch_pf_init(a, (hipStream_t)stream) : launch_pf_step(a, (hipStream_t)stream));
    return MPCCBF_OK;
}

extern "C" {

int mpccbf_pf_init(const mpccbf_pf_params* p, const mpccbf_pf_batch* b, int32_t device, void* stream) {
    return pf_enqueue(p, b, device, stream, true, 0);
}

int mpccbf_pf_step(const mpccbf_pf_params* p, const mpccbf_pf_batch* b, int32_t device, void* stream) {
    return pf_enqueue(p, b, device, stream, false, 0);
}

}  // extern "C"

// ---- safety monitor ------------------------------------------------------------------------------

// The monitor's own fields (what mpccbf_set_monitor, mpccbf_monitor_reset and mpccbf_monitor_score
// all refuse): empty when they are good. watch: the watch radius with its default applied.
static std::string monitor_error(const mpccbf_monitor* m, double* watch) {
    if (!m) return "monitor: null monitor";
    if (m->shape_type != 0 && m->shape_type != 1) return "monitor: shape_type must be 0 (circle) or 1 (box)";
    if (!(m->shape[0] > 0.0) || !std::isfinite(m->shape[0]))
        return "monitor: the shape's radius / half extent must be positive and finite";
    if (m->shape_type == 1 && (!(m->shape[1] > 0.0) || !std::isfinite(m->shape[1])))
        return "monitor: the box's half extents must be positive and finite";
    if (!(m->d_min > 0.0) || !std::isfinite(m->d_min)) return "monitor: d_min must be positive and finite";
    if (!(m->goal_radius >= 0.0) || !std::isfinite(m->goal_radius)) return "monitor: goal_radius must be >= 0 and finite";
    const double w = m->watch_radius == 0.0 ? 3.0 * m->d_min : m->watch_radius;
    // the largest centre distance at which the shape test can hold (box: offsets below 2 half on both
    // axes, with room for the roundings of the script's corner arithmetic)
    const double reach = m->shape_type == 1 ? 2.0 * std::hypot(m->shape[0], m->shape[1]) * (1.0 + 0x1p-20) : 2.0 * m->shape[0];
    if (!std::isfinite(w) || !(w >= m->d_min) || !(w >= reach))
        return "monitor: watch_radius must cover d_min and the shape's reach";
    if (m->rows < 1) return "monitor: rows must be >= 1";
    if (!m->summary || !m->reached_at || !m->min_d2 || !m->hit_samples || !m->unsafe_samples)
        return "monitor: summary, reached_at, min_d2, hit_samples and unsafe_samples are required";
    if (!m->scratch) return "monitor: scratch is required";
    if (m->sample_log_rows < 0 || (m->sample_log && m->sample_log_rows == 0))
        return "monitor: a sample log needs sample_log_rows >= 1";
    *watch = w;
    return "";
}

static void monitor_outputs(const mpccbf_monitor* m, MonitorArgs& a) {
    a.summary = (unsigned long long*)m->summary;
    a.reached_at = (unsigned long long*)m->reached_at;
    a.min_d2 = (unsigned long long*)m->min_d2;
    a.hit_samples = (uint32_t*)m->hit_samples;
    a.unsafe_samples = (uint32_t*)m->unsafe_samples;
    a.sample_log = (unsigned long long*)m->sample_log;
    a.sample_log_rows = m->sample_log ? m->sample_log_rows : 0;
}

std::string mpccbf::monitor_attach_error(const mpccbf_monitor* m) {
    double w;
    return monitor_error(m, &w);
}

int mpccbf::monitor_enqueue(const mpccbf_monitor* m, const double* samples, int32_t num_samples, int64_t sample_stride,
                            int64_t row_stride, int32_t agent_first, int32_t num_agents, const double* fixed_states,
                            int32_t num_states, const double* goals, int64_t sample_first, int32_t device,
                            void* stream) {
    double watch = 0.0;
    const std::string merr = monitor_error(m, &watch);
    if (!merr.empty()) return fail(MPCCBF_ERR_INVALID_ARGUMENT, merr);
    if (num_samples < 0 || num_states < 0 || num_agents < 0 || agent_first < 0)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "monitor: negative count");
    if ((int64_t)agent_first + num_agents > num_states)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "monitor: agent_first + num_agents exceeds num_states");
    if (num_states > MONITOR_MAX_ROWS) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "monitor: num_states > 2^20");
    if (num_states > m->rows)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "monitor: rows (" + std::to_string(m->rows) + ") < num_states (" +
                                                     std::to_string(num_states) + ")");
    if (sample_first < -1) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "monitor: sample_first < -1");
    if (sample_first >= 0 && sample_first + (int64_t)num_samples > MONITOR_MAX_SAMPLES)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT, "monitor: sample_first + num_samples > 2^23");
    if (num_samples == 0 || num_states == 0) return MPCCBF_OK;
    if (monitor_scratch_bytes(num_states, num_samples) > m->scratch_bytes)
        return fail(MPCCBF_ERR_INVALID_ARGUMENT,
                    "monitor: scratch_bytes (" + std::to_string(m->scratch_bytes) + ") < " +
                        std::to_string(monitor_scratch_bytes(num_states, num_samples)) + " for " +
                        std::to_string(num_states) + " rows x " + std::to_string(num_samples) + " samples");
    if (num_agents > 0 && !samples) return fail(MPCCBF_ERR_INVALID_ARGUMENT, "monitor: samples is required");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(MPCCBF_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    MonitorArgs a;
    std::memset(&a, 0, sizeof(a));
    a.samples = samples;
    a.num_samples = num_samples;
    a.sample_stride = sample_stride;
    a.row_stride = row_stride;
    a.agent_first = agent_first;
    a.num_agents = num_agents;
    a.fixed = fixed_states;
    a.num_states = num_states;
    a.goals = goals;
    a.sample_first = sample_first;
    a.box = m->shape_type == 1;
    a.half_x = m->shape[0];
    a.half_y = m->shape[1];
    a.dmin2 = m->d_min * m->d_min;
    const double gr = m->goal_radius == 0.0 ? 1.0 : m->goal_radius;
    a.goal2 = gr * gr;
    a.watch2 = watch * watch;
    a.inv_cell = grid_inv_cell(watch);
    a.mask = monitor_table_size(num_states) - 1u;
    monitor_outputs(m, a);
    monitor_carve(m->scratch, num_states, num_samples, a);
    HIP_TRY(launch_monitor_score(a, (hipStream_t)stream));
    return MPCCBF_OK;
}

extern "C" {

size_t mpccbf_monitor_scratch_bytes(int32_t rows, int32_t max_samples) {
    if (rows < 0 || rows > MONITOR_MAX_ROWS || max_samples < 0) return 0;
    return monitor_scratch_bytes(rows, max_samples);
}

uint32_t mpccbf_monitor_table_size(int32_t num_rows) {
    return monitor_table_size(num_rows < 0 ? 0 : (num_rows > MONITOR_MAX_ROWS ? MONITOR_MAX_ROWS : num_rows));
}

int mpccbf_monitor_reset(const mpccbf_monitor* m, int32_t device, void* stream) {
    double watch = 0.0;
    const std::string merr = monitor_error(m, &watch);
    if (!merr.empty()) return fail(MPCCBF_ERR_INVALID_ARGUMENT, merr);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(MPCCBF_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    MonitorArgs a;
    std::memset(&a, 0, sizeof(a));
    monitor_outputs(m, a);
    HIP_TRY(launch_monitor_reset(a, m->rows, (hipStream_t)stream));
    return MPCCBF_OK;
}

int mpccbf_monitor_score(const mpccbf_monitor* m, const double* samples, int32_t num_samples, int64_t sample_stride,
                         int64_t row_stride, int32_t agent_first, int32_t num_agents, const double* fixed_states,
                         int32_t num_states, const double* goals, int64_t sample_first, int32_t device,
                         void* stream) {
    return monitor_enqueue(m, samples, num_samples, sample_stride, row_stride, agent_first, num_agents, fixed_states,
                           num_states, goals, sample_first, device, stream);
}

}  // extern "C"
