/*
 * mpccbf.h — C ABI of the MI355X-native batched MPC-CBF QP solver (libmpccbf.so).
 *
 * This is the drop-in boundary that replaces the CPLEX call of the reference hot path:
 *
 *   qpcpp::Solver<double>::solve(Problem&)          workspace/lib/qpcpp/include/qpcpp/solvers/Solver.h:27-37
 *   qpcpp::CPLEXSolver<double>::solve(Problem&)     workspace/lib/qpcpp/src/solvers/CPLEX.cpp:35-177
 *   called from ConnectivityIMPCCBF::optimize        workspace/lib/mpc_cbf/src/controller/ConnectivityIMPCCBF.cpp:199-211
 *
 * Two entry families:
 *   (1) mpccbf_qp_solve_dense*: one generic dense QP in the flattened CPLEX form (what
 *       CPLEXSolver::solve builds from a qpcpp::Problem, CPLEX.cpp:52-147). The C++ adapter
 *       qpcpp::HIPSolver<double> (mpc-cbf_amd/csrc/qpcpp/) flattens a Problem into this.
 *   (2) mpccbf_create / mpccbf_impc_solve: the structured, batched path. The parameter-only
 *       operators of the MPC-CBF QP (PiecewiseBezierMPCQPOperations ctor, :9-38) are built once
 *       per context; each call runs ConnectivityIMPCCBF::optimize (ConnectivityIMPCCBF.cpp:47-215)
 *       for a whole batch of agents on the GPU: both IMPC iterations, the closed-form safety-CBF
 *       rows (ConnectivityCBF.cpp:152-198, in place of GiNaC substitution), and the QP solves.
 *
 * Conventions
 *   - All numbers are FP64 (the reference instantiates <double, 3U>).
 *   - A state is 6 doubles [px, py, yaw, vx, vy, vyaw] (model::State, DIM = 3).
 *   - Infinite bounds: any value <= -1e300 / >= 1e300 (numeric_limits<double>::lowest()/max()
 *     as used by qpcpp::Problem, Problem.h:366-372).
 *   - Solve statuses are qpcpp::SolveStatus indices (Solver.h:13-21): MPCCBF_OPTIMAL == 0 ...
 *   - Functions return MPCCBF_OK (0) or a negative error code; they never throw. The last
 *     error message of the calling thread is available from mpccbf_last_error().
 *   - Pointers in mpccbf_batch are DEVICE pointers; work is enqueued on the given hipStream_t
 *     (passed as void*; NULL = default stream) and is asynchronous. The dense-QP functions take
 *     HOST pointers and are synchronous.
 *   - One context per host thread/stream (contexts hold device buffers; not thread-safe).
 */
#ifndef MPCCBF_H
#define MPCCBF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCCBF_ABI_VERSION 12

/* qpcpp::SolveStatus (Solver.h:13-21) */
enum {
    MPCCBF_OPTIMAL = 0,
    MPCCBF_FEASIBLE = 1,
    MPCCBF_UNBOUNDED = 2,
    MPCCBF_INFEASIBLE = 3,
    MPCCBF_ERROR = 4,
    MPCCBF_UNKNOWN = 5, /* also: IMPC iteration not attempted (reference `break`, :208-211) */
    MPCCBF_INFEASIBLEORUNBOUNDED = 6
};

/* API return codes */
enum {
    MPCCBF_OK = 0,
    MPCCBF_ERR_INVALID_ARGUMENT = -1, /* std::invalid_argument / runtime_error in the reference */
    MPCCBF_ERR_HIP = -2,
    MPCCBF_ERR_CAPACITY = -3,
    MPCCBF_ERR_NO_DEVICE = -4,
    MPCCBF_ERR_INTERNAL = -5
};

/* Parameters: the JSON keys of experiments/config/base_config.json as parsed and validated by
 * common/include/common/parsing.hpp:20-214 (mpc_params, physical_limits, cbf_params, bezier_params). */
typedef struct mpccbf_params {
    double h, Ts;
    int32_t k_hor;
    double w_pos_err, w_u_eff;
    int32_t spd_f;
    double v_min[3], v_max[3], a_min[3], a_max[3];
    double d_min;
    int32_t cbf_horizon, impc_iter, slack_mode;
    double slack_cost, slack_decay_rate;
    int32_t num_pieces, num_control_points;
    double piece_max_parameter;
    int32_t continuity_upto_degree;
    /* controller family: 0 = ConnectivityIMPCCBF (collision CBF against neighbour states,
     * continuity d <= degree), 1 = FovBezierIMPCCBF (FoV CBFs against neighbour positions +
     * Voronoi rows on piece 0, continuity d < degree; FovBezierIMPCCBF.cpp:44-223) */
    int32_t cbf_mode;
    double fov_beta;  /* field of view (rad); FovCBF(fov, Ds, Rs, ...) (FovCBF.cpp:41-52) */
    double fov_Ds;    /* safety distance (the FoV example passes aligned_box[0]) */
    double fov_Rs;    /* sensing range (fov_cbf_params.Rs) */
    double bbox[3];   /* robot aligned-box half extents (Voronoi shift, math/src/Helpers.cpp:20-36) */
} mpccbf_params;

typedef struct mpccbf_ctx mpccbf_ctx;

/* Context options (all optional; zero-initialise for defaults). */
typedef struct mpccbf_options {
    int32_t device;            /* HIP device ordinal (default 0) */
    int32_t keep_redundant;    /* 1: keep every box row (no exact host-side redundancy removal) */
    int32_t no_cbf_filter;     /* 1: keep every CBF row (no exact in-kernel redundancy filter) */
    int32_t max_pdip_iters;    /* default 60 */
    double tolerance;          /* PDIP relative tolerance, default 1e-9 */
    /* Interior-point warm start of IMPC iteration 1 — used only when the dual active-set solve
     * is off (dual_as_steps < 0; by default the active set solves first and the PDIP runs cold):
     * iteration 0's primal-dual point, slacks and duals floored at warm_delta: 0 = default
     * (0.3), < 0 = cold start. A warm start that does not converge is certified by phase 1 and,
     * when the QP is feasible, re-solved cold, so statuses do not depend on it. */
    double warm_delta;
    /* Solver pipeline (ABI 10). Zero selects the default; these are the only inputs that change
     * the solver's path (no environment variable does, except in the diagnostics build). */
    int32_t dual_as_steps;     /* dual active-set step limit per QP: 0 = 24, < 0 = off (the PDIP alone) */
    int32_t no_fast_start;     /* 1: no unconstrained-minimiser fast start in the PDIP path */
    int32_t early_it;          /* PDIP divergence test from this iteration on: 0 = 10, < 0 = off */
    int32_t das_warm_steps;    /* IMPC iteration 1 starts the active set from iteration 0's when that
                                  took at least this many steps: 0 = 3, < 0 = never */
    int32_t lean;              /* 1: lean main launch (fast start + active set; the rest deferred to
                                  the fallback launch). Collision controller only */
} mpccbf_options;

/* Validates p like parsing.hpp:37-135,182-214, builds the parameter-only operators on the host
 * and uploads them. Returns MPCCBF_ERR_INVALID_ARGUMENT with the reference's message on bad
 * parameters. */
int mpccbf_create(const mpccbf_params* p, const mpccbf_options* opt, mpccbf_ctx** out);
void mpccbf_destroy(mpccbf_ctx* ctx);

/* Sizes: n = num_pieces * 3 * num_control_points decision variables (curve control points,
 * layout [piece][dim][control point], BezierQPOperations.cpp:180-204); nz = free dimension
 * after the equality constraints; rows = shared inequality rows kept after exact reduction. */
int mpccbf_num_vars(const mpccbf_ctx* ctx);
int mpccbf_reduced_dim(const mpccbf_ctx* ctx);
int mpccbf_num_shared_rows(const mpccbf_ctx* ctx);

/* One IMPC control step for a batch of agents (ConnectivityIMPCCBF::optimize per agent).
 * Inputs (device):
 *   states      num_states x 6, every agent visible to this batch (local + gathered)
 *   agent_first the batch solves agents [agent_first, agent_first + num_agents) of `states`
 *   targets     num_agents x 3: reference position replicated over the horizon
 *               (MPCCBFFormationControl_example.cpp:143-144); or NULL and give `refs`
 *   refs        num_agents x 3*k_hor full reference trajectory (ref_positions); or NULL
 *   nb_row_ptr  num_agents + 1 CSR offsets (nb_row_ptr[0] may be nonzero)
 *   nb_col      neighbour indices into `states` (the reference uses all N-1 others, :59-67)
 *   knn_k, knn_radius   used when nb_row_ptr is NULL: the neighbours of each agent are its
 *               knn_k nearest others (planar) within knn_radius, found on the device in the same
 *               launch sequence (spatial hash of `states` + in-kernel 3x3-cell query; in
 *               mpccbf_run_steps the IMPC kernel itself fills the next step's hash table);
 *               knn_k <= 16; any number of agents within the radius (beyond 64 candidates the
 *               query streams them through a running k-nearest set).
 *               The contract of every query (and of mpccbf_build_neighbors): j != self; squared
 *               distance dx*dx + dy*dy <= knn_radius^2 as computed in double (inclusive); the
 *               knn_k nearest, ties broken by the smaller agent index; the list sorted by index.
 *               The hash cells have edge knn_radius * (1 + 2^-20), so that the rounding of the
 *               cell coordinates never hides a neighbour within the radius from the 3x3-cell
 *               query: guaranteed for |x|, |y| <= 2^30 * knn_radius (derivation at grid_inv_cell,
 *               kernels/impc.hpp).
 *               Capacity: the default separable kernel keeps up to 16 live (unfiltered) CBF rows
 *               per IMPC iteration and agent (slack mode: 16 neighbours); an agent beyond it is
 *               re-solved in the same call by the fallback launch of the same separable solver
 *               with 8 CBF row slots per lane (128 rows; slack mode: the neighbours with a live
 *               row compacted into the 16 lanes); beyond that its QPs report ERROR (the agent's
 *               earlier iterations and every other agent are unaffected). The dense layouts have
 *               no capacity launch: with m shared box rows the 16-lane one holds 64 - m CBF rows
 *               per agent and the 64-lane one 256 - m. The default variant takes the 16-lane one
 *               only when no agent can exceed its slots (grid lists with knn_k x cbf_horizon <=
 *               64 - m), else the 64-lane one; a dense layout forced by mpccbf_set_variant (1: 64
 *               lanes x 1 slot, 3: 16 lanes x 4 slots) reports ERROR beyond 64 - m rows. A QP whose
 *               data is not finite (NaN / Inf state, target or neighbour state) reports ERROR
 *               slack_mode requires cbf_horizon <= 2 (a neighbour's lane holds its rows of two
 *               samples): with the collision controller a solve beyond it launches nothing and
 *               returns MPCCBF_ERR_CAPACITY; with the FoV controller mpccbf_create refuses the
 *               parameters (MPCCBF_ERR_INVALID_ARGUMENT)
 * Outputs (device, any may be NULL):
 *   x           num_agents x n: control points of the last OPTIMAL iteration (the curve the
 *               driver keeps, example :160-164); NaN if no iteration was OPTIMAL
 *   status      num_agents x impc_iter SolveStatus per IMPC iteration (UNKNOWN = not attempted)
 *   obj         num_agents x impc_iter optimal objective x^T H x + c^T x (CPLEX.cpp:144-146)
 *   iters       num_agents x impc_iter solver steps of that QP: dual active-set steps plus the
 *               interior-point Newton steps of every PDIP attempt (when the active-set solve
 *               gives up, or in slack mode); 0 when the unconstrained minimiser satisfies every
 *               row; phase-1 steps not included
 *   primal_res, dual_res  num_agents x impc_iter: OPTIMAL — scaled primal residual
 *               max_i |r_i| / (1 + |bound_i|) over the condensed QP's rows (bounds every row's
 *               violation) and relative dual residual ||P y + q + G^T z||_inf / (1 + ||q||_inf)
 *               of the returned point; INFEASIBLE certified by phase 1 — the minimal uniform row
 *               violation t* (absolute, > 1e-6) and NaN; otherwise NaN
 *   next_states num_agents x 6: position/velocity of the kept curve at t = h (Jacobi update of
 *               the closed-loop driver, example :188-207, without noise); unchanged input if no
 *               curve was found.
 *   stamps      diagnostics, normally NULL: num_agents x 8 int64 wall-clock stamps (s_memrealtime)
 *               at the kernel's phase boundaries (start, setup, neighbours, CBF rows 0, solve 0,
 *               CBF rows 1, solve 1, end) — written by the diagnostics builds only (make stamps /
 *               prof); the release library compiles the stamp code out and ignores the pointer.
 *   nb_out      diagnostics, normally NULL (ABI 10): num_agents x 16 int32, the neighbour list each
 *               agent's QPs were built from, in the kernel's order (grid mode: the in-kernel query's
 *               k nearest, sorted by index; CSR: the given list), -1 after the last; lists longer
 *               than 16 are truncated here (not in the solve). Written by the release kernels of
 *               every layout; in grid mode it is the list input of mpccbf_cap_audit_run. */
typedef struct mpccbf_batch {
    int32_t num_states;
    const double* states;
    int32_t agent_first;
    int32_t num_agents;
    const double* targets;
    const double* refs;
    const int32_t* nb_row_ptr;
    const int32_t* nb_col;
    double* x;
    int32_t* status;
    double* obj;
    int32_t* iters;
    double* next_states;
    int32_t knn_k;
    double knn_radius;
    int64_t* stamps;
    /* Closed-loop simulator semantics (MPCCBFFormationControl_example.cpp:150-221), optional.
     * traj_t != NULL (device, num_agents): x is the persistent trajectory store — an agent whose
     * optimize() yields a curve (trajs non-empty) gets it written to x and traj_t = 0; one
     * without keeps its previous x; the next state is that curve (position, velocity) at
     * t = min(traj_t + Ts * int(h / Ts), max parameter), which becomes the new traj_t. With no
     * curve yet (traj_t < 0; initialise to -1) the agent holds its position at zero velocity.
     * traj_t == NULL: next state = this step's curve at t = h, or the current state if none. */
    double* traj_t;
    double pos_std, vel_std;  /* Gaussian noise added to the next state's position / velocity
                                 (math::addRandomNoise, Random.cpp:7-28) at each of the int(h / Ts)
                                 control sub-steps: with a curve only the last draw remains (each
                                 sub-step re-evaluates the curve); holding position (no curve yet)
                                 the position draws accumulate; 0 = off */
    uint64_t noise_seed;      /* counter-based: noise(seed, step_index, agent, component) */
    int64_t step_index;       /* mpccbf_run_steps adds the step number */
    /* FoV controller in slack mode (FovBezierIMPCCBF::optimize's other_robot_covs,
     * FovBezierIMPCCBF.cpp:48-81): device, num_states x 3 = (cxx, cxy, cyy), the position block
     * of each agent's estimate covariance as its observers hold it; orders the neighbours by
     * distanceToEllipse for the slack weights. NULL = unknown (infinite: every distance is -5,
     * weights follow the neighbour list order). Ignored otherwise. */
    const double* cov;
    double* primal_res;       /* out, num_agents x impc_iter, or NULL (see above) */
    double* dual_res;
    /* Closed-loop records (needs traj_t): device, num_agents x int(h / Ts) x 6, the state after
     * each control sub-step of this step as the example appends them to states.json
     * (MPCCBFFormationControl_example.cpp:188-221): the kept curve at traj_t + Ts k (clamped) plus
     * noise, or, with no curve yet, the held position with the noise accumulated over the
     * sub-steps and a zero velocity plus noise. The last record is the next state. NULL: none. */
    double* substeps;
    int32_t* nb_out;          /* out, num_agents x 16, or NULL (see above) */
} mpccbf_batch;

int mpccbf_impc_solve(mpccbf_ctx* ctx, const mpccbf_batch* batch, void* hip_stream);

/* ---- Closed-loop stepping (the MPCCBFFormationControl_example.cpp:131-231 loop: every agent
 * re-plans from the states the previous step produced — a Jacobi sweep, where the reference
 * updates robots one after another — with the batch's fallback / noise semantics) ------------
 *
 * mpccbf_run_steps enqueues num_steps control steps back to back on the stream. Step s reads
 * table T_s (T_0 = batch->states, then alternating with run->states_alt; both num_states x 6,
 * device) and writes the next states of agents [agent_first, agent_first + num_agents) into
 * T_{s+1}. Rows of other agents are carried over (copy), or, with a communicator, filled by one
 * in-place RCCL all-gather of every rank's block (ranks own equal contiguous blocks:
 * agent_first = rank * num_agents, num_states = nranks * num_agents). batch->next_states is
 * ignored; batch->status / iters receive the last step unless per-step logs are given.
 * When step_ms or solve_ms is given the call waits for the GPU and fills them (host arrays,
 * num_steps entries: device time of each step, and of its IMPC kernel alone). */
typedef struct mpccbf_comm mpccbf_comm;
#define MPCCBF_COMM_ID_BYTES 128
int mpccbf_comm_unique_id(char id_out[MPCCBF_COMM_ID_BYTES]);  /* on one rank; share the bytes */
int mpccbf_comm_create(const char id[MPCCBF_COMM_ID_BYTES], int32_t nranks, int32_t rank,
                       int32_t device, mpccbf_comm** out);     /* collective over the nranks */
void mpccbf_comm_destroy(mpccbf_comm* comm);
/* In-process group of nranks communicators (comms_out[r] for rank r) on one device: the ranks are
 * host threads of this process, each running mpccbf_run_steps on its own stream with its own
 * context and state tables; the per-step all-gather becomes device copies between those tables
 * (one event per rank and step, a host barrier per step). The multi-GPU data flow on one GPU —
 * for testing and for running several shards on one device. */
int mpccbf_comm_create_local(int32_t nranks, int32_t device, mpccbf_comm** comms_out);

typedef struct mpccbf_run {
    int32_t num_steps;
    double* states_alt;     /* second state table (device) */
    int32_t* status_log;    /* num_steps x num_agents x impc_iter (device), or NULL */
    int32_t* iters_log;     /* likewise, or NULL */
    float* step_ms;         /* host, num_steps, or NULL */
    float* solve_ms;        /* host, num_steps, or NULL */
    mpccbf_comm* comm;      /* NULL: single process */
    int32_t reserve_steps;  /* keep timing events for this many steps (avoids creating them later) */
    int32_t solve_stride;   /* time the IMPC kernel on every solve_stride-th step only (<= 1: all);
                               solve_ms of untimed steps is set to -1 */
    int32_t final_table;    /* out: 0 = batch->states holds the final states, 1 = states_alt */
    /* ABI 11: device clock of every step's IMPC launch, or NULL: num_steps x kernel_clock_waves x 2
     * uint64 (device, zero-filled by the call). Wave w of step s's launch writes the pair [s][w] =
     * (the s_memrealtime counter, 100 MHz, when the wave started, when it finished) with plain
     * stores; waves without an agent write nothing. The launch's own duration is the largest end
     * minus the smallest start over the nonzero pairs, without the dispatch gaps that events around
     * it include. kernel_clock_waves >= mpccbf_impc_launch_waves(ctx, num_agents); the collision
     * kernels only (the FoV kernels write nothing). */
    uint64_t* kernel_clock;
    int32_t kernel_clock_waves;
    /* ABI 12: 1 = this call continues the context's previous mpccbf_run_steps call: batch->states
     * is that call's final table, unchanged since, with the same agent range and neighbour
     * query (knn_k, knn_radius). Its first step then reads the neighbour table the previous call's
     * last step filled, instead of rebuilding table 0 (two memsets and an insert launch per call).
     * That table holds copies of the states, so the rule is: only a grid-mode (nb_row_ptr NULL)
     * mpccbf_run_steps call that ran at least one step leaves a rotation to continue. After any
     * other call on the context (mpccbf_impc_solve in grid or CSR mode, mpccbf_run_steps with CSR
     * lists, zero steps or zero agents) the next call rebuilds, and so does a call whose pointer,
     * num_states, agent range or query differs from the previous call's. A caller that itself
     * overwrites the final table between two grid-mode calls and still asks to continue is
     * outside this contract (the library cannot see the write): pass 0. 0: always rebuild. */
    int32_t continue_tables;
} mpccbf_run;

int mpccbf_run_steps(mpccbf_ctx* ctx, const mpccbf_batch* batch, mpccbf_run* run, void* hip_stream);

/* Tuning knob: kernel layout for mpccbf_impc_solve. 0 (default): share-adaptive — the separable
 * collision controller runs one agent per wave64 (impc_wide_kernel) up to one agent per SIMD of the
 * device (1,024 on MI355X) and 16 lanes per agent (impc_sep_kernel, 4 agents per wave) beyond;
 * 4: the 16-lane kernel at any count; 5: the one-agent-per-wave kernel at any count; 1 / 3: the
 * dense 6 x 6 layouts (64 / 16 lanes per agent). */
int mpccbf_set_variant(mpccbf_ctx* ctx, int variant);
/* Name of the IMPC kernel instantiation the current variant launches (diagnostics). */
const char* mpccbf_kernel_name(const mpccbf_ctx* ctx);
/* Launch form of the context's last IMPC main launch (diagnostics; a static string): "loop" when it
 * ran the instantiation specialised on the closed-loop launch's options — mpccbf_run_steps in grid
 * mode with targets, traj_t, x, obj and the status / iteration logs or buffers, and none of
 * substeps, cov, nb_out, primal_res, dual_res — else "generic". Same kernel name, same results. */
const char* mpccbf_launch_form(const mpccbf_ctx* ctx);

/* Active-set store (feature macro; MPCCBF_ABI_VERSION is unchanged: no struct changed layout).
 *
 * Attach (store != NULL) or detach a caller-owned device buffer of rows x 8 int32, indexed by the
 * agent's index into mpccbf_batch.states (rows >= num_states of every later call, else
 * MPCCBF_ERR_INVALID_ARGUMENT at that call). Zero-filled = no record.
 *
 * Record of an agent, written by every mpccbf_impc_solve / mpccbf_run_steps step that solves it:
 *   [0]     k, the number of sides of the final active set, 0 <= k <= 5
 *   [1..5]  the sides' keys (k of them, the rest 0)
 *   [6]     solver steps of the solve that produced the set, plus one per side that a warm start
 *           offered that solve (so a set that was confirmed in 0 steps does not look worthless)
 *   [7]     the IMPC iteration the set belongs to
 * The set is the final active set of the iteration whose curve is returned in x (the last OPTIMAL
 * iteration): the constraints that hold with equality there and carry a multiplier. The whole
 * record is zero when no iteration was OPTIMAL, when the optimum came from a path without an exact
 * active set (the interior-point solver), and for agents solved by a kernel without the store:
 * slack mode, the FoV controller and the dense layouts (variants 1 / 3, non-separable operators)
 * zero their agents' records and never read them. Supported: the separable collision controller
 * without slack variables in both layouts (16 lanes per agent, one agent per wave) and their
 * capacity launch; a record written by one layout is read by the other. While a store is attached
 * mpccbf_options::lean is ignored (the 16-lane layout runs its full kernel).
 *
 * Keys do not depend on lanes, slots or the order of the neighbour list:
 *   key >= 0, a box side:  key = (channel * 16 + row) * 2 + upper
 *       channel 0 / 1 / 2 = x / y / yaw, upper = 1 for the row's upper bound, 0 for its lower;
 *       row r of channel d is the r-th row, in order, among the rows of mpccbf_host_operators' G
 *       whose non-zero columns are 2 d and 2 d + 1 (the separable layout: every row of G touches
 *       one channel). The side is tight when G[i] y = hi[i] - Gs[i] s0 (upper; lo for lower).
 *   key < 0, a CBF side:   key = -(1 + neighbour * 8 + sample)
 *       neighbour = the other agent's index into mpccbf_batch.states, sample = the CBF sample k
 *       (0 <= k < cbf_horizon <= 8) of the iteration's QP (iteration 0 has sample 0 only).
 *
 * With a store attached the dual active set warm-starts across steps: a solve reads the agent's
 * record and, when [6] >= min_steps, maps its keys onto the new QP's own sides — box sides by
 * (channel, row), every CBF side of neighbour j onto j's sample-0 row of iteration 0; keys whose
 * neighbour left the list or whose row the filter dropped are skipped — and starts iteration 0
 * from the equality QP on them if every multiplier has its side's sign, else cold. Statuses and
 * solutions do not depend on the record (any subset of a QP's sides is a legal start and the
 * optimum is unique); a stale or arbitrary record costs solver steps only. min_steps: 0 = the
 * default (3), < 0 = export only, never warm-start. One buffer serves every step of
 * mpccbf_run_steps, read and written in place; each rank touches its own agents' rows only. */
#define MPCCBF_HAS_ACTIVE_STORE 1
int mpccbf_set_active_store(mpccbf_ctx* ctx, int32_t* store, int32_t rows, int32_t min_steps);

/* Neighbour-cap audit (feature macro; MPCCBF_ABI_VERSION is unchanged: no struct changed layout).
 *
 * The reference hands every one of the N - 1 other robots to each robot's QP
 * (ConnectivityIMPCCBF.cpp:59-67); a solve with capped lists (the knn_k nearest, or shorter CSR
 * lists) drops rows. The QPs are strictly convex in the reduced variables, so a capped QP's optimum
 * that satisfies every dropped row is also the unique optimum of the all-others QP, and a capped
 * QP that is INFEASIBLE stays INFEASIBLE with more rows. mpccbf_cap_audit_run evaluates that
 * certificate for a batch that mpccbf_impc_solve (or a one-step mpccbf_run_steps) just solved.
 *
 * batch: as the solve read and filled it — states the table that step read, the same agent_first,
 * num_agents, targets / refs, knn_k / knn_radius; x and status as the solve wrote them (required).
 * The lists are nb_row_ptr / nb_col (CSR mode; any order, duplicates allowed) or, in grid mode
 * (nb_row_ptr NULL), the nb_out of that solve (required; knn_k <= 16, so it holds the whole list).
 *
 * Agent a's dropped set is every row j != a of states that is not in its list (no radius). A
 * dropped row of IMPC iteration it and CBF sample k is the safety CBF row (a, b) of
 * (ego e, state j): iteration 0 has sample 0 only, e = the agent's state; iteration 1 has
 * k < cbf_horizon, e = position and velocity of the iteration-0 curve at parameter h k. The row is
 * live when !(b >= bmax), bmax = sum_d max(-a_d a_min_d, -a_d a_max_d) (the solver's own exact drop
 * rule, applied whatever mpccbf_options::no_cbf_filter says); a row with a non-finite b is not
 * live. Its excess is v = -a . acc_it(h k) - b with acc_it the second derivative of iteration it's
 * solution curve, its scaled excess v / (1 + |b|); it is violated when the scaled excess is above
 * tol (0 = 1e-6, the solver's feasibility tolerance).
 *
 * counts[a] (8 int32):
 *   [0]  live dropped rows of iteration 0
 *   [1]  of those, violated by the iteration-0 solution (0 when status[0] is not OPTIMAL)
 *   [2]  live dropped rows of iteration 1, over all samples
 *   [3]  of those, violated by the iteration-1 solution (0 when status[1] is not OPTIMAL)
 *   [4], [5]  the dropped neighbour (state index) with the largest scaled excess among the live
 *        rows of iteration 0 / 1 (ties: the smaller index, then the smaller sample); -1 when there
 *        is none or that iteration has no solution
 *   [6]  size of the dropped set
 *   [7]  certificate bits. Bit 0: iteration 0 is that of the all-others lists (status[0] OPTIMAL
 *        and [1] == 0, or status[0] INFEASIBLE). Bit 1: iteration 1 likewise (bit 0, and status[1]
 *        OPTIMAL with [3] == 0, or status[1] INFEASIBLE, or no iteration 1). Any other status
 *        (ERROR, UNKNOWN after an attempted solve) sets no bit.
 *   [2], [3], [5] are -1 when iteration 1 had no QP (impc_iter == 1, or status[0] not OPTIMAL).
 * excess[a] = the largest scaled excess of iteration 0 and of iteration 1 (NaN where [4] / [5] is
 * -1). live_nb[a] = the first 8 distinct dropped neighbours, in ascending state index, with a live
 * row in either iteration, -1 padded. An agent whose own state or a listed neighbour's state is
 * not finite audits as no live row and no bits.
 *
 * Iteration 0's solution is not returned by a solve whose iteration 1 succeeded, so the call runs
 * the context's own IMPC launch once more on the batch with one iteration, into context scratch
 * (no closed-loop state, no diagnostics, no active store read or written): the batch's x, status,
 * obj, iters, traj_t and an attached store are left untouched. x0_out receives those iteration-0
 * solutions (NaN where iteration 0 was not OPTIMAL). Like any mpccbf_impc_solve the call ends a
 * mpccbf_run::continue_tables rotation (the next mpccbf_run_steps rebuilds its table; its results
 * are those of a run without the audit). Asynchronous on the stream.
 *
 * Supported: the separable collision controller without slack variables in both layouts and their
 * capacity launch (the audit itself does not depend on the layout), impc_iter <= 2; slack mode,
 * the FoV controller and the dense layouts return MPCCBF_ERR_INVALID_ARGUMENT. Capacity: the
 * kernel keeps one membership bitmap over states per agent in LDS, num_states <= 65,536
 * (MPCCBF_ERR_CAPACITY beyond). Zero agents: MPCCBF_OK. */
#define MPCCBF_HAS_CAP_AUDIT 1
typedef struct mpccbf_cap_audit {
    int32_t* counts;   /* out, num_agents x 8 */
    double*  excess;   /* out, num_agents x 2, or NULL */
    int32_t* live_nb;  /* out, num_agents x 8, or NULL */
    double*  x0_out;   /* out, num_agents x n, or NULL: the iteration-0 solutions the audit used */
    double   tol;      /* 0 = 1e-6 */
} mpccbf_cap_audit;
int mpccbf_cap_audit_run(mpccbf_ctx* ctx, const mpccbf_batch* batch, const mpccbf_cap_audit* audit,
                         void* hip_stream);

/* Connectivity maintenance (feature macro; MPCCBF_ABI_VERSION is unchanged: no struct changed layout).
 *
 * Attach (c != NULL) or detach the connectivity rows of ConnectivityIMPCCBF
 * (ConnectivityIMPCCBF.cpp:143-157, 177-192, which the reference keeps commented out;
 * ConnectivityMPCCBFQPOperations.cpp:44-86, 111-173) to every later mpccbf_impc_solve /
 * mpccbf_run_steps step of the context. A team is a contiguous range of rows of
 * mpccbf_batch.states, team t = rows team_ptr[t] .. team_ptr[t+1]-1, 2 <= members <= 16; teams do
 * not depend on the neighbour lists (the safety rows still come from the batch's CSR or k-nearest
 * lists). Rows outside every team, and teams of one, get no new rows.
 *
 * Per step and team, from the table the step reads: the Laplacian weights
 * w_ij = exp((d_max^2 - d_ij^2)^2 / sigma) - 1 for d_ij <= d_max (else 0), sigma = d_max^4 / ln 2
 * (ConnectivityCBF::getLambda2), lambda2 and the unit Fiedler vector v (sign immaterial), by a
 * launch of its own ahead of the step's IMPC launch on the same stream. lambda2 > lambda2_switch:
 * the connectivity row, else the CLF rows. Rows of agent i per IMPC iteration: iteration 0 at sample
 * k = 0 with the ego state e = the agent's state; iteration it > 0 at samples k < cbf_horizon with
 * e = position and velocity of the previous iteration's curve at h k; the other members stay at
 * their current states, lambda2 and v at their current-state values; U_k is the acceleration at
 * sample k.
 *   connectivity row:  -(g_x, g_y, 0)^T U_k x <= e_v^T H e_v + 5 g.e_v + 5 (g.e_v + 5 (lambda2 - lambda2_min)),
 *       g / H the gradient / Hessian of lambda2 over the ego position with the Fiedler entries held
 *       fixed, summed over every other member (ConnectivityCBF.cpp:430-512);
 *   CLF rows, one per other member j:  +a^T U_k x <= -B,  V = (|p - p_j| - 2)^2, a = grad V,
 *       B = Lf^2 V + 5 Lf V + 2 V (ConnectivityCBF.cpp:200-243; ConnectivityControl.cpp:72-82's sign).
 * The safety rows' exact box-implication filter applies (mpccbf_options::no_cbf_filter keeps every
 * row); a row that no acceleration satisfies makes the QP INFEASIBLE.
 *
 * While attached the solves run the connectivity launch (16 lanes per agent, 64 staged rows per
 * agent and iteration: a full team of 16 at cbf_horizon 2 fits; beyond it the agent's QP reports
 * ERROR) whatever mpccbf_set_variant says; mpccbf_kernel_name reports it. A team of more than 16
 * members reports ERROR for its agents and NaN in lambda2; every other agent is unaffected. After a
 * detach every call is what it was before the attach. An attached active-set store gets zero
 * records from these launches; mpccbf_cap_audit_run returns MPCCBF_ERR_INVALID_ARGUMENT.
 * team_ptr[num_teams] must not exceed num_states of a later solve (MPCCBF_ERR_INVALID_ARGUMENT at
 * that call). With a communicator each rank computes the spectra of the teams that intersect its
 * agent range (a team may straddle ranks: the state table is gathered).
 *
 * Refused with MPCCBF_ERR_INVALID_ARGUMENT: bad arguments (checked first, without a context),
 * slack mode (the reference indexes the connectivity row's slack by self_idx into N - 1 slack
 * variables), the FoV controller (cbf_mode 1), non-separable operators, d_max <= d_min. */
#define MPCCBF_HAS_CONNECTIVITY 1
typedef struct mpccbf_connectivity {
    double d_max;
    double lambda2_min;     /* 0 = 0.1 */
    double lambda2_switch;  /* 0 = 0.1 */
    int32_t num_teams;
    const int32_t* team_ptr; /* HOST, num_teams + 1 non-decreasing offsets into the rows of `states`; copied */
    double* lambda2;        /* out, device, num_teams, or NULL: this step's lambda2 per team (NaN: team > 16) */
    double* fiedler;        /* out, device, team_ptr[num_teams] - team_ptr[0] entries (state row r at
                               r - team_ptr[0]), or NULL */
} mpccbf_connectivity;
int mpccbf_set_connectivity(mpccbf_ctx* ctx, const mpccbf_connectivity* c /* NULL detaches */);

/* ABI 11: waves of the IMPC launch mpccbf_impc_solve / mpccbf_run_steps makes for num_agents
 * agents with the context's variant that write mpccbf_run::kernel_clock (0: that kernel has no
 * clock). */
int32_t mpccbf_impc_launch_waves(const mpccbf_ctx* ctx, int32_t num_agents);

/* Neighbour lists on the device: for each agent of [agent_first, agent_first+num_agents) the
 * (at most) k nearest other agents of `states` (planar distance) within `radius`, sorted by
 * index; k <= 0 means all N-1 others (reference semantics, radius ignored). row_ptr gets
 * num_agents + 1 entries, col capacity num_agents * (k > 0 ? k : num_states - 1). */
int mpccbf_build_neighbors(mpccbf_ctx* ctx, const double* states, int32_t num_states,
                           int32_t agent_first, int32_t num_agents, int32_t k, double radius,
                           int32_t* row_ptr, int32_t* col, void* hip_stream);

/* The FoV controller's per-neighbour rows on the device, by the same device functions the IMPC
 * kernel evaluates (for parity checks of the rows themselves): for count (ego, neighbour) pairs
 * (ego: count x 6, nb_xy: count x 2, device) the box-shifted Voronoi hyperplane
 * (separating_hyperplanes::voronoi, Voronoi.cpp:10-29, math::shiftHyperplane, Helpers.cpp:20-36;
 * bbox: host, 3 half extents, NULL = 0) as voronoi[i] = (nx, ny, 0, offset), n . p + offset = 0,
 * and the four FoV HOCBF rows (FovCBF::get{Safety,LB,RB,Range}{Constraints,Bound},
 * FovCBF.cpp:622-810) as fov_rows[i][kind] = (a0, a1, a2, b), kind = safety, left, right, range
 * (b = DBL_MAX for the border rows of a 360-degree field of view). Either output may be NULL. */
int mpccbf_fov_rows_eval(int32_t count, const double* ego, const double* nb_xy, double fov, double Ds,
                         double Rs, const double* bbox, double* voronoi, double* fov_rows, void* hip_stream);

/* ---- Batched CBF-only controller (FovControl::optimize, cbf/src/controller/FovControl.cpp:17-86)
 * Per agent: min ||u - u_des||^2 over the control input u (3) subject to the 4 FoV HOCBF rows of
 * every observed neighbour (FovQPGenerator.cpp:12-115), the velocity CBF rows
 * u_d <= vmax_d - v_d and -u_d <= v_d - vmin_d (FovCBF.cpp:112-146, linear alpha) and
 * u_min <= u <= u_max. slack_mode: one slack variable >= 0 per observed neighbour relaxes its FoV
 * rows (FovControl.cpp:25-62). No context needed; all pointers are device pointers, asynchronous
 * on the stream. */
typedef struct mpccbf_fov_control_params {
    double fov, Ds, Rs;       /* FovCBF(fov, safety_dist, max_dist, ...) */
    double v_min[3], v_max[3];
    double u_min[3], u_max[3];
    int32_t slack_mode;
    double slack_cost, slack_decay_rate;
    int32_t max_pdip_iters;   /* default 60 */
    double tolerance;         /* default 1e-9 */
} mpccbf_fov_control_params;

typedef struct mpccbf_fov_control_batch {
    int32_t num_agents;
    const double* states;      /* num_agents x 6: ego (x, y, yaw, vx, vy, w) */
    const double* desired_u;   /* num_agents x 3 */
    const int32_t* nb_row_ptr; /* num_agents + 1: observed neighbours of agent i are */
    const double* nb_xy;       /* rows nb_row_ptr[i] .. nb_row_ptr[i+1]-1 of nb_xy (x, y) */
    double* u;                 /* out, num_agents x 3 (NaN when not OPTIMAL) */
    int32_t* status;           /* out, num_agents (qpcpp::SolveStatus), or NULL */
    double* obj;               /* out, ||u - u_des||^2, or NULL */
    int32_t* iters;            /* out, PDIP iterations, or NULL */
    const double* nb_cov;      /* slack mode: per observed neighbour (cxx, cxy, cyy), the estimate's
                                  position covariance ordering the slack weights by
                                  distanceToEllipse (FovControl.cpp:25-46); NULL = unknown */
} mpccbf_fov_control_batch;

/* Capacity: 4 * neighbours + 9 <= 64 rows per agent (13 observed neighbours) without slack;
 * 16 observed neighbours in slack mode (one slack variable each, cost slack_cost *
 * decay^{idx[i]}, included in obj); beyond it the agent's status is MPCCBF_ERROR.
 *
 * (The FoV controller inside mpccbf_impc_solve / mpccbf_run_steps, cbf_mode 1, has its own capacity,
 * per agent and IMPC iteration: 16 observed neighbours, 8 in slack mode, and 192 rows. The rows
 * are the shared box rows (mpccbf_num_shared_rows: 72 at k_hor 20), 4 Voronoi rows per neighbour
 * and the FoV rows the in-kernel filter keeps — at most 4 per neighbour in iteration 0 and
 * 4 * cbf_horizon from iteration 1 on; 2 and 2 * cbf_horizon at fov_beta = 2 pi, which has no
 * border rows; every one of them with mpccbf_options::no_cbf_filter. E.g. without the filter at
 * cbf_horizon 2 ten neighbours fill 72 + 40 + 80 = 192 rows and eleven do not fit. In slack mode
 * the FoV rows live in a slack image of 80 rows behind the others: box + Voronoi rows, rounded up
 * to a multiple of 16, plus 80 must not exceed 192 — 8 neighbours at 72 box rows land on it
 * exactly; with mpccbf_options::keep_redundant (117 box rows at k_hor 20) no neighbour count fits,
 * not even none. An iteration over a cap reports MPCCBF_ERROR and the iterations after it
 * UNKNOWN, the agent keeping the curve of the iterations before; other agents are unaffected.) */
int mpccbf_fov_control_solve(const mpccbf_fov_control_params* p, const mpccbf_fov_control_batch* b,
                             int32_t device, void* hip_stream);

/* ---- Batched particle filters for the FoV controllers' neighbour estimates (feature macro;
 * MPCCBF_ABI_VERSION is unchanged: no struct changed layout) ---------------------------------
 *
 * One particle filter per (observer, neighbour) pair, over the neighbour's planar position:
 * pf::ParticleFilter (particle_filter/src/detail/particle_filter.cpp) driven by
 * PFApplications::processFovUpdate (particle_filter/src/pf_applications.cpp:6-44), as
 * cbf/examples/fov/CBFControl_example.cpp:96-99,145-168,192-194 sets it up. No context needed; all
 * pointers are device pointers; asynchronous on the stream.
 *
 * Pairs are the entries of a CSR list: observer agent_first + i (a row of `states`) holds the pairs
 * e = nb_row_ptr[i] .. nb_row_ptr[i+1]-1, pair e estimates row nb_col[e] of `states`, and e indexes
 * every per-pair buffer (nb_row_ptr[0] may be nonzero: a call works on the pairs nb_row_ptr[0] ..
 * nb_row_ptr[0] + num_pairs - 1 and leaves every other pair's rows untouched, so observers can be
 * split over calls or ranks on shared buffers). A pair whose nb_col entry is not a row of `states`
 * is skipped.
 *
 * mpccbf_pf_init (ParticleFilter::init, particle_filter.cpp:12-56): particles = x0 + chol(init_cov) z,
 * weights 1 / P, est_xy = x0, est_cov = init_cov, flags 0; x0 = the neighbour's position in `states`
 * or, when init_xy is given, init_xy[e].
 *
 * mpccbf_pf_step (processFovUpdate), per pair:
 *   1. predict: p += input[e] dt + W z, z ~ N(0, I) per particle; W = `process` is a plain matrix
 *      multiplier, as in the reference (particle_filter.cpp:63-75); input NULL = 0
 *   2. negative information: w /= weight_reduction for every particle inside the observer's field of
 *      view (math::insideFOV, Geometry.cpp:59-73: |bearing| <= fov / 2 and distance <= Rs)
 *   3. only if the neighbour's position in `states` is inside the observer's field of view:
 *      w = exp(-1/2 d^T R^-1 d), d = particle - that position, R = meas_cov; normalised to sum 1
 *      (this overwrites the weights of 2, as in the reference)
 *   4. multinomial resampling: P draws u in [0, 1), ancestor = the first j with
 *      u < (sum_{i<=j} w_i) / sum w, clamped to P - 1 (std::discrete_distribution's rule); the new
 *      particle and weight are the ancestor's; the weights are not renormalised
 *   5. est_xy = mean of the particles, est_cov = sum (p - mean)(p - mean)^T / (P - 1) as
 *      (cxx, cxy, cyy): the row formats of mpccbf_fov_control_batch.nb_xy / nb_cov
 * Where the reference is undefined (a zero weight sum): when the sum of the weights is 0 or not
 * finite after 2 or after 3, the weights become 1 / P and bit 1 of the pair's flag word is set.
 * Bit 0 of the flag word: the neighbour was measured this step (3 ran).
 *
 * Randomness is counter-based: every draw is a pure function of (seed, step_index, the observer's
 * row in `states`, the neighbour's row, particle, component) — components 0 / 1 the x / y normal of
 * the predict, 2 the resampling uniform, 3 / 4 the x / y normal of init — so a call repeats bit for
 * bit and a pair's results do not depend on the split of the observers over calls.
 *
 * Refused with MPCCBF_ERR_INVALID_ARGUMENT on the host, before any device call: num_particles
 * outside 2 .. 1024, init_cov or meas_cov not positive definite, weight_reduction <= 0, a negative
 * count, agent_first + num_agents > num_states, a NULL required pointer (states, nb_row_ptr, nb_col,
 * particles, weights, est_xy, est_cov) with num_pairs > 0. num_pairs == 0 or num_agents == 0:
 * MPCCBF_OK, nothing launched. */
#define MPCCBF_HAS_PF 1
typedef struct mpccbf_pf_params {
    int32_t num_particles;    /* P, 2 .. 1024 */
    double init_cov[3];       /* (cxx, cxy, cyy) of the initial particle cloud */
    double process[4];        /* W, row-major 2 x 2 */
    double meas_cov[3];       /* R as (cxx, cxy, cyy) */
    double dt;                /* the reference hard-codes 0.2 (particle_filter.cpp:19) */
    double fov, Rs;           /* the observers' field of view (rad) and sensing range */
    double weight_reduction;  /* pf_applications.h's weight_reduction_factor */
    uint64_t seed;
} mpccbf_pf_params;

typedef struct mpccbf_pf_batch {
    int32_t num_states;
    const double* states;      /* num_states x 6 */
    int32_t agent_first;
    int32_t num_agents;        /* row i of nb_row_ptr is observer agent_first + i */
    const int32_t* nb_row_ptr; /* num_agents + 1 */
    const int32_t* nb_col;
    int32_t num_pairs;         /* nb_row_ptr[num_agents] - nb_row_ptr[0] (the host knows it) */
    const double* input;       /* pairs x 2 (ux, uy), or NULL */
    const double* init_xy;     /* pairs x 2, or NULL; mpccbf_pf_init only */
    double* particles;         /* pairs x 2 x P: x then y */
    double* weights;           /* pairs x P */
    double* est_xy;            /* out, pairs x 2 */
    double* est_cov;           /* out, pairs x 3 */
    int32_t* flags;            /* out, pairs, or NULL */
    int32_t* ancestors;        /* out, pairs x P, or NULL: the resampling's choices (mpccbf_pf_step) */
    int64_t step_index;
} mpccbf_pf_batch;

int mpccbf_pf_init(const mpccbf_pf_params* p, const mpccbf_pf_batch* b, int32_t device, void* hip_stream);
int mpccbf_pf_step(const mpccbf_pf_params* p, const mpccbf_pf_batch* b, int32_t device, void* hip_stream);

/* ---- FoV IMPC on each observer's own neighbour estimates (feature macro; MPCCBF_ABI_VERSION is
 * unchanged: no struct changed layout) -----------------------------------------------------------
 *
 * FovBezierIMPCCBF::optimize(curves, state, other_robot_positions, other_robot_covs, ref) plans from
 * one position and one covariance per (observer, neighbour) pair (FovBezierIMPCCBF.cpp:48-52); both
 * feed the Voronoi rows, the four FoV CBF rows of every IMPC iteration and the distanceToEllipse
 * slack order (:58-81, 115-200). mpccbf_set_fov_estimates attaches those two vectors to a context of
 * the FoV controller (the attach idiom of mpccbf_set_active_store / mpccbf_set_connectivity).
 *
 * Pair indexing: pair e is CSR entry e of the batch's nb_row_ptr / nb_col, and e indexes every
 * per-pair buffer — mpccbf_pf_batch's indexing, a nonzero nb_row_ptr[0] included: est_xy / est_cov of
 * mpccbf_pf_step pass unchanged as nb_xy / nb_cov.
 *
 * While attached, every FoV mpccbf_impc_solve / mpccbf_run_steps step (CSR lists) changes two reads:
 *   - pair e's neighbour position is nb_xy[e] where it was states[nb_col[e]]: in the Voronoi rows, in
 *     the safety / left / right / range rows of iteration 0 and in their predicted forms of the later
 *     iterations;
 *   - the slack order is by distanceToEllipse(ego, nb_xy[e], nb_cov[e]), or -5 for every pair when
 *     nb_cov is NULL (the list order applies); mpccbf_batch::cov is ignored.
 * nb_col[e] still names the neighbour: it is what nb_out reports and the row the filter measures.
 * Nothing else changes: the ego state, targets, closed-loop store, noise and outputs are as they are.
 * mpccbf_kernel_name reports the estimate form, impc_fov_kernel<false,true> / <true,true>.
 *
 * With pf given, est_xy / est_cov must be the buffers nb_xy / nb_cov name (nb_cov may be NULL), and
 * step s of mpccbf_run_steps enqueues mpccbf_pf_step over the batch's lists against the table that
 * step reads, with step_index = batch.step_index + s and input NULL, ahead of the step's IMPC launch
 * on the same stream: mpccbf_run_steps(n) is bit for bit n x (mpccbf_pf_step; mpccbf_impc_solve).
 * mpccbf_impc_solve never steps the filter; the caller runs mpccbf_pf_init itself. pf is copied; the
 * buffers stay the caller's and must outlive the attach.
 *
 * Refused at the attach with MPCCBF_ERR_INVALID_ARGUMENT, on the host before any device call: the
 * collision controller (cbf_mode 0), num_pairs < 0, a NULL nb_xy with num_pairs > 0, pf with a
 * missing buffer (particles, weights, est_xy, est_cov), with est_xy != nb_xy, with a nb_cov that is
 * neither NULL nor est_cov, or with parameters mpccbf_pf_step refuses. Refused at a solve with
 * MPCCBF_ERR_INVALID_ARGUMENT while attached: grid mode (nb_row_ptr NULL: estimates belong to fixed
 * pairs) and a communicator of more than one rank.
 *
 * On the device: an observer whose list reaches a pair index >= num_pairs reports MPCCBF_ERROR for
 * its QPs and reads nothing out of range; an observer with a non-finite estimate reports MPCCBF_ERROR
 * (the non-finite rule of every solve); every other agent is unaffected in both cases. The
 * per-observer caps are those of the unattached solve (16 observed neighbours, 8 in slack mode).
 * After a detach every call is what it was before the attach. */
#define MPCCBF_HAS_FOV_ESTIMATES 1
typedef struct mpccbf_fov_estimates {
    int32_t num_pairs;        /* rows of every per-pair buffer */
    const double* nb_xy;      /* device, pairs x 2: est_xy's format */
    const double* nb_cov;     /* device, pairs x 3 (cxx, cxy, cyy), or NULL = unknown (infinite) */
    /* optional filter driven by mpccbf_run_steps (pf NULL: the estimates are the caller's and the
     * buffers below are not read) */
    const mpccbf_pf_params* pf;   /* copied */
    double* particles;        /* pairs x 2 x P */
    double* weights;          /* pairs x P */
    double* est_xy;           /* == nb_xy */
    double* est_cov;          /* == nb_cov unless that is NULL */
    int32_t* flags;           /* pairs, or NULL */
} mpccbf_fov_estimates;
int mpccbf_set_fov_estimates(mpccbf_ctx* ctx, const mpccbf_fov_estimates* e /* NULL detaches */);

/* ---- Closed-loop safety monitor (feature macro; MPCCBF_ABI_VERSION is unchanged: no struct changed
 * layout) ------------------------------------------------------------------------------------------
 *
 * Scores snapshots of a swarm on the device with the semantics of the reference's post-processing
 * script (workspace/experiments/python/metrics/collision_check.py:11-80), so a closed-loop run says
 * whether it stayed safe without its trace leaving the device. A sample is one snapshot of every
 * row's (x, y, ., ., ., .); samples are numbered from 0 after a reset.
 *
 * Per sample, over every unordered pair of rows i < j whose squared distance dx*dx + dy*dy, as
 * computed in double (products and sum rounded separately), is <= watch_radius^2 (inclusive):
 *   collision    box: rectangles_collide (:11-20) on the script's boxes (:28-39), term by term: corner
 *                = centre - half / 2, extent = 2 half, strict < and >; only additions and comparisons,
 *                so every decision is the script's, touching edges included. circle: d2 <= (2 r)^2,
 *                where the script tests hypot(dx, dy) <= 2 r: the two can differ by one rounding for
 *                a pair at the threshold.
 *   inside d_min d2 < d_min^2: the pair has left the CBF's own safe set.
 * Pairs beyond watch_radius are not seen: it must cover d_min and the shape's reach (circle 2 r, box
 * 2 |half| (1 + 2^-20)), so no collision and no pair inside d_min is missed; min_d2 is +inf for a row
 * with no other row that near. Goal test, agents only: dx*dx + dy*dy <= goal_radius^2 against the
 * agent's goal (the script takes the norm; the two can differ by one rounding at the threshold).
 *
 * Outputs (device; all integers, accumulated by atomic add and 64-bit unsigned atomic min, so they
 * repeat bit for bit in any order of arrival). summary, MPCCBF_MONITOR_WORDS int64:
 *   [0]  samples scored since the reset
 *   [1]  first collision as (sample << 40) | (i << 20) | j, the script's order (earliest sample, then
 *        smallest i, then smallest j); -1 = none
 *   [2]  colliding pair-samples   [3]  pair-samples inside d_min
 *   [4]  bits of the smallest squared distance seen (a non-negative double orders as its bits); +inf
 * Per row of the state table (index = the row's index in the table): reached_at = the first sample
 * with the agent inside its goal area (-1: never; rows that are no agents stay -1), min_d2, hit_samples
 * = samples in which the row is part of a colliding pair, unsafe_samples = samples with another row
 * inside d_min. sample_log (optional): row s = (colliding pairs, pairs inside d_min, bits of the
 * smallest squared distance) of sample s, for s < sample_log_rows.
 *
 * mpccbf_monitor_score scores num_samples samples of num_states rows. `samples` holds the agents'
 * states, agent a (row agent_first + a) of sample s at samples[s * sample_stride + a * row_stride]
 * (strides in doubles: a state table is (., 6), a mpccbf_batch::substeps buffer or a trace
 * traj[n][ts][6] is (6, ts * 6)). fixed_states (may be NULL) is a num_states x 6 table whose rows
 * outside the agent range take part in every sample as static rows, keeping their table index; with
 * NULL there are no such rows. goals: num_agents x 3, or NULL for no goal scoring. sample_first: the
 * index of the first sample, or -1 to continue at summary[0] (read on the device). Samples whose
 * index would reach 2^23 are not scored and not counted. Each call enqueues four operations (a
 * memset and three launches) on the stream: no host synchronisation, no allocation.
 *
 * One spatial hash per sample (count, scan, scatter: a cell holds any number of rows; cell edge and
 * table size by the rules of mpccbf_build_neighbors, mpccbf_monitor_table_size(num_states) buckets),
 * in the caller's scratch: mpccbf_monitor_scratch_bytes(rows, the most samples of one call).
 *
 * Refused with MPCCBF_ERR_INVALID_ARGUMENT on the host, before any device call: a NULL monitor, a
 * missing output (summary, reached_at, min_d2, hit_samples, unsafe_samples, scratch), a bad shape
 * (shape_type outside 0 / 1, a radius or half extent that is not positive and finite), d_min not
 * positive and finite, goal_radius < 0, watch_radius below d_min or below the shape's reach, rows < 1,
 * sample_log_rows < 0; at a score also negative counts, an agent range outside num_states,
 * num_states > rows, num_states > 2^20, sample_first < -1, sample_first + num_samples > 2^23, a
 * scratch smaller than mpccbf_monitor_scratch_bytes(num_states, num_samples), NULL samples with
 * agents to score. num_samples == 0 or num_states == 0: MPCCBF_OK, nothing enqueued.
 *
 * mpccbf_set_monitor attaches a monitor (copied; its buffers stay the caller's) to a context. While
 * attached, every mpccbf_impc_solve that is given next_states, and every step of mpccbf_run_steps,
 * enqueues one mpccbf_monitor_score after that step's IMPC launch on the same stream: the step's
 * substeps records (int(h / Ts) samples) when the batch gives substeps, else the one next-state
 * sample (table T_{s+1} in mpccbf_run_steps). The other rows of the state table are the fixed rows,
 * the goals are batch->targets (none with refs), and the sample index continues at summary[0] until
 * mpccbf_monitor_reset. The IMPC launch is untouched: no argument is added, removed or changed, so
 * kernel name, launch form ("loop" included) and every solve output are what they are unattached.
 * Refused at a solve while attached: num_states > rows, a scratch too small for the step's samples,
 * and a communicator of more than one rank. Limits: pairs beyond watch_radius are not seen, 2^20
 * rows, 2^23 samples, a single rank. */
#define MPCCBF_HAS_MONITOR 1
#define MPCCBF_MONITOR_WORDS 5
typedef struct mpccbf_monitor {
    int32_t shape_type;      /* 0 circle, 1 box (collision_check.py:22-41) */
    double  shape[2];        /* radius, - | half extents cx, cy as the script takes them */
    double  d_min;           /* the CBF's safe distance */
    double  goal_radius;     /* 0 = 1.0 (the script's default) */
    double  watch_radius;    /* 0 = 3 d_min; >= d_min and >= the shape's reach, else INVALID_ARGUMENT */
    int32_t rows;            /* capacity of the per-row arrays (>= num_states scored) */
    int64_t* summary;        /* device, MPCCBF_MONITOR_WORDS: samples, first-collision key (-1),
                                colliding pair-samples, pair-samples inside d_min, min d2 bits */
    int64_t* reached_at;     /* device, rows: first sample inside the goal area, -1 */
    double*  min_d2;         /* device, rows: smallest squared distance to another row, +inf beyond watch_radius */
    int32_t* hit_samples;    /* device, rows: samples in which the row collides */
    int32_t* unsafe_samples; /* device, rows: samples with another row inside d_min */
    int64_t* sample_log;     /* device, sample_log_rows x 3 (hits, inside d_min, min d2 bits), or NULL */
    int32_t  sample_log_rows;
    void*    scratch; size_t scratch_bytes;  /* >= mpccbf_monitor_scratch_bytes(rows, max samples per call) */
} mpccbf_monitor;
size_t mpccbf_monitor_scratch_bytes(int32_t rows, int32_t max_samples);
uint32_t mpccbf_monitor_table_size(int32_t num_rows);
/* initialises every output (summary, the per-row arrays over `rows`, the sample log) */
int mpccbf_monitor_reset(const mpccbf_monitor* m, int32_t device, void* hip_stream);
int mpccbf_monitor_score(const mpccbf_monitor* m, const double* samples, int32_t num_samples,
                         int64_t sample_stride, int64_t row_stride, int32_t agent_first, int32_t num_agents,
                         const double* fixed_states, int32_t num_states, const double* goals,
                         int64_t sample_first, int32_t device, void* hip_stream);
int mpccbf_set_monitor(mpccbf_ctx* ctx, const mpccbf_monitor* m /* NULL detaches */);

/* ---- Batched CBF-only connectivity controller (ConnectivityControl::optimize,
 * cbf/src/controller/ConnectivityControl.cpp:22-99) for teams of robots ----------------------
 * Per robot of a team (<= 16 robots; robots of team t are rows team_ptr[t] .. team_ptr[t+1]-1):
 * min ||u - u_des||^2 over u (3) subject to the safety CBF rows against every other team member
 * (ConnectivityCBF.cpp:152-198, d_min, cubic alpha), the velocity CBF rows (:250-286) and, when the
 * team's algebraic connectivity lambda2 (weighted Laplacian, :375-414, d_max) exceeds 0.1, the
 * connectivity CBF row (:430-512), else one CLF row per other member (:200-243). u is unbounded
 * (the reference's addControlBoundConstraint is commented out, :60). slack_mode: num_robots slack
 * variables, weights slack_cost * decay^i (:31-38); neighbour i's safety / CLF rows take slack i,
 * the connectivity row the last one. All pointers are device pointers; asynchronous. */
typedef struct mpccbf_connectivity_control_params {
    double d_min, d_max;
    double v_min[3], v_max[3];
    int32_t slack_mode;
    double slack_cost, slack_decay_rate;
    int32_t max_pdip_iters;   /* default 60 */
    double tolerance;         /* default 1e-9 */
} mpccbf_connectivity_control_params;

typedef struct mpccbf_connectivity_control_batch {
    int32_t num_teams;
    const int32_t* team_ptr;   /* num_teams + 1 offsets into the robot rows */
    const double* states;      /* robots x 6 (x, y, yaw, vx, vy, w) */
    const double* desired_u;   /* robots x 3 */
    double* u;                 /* out, robots x 3 (NaN when not OPTIMAL) */
    int32_t* status;           /* out, robots (qpcpp::SolveStatus), or NULL */
    double* obj;               /* out, ||u - u_des||^2 (+ slack cost), or NULL */
    int32_t* iters;            /* out, PDIP iterations, or NULL */
    double* lambda2;           /* out, num_teams, or NULL (NaN: a team of 0 or of more than 16) */
} mpccbf_connectivity_control_batch;

/* A team with more than 16 robots gets status MPCCBF_ERROR (NaN u and obj, 0 iterations) for all
 * its robots and NaN in lambda2. An empty team (team_ptr[t] == team_ptr[t+1]) has no rows, so none
 * is written, and no spectrum: its lambda2 is NaN. A team of 1 has lambda2 = 0 and only its
 * velocity rows. */
int mpccbf_connectivity_control_solve(const mpccbf_connectivity_control_params* p,
                                      const mpccbf_connectivity_control_batch* b, int32_t device,
                                      void* hip_stream);

/* ---- Formation-control rollouts in the example's order (feature macro; MPCCBF_ABI_VERSION is
 * unchanged: no struct changed layout) ---------------------------------------------------------
 *
 * The closed loop of cbf/examples/connectivity/CBFFormationControl_example.cpp:136-187 for a batch of
 * independent teams (<= 16 robots each), one wavefront per team, the whole loop on the device. Per
 * step, robot by robot in index order (robots before it have already moved): the critically damped
 * spring control toward its target (Controls.h:18-27, spring_constant; the example's 0.5), the
 * controller of mpccbf_connectivity_control_solve on the team's table as it stands (lambda2 is
 * recomputed at every robot's turn), zero control unless OPTIMAL (:168-172), the double integrator
 * (pos += Ts vel + Ts^2 u / 2, vel += Ts u; no yaw wrap) and the state noise pos_std / vel_std times
 * normal_sample(team_seed[t], absolute step, robot's index in its team, component), a pure function
 * of those four, so a team's run does not depend on its place in the batch or on how the steps are
 * split over calls. After the last robot of step s the table is sample step_first + s.
 *
 * Records (optional, per decision, [num_steps][robots] rows in the order of `states`, robots =
 * team_ptr[num_teams]): trace (the table's rows after the step), cbf_u (the control applied: zero
 * where the solve failed), desired_u, status, lambda2 (what that decision saw), iters.
 * Summary (optional, in/out so that calls chain; the caller initialises -1 / +inf / 0), scored as
 * experiments/python/metrics/collision_check.py scores a states.json: arrival_sample = the first
 * sample with the robot within goal_radius of its target (planar norm, <=); first_collision =
 * (sample, i, j) of the first colliding pair (i < j indices in the team) under the script's box test
 * on shape_half (:11-20, 28-39), earliest sample, then smallest i, then smallest j; min_d2 = the
 * smallest squared planar distance of two robots of the team over the samples; fail_count = the
 * decisions whose status was not OPTIMAL.
 *
 * The call is stateless and asynchronous: it enqueues ceil(num_steps / steps_per_launch) launches on
 * the stream (steps_per_launch 0 = MPCCBF_FORMATION_STEPS_PER_LAUNCH) and returns; the results do not
 * depend on the split. A team of more than 16 robots takes no step: every decision of it reports
 * MPCCBF_ERROR with NaN cbf_u and lambda2, its states stay and its trace rows copy them, its
 * fail_count counts them all. An empty team writes nothing.
 * Refused with MPCCBF_ERR_INVALID_ARGUMENT on the host, before any device call: a NULL argument, the
 * parameters mpccbf_connectivity_control_solve refuses, Ts not positive and finite, negative or
 * non-finite spring_constant, pos_std, vel_std or goal_radius, shape_half not positive and finite,
 * steps_per_launch < 0, negative num_teams, num_steps or step_first, step_first + num_steps beyond
 * 2^31 - 1, and with teams and steps to run a NULL team_ptr, states, targets or team_seed.
 * num_teams == 0 or num_steps == 0: MPCCBF_OK, nothing enqueued. */
#define MPCCBF_HAS_FORMATION_ROLLOUT 1
#define MPCCBF_FORMATION_STEPS_PER_LAUNCH 2
typedef struct mpccbf_formation_params {
    double Ts;
    double spring_constant;
    double pos_std, vel_std;
    double shape_half[2];      /* the box's half extents as collision_check.py takes them */
    double goal_radius;        /* as given (the script's default is 1.0); 0: only a robot on its target */
    int32_t steps_per_launch;  /* 0 = MPCCBF_FORMATION_STEPS_PER_LAUNCH */
} mpccbf_formation_params;

typedef struct mpccbf_formation_batch {
    int32_t num_teams;
    const int32_t* team_ptr;    /* num_teams + 1 offsets into the robot rows */
    double* states;             /* robots x 6, in/out: the table after the last step */
    const double* targets;      /* robots x 3 */
    const uint64_t* team_seed;  /* num_teams */
    int64_t step_first;         /* absolute index of the first step (noise key, sample numbers) */
    int32_t num_steps;
    double* trace;              /* out, [num_steps][robots][6], or NULL */
    double* cbf_u;              /* out, [num_steps][robots][3], or NULL */
    double* desired_u;          /* out, [num_steps][robots][3], or NULL */
    int32_t* status;            /* out, [num_steps][robots], or NULL */
    double* lambda2;            /* out, [num_steps][robots], or NULL */
    int32_t* iters;             /* out, [num_steps][robots], or NULL */
    int32_t* arrival_sample;    /* in/out, robots (-1: not yet), or NULL */
    int32_t* first_collision;   /* in/out, num_teams x 3 (sample, i, j; -1: none), or NULL */
    double* min_d2;             /* in/out, num_teams (+inf), or NULL */
    int32_t* fail_count;        /* in/out, num_teams, or NULL */
} mpccbf_formation_batch;

int mpccbf_formation_rollout(const mpccbf_connectivity_control_params* p, const mpccbf_formation_params* f,
                             const mpccbf_formation_batch* b, int32_t device, void* hip_stream);

/* ---- MPC-CBF team rollouts in the example's order (feature macro; MPCCBF_ABI_VERSION is unchanged:
 * no struct changed layout) -----------------------------------------------------------------------
 *
 * The closed loop of mpc_cbf/examples/MPCCBFFormationControl_example.cpp:131-231 for a batch of
 * independent teams (<= 16 robots each), one wavefront per team, the whole loop on the device, with
 * the context's operators. Per step, robot by robot in index order (robots before it have already
 * moved, :140, :201): ConnectivityIMPCCBF::optimize against every other robot of the team in index
 * order, read from the team's table as it stands (the pipeline of mpccbf_impc_solve's dense 64 x 4
 * layout, impc_kernel<6,64,4>: both IMPC iterations, iteration 1 only after an OPTIMAL iteration 0,
 * the kept curve the last OPTIMAL iteration's); then the closed-loop semantics of mpccbf_batch.traj_t:
 * a new curve resets traj_t to 0; with a kept curve, nsub = int(h / Ts) sub-steps at traj_t + Ts k
 * clamped to the curve's range; with no curve yet the robot holds its position at zero velocity, the
 * sub-steps' noise accumulating (:208-221). The noise is pos_std / vel_std times normal_sample(
 * team_seed[t], absolute step, robot's index in its team, component, sub-step), a pure function of
 * those, so a team's run depends on nothing but its own seed and data: not on its place in the batch,
 * nor on how the steps are split over launches and calls. A team alone with team_seed = noise_seed is
 * the loop of one mpccbf_impc_solve per robot (agent_first = i, num_agents = 1, next_states written
 * back in place) with all-others lists.
 *
 * Carried between steps, launches and calls, in/out, initialised by the caller: states; x_keep
 * (robots x n, n = mpccbf_num_vars: the kept curves, NaN = none); traj_t (robots, -1 = none); the
 * summary. Records (optional, per decision, [num_steps][robots] rows in the order of `states`, robots
 * = team_ptr[num_teams]): status, obj, iters (x impc_iter each, as mpccbf_batch's), x (the kept curve
 * after the decision), traj_t0 (traj_t as the decision found it), substeps (nsub x 6: the states the
 * example writes to states.json; the last one is the robot's new row), trace (the table after the
 * step).
 * Summary (optional, in/out so that calls chain; the caller initialises -1 / +inf / 0), scored as
 * experiments/python/metrics/collision_check.py scores a states.json over the sub-step samples,
 * sample number step * nsub + k, after the last robot of the step has moved: arrival_sample,
 * first_collision, min_d2 as mpccbf_formation_batch's; fail_count = the decisions without an OPTIMAL
 * iteration.
 *
 * Asynchronous: it enqueues ceil(num_steps / steps_per_launch) launches on the stream
 * (steps_per_launch 0 = MPCCBF_TEAM_STEPS_PER_LAUNCH) and returns; the results do not depend on the
 * split. The context keeps a device copy of the all-others lists and, when substeps is not recorded,
 * one step's sub-step rows; both are allocated at the first call that needs them (a growth
 * synchronises the device). An attached active-set store, monitor or neighbour-cap audit is not
 * consulted. A team of more than 16 robots takes no step: every decision of it reports MPCCBF_ERROR
 * (later iterations UNKNOWN, NaN obj), its states stay, its x, traj_t0, substeps and trace rows copy
 * what it has, its fail_count counts them all. An empty team writes nothing.
 * Refused with MPCCBF_ERR_INVALID_ARGUMENT on the host, before any launch (mpccbf_last_error names
 * the reason): a NULL argument; a FoV context (cbf_mode 1); slack_mode; operators the dense 64 x 4
 * layout does not take (reduced dimension != 6, 256 or more shared rows); 15 * cbf_horizon > 256 -
 * shared rows (a full team's CBF rows would not fit: no team of 1 .. 16 can meet a capacity error in
 * the kernel); a context with connectivity rows attached (a context is never bound to a communicator:
 * mpccbf_run_steps alone takes one, so the rollout is single-rank by construction); negative or
 * non-finite pos_std, vel_std or goal_radius, shape_half not positive and finite, steps_per_launch
 * < 0, negative num_teams, num_steps or step_first, step_first + num_steps beyond 2^31 - 1, with
 * arrival_sample or first_collision given (step_first + num_steps) * nsub beyond 2^31 - 1 (their
 * sample numbers are int32), and with teams and steps to run a NULL team_ptr, states, targets,
 * team_seed, x_keep or traj_t. num_teams == 0 or num_steps == 0: MPCCBF_OK, nothing enqueued. */
#define MPCCBF_HAS_TEAM_ROLLOUT 1
#define MPCCBF_TEAM_STEPS_PER_LAUNCH 2
typedef struct mpccbf_team_rollout_params {
    double pos_std, vel_std;
    double shape_half[2];      /* the box's half extents as collision_check.py takes them */
    double goal_radius;        /* as given (the script's default is 1.0); 0: only a robot on its target */
    int32_t steps_per_launch;  /* 0 = MPCCBF_TEAM_STEPS_PER_LAUNCH */
} mpccbf_team_rollout_params;

typedef struct mpccbf_team_batch {
    int32_t num_teams;
    const int32_t* team_ptr;    /* num_teams + 1 offsets into the robot rows */
    double* states;             /* robots x 6, in/out: the table after the last step */
    const double* targets;      /* robots x 3 */
    const uint64_t* team_seed;  /* num_teams */
    int64_t step_first;         /* absolute index of the first step (noise key, sample numbers) */
    int32_t num_steps;
    double* x_keep;             /* in/out, robots x n: the kept curves (NaN: none) */
    double* traj_t;             /* in/out, robots: the kept curve's evaluation time (-1: none) */
    int32_t* status;            /* out, [num_steps][robots][impc_iter], or NULL */
    double* obj;                /* out, [num_steps][robots][impc_iter], or NULL */
    int32_t* iters;             /* out, [num_steps][robots][impc_iter], or NULL */
    double* x;                  /* out, [num_steps][robots][n], or NULL */
    double* traj_t0;            /* out, [num_steps][robots], or NULL */
    double* substeps;           /* out, [num_steps][robots][nsub][6], or NULL */
    double* trace;              /* out, [num_steps][robots][6], or NULL */
    int32_t* arrival_sample;    /* in/out, robots (-1: not yet), or NULL */
    int32_t* first_collision;   /* in/out, num_teams x 3 (sample, i, j; -1: none), or NULL */
    double* min_d2;             /* in/out, num_teams (+inf), or NULL */
    int32_t* fail_count;        /* in/out, num_teams, or NULL */
} mpccbf_team_batch;

int mpccbf_team_rollout(mpccbf_ctx* ctx, const mpccbf_team_rollout_params* p, const mpccbf_team_batch* b,
                        void* hip_stream);

/* Generic dense QP in the flattened CPLEX form (host pointers; synchronous):
 *   minimise  x^T H x + c^T x + c0        (H symmetric: sum_{i<=j} q_ij x_i x_j, CPLEX.cpp:122-147)
 *   s.t.      lo_r <= A_r x <= hi_r       (rows; lo == hi is an equality)
 *             vlo_i <= x_i <= vhi_i
 * The host validates and packs the nonzeros; the device eliminates the equalities (Householder QR
 * with column pivoting: null space + minimum-norm particular solution) and solves the reduced
 * problem with the interior-point kernel. A QP with more than 64 variables or 64 equality rows
 * (fixed variables count as equalities) is reduced on the host the same way and solved by the same
 * device kernel. Inconsistent equalities are INFEASIBLE whatever the sizes; otherwise reduced
 * dimension <= 8 and 256 reduced rows (MPCCBF_ERR_CAPACITY beyond). x_out is written only if
 * *status_out is OPTIMAL (Solver.h:33-35). */
typedef struct mpccbf_dense_qp {
    int32_t n, m;
    const double* H;  /* n x n row-major */
    const double* c;  /* n */
    double c0;
    const double* A;  /* m x n row-major */
    const double* lo;
    const double* hi;
    const double* vlo; /* n, or NULL = free */
    const double* vhi;
} mpccbf_dense_qp;

int mpccbf_qp_solve_dense(const mpccbf_dense_qp* qp, double* x_out, double* obj_out,
                          int32_t* status_out);
/* Batched form: count independent QPs solved in one launch. */
int mpccbf_qp_solve_dense_batch(int32_t count, const mpccbf_dense_qp* qps, double* const* x_out,
                                double* obj_out, int32_t* status_out);

/* Host-only inspection of the condensed operators (no device needed; used by the CPU tests).
 * Call once with capacity_ok = 0 to get the sizes, then again with every pointer sized:
 *   H n*n, Z n*nz, Xs n*6, Pr nz*nz, Qs nz*6, Qt nz*3, Ks 6*6, Kt 3*6,
 *   G m*nz, Gs m*6, lo/hi m, Cs mc*6, clo/chi mc, UZ0 3*nz, US0 3*6 (any pointer may be NULL).
 * Objective of the condensed QP: 1/2 y^T Pr y + (Qs s0 + Qt t)^T y + s0^T Ks s0 + t^T Kt s0,
 * full decision vector x = Xs s0 + Z y. */
typedef struct mpccbf_host_ops {
    int32_t n, nz, m, mc, rows_total, rows_removed;
    int32_t capacity_ok;
    double *H, *Z, *Xs, *Pr, *Qs, *Qt, *Ks, *Kt, *G, *Gs, *lo, *hi, *Cs, *clo, *chi, *UZ0, *US0;
} mpccbf_host_ops;
int mpccbf_host_operators(const mpccbf_params* p, int32_t keep_redundant, mpccbf_host_ops* out);
const char* mpccbf_host_last_error(void);

/* Host-only inspection of the launch plan and the operator packing (no device needed; used by the
 * CPU tests; MPCCBF_ABI_VERSION is unchanged: no struct changed layout). For a context created from
 * (params, options; options NULL = defaults) on a device whose share-adaptive threshold is wide_max
 * (4 x its compute units; mpccbf_create's own), with this variant, an active store and connectivity
 * attached or not: what mpccbf_kernel_name and mpccbf_impc_launch_waves report after a solve of
 * num_agents agents with caller lists (csr) or the k nearest (knn_k), whether that launch reads
 * the store and defers agents, the capacity launch that follows ("": none), and the layout of the
 * operator buffer. The strings are static. buf: NULL, or buf_capacity doubles that receive the
 * buffer's head (call once for `total`). offsets: every operator's offset into the buffer. */
#define MPCCBF_HOST_PLAN_OFFSETS 38
typedef struct mpccbf_host_plan {
    const char* kernel_name;
    const char* capacity_name;
    int32_t block_size, agents_per_block; /* the main launch: ceil(num_agents / agents_per_block) blocks */
    int32_t clock_waves;
    int32_t store, defers;
    int32_t hot, total;        /* doubles: the prefix of the separable collision kernels' operators, all */
    int32_t wide_capacity;     /* the largest `hot` the one-agent-per-wave kernel stages */
    int32_t sep, sep_rows_per_dim, sep_sb, o_Gsep; /* separable layout: 3 x sep_sb x 16 rows of 10 doubles
                                  [g0 g1 | Gs(6) | lo hi] at o_Gsep, channel-major, row f of a channel in
                                  slot f / 16, lane f % 16; unused rows are g = 0, [-1, 1] */
    int32_t offsets[MPCCBF_HOST_PLAN_OFFSETS];
    double* buf;
    int32_t buf_capacity;
} mpccbf_host_plan;
int mpccbf_host_launch_plan(const mpccbf_params* p, const mpccbf_options* opt, int32_t variant,
                            int32_t num_agents, int32_t csr, int32_t knn_k, int32_t store,
                            int32_t connectivity, int32_t wide_max, mpccbf_host_plan* out);
/* The same plan's main launch with the launch-uniform options given (bit i of `facts` set: option i
 * of MPCCBF_FACT_* is given / on): its kernel id (the library's ImpcKernel), name and launch form
 * ("generic", "loop"; static strings). Any pointer may be NULL. */
enum {
    MPCCBF_FACT_TARGETS = 0, MPCCBF_FACT_TRAJ_T, MPCCBF_FACT_SUBSTEPS, MPCCBF_FACT_COV, MPCCBF_FACT_NB_OUT,
    MPCCBF_FACT_PRIMAL_RES, MPCCBF_FACT_DUAL_RES, MPCCBF_FACT_CONE, MPCCBF_FACT_X, MPCCBF_FACT_STATUS,
    MPCCBF_FACT_OBJ, MPCCBF_FACT_ITERS, MPCCBF_FACT_NEXT_STATES, MPCCBF_FACT_INSERT,
    MPCCBF_FACT_EST, /* per-pair FoV estimates attached (mpccbf_set_fov_estimates) */
    MPCCBF_FACT_COUNT
};
int mpccbf_host_launch_form(const mpccbf_params* p, const mpccbf_options* opt, int32_t variant,
                            int32_t num_agents, int32_t csr, int32_t knn_k, int32_t store,
                            int32_t connectivity, int32_t wide_max, uint32_t facts, int32_t* kernel_id,
                            const char** kernel_name, const char** form);

/* Diagnostics */
const char* mpccbf_last_error(void);
const char* mpccbf_status_string(int32_t status); /* SolveStatusToStr, Solver.cpp:4-28 */
int mpccbf_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MPCCBF_H */
