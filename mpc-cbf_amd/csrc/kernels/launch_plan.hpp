// launch_plan.hpp — every decision of one IMPC step's launches, derived in one place on the host:
// which instantiation runs, its block and grid, whether it writes the launch clock, reads the
// active-set store or defers agents, and which capacity launch follows. impc_launch_plan
// (launch_plan.hip) forms the plan; the launchers of the kernels' translation units switch on its
// kernel ids and hold no condition of their own; capi.hip reads everything else from it.
#pragma once

#include <hip/hip_runtime.h>

#include "impc.hpp"

namespace mpccbf {

struct ConnArgs;
struct SpectrumArgs;
struct AuditArgs;

enum ImpcKernel : int32_t {
    IMPC_NONE = 0,     // no instantiation fits (the launch reports hipErrorInvalidValue)
    IMPC_DENSE_16_4,   // impc_kernel.hip: impc_kernel<6,16,4> (impc_dense.hpp)
    IMPC_DENSE_64_1,   // impc_kernel<6,64,1>
    IMPC_DENSE_64_4,   // impc_kernel<6,64,4>
    IMPC_SEP,          // impc_sep_kernel<1,1,false,256> (impc_sep.hpp)
    IMPC_SEP_LEAN,     // impc_sep_kernel<1,1,false,256,false,true>
    IMPC_SLACK1,       // impc_sep_kernel<1,2,true,256>
    IMPC_SLACK2,       // impc_sep_kernel<2,2,true,128>
    IMPC_WIDE,         // impc_wide_kernel<256> (impc_wide_kernels.hpp)
    IMPC_QUEUE1,       // capacity launches: impc_sep_kernel<1,1,false,64,true>
    IMPC_QUEUE8,       //   impc_sep_kernel<1,8,false,64,true>
    IMPC_QUEUE_SLACK1, //   impc_sep_kernel<1,2,true,64,true>
    IMPC_QUEUE_SLACK2, //   impc_sep_kernel<2,2,true,64,true>
    IMPC_SEP_STORE,    // impc_store.hip: impc_sep_store_kernel<1,256,false> (impc_sep.hpp)
    IMPC_WIDE_STORE,   //   impc_wide_store_kernel<256> (impc_wide_kernels.hpp)
    IMPC_QUEUE1_STORE, //   impc_sep_store_kernel<1,64,true>
    IMPC_QUEUE8_STORE, //   impc_sep_store_kernel<8,64,true>
    IMPC_CONN,         // impc_conn.hip: impc_sep_conn_kernel<4,64> (impc_sep.hpp)
    IMPC_FOV,          // impc_fov.hip: impc_fov_kernel<false> (impc_fov.hpp)
    IMPC_FOV_SLACK,    //   impc_fov_kernel<true>
    IMPC_SEP_LOOP,     // impc_kernel.hip: IMPC_SEP in the loop form (FORM_LOOP, impc.hpp), reported under
                       //   IMPC_SEP's name
    IMPC_FOV_EST,        // impc_fov_est.hip: impc_fov_kernel<false,true>, the estimate form (ImpcArgs::est_xy)
    IMPC_FOV_SLACK_EST,  //   impc_fov_kernel<true,true>
};

// What is the same for every agent of one launch and known where ImpcArgs is filled (impc_enqueue):
// the options the loop form fixes at compile time. All false (the default): no launch qualifies.
struct LaunchFacts {
    bool targets;      // ImpcArgs::targets (else refs)
    bool traj_t;       // closed-loop simulator semantics
    bool substeps, cov, nb_out, primal_res, dual_res;  // optional inputs / outputs given
    bool cone;         // GridArgs::cone > 0
    bool x, status, obj, iters, next_states;  // outputs given
    bool insert;       // the launch fills the next step's neighbour table (GridArgs::ins_cnt)
    bool est;          // per-pair neighbour estimates attached (ImpcArgs::est_xy; FoV controller)
};

// The facts of these arguments, as a launch with them holds them
inline LaunchFacts launch_facts(const ImpcArgs& a) {
    LaunchFacts f{};
    f.targets = a.targets != nullptr;
    f.traj_t = a.traj_t != nullptr;
    f.substeps = a.substeps != nullptr;
    f.cov = a.cov != nullptr;
    f.nb_out = a.nb_out != nullptr;
    f.primal_res = a.primal_res != nullptr;
    f.dual_res = a.dual_res != nullptr;
    f.cone = a.grid.cone > 0.0;
    f.x = a.x != nullptr;
    f.status = a.status != nullptr;
    f.obj = a.obj != nullptr;
    f.iters = a.iters != nullptr;
    f.next_states = a.next_states != nullptr;
    f.insert = a.grid.ins_cnt != nullptr;
    f.est = a.est_xy != nullptr;
    return f;
}

struct LaunchPlan {
    ImpcKernel kernel;    // the main launch
    const char* name;     // its instantiation ("": none fits; the FoV and connectivity names are
                          // reported even where their launch refuses the operators)
    int32_t block_size;
    int32_t agents_per_block;  // grid: ceil(n / agents_per_block) blocks
    int32_t clock_waves;  // waves that write ImpcArgs::kclock: blocks * block_size / 64, or 0 for
                          // the kernels without a launch clock (dense, FoV)
    bool store;           // the launches read and write the active-set store
    bool defer;           // the main launch appends to ImpcArgs::defer; `capacity` must follow
    ImpcKernel capacity;  // the capacity launch (IMPC_QUEUE_*: its blocks), IMPC_NONE: none
    LaunchForm form;      // the main launch's form (FORM_LOOP: IMPC_SEP_LOOP alone)
};
const char* launch_form_name(LaunchForm f);  // "generic", "loop"
constexpr int IMPC_QUEUE_BLOCK = 64, IMPC_QUEUE_AGENTS = 4;

// Bounds of the kernels, defined next to them: the operator prefix the one-agent-per-wave kernel
// stages in LDS (doubles), the dense row image of the FoV kernel (rows)
extern const int IMPC_WIDE_OPS_MAX;
extern const int IMPC_FOV_ROWS_MAX;

// Pure: no HIP runtime call, no context state. `op` as mpccbf_create packed it (a store attached
// turns DevOps::lean off here, not in a copy); n: the agents of the launch.
// facts: the launch-uniform options; IMPC_SEP becomes IMPC_SEP_LOOP (same name, shape and clock)
// exactly when every one of them is what the loop form fixes; IMPC_FOV / IMPC_FOV_SLACK become
// their estimate forms exactly when facts.est is set.
LaunchPlan impc_launch_plan(const DevOps& op, int variant, int n, bool csr, int knn_k, bool store, bool conn,
                            const LaunchFacts& facts = LaunchFacts{});

inline int plan_blocks(const LaunchPlan& p, int n) { return (n + p.agents_per_block - 1) / p.agents_per_block; }

template <class Kernel, class... Args>
inline hipError_t launch_kernel(Kernel kernel, int blocks, int block_size, size_t lds, hipStream_t s,
                                const Args&... args) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(block_size), lds, s, args...);
    return hipGetLastError();
}

// The launchers: one per translation unit that instantiates IMPC kernels, `k` one of that unit's
// ids (any other: hipErrorInvalidValue), grid and block as the plan gives them.
hipError_t launch_impc(ImpcKernel k, int blocks, int block_size, const DevOps& op, const double* buf,
                       const ImpcArgs& a, hipStream_t s);
hipError_t launch_impc_store(ImpcKernel k, int blocks, int block_size, const DevOps& op, const double* buf,
                             const ImpcArgs& a, const StoreArgs& st, hipStream_t s);
hipError_t launch_impc_conn(ImpcKernel k, int blocks, int block_size, const DevOps& op, const double* buf,
                            const ImpcArgs& a, const ConnArgs& cn, hipStream_t s);
hipError_t launch_impc_fov(ImpcKernel k, int blocks, int block_size, const DevOps& op, const double* buf,
                           const ImpcArgs& a, hipStream_t s);
hipError_t launch_impc_fov_est(ImpcKernel k, int blocks, int block_size, const DevOps& op, const double* buf,
                               const ImpcArgs& a, hipStream_t s);

// The library's other launches (impc_fov.hip, impc_conn.hip, cap_audit.hip, neighbors.hip)
hipError_t launch_fov_rows_eval(int count, const double* ego, const double* nb, double fov, double Ds, double Rs,
                                double bbx, double bby, double* vor, double* rows, hipStream_t s);
hipError_t launch_team_spectrum(const SpectrumArgs& a, hipStream_t s);
hipError_t launch_cap_audit(const DevOps& op, const double* buf, const AuditArgs& a, hipStream_t s);
int launch_neighbors(const double* states, int num_states, int first, int num_agents, int k, double radius,
                     int32_t* row_ptr, int32_t* col, void* scratch, size_t scratch_bytes, hipStream_t s);
size_t neighbors_scratch_bytes(int num_states, int num_agents, int k);
size_t grid_table_bytes(int num_states);
void grid_table_carve(void* base, int num_states, uint32_t** cnt, uint32_t** slots, double** sst);
hipError_t launch_grid_insert(const double* states, int n, int skip0, int skip1, double radius, uint32_t* cnt,
                              uint32_t* slots, double* sst, hipStream_t s);

}  // namespace mpccbf
