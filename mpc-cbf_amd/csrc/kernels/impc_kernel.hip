// impc_kernel.hip — one fused launch per control step: ConnectivityIMPCCBF::optimize for a
// batch of agents (mpc_cbf/src/controller/ConnectivityIMPCCBF.cpp:47-215).
//
// Mapping (gfx950, wave64): one agent per group of G lanes. Per agent:
//   1. state-dependent parts of the condensed QP: q = Qs s0 + Qt t, shared row bounds shifted by
//      Gs s0, constant-row feasibility (e.g. the k = 0 velocity bound, which the initial-state
//      equality pins);
//   2. IMPC iteration 0: closed-form safety-CBF rows at the current state
//      (ConnectivityCBF.cpp:152-198 via ConnectivityMPCCBFQPOperations.cpp:192-205), exact
//      redundancy filter, compaction into the group's LDS staging area, PDIP solve;
//   3. IMPC iteration 1 (only after OPTIMAL, :158): predicted ego states from iteration 0's curve
//      at h_samples(k), k < cbf_horizon (:161-168), CBF rows per (neighbour, k) (:252-272), solve;
//   4. outputs: per-iteration status/objective/iterations, control points of the kept curve
//      (x = Xs s0 + Z y), and the closed-loop next state (curve at t = h).
// Two solver layouts share steps 1-4:
//   impc_sep_kernel — dimension-separable operators (base_config.json): G = 16 lanes, lane l holds
//                     box row l of each channel and CBF row l; pdip_sep.hpp;
//   impc_kernel     — any operators: rows spread over G lanes x R slots, dense NZ x NZ normal
//                     matrix; pdip.hpp.
// Shared operators are read through the scalar/L1/L2 path (uniform addresses); per-agent inputs
// are a 48-byte state, a 24-byte target and the neighbour states (gathered, L2-resident).
//
// The kernels are in one header per layout: impc_dense.hpp (impc_kernel), impc_sep.hpp (the 16-lane
// agent and its wrappers), impc_wide_kernels.hpp (one agent per wave). This file holds the launchers
// (launch_plan.hpp) of the kernels launched without a store or connectivity: a switch from the
// plan's kernel id to the instantiation, grid and block as the plan gives them; which kernel runs
// when is impc_launch_plan's alone. The store and connectivity kernels are instantiated in
// impc_store.hip and impc_conn.hip ("Why separate translation units").
#include "impc_dense.hpp"
#include "impc_sep.hpp"
#include "impc_wide_kernels.hpp"
#include "launch_plan.hpp"

namespace mpccbf {

const int IMPC_WIDE_OPS_MAX = dev::WIDE_OPS;

// dense layout: the LDS row image of the agents of a block (G lanes per agent, R row slots per lane)
template <int NZ, int G, int R>
static hipError_t launch_impc_dense(int blocks, int block_size, const DevOps& op, const double* buf,
                                    const ImpcArgs& a, hipStream_t s) {
    const size_t lds = (size_t)(block_size / G) * (R * G - op.m) * (NZ + 1) * sizeof(double);
    return launch_kernel(dev::impc_kernel<NZ, G, R>, blocks, block_size, lds, s, op, buf, a);
}

// Layouts of the separable collision controller (mpccbf_set_variant, impc_launch_plan):
//   0 (default) — share-adaptive: up to one agent per SIMD of the device (1,024 on MI355X: config
//       4's rank share) the one-agent-per-wave kernel (its fallback as a second launch); beyond,
//       the 16-lane kernel (4 agents per wave: one wave per SIMD covers 4 x as many agents);
//   4 — the 16-lane kernel at any count (the layout of rounds 1-4);
//   5 — the one-agent-per-wave kernel at any count.
// The 16-lane main launch (IMPC_SEP) runs the lean pipeline — the fast start and the dual active set
// — inline and finishes the agents they do not settle with an out-of-line call of the full pipeline
// in the same wave (impc_sep_complete, impc_sep.hpp): 1.2 us per config-3 step under the kernel that
// had the interior-point solver inlined. (Round 6, measured and dropped: the same split with the
// full pipeline inlined after the IMPC loop ran the lean part 1.6 us slower than the lean kernel
// alone and 0.5 us slower than the full kernel.) IMPC_SEP_LEAN is the two-launch form of the split
// (mpccbf_options.lean): the unsettled agents go to the queue and IMPC_QUEUE1.
// Capacity launches (IMPC_QUEUE*): the agents the main launch deferred (the queue in a.queue):
//   slack mode, more than 16 neighbours — the slack solver, the neighbours with a live row
//   compacted into the lanes;
//   otherwise — the full separable pipeline (dual active set, PDIP attempts, phase 1): with 16 CBF
//   row slots when no agent can exceed them, else 8 slots per lane (128 rows). Agents beyond
//   that report ERROR.
hipError_t launch_impc(ImpcKernel k, int blocks, int block_size, const DevOps& op, const double* buf,
                       const ImpcArgs& a, hipStream_t s) {
    auto go = [&](auto kernel) { return launch_kernel(kernel, blocks, block_size, 0, s, op, buf, a); };
    // (the cases in the order the instantiations have always had: the compiler lays
    // the kernels out in it, and tools/code_sizes.py's hashes see a kernel's distance to its data)
    switch (k) {
        case IMPC_WIDE: return go(dev::impc_wide_kernel<256>);
        case IMPC_QUEUE_SLACK2: return go(dev::impc_sep_kernel<2, 2, true, 64, true>);
        case IMPC_QUEUE_SLACK1: return go(dev::impc_sep_kernel<1, 2, true, 64, true>);
        case IMPC_QUEUE8: return go(dev::impc_sep_kernel<1, 8, false, 64, true>);
        case IMPC_QUEUE1: return go(dev::impc_sep_kernel<1, 1, false, 64, true>);
        case IMPC_SLACK1: return go(dev::impc_sep_kernel<1, 2, true, 256>);
        // (two box slots per lane: 128-thread blocks, the 256-thread block's LDS is past 160 KB)
        case IMPC_SLACK2: return go(dev::impc_sep_kernel<2, 2, true, 128>);
        case IMPC_SEP_LEAN: return go(dev::impc_sep_kernel<1, 1, false, 256, false, true>);
        case IMPC_SEP: return go(dev::impc_sep_kernel<1, 1, false, 256>);
        case IMPC_DENSE_16_4: return launch_impc_dense<6, 16, 4>(blocks, block_size, op, buf, a, s);
        case IMPC_DENSE_64_1: return launch_impc_dense<6, 64, 1>(blocks, block_size, op, buf, a, s);
        case IMPC_DENSE_64_4: return launch_impc_dense<6, 64, 4>(blocks, block_size, op, buf, a, s);
        // (the loop form of IMPC_SEP, FORM_LOOP: the closed-loop launch's options as constants)
        case IMPC_SEP_LOOP: return go(dev::impc_sep_kernel<1, 1, false, 256, false, false, FORM_LOOP>);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mpccbf
