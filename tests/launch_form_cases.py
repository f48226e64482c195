"""Inputs of the launch-form tests (test_launch_form_inputs.py on the CPU, test_gpu_launch_form.py on
the GPU): the loop form of the 16-lane main launch (FORM_LOOP, csrc/kernels/impc.hpp) against the
generic form of the same library.

The swarm is test_gpu_inkernel_completion.py's compressed lattice (64 agents at 0.45 x the spacing:
CBF sides active, INFEASIBLE agents included) with its last agent moved out of every radius, so that
one agent has no neighbour. The closed loop starts with a stored curve for the even agents (the
constant curve at the agent's position, evaluation time 0) and none for the odd ones (traj_t = -1):
an agent whose first QP is INFEASIBLE then falls back to its stored curve when even and holds its
position when odd, both already at step 0, where the CPU oracle can name them.
"""
import numpy as np

from mpccbf import swarm

N, K, RADIUS, SCALE = 64, 8, 6.0, 0.45
SEP16 = 4  # mpccbf_set_variant: the 16-lane kernel at any count
STEPS = 10
MAIN = "impc_sep_kernel<1,1,false,256>"
NOISE = dict(pos_std=1e-3, vel_std=1e-3, noise_seed=11)
FAR = 1000.0  # the lone agent's offset (m)

# (label, num_states, agent_first, num_agents): the whole table of 1, 15, 17 and 64 agents (a partial
# group of four, a partial block of 16, four blocks), and a sub-range of the 64-agent table
SHAPES = [("n1", 1, 0, 1), ("n15", 15, 0, 15), ("n17", 17, 0, 17), ("n64", 64, 0, 64), ("sub", 64, 5, 40)]


def config():
    return swarm.config(15)


def scenario(num_states=N):
    """(states, targets) of the first num_states agents; the 64-agent table's last agent is alone."""
    states, targets = swarm.lattice_swarm(N, seed=swarm.SEED)
    states[:, :2] *= SCALE
    shift = np.array([FAR, FAR]) - states[N - 1, :2]
    states[N - 1, :2] += shift
    targets[N - 1, :2] += shift
    return states[:num_states].copy(), targets[:num_states].copy()


def has_stored_curve(agent):
    return agent % 2 == 0


def initial_curves(cfg, states, first, count):
    """(x, traj_t) the closed loop starts from for agents first .. first + count - 1: the constant
    curve at the agent's position (every control point of channel d = state d) at time 0 for the
    agents with a stored curve, NaN and -1 for the others."""
    P, C = cfg["num_pieces"], cfg["num_control_points"]
    x = np.full((count, P, 3, C), np.nan)
    t = np.full(count, -1.0)
    for i in range(count):
        if has_stored_curve(first + i):
            x[i] = states[first + i, :3][None, :, None]
            t[i] = 0.0
    return x.reshape(count, P * 3 * C), t
