"""Python host binding of libmpccbf.so (include/mpccbf.h) — the MI355X batched MPC-CBF solver.

The product is the C ABI + HIP kernels; this module only marshals torch device tensors (device
memory, streams) into it. There is no CPU fallback: without the built library, or without a
GPU, every solve raises.
"""
from ._lib import (  # noqa: F401
    LIB_PATH, MpccbfError, Params, Options, Context, status_name, build_library, load,
    dense_qp_solve, dense_qp_solve_batch, STATUS_NAMES, OPTIMAL, FEASIBLE, UNBOUNDED, INFEASIBLE, ERROR, UNKNOWN,
    INFEASIBLEORUNBOUNDED, Comm, comm_unique_id, fov_control_solve, fov_control_params,
    connectivity_control_solve, decode_active_sides, encode_active_side, audit_summary,
    PfParams, PfBatch, pf_params, pf_init, pf_step, formation_rollout,
)
from . import swarm  # noqa: F401
from . import monitor  # noqa: F401
from .monitor import SafetyMonitor  # noqa: F401
from . import formation  # noqa: F401
from .formation import FormationRollouts  # noqa: F401
from . import team_rollout  # noqa: F401  (the binding's function is _lib.team_rollout)
from .team_rollout import TeamRollouts  # noqa: F401
from .estimator import FovEstimator  # noqa: F401
from .fov_control_sim import FovControlLoop  # noqa: F401
from .fov_impc_sim import FovImpcLoop  # noqa: F401
