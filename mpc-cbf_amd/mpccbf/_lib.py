"""ctypes marshalling for libmpccbf.so. Mirrors include/mpccbf.h one to one."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # mpc-cbf_amd/
LIB_PATH = os.environ.get("MPCCBF_LIB") or os.path.join(PKG_DIR, "build", "libmpccbf.so")

OPTIMAL, FEASIBLE, UNBOUNDED, INFEASIBLE, ERROR, UNKNOWN, INFEASIBLEORUNBOUNDED = range(7)
STATUS_NAMES = ["OPTIMAL", "FEASIBLE", "UNBOUNDED", "INFEASIBLE", "ERROR", "UNKNOWN",
                "INFEASIBLEORUNBOUNDED"]

# every symbol include/mpccbf.h declares (checked by tests/test_capi_symbols.py)
EXPORTED = [
    "mpccbf_create", "mpccbf_destroy", "mpccbf_num_vars", "mpccbf_reduced_dim",
    "mpccbf_num_shared_rows", "mpccbf_impc_solve", "mpccbf_set_variant", "mpccbf_build_neighbors",
    "mpccbf_qp_solve_dense", "mpccbf_qp_solve_dense_batch", "mpccbf_last_error",
    "mpccbf_status_string", "mpccbf_abi_version", "mpccbf_run_steps", "mpccbf_comm_unique_id",
    "mpccbf_comm_create", "mpccbf_comm_destroy", "mpccbf_kernel_name", "mpccbf_fov_control_solve",
    "mpccbf_connectivity_control_solve", "mpccbf_host_operators", "mpccbf_host_last_error",
    "mpccbf_comm_create_local", "mpccbf_fov_rows_eval", "mpccbf_impc_launch_waves",
    "mpccbf_set_active_store", "mpccbf_cap_audit_run", "mpccbf_set_connectivity",
    "mpccbf_host_launch_plan", "mpccbf_pf_init", "mpccbf_pf_step", "mpccbf_launch_form",
    "mpccbf_host_launch_form", "mpccbf_set_fov_estimates", "mpccbf_monitor_scratch_bytes",
    "mpccbf_monitor_table_size", "mpccbf_monitor_reset", "mpccbf_monitor_score", "mpccbf_set_monitor",
    "mpccbf_formation_rollout", "mpccbf_team_rollout",
]

# ImpcKernel ids (csrc/kernels/launch_plan.hpp) of the 16-lane main launch: generic and loop form
IMPC_SEP, IMPC_SEP_LOOP = 4, 20

# the launch-uniform options of one IMPC launch, in the bit order of MPCCBF_FACT_* (mpccbf.h)
LAUNCH_FACTS = ("targets", "traj_t", "substeps", "cov", "nb_out", "primal_res", "dual_res", "cone", "x",
                "status", "obj", "iters", "next_states", "insert", "est")
# the closed-loop launch of run_steps in grid mode as bench.py drives it: the loop form's options
LOOP_LAUNCH = dict.fromkeys(LAUNCH_FACTS, False)
LOOP_LAUNCH.update(dict.fromkeys(("targets", "traj_t", "x", "status", "obj", "iters", "next_states", "insert"), True))

# active-set store (mpccbf_set_active_store): int32 words per record, side keys per record
ACTIVE_STORE_WORDS = 8
ACTIVE_STORE_KEYS = 5


# neighbour-cap audit (mpccbf_cap_audit_run): int32 words per agent in counts, entries in live_nb
CAP_AUDIT_WORDS = 8
CAP_AUDIT_LIVE_NB = 8


class MpccbfError(RuntimeError):
    pass


def kernel_clock_us(clock) -> np.ndarray:
    """Per-launch durations in microseconds from a (num_steps, W, 2) kernel_clock array (numpy
    int64 / uint64): the largest wave end minus the smallest wave start over the written pairs;
    NaN for a step with no pair."""
    c = np.asarray(clock).view(np.uint64).astype(np.float64)
    t0, t1 = c[..., 0], c[..., 1]
    on = t1 > 0
    start = np.where(on, t0, np.inf).min(axis=1)
    end = np.where(on, t1, -np.inf).max(axis=1)
    return np.where(np.isfinite(start), (end - start) * 1e-2, np.nan)


def encode_active_side(side) -> int:
    """Key of one active side: ("box", channel, row, side) with side 0 = lower / 1 = upper (or
    "lower" / "upper"), or ("cbf", neighbour, sample). The encoding of include/mpccbf.h."""
    if side[0] == "box":
        _, channel, row, ul = side
        ul = {"lower": 0, "upper": 1}.get(ul, ul)
        if not (0 <= channel < 3 and 0 <= row < 16 and ul in (0, 1)):
            raise ValueError(f"box side out of range: {side}")
        return (channel * 16 + row) * 2 + ul
    if side[0] == "cbf":
        _, nb, sample = side
        if not (nb >= 0 and 0 <= sample < 8):
            raise ValueError(f"CBF side out of range: {side}")
        return -(1 + nb * 8 + sample)
    raise ValueError(f"unknown side kind: {side}")


def decode_active_sides(record) -> list:
    """The sides of one active-set record (8 int32: [k | keys | steps | iteration], see
    mpccbf_set_active_store in include/mpccbf.h) as a list of ("box", channel, row, side) with
    side 0 = lower / 1 = upper, and ("cbf", neighbour, sample)."""
    rec = [int(v) for v in record]
    if len(rec) != ACTIVE_STORE_WORDS:
        raise ValueError(f"an active-set record has {ACTIVE_STORE_WORDS} words")
    k = rec[0]
    if not 0 <= k <= ACTIVE_STORE_KEYS:
        raise ValueError(f"record holds k = {k} sides (0 .. {ACTIVE_STORE_KEYS})")
    out = []
    for key in rec[1:1 + k]:
        if key >= 0:
            if key >= 96:
                raise ValueError(f"box key {key} out of range")
            out.append(("box", key >> 5, (key >> 1) & 15, key & 1))
        else:
            v = -(key + 1)
            out.append(("cbf", v >> 3, v & 7))
    return out


def audit_summary(counts) -> dict:
    """Totals of a neighbour-cap audit's counts (num_agents x 8 int32, mpccbf_cap_audit in
    include/mpccbf.h; a tensor or an array; host-side): the live dropped rows and the violated ones
    of IMPC iteration 0 / 1 (agents without an iteration 1, words -1, add nothing), the agents
    whose iteration 0 / iteration 1 is certified to be that of the all-others lists (bits 0 / 1 of
    word 7), and the agents without the full certificate."""
    if hasattr(counts, "detach"):
        counts = counts.detach().cpu().numpy()
    c = np.asarray(counts, dtype=np.int64).reshape(-1, CAP_AUDIT_WORDS)
    tot = [int(np.clip(c[:, w], 0, None).sum()) for w in range(4)]
    bit0 = int(np.count_nonzero(c[:, 7] & 1))
    bit1 = int(np.count_nonzero(c[:, 7] & 2))
    return {"agents": int(c.shape[0]), "live0": tot[0], "violated0": tot[1], "live1": tot[2],
            "violated1": tot[3], "certified0": bit0, "certified1": bit1,
            "uncertified": int(c.shape[0]) - bit1}


def status_name(s: int) -> str:
    return STATUS_NAMES[s] if 0 <= s < len(STATUS_NAMES) else str(s)


class Params(C.Structure):
    _fields_ = [
        ("h", C.c_double), ("Ts", C.c_double), ("k_hor", C.c_int32),
        ("w_pos_err", C.c_double), ("w_u_eff", C.c_double), ("spd_f", C.c_int32),
        ("v_min", C.c_double * 3), ("v_max", C.c_double * 3),
        ("a_min", C.c_double * 3), ("a_max", C.c_double * 3),
        ("d_min", C.c_double),
        ("cbf_horizon", C.c_int32), ("impc_iter", C.c_int32), ("slack_mode", C.c_int32),
        ("slack_cost", C.c_double), ("slack_decay_rate", C.c_double),
        ("num_pieces", C.c_int32), ("num_control_points", C.c_int32),
        ("piece_max_parameter", C.c_double), ("continuity_upto_degree", C.c_int32),
        ("cbf_mode", C.c_int32), ("fov_beta", C.c_double), ("fov_Ds", C.c_double),
        ("fov_Rs", C.c_double), ("bbox", C.c_double * 3),
    ]

    @classmethod
    def from_dict(cls, cfg: dict) -> "Params":
        p = cls()
        for k, v in cfg.items():
            if isinstance(v, (list, tuple)):
                arr = getattr(p, k)
                for i, x in enumerate(v):
                    arr[i] = x
            else:
                setattr(p, k, v)
        return p


class Options(C.Structure):
    _fields_ = [("device", C.c_int32), ("keep_redundant", C.c_int32),
                ("no_cbf_filter", C.c_int32), ("max_pdip_iters", C.c_int32),
                ("tolerance", C.c_double), ("warm_delta", C.c_double),
                ("dual_as_steps", C.c_int32), ("no_fast_start", C.c_int32), ("early_it", C.c_int32),
                ("das_warm_steps", C.c_int32), ("lean", C.c_int32)]


class Batch(C.Structure):
    _fields_ = [
        ("num_states", C.c_int32), ("states", C.c_void_p), ("agent_first", C.c_int32),
        ("num_agents", C.c_int32), ("targets", C.c_void_p), ("refs", C.c_void_p),
        ("nb_row_ptr", C.c_void_p), ("nb_col", C.c_void_p), ("x", C.c_void_p),
        ("status", C.c_void_p), ("obj", C.c_void_p), ("iters", C.c_void_p),
        ("next_states", C.c_void_p), ("knn_k", C.c_int32), ("knn_radius", C.c_double),
        ("stamps", C.c_void_p), ("traj_t", C.c_void_p), ("pos_std", C.c_double),
        ("vel_std", C.c_double), ("noise_seed", C.c_uint64), ("step_index", C.c_int64),
        ("cov", C.c_void_p), ("primal_res", C.c_void_p), ("dual_res", C.c_void_p),
        ("substeps", C.c_void_p), ("nb_out", C.c_void_p),
    ]


class CapAudit(C.Structure):
    _fields_ = [("counts", C.c_void_p), ("excess", C.c_void_p), ("live_nb", C.c_void_p),
                ("x0_out", C.c_void_p), ("tol", C.c_double)]


class Connectivity(C.Structure):
    _fields_ = [("d_max", C.c_double), ("lambda2_min", C.c_double), ("lambda2_switch", C.c_double),
                ("num_teams", C.c_int32), ("team_ptr", C.c_void_p), ("lambda2", C.c_void_p),
                ("fiedler", C.c_void_p)]


class FovEstimates(C.Structure):
    _fields_ = [("num_pairs", C.c_int32), ("nb_xy", C.c_void_p), ("nb_cov", C.c_void_p), ("pf", C.c_void_p),
                ("particles", C.c_void_p), ("weights", C.c_void_p), ("est_xy", C.c_void_p),
                ("est_cov", C.c_void_p), ("flags", C.c_void_p)]


# safety monitor (mpccbf_monitor): int64 words of its summary
MONITOR_WORDS = 5


class Monitor(C.Structure):
    _fields_ = [("shape_type", C.c_int32), ("shape", C.c_double * 2), ("d_min", C.c_double),
                ("goal_radius", C.c_double), ("watch_radius", C.c_double), ("rows", C.c_int32),
                ("summary", C.c_void_p), ("reached_at", C.c_void_p), ("min_d2", C.c_void_p),
                ("hit_samples", C.c_void_p), ("unsafe_samples", C.c_void_p), ("sample_log", C.c_void_p),
                ("sample_log_rows", C.c_int32), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


class Run(C.Structure):
    _fields_ = [("num_steps", C.c_int32), ("states_alt", C.c_void_p), ("status_log", C.c_void_p),
                ("iters_log", C.c_void_p), ("step_ms", C.c_void_p), ("solve_ms", C.c_void_p),
                ("comm", C.c_void_p), ("reserve_steps", C.c_int32), ("solve_stride", C.c_int32),
                ("final_table", C.c_int32), ("kernel_clock", C.c_void_p),
                ("kernel_clock_waves", C.c_int32), ("continue_tables", C.c_int32)]


class DenseQP(C.Structure):
    _fields_ = [("n", C.c_int32), ("m", C.c_int32), ("H", C.c_void_p), ("c", C.c_void_p),
                ("c0", C.c_double), ("A", C.c_void_p), ("lo", C.c_void_p), ("hi", C.c_void_p),
                ("vlo", C.c_void_p), ("vhi", C.c_void_p)]


def build_library(quiet: bool = True) -> str:
    """Compile libmpccbf.so for gfx950 with hipcc (works without a GPU)."""
    out = subprocess.run(["make", "-C", PKG_DIR, "-j8"], capture_output=True, text=True)
    if out.returncode != 0:
        raise MpccbfError("libmpccbf build failed:\n" + out.stdout[-4000:] + out.stderr[-4000:])
    return LIB_PATH


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MpccbfError(f"{LIB_PATH} not built: run `make -C mpc-cbf_amd` (no CPU fallback)")
    # torch ships its own libamdhip64 (soname libamdhip64.so.7, the one libmpccbf needs). Load
    # torch first so the dynamic loader binds libmpccbf to that same HIP runtime: one runtime per
    # process, so torch's device pointers, streams and events are valid handles for the library.
    # (Loading libmpccbf first would pull /opt/rocm's copy and leave torch with a second one.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.mpccbf_create.argtypes = [C.POINTER(Params), C.POINTER(Options), C.POINTER(vp)]
    L.mpccbf_destroy.argtypes = [vp]
    L.mpccbf_destroy.restype = None
    for f in ("mpccbf_num_vars", "mpccbf_reduced_dim", "mpccbf_num_shared_rows"):
        getattr(L, f).argtypes = [vp]
    L.mpccbf_impc_solve.argtypes = [vp, C.POINTER(Batch), vp]
    L.mpccbf_set_variant.argtypes = [vp, C.c_int]
    if hasattr(L, "mpccbf_set_active_store"):  # (MPCCBF_LIB may name a library from before the store)
        L.mpccbf_set_active_store.argtypes = [vp, vp, C.c_int32, C.c_int32]
    if hasattr(L, "mpccbf_cap_audit_run"):
        L.mpccbf_cap_audit_run.argtypes = [vp, C.POINTER(Batch), C.POINTER(CapAudit), vp]
    if hasattr(L, "mpccbf_set_connectivity"):
        L.mpccbf_set_connectivity.argtypes = [vp, C.POINTER(Connectivity)]
    if hasattr(L, "mpccbf_set_fov_estimates"):
        L.mpccbf_set_fov_estimates.argtypes = [vp, C.POINTER(FovEstimates)]
    if hasattr(L, "mpccbf_set_monitor"):  # (MPCCBF_LIB may name a library from before the monitor)
        L.mpccbf_set_monitor.argtypes = [vp, C.POINTER(Monitor)]
        L.mpccbf_monitor_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
        L.mpccbf_monitor_scratch_bytes.restype = C.c_size_t
        L.mpccbf_monitor_table_size.argtypes = [C.c_int32]
        L.mpccbf_monitor_table_size.restype = C.c_uint32
        L.mpccbf_monitor_reset.argtypes = [C.POINTER(Monitor), C.c_int32, vp]
        L.mpccbf_monitor_score.argtypes = [C.POINTER(Monitor), vp, C.c_int32, C.c_int64, C.c_int64, C.c_int32,
                                           C.c_int32, vp, C.c_int32, vp, C.c_int64, C.c_int32, vp]
    L.mpccbf_build_neighbors.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_double, vp, vp, vp]
    L.mpccbf_qp_solve_dense.argtypes = [C.POINTER(DenseQP), vp, vp, vp]
    L.mpccbf_qp_solve_dense_batch.argtypes = [C.c_int32, C.POINTER(DenseQP), vp, vp, vp]
    L.mpccbf_run_steps.argtypes = [vp, C.POINTER(Batch), C.POINTER(Run), vp]
    L.mpccbf_comm_unique_id.argtypes = [C.c_char_p]
    L.mpccbf_comm_create.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.mpccbf_comm_create_local.argtypes = [C.c_int32, C.c_int32, C.POINTER(vp)]
    L.mpccbf_comm_destroy.argtypes = [vp]
    L.mpccbf_comm_destroy.restype = None
    L.mpccbf_kernel_name.argtypes = [vp]
    L.mpccbf_kernel_name.restype = C.c_char_p
    if hasattr(L, "mpccbf_launch_form"):  # (MPCCBF_LIB may name a library from before the launch forms)
        L.mpccbf_launch_form.argtypes = [vp]
        L.mpccbf_launch_form.restype = C.c_char_p
    L.mpccbf_impc_launch_waves.argtypes = [vp, C.c_int32]
    L.mpccbf_impc_launch_waves.restype = C.c_int32
    L.mpccbf_last_error.restype = C.c_char_p
    L.mpccbf_fov_rows_eval.argtypes = [C.c_int32, vp, vp, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp]
    L.mpccbf_status_string.restype = C.c_char_p
    L.mpccbf_status_string.argtypes = [C.c_int32]
    for f in ("mpccbf_pf_init", "mpccbf_pf_step"):
        # (PfParams / PfBatch are defined below; resolved at call time)
        getattr(L, f).argtypes = [C.POINTER(PfParams), C.POINTER(PfBatch), C.c_int32, vp]
    if hasattr(L, "mpccbf_formation_rollout"):  # (MPCCBF_LIB may name a library from before the rollouts)
        L.mpccbf_formation_rollout.argtypes = [C.POINTER(ConnControlParams), C.POINTER(FormationParams),
                                               C.POINTER(FormationBatch), C.c_int32, vp]
    if hasattr(L, "mpccbf_team_rollout"):  # (MPCCBF_LIB may name a library from before the team rollouts)
        L.mpccbf_team_rollout.argtypes = [vp, C.POINTER(TeamRolloutParams), C.POINTER(TeamBatch), vp]
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        msg = load().mpccbf_last_error().decode()
        raise MpccbfError(f"mpccbf error {rc}: {msg}")


def _ptr(t) -> int | None:
    if t is None:
        return None
    import torch  # noqa: F401  (device tensors only)
    if not t.is_cuda:
        raise MpccbfError("libmpccbf batch entry points take device tensors")
    if not t.is_contiguous():
        raise MpccbfError("tensor must be contiguous")
    return t.data_ptr()


def _stream(stream):
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    return getattr(stream, "cuda_stream", stream)


class PreparedRun:
    """One marshalled mpccbf_run_steps call (Context.prepare_run_steps): calling it runs the steps
    (the C call alone); it holds the tensors its pointers refer to."""

    def __init__(self, ctx, batch, run, stream, states, states_alt, num_steps, step_ms, solve_ms, keep):
        self._ctx, self._b, self._r, self._s = ctx, batch, run, stream
        self._fn = load().mpccbf_run_steps
        self._tables = (states, states_alt)
        self._n, self._step_ms, self._solve_ms, self._keep = num_steps, step_ms, solve_ms, keep

    def __call__(self):
        _check(self._fn(self._ctx._h, C.byref(self._b), C.byref(self._r), self._s))
        est = self._ctx._fov_estimator
        if est is not None and self._b.nb_row_ptr:  # (the attached filter stepped once per step)
            est.step_index += self._n
        out = {"final": self._tables[0] if self._r.final_table == 0 else self._tables[1]}
        if self._solve_ms is not None:
            # copies: the library overwrites both host buffers at the next call
            out["step_ms"] = None if self._step_ms is None else self._step_ms[:self._n].copy()
            sm = self._solve_ms[:self._n]
            out["solve_ms"] = sm[sm >= 0]
        return out


class Context:
    """One controller configuration on one device (mpccbf_create / mpccbf_destroy)."""

    def __init__(self, cfg: dict, device: int = 0, keep_redundant: bool = False,
                 no_cbf_filter: bool = False, max_iters: int = 0, tol: float = 0.0,
                 warm_delta: float = 0.0, dual_as_steps: int = 0, no_fast_start: bool = False,
                 early_it: int = 0, das_warm_steps: int = 0, lean: bool = False):
        """warm_delta: IMPC iteration-1 warm start floor (0 = default 0.3, < 0 = cold start);
        dual_as_steps: active-set step limit (0 = default, < 0 = the PDIP alone); the other solver
        options as mpccbf_options (include/mpccbf.h), 0 = default."""
        L = load()
        self.cfg = dict(cfg)
        self.params = Params.from_dict(cfg)
        o = Options(device=device, keep_redundant=int(keep_redundant),
                    no_cbf_filter=int(no_cbf_filter), max_pdip_iters=max_iters, tolerance=tol,
                    warm_delta=warm_delta, dual_as_steps=int(dual_as_steps),
                    no_fast_start=int(no_fast_start), early_it=int(early_it),
                    das_warm_steps=int(das_warm_steps), lean=int(lean))
        h = C.c_void_p()
        _check(L.mpccbf_create(C.byref(self.params), C.byref(o), C.byref(h)))
        self._h = h
        self.n = L.mpccbf_num_vars(h)
        self.nz = L.mpccbf_reduced_dim(h)
        self.shared_rows = L.mpccbf_num_shared_rows(h)
        self.impc_iter = int(cfg["impc_iter"])
        self.k_hor = int(cfg["k_hor"])
        self.device = device
        self._active_store = None
        self._connectivity = None
        self._fov_estimates = None   # the tensors attached by set_fov_estimates / set_fov_estimator
        self._fov_estimator = None   # the FovEstimator run_steps drives, or None
        self._monitor = None         # the attached SafetyMonitor, or None
        self._last_knn = (0, 0.0)  # the neighbour query of the last solve (audit_neighbors' default)

    def close(self):
        if getattr(self, "_h", None):
            load().mpccbf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_variant(self, v: int):
        _check(load().mpccbf_set_variant(self._h, v))

    def set_active_store(self, store, min_steps: int = 0):
        """Attach a (rows, 8) contiguous int32 device tensor as the active-set store, or detach
        with None (mpccbf_set_active_store): every later solve writes each agent's final active
        set into its row and warm-starts from it (min_steps: 0 = default threshold, < 0 = export
        only). The context keeps a reference to the tensor while it is attached."""
        if store is None:
            _check(load().mpccbf_set_active_store(self._h, None, 0, int(min_steps)))
            self._active_store = None
            return
        import torch
        if not isinstance(store, torch.Tensor) or not store.is_cuda:
            raise MpccbfError("the active store must be a device tensor")
        if store.device.index != self.device:
            raise MpccbfError(f"the active store is on {store.device}, the context on device {self.device}")
        if store.dtype != torch.int32:
            raise MpccbfError("the active store must be int32")
        if store.dim() != 2 or store.shape[1] != ACTIVE_STORE_WORDS or store.shape[0] < 1:
            raise MpccbfError(f"the active store must have shape (rows >= 1, {ACTIVE_STORE_WORDS})")
        if not store.is_contiguous():
            raise MpccbfError("the active store must be contiguous")
        _check(load().mpccbf_set_active_store(self._h, store.data_ptr(), int(store.shape[0]), int(min_steps)))
        self._active_store = store

    def set_connectivity(self, team_ptr, d_max=None, lambda2_min=0.1, lambda2_switch=0.1, lambda2=None,
                         fiedler=None):
        """Attach the connectivity-maintenance rows (mpccbf_set_connectivity), or detach with
        team_ptr None. team_ptr: host integers, num_teams + 1 non-decreasing offsets into the rows of
        the state table (team t = rows team_ptr[t] .. team_ptr[t+1]-1, 2 .. 16 members); d_max: the
        connectivity range. lambda2 (num_teams) / fiedler (team_ptr[-1] - team_ptr[0]): optional
        float64 device tensors every later step writes its teams' lambda2 and Fiedler entries
        into; the context keeps a reference to them while attached."""
        if team_ptr is None:
            _check(load().mpccbf_set_connectivity(self._h, None))
            self._connectivity = None
            return
        if d_max is None:
            raise MpccbfError("set_connectivity needs d_max")
        tp = np.ascontiguousarray(np.asarray(team_ptr).reshape(-1), dtype=np.int32)
        if tp.size < 1:
            raise MpccbfError("team_ptr needs at least one offset")
        import torch
        for name, t, size in (("lambda2", lambda2, tp.size - 1), ("fiedler", fiedler, int(tp[-1]) - int(tp[0]))):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
                raise MpccbfError(f"{name} must be a contiguous float64 device tensor")
            if t.numel() < size:
                raise MpccbfError(f"{name} needs {size} entries")
        k = Connectivity(d_max=float(d_max), lambda2_min=float(lambda2_min), lambda2_switch=float(lambda2_switch),
                         num_teams=int(tp.size - 1), team_ptr=tp.ctypes.data, lambda2=_ptr(lambda2),
                         fiedler=_ptr(fiedler))
        _check(load().mpccbf_set_connectivity(self._h, C.byref(k)))
        self._connectivity = (tp, lambda2, fiedler)

    def _check_pair_tensor(self, name, t, cols, rows=None):
        import torch
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
            raise MpccbfError(f"{name} must be a contiguous float64 device tensor")
        if t.device.index != self.device:
            raise MpccbfError(f"{name} is on {t.device}, the context on device {self.device}")
        if t.dim() != 2 or t.shape[1] != cols or (rows is not None and t.shape[0] != rows):
            raise MpccbfError(f"{name} must have shape (pairs, {cols})")

    def set_fov_estimates(self, nb_xy, nb_cov=None):
        """Attach each observer's own neighbour estimates (mpccbf_set_fov_estimates), or detach with
        nb_xy None. nb_xy (pairs x 2) / nb_cov (pairs x 3 = (cxx, cxy, cyy), None = unknown):
        float64 device tensors indexed by the CSR entry of the lists a later solve is given —
        FovEstimator's est_xy / est_cov pass unchanged. While attached every FoV solve in CSR mode
        takes pair e's neighbour position from nb_xy[e] and the slack order from nb_cov[e] (cov= is
        ignored); the tensors are read at every solve, so writing into them updates the estimates.
        The context keeps a reference to them while attached."""
        if nb_xy is None:
            _check(load().mpccbf_set_fov_estimates(self._h, None))
            self._fov_estimates = self._fov_estimator = None
            return
        self._check_pair_tensor("nb_xy", nb_xy, 2)
        if nb_cov is not None:
            self._check_pair_tensor("nb_cov", nb_cov, 3, rows=nb_xy.shape[0])
        e = FovEstimates(num_pairs=int(nb_xy.shape[0]), nb_xy=_ptr(nb_xy), nb_cov=_ptr(nb_cov))
        _check(load().mpccbf_set_fov_estimates(self._h, C.byref(e)))
        self._fov_estimates, self._fov_estimator = (nb_xy, nb_cov), None

    def set_fov_estimator(self, est, use_cov: bool = True):
        """Attach a FovEstimator's own tensors and parameters: solves read its est_xy / est_cov as
        set_fov_estimates does, and every step of run_steps (CSR lists: the estimator's) first steps
        the filter against the table that step reads (mpccbf_pf_step, no motion input), exactly as
        est.step(states) followed by impc_solve; est.step_index advances by the steps run.
        impc_solve never steps it; est.init(states) is the caller's. use_cov=False: the slack order
        takes every covariance as unknown. Detach with set_fov_estimates(None)."""
        if est.device != self.device:
            raise MpccbfError(f"the estimator is on device {est.device}, the context on device {self.device}")
        e = FovEstimates(num_pairs=int(est.rows), nb_xy=_ptr(est.est_xy), nb_cov=_ptr(est.est_cov) if use_cov else None,
                         pf=C.addressof(est.params), particles=_ptr(est.particles), weights=_ptr(est.weights),
                         est_xy=_ptr(est.est_xy), est_cov=_ptr(est.est_cov), flags=_ptr(est.flags))
        _check(load().mpccbf_set_fov_estimates(self._h, C.byref(e)))
        self._fov_estimates, self._fov_estimator = (est.est_xy, est.est_cov), est

    def set_monitor(self, mon):
        """Attach a SafetyMonitor (mpccbf_set_monitor), or detach with None. While attached, every
        impc_solve that is given next_states and every step of run_steps enqueues one score of that
        step's samples behind its IMPC launch: the substeps records when substeps= is given, else
        the next states; the goals are targets=. The IMPC launch itself is unchanged. The context
        keeps a reference to the monitor while it is attached."""
        if mon is None:
            _check(load().mpccbf_set_monitor(self._h, None))
            self._monitor = None
            return
        if mon.device != self.device:
            raise MpccbfError(f"the monitor is on device {mon.device}, the context on device {self.device}")
        _check(load().mpccbf_set_monitor(self._h, C.byref(mon.struct)))
        self._monitor = mon

    def _monitor_agents(self, agent_first, num_agents, scored):
        # (the attached monitor's result() takes its goal statistics over the agents last scored)
        if self._monitor is not None and scored and num_agents > 0:
            self._monitor.agents = (int(agent_first), int(num_agents))

    def alloc_active_store(self, num_states: int, device=None):
        """A zero-filled (num_states, 8) int32 store (no records) for set_active_store."""
        import torch
        dev = device or torch.device("cuda", self.device)
        return torch.zeros((int(num_states), ACTIVE_STORE_WORDS), dtype=torch.int32, device=dev)

    @property
    def kernel_name(self) -> str:
        return load().mpccbf_kernel_name(self._h).decode()

    @property
    def launch_form(self) -> str:
        """The last IMPC main launch's form (mpccbf_launch_form): "loop" or "generic"."""
        return load().mpccbf_launch_form(self._h).decode()

    def build_neighbors(self, states, first, count, k, radius, row_ptr, col, stream=None):
        _check(load().mpccbf_build_neighbors(self._h, _ptr(states), states.shape[0], first, count,
                                             k, float(radius), _ptr(row_ptr), _ptr(col),
                                             _stream(stream)))

    def impc_solve(self, states, nb_row_ptr=None, nb_col=None, targets=None, refs=None,
                   agent_first=0, num_agents=None, x=None, status=None, obj=None, iters=None,
                   next_states=None, knn_k=0, knn_radius=0.0, stream=None, stamps=None,
                   traj_t=None, pos_std=0.0, vel_std=0.0, noise_seed=0, step_index=0, cov=None,
                   primal_res=None, dual_res=None, substeps=None, nb_out=None):
        """CSR neighbours (nb_row_ptr/nb_col) or, with both None, the knn_k nearest within
        knn_radius found on the device in the same launch sequence. traj_t (float64, one per
        agent, initialised to -1) turns on the closed-loop simulator semantics: x persists the
        last successful curve and the next state follows it (see mpccbf_batch)."""
        if num_agents is None:
            num_agents = states.shape[0] - agent_first
        self._last_knn = (int(knn_k), float(knn_radius))
        b = Batch(num_states=states.shape[0], states=_ptr(states), agent_first=agent_first,
                  num_agents=num_agents, targets=_ptr(targets), refs=_ptr(refs),
                  nb_row_ptr=_ptr(nb_row_ptr), nb_col=_ptr(nb_col), x=_ptr(x),
                  status=_ptr(status), obj=_ptr(obj), iters=_ptr(iters),
                  next_states=_ptr(next_states), knn_k=int(knn_k), knn_radius=float(knn_radius),
                  stamps=_ptr(stamps), traj_t=_ptr(traj_t), pos_std=float(pos_std),
                  vel_std=float(vel_std), noise_seed=int(noise_seed), step_index=int(step_index),
                  cov=_ptr(cov), primal_res=_ptr(primal_res), dual_res=_ptr(dual_res),
                  substeps=_ptr(substeps), nb_out=_ptr(nb_out))
        _check(load().mpccbf_impc_solve(self._h, C.byref(b), _stream(stream)))
        self._monitor_agents(agent_first, num_agents, next_states is not None)

    def audit_neighbors(self, states, *, x, status, targets=None, refs=None, nb_row_ptr=None, nb_col=None,
                        nb_out=None, agent_first=0, num_agents=None, knn_k=None, knn_radius=None, tol=0.0,
                        live_nb=False, x0=False, stream=None):
        """Neighbour-cap audit of the batch impc_solve (or a one-step run_steps) just solved
        (mpccbf_cap_audit_run): states, targets / refs, the agent range and knn_k / knn_radius as
        in that solve (the query defaults to the context's last solve's), x and status as it filled them, and its lists: nb_row_ptr / nb_col, or in
        grid mode the nb_out it wrote. Returns a dict of device tensors: counts (num_agents x 8
        int32, see mpccbf_cap_audit; audit_summary() totals them), excess (num_agents x 2) and,
        on request, live_nb (num_agents x 8 int32) and x0 (num_agents x n, the iteration-0
        solutions). The solve's outputs and an attached active store are left untouched."""
        import torch
        if num_agents is None:
            num_agents = states.shape[0] - agent_first
        if knn_k is None:
            knn_k = self._last_knn[0]
        if knn_radius is None:
            knn_radius = self._last_knn[1]
        dev = states.device
        rows = max(int(num_agents), 1)  # (at least one row: an empty tensor has no pointer to pass)
        out = {"counts": torch.zeros((rows, CAP_AUDIT_WORDS), dtype=torch.int32, device=dev),
               "excess": torch.full((rows, 2), float("nan"), dtype=torch.float64, device=dev)}
        if live_nb:
            out["live_nb"] = torch.full((rows, CAP_AUDIT_LIVE_NB), -1, dtype=torch.int32, device=dev)
        if x0:
            out["x0"] = torch.full((rows, self.n), float("nan"), dtype=torch.float64, device=dev)
        b = Batch(num_states=states.shape[0], states=_ptr(states), agent_first=agent_first,
                  num_agents=num_agents, targets=_ptr(targets), refs=_ptr(refs),
                  nb_row_ptr=_ptr(nb_row_ptr), nb_col=_ptr(nb_col), x=_ptr(x), status=_ptr(status),
                  knn_k=int(knn_k), knn_radius=float(knn_radius), nb_out=_ptr(nb_out))
        a = CapAudit(counts=_ptr(out["counts"]), excess=_ptr(out["excess"]), live_nb=_ptr(out.get("live_nb")),
                     x0_out=_ptr(out.get("x0")), tol=float(tol))
        _check(load().mpccbf_cap_audit_run(self._h, C.byref(b), C.byref(a), _stream(stream)))
        return {k: v[:max(int(num_agents), 0)] for k, v in out.items()}

    def run_steps(self, *args, **kw):
        """Closed-loop control steps on the device (mpccbf_run_steps): prepare_run_steps(...)()
        in one call; see prepare_run_steps for the arguments and the returned dict."""
        return self.prepare_run_steps(*args, **kw)()

    def prepare_run_steps(self, states, states_alt, num_steps, targets=None, refs=None, agent_first=0,
                  num_agents=None, knn_k=0, knn_radius=0.0, nb_row_ptr=None, nb_col=None, x=None,
                  status=None, obj=None, iters=None, status_log=None, iters_log=None,
                  timing=False, comm=None, reserve_steps=0, solve_stride=1, step_timing=True,
                  stream=None, traj_t=None, pos_std=0.0, vel_std=0.0, noise_seed=0, step_index=0,
                  cov=None, kernel_clock=None, stamps=None, continue_tables=False, nb_out=None,
                  substeps=None):
        """The arguments of one mpccbf_run_steps call, marshalled once (checks, ctypes structures,
        the stream handle): returns a PreparedRun whose call () runs the steps — a caller that
        times the steps prepares them outside its timed region. The call returns a dict with the
        table holding the final states ('final', a tensor) and, with timing=True, per-step
        device times 'step_ms' and IMPC-kernel times 'solve_ms' (numpy, ms). kernel_clock: a
        (num_steps, W, 2) device tensor (torch.int64, W >= launch_waves(num_agents)) for every
        wave's start / end of every IMPC launch (s_memrealtime, 100 MHz ticks; zero: no wave);
        kernel_clock_us() turns it into per-launch durations. stamps: the diagnostics builds' phase
        stamps (as impc_solve; every step overwrites them). nb_out: as impc_solve (every step
        overwrites it: it ends holding the lists of the last step). substeps: as impc_solve (every
        step overwrites it; an attached monitor scores each step's records before the next step)."""
        if num_agents is None:
            num_agents = states.shape[0] - agent_first
        self._last_knn = (int(knn_k), float(knn_radius))
        if kernel_clock is not None:
            # the library writes num_steps x W x 2 uint64 words from the base pointer: a shorter,
            # narrower or strided tensor would be written out of bounds (W itself is checked
            # against the launch's waves by mpccbf_run_steps)
            if (kernel_clock.dim() != 3 or not kernel_clock.is_contiguous() or kernel_clock.element_size() != 8
                    or kernel_clock.shape[0] < num_steps or kernel_clock.shape[2] != 2):
                raise ValueError("kernel_clock must be a contiguous (>= num_steps, W, 2) tensor of 8-byte elements")
        b = Batch(num_states=states.shape[0], states=_ptr(states), agent_first=agent_first,
                  num_agents=num_agents, targets=_ptr(targets), refs=_ptr(refs),
                  nb_row_ptr=_ptr(nb_row_ptr), nb_col=_ptr(nb_col), x=_ptr(x),
                  status=_ptr(status), obj=_ptr(obj), iters=_ptr(iters), next_states=None,
                  knn_k=int(knn_k), knn_radius=float(knn_radius), stamps=_ptr(stamps),
                  traj_t=_ptr(traj_t), pos_std=float(pos_std), vel_std=float(vel_std),
                  noise_seed=int(noise_seed), step_index=int(step_index), cov=_ptr(cov),
                  nb_out=_ptr(nb_out), substeps=_ptr(substeps))
        self._monitor_agents(agent_first, num_agents, num_steps > 0)
        step_ms = np.zeros(max(num_steps, 1), dtype=np.float32) if timing and step_timing else None
        solve_ms = np.zeros(max(num_steps, 1), dtype=np.float32) if timing else None
        r = Run(num_steps=num_steps, states_alt=_ptr(states_alt), status_log=_ptr(status_log),
                iters_log=_ptr(iters_log),
                step_ms=None if step_ms is None else step_ms.ctypes.data,
                solve_ms=None if solve_ms is None else solve_ms.ctypes.data,
                comm=None if comm is None else comm.handle, reserve_steps=reserve_steps,
                solve_stride=solve_stride, kernel_clock=_ptr(kernel_clock),
                kernel_clock_waves=0 if kernel_clock is None else int(kernel_clock.shape[1]),
                continue_tables=int(bool(continue_tables)))
        return PreparedRun(self, b, r, _stream(stream), states, states_alt, num_steps, step_ms, solve_ms,
                           keep=(targets, refs, nb_row_ptr, nb_col, x, status, obj, iters, status_log,
                                 iters_log, traj_t, cov, kernel_clock, stamps, nb_out, substeps))

    def launch_waves(self, num_agents: int) -> int:
        """Waves of the IMPC launch for num_agents that write the launch clock (0: no clock)."""
        return int(load().mpccbf_impc_launch_waves(self._h, int(num_agents)))

    def alloc_outputs(self, num_agents: int, device=None):
        import torch
        dev = device or torch.device("cuda", self.device)
        return dict(
            x=torch.empty((num_agents, self.n), dtype=torch.float64, device=dev),
            status=torch.empty((num_agents, self.impc_iter), dtype=torch.int32, device=dev),
            obj=torch.empty((num_agents, self.impc_iter), dtype=torch.float64, device=dev),
            iters=torch.empty((num_agents, self.impc_iter), dtype=torch.int32, device=dev),
            next_states=torch.empty((num_agents, 6), dtype=torch.float64, device=dev),
            primal_res=torch.empty((num_agents, self.impc_iter), dtype=torch.float64, device=dev),
            dual_res=torch.empty((num_agents, self.impc_iter), dtype=torch.float64, device=dev),
        )


class HostOps(C.Structure):
    _fields_ = [("n", C.c_int32), ("nz", C.c_int32), ("m", C.c_int32), ("mc", C.c_int32),
                ("rows_total", C.c_int32), ("rows_removed", C.c_int32),
                ("capacity_ok", C.c_int32)] + [
        (f, C.c_void_p) for f in ("H", "Z", "Xs", "Pr", "Qs", "Qt", "Ks", "Kt", "G", "Gs", "lo",
                                  "hi", "Cs", "clo", "chi", "UZ0", "US0")]


def host_operators(cfg: dict, keep_redundant: bool = False) -> dict:
    """Host-only condensed operators (mpccbf_host_operators); no GPU needed."""
    L = load()
    L.mpccbf_host_operators.argtypes = [C.POINTER(Params), C.c_int32, C.POINTER(HostOps)]
    L.mpccbf_host_last_error.restype = C.c_char_p
    p = Params.from_dict(cfg)
    o = HostOps(capacity_ok=0)
    rc = L.mpccbf_host_operators(C.byref(p), int(keep_redundant), C.byref(o))
    if rc != 0:
        raise MpccbfError(L.mpccbf_host_last_error().decode())
    n, nz, m, mc = o.n, o.nz, o.m, o.mc
    shapes = dict(H=(n, n), Z=(n, nz), Xs=(n, 6), Pr=(nz, nz), Qs=(nz, 6), Qt=(nz, 3),
                  Ks=(6, 6), Kt=(3, 6), G=(m, nz), Gs=(m, 6), lo=(m,), hi=(m,), Cs=(mc, 6),
                  clo=(mc,), chi=(mc,), UZ0=(3, nz), US0=(3, 6))
    arrs = {k: np.zeros(s) for k, s in shapes.items()}
    o.capacity_ok = 1
    for k, a in arrs.items():
        setattr(o, k, a.ctypes.data if a.size else None)
    rc = L.mpccbf_host_operators(C.byref(p), int(keep_redundant), C.byref(o))
    if rc != 0:
        raise MpccbfError(L.mpccbf_host_last_error().decode())
    arrs.update(n=n, nz=nz, m=m, mc=mc, rows_total=o.rows_total, rows_removed=o.rows_removed)
    return arrs


HOST_PLAN_OFFSETS = 38


class HostPlan(C.Structure):
    _fields_ = [("kernel_name", C.c_char_p), ("capacity_name", C.c_char_p)] + [
        (f, C.c_int32) for f in ("block_size", "agents_per_block", "clock_waves", "store", "defers", "hot",
                                 "total", "wide_capacity", "sep", "sep_rows_per_dim", "sep_sb", "o_Gsep")] + [
        ("offsets", C.c_int32 * HOST_PLAN_OFFSETS), ("buf", C.c_void_p), ("buf_capacity", C.c_int32)]


def host_launch_plan(cfg: dict, variant: int = 0, num_agents: int = 0, csr: bool = False, knn_k: int = 0,
                     store: bool = False, connectivity: bool = False, wide_max: int = 1024,
                     with_buffer: bool = False, launch: dict = None, **options) -> dict:
    """Host-only launch plan and operator packing (mpccbf_host_launch_plan); no GPU needed.
    options: fields of mpccbf_options (lean=1, keep_redundant=1, ...). Returns the fields of
    mpccbf_host_plan as a dict (names decoded, offsets a list; buf: the packed operators as a numpy
    array when with_buffer). launch: the launch-uniform options (keys of LAUNCH_FACTS -> bool, e.g.
    LOOP_LAUNCH; default: none given) — the dict then also has the main launch's kernel_id, its
    launch_form ("generic" / "loop") and, for that launch, kernel_name (mpccbf_host_launch_form)."""
    L = load()
    L.mpccbf_host_launch_plan.argtypes = [C.POINTER(Params), C.POINTER(Options)] + [C.c_int32] * 7 + [
        C.POINTER(HostPlan)]
    L.mpccbf_host_last_error.restype = C.c_char_p
    p, o, out = Params.from_dict(cfg), Options(**options), HostPlan()
    args = (C.byref(p), C.byref(o), int(variant), int(num_agents), int(csr), int(knn_k), int(store),
            int(connectivity), int(wide_max), C.byref(out))
    buf = None
    for _ in range(2 if with_buffer else 1):
        if L.mpccbf_host_launch_plan(*args) != 0:
            raise MpccbfError(L.mpccbf_host_last_error().decode())
        if with_buffer and buf is None:
            buf = np.zeros(out.total)
            out.buf, out.buf_capacity = buf.ctypes.data, out.total
    r = {f: getattr(out, f) for f, _ in HostPlan._fields_ if f not in ("offsets", "buf", "buf_capacity")}
    r.update(kernel_name=out.kernel_name.decode(), capacity_name=out.capacity_name.decode(),
             offsets=list(out.offsets), buf=buf)
    if launch is not None:
        unknown = set(launch) - set(LAUNCH_FACTS)
        if unknown:
            raise ValueError(f"unknown launch facts: {sorted(unknown)}")
        mask = sum(1 << i for i, f in enumerate(LAUNCH_FACTS) if launch.get(f))
        L.mpccbf_host_launch_form.argtypes = [C.POINTER(Params), C.POINTER(Options)] + [C.c_int32] * 7 + [
            C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
        kid, name, form = C.c_int32(), C.c_char_p(), C.c_char_p()
        if L.mpccbf_host_launch_form(*args[:-1], mask, C.byref(kid), C.byref(name), C.byref(form)) != 0:
            raise MpccbfError(L.mpccbf_host_last_error().decode())
        r.update(kernel_id=kid.value, kernel_name=name.value.decode(), launch_form=form.value.decode())
    return r


def dense_qp_solve(H, c, A, lo, hi, vlo=None, vhi=None, c0=0.0):
    """Generic dense QP (mpccbf_qp_solve_dense); host numpy arrays. Returns (status, x, obj)."""
    L = load()
    H = np.ascontiguousarray(H, dtype=np.float64)
    c = np.ascontiguousarray(c, dtype=np.float64)
    n = c.shape[0]
    A = np.ascontiguousarray(A, dtype=np.float64).reshape(-1, n)
    lo = np.ascontiguousarray(lo, dtype=np.float64)
    hi = np.ascontiguousarray(hi, dtype=np.float64)
    vlo_a = None if vlo is None else np.ascontiguousarray(vlo, dtype=np.float64)
    vhi_a = None if vhi is None else np.ascontiguousarray(vhi, dtype=np.float64)
    qp = DenseQP(n=n, m=A.shape[0], H=H.ctypes.data, c=c.ctypes.data, c0=c0, A=A.ctypes.data,
                 lo=lo.ctypes.data, hi=hi.ctypes.data,
                 vlo=None if vlo_a is None else vlo_a.ctypes.data,
                 vhi=None if vhi_a is None else vhi_a.ctypes.data)
    x = np.zeros(n)
    obj = np.zeros(1)
    st = np.zeros(1, dtype=np.int32)
    _check(L.mpccbf_qp_solve_dense(C.byref(qp), x.ctypes.data, obj.ctypes.data, st.ctypes.data))
    return int(st[0]), x, float(obj[0])


class DenseBatchCall:
    """A batch of generic dense QPs marshalled once into the C ABI's mpccbf_dense_qp array (what a
    C++ caller holds anyway: pointers to its own arrays); run() is one
    mpccbf_qp_solve_dense_batch call on them. qps: list of dicts with H, c, A, lo, hi and
    optional vlo, vhi, c0."""

    def __init__(self, qps):
        self.L = load()
        self.keep = []  # hold the arrays alive for the calls
        self.count = len(qps)
        self.arr = (DenseQP * max(self.count, 1))()
        self.xs = []
        for k, q in enumerate(qps):
            c = np.ascontiguousarray(q["c"], dtype=np.float64)
            n = c.shape[0]
            H = np.ascontiguousarray(q["H"], dtype=np.float64).reshape(n, n)
            A = np.ascontiguousarray(q.get("A", np.zeros((0, n))), dtype=np.float64).reshape(-1, n)
            lo = np.ascontiguousarray(q.get("lo", np.zeros(0)), dtype=np.float64)
            hi = np.ascontiguousarray(q.get("hi", np.zeros(0)), dtype=np.float64)
            vlo = q.get("vlo")
            vhi = q.get("vhi")
            vlo = None if vlo is None else np.ascontiguousarray(vlo, dtype=np.float64)
            vhi = None if vhi is None else np.ascontiguousarray(vhi, dtype=np.float64)
            self.keep += [c, H, A, lo, hi, vlo, vhi]
            self.arr[k] = DenseQP(n=n, m=A.shape[0], H=H.ctypes.data, c=c.ctypes.data, c0=q.get("c0", 0.0),
                                  A=A.ctypes.data if A.size else None, lo=lo.ctypes.data if lo.size else None,
                                  hi=hi.ctypes.data if hi.size else None,
                                  vlo=None if vlo is None else vlo.ctypes.data,
                                  vhi=None if vhi is None else vhi.ctypes.data)
            self.xs.append(np.full(n, np.nan))
        self.xptr = (C.c_void_p * max(self.count, 1))(*[x.ctypes.data for x in self.xs])
        self.obj = np.zeros(max(self.count, 1))
        self.st = np.zeros(max(self.count, 1), dtype=np.int32)

    def run(self):
        """Returns (status[count], list of x (None unless OPTIMAL), obj[count])."""
        for x in self.xs:
            x.fill(np.nan)
        _check(self.L.mpccbf_qp_solve_dense_batch(self.count, self.arr, C.cast(self.xptr, C.c_void_p),
                                                  self.obj.ctypes.data, self.st.ctypes.data))
        n = self.count
        return (self.st[:n].copy(), [self.xs[k].copy() if self.st[k] == 0 else None for k in range(n)],
                self.obj[:n].copy())

    def run_raw(self):
        """The C call alone (outputs stay in self.st / self.obj / self.xs)."""
        _check(self.L.mpccbf_qp_solve_dense_batch(self.count, self.arr, C.cast(self.xptr, C.c_void_p),
                                                  self.obj.ctypes.data, self.st.ctypes.data))


def dense_qp_solve_batch(qps):
    """Batched generic dense QPs (mpccbf_qp_solve_dense_batch): one launch for all of them.
    qps: list of dicts with H, c, A, lo, hi and optional vlo, vhi, c0. Returns
    (status[count], list of x (None unless OPTIMAL), obj[count])."""
    return DenseBatchCall(qps).run()


COMM_ID_BYTES = 128


class FovControlParams(C.Structure):
    _fields_ = [("fov", C.c_double), ("Ds", C.c_double), ("Rs", C.c_double),
                ("v_min", C.c_double * 3), ("v_max", C.c_double * 3),
                ("u_min", C.c_double * 3), ("u_max", C.c_double * 3),
                ("slack_mode", C.c_int32), ("slack_cost", C.c_double),
                ("slack_decay_rate", C.c_double), ("max_pdip_iters", C.c_int32),
                ("tolerance", C.c_double)]


class FovControlBatch(C.Structure):
    _fields_ = [("num_agents", C.c_int32), ("states", C.c_void_p), ("desired_u", C.c_void_p),
                ("nb_row_ptr", C.c_void_p), ("nb_xy", C.c_void_p), ("u", C.c_void_p),
                ("status", C.c_void_p), ("obj", C.c_void_p), ("iters", C.c_void_p),
                ("nb_cov", C.c_void_p)]


def fov_control_params(cfg: dict) -> FovControlParams:
    """FovControl parameters from a config dict: fov_beta / fov_Ds / fov_Rs, v_min / v_max and the
    control bounds u_min / u_max (default: the acceleration bounds a_min / a_max)."""
    p = FovControlParams()
    p.fov, p.Ds, p.Rs = cfg["fov_beta"], cfg["fov_Ds"], cfg["fov_Rs"]
    for d in range(3):
        p.v_min[d], p.v_max[d] = cfg["v_min"][d], cfg["v_max"][d]
        p.u_min[d] = cfg.get("u_min", cfg["a_min"])[d]
        p.u_max[d] = cfg.get("u_max", cfg["a_max"])[d]
    p.slack_mode = int(cfg.get("control_slack_mode", 0))
    p.slack_cost = cfg.get("slack_cost", 0.0)
    p.slack_decay_rate = cfg.get("slack_decay_rate", 1.0)
    return p


def fov_control_solve(cfg: dict, states, desired_u, nb_row_ptr, nb_xy, u, status=None, obj=None,
                      iters=None, device: int = 0, stream=None, nb_cov=None):
    """Batched FovControl::optimize (mpccbf_fov_control_solve): device tensors in, u out.
    Slack mode: cfg["control_slack_mode"] with slack_cost / slack_decay_rate; nb_cov (one
    (cxx, cxy, cyy) row per observed neighbour) orders the slack weights."""
    b = FovControlBatch(num_agents=states.shape[0], states=_ptr(states), desired_u=_ptr(desired_u),
                        nb_row_ptr=_ptr(nb_row_ptr), nb_xy=_ptr(nb_xy), u=_ptr(u),
                        status=_ptr(status), obj=_ptr(obj), iters=_ptr(iters), nb_cov=_ptr(nb_cov))
    p = fov_control_params(cfg)
    _check(load().mpccbf_fov_control_solve(C.byref(p), C.byref(b), device, _stream(stream)))


class PfParams(C.Structure):
    _fields_ = [("num_particles", C.c_int32), ("init_cov", C.c_double * 3), ("process", C.c_double * 4),
                ("meas_cov", C.c_double * 3), ("dt", C.c_double), ("fov", C.c_double), ("Rs", C.c_double),
                ("weight_reduction", C.c_double), ("seed", C.c_uint64)]


class PfBatch(C.Structure):
    _fields_ = [("num_states", C.c_int32), ("states", C.c_void_p), ("agent_first", C.c_int32),
                ("num_agents", C.c_int32), ("nb_row_ptr", C.c_void_p), ("nb_col", C.c_void_p),
                ("num_pairs", C.c_int32), ("input", C.c_void_p), ("init_xy", C.c_void_p),
                ("particles", C.c_void_p), ("weights", C.c_void_p), ("est_xy", C.c_void_p),
                ("est_cov", C.c_void_p), ("flags", C.c_void_p), ("ancestors", C.c_void_p),
                ("step_index", C.c_int64)]


def pf_params(cfg: dict, seed: int = 0) -> PfParams:
    """Particle-filter parameters from a config dict: fov_beta / fov_Rs and the optional keys
    pf_num_particles, pf_init_cov, pf_process, pf_meas_cov ((cxx, cxy, cyy) / row-major 2 x 2 W),
    pf_dt, pf_weight_reduction. Defaults: CBFControl_example.cpp:96-99 (100 particles, 1.0 I,
    0.25 I, 0.05 I), the filter's dt 0.2 (particle_filter.cpp:19) and a reduction of 10."""
    p = PfParams()
    p.num_particles = int(cfg.get("pf_num_particles", 100))
    for name, key, default in (("init_cov", "pf_init_cov", (1.0, 0.0, 1.0)),
                               ("process", "pf_process", (0.25, 0.0, 0.0, 0.25)),
                               ("meas_cov", "pf_meas_cov", (0.05, 0.0, 0.05))):
        arr = getattr(p, name)
        vals = cfg.get(key, default)
        if len(vals) != len(arr):
            raise ValueError(f"{key} needs {len(arr)} entries")
        for i, v in enumerate(vals):
            arr[i] = float(v)
    p.dt = float(cfg.get("pf_dt", 0.2))
    p.fov, p.Rs = float(cfg["fov_beta"]), float(cfg["fov_Rs"])
    p.weight_reduction = float(cfg.get("pf_weight_reduction", 10.0))
    p.seed = int(seed) & ((1 << 64) - 1)
    return p


def _pf_call(fn_name, params, states, nb_row_ptr, nb_col, num_pairs, particles, weights, est_xy, est_cov,
             agent_first, num_agents, input, init_xy, flags, ancestors, step_index, device, stream):
    fn = getattr(load(), fn_name)
    if num_agents is None:
        num_agents = states.shape[0] - agent_first
    b = PfBatch(num_states=states.shape[0], states=_ptr(states), agent_first=int(agent_first),
                num_agents=int(num_agents), nb_row_ptr=_ptr(nb_row_ptr), nb_col=_ptr(nb_col),
                num_pairs=int(num_pairs), input=_ptr(input), init_xy=_ptr(init_xy),
                particles=_ptr(particles), weights=_ptr(weights), est_xy=_ptr(est_xy),
                est_cov=_ptr(est_cov), flags=_ptr(flags), ancestors=_ptr(ancestors),
                step_index=int(step_index))
    _check(fn(C.byref(params), C.byref(b), int(device), _stream(stream)))


def pf_init(params: PfParams, states, nb_row_ptr, nb_col, num_pairs, particles, weights, est_xy, est_cov,
            agent_first=0, num_agents=None, init_xy=None, flags=None, step_index=0, device: int = 0,
            stream=None):
    """Batched ParticleFilter::init (mpccbf_pf_init): one filter per CSR entry of nb_row_ptr / nb_col
    (device tensors; observer agent_first + i holds the pairs nb_row_ptr[i] .. nb_row_ptr[i+1]-1, which
    index particles (pairs x 2 x P), weights (pairs x P), est_xy (pairs x 2), est_cov (pairs x 3) and
    flags); num_pairs = the pairs of this call (host integer)."""
    _pf_call("mpccbf_pf_init", params, states, nb_row_ptr, nb_col, num_pairs, particles, weights, est_xy,
             est_cov, agent_first, num_agents, None, init_xy, flags, None, step_index, device, stream)


def pf_step(params: PfParams, states, nb_row_ptr, nb_col, num_pairs, particles, weights, est_xy, est_cov,
            agent_first=0, num_agents=None, input=None, flags=None, ancestors=None, step_index=0,
            device: int = 0, stream=None):
    """Batched PFApplications::processFovUpdate (mpccbf_pf_step): predict, negative information,
    measurement update of the visible neighbours, resampling, estimate; arguments as pf_init, input
    (pairs x 2) the optional per-pair motion input, ancestors (pairs x P int32) the resampling's
    choices. est_xy / est_cov have the row formats of fov_control_solve's nb_xy / nb_cov."""
    _pf_call("mpccbf_pf_step", params, states, nb_row_ptr, nb_col, num_pairs, particles, weights, est_xy,
             est_cov, agent_first, num_agents, input, None, flags, ancestors, step_index, device, stream)


def fov_rows_eval(ego, nb_xy, fov: float, Ds: float, Rs: float, bbox=(0.0, 0.0, 0.0), stream=None):
    """The FoV controller's per-neighbour rows on the device (mpccbf_fov_rows_eval): ego (n x 6)
    and nb_xy (n x 2) device tensors -> (voronoi n x 4 = (nx, ny, 0, offset), fov rows n x 4 x 4 =
    (a0, a1, a2, b) per kind: safety, left, right, range)."""
    import torch
    n = ego.shape[0]
    vor = torch.empty((n, 4), dtype=torch.float64, device=ego.device)
    rows = torch.empty((n, 4, 4), dtype=torch.float64, device=ego.device)
    bb = (C.c_double * 3)(*bbox)
    _check(load().mpccbf_fov_rows_eval(n, _ptr(ego), _ptr(nb_xy), fov, Ds, Rs, C.cast(bb, C.c_void_p),
                                       _ptr(vor), _ptr(rows), _stream(stream)))
    return vor, rows


class ConnControlParams(C.Structure):
    _fields_ = [("d_min", C.c_double), ("d_max", C.c_double), ("v_min", C.c_double * 3),
                ("v_max", C.c_double * 3), ("slack_mode", C.c_int32), ("slack_cost", C.c_double),
                ("slack_decay_rate", C.c_double), ("max_pdip_iters", C.c_int32),
                ("tolerance", C.c_double)]


class ConnControlBatch(C.Structure):
    _fields_ = [("num_teams", C.c_int32), ("team_ptr", C.c_void_p), ("states", C.c_void_p),
                ("desired_u", C.c_void_p), ("u", C.c_void_p), ("status", C.c_void_p),
                ("obj", C.c_void_p), ("iters", C.c_void_p), ("lambda2", C.c_void_p)]


def conn_control_params(cfg: dict) -> ConnControlParams:
    """The connectivity controller's parameters from a config dict: d_min, d_max, v_min, v_max,
    control_slack_mode, slack_cost, slack_decay_rate."""
    p = ConnControlParams()
    p.d_min, p.d_max = cfg["d_min"], cfg["d_max"]
    for d in range(3):
        p.v_min[d], p.v_max[d] = cfg["v_min"][d], cfg["v_max"][d]
    p.slack_mode = int(cfg.get("control_slack_mode", 0))
    p.slack_cost = cfg.get("slack_cost", 0.0)
    p.slack_decay_rate = cfg.get("slack_decay_rate", 1.0)
    return p


def connectivity_control_solve(cfg: dict, team_ptr, states, desired_u, u, status=None, obj=None,
                               iters=None, lambda2=None, device: int = 0, stream=None):
    """Batched ConnectivityControl::optimize (mpccbf_connectivity_control_solve) for teams of
    robots (team t = rows team_ptr[t] .. team_ptr[t+1]-1 of states / desired_u). cfg keys: d_min,
    d_max, v_min, v_max, control_slack_mode, slack_cost, slack_decay_rate."""
    p = conn_control_params(cfg)
    b = ConnControlBatch(num_teams=team_ptr.shape[0] - 1, team_ptr=_ptr(team_ptr),
                         states=_ptr(states), desired_u=_ptr(desired_u), u=_ptr(u),
                         status=_ptr(status), obj=_ptr(obj), iters=_ptr(iters),
                         lambda2=_ptr(lambda2))
    _check(load().mpccbf_connectivity_control_solve(C.byref(p), C.byref(b), device, _stream(stream)))


FORMATION_STEPS_PER_LAUNCH = 2  # MPCCBF_FORMATION_STEPS_PER_LAUNCH


class FormationParams(C.Structure):
    _fields_ = [("Ts", C.c_double), ("spring_constant", C.c_double), ("pos_std", C.c_double),
                ("vel_std", C.c_double), ("shape_half", C.c_double * 2), ("goal_radius", C.c_double),
                ("steps_per_launch", C.c_int32)]


class FormationBatch(C.Structure):
    _fields_ = [("num_teams", C.c_int32), ("team_ptr", C.c_void_p), ("states", C.c_void_p),
                ("targets", C.c_void_p), ("team_seed", C.c_void_p), ("step_first", C.c_int64),
                ("num_steps", C.c_int32), ("trace", C.c_void_p), ("cbf_u", C.c_void_p),
                ("desired_u", C.c_void_p), ("status", C.c_void_p), ("lambda2", C.c_void_p),
                ("iters", C.c_void_p), ("arrival_sample", C.c_void_p), ("first_collision", C.c_void_p),
                ("min_d2", C.c_void_p), ("fail_count", C.c_void_p)]


def formation_rollout(cfg: dict, team_ptr, states, targets, team_seed, num_steps: int, step_first: int = 0, *,
                      Ts: float, spring_constant: float = 0.5, pos_std: float = 0.0, vel_std: float = 0.0,
                      shape_half=(0.2, 0.2), goal_radius: float = 1.0, steps_per_launch: int = 0,
                      trace=None, cbf_u=None, desired_u=None, status=None, lambda2=None, iters=None,
                      arrival_sample=None, first_collision=None, min_d2=None, fail_count=None,
                      device: int = 0, stream=None):
    """The formation-control example's closed loop for a batch of teams on the device
    (mpccbf_formation_rollout): num_steps steps from step_first, robots in index order. Device
    tensors: team_ptr (int32, teams + 1), states (robots x 6, in/out), targets (robots x 3),
    team_seed (int64 holding the uint64 seeds' bits, teams); the optional records
    [num_steps][robots][.] and the in/out summary (arrival_sample int32 robots, first_collision int32
    teams x 3, min_d2 float64 teams, fail_count int32 teams). cfg: the keys of
    connectivity_control_solve."""
    p = conn_control_params(cfg)
    f = FormationParams(Ts=Ts, spring_constant=spring_constant, pos_std=pos_std, vel_std=vel_std,
                        goal_radius=goal_radius, steps_per_launch=int(steps_per_launch))
    f.shape_half[0], f.shape_half[1] = float(shape_half[0]), float(shape_half[1])
    b = FormationBatch(num_teams=team_ptr.shape[0] - 1, team_ptr=_ptr(team_ptr), states=_ptr(states),
                       targets=_ptr(targets), team_seed=_ptr(team_seed), step_first=int(step_first),
                       num_steps=int(num_steps), trace=_ptr(trace), cbf_u=_ptr(cbf_u),
                       desired_u=_ptr(desired_u), status=_ptr(status), lambda2=_ptr(lambda2),
                       iters=_ptr(iters), arrival_sample=_ptr(arrival_sample),
                       first_collision=_ptr(first_collision), min_d2=_ptr(min_d2), fail_count=_ptr(fail_count))
    L = load()
    if not hasattr(L, "mpccbf_formation_rollout"):
        raise MpccbfError(f"{LIB_PATH} has no mpccbf_formation_rollout (a library from before the rollouts)")
    _check(L.mpccbf_formation_rollout(C.byref(p), C.byref(f), C.byref(b), int(device), _stream(stream)))


TEAM_STEPS_PER_LAUNCH = 2  # MPCCBF_TEAM_STEPS_PER_LAUNCH


class TeamRolloutParams(C.Structure):
    _fields_ = [("pos_std", C.c_double), ("vel_std", C.c_double), ("shape_half", C.c_double * 2),
                ("goal_radius", C.c_double), ("steps_per_launch", C.c_int32)]


class TeamBatch(C.Structure):
    _fields_ = [("num_teams", C.c_int32), ("team_ptr", C.c_void_p), ("states", C.c_void_p),
                ("targets", C.c_void_p), ("team_seed", C.c_void_p), ("step_first", C.c_int64),
                ("num_steps", C.c_int32), ("x_keep", C.c_void_p), ("traj_t", C.c_void_p),
                ("status", C.c_void_p), ("obj", C.c_void_p), ("iters", C.c_void_p), ("x", C.c_void_p),
                ("traj_t0", C.c_void_p), ("substeps", C.c_void_p), ("trace", C.c_void_p),
                ("arrival_sample", C.c_void_p), ("first_collision", C.c_void_p), ("min_d2", C.c_void_p),
                ("fail_count", C.c_void_p)]


def team_rollout(ctx, team_ptr, states, targets, team_seed, x_keep, traj_t, num_steps: int, step_first: int = 0, *,
                 pos_std: float = 0.0, vel_std: float = 0.0, shape_half=(0.2, 0.2), goal_radius: float = 1.0,
                 steps_per_launch: int = 0, status=None, obj=None, iters=None, x=None, traj_t0=None,
                 substeps=None, trace=None, arrival_sample=None, first_collision=None, min_d2=None,
                 fail_count=None, stream=None):
    """The MPC-CBF example's closed loop for a batch of teams on the device (mpccbf_team_rollout) with
    the operators of the Context `ctx`: num_steps steps from step_first, robots in index order.
    Device tensors: team_ptr (int32, teams + 1), states (robots x 6, in/out), targets (robots x 3),
    team_seed (int64 holding the uint64 seeds' bits, teams), x_keep (robots x ctx.n, in/out, NaN = no
    curve), traj_t (robots, in/out, -1 = none); the optional records [num_steps][robots][.] and the
    in/out summary (arrival_sample int32 robots, first_collision int32 teams x 3, min_d2 float64
    teams, fail_count int32 teams)."""
    p = TeamRolloutParams(pos_std=pos_std, vel_std=vel_std, goal_radius=goal_radius,
                          steps_per_launch=int(steps_per_launch))
    p.shape_half[0], p.shape_half[1] = float(shape_half[0]), float(shape_half[1])
    b = TeamBatch(num_teams=team_ptr.shape[0] - 1, team_ptr=_ptr(team_ptr), states=_ptr(states),
                  targets=_ptr(targets), team_seed=_ptr(team_seed), step_first=int(step_first),
                  num_steps=int(num_steps), x_keep=_ptr(x_keep), traj_t=_ptr(traj_t), status=_ptr(status),
                  obj=_ptr(obj), iters=_ptr(iters), x=_ptr(x), traj_t0=_ptr(traj_t0), substeps=_ptr(substeps),
                  trace=_ptr(trace), arrival_sample=_ptr(arrival_sample), first_collision=_ptr(first_collision),
                  min_d2=_ptr(min_d2), fail_count=_ptr(fail_count))
    L = load()
    if not hasattr(L, "mpccbf_team_rollout"):
        raise MpccbfError(f"{LIB_PATH} has no mpccbf_team_rollout (a library from before the team rollouts)")
    _check(L.mpccbf_team_rollout(ctx._h, C.byref(p), C.byref(b), _stream(stream)))


def comm_unique_id() -> bytes:
    """RCCL unique id (mpccbf_comm_unique_id), created on one rank and shared with the others."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(load().mpccbf_comm_unique_id(buf))
    return buf.raw


class Comm:
    """RCCL communicator for the per-step all-gather of agent states (mpccbf_comm_create):
    collective — every rank constructs it with the same id."""

    def __init__(self, uid: bytes, nranks: int, rank: int, device: int, _handle=None):
        if _handle is not None:
            self.handle, self.nranks, self.rank = _handle, nranks, rank
            return
        if len(uid) != COMM_ID_BYTES:
            raise ValueError("communicator id must be 128 bytes")
        h = C.c_void_p()
        _check(load().mpccbf_comm_create(uid, nranks, rank, device, C.byref(h)))
        self.handle = h
        self.nranks, self.rank = nranks, rank

    @classmethod
    def local_group(cls, nranks: int, device: int = 0) -> list:
        """mpccbf_comm_create_local: nranks in-process communicators (one host thread per rank,
        one device), the multi-GPU data flow of mpccbf_run_steps on a single GPU."""
        hs = (C.c_void_p * nranks)()
        _check(load().mpccbf_comm_create_local(nranks, device, hs))
        return [cls(b"", nranks, r, device, _handle=C.c_void_p(hs[r])) for r in range(nranks)]

    def close(self):
        if getattr(self, "handle", None):
            load().mpccbf_comm_destroy(self.handle)
            self.handle = None
