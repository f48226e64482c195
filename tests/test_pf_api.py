"""CPU: the argument checks of mpccbf_pf_init / mpccbf_pf_step (made on the host before any device
call, so they need no GPU) and the defaults of pf_params."""
import ctypes as C
import math

import numpy as np
import pytest

from mpccbf import _lib, swarm

INVALID = -1  # MPCCBF_ERR_INVALID_ARGUMENT


def _params(**over):
    cfg = dict(swarm.fov_config(20), **over)
    return _lib.pf_params(cfg, seed=over.get("seed", 0))


def _batch(**over):
    """A well-formed batch over host memory: only ever handed to calls that must refuse it or that
    launch nothing."""
    keep = dict(states=np.zeros((4, 6)), rp=np.array([0, 1, 2], dtype=np.int32), col=np.array([1, 0], dtype=np.int32),
                particles=np.zeros((2, 2, 100)), weights=np.zeros((2, 100)), est_xy=np.zeros((2, 2)),
                est_cov=np.zeros((2, 3)))
    b = _lib.PfBatch(num_states=4, states=keep["states"].ctypes.data, agent_first=0, num_agents=2,
                     nb_row_ptr=keep["rp"].ctypes.data, nb_col=keep["col"].ctypes.data, num_pairs=2,
                     particles=keep["particles"].ctypes.data, weights=keep["weights"].ctypes.data,
                     est_xy=keep["est_xy"].ctypes.data, est_cov=keep["est_cov"].ctypes.data, step_index=0)
    for k, v in over.items():
        setattr(b, k, v)
    b._keep = keep
    return b


def _calls(mpclib):
    L = mpclib.load()
    return [L.mpccbf_pf_init, L.mpccbf_pf_step]


BAD_PARAMS = [
    ("particles_1", dict(pf_num_particles=1)),
    ("particles_0", dict(pf_num_particles=0)),
    ("particles_1025", dict(pf_num_particles=1025)),
    ("init_cov_indefinite", dict(pf_init_cov=(1.0, 2.0, 1.0))),
    ("init_cov_zero", dict(pf_init_cov=(0.0, 0.0, 1.0))),
    ("init_cov_negative", dict(pf_init_cov=(-1.0, 0.0, -1.0))),
    ("init_cov_nan", dict(pf_init_cov=(math.nan, 0.0, 1.0))),
    ("meas_cov_singular", dict(pf_meas_cov=(1.0, 1.0, 1.0))),
    ("meas_cov_negative", dict(pf_meas_cov=(0.05, 0.0, -0.05))),
    ("reduction_zero", dict(pf_weight_reduction=0.0)),
    ("reduction_negative", dict(pf_weight_reduction=-10.0)),
    ("reduction_nan", dict(pf_weight_reduction=math.nan)),
]


@pytest.mark.parametrize("name,over", BAD_PARAMS, ids=[b[0] for b in BAD_PARAMS])
def test_bad_parameters_are_refused(mpclib, name, over):
    p, b = _params(**over), _batch()
    for fn in _calls(mpclib):
        assert fn(C.byref(p), C.byref(b), 0, None) == INVALID
        assert mpclib.load().mpccbf_last_error().decode()


BAD_BATCH = [
    ("num_states_negative", dict(num_states=-1)),
    ("num_agents_negative", dict(num_agents=-1)),
    ("num_pairs_negative", dict(num_pairs=-1)),
    ("agent_first_negative", dict(agent_first=-1)),
    ("agents_beyond_states", dict(agent_first=3)),
    ("null_states", dict(states=None)),
    ("null_row_ptr", dict(nb_row_ptr=None)),
    ("null_col", dict(nb_col=None)),
    ("null_particles", dict(particles=None)),
    ("null_weights", dict(weights=None)),
    ("null_est_xy", dict(est_xy=None)),
    ("null_est_cov", dict(est_cov=None)),
]


@pytest.mark.parametrize("name,over", BAD_BATCH, ids=[b[0] for b in BAD_BATCH])
def test_bad_batches_are_refused(mpclib, name, over):
    p, b = _params(), _batch(**over)
    for fn in _calls(mpclib):
        assert fn(C.byref(p), C.byref(b), 0, None) == INVALID


def test_null_structures_are_refused(mpclib):
    p, b = _params(), _batch()
    for fn in _calls(mpclib):
        assert fn(None, C.byref(b), 0, None) == INVALID
        assert fn(C.byref(p), None, 0, None) == INVALID


def test_zero_sizes_are_successful_no_ops(mpclib):
    p = _params()
    for fn in _calls(mpclib):
        assert fn(C.byref(p), C.byref(_batch(num_pairs=0)), 0, None) == 0
        assert fn(C.byref(p), C.byref(_batch(num_agents=0)), 0, None) == 0
        # nothing is dereferenced: every pointer may be NULL
        empty = _lib.PfBatch(num_states=0, num_agents=0, num_pairs=0)
        assert fn(C.byref(p), C.byref(empty), 0, None) == 0
    # ... but the parameters are still checked
    bad = _params(pf_num_particles=1)
    assert _calls(mpclib)[1](C.byref(bad), C.byref(_batch(num_pairs=0)), 0, None) == INVALID


def test_pf_params_defaults_are_the_examples(mpclib):
    """CBFControl_example.cpp:96-99: 100 particles, initCov 1.0 I, processCov 0.25 I, measCov 0.05 I;
    the filter's dt 0.2 (particle_filter.cpp:19); reduction 10."""
    cfg = swarm.fov_config(20)
    p = _lib.pf_params(cfg)
    assert p.num_particles == 100
    assert list(p.init_cov) == [1.0, 0.0, 1.0]
    assert list(p.process) == [0.25, 0.0, 0.0, 0.25]
    assert list(p.meas_cov) == [0.05, 0.0, 0.05]
    assert p.dt == 0.2 and p.weight_reduction == 10.0 and p.seed == 0
    assert p.fov == cfg["fov_beta"] and p.Rs == cfg["fov_Rs"]
    q = _lib.pf_params(dict(cfg, pf_num_particles=64, pf_process=(0.1, 0.2, 0.3, 0.4), pf_dt=0.1), seed=9)
    assert q.num_particles == 64 and list(q.process) == [0.1, 0.2, 0.3, 0.4] and q.dt == 0.1 and q.seed == 9
    with pytest.raises(ValueError):
        _lib.pf_params(dict(cfg, pf_init_cov=(1.0, 0.0)))


def test_new_names_are_exported(mpclib):
    for name in ("pf_params", "pf_init", "pf_step", "PfParams", "PfBatch", "FovEstimator", "FovControlLoop"):
        assert hasattr(mpclib, name), name
    assert "mpccbf_pf_init" in _lib.EXPORTED and "mpccbf_pf_step" in _lib.EXPORTED
