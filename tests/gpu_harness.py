"""What the GPU tests share on the device side: the device guard, host <-> device conversion,
pre-filled outputs, one solve against the oracle's inputs, and the torch front ends of the identity
rules of parity_rule.py. torch is imported inside the functions, so CPU tests can import this."""
import numpy as np
import pytest

import parity_rule as PR

NAN_OR_M7 = (float("nan"), -7)  # what a launch leaves unwritten compares equal on both sides


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test needs a visible MI355X")
    return torch


def to_device(a, dtype=None, device=None):
    """A host array as a contiguous device tensor of the same dtype (or `dtype`); an empty array
    becomes a one-element placeholder (the library wants a valid pointer for an empty nb_col)."""
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros(1, a.dtype)
    return torch.tensor(a, dtype=dtype, device=torch.device("cuda", 0) if device is None else device)


def to_host(out):
    """A dict of device tensors (None entries left out) as host arrays."""
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def fresh_outputs(ctx, n, nb_out=False, guard=0, fill=NAN_OR_M7):
    """ctx.alloc_outputs(n) pre-filled with a sentinel: fill is one value for every buffer or
    (floating-point fill, integer fill). nb_out: an (n, 16) int32 "nb_out" as well. guard > 0: the
    outputs are the leading n rows of buffers `guard` rows longer, and (views, full) is returned."""
    import torch
    ffill, ifill = fill if isinstance(fill, tuple) else (fill, fill)
    full = ctx.alloc_outputs(n + guard)
    if nb_out:
        full["nb_out"] = torch.empty((n + guard, 16), dtype=torch.int32, device=full["x"].device)
    for v in full.values():
        v.fill_(ffill if v.is_floating_point() else ifill)
    return ({k: v[:n] for k, v in full.items()}, full) if guard else full


def run_gpu(ctx, states, targets, row_ptr, col, torch, cov=None, refs=None):
    """refs (n x 3 k_hor): passed as mpccbf_batch.refs in place of the replicated targets."""
    dev = torch.device("cuda", 0)
    st = torch.tensor(states, dtype=torch.float64, device=dev)
    tg = None if refs is not None else torch.tensor(targets, dtype=torch.float64, device=dev)
    rf = None if refs is None else torch.tensor(refs, dtype=torch.float64, device=dev)
    rp = torch.tensor(row_ptr, dtype=torch.int32, device=dev)
    cl = to_device(col, torch.int32)
    out = ctx.alloc_outputs(len(states))
    cv = None if cov is None else torch.tensor(cov, dtype=torch.float64, device=dev)
    ctx.impc_solve(st, rp, cl, targets=tg, refs=rf, cov=cv, **out)
    torch.cuda.synchronize()
    return to_host(out)


def run_oracle(cfg, states, targets, row_ptr, col, agents, cov=None, refs=None):
    import oracle_lib as O
    from mpccbf import swarm
    p = O.make_params(cfg)
    if refs is None:
        refs = swarm.refs_from_targets(targets, cfg["k_hor"])
    res = []
    for a in agents:
        res.append(O.impc_optimize(p, states, a, col[row_ptr[a]:row_ptr[a + 1]], refs[a], covs=cov))
    return res


def _manual_loop(ctx, st0, tg, steps, first, count, torch):
    a = st0.clone()
    b = st0.clone()
    out = ctx.alloc_outputs(count)
    for _ in range(steps):
        b.copy_(a)  # rows outside the batch carry over
        ctx.impc_solve(a, targets=tg, agent_first=first, num_agents=count, knn_k=8, knn_radius=6.0,
                       x=out["x"], status=out["status"], obj=out["obj"], iters=out["iters"],
                       next_states=b[first:first + count])
        a, b = b, a
    torch.cuda.synchronize()
    return a.cpu().numpy(), out["status"].cpu().numpy()


class Solver:
    """One FoV case on one context: the device copies of its tables (and of its per-pair estimates
    nb_xy / nb_cov where the case has them) and a solve that returns fresh, pre-filled outputs.
    kernel_names: {"plain": ..., "slack": ...}; given, every solve asserts the kernel the launch
    took (solve's `kernel`: another expected name, the estimate form's)."""

    def __init__(self, mpclib, cfg, case, kernel_names=None, **opts):
        self.torch = require_gpu()
        self.cfg = cfg
        self.kernel_names = kernel_names
        self.ctx = mpclib.Context(cfg, **opts)
        self.case = c = case
        self.states = to_device(c["states"])
        self.targets = to_device(c["targets"])
        self.rp = to_device(c["rp"], self.torch.int32)
        self.col = to_device(c["col"], self.torch.int32)
        if "nb_xy" in c:
            self.nb_xy = to_device(c["nb_xy"])
            self.nb_cov = to_device(c["nb_cov"])

    def solve(self, cov=None, grid=False, kernel=None):
        """cov: a host array or a device tensor. grid: the device query (8 nearest within Rs)
        in place of the case's lists."""
        c, n = self.case, self.case["num_agents"]
        out = fresh_outputs(self.ctx, n, nb_out=True)
        lists = dict(knn_k=8, knn_radius=self.cfg["fov_Rs"]) if grid else dict(nb_row_ptr=self.rp, nb_col=self.col)
        if cov is not None and not isinstance(cov, self.torch.Tensor):
            cov = to_device(cov)
        self.ctx.impc_solve(self.states, targets=self.targets, agent_first=c["agent_first"], num_agents=n,
                            cov=cov, **lists, **out)
        self.torch.cuda.synchronize()
        if kernel or self.kernel_names:
            want = kernel or self.kernel_names["slack" if self.cfg["slack_mode"] else "plain"]
            assert self.ctx.kernel_name == want, (self.ctx.kernel_name, want)
        return out


def _host(a):
    """Tensors, host arrays, or dicts of either, on the host."""
    if isinstance(a, dict):
        return {k: _host(v) for k, v in a.items() if v is not None}
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def same_bits(a, b, keys=None, what="", rows=None):
    """parity_rule.same_bits on device tensors or dicts of them (rows: a row selection first)."""
    PR.same_bits(*_rows(_host(a), _host(b), keys, rows), keys=keys, what=what)


def same_values(a, b, keys=None, what="", rows=None):
    """parity_rule.same_values on device tensors or dicts of them."""
    PR.same_values(*_rows(_host(a), _host(b), keys, rows), keys=keys, what=what)


def _rows(a, b, keys, rows):
    if rows is None:
        return a, b
    rows = _host(rows)
    if isinstance(a, dict):
        ks = keys if keys is not None else a
        return {k: a[k][rows] for k in ks}, {k: b[k][rows] for k in ks}
    return a[rows], b[rows]
