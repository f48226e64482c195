"""What planning from per-observer estimates costs (Context.set_fov_estimates / set_fov_estimator):
event-timed FoV IMPC launches at BASELINE config 5's per-GPU shape, 512 agents x (up to) 8 visible
neighbours from caller lists, in both slack settings:

  unattached   impc_fov_kernel<SLACK> on the state table's positions (today's launch);
  attached     impc_fov_kernel<SLACK, true> on estimates 0.2 m off the true positions with random
               covariances;
  filter step  one mpccbf_run_steps step with the estimator attached (100 particles): the filter's
               launch and the IMPC launch, device time of the whole step and of the IMPC kernel alone.

Per launch kind: a warm-up, then `launches` launches each between its own pair of events (median /
p10 / p90); the run_steps figures are medians over the steps of one closed-loop call after its first
ten, next to the same closed loop unattached (true positions, covariances 0.1 I): the loop's QPs
are harder than the first step's, with or without estimates. The profiler is off. With --parent-lib
(a libmpccbf.so built from the parent commit) the unattached launch is measured on both libraries in
fresh processes, alternating parent, this, `rounds` times: the parent figures' spread is the noise
the unattached launch has to sit inside. One JSON line per process goes to
profiles/fov_estimates_measure.jsonl. Needs a GPU (no fallback).

    python tools/fov_est_measure.py [--launches 500] [--parent-lib PATH] [--rounds 3] [--out FILE]
"""
import argparse
import json
import math
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mpc-cbf_amd"))

N, K, PARTICLES = 512, 8, 100
SETTINGS = {"plain": {}, "slack": dict(slack_mode=1, slack_cost=1000.0, slack_decay_rate=0.9)}


def _stats(us):
    return dict(median=float(np.median(us)), p10=float(np.percentile(us, 10)), p90=float(np.percentile(us, 90)))


def _time_launches(torch, fn, launches):
    for _ in range(100):  # warm-up: the code object, the clocks
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return _stats(np.array([a.elapsed_time(b) for a, b in ev]) * 1e3)


def measure(tag, launches):
    import torch
    import mpccbf
    from mpccbf import swarm
    if not torch.cuda.is_available():
        sys.exit("fov_est_measure needs a GPU")
    has_est = hasattr(mpccbf.load(), "mpccbf_set_fov_estimates")
    dev = torch.device("cuda", 0)
    states, targets = swarm.heading_swarm(N)
    rp, col = swarm.fov_csr(states, K, 6.0, 2.0 * math.pi / 3.0)
    pairs = int(rp[-1])
    rng = np.random.default_rng(7)
    nb_xy = states[col, :2] + 0.2 * rng.normal(size=(pairs, 2))
    var = rng.uniform(0.02, 0.3, size=(pairs, 2))
    nb_cov = np.stack([var[:, 0], np.zeros(pairs), var[:, 1]], axis=1)
    t = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)  # noqa: E731
    st, tg, d_rp, d_col = t(states), t(targets), t(rp, torch.int32), t(col, torch.int32)
    cov = t(np.tile([0.1, 0.0, 0.1], (N, 1)))
    line = dict(tag=tag, lib=os.path.relpath(mpccbf.LIB_PATH, REPO), agents=N, neighbours=K, pairs=pairs,
                launches=launches, has_estimates=has_est)
    for name, over in SETTINGS.items():
        cfg = swarm.fov_config(20, **over)
        ctx = mpccbf.Context(cfg)
        out = ctx.alloc_outputs(N)
        solve = lambda: ctx.impc_solve(st, nb_row_ptr=d_rp, nb_col=d_col, targets=tg, cov=cov, **out)  # noqa: E731
        res = dict(unattached_us=_time_launches(torch, solve, launches), unattached_kernel=ctx.kernel_name)
        steps = 60

        def closed_loop():  # one run_steps call from the initial swarm; (step, IMPC kernel) times in us
            a, b = st.clone(), torch.empty_like(st)
            traj_t = torch.full((N,), -1.0, dtype=torch.float64, device=dev)
            out["x"].fill_(float("nan"))
            r = ctx.prepare_run_steps(a, b, steps, targets=tg, nb_row_ptr=d_rp, nb_col=d_col, x=out["x"],
                                      status=out["status"], obj=out["obj"], iters=out["iters"], traj_t=traj_t,
                                      cov=cov, pos_std=0.001, vel_std=0.01, noise_seed=1, timing=True)()
            return _stats(r["step_ms"][10:] * 1e3), _stats(r["solve_ms"][10:] * 1e3)

        res["unattached_loop_step_us"], res["unattached_loop_impc_kernel_us"] = closed_loop()
        if has_est:
            ctx.set_fov_estimates(t(nb_xy), t(nb_cov))
            res["attached_us"] = _time_launches(torch, solve, launches)
            res["attached_kernel"] = ctx.kernel_name
            res["attached_optimal_share"] = float((out["status"] == 0).double().mean().item())
            # one run_steps step with the filter in the loop
            est = mpccbf.FovEstimator(dict(cfg, pf_num_particles=PARTICLES), rp, col, N, seed=1)
            est.init(st)
            ctx.set_fov_estimator(est)
            res["filter_step_us"], res["filter_step_impc_kernel_us"] = closed_loop()
            res["filter_step_optimal_share"] = float((out["status"] == 0).double().mean().item())
            res["filter_particles"] = PARTICLES
            ctx.set_fov_estimates(None)
        line[name] = res
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--parent-lib", default=None, help="libmpccbf.so of the parent commit (the comparison basis)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fov_estimates_measure.jsonl"))
    ap.add_argument("--rounds", type=int, default=3, help="alternations of parent and this library")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args.child, args.launches)))
        return
    order = [("this", None)]
    if args.parent_lib:
        order = [(f"{who}-{i + 1}", lib) for i in range(args.rounds) for who, lib in (("parent", args.parent_lib), ("this", None))]
    lines = []
    for tag, lib in order:  # a fresh process per library: one HIP runtime, one libmpccbf each
        env = dict(os.environ)
        env.pop("MPCCBF_LIB", None)
        if lib:
            env["MPCCBF_LIB"] = os.path.abspath(lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tag, "--launches", str(args.launches)],
                           env=env, capture_output=True, text=True, timeout=600)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            sys.exit(f"{tag}: measurement failed\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        lines.append(json.loads(got[-1][len("RESULT "):]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if __name__ == "__main__":
    main()
