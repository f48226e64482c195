"""What the safety monitor costs (Context.set_monitor) and whether the closed-loop launch stays what
it was: event-timed mpccbf_run_steps closed loops, per process

  collision  config 3: 4,096 agents, horizon 15, grid mode (8 nearest within 3 d_min), the launch
             bench.py drives (the loop form); the monitor scores one sample (the next states) per step;
  fov        512 FoV agents, horizon 20, grid mode, with sub-step records (the generic form); the
             monitor scores the step's 10 records.

Per workload: the step time unattached, the step time with the monitor attached (both medians over
the steps of one run_steps call after its first ten, device time between the steps' events), the
monitor's own four operations alone (a warm-up, then `launches` scores each between its own pair of
events) and, as a yardstick for the hash pipeline, mpccbf_build_neighbors on the same table (count,
scan, scatter, query, compact). With --parent-lib (a libmpccbf.so built from the parent commit) the
unattached loop is measured on both libraries in fresh processes, alternating parent, this, `rounds`
times: the unattached step times must agree within the spread of the processes, the evidence that
the hot launch is untouched. The profiler is off. One JSON line per process goes to
profiles/monitor_measure.jsonl. Needs a GPU (no fallback).

    python tools/monitor_measure.py [--launches 300] [--steps 110] [--parent-lib PATH] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mpc-cbf_amd"))

KNN = 8


def _stats(us):
    return dict(median=float(np.median(us)), p10=float(np.percentile(us, 10)), p90=float(np.percentile(us, 90)))


def _time_launches(torch, fn, launches):
    for _ in range(50):  # warm-up: the code object, the clocks
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return _stats(np.array([a.elapsed_time(b) for a, b in ev]) * 1e3)


def _workload(torch, mpccbf, name, steps, launches, has_monitor):
    from mpccbf import swarm
    dev = torch.device("cuda", 0)
    fov = name == "fov"
    if fov:
        n, cfg = 512, swarm.fov_config(20)
        states, targets = swarm.heading_swarm(n)
        radius = cfg["fov_Rs"]
    else:
        n, cfg = 4096, swarm.config(15)
        states, targets = swarm.lattice_swarm(n)
        radius = 3.0 * cfg["d_min"]
    nsub = int(cfg["h"] / cfg["Ts"])
    st = torch.tensor(states, dtype=torch.float64, device=dev)
    tg = torch.tensor(targets, dtype=torch.float64, device=dev)
    ctx = mpccbf.Context(cfg)
    out = ctx.alloc_outputs(n)
    substeps = torch.zeros((n, nsub, 6), dtype=torch.float64, device=dev) if fov else None
    slog = torch.zeros((steps, n, cfg["impc_iter"]), dtype=torch.int32, device=dev)
    ilog = torch.zeros_like(slog)

    def closed_loop():  # one run_steps call from the initial swarm: (step, IMPC kernel) times in us
        a, b = st.clone(), torch.empty_like(st)
        traj_t = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        out["x"].fill_(float("nan"))
        extra = dict(substeps=substeps) if fov else {}
        r = ctx.prepare_run_steps(a, b, steps, targets=tg, knn_k=KNN, knn_radius=radius, x=out["x"],
                                  status=out["status"], obj=out["obj"], iters=out["iters"], status_log=slog,
                                  iters_log=ilog, traj_t=traj_t, pos_std=0.001, vel_std=0.01, noise_seed=1,
                                  timing=True, **extra)()
        return _stats(r["step_ms"][10:] * 1e3), _stats(r["solve_ms"][10:] * 1e3), r["final"]

    res = dict(agents=n, samples_per_step=nsub if fov else 1)
    closed_loop()  # (warm-up: code objects, the context's tables)
    res["unattached_step_us"], res["unattached_impc_kernel_us"], final = closed_loop()
    res["kernel"], res["launch_form"] = ctx.kernel_name, ctx.launch_form
    # the yardstick: the CSR builder's hash pipeline on the final table
    rp = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    col = torch.zeros(n * KNN, dtype=torch.int32, device=dev)
    res["build_neighbors_us"] = _time_launches(
        torch, lambda: ctx.build_neighbors(final, 0, n, KNN, radius, rp, col), launches)
    if has_monitor:
        mon = mpccbf.SafetyMonitor(n, d_min=cfg["d_min"], max_samples=nsub)
        ctx.set_monitor(mon)
        res["attached_step_us"], res["attached_impc_kernel_us"], final = closed_loop()
        res["attached_launch_form"] = ctx.launch_form
        torch.cuda.synchronize()
        res["monitor_result"] = {k: (v if not isinstance(v, float) or np.isfinite(v) else str(v))
                                 for k, v in mon.result().items()}
        ctx.set_monitor(None)
        samples = substeps if fov else final
        res["monitor_score_us"] = _time_launches(torch, lambda: mon.score(samples, goals=tg), launches)
    return res


def measure(tag, steps, launches):
    import torch
    import mpccbf
    if not torch.cuda.is_available():
        sys.exit("monitor_measure needs a GPU")
    has_monitor = hasattr(mpccbf.load(), "mpccbf_set_monitor")
    line = dict(tag=tag, lib=os.path.relpath(mpccbf.LIB_PATH, REPO) if tag.startswith("this") else
                "libmpccbf.so built from the parent commit", steps=steps, launches=launches, has_monitor=has_monitor)
    for name in ("collision", "fov"):
        line[name] = _workload(torch, mpccbf, name, steps, launches, has_monitor)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--steps", type=int, default=110)
    ap.add_argument("--parent-lib", default=None, help="libmpccbf.so of the parent commit (the comparison basis)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "monitor_measure.jsonl"))
    ap.add_argument("--rounds", type=int, default=3, help="alternations of parent and this library")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args.child, args.steps, args.launches)))
        return
    order = [("this-1", None)]
    if args.parent_lib:
        order = [(f"{who}-{i + 1}", lib) for i in range(args.rounds) for who, lib in (("parent", args.parent_lib), ("this", None))]
    lines = []
    for tag, lib in order:  # a fresh process per library: one HIP runtime, one libmpccbf each
        env = dict(os.environ)
        env.pop("MPCCBF_LIB", None)
        if lib:
            env["MPCCBF_LIB"] = os.path.abspath(lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tag, "--launches", str(args.launches),
                            "--steps", str(args.steps)], env=env, capture_output=True, text=True, timeout=300)
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
