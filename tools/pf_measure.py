"""What a particle-filter step costs (mpccbf_pf_step, csrc/kernels/pf_fov.hip): event-timed launches
for observers x neighbours x particles = 512 x 8 x 100 (BASELINE config 5's shape), 4096 x 8 x 100
and 512 x 8 x 1024. The observers are a heading swarm (lattice positions, random headings); each
tracks the 8 next rows of the table, so measured and hidden neighbours mix. Per shape: a warm-up,
then `launches` steps each between its own pair of events (median / p10 / p90 of one launch), and
the same number enqueued back to back between one pair (the time per step a control loop sees).
The filters free-run over the launches (step_index advances), the profiler is off. One JSON line
per shape goes to profiles/pf_measure.jsonl with the algorithmic bytes of a step (state read plus
written, from the shapes) over the measured time, next to the FoV IMPC launch the step would
precede (README: 48.3 us). Needs a GPU (no fallback).

    python tools/pf_measure.py [--launches 1000] [--out profiles/pf_measure.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mpc-cbf_amd"))

FOV_IMPC_LAUNCH_US = 48.3  # README, config 5
SHAPES = ((512, 8, 100), (4096, 8, 100), (512, 8, 1024))


def step_bytes(pairs, P):
    """Algorithmic bytes of one step: particles and weights read and written (3 P doubles each
    way), the ancestors (P int32), the estimate (5 doubles), the flag word, and per pair the
    observer's (x, y, yaw) and the neighbour's (x, y)."""
    return pairs * (2 * 3 * P * 8 + P * 4 + 5 * 8 + 4 + 5 * 8)


def measure(mpccbf, torch, observers, k, P, launches):
    from mpccbf import swarm
    cfg = dict(swarm.fov_config(20), pf_num_particles=P)
    states, _ = swarm.heading_swarm(observers, seed=11)
    rp = (np.arange(observers + 1) * k).astype(np.int32)
    col = ((np.arange(observers)[:, None] + 1 + np.arange(k)[None, :]) % observers).astype(np.int32).reshape(-1)
    dev = torch.device("cuda", 0)
    st = torch.tensor(states, dtype=torch.float64, device=dev)
    est = mpccbf.FovEstimator(cfg, rp, col, observers, seed=1)
    est.init(st)
    for _ in range(50):  # warm-up: the code object, the clocks
        est.step(st)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        est.step(st)
        b.record()
    torch.cuda.synchronize()
    single = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        est.step(st)
    b.record()
    torch.cuda.synchronize()
    chained = a.elapsed_time(b) * 1e3 / launches
    flags = est.flags.cpu().numpy()
    pairs = observers * k
    by = step_bytes(pairs, P)
    med = float(np.median(single))
    return dict(observers=observers, neighbours=k, particles=P, pairs=pairs, launches=launches,
                launch_event_us=dict(median=med, p10=float(np.percentile(single, 10)),
                                     p90=float(np.percentile(single, 90))),
                back_to_back_us_per_step=float(chained), step_bytes=by,
                gbytes_per_s_at_median=by / med * 1e-3, lds_bytes_per_block=32 * P,
                measured_share_last_step=float(np.mean(flags & 1)), reset_share_last_step=float(np.mean((flags & 2) > 0)),
                estimates_finite=bool(torch.isfinite(est.est_xy).all().item() and torch.isfinite(est.est_cov).all().item()),
                fov_impc_launch_us=FOV_IMPC_LAUNCH_US, share_of_fov_impc_launch=med / FOV_IMPC_LAUNCH_US)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pf_measure.jsonl"))
    args = ap.parse_args()
    import torch
    import mpccbf
    if not torch.cuda.is_available():
        sys.exit("pf_measure needs a GPU")
    lines = [measure(mpccbf, torch, n, k, P, args.launches) for n, k, P in SHAPES]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if __name__ == "__main__":
    main()
