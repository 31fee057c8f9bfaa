"""What the divergence guard costs per captured fine-tuning step on an MI355X -> profiles/guard_bench.json.

The workload is bench.py's config 3: the S-wn18rr-shaped graph, B = 16, 128 strict negatives, AdamW, one hipGraph replay per step
(engine.GraphedTrainStep).  Variants:
  * off        -- no guard (``guard=None``: the step records and launches what it did before the guard existed)
  * poll_1     -- engine.FiniteGuard(task, poll_every=1): scans + commit inside the graph, one 16-byte read per step
  * poll_100   -- poll_every=100: the same graph, the record read on every 100th step
  * parent_off -- ``off`` run from ANOTHER checkout (``--parent DIR``: the parent commit, built), same box, same run
Every measurement is a fresh child process (one process on the GPU at a time) that times ``--steps`` device-synchronised steps
after 5 warm-up steps and reports their median; the variants are interleaved over ``--rounds`` rounds, and the spread of a
variant's medians over the rounds is the run-to-run spread the differences have to be read against.

    python tools/guard_bench.py [--parent DIR] [--rounds 3] [--steps 200] [--out profiles/guard_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {"off": None, "poll_1": 1, "poll_100": 100}


def measure(root, variant, steps, seed=1024, B=16):
    """Child: median ms per step of ``variant`` with the package and bench.py of ``root``."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import bench
    from ultra_torchdrug_amd import engine
    dev = torch.device("cuda:0")
    task, triples, _, n_fact = bench.transductive_task("S-wn18rr", dev, 512, seed)
    bench.prepare_plans(task)
    facts = torch.from_numpy(triples[:n_fact]).to(dev)
    task.train()
    optimizer = bench.make_optimizer(task)
    pick = np.random.default_rng(seed)
    torch.manual_seed(seed)
    draw = lambda: facts[torch.from_numpy(pick.choice(n_fact, B, replace=False)).to(dev)]
    kwargs = {}
    if VARIANTS[variant] is not None:
        kwargs["guard"] = engine.FiniteGuard(task, poll_every=VARIANTS[variant])
    step = engine.GraphedTrainStep(task, optimizer, draw(), **kwargs)
    batches = [draw() for _ in range(steps + 5)]
    times = []
    for i, batch in enumerate(batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(batch)
        torch.cuda.synchronize()
        if i >= 5:
            times.append(1e3 * (time.perf_counter() - t0))
    scanned = sum(p.numel() for p in task.parameters()) + sum(p.numel() for p in task.parameters() if p.grad is not None) + 1
    print(json.dumps({"variant": variant, "median_ms": float(np.median(times)), "p10_ms": float(np.percentile(times, 10)),
                      "p90_ms": float(np.percentile(times, 90)), "steps": steps, "mode": step.mode,
                      "scanned_bytes_per_step": 4 * scanned if kwargs else 0}), flush=True)


def child(root, variant, steps):
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", variant, "--root", root, "--steps", str(steps)],
                         capture_output=True, text=True, timeout=900)
    lines = [line for line in run.stdout.splitlines() if line.startswith("{")]
    if run.returncode != 0 or not lines:
        raise RuntimeError("guard_bench child %s (%s) failed: %s" % (variant, root, run.stderr[-2000:]))
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guard_bench.json"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (guard-off figure of the code before)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one is not None:
        return measure(os.path.abspath(args.root), args.one, args.steps)
    import torch
    plan = ([("parent_off", os.path.abspath(args.parent), "off")] if args.parent else []) + [(v, ROOT, v) for v in VARIANTS]
    runs = {name: [] for name, _, _ in plan}
    for _ in range(args.rounds):
        for name, root, variant in plan:
            got = child(root, variant, args.steps)
            runs[name].append(got)
            print(name, json.dumps(got), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "workload": "bench.py config 3: S-wn18rr-shaped fine-tuning, B = 16, 128 strict negatives, AdamW, one hipGraph replay "
                       "per step (engine.GraphedTrainStep, mode single)",
           "timing": "per child process: median of %d device-synchronised steps (host clock) after 5 warm-up steps, ms; "
                     "%d rounds, variants interleaved, one process at a time" % (args.steps, args.rounds),
           "variants": {}}
    for name, got in runs.items():
        medians = sorted(g["median_ms"] for g in got)
        out["variants"][name] = {"median_of_rounds_ms": medians[len(medians) // 2], "min_round_ms": medians[0],
                                 "max_round_ms": medians[-1], "rounds": got}
    base = out["variants"]["off"]["median_of_rounds_ms"]
    out["run_to_run_spread_ms"] = max(v["max_round_ms"] - v["min_round_ms"] for v in out["variants"].values())
    for name in ("poll_1", "poll_100"):
        out["variants"][name]["over_off_ms"] = out["variants"][name]["median_of_rounds_ms"] - base
    if args.parent:
        out["off_minus_parent_off_ms"] = base - out["variants"]["parent_off"]["median_of_rounds_ms"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
