"""What a remove_one_hop=True fine-tuning step costs on an MI355X, eager and captured -> profiles/one_hop_bench.json.

The workload is bench.py's config 3 -- the S-wn18rr-shaped graph, B = 16, 128 strict negatives, AdamW -- with an entity model
that drops every edge between a batch's heads and tails (``remove_one_hop=True``, ultra/model.py:57-74).  Variants:
  * parent_eager     -- ``engine.train_step`` from ANOTHER checkout (``--parent DIR``: the parent commit, built): the mask route
                        (``graph.match`` with a wildcard, a host read, a mask over all edges), the only way such a model could train
  * eager            -- ``engine.train_step`` at this commit: the edges go by ``ultra_pair_removal``
  * captured         -- ``engine.GraphedTrainStep`` at this commit: one hipGraph replay per step
  * captured_triples -- the same captured step with ``remove_one_hop=False``: the floor the pair lookup adds to
Every measurement is a fresh child process (one process on the GPU at a time) that times ``--steps`` device-synchronised steps
after 5 warm-up steps and reports their median; the variants are interleaved over ``--rounds`` rounds, and the spread of a
variant's medians over the rounds is the run-to-run spread the differences have to be read against.

    python tools/one_hop_bench.py [--parent DIR] [--rounds 3] [--steps 100] [--out profiles/one_hop_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# variant -> (remove_one_hop, captured)
VARIANTS = {"eager": (True, False), "captured": (True, True), "captured_triples": (False, True)}


def measure(root, variant, steps, seed=1024, B=16):
    """Child: median ms per step of ``variant`` with the package and bench.py of ``root``."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import bench
    from ultra_torchdrug_amd import engine
    one_hop, captured = VARIANTS[variant]
    dev = torch.device("cuda:0")
    task, triples, _, n_fact = bench.transductive_task("S-wn18rr", dev, 512, seed)
    task.model.remove_one_hop = one_hop             # (an attribute the forward reads: set the same way on either checkout)
    bench.prepare_plans(task)
    facts = torch.from_numpy(triples[:n_fact]).to(dev)
    task.train()
    optimizer = bench.make_optimizer(task)
    pick = np.random.default_rng(seed)
    torch.manual_seed(seed)
    draw = lambda: facts[torch.from_numpy(pick.choice(n_fact, B, replace=False)).to(dev)]
    if captured:
        step = engine.GraphedTrainStep(task, optimizer, draw())
    else:
        first = draw()
        step = lambda batch: engine.train_step(task, optimizer, batch)
        step(first)
    batches = [draw() for _ in range(steps + 5)]
    times = []
    for i, batch in enumerate(batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(batch)
        torch.cuda.synchronize()
        if i >= 5:
            times.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps({"variant": variant, "median_ms": float(np.median(times)), "p10_ms": float(np.percentile(times, 10)),
                      "p90_ms": float(np.percentile(times, 90)), "steps": steps, "remove_one_hop": one_hop,
                      "mode": step.mode if captured else "eager"}), flush=True)


def child(root, variant, steps):
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", variant, "--root", root, "--steps", str(steps)],
                         capture_output=True, text=True, timeout=900)
    lines = [line for line in run.stdout.splitlines() if line.startswith("{")]
    if run.returncode != 0 or not lines:
        raise RuntimeError("one_hop_bench child %s (%s) failed: %s" % (variant, root, run.stderr[-2000:]))
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "one_hop_bench.json"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (the eager mask-route step)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one is not None:
        return measure(os.path.abspath(args.root), args.one, args.steps)
    import torch
    plan = ([("parent_eager", os.path.abspath(args.parent), "eager")] if args.parent else []) + [(v, ROOT, v) for v in VARIANTS]
    runs = {name: [] for name, _, _ in plan}
    for _ in range(args.rounds):
        for name, root, variant in plan:
            got = child(root, variant, args.steps)
            runs[name].append(got)
            print(name, json.dumps(got), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "workload": "bench.py config 3 with remove_one_hop=True: S-wn18rr-shaped fine-tuning, B = 16, 128 strict negatives, "
                       "AdamW; eager (engine.train_step) or one hipGraph replay per step (engine.GraphedTrainStep)",
           "timing": "per child process: median of %d device-synchronised steps (host clock) after 5 warm-up steps, ms; "
                     "%d rounds, variants interleaved, one process at a time" % (args.steps, args.rounds),
           "variants": {}}
    for name, got in runs.items():
        medians = sorted(g["median_ms"] for g in got)
        out["variants"][name] = {"median_of_rounds_ms": medians[len(medians) // 2], "min_round_ms": medians[0],
                                 "max_round_ms": medians[-1], "rounds": got}
    ms = {name: v["median_of_rounds_ms"] for name, v in out["variants"].items()}
    out["run_to_run_spread_ms"] = {name: v["max_round_ms"] - v["min_round_ms"] for name, v in out["variants"].items()}
    out["captured_minus_captured_triples_ms"] = ms["captured"] - ms["captured_triples"]
    out["eager_over_captured"] = ms["eager"] / ms["captured"]
    if args.parent:
        out["parent_eager_over_captured"] = ms["parent_eager"] / ms["captured"]
        out["parent_eager_minus_eager_ms"] = ms["parent_eager"] - ms["eager"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
