"""Child process of tests/test_finite_guard_cpu.py::test_two_gloo_ranks_raise_at_the_same_call_when_one_of_them_is_poisoned (not
a test module itself): ONE rank of a two-rank gloo job on CPU tensors that takes guarded ``engine.train_step`` calls; before the
third call rank 1 alone sets a weight to ``inf``.

    python finite_guard_ranks_child.py RANK WORLD PORT

Prints one JSON line: the call at which this rank raised, what the error named, whether the next call raised again, whether a
``communicate=False`` step after ``reset()`` passed (it decides locally), and whether a barrier behind all of it went through."""
import json
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (os.path.dirname(HERE), HERE):
    if path not in sys.path:
        sys.path.insert(0, path)

WEIGHT = "model.layers.0.linear.weight"


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      OMP_NUM_THREADS="2")
    torch.set_num_threads(2)
    from oracle_ops import oracle_rspmm
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    engine.init_distributed("gloo")
    triples, n, r = synthetic_triples("S-tiny", 1024)
    torch.manual_seed(1024)
    task = build_ultra(r)
    task.preprocess(Graph(torch.from_numpy(triples), num_node=n, num_relation=r))
    task.num_negative = 16
    task.train()
    triples = torch.from_numpy(triples)
    optimizer = torch.optim.AdamW(task.parameters(), lr=1e-3)
    guard = engine.FiniteGuard(task)
    report = {"rank": rank, "raised_at": None, "steps_done": 0}
    torch.manual_seed(100 + rank)

    def step(call, **kwargs):
        at = 16 * call + 8 * rank
        return engine.train_step(task, optimizer, triples[at:at + 8], guard=guard, **kwargs)

    with oracle_rspmm(0):
        for call in (1, 2, 3):
            if call == 3 and rank == 1:
                with torch.no_grad():
                    dict(task.named_parameters())[WEIGHT][1, 5] = float("inf")
            try:
                step(call)
                report["steps_done"] = call
            except engine.NonFiniteError as err:
                report.update(raised_at=call, kind=err.kind, name=err.name, step=err.step)
                break
        try:
            step(4)
            report["raises_again"] = False
        except engine.NonFiniteError:
            report["raises_again"] = True
        guard.reset()
        try:
            step(5, communicate=False)
            report["local_only_passes"] = True
        except engine.NonFiniteError:
            report["local_only_passes"] = False
    dist.barrier()
    report["barrier"] = True
    print(json.dumps(report), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
