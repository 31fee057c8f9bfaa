"""Rotate messages per layer on an MI355X -> profiles/rotate_bench.json.

For S-codexs and S-fb15k237 at B = 16 and S-stress at B = 1 (D = 64, F = B * 64): forward and backward ms of one layer's operator
(median of 20 after 5 warm-ups, HIP events) for
  * rotate_native        -- functional.rotate_rspmm_forward / rotate_rspmm_backward (csrc/rotate.inc: rotate_segment_kernel)
  * distmult_general     -- the DistMult general kernel on the same plan (ultra_rspmm_force_general_path bits 0 and 3)
  * distmult_default     -- the DistMult path the library picks
  * rotate_materialised  -- layer.message + layer.aggregate's arithmetic (gather, complex product, * w, scatter_add) with its
                            torch.cuda.max_memory_allocated; on S-stress only its estimated bytes ("not attempted")
plus algorithmic bytes (forward = E * 8 index / weight + E * F * 4 gathered + N * F * 4 written + R * F * 4;
backward = both plans' walks: 2 E * 12 index bytes, 2 E * F * 4 gathered + (N + R) * F * 4 written) and the fraction of
8 TB/s.  Kernel names for a rocprofv3 --kernel-trace --stats run of their own: rotate_segment_kernel, segment_kernel,
quad_kernel / rowgroup_kernel, fixup_kernel.

    python tools/rotate_bench.py [--out profiles/rotate_bench.json] [--shapes S-codexs,S-fb15k237,S-stress]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12


def timed(fn, warmup=5, reps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def materialised(dst, src, rel, w, relation, x, n, B, D):
    """layer.message (rotate) + aggregate (sum) without the boundary rows: the (E, B, D) route of the parent commit."""
    node_re, node_im = x.view(n, B, D)[src].chunk(2, dim=-1)
    edge_re, edge_im = relation.view(-1, B, D)[rel].chunk(2, dim=-1)
    message = torch.cat([node_re * edge_re - node_im * edge_im, node_re * edge_im + node_im * edge_re], dim=-1)
    weighted = message * w.view(-1, 1, 1)
    out = torch.zeros(n, B, D, device=x.device)
    return out.scatter_add(0, dst.view(-1, 1, 1).expand_as(weighted), weighted)


def bench_shape(name, B, D=64):
    from ultra_torchdrug_amd import RelCSR, _lib, functional as UF
    from ultra_torchdrug_amd.data import SHAPES, synthetic_triples
    dev = torch.device("cuda:0")
    n, _, r = SHAPES[name]
    triples, _, _ = synthetic_triples(name, 1024)
    t = torch.from_numpy(triples).to(dev)
    dst, src, rel = torch.cat([t[:, 1], t[:, 0]]), torch.cat([t[:, 0], t[:, 1]]), torch.cat([t[:, 2], t[:, 2] + r])
    R, F = 2 * r, B * D
    csr = RelCSR(dst, src, rel, None, n, n, R)
    E = csr.n_edges
    gen = torch.Generator(device=dev).manual_seed(1)
    relation = torch.randn(R, F, device=dev, generator=gen)
    x = torch.randn(n, F, device=dev, generator=gen)
    grad = torch.randn(n, F, device=dev, generator=gen)
    lib = _lib.load()
    fwd_bytes = E * 8 + E * F * 4 + n * F * 4 + R * F * 4
    bwd_bytes = 2 * E * 12 + 2 * E * F * 4 + (n + R) * F * 4
    res = {"nodes": n, "edges": E, "relations": R, "B": B, "F": F,
           "algorithmic_bytes": {"forward": fwd_bytes, "backward": bwd_bytes}}
    _ = csr.fwd, csr.by_src, csr.by_rel

    def leg(fwd, bwd):
        f, b = timed(fwd), timed(bwd)
        return {"forward_ms": f, "backward_ms": b,
                "forward_frac_8tbs": fwd_bytes / (f * 1e-3) / PEAK, "backward_frac_8tbs": bwd_bytes / (b * 1e-3) / PEAK}

    with torch.no_grad():
        res["rotate_native"] = leg(lambda: UF.rotate_rspmm_forward(csr, relation, x, "add", D),
                                   lambda: UF.rotate_rspmm_backward(csr, relation, x, None, grad, "add", D))
        res["distmult_default"] = leg(lambda: UF.rspmm_forward(csr, relation, x, "add", "mul"),
                                      lambda: UF.rspmm_backward(csr, relation, x, None, grad, "add", "mul"))
        _lib.check(lib.ultra_rspmm_force_general_path(1 | 8))
        try:
            res["distmult_general"] = leg(lambda: UF.rspmm_forward(csr, relation, x, "add", "mul"),
                                          lambda: UF.rspmm_backward(csr, relation, x, None, grad, "add", "mul"))
        finally:
            _lib.check(lib.ultra_rspmm_force_general_path(0))
    res["rotate_native"]["vs_distmult_general"] = {
        k: res["rotate_native"][k] / res["distmult_general"][k] for k in ("forward_ms", "backward_ms")}
    mat_bytes = E * F * 4
    if name == "S-stress":
        res["rotate_materialised"] = {"status": "not attempted", "one_E_B_D_tensor_bytes": mat_bytes,
                                      "estimated_live_bytes_forward": 4 * mat_bytes}
        return res
    w = torch.ones(E, device=dev)
    ed, es, er = csr.dst, csr.src, csr.rel_id
    rel_g, x_g = relation.clone().requires_grad_(), x.clone().requires_grad_()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        f = timed(lambda: materialised(ed, es, er, w, relation, x, n, B, D))

    def fwd_bwd():
        out = materialised(ed, es, er, w, rel_g, x_g, n, B, D)
        torch.autograd.grad(out, (rel_g, x_g), grad.view(n, B, D))
    fb = timed(fwd_bwd)
    res["rotate_materialised"] = {"forward_ms": f, "backward_ms": fb - f, "forward_plus_backward_ms": fb,
                                  "peak_bytes_above_inputs": torch.cuda.max_memory_allocated() - base,
                                  "one_E_B_D_tensor_bytes": mat_bytes}
    native = res["rotate_native"]["forward_ms"] + res["rotate_native"]["backward_ms"]
    res["rotate_native"]["speedup_fwd_bwd_vs_materialised"] = fb / native
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rotate_bench.json"))
    ap.add_argument("--shapes", default="S-codexs,S-fb15k237,S-stress")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "D": 64, "timing": "median of 20 after 5 warm-ups, HIP events",
           "shapes": {}}
    for name in args.shapes.split(","):
        out["shapes"][name] = bench_shape(name, 1 if name == "S-stress" else 16)
        print(name, json.dumps(out["shapes"][name]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
