"""Pure-torch restatement of one beam-search step of ``TransferNBFNet.visualize`` ("Explaining a prediction"),
written from the documented semantics alone; the CPU operator and the HIP kernel must equal it bit for bit.

Vectorised over edges (chunked, so that the (E, K, K) near-equality table stays small) and over rows (two stable sorts);
runs on whatever device its inputs live on."""
import torch

ATOL = 1e-8
RTOL = 1e-5


def beam_step(row_ptr, src, grad, input, tail, chunk=1 << 18):
    """``(distance, back_edge, back_rank)`` of one layer; same argument conventions as ``functional.beam_search_step``."""
    dev = input.device
    n, K = input.shape
    E = src.numel()
    row_ptr, src = row_ptr.long(), src.long()
    dst = torch.repeat_interleave(torch.arange(n, device=dev), row_ptr[1:] - row_ptr[:-1])
    atol = torch.tensor(ATOL, dtype=torch.float32, device=dev)
    rtol = torch.tensor(RTOL, dtype=torch.float32, device=dev)
    ks = torch.arange(K, device=dev)
    kept_parts, value_parts, prev_parts = [], [], []
    for e0 in range(0, E, chunk):
        e1 = min(E, e0 + chunk)
        m = input[src[e0:e1]] + grad[e0:e1].unsqueeze(-1)                       # one f32 add per candidate
        cand = torch.isfinite(m) & (src[e0:e1] != tail).unsqueeze(-1)
        a, b = m.unsqueeze(-1), m.unsqueeze(-2)                                 # [e, k, k'] = (m_k, m_k')
        close = (a == b) | ((a - b).abs() <= atol + rtol * b.abs())
        close = close & cand.unsqueeze(-2) & (ks.view(1, 1, K) <= ks.view(1, K, 1))
        # smallest matching k' (k' = k always matches a candidate)
        prev = torch.where(close, ks.view(1, 1, K), torch.full_like(ks, K).view(1, 1, K)).amin(-1)
        dup = torch.zeros_like(cand)
        dup[:, 1:] = cand[:, :-1] & (prev[:, 1:] == prev[:, :-1])
        kept_parts.append(cand & ~dup)
        value_parts.append(m)
        prev_parts.append(prev)
    distance = torch.full((n, K), float("-inf"), dtype=torch.float32, device=dev)
    back_edge = torch.full((n, K), -1, dtype=torch.int32, device=dev)
    back_rank = torch.full((n, K), -1, dtype=torch.int32, device=dev)
    if E == 0:
        return distance, back_edge, back_rank
    kept = torch.cat(kept_parts).flatten()
    flat = kept.nonzero().squeeze(-1)                     # ascending (edge, beam) order
    if flat.numel() == 0:
        return distance, back_edge, back_rank
    value = torch.cat(value_parts).flatten()[flat]
    prev = torch.cat(prev_parts).flatten()[flat]
    edge = flat // K
    row = dst[edge]
    # value descending (ties keep (edge, beam) order; -0.0 sorts with +0.0), then rows ascending
    order = torch.sort(value + 0.0, descending=True, stable=True).indices
    order = order[torch.sort(row[order], stable=True).indices]
    row, value, edge, prev = row[order], value[order], edge[order], prev[order]
    count = torch.bincount(row, minlength=n)
    start = torch.cumsum(count, 0) - count
    rank = torch.arange(row.numel(), device=dev) - start[row]
    sel = rank < K
    row, rank = row[sel], rank[sel]
    distance[row, rank] = value[sel]
    back_edge[row, rank] = edge[sel].to(torch.int32)
    back_rank[row, rank] = prev[sel].to(torch.int32)
    return distance, back_edge, back_rank


def csr_of(dst, src, n):
    """Coalesced-order CSR of an edge list already sorted by destination: ``(row_ptr int32, src int32)``."""
    dst = torch.as_tensor(dst).long()
    row_ptr = torch.zeros(n + 1, dtype=torch.long)
    row_ptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
    return row_ptr.to(torch.int32), torch.as_tensor(src).to(torch.int32)


def coalesced_csr(seed, n_node, n_edge, n_rel, isolated=0, hub_row=None, hub_edges=0, self_loops=0, duplicates=0):
    """A random graph's coalesced dst-CSR as ``RelCSR`` builds it (duplicate triples merged): ``(row_ptr, src)`` int32 CPU.
    ``isolated`` trailing nodes get no edges at all; ``hub_row`` receives ``hub_edges`` extra in-edges."""
    from ultra_torchdrug_amd import RelCSR
    g = torch.Generator().manual_seed(seed)
    live = max(n_node - isolated, 1)
    dst = torch.randint(0, live, (n_edge,), generator=g)
    src = torch.randint(0, live, (n_edge,), generator=g)
    rel = torch.randint(0, n_rel, (n_edge,), generator=g)
    if hub_row is not None and hub_edges:
        dst[:hub_edges] = hub_row
    if self_loops:
        src[-self_loops:] = dst[-self_loops:]
    if duplicates:
        dst, src, rel = (torch.cat([x, x[:duplicates]]) for x in (dst, src, rel))
    csr = RelCSR(dst, src, rel, None, n_node, n_node, n_rel, builder="torch")
    row_ptr, src32, _, _ = csr.csr_arrays
    return row_ptr, src32


def beam_inputs(seed, n_node, K, n_edge, empty=0.3, near=True, ties=True):
    """Previous-layer beams ``(N, K)`` (descending rows, ``-inf`` tails, some empty rows), near-equal and exactly tied beams,
    and edge gradients ``(E,)`` with exact ties and near-equal values; seeded, CPU."""
    g = torch.Generator().manual_seed(seed)
    beams = torch.randn(n_node, K, generator=g).sort(dim=1, descending=True).values
    if near and K > 1:
        # every other beam within the isclose tolerance of its left neighbour (1e-5 relative), some exactly equal
        step = beams[:, :-1].abs() * 4e-6 * torch.rand(n_node, K - 1, generator=g)
        beams[:, 1:] = torch.where(torch.rand(n_node, K - 1, generator=g) < 0.3, beams[:, :-1] - step, beams[:, 1:])
        beams[:, 1:] = torch.where(torch.rand(n_node, K - 1, generator=g) < 0.1, beams[:, :-1], beams[:, 1:])
        beams = beams.sort(dim=1, descending=True).values
    count = torch.randint(0, K + 1, (n_node,), generator=g)
    beams[torch.arange(K).view(1, K) >= count.view(-1, 1)] = float("-inf")
    beams[torch.rand(n_node, generator=g) < empty] = float("-inf")
    grad = torch.randn(n_edge, generator=g)
    if ties:
        grad = torch.where(torch.rand(n_edge, generator=g) < 0.2, grad.round(decimals=1), grad)
    return beams, grad
