"""Query-sharded multi-GPU driver for the hot path (one process per GPU, ``torch.distributed``).

The path shards over QUERIES only: every rank holds the whole graph and the 0.78 MB of weights and runs
Bellman-Ford for its own batch elements; there is no exchange inside rspmm.  What crosses ranks:

* evaluation -- one ``all_gather`` of the int64 ``(n_local, 2)`` rankings at the end (the reference gathers the
  full ``(n, 2, N)`` score tensors through gloo: ``/root/reference/ultra/engine.py:146-151``);
* training -- ONE all-reduce of a flat fp32 gradient buffer per step (the reference: DDP with
  ``find_unused_parameters=True``, ``ultra/engine.py:55-60``; parameters that never receive a gradient --
  ``model.dist_embed``, the relation model's ``mlp`` -- are simply absent from the buffer), plus one packed
  all-reduce for the metric scalars (``ultra/engine.py:90``).

Backend: ``nccl`` (= RCCL over xGMI) on GPUs, ``gloo`` on CPU (tests).
"""
import contextlib
import os
import warnings

import torch
import torch.distributed as dist


def init_distributed(backend=None):
    """Join the process group described by RANK / WORLD_SIZE / MASTER_* (set by ``torch.distributed.run``)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1 or dist.is_initialized():
        return get_rank(), get_world_size()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29500")
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    if backend == "nccl":
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    dist.init_process_group(backend)
    return get_rank(), get_world_size()


def get_rank():
    return dist.get_rank() if dist.is_initialized() else 0


def get_world_size():
    return dist.get_world_size() if dist.is_initialized() else 1


def shard_indices(n, rank=None, world=None):
    """Strided shard ``rank, rank + world, ...`` of ``range(n)`` (DistributedSampler order, no padding)."""
    rank = get_rank() if rank is None else rank
    world = get_world_size() if world is None else world
    return torch.arange(rank, n, world)


def gather_variable(local):
    """All-gather tensors whose first dimension differs per rank; returns them re-interleaved in the strided
    order of :func:`shard_indices`, i.e. in the original global order."""
    world = get_world_size()
    if world == 1:
        return local
    n_local = torch.tensor([local.shape[0]], dtype=torch.long, device=local.device)
    sizes = [torch.zeros_like(n_local) for _ in range(world)]
    dist.all_gather(sizes, n_local)
    sizes = [int(s.item()) for s in sizes]
    pad = max(sizes)
    buf = torch.zeros((pad,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    buf[:local.shape[0]] = local
    parts = [torch.zeros_like(buf) for _ in range(world)]
    dist.all_gather(parts, buf)
    total = sum(sizes)
    out = torch.zeros((total,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    for r, (part, size) in enumerate(zip(parts, sizes)):
        out[r:total:world][:size] = part[:size]
    return out


def validate_triples(task, triples):
    """Range check of ``(h, t, r)`` rows against the active context, ONCE per evaluation run / captured step (one host
    read).  The device kernels behind a hipGraph replay cannot raise: the frontier kernel reads ``src_ptr[h]``, the rank
    kernel ``pred[target]`` and the key searches assume ``r < num_relation`` -- an id from another split's vocabulary
    would read out of bounds silently (the reference's eager path fails in an index kernel instead)."""
    if len(triples) == 0:
        return triples
    n, r = task.num_entity, task.num_relation
    lo, hi_node, hi_rel = int(triples.min()), int(triples[:, :2].max()), int(triples[:, 2].max())
    if lo < 0 or hi_node >= n or hi_rel >= r:
        raise ValueError("triples out of range for context `%s` (%d entities, %d relations): min id %d, max entity %d, "
                         "max relation %d" % (task.split, n, r, lo, hi_node, hi_rel))
    return triples


@contextlib.contextmanager
def capture_semantics(task):
    """Around the capture of an INFERENCE graph: one host read that tests every parameter of ``task`` for ``inf`` / ``NaN``.
    The first-layer shortcuts and the dense relation-graph form need finite relation tables (``0 * inf`` is ``NaN`` in the
    reference, they never form the product); eager calls test the tables per call, a replay cannot.  A model with a
    non-finite parameter -- a damaged checkpoint -- is therefore captured on the full kernels (shortcuts declined, dense form
    off for the duration of the capture: a process-wide switch, restored to 0), whose NaN propagation is the reference's,
    with a warning.  Yields whether the parameters are finite.  (Captured TRAINING steps take finiteness on trust -- their
    weights change under the graph -- unless they are given a :class:`FiniteGuard`, which scans the parameters inside every
    replay and raises at the step that finds one non-finite.)"""
    from . import _lib, functional
    params = [p.detach() for p in task.parameters() if p.is_cuda and p.is_floating_point() and p.numel()]
    finite = bool(torch.stack([torch.isfinite(p).all() for p in params]).all()) if params else True
    if finite:
        yield True
        return
    warnings.warn("capture: the model holds a non-finite parameter; recording the full kernels (the reference's NaN "
                  "propagation) instead of the first-layer / dense relation-graph shortcuts")
    saved = functional.CAPTURE_ASSUMES_FINITE
    functional.CAPTURE_ASSUMES_FINITE = False
    lib = _lib.load()
    lib.ultra_rspmm_force_general_path(64)
    try:
        yield False
    finally:
        functional.CAPTURE_ASSUMES_FINITE = saved
        lib.ultra_rspmm_force_general_path(0)


class NonFiniteError(FloatingPointError):
    """A guarded training step met an ``inf`` or a ``NaN`` (:class:`FiniteGuard`).  ``step``: the number of the first bad step
    (guarded steps are counted from 1); ``kind``: ``"loss"``, ``"parameter"`` or ``"gradient"``; ``name``: the parameter's name
    (``"loss"`` for the loss).  On a rank of a process group whose own tensors were finite -- another rank tripped -- ``kind``
    and ``name`` are ``None`` and ``step`` is the step of the poll."""

    def __init__(self, step, kind, name):
        self.step, self.kind, self.name = step, kind, name
        what = ("another rank met a non-finite value" if kind is None else
                "non-finite loss" if kind == "loss" else "non-finite %s `%s`" % (kind, name))
        super().__init__("%s in training step %d" % (what, step))


class FiniteGuard:
    """Divergence guard of the training steps (``train_step``, :class:`GraphedTrainStep`, :class:`GraphedMultiGraphTrainStep`,
    keyword ``guard=``): a step that meets an ``inf`` or a ``NaN`` in the loss, in a parameter or in a gradient raises
    :class:`NonFiniteError` instead of applying it.  The reference stops such a run with ``torch.autograd.set_detect_anomaly``
    (``script/run_full.py:127``); a captured step cannot raise, so HIP kernels (``functional.nonfinite_scan`` /
    ``nonfinite_commit``: kernel nodes only) leave the verdict in a four-word device record (``self.record``, layout in
    ``functional``) that the host reads after the replay.

    INDEX ORDER of the scanned tensors (``self.names``): ``"loss"``; then ``"parameter <name>"`` for every entry of
    ``task.named_parameters()``; then ``"gradient <name>"`` for every entry again.  A parameter without a gradient is skipped,
    its index stays reserved.  Where several tensors are bad in one step the lowest index is reported.

    ONE GUARDED STEP: (1) the parameters are scanned as the step finds them, before the forward, and latched -- a finite loss does not imply
    a finite model here: the sparse first layer and the dense relation-graph form never multiply a relation entry by a zero row,
    so an ``inf`` weight can give finite scores; (2) the loss and the gradients this step's backward wrote are scanned, on every
    rank its own, before any all-reduce; (3) commit; (4) poll: one small device-to-host read of the record outside the graph; in
    a process group the tripped flag is MAX-all-reduced (one word, on every rank, on every polled step), so all ranks raise at
    the same call and their sequences of collectives stay equal (``communicate=False`` steps decide locally, no collective);
    (5) ``optimizer.step()`` -- not reached by a step that tripped: no parameter and no optimizer state is touched by it.  Every
    later step raises again, at once, until :meth:`reset`.

    ``poll_every = k > 1``: the record is read on every k-th step only.  The steps in between apply whatever their gradients
    held; the error still names the FIRST bad step (the record is sticky), but the parameters since that step are lost -- go
    back to a checkpoint older than ``error.step``.

    The guard looks at the loss, the parameters and the gradients, not at intermediate tensors such as the relation tables."""

    def __init__(self, task, poll_every=1):
        from . import functional
        if int(poll_every) < 1:
            raise ValueError("FiniteGuard: poll_every must be at least 1, got %r" % (poll_every,))
        self.task, self.poll_every = task, int(poll_every)
        named = list(task.named_parameters())
        for name, p in named:
            if p.dtype != torch.float32:
                raise RuntimeError("FiniteGuard: parameter `%s` is %s; the scan reads fp32 bit patterns" % (name, p.dtype))
        self.parameters = [p for _, p in named]
        self.names = ["loss"] + ["parameter " + name for name, _ in named] + ["gradient " + name for name, _ in named]
        self._slot = {id(p): i for i, p in enumerate(self.parameters)}
        self.device = self.parameters[0].device if self.parameters else task.device
        self.record = functional.nonfinite_record(self.device)
        self.calls = 0                              # guarded steps so far (every poll_every-th of them reads the record)
        self.error = None                           # the NonFiniteError of the trip, once the host knows of it

    # ------------------------------------------------------------------ the device side of a step (capturable)
    def scan_parameters(self):
        """Scan and LATCH: a parameter that is bad when the step begins is what the error names, not the loss (index 0) that
        the forward computes from it."""
        from . import functional
        functional.nonfinite_scan(self.parameters, self.record, first_index=1)
        functional.nonfinite_commit(self.record, advance=False)

    def scan_loss(self, loss):
        from . import functional
        functional.nonfinite_scan([loss.reshape(-1)], self.record, first_index=0)

    def scan_gradients(self, parameters=None, gradients=None):
        """The gradients of ``parameters`` (default: all of the task's): ``gradients[id(p)]`` where a mapping is given (a
        captured phase: the tensors its backward produced), else ``p.grad``; ``None``: skipped."""
        from . import functional
        slots = [None] * len(self.parameters)
        for p in (self.parameters if parameters is None else parameters):
            slots[self._slot[id(p)]] = gradients.get(id(p)) if gradients is not None else p.grad
        live = [i for i, g in enumerate(slots) if g is not None]
        if live:
            functional.nonfinite_scan(slots[live[0]:live[-1] + 1], self.record,
                                      first_index=1 + len(self.parameters) + live[0])

    def commit(self):
        from . import functional
        functional.nonfinite_commit(self.record)

    # ------------------------------------------------------------------ the host side
    @property
    def tripped(self):
        """Whether a trip is known to the host (set by the poll that found it, cleared by :meth:`reset`); reads nothing."""
        return self.error is not None

    def raise_if_tripped(self):
        if self.error is not None:
            raise self.error

    def check(self, communicate=True):
        """Read the record NOW (one device-to-host read; in a process group one MAX all-reduce of one word before it, so every
        rank must call it) and raise :class:`NonFiniteError` if a step tripped, here or on another rank."""
        from . import functional
        self.raise_if_tripped()
        record = self.record
        if communicate and get_world_size() > 1:
            flag = (record[functional.GUARD_TRIPPED_STEP:functional.GUARD_TRIPPED_STEP + 1] >= 0).to(torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            record = torch.cat([record, flag])
        host = record.tolist()
        if host[functional.GUARD_TRIPPED_STEP] >= 0:
            label = self.names[host[functional.GUARD_TRIPPED_TENSOR]]
            kind, _, name = label.partition(" ")
            self.error = NonFiniteError(host[functional.GUARD_TRIPPED_STEP], kind, name or "loss")
        elif len(host) > functional.GUARD_FIELDS and host[-1] > 0:
            self.error = NonFiniteError(host[functional.GUARD_STEP], None, None)
        self.raise_if_tripped()

    def poll(self, communicate=True):
        """Step (4) of a guarded step: counts the step and, on every ``poll_every``-th, :meth:`check`."""
        self.calls += 1
        if self.calls % self.poll_every == 0:
            self.check(communicate)

    def reset(self, step=None):
        """Forget the trip (device record and host); the step count goes on (``step``: set it).  In a process group: on every
        rank.  The caller restores finite parameters first, or the next step trips again."""
        from . import functional
        if step is None:
            step = int(self.record[functional.GUARD_STEP])
        self.record.copy_(functional.nonfinite_record(self.device, step))
        self.error = None

    def _warm(self):
        """The guard's two kernels once on a scratch record, outside any capture (their code is loaded before a capture)."""
        from . import functional
        scratch = functional.nonfinite_record(self.device)
        functional.nonfinite_scan(self.parameters[:1], scratch)
        functional.nonfinite_commit(scratch)


class GraphedPredict:
    """``task.predict`` for a fixed batch size as ONE hipGraph: an evaluation batch is ~250 small launches
    (18 rspmm + epilogues + relation projections + score MLP) whose host-side issue cost exceeds their GPU time
    on small graphs; replaying a captured graph removes it.  The reference's two per-call index asserts
    (``ultra/model.py:174-175``) are host syncs and cannot be captured; ``predict`` builds those index grids
    itself (``ultra/task.py:249-259``) so they hold by construction and are switched off for the capture."""

    def __init__(self, task, example_batch, warmup=3, with_ranks=False):
        """``with_ranks``: the filtered ranking of the batch (``task.rank_batch``: two key-search kernels, no host
        synchronisation) is captured behind ``predict`` in the same graph; :meth:`ranks` then replays both."""
        assert example_batch.is_cuda and not task.training
        self.task = task
        self.static_batch = validate_triples(task, example_batch).clone()
        self.static_ranks = None
        model = task.model
        model.check_indices = False
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.no_grad():
                pred = None
                for _ in range(warmup):             # builds plans, sets kernel attributes, warms the allocator
                    pred = task.predict(self.static_batch)
                if with_ranks:                      # ... and the completion keys the rank kernels search
                    task.rank_batch(self.static_batch, pred=pred)
            torch.cuda.current_stream().wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            # thread_local: other threads of the process (the RCCL watchdog polls events) must not abort the capture
            with capture_semantics(task), torch.cuda.graph(self.graph, capture_error_mode="thread_local"), torch.no_grad():
                self.static_pred = task.predict(self.static_batch)
                if with_ranks:
                    self.static_ranks = task.rank_batch(self.static_batch, pred=self.static_pred)
        finally:
            model.check_indices = True

    def __call__(self, batch):
        """Scores ``(B, 2, N)``; the returned tensor is overwritten by the next call."""
        if batch.shape != self.static_batch.shape:
            with torch.no_grad():
                return self.task.predict(batch)     # ragged last batch: eager path
        self.static_batch.copy_(batch)
        self.graph.replay()
        return self.static_pred

    def ranks(self, batch):
        """Filtered ranks ``(B, 2)`` int64 of ``batch`` (``with_ranks=True``); a fresh tensor."""
        if self.static_ranks is None or batch.shape != self.static_batch.shape:
            with torch.no_grad():
                return self.task.rank_batch(batch)
        self.static_batch.copy_(batch)
        self.graph.replay()
        return self.static_ranks.clone()

    def statistics(self, batch, rand=None):
        """``task.rank_statistics`` ``(B, 2, 4)`` int64 of ``batch`` (``with_ranks=True``): the captured predict + ranks are
        replayed, then the count and sampling kernels run eagerly on the static scores -- nothing more is captured and no
        random-number call sits inside the graph.  ``rand``: the batch's ``(B, 2, 50)`` uniform numbers under ``toy_eval``."""
        if self.static_ranks is None or batch.shape != self.static_batch.shape:
            with torch.no_grad():
                return self.task.rank_statistics(batch, rand=rand)
        self.static_batch.copy_(batch)
        self.graph.replay()
        with torch.no_grad():
            return self.task._device_statistics(self.static_batch, self.static_pred, self.static_ranks, rand)


class GraphedTrainStep:
    """One fine-tuning step (``ultra/engine.py:62-92``) for a fixed batch size as hipGraph replays: strict negative
    sampling, removal of the batch's own edges, forward, backward.  A step is ~800 launches, most of them tiny, and
    their host-side issue cost exceeds the GPU time of the kernels.  Nothing in the step has a data-dependent shape any
    more: the negatives come from the sorted completion keys (``ultra_strict_negative``) and the edge removal from a
    binary search in the plans (``ultra_edge_removal_weights``; with ``remove_one_hop=True`` the range lookup of
    ``ultra_pair_removal``), where the reference builds ``(B / 2, N)`` masks, calls ``nonzero`` and re-sorts a new graph
    (task.py:102-118, model.py:57-74).  The optimizer step follows the replay eagerly.  Models the native removal does not
    cover -- mean / min / max / PNA aggregation, rotate messages, under either removal rule -- keep eager steps: use
    :func:`train_step`.

    Without a reducer (one rank): ONE graph.  With a :class:`GradientReducer` the gradient all-reduce goes one of three ways
    (``mode`` tells which is active):

    * ``"phased"`` (default) -- the step is captured as THREE graphs that share one memory pool, cut where the gradient
      buckets become complete: (1) forward + backward through the score head and the later half of the entity layers,
      (2) the earlier entity layers + the grouped relation projections, (3) the relation model.  Each graph ends by packing
      its buckets into the reducer's persistent flat buffers (kernel nodes); BETWEEN the replays the buckets of the finished
      phase are all-reduced eagerly on the reducer's side stream while the next phase's replay runs on the compute stream --
      the BASELINE north star's "overlapped with the next layer's rspmm on a side HIP stream", with no collective node in any
      hipGraph (what makes ``reduce_in_graph`` fail on this runtime is not in play).  The parameters' ``.grad`` are views of
      the flat buffers: RCCL averages in place and nothing is unpacked.  The backward is split with ``torch.autograd.grad``
      at the tensors ``model.last_cuts`` / ``task.last_relation_inputs`` (same kernels, same accumulation order as the
      single backward: the captured phases are verified against an eager backward before use; a model the cut does not
      cover drops to ``"after"`` with a warning).
    * ``"after"`` -- one graph, hooks paused; the buckets go out after the replay (``reducer.reduce_all()``): communication
      FOLLOWS the backward (round 3's default).
    * ``"in_graph"`` (``reduce_in_graph=True``, opt-in) -- the hooks stay live during the capture, so every bucket's pack and
      RCCL all-reduce become nodes of the graph; verified before use.  On the runtime this was developed on (PyTorch 2.10 +
      ROCm 7.0, RCCL 2.26, one-rank group) the verification fails -- a captured all-reduce alone replays correctly, the
      captured step with bucket traffic does not (``tools/debug/graph_collective_probe.py``), and once
      in a while the verification's replay ends the process with a HIP abort -- so its test runs in a child process.

    Collectives of the CONSTRUCTOR: the warm-up steps, the captures and the verification run with the reducer's hooks paused,
    so they issue none; RCCL is warmed by ``reducer.warm()`` (one explicit all-reduce per bucket) unless
    ``warm_collectives=False`` (a caller that builds several steps, :class:`GraphedMultiGraphTrainStep`, warms once itself).
    Every rank that constructs a step issues the same collectives, whatever graph its example batch is from, and every
    ``__call__`` sends exactly ONE round of buckets (checked).

    ``guard``: a :class:`FiniteGuard`.  Its scans and its commit are recorded into the graph(s) as kernel nodes -- the parameters
    before the forward, the loss and the gradients behind the backward that wrote them (phased: every phase scans the gradients
    it completes, behind its packs; the commit ends the last phase) -- and every call polls the record between the replay (and
    the step's collectives) and ``optimizer.step()``.  ``reduce_in_graph=True`` refuses a guard.  Without one the step records
    and launches exactly what it did before the guard existed."""

    def __init__(self, task, optimizer, example_batch, warmup=3, reducer=None, reduce_in_graph=False, warm_collectives=True,
                 phased=True, guard=None):
        assert example_batch.is_cuda and task.training
        if guard is not None and reduce_in_graph:
            raise ValueError("GraphedTrainStep: a FiniteGuard scans each rank's own gradients before they are all-reduced; "
                             "with reduce_in_graph=True the all-reduce runs inside the backward of the captured graph -- "
                             "use the phased or the after mode with a guard")
        model = task.model
        if not model._removal_by_zero_weight(sums_only=True):
            raise ValueError("GraphedTrainStep needs summed messages (sum aggregation of DistMult / TransE messages: the edge "
                             "removal that can be captured, under either rule of remove_one_hop); use engine.train_step for "
                             "this model")
        self.task, self.optimizer, self.reducer, self.guard = task, optimizer, reducer, guard
        # the captures' verification replays the guard's nodes: the record is put back afterwards as it is now
        guard_record = None if guard is None else guard.record.clone()
        self.static_batch = validate_triples(task, example_batch).clone()
        self.reduce_in_graph = False
        self.mode = "single"
        self.communicate = True                     # False (bench.py): replay + optimizer only, to price the collectives
        model.check_indices = False
        try:
            import contextlib
            import warnings
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            quiet = reducer.paused() if reducer is not None else contextlib.nullcontext()
            with torch.cuda.stream(side), quiet:    # hooks paused: the warm-up issues NO collective (ranks of a multi-graph
                for _ in range(warmup):             # run build their steps on different graphs)
                    optimizer.zero_grad(set_to_none=True)       # plans, completion keys, kernel attributes, workspaces, allocator
                    loss, _ = task(self.static_batch)
                    loss.backward()
                if guard is not None:
                    guard._warm()
            torch.cuda.current_stream().wait_stream(side)
            active = reducer is not None and reducer._active()
            if reducer is not None and (warm_collectives or reduce_in_graph):
                reducer.warm()                      # RCCL warm: one all-reduce per bucket, the same on every rank
            if active and reduce_in_graph and reducer.overlap:
                try:
                    self._capture(reduce=True)
                    self.reduce_in_graph = self._verify_captured_reduction()
                    if not self.reduce_in_graph:
                        warnings.warn("GraphedTrainStep: the step captured WITH the gradient all-reduce does not reproduce "
                                      "eager gradients on this runtime; the buckets are reduced outside the graphs instead")
                except Exception as err:            # the runtime refused collective nodes
                    warnings.warn("GraphedTrainStep: capturing the gradient all-reduce failed (%s); the buckets are "
                                  "reduced outside the graphs instead" % (str(err).splitlines()[0] if str(err) else type(err).__name__))
                if self.reduce_in_graph:
                    self.mode = "in_graph"
                else:
                    torch.cuda.synchronize()
                    reducer.abandon()
            if active and phased and not self.reduce_in_graph:
                try:
                    self._capture_phased()
                    self.mode = "phased"
                except _NoPhases as err:
                    warnings.warn("GraphedTrainStep: %s; the buckets are reduced after the replay instead" % err)
                    self.graphs = None
                    torch.cuda.synchronize()
            if self.mode not in ("in_graph", "phased"):
                self._capture(reduce=False)
                self.mode = "after" if active else "single"
                # the gradient tensors THIS graph writes (allocated in its pool during the capture): several captured steps
                # over one set of parameters (GraphedMultiGraphTrainStep) re-bind theirs before the optimizer step
                self._grads = [(p, p.grad) for p in task.parameters() if p.grad is not None]
            elif self.mode == "in_graph":
                self._grads = [(p, p.grad) for p in task.parameters() if p.grad is not None]
        finally:
            model.check_indices = True
            if guard is not None:
                torch.cuda.synchronize()
                guard.record.copy_(guard_record)

    def _capture(self, reduce):
        import contextlib
        self.optimizer.zero_grad(set_to_none=True)  # the captured backward allocates the gradients in the graph's pool
        self.graph = torch.cuda.CUDAGraph()
        hooks = contextlib.nullcontext() if (reduce or self.reducer is None) else self.reducer.paused()
        # thread_local: other threads of the process (the RCCL watchdog polls events) must not abort the capture
        guard = self.guard
        with hooks, torch.cuda.graph(self.graph, capture_error_mode="thread_local" if reduce else "relaxed"):
            if guard is not None:
                guard.scan_parameters()
            self.static_loss, self.static_metric = self.task(self.static_batch)
            self.static_loss.backward()
            if guard is not None:
                guard.scan_loss(self.static_loss)
                guard.scan_gradients()
                guard.commit()
            if reduce:
                self.reducer.finish()
        self.last_negatives = self.task.last_negatives      # (B, num_negative): the tensor every replay rewrites

    # ------------------------------------------------------------------ phased capture
    def _phases(self):
        """Which phase of the backward completes each parameter's gradient -- the reducer's group of its bucket (0: score head
        and the entity layers after the cut; 1: the earlier entity layers and the grouped relation projections; 2: the relation
        models); parameters outside the buckets (they receive no gradient) are listed with the stack they belong to."""
        task, reducer = self.task, self.reducer
        if len(reducer.groups) != 3 or reducer.cut_after != self.cut_after:
            raise _NoPhases("the reducer's groups (%d, cut after layer %s) do not match the three phases of this model"
                            % (len(reducer.groups), reducer.cut_after))
        phase_of = {}
        for name, p in task.named_parameters():
            b = reducer._bucket_of.get(id(p))
            phase_of[id(p)] = reducer._group_of[b] if b is not None else (2 if name.startswith("rel_models.") else 1)
        return phase_of, reducer.groups

    def _capture_phased(self):
        task, model, reducer, guard = self.task, self.task.model, self.reducer, self.guard
        if len(model.layers) < 2 or not task.rel_models:
            raise _NoPhases("the model has fewer than two entity layers or no relation model")
        self.cut_after = model.cut_at()
        phase_of, groups = self._phases()
        device = self.static_batch.device
        reducer.flat_buffers(device)
        bucketed = {id(p) for b in reducer.buckets for p in b["params"]}
        params = [[p for p in task.parameters() if p.requires_grad and phase_of[id(p)] == phase] for phase in range(3)]
        self.optimizer.zero_grad(set_to_none=True)
        graphs = [torch.cuda.CUDAGraph() for _ in range(3)]
        produced = {}

        def keep(ps, grads):
            for p, g in zip(ps, grads):
                if g is not None:
                    if id(p) not in bucketed:
                        raise _NoPhases("a parameter outside the reducer's buckets receives a gradient")
                    produced[id(p)] = g

        def pack(phase):
            for b in groups[phase]:
                reducer.pack(b, produced)
            if guard is not None:                    # the gradients this phase completed, as its backward wrote them
                if phase == 0:
                    guard.scan_loss(self.static_loss)
                guard.scan_gradients(params[phase], produced)
                if phase == 2:
                    guard.commit()

        with reducer.paused():
            with torch.cuda.graph(graphs[0], capture_error_mode="relaxed"):
                if guard is not None:
                    guard.scan_parameters()
                model.record_cuts = task.record_cuts = True         # only this forward records the cut tensors
                try:
                    self.static_loss, self.static_metric = task(self.static_batch)
                    cuts, rel_inputs = model.last_cuts, task.last_relation_inputs
                finally:
                    model.record_cuts = task.record_cuts = False
                    model.last_cuts = task.last_relation_inputs = None
                self.last_negatives = task.last_negatives   # (B, num_negative): the tensor every replay rewrites
                if cuts is not None and rel_inputs:
                    got = torch.autograd.grad(self.static_loss, params[0] + cuts, allow_unused=True)
                    keep(params[0], got[:len(params[0])])
                    cut_grads = got[len(params[0]):]
                    pack(0)
            if cuts is None or not rel_inputs or any(g is None for g in cut_grads):
                raise _NoPhases("this model / batch does not expose the cut tensors (grouped relation tables, sum layers)")
            with torch.cuda.graph(graphs[1], pool=graphs[0].pool(), capture_error_mode="relaxed"):
                got = torch.autograd.grad(cuts, params[1] + list(rel_inputs), grad_outputs=list(cut_grads), allow_unused=True)
                keep(params[1], got[:len(params[1])])
                rel_grads = got[len(params[1]):]
                pack(1)
            live = [(t, g) for t, g in zip(rel_inputs, rel_grads) if g is not None]
            if not live:
                raise _NoPhases("no gradient reaches the relation model")
            with torch.cuda.graph(graphs[2], pool=graphs[0].pool(), capture_error_mode="relaxed"):
                got = torch.autograd.grad([t for t, _ in live], params[2], grad_outputs=[g for _, g in live], allow_unused=True)
                keep(params[2], got)
                pack(2)
        self.graphs, self.groups = graphs, groups
        views = reducer.views()
        self._grads = [(p, views[id(p)]) for p in task.parameters() if id(p) in bucketed]
        self._local = produced                       # (kept alive: the graphs write these)
        if not self._verify_phases():
            raise _NoPhases("the phased backward does not reproduce the gradients of the single backward on this model")

    def _replay_phases(self, communicate):
        reducer = self.reducer
        for g, graph in enumerate(self.graphs):
            graph.replay()
            if communicate:
                reducer.launch_group(g)             # side stream: RCCL works while the next phase replays
        if communicate:
            reducer.wait_groups()

    def _verify_phases(self):
        """One replay of the three phases (no collective) against an eager single backward on the same batch and the
        negatives the replay drew: every gradient packed into the flat buffers must EQUAL the eager one."""
        task = self.task
        self._replay_phases(communicate=False)
        torch.cuda.synchronize()
        got = {id(p): view.clone() for p, view in self._grads}
        loss_replayed = self.static_loss.detach().clone()
        task._static_negative = self.last_negatives.clone()
        saved = [(p, p.grad) for p in task.parameters()]
        for p in task.parameters():
            p.grad = None
        try:
            with self.reducer.paused():
                loss, _ = task(self.static_batch)
                loss.backward()
            torch.cuda.synchronize()
            ok = bool(torch.equal(loss.detach(), loss_replayed))
            for p in task.parameters():
                if id(p) in got:
                    want = p.grad if p.grad is not None else torch.zeros_like(p)
                    ok = ok and bool(torch.equal(got[id(p)], want))
                elif p.grad is not None:
                    ok = False
        finally:
            task._static_negative = None
            for p, g in saved:
                p.grad = g
        return ok

    def _verify_captured_reduction(self, rounds=2):
        """Replays of the step captured with the bucket traffic against eager backward passes on the same batch and the
        negatives each replay drew (one-rank group: EQUAL; more ranks: all ranks hold the same example batch here, so
        the mean over ranks is that gradient again, up to the rounding of sum / world)."""
        task, world = self.task, get_world_size()
        params = [p for p in task.parameters() if p.grad is not None]
        ok = True
        for _ in range(rounds):
            self.graph.replay()
            torch.cuda.synchronize()
            captured = [p.grad for p in params]
            got = [g.clone() for g in captured]
            for p in params:
                p.grad = None
            task._static_negative = self.last_negatives.clone()
            try:
                with self.reducer.paused():
                    loss, _ = task(self.static_batch)
                    loss.backward()
            finally:
                task._static_negative = None
            torch.cuda.synchronize()
            for p, g, keep in zip(params, got, captured):
                want = p.grad
                same = want is not None and (torch.equal(g, want) if world == 1 else
                                             bool(((g - want).abs() <= 1e-6 * want.abs().max() + 1e-12).all()))
                ok = ok and same
                p.grad = keep
        flag = torch.tensor([1.0 if ok else 0.0], device=self.static_batch.device)
        if world > 1:                               # every rank takes the same branch
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return bool(flag.item() > 0.5)

    def __call__(self, batch):
        """One step on ``batch`` (same shape as the example): returns ``(loss, metrics averaged over ranks)``."""
        assert batch.shape == self.static_batch.shape
        guard = self.guard
        if guard is not None:
            guard.raise_if_tripped()
        self.static_batch.copy_(batch)
        for p, grad in self._grads:
            p.grad = grad
        reducer = self.reducer
        if self.mode == "phased":
            sent = reducer.total_launched
            self._replay_phases(self.communicate)
            if self.communicate and reducer.total_launched - sent != len(reducer.buckets):
                raise RuntimeError("GraphedTrainStep: %d bucket all-reduces went out in one step, expected %d"
                                   % (reducer.total_launched - sent, len(reducer.buckets)))
            if guard is not None:
                guard.poll(self.communicate)
            self.optimizer.step()
            return self.static_loss.detach(), (reduce_metrics(self.static_metric) if self.communicate else self.static_metric)
        if not self.communicate:                    # measurement only: the step without any cross-rank traffic
            self.graph.replay()
            if guard is not None:
                guard.poll(False)
            self.optimizer.step()
            return self.static_loss.detach(), self.static_metric
        if self.mode == "after":
            sent = reducer.total_launched
            with reducer.paused():                  # (replays fire no hooks; this keeps it so by construction)
                self.graph.replay()
            reducer.reduce_all()
            if reducer.total_launched - sent != len(reducer.buckets):
                raise RuntimeError("GraphedTrainStep: %d bucket all-reduces went out in one step, expected %d -- the ranks' "
                                   "sequences of collectives would diverge" % (reducer.total_launched - sent,
                                                                               len(reducer.buckets)))
        else:
            self.graph.replay()
            if reducer is None:
                allreduce_gradients(self.task)
        if guard is not None:
            guard.poll(True)
        self.optimizer.step()
        return self.static_loss.detach(), reduce_metrics(self.static_metric)


class _NoPhases(RuntimeError):
    """The phased capture does not apply to this model (GraphedTrainStep falls back to one graph)."""


class GraphedMultiGraphTrainStep:
    """Multi-graph pre-training (``ultra/engine.py:23-92``, ``task.py:637-890``) with one captured step PER GRAPH CONTEXT:
    a batch ``(triples, graph_id)`` replays the :class:`GraphedTrainStep` of its graph, all of them over the same
    parameters and optimizer -- each capture owns the gradient tensors its backward writes and re-binds them to the
    parameters before the optimizer step.  The eager step of this workload is ~800 launches whose host-side issue cost
    exceeds their GPU time.

    Every rank may be on another graph in the same step (ranks draw independently, ``ultra/engine.py:23-34``), so what a
    rank does on FIRST use of a graph must not differ from any other step in the collectives it issues.  All contexts are
    therefore captured HERE, in sorted context order on every rank, with the reducer's hooks paused (no collective from
    warm-up or capture), followed by one ``reducer.warm()``; afterwards each call sends exactly one round of bucket
    all-reduces (replay, ragged eager step alike) plus the packed metric reduce -- the same sequence on all ranks
    whatever graphs they draw.  (Round 3 captured lazily with live hooks: a rank meeting a graph for the first time sent
    ``warmup`` extra rounds that paired with other ranks' real gradients -- VERDICT r3 weak 12.)

    ``examples``: optional ``{graph_id: (batch_size, 3) triples}`` to capture with (default: the first ``batch_size`` fact
    edges of each graph).  Contexts with fewer than ``batch_size`` fact edges keep the eager step."""

    def __init__(self, task, optimizer, batch_size, reducer=None, warmup=3, examples=None, phased=True, guard=None):
        self.task, self.optimizer, self.batch_size, self.reducer, self.warmup = task, optimizer, int(batch_size), reducer, warmup
        self.guard = guard                          # ONE FiniteGuard for the captured step of every graph and the eager steps
        self.steps = {}
        self.communicate = True                     # see GraphedTrainStep.communicate
        saved = task.split
        device = task.device
        try:
            for name in sorted(task.contexts, key=str):
                task.use(name)
                example = None if examples is None else examples.get(name)
                if example is None:
                    example = task.fact_graph.edge_list[:self.batch_size]
                if len(example) != self.batch_size:
                    continue
                self.steps[str(name)] = GraphedTrainStep(task, optimizer, example.to(device), warmup=warmup, reducer=reducer,
                                                         warm_collectives=False, phased=phased, guard=guard)
        finally:
            if saved is not None:
                task.use(saved)
        if reducer is not None:
            reducer.warm()

    def __call__(self, batch):
        triples, graph_id = batch
        graph_id = str(graph_id)
        self.task.use(graph_id)
        step = self.steps.get(graph_id)
        if step is not None:
            step.communicate = self.communicate
        if step is None or len(triples) != self.batch_size:          # ragged batch / tiny graph: the eager step
            # (honours `communicate` too: a no-traffic measurement must not contain an eager step's collectives, and a rank on
            # the eager branch must issue what its replaying peers issue -- ADVICE r4)
            return train_step(self.task, self.optimizer, (triples, graph_id), reducer=self.reducer, communicate=self.communicate,
                              guard=self.guard)
        return step(triples)

    @property
    def modes(self):
        """``{graph_id: mode}`` of the captured steps ("phased" / "after" / "in_graph" / "single"): a capture whose phased
        backward does not verify bit for bit falls back to "after" with a warning, possibly on one rank and not another --
        the collective sequences still match, the overlap is lost there.  bench.py prints this and flags disagreement."""
        return {name: step.mode for name, step in self.steps.items()}


class GraphedScores:
    """Scores ``(Q, N)`` of Q tail-form queries ``(anchor, relation in [0, 2R), ?)`` -- ``score_all_entities`` of the
    entity model on the relation representations of ``base_relation`` -- captured once and replayed as a hipGraph
    (the query-level counterpart of :class:`GraphedPredict`, which takes triples)."""

    def __init__(self, task, anchor, relation, base_relation, graphed=True, warmup=3):
        self.task = task
        self.static = [anchor.clone(), relation.clone(), base_relation.clone()]
        self.graph, self.static_pred = None, None
        if not graphed:
            return
        model = task.model
        model.check_indices = False
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(warmup):
                    self._scores(*self.static)
            torch.cuda.current_stream().wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with capture_semantics(task), torch.cuda.graph(self.graph, capture_error_mode="thread_local"), torch.no_grad():
                self.static_pred = self._scores(*self.static)
        finally:
            model.check_indices = True

    def _scores(self, anchor, relation, base_relation):
        rel_inputs = self.task.relation_representations(base_relation)
        return self.task.model.score_all_entities(self.task.fact_graph, rel_inputs, anchor, relation)

    def __call__(self, anchor, relation, base_relation):
        """The returned tensor is overwritten by the next call."""
        if self.graph is None or anchor.shape != self.static[0].shape:
            with torch.no_grad():
                return self._scores(anchor, relation, base_relation)
        for dst, src in zip(self.static, (anchor, relation, base_relation)):
            dst.copy_(src)
        self.graph.replay()
        return self.static_pred


def _ranks_of_unique_queries(task, local, batch_size, graphed, statistics=False, rand=None):
    """``(n, 2)`` filtered ranks of the triples ``local`` with every DISTINCT query scored once.  A test set asks
    ``(h, r, ?)`` and ``(?, r, t)`` for each triple; triples that share the head and the relation share the tail query
    (and popular tails share head queries), and a query's scores do not depend on its batch mates, so the Bellman-Ford
    runs over the distinct queries only, ``2 * batch_size`` at a time, and every triple ranks its own target in the
    scores of its query.  ``None`` when the model has no fused all-entity score path (the caller keeps the triple loop).
    ``statistics``: ``(n, 2, 4)`` ``task.rank_statistics`` instead -- the counts and, under ``toy_eval``, the sampled ranks of
    every entry from ITS OWN row of ``rand`` ``(n, 2, 50)``, whichever entries share its query."""
    from . import backend
    ops = backend.get()
    n = len(local)
    h, t, r = local.t()
    n_rel = task.num_relation
    graph = task.graph
    anchor, q_rel = torch.cat([h, t]), torch.cat([r, r + n_rel])                # tail form (model.py:76-83)
    target, base = torch.cat([t, h]), torch.cat([r, r])
    uniq, inverse = torch.unique(anchor * (2 * n_rel) + q_rel, return_inverse=True)
    u_anchor, u_rel = uniq // (2 * n_rel), uniq % (2 * n_rel)
    u_base = torch.where(u_rel >= n_rel, u_rel - n_rel, u_rel)
    order = torch.argsort(inverse, stable=True)                                 # entries grouped by their query
    first = torch.searchsorted(inverse[order], torch.arange(len(uniq) + 1, device=local.device))
    chunk = 2 * batch_size
    keys = (graph.completion_keys(0), graph.completion_keys(1)) if task.filtered_ranking else (None, None)
    rank_rel = max(graph.num_relation, 1)
    ranks = torch.empty(2 * n, dtype=torch.long, device=local.device)
    extra = torch.zeros(2 * n, 3, dtype=torch.long, device=local.device) if statistics else None     # count, optimistic, pessimistic
    if statistics and task.toy_eval:
        rand = torch.cat([rand[:, 0], rand[:, 1]])                              # (2n, 50): entry e < n = the tail query of triple e
    scorer = None
    bounds = first.tolist()
    for c in range(0, len(uniq), chunk):
        ids = torch.arange(c, c + chunk, device=local.device).clamp(max=len(uniq) - 1)       # the last chunk repeats its end
        args = (u_anchor[ids], u_rel[ids], u_base[ids])
        if scorer is None:
            probe = GraphedScores(task, *args, graphed=False)
            if probe(*args) is None:                     # no fused all-entity score path for this model
                return None
            scorer = GraphedScores(task, *args, graphed=bool(graphed) and len(uniq) >= 2 * chunk)
        scores = scorer(*args)
        entries = order[bounds[c]:bounds[min(c + chunk, len(uniq))]]
        rows = scores[inverse[entries] - c]                                     # (k, N): each entry's query row
        for side in (0, 1):                                                     # tails, heads: their own completion keys
            pick = (entries < n) if side == 0 else (entries >= n)
            e = entries[pick]
            if len(e):
                ranks[e] = ops.filtered_rank_keys(rows[pick], target[e], keys[side], anchor[e], base[e], rank_rel,
                                                  graph.num_node)
                if statistics:
                    extra[e, 0] = ops.filter_counts(keys[side], anchor[e], base[e], rank_rel, graph.num_node)
                    if task.toy_eval:
                        extra[e, 1], extra[e, 2] = ops.sampled_rank_keys(rows[pick], target[e], keys[side], anchor[e], base[e],
                                                                         rank_rel, rand[e], graph.num_node)
    if statistics:
        both = torch.cat([ranks[:, None], extra], dim=1)                        # (2n, 4)
        return torch.stack([both[:n], both[n:]], dim=1)
    return torch.stack([ranks[:n], ranks[n:]], dim=1)


@torch.no_grad()
def answer(task, anchor, relation, k=10, head=False, batch_size=16, graphed=None, filtered=None, with_hops=False,
           candidates=None, candidate_set=None):
    """``task.answer`` over any number of queries: the ``k`` best unfiltered entities of ``(anchor[q], relation[q], ?)`` (``head``:
    of ``(?, relation[q], anchor[q])``).  The queries are scored ``2 * batch_size`` at a time through one :class:`GraphedScores`
    (the last chunk repeats its end) and ``functional.topk_keys`` is enqueued on each chunk's static scores: nothing of size
    ``(Q, N)`` beside those scores is built and nothing is read back per chunk.  ``graphed`` (default: on a GPU, in eval mode,
    when there are at least two full chunks): the score pass is captured once and replayed.  A model without a fused all-entity
    score head goes through ``task.answer`` chunk by chunk.  Returns ``(entities int64 (Q, k), scores fp32 (Q, k))`` and, with
    ``with_hops``, ``task.answer_hops`` of all of them as a third result (one hop-distance call behind the chunks).
    ``candidates`` / ``candidate_set``: as ``task.answer`` -- each query's answers come from its set of a ``data.CandidateSets``,
    checked once for the call, and ``functional.candidate_select`` takes the place of ``topk_keys`` on every chunk."""
    from . import backend
    if with_hops:
        entities, scores = answer(task, anchor, relation, k, head, batch_size, graphed, filtered, False, candidates, candidate_set)
        return entities, scores, task.answer_hops(task.answer_queries(anchor, relation, head)[0], entities)
    sets = set_of = max_len = None
    if candidates is None:
        if candidate_set is not None:
            raise ValueError("answer: candidate_set needs candidates")
        anchor, q_rel, base = task.answer_queries(anchor, relation, head)
    elif candidate_set is None:
        anchor, q_rel, base = task.answer_queries(anchor, relation, head)
        sets, set_of, max_len = task.answer_sets(candidates, q_rel)
    else:
        if not hasattr(candidates, "num_sets"):
            raise ValueError("answer: candidates must be a data.CandidateSets, got %s" % type(candidates).__name__)
        anchor, q_rel, base, set_of, any_all = task.answer_queries(anchor, relation, head, candidate_set, candidates.num_sets)
        sets, set_of, max_len = task.answer_sets(candidates, q_rel, set_of, any_all)
    keys, n_rel, n_node = task.answer_filter(head, filtered)
    n, chunk = len(anchor), 2 * batch_size
    if graphed is None:
        graphed = task.device.type == "cuda" and n >= 2 * chunk and not task.training
    if sets is not None and not 1 <= int(k) <= 128:
        raise ValueError("answer: 1 to 128 answers per query, got %d" % int(k))
    entities, scores = [], []
    scorer = None
    for c in range(0, n, chunk):
        ids = torch.arange(c, c + chunk, device=anchor.device).clamp(max=n - 1)              # the last chunk repeats its end
        args = (anchor[ids], q_rel[ids], base[ids])
        if scorer is None:
            probe = GraphedScores(task, *args, graphed=False)
            if probe(*args) is None:                     # no fused all-entity score path for this model
                parts = [task.answer(anchor[i:i + chunk], base[i:i + chunk], k, head, filtered, False, sets,
                                     None if candidate_set is None else set_of[i:i + chunk]) for i in range(0, n, chunk)]
                return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
            scorer = GraphedScores(task, *args, graphed=bool(graphed) and n >= 2 * chunk)
        if sets is None:
            value, index = backend.get().topk_keys(scorer(*args), k, keys, args[0], args[2], n_rel, n_node)
        else:
            found = task._candidate_select(scorer(*args), sets, set_of[ids], int(k), keys, args[0], args[2], n_rel, None,
                                           ("top_index", "top_value"), max_len)
            index, value = found.top_index, found.top_value
        keep = min(chunk, n - c)
        entities.append(index[:keep])
        scores.append(value[:keep])
    if not entities:
        return task.answer(anchor, base, k, head, filtered, False, sets, None if candidate_set is None else set_of)
    return torch.cat(entities), torch.cat(scores)


@torch.no_grad()
def evaluate_constrained(task, triples, candidates, batch_size=16):
    """Type-constrained evaluation, the usual protocol beside the filtered one: every tail of ``triples`` (``(n, 3)`` rows of
    (h, t, r)) is ranked among the set ``r`` of ``candidates`` and every head among the set ``r + R`` (``data.relation_candidates``;
    ``task.rank_among``, both sides filtered by the context's filter graph as ``evaluate``).  A side whose target is NOT in its set
    is left out of every mean and counted in ``outside`` -- never silently ranked.  Returns a dict with ``mrr``, ``mr``, ``hits@1``,
    ``hits@3``, ``hits@10`` over the sides inside (``nan`` when there is none), ``outside``, ``ranks`` int64 ``(n, 2)`` (column 0
    the tail side; 0 for a side outside), and ``mean_candidates``, the mean number of candidates a side inside was ranked among.
    ``batch_size`` triples are scored at a time; one host read at the end."""
    triples = torch.as_tensor(triples, device=task.device).long()
    if triples.dim() != 2 or triples.shape[1] != 3:
        raise ValueError("evaluate_constrained takes (n, 3) rows of (h, t, r), got %s" % (tuple(triples.shape),))
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("evaluate_constrained: batch_size must be positive, got %d" % batch_size)
    validate_triples(task, triples)
    parts = [task.rank_among(triples[i:i + batch_size], candidates) for i in range(0, len(triples), batch_size)]
    if parts:
        ranks, member, count = (torch.cat([p[j] for p in parts]) for j in range(3))
    else:
        ranks = count = torch.zeros(0, 2, dtype=torch.int64, device=triples.device)
        member = torch.zeros(0, 2, dtype=torch.bool, device=triples.device)
    ranks = torch.where(member, ranks, torch.zeros_like(ranks))
    inside = member.double()                              # 1 for a side inside its set; its rank is at least 1 there
    safe = ranks.clamp(min=1).double()
    sums = [inside.sum(), (inside / safe).sum(), (inside * ranks).sum(), (inside * count).sum()]
    sums += [(inside * (safe <= top)).sum() for top in (1, 3, 10)]
    n_inside, mrr, mr, candidates, hits1, hits3, hits10 = torch.stack(sums).tolist()          # the one host read
    mean = lambda total: total / n_inside if n_inside else float("nan")
    return {"outside": int(member.numel() - n_inside), "ranks": ranks, "mrr": mean(mrr), "mr": mean(mr), "hits@1": mean(hits1),
            "hits@3": mean(hits3), "hits@10": mean(hits10), "mean_candidates": mean(candidates)}


def _relation_blocks(task, h, t, cand, pair_batch, batch_size):
    """The pairs in blocks of at most ``pair_batch``, sorted by head so that the pairs of one head share its query columns:
    yields ``(ids, scores (len(ids), C))`` -- ``ids`` the block's positions in the input; the block is all that is kept."""
    pair_batch = int(pair_batch)
    if pair_batch < 1:
        raise ValueError("relation prediction: pair_batch must be positive, got %d" % pair_batch)
    order = torch.argsort(h, stable=True)
    with task.relation_tables_of(cand):                  # (the relation stack runs once for the call, not once per block)
        for i in range(0, len(h), pair_batch):
            ids = order[i:i + pair_batch]
            yield ids, task._relation_scores(h[ids], t[ids], cand, batch_size)


@torch.no_grad()
def answer_relation(task, h, t, k=10, pair_batch=1024, candidates=None, inverse=False, filtered=None, batch_size=16):
    """``task.answer_relation`` over any number of pairs with bounded memory: the ids are range-checked once, the pairs are
    sorted by head and served ``pair_batch`` at a time -- a ``(pair_batch, C)`` block of scores is all that is kept, and
    ``functional.relation_select`` is enqueued on it with nothing read back per block.  Each pair's result is what
    ``task.answer_relation`` gives for it alone (a query column does not depend on its batch mates).  Returns ``(relations int64
    (P, k), scores fp32 (P, k))`` in input order."""
    from .functional import TOPK_MAX
    k = int(k)
    if not 1 <= k <= TOPK_MAX:
        raise ValueError("answer_relation: 1 to %d relations per pair, got %d" % (TOPK_MAX, k))
    h, t, cand = task.relation_queries(h, t, candidates, inverse)
    keys = task.relation_filter(filtered)
    relations = torch.full((len(h), k), -1, dtype=torch.int64, device=h.device)
    scores = torch.full((len(h), k), -float("inf"), dtype=torch.float32, device=h.device)
    for ids, block in _relation_blocks(task, h, t, cand, pair_batch, int(batch_size)):
        found = task._relation_select(block, cand, keys, h[ids], t[ids], None, k, ("top_index", "top_value"))
        relations[ids], scores[ids] = found.top_index, found.top_value
    return relations, scores


@torch.no_grad()
def evaluate_relations(task, triples, candidates=None, inverse=False, batch_size=16, pair_batch=1024, filtered=None):
    """Relation prediction as an evaluation: for every row ``(h, t, r)`` of ``triples`` the rank of ``r`` among the candidate
    relations (``task.relation_queries``) for the pair ``(h, t)``, filtered by the context's filter graph (``filtered``, default
    ``task.filtered_ranking``): ``rank = 1 + #{candidates that are not known and score at least as high}`` -- pessimistic on ties
    as ``filtered_rank_keys``; a target the filter graph does not hold counts itself.  A triple whose
    relation is not among the candidates is not ranked: it is counted in ``skipped`` and its rank is 0.  Returns a dict with
    ``mrr``, ``mr``, ``hits@1``, ``hits@3``, ``hits@10`` over the ranked triples (``nan`` when there is none), ``skipped`` and
    ``ranks`` int64 ``(n,)`` in input order.  Memory as :func:`answer_relation`; one host read at the end."""
    triples = torch.as_tensor(triples, device=task.device).long()
    if triples.dim() != 2 or triples.shape[1] != 3:
        raise ValueError("evaluate_relations takes (n, 3) rows of (h, t, r), got %s" % (tuple(triples.shape),))
    validate_triples(task, triples)
    h, t, cand = task.relation_queries(triples[:, 0], triples[:, 1], candidates, inverse)
    keys = task.relation_filter(filtered)
    ranks = torch.zeros(len(triples), dtype=torch.int64, device=triples.device)
    for ids, block in _relation_blocks(task, h, t, cand, pair_batch, int(batch_size)):
        ranks[ids] = task._relation_select(block, cand, keys, h[ids], t[ids], triples[ids, 2], 1, ("rank",)).rank
    ranked = ranks[ranks > 0].double()
    result = {"skipped": int(len(ranks) - len(ranked)), "ranks": ranks}
    none = float("nan")
    result["mrr"] = float((1 / ranked).mean()) if len(ranked) else none
    result["mr"] = float(ranked.mean()) if len(ranked) else none
    for top in (1, 3, 10):
        result["hits@%d" % top] = float((ranked <= top).double().mean()) if len(ranked) else none
    return result


def explain(task, triples, batch_size=16, head=False):
    """``task.explain`` over any number of triples (``(n, 3)`` rows of (h, t, r) in the current context): range-checked once
    (:func:`validate_triples`), explained ``batch_size`` at a time (the last chunk is ragged), results in input order -- a list of
    ``n`` ``(paths, weights)`` pairs, each chunk equal to ``task.explain`` of its rows.  Activation memory grows with
    ``batch_size``: one ``(N, batch_size, D)`` tensor per layer is kept for the backward."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("explain: batch_size must be positive, got %d" % batch_size)
    triples = torch.as_tensor(triples, device=task.device).long()
    if triples.dim() != 2 or triples.shape[1] != 3:
        raise ValueError("explain takes (n, 3) rows of (h, t, r), got %s" % (tuple(triples.shape),))
    validate_triples(task, triples)
    results = []
    for i in range(0, len(triples), batch_size):
        results.extend(task.explain(triples[i:i + batch_size], head=head))
    return results


@torch.no_grad()
def answer_query(task, structure, anchors, relations, k=10, batch_size=16, filtered=False, **cut):
    """``task.answer_query`` over any number of queries of ONE structure: the ids are parsed and range-checked once, then the
    queries run ``batch_size`` at a time (the last chunk is ragged: nothing is padded, a set projection costs what its queries
    cost) and everything runs eager -- a whole query is not captured in a hipGraph.  ``cut``: ``threshold`` / ``max_sources`` of
    ``task.project``.  Queries are independent columns of every kernel on the route, so each chunk equals ``task.answer_query``
    of the same rows.  ``filtered``: as in ``task.answer_query``, the exact answers on the filter graph are left out.  Returns
    ``(entities int64 (Q, k), membership fp32 (Q, k))``."""
    unknown = set(cut) - {"threshold", "max_sources"}
    if unknown:
        raise TypeError("answer_query: unknown arguments %s" % sorted(unknown))
    threshold, max_sources = cut.get("threshold", 0.0), cut.get("max_sources")
    task._check_cut(max_sources)
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("answer_query: batch_size must be positive, got %d" % batch_size)
    tree, anchors, relations = task.query_inputs(structure, anchors, relations)
    parts = [task._answer_query_checked(tree, anchors[i:i + batch_size], relations[i:i + batch_size], k, threshold, max_sources,
                                        filtered)
             for i in range(0, len(anchors), batch_size)]
    if not parts:
        return task._answer_query_checked(tree, anchors, relations, k, threshold, max_sources, filtered)
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


@torch.no_grad()
def evaluate_queries(task, structure, anchors, relations, batch_size=16, threshold=0.0, max_sources=None, return_ranks=False):
    """Filtered ranking metrics of logical queries of ONE structure over their HARD answers.  With
    ``easy`` = the exact answers on the fact graph and ``full`` = those on the filter graph (``task.query_answer_bits``, all
    queries at once, 64 per machine word): ``hard = full & ~easy`` are the answers that need a held-out edge, and every hard
    answer is ranked by its membership (``task.query_memberships``, ``batch_size`` queries at a time, with the cut ``threshold``
    / ``max_sources``) among the entities outside ``excluded = easy | full`` and itself -- ``functional.set_ranks``, pessimistic
    on ties.  Per query with at least one hard answer: the mean over its hard answers of ``1 / rank``, ``rank`` and ``rank <=
    K``; the result is the mean of those over such queries, in float64 from the integer ranks: ``{"mrr", "mr", "hits@1",
    "hits@3", "hits@10", "num_queries", "num_evaluated", "num_hard_answers"}`` (the metrics are NaN when no query has a hard
    answer).  ``return_ranks``: also ``(query int64 (T,), entity int64 (T,), rank int64 (T,))``, ordered by query, then entity.
    The hard answers are listed with ``nonzero``: one host read, so this call is not captured."""
    from . import functional
    task._check_cut(max_sources)
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("evaluate_queries: batch_size must be positive, got %d" % batch_size)
    tree, anchors, relations = task.query_inputs(structure, anchors, relations)
    n_query, n_node, dev = len(anchors), task.num_entity, anchors.device
    if n_query:
        easy = task.query_answer_bits(tree, anchors, relations, "fact")
        full = task.query_answer_bits(tree, anchors, relations, "filter")
        hard = functional.unpack_sets(full & ~easy, n_query)
        query, entity = hard.nonzero(as_tuple=True)                               # ordered by query, then entity
        count = hard.sum(dim=1)
    else:
        query = entity = count = torch.zeros(0, dtype=torch.int64, device=dev)
    if len(query):
        scores = torch.cat([task.query_memberships(tree, anchors[i:i + batch_size], relations[i:i + batch_size], threshold,
                                                   max_sources).float() for i in range(0, n_query, batch_size)])
        target_ptr = torch.cat([count[:1] * 0, count.cumsum(0)])
        rank = functional.set_ranks(scores, easy | full, target_ptr, entity)
    else:
        rank = query
    ranks, owner, per_query = rank.cpu(), query.cpu(), count.cpu()
    evaluated = per_query > 0
    n_evaluated = int(evaluated.sum())

    def mean_of(values):
        if n_evaluated == 0:
            return float("nan")
        sums = torch.zeros(n_query, dtype=torch.float64).index_add_(0, owner, values.double())
        return float((sums[evaluated] / per_query[evaluated].double()).mean())

    result = {"mrr": mean_of(1.0 / ranks.double()), "mr": mean_of(ranks)}
    for k in (1, 3, 10):
        result["hits@%d" % k] = mean_of(ranks <= k)
    result.update(num_queries=n_query, num_evaluated=n_evaluated, num_hard_answers=int(len(ranks)))
    return (result, (query, entity, rank)) if return_ranks else result


# engine.evaluate scores distinct queries instead of triples when the shard holds at most this share of distinct queries
UNIQUE_QUERY_GAIN = 0.9


@torch.no_grad()
def evaluate(task, triples, batch_size=16, graphed=None, cache_relations=None, unique_queries=None, generator=None):
    """Filtered ranking of ``triples`` ((n, 3) rows of (h, t, r)) sharded over ranks; every rank returns the
    metrics of the WHOLE set.  Only int64 ranks cross ranks.  ``graphed`` (default: on a GPU, when the shard holds at
    least two full batches): ``predict`` is captured once and replayed as a hipGraph for every full batch.
    ``cache_relations`` (default: in eval mode, when the shard has more batches than the relation vocabulary needs
    passes): the relation representations of all R relations are computed once for the run
    (``task.cache_relation_representations``) instead of once per batch -- same bits, the relation stack leaves the
    per-batch path.  The cache is dropped before returning.  ``unique_queries`` (default: in eval mode on a GPU with
    full-batch evaluation, when at most ``UNIQUE_QUERY_GAIN`` of the shard's 2n queries are distinct): every distinct query
    of the shard is scored once (:func:`_ranks_of_unique_queries`) -- same ranks, fewer Bellman-Ford passes on test sets
    whose triples share heads or tails; on sets that repeat few queries the triple loop is the faster one and stays.
    A task with a sampled metric ``hits@K_N`` or ``toy_eval`` (``task.needs_statistics``) gathers the int64 ``(n, 2, 4)``
    ``task.rank_statistics`` instead of the ranks, through the same gather.  Under ``toy_eval`` the uniform numbers that define
    the draws come ONCE for the whole triple set, ``(len(triples), 2, 50)`` from ``generator`` (a ``torch.Generator`` of the
    task's device; in a process group rank 0's numbers are broadcast) and every triple uses its own row: the metrics do not depend on
    ``batch_size``, ``graphed``, ``unique_queries`` or the shard boundaries.  Returns ``(metrics, ranking)``; the ranking is
    the float ``0.5 * (optimistic + pessimistic) + 1`` under ``toy_eval``."""
    device = task.device
    mine = shard_indices(len(triples))
    local = validate_triples(task, triples[mine].to(device))
    statistics = task.needs_statistics
    rand = None
    if statistics and task.toy_eval:
        from .task import TOY_EVAL_SAMPLES
        rand = torch.rand(len(triples), 2, TOY_EVAL_SAMPLES, generator=generator, device=device)
        if get_world_size() > 1:
            dist.broadcast(rand, 0)         # ranks are seeded apart (seed + rank): every rank uses rank 0's numbers
        rand = rand[mine.to(device)]
    if graphed is None:
        graphed = device.type == "cuda" and len(local) >= 2 * batch_size and not task.training
    if cache_relations is None:
        cache_relations = not task.training and len(local) > task.num_relation
    if cache_relations:
        task.cache_relation_representations(batch_size)
    if unique_queries is None:
        unique_queries = (device.type == "cuda" and not task.training and task.full_batch_eval and task.fuse_sides
                          and len(local) > 0)
        if unique_queries:
            # worth it only where the shard repeats queries: a pass over 2B distinct queries costs what a batch of B triples
            # costs, plus the per-entry gather of score rows (measured: a set with ~2n distinct queries ran 285 ms this way
            # against 266 ms for the triple loop) -- one torch.unique and one host read per run decide
            h, t, r = local.t()
            n_rel = task.num_relation
            keys = torch.cat([h * (2 * n_rel) + r, t * (2 * n_rel) + r + n_rel])
            unique_queries = int(torch.unique(keys).numel()) <= UNIQUE_QUERY_GAIN * keys.numel()
    try:
        ranks = (_ranks_of_unique_queries(task, local, batch_size, graphed, statistics, rand)
                 if unique_queries and len(local) else None)
        if ranks is None:
            # predict AND the filtered ranking of a batch as one replay (only the (B, 2) ranks are copied out per batch)
            replay = GraphedPredict(task, local[:batch_size], with_ranks=True) if graphed and len(local) >= batch_size else None
            ranks = []
            for i in range(0, len(local), batch_size):
                batch = local[i:i + batch_size]
                if statistics:
                    batch_rand = None if rand is None else rand[i:i + batch_size]
                    ranks.append(replay.statistics(batch, batch_rand) if replay is not None
                                 else task.rank_statistics(batch, rand=batch_rand))
                else:
                    ranks.append(replay.ranks(batch) if replay is not None else task.rank_batch(batch))
            ranks = torch.cat(ranks) if ranks else torch.zeros((0, 2, 4) if statistics else (0, 2), dtype=torch.long, device=device)
    finally:
        if cache_relations:
            task.clear_relation_cache()
    if statistics:
        # (n, 2, 4) int64 through the one gather, beside the relation column when the metrics are grouped by it
        flat = ranks.reshape(len(ranks), 8)
        both = gather_variable(torch.cat([flat, local[:, 2:3]], dim=1) if task.metric_per_rel else flat)
        stats = both[:, :8].reshape(-1, 2, 4)
        ranking = task.toy_ranking(stats) if task.toy_eval else stats[..., 0].contiguous()
        rel = both[:, 8].contiguous() if task.metric_per_rel else None
        return task.evaluate(ranking, rel=rel, num_candidates=stats[..., 1].contiguous()), ranking
    if task.metric_per_rel:
        # the reference's target() returns the relation of every ranked triple beside the masks (task.py:290-292) and
        # evaluate() groups by it; one more column through the same gather
        both = gather_variable(torch.cat([ranks, local[:, 2:3]], dim=1))
        ranking = both[:, :2].contiguous()
        return task.evaluate(ranking, rel=both[:, 2].contiguous()), ranking
    ranking = gather_variable(ranks)
    return task.evaluate(ranking), ranking


@torch.no_grad()
def evaluate_by_distance(task, triples, max_hops=None, **evaluate_kwargs):
    """:func:`evaluate`, and its metrics again per hop distance between head and tail (the standard diagnostic of this model
    family: a model of L layers conditions a score on the anchor only within L hops, so a weak result on a new graph is either the
    model or the graph's diameter).  ``max_hops`` defaults to the number of layers.  :func:`evaluate` runs once, unchanged;
    ``distance`` = ``task.hop_distance(triples, num_iters=max_hops)`` is computed on every rank for the whole set (cheap, no
    collective).  Returns ``(by_distance, distance, ranking)``: ``by_distance`` maps ``0, 1, ..., max_hops`` and ``"beyond"``
    (farther than ``max_hops``, or unreachable) to ``{"count": rows, **task.evaluate(those rows)}`` with the ``rel=`` /
    ``num_candidates=`` arguments :func:`evaluate` passes, restricted to the rows; empty buckets are left out, and the buckets
    partition the triples.  ``distance`` int32 ``(n,)`` holds ``task.num_entity`` for "beyond"."""
    if max_hops is None:
        max_hops = len(task.model.layers)
    max_hops = int(max_hops)
    if max_hops < 0:
        raise ValueError("evaluate_by_distance: max_hops must not be negative, got %d" % max_hops)
    _, ranking = evaluate(task, triples, **evaluate_kwargs)
    triples = triples.to(task.device)
    distance = task.hop_distance(triples, num_iters=max_hops)
    rel = triples[:, 2].contiguous() if task.metric_per_rel else None
    num_candidates = None
    if task.needs_statistics:
        # what evaluate() gathered as rank_statistics column 1: the number of unfiltered candidates of either query of a triple
        from . import backend
        graph, (h, t, r) = task.graph, triples.t()
        if backend.get().accepts(triples):
            n_rel = max(graph.num_relation, 1)
            keys = (graph.completion_keys(0), graph.completion_keys(1)) if task.filtered_ranking else (None, None)
            num_candidates = torch.stack([backend.get().filter_counts(keys[0], h, r, n_rel, graph.num_node),
                                          backend.get().filter_counts(keys[1], t, r, n_rel, graph.num_node)], dim=1)
        else:
            batch_size = evaluate_kwargs.get("batch_size", 16)
            mask = [task.target(triples[i:i + batch_size])[0].sum(dim=-1) for i in range(0, len(triples), batch_size)]
            num_candidates = torch.cat(mask) if mask else torch.zeros(0, 2, dtype=torch.long, device=triples.device)
            if not task.filtered_ranking:
                num_candidates = torch.full_like(num_candidates, graph.num_node)
    by_distance = {}
    for name in list(range(max_hops + 1)) + ["beyond"]:
        rows = (distance > max_hops) if name == "beyond" else (distance == name)
        count = int(rows.sum())
        if count:
            by_distance[name] = {"count": count,
                                 **task.evaluate(ranking[rows], rel=None if rel is None else rel[rows],
                                                 num_candidates=None if num_candidates is None else num_candidates[rows])}
    return by_distance, distance, ranking


@torch.no_grad()
def evaluate_all(task, test_sets, batch_size=16, **kwargs):
    """Evaluation of multi-graph pre-training (``ultra/engine.py:100-159``): ``test_sets`` maps a graph context of
    ``task`` (``task.add_context``; the reference's ``graph_<id>``) to the ``(n, 3)`` triples of that graph's split; every
    graph is evaluated in turn with :func:`evaluate` (query-sharded over the ranks, one int64 rank gather per graph --
    the reference gathers each graph's score tensors) and the metrics are AVERAGED over the graphs with equal weight, as
    the reference does (``:154-157``).  Contexts are visited in sorted name order, so all ranks issue the same sequence
    of collectives.  Returns ``(mean metrics as floats, {graph: metrics}, {graph: ranking})``; the active context is
    restored afterwards.  ``generator`` (``toy_eval``) goes to every :func:`evaluate` in turn."""
    if not test_sets:
        raise ValueError("evaluate_all: no test sets")
    saved = task.split
    per_graph, rankings = {}, {}
    try:
        for name in sorted(test_sets, key=str):
            task.use(name)
            per_graph[str(name)], rankings[str(name)] = evaluate(task, test_sets[name], batch_size=batch_size, **kwargs)
    finally:
        if saved is not None:
            task.use(saved)
    names = list(per_graph[next(iter(per_graph))])
    mean = {k: float(sum(float(m[k]) for m in per_graph.values())) / len(per_graph) for k in names}
    return mean, per_graph, rankings


def sample_edges_from_graph(task, batch_size, generator=None):
    """Multi-graph pre-training batch (``ultra/engine.py:23-34``): draw a graph with probability proportional to its
    number of fact edges, then ``batch_size`` distinct fact edges of it.  Returns ``(triples, graph_id)``.  Every rank
    draws independently (ranks are seeded ``seed + rank``, ``script/run_full.py:102-107``), so ranks may train on
    different graphs in the same step; the gradient all-reduce is also the straggler barrier."""
    names = sorted(task.contexts)
    sizes = torch.tensor([task.contexts[n]["fact_graph"].num_edge for n in names], dtype=torch.float)
    graph_id = names[int(torch.multinomial(sizes / sizes.sum(), 1, generator=generator))]
    fact = task.contexts[graph_id]["fact_graph"]
    pick = torch.randperm(fact.num_edge, generator=generator)[:batch_size]
    return fact.edge_list[pick.to(fact.device)], graph_id


def allreduce_gradients(module, average=True):
    """One flat all-reduce over every parameter that has a gradient on this step.  Which parameters have one is
    a static property of the architecture, so all ranks build the same buffer."""
    world = get_world_size()
    params = [p for p in module.parameters() if p.grad is not None]
    if world == 1 or not params:
        return 0
    flat = torch.cat([p.grad.reshape(-1) for p in params])
    dist.all_reduce(flat)
    if average:
        flat /= world
    offset = 0
    for p in params:
        n = p.numel()
        p.grad.copy_(flat[offset:offset + n].view_as(p.grad))
        offset += n
    return flat.numel()


# parameters of the shipped architecture that never receive a gradient (the reference needs
# find_unused_parameters=True for them, ultra/engine.py:55-60): `dist_embed` is never used in forward
# (ultra/model.py:55) and the relation model's `mlp` is constructed but not called (ultra/rel_model.py:263,376-378)
UNUSED_PARAMETER_MARKS = ("model.dist_embed.", ".model.mlp.")


class GradientReducer:
    """Bucketed gradient all-reduce that overlaps the backward pass (what DDP does for the reference,
    ``ultra/engine.py:55-60``; BASELINE north star: "overlapped with the next layer's rspmm on a side HIP stream").

    BUCKETS follow the order in which backward produces gradients: the score head first, then the entity layers last to
    first (each layer's ``linear`` + ``layer_norm``: ready right after its rspmm backward), then ONE bucket with the relation
    projections of all entity layers (a single grouped autograd node that runs after the first layer's backward; round 3 kept
    them in their layers' buckets, so no entity bucket could leave before the whole entity stack was done), then the
    relation-model layers last to first.  All buckets are slices of ONE persistent flat buffer (allocated once: nothing is
    allocated or freed per step).  GROUPS are runs of consecutive buckets that complete in one phase of the backward -- (0) the
    score head and the later half of the entity layers, (1) the earlier entity layers and the projections, (2) the relation
    model -- and a group is the unit of communication: ONE all-reduce over the group's contiguous slice, enqueued on a SIDE
    stream as soon as the group's last bucket is packed (RCCL runs it there while the compute stream continues with the next
    layers' backward).  Three collectives per step instead of fourteen: on xGMI a 30-200 KB all-reduce is latency, not bandwidth
    (the reference's DDP sends its 0.78 MB of gradients as one bucket).  Every path -- eager hooks, ``finish()`` after a paused
    backward, the phased captured step -- sends the SAME groups in the same order, so ranks in different modes or on different
    graphs (multi-graph pre-training, ``ultra/engine.py:23-34``) issue identical sequences of collectives.

    A ``post_accumulate_grad`` hook per parameter counts a bucket down; complete buckets are packed on the compute stream in bucket
    order (one ``cat`` kernel each).  ``finish()`` makes the compute stream wait for the side stream and unpacks the averaged
    gradients; it must run before ``optimizer.step()`` and after EVERY backward whose hooks were live (a backward without it
    leaves groups in flight: a second one is refused).  Parameters that never receive a gradient (``UNUSED_PARAMETER_MARKS``)
    are excluded statically."""

    def __init__(self, module, average=True, overlap=True, single_rank=False):
        """``single_rank``: issue the collectives even in a one-rank group (a one-GPU box can then exercise the RCCL
        path -- streams, hooks, packing -- end to end; the reduction itself is the identity there)."""
        self.module, self.average, self.overlap = module, average, overlap
        self.single_rank = single_rank
        named = [(k, p) for k, p in module.named_parameters()
                 if p.requires_grad and not any(mark in k for mark in UNUSED_PARAMETER_MARKS)]

        def bucket_key(name):
            parts = name.split(".")
            if "relation_projection" in parts:
                # the grouped projections of ALL entity layers are one autograd node whose backward runs after the first
                # entity layer's (model._relation_tables): their gradients become ready together, late -- in a bucket of
                # their own, or every entity layer's bucket would wait for them and nothing would overlap
                return (2, 0, parts[0] + ".relation_projections")
            if "layers" in parts and not name.startswith("model.mlp"):
                i = parts.index("layers")
                stack = 0 if parts[0] == "model" else 1
                return (1 + 2 * stack, -int(parts[i + 1]), ".".join(parts[:i + 2]))
            return (0, 0, parts[0] + "." + parts[1] if len(parts) > 1 else parts[0])      # score head, query embeddings

        by_key = {}
        for name, p in named:
            by_key.setdefault(bucket_key(name), []).append((name, p))
        keys = sorted(by_key)
        self.buckets = []
        for key in keys:
            params = [p for _, p in by_key[key]]
            self.buckets.append({"name": key[2], "params": params, "names": [n for n, _ in by_key[key]],
                                 "numel": sum(p.numel() for p in params), "flat": None})
        self._bucket_of = {}
        for b, bucket in enumerate(self.buckets):
            for p in bucket["params"]:
                self._bucket_of[id(p)] = b
        # groups: where the phased backward is cut (GraphedTrainStep) -- after the entity layer model.cut_at() (the middle)
        model = getattr(module, "model", None)
        cut = model.cut_at() if hasattr(model, "cut_at") else None
        if not isinstance(cut, int):
            entity = [-key[1] for key in keys if key[0] == 1]
            cut = (max(entity) + 1) // 2 if entity else 0
        self.cut_after = cut
        phases = [0 if key[0] == 0 else ((0 if -key[1] >= cut else 1) if key[0] == 1 else (1 if key[0] == 2 else 2)) for key in keys]
        self.groups = []
        for b, phase in enumerate(phases):              # (phases are non-decreasing in bucket order)
            if not self.groups or phases[b - 1] != phase:
                self.groups.append([])
            self.groups[-1].append(b)
        self._group_of = {b: g for g, group in enumerate(self.groups) for b in group}
        self._flat_all = None
        self._group_flat = [None] * len(self.groups)
        self._work = [None] * len(self.groups)
        self._side = None
        self._handles = []
        self._paused = False
        self.launched_from_hooks = 0            # buckets packed (and their groups sent) from hooks, i.e. during backward, last step
        self.total_launched = 0                 # buckets whose reduction was issued since construction (gradient rounds + warm())
        self.collectives = 0                    # all-reduce calls issued since construction
        self.sent = []                          # (group, elements) of the last 64 collectives, in issue order: what a rank SAID
        self.rounds = 0                         # completed rounds that carried gradients
        self._reset()
        if overlap:
            for bucket in self.buckets:
                for p in bucket["params"]:
                    self._handles.append(p.register_post_accumulate_grad_hook(self._on_grad))

    def _reset(self):
        self._pending = [len(b["params"]) for b in self.buckets]
        self._ready = [False] * len(self.buckets)
        self._next = 0                          # next bucket to pack / send
        self._launched = 0
        self._from_hooks = 0

    def remove_hooks(self):
        for h in self._handles:
            h.remove()
        self._handles = []

    def paused(self):
        """Context in which the hooks do nothing (a backward whose gradients are reduced later by ``reduce_all()``, e.g.
        the capture of a step whose collectives stay outside the graph)."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            saved, self._paused = self._paused, True
            try:
                yield self
            finally:
                self._paused = saved
        return ctx()

    def abandon(self):
        """Forget groups in flight (after a failed capture: their work handles belong to a dead graph)."""
        self._work = [None] * len(self.groups)
        self._reset()

    def _active(self):
        return dist.is_initialized() and (get_world_size() > 1 or self.single_rank)

    def _op(self):
        """Averaging inside the collective where the backend has it (RCCL: no division kernel per group); gloo sums."""
        if self.average and get_world_size() > 1 and dist.get_backend() == "nccl":
            return dist.ReduceOp.AVG, False
        return dist.ReduceOp.SUM, self.average and get_world_size() > 1

    # ------------------------------------------------------------------ buffers
    def flat_buffers(self, device):
        """The persistent flat buffer (allocated on first use, never per step): one slice per bucket, one per group."""
        if self._flat_all is None or self._flat_all.device != device:
            self._flat_all = torch.zeros(sum(b["numel"] for b in self.buckets), dtype=torch.float32, device=device)
            offset = 0
            for g, group in enumerate(self.groups):
                first = offset
                for b in group:
                    self.buckets[b]["flat"] = self._flat_all[offset:offset + self.buckets[b]["numel"]]
                    offset += self.buckets[b]["numel"]
                self._group_flat[g] = self._flat_all[first:offset]
        return [bucket["flat"] for bucket in self.buckets]

    def views(self):
        """``{id(param): view of its slice of the flat buffer}``: a step that packs its gradients into the flat buffer binds
        these as ``param.grad`` -- the all-reduce then happens in place under the optimizer's feet and nothing is unpacked."""
        out = {}
        for bucket in self.buckets:
            offset = 0
            for p in bucket["params"]:
                out[id(p)] = bucket["flat"][offset:offset + p.numel()].view_as(p)
                offset += p.numel()
        return out

    def pack(self, b, grads):
        """Bucket ``b``'s gradients (``{id(param): tensor}``; a parameter without one counts as zeros) into its slice of the flat
        buffer: ONE kernel on the current stream (``cat``; ``copy_()`` of same-dtype tensors would be a device-to-device memcpy,
        i.e. a memcpy NODE under hipGraph capture: kernels only, see DESIGN.md on memset nodes), capturable."""
        bucket = self.buckets[b]
        torch.cat([(grads[id(p)] if grads.get(id(p)) is not None else torch.zeros_like(p)).reshape(-1)
                   for p in bucket["params"]], out=bucket["flat"])

    def _send(self, g):
        """The all-reduce of group ``g`` (already packed): on the side stream, behind everything the compute stream has been
        given so far."""
        flat = self._group_flat[g]
        op = self._op()[0]
        if flat.is_cuda:
            if self._side is None:
                self._side = torch.cuda.Stream(device=flat.device)
            self._side.wait_stream(torch.cuda.current_stream(flat.device))   # the packs must be complete
            with torch.cuda.stream(self._side):
                self._work[g] = dist.all_reduce(flat, op=op, async_op=True)  # RCCL, enqueued behind the side stream
        else:
            self._work[g] = dist.all_reduce(flat, op=op, async_op=True)
        self.collectives += 1
        self.sent = (self.sent + [(g, int(flat.numel()))])[-64:]

    def warm(self):
        """One explicit all-reduce per group, in order, on the side stream: initialises RCCL's channels and allocates the
        persistent flat buffer outside any captured or timed step.  A collective like any other: every rank must call it at
        the same point (the constructors of the graphed steps do).  Gradients are not touched.  Returns the number of
        collectives issued."""
        if not self._active():
            return 0
        self.flat_buffers(next(p.device for b in self.buckets for p in b["params"]))
        for g, group in enumerate(self.groups):
            self._send(g)
            self.total_launched += len(group)
        for g in range(len(self.groups)):
            self._work[g].wait()
            self._work[g] = None
        return len(self.groups)

    # ------------------------------------------------------------------ hooks (autograd thread, during backward)
    def _on_grad(self, param):
        if self._paused or not self._active():
            return
        b = self._bucket_of[id(param)]
        self._pending[b] -= 1
        if self._pending[b] < 0:
            raise RuntimeError("GradientReducer: a second backward reached bucket `%s` before finish() -- call finish() "
                               "after every backward (or run the backward under paused())" % self.buckets[b]["name"])
        if self._pending[b] == 0:
            self._ready[b] = True
            while self._next < len(self.buckets) and self._ready[self._next]:
                self._launch(self._next)
                self._from_hooks += 1

    def _launch(self, b):
        """Pack bucket ``b`` from the parameters' ``.grad`` (always in bucket order) and, when it completes its group, send
        the group."""
        if b != self._next:
            raise RuntimeError("GradientReducer: bucket %d packed out of order (next is %d)" % (b, self._next))
        bucket = self.buckets[b]
        ref = next((p.grad for p in bucket["params"] if p.grad is not None), bucket["params"][0])
        self.flat_buffers(ref.device)
        self.pack(b, {id(p): p.grad for p in bucket["params"]})
        self._next += 1
        self._launched += 1
        self.total_launched += 1
        g = self._group_of[b]
        if b == self.groups[g][-1]:
            self._send(g)

    # ------------------------------------------------------------------ phased steps (engine.GraphedTrainStep)
    def launch_group(self, g):
        """All-reduce group ``g``, whose buckets the caller has packed (:meth:`pack`, e.g. as the last kernels of a captured
        phase): the groups go out in order; the compute stream goes on (the next phase's replay) while RCCL works.
        :meth:`wait_groups` ends the round."""
        if not self._active():
            return
        group = self.groups[g]
        if group[0] != self._next:
            raise RuntimeError("GradientReducer: group %d sent out of order (next bucket is %d): every rank must issue the "
                               "groups in the same order" % (g, self._next))
        self._send(g)
        self._next = group[-1] + 1
        self._launched += len(group)
        self.total_launched += len(group)

    def _wait_all(self):
        divide = self._op()[1]
        for g in range(len(self.groups)):
            self._work[g].wait()                    # the current stream (or the host, gloo) waits for this collective
            if divide:                              # (gloo only: RCCL averages inside the collective)
                self._group_flat[g].div_(get_world_size())
            self._work[g] = None

    def wait_groups(self):
        """The compute stream waits for every group sent by :meth:`launch_group`; the flat buffer then holds the averaged
        gradients (bound as ``param.grad`` through :meth:`views`).  All groups must have been sent."""
        if not self._active():
            self._reset()
            return
        if self._next != len(self.buckets):
            raise RuntimeError("GradientReducer: %d of %d buckets were sent in this round" % (self._next, len(self.buckets)))
        self._wait_all()
        self.rounds += 1
        self._reset()

    # ------------------------------------------------------------------ after backward, before optimizer.step()
    def finish(self):
        """Wait for every group (packing and sending those the hooks did not: ``overlap=False``, ``paused()`` or a graph
        replay) and write the reduced gradients back.  Returns the number of fp32 elements reduced."""
        if not self._active():
            self._reset()
            return 0
        while self._next < len(self.buckets):                               # in bucket order, on every rank
            self._launch(self._next)
        self._wait_all()
        total = 0
        for bucket in self.buckets:
            flat = bucket["flat"]
            offset = 0
            for p in bucket["params"]:
                n = p.numel()
                if p.grad is None:
                    p.grad = flat[offset:offset + n].view_as(p).clone()
                else:                                                       # an elementwise kernel, not a memcpy (see pack)
                    torch.mul(flat[offset:offset + n].view_as(p.grad), 1.0, out=p.grad)
                offset += n
            total += flat.numel()
        self.launched_from_hooks = self._from_hooks
        self.rounds += 1
        self._reset()
        return total

    reduce_all = finish


def reduce_metrics(metric):
    """Mean over ranks of a dict of 0-d tensors, in one packed all-reduce (``ultra/engine.py:90``)."""
    world = get_world_size()
    if world == 1 or not metric:
        return metric
    keys = sorted(metric)
    packed = torch.stack([metric[k].detach().float().reshape(()) for k in keys])
    dist.all_reduce(packed)
    packed /= world
    return {k: packed[i] for i, k in enumerate(keys)}


def train_step(task, optimizer, batch, reducer=None, communicate=True, guard=None):
    """One fine-tuning step (``ultra/engine.py:62-92`` / torchdrug ``Engine.train``): forward, backward,
    gradient all-reduce, optimizer step.  Returns (loss, metrics averaged over ranks).  ``reducer``: a
    :class:`GradientReducer` over ``task`` -- its hooks start each layer's all-reduce on a side stream while backward
    is still running; without one the gradients go through one flat blocking all-reduce after backward.
    ``communicate=False`` (timing only: what the collectives cost): no cross-rank traffic at all -- the backward runs with the
    reducer's hooks paused, no gradient and no metric reduce.  ``guard``: a :class:`FiniteGuard` -- the step raises
    :class:`NonFiniteError` before ``optimizer.step()`` when its loss, a parameter or a gradient is not finite (the gradient
    all-reduce of the step has been issued and retired by then, on every rank)."""
    return _train_step(task, optimizer, lambda: task(batch), reducer, communicate, guard)


def train_query_step(task, optimizer, structure, anchors, relations, positives, negatives, reducer=None, communicate=True,
                     guard=None, **cut):
    """One training step over logical queries of ONE structure (an addition of this package):
    :func:`train_step` with ``task.query_loss(structure, anchors, relations, positives, negatives, **cut)`` as the loss --
    the same backward, guard, gradient reduce and optimizer step, so a :class:`FiniteGuard` and the reducers work unchanged.
    ``cut``: ``threshold`` / ``max_sources`` of ``task.answer_query``.  Eager only (no captured form).  Returns ``(loss,
    metrics)`` with the loss as the one metric, ``"query binary cross entropy"``."""

    def compute():
        loss = task.query_loss(structure, anchors, relations, positives, negatives, **cut)
        return loss, {"query binary cross entropy": loss.detach()}

    return _train_step(task, optimizer, compute, reducer, communicate, guard)


def _train_step(task, optimizer, compute, reducer, communicate, guard):
    """:func:`train_step` around ``compute() -> (loss, metric)``."""
    import contextlib
    if guard is not None:
        guard.raise_if_tripped()
        guard.scan_parameters()
    loss, metric = compute()
    optimizer.zero_grad(set_to_none=True)
    with (reducer.paused() if (reducer is not None and not communicate) else contextlib.nullcontext()):
        loss.backward()
    if guard is not None:                           # this rank's own gradients: before the all-reduce mixes the ranks'
        guard.scan_loss(loss)
        guard.scan_gradients()
        guard.commit()
    if communicate:
        if reducer is not None:
            reducer.finish()
        else:
            allreduce_gradients(task)
    if guard is not None:
        guard.poll(communicate)
    optimizer.step()
    return loss.detach(), (reduce_metrics(metric) if communicate else metric)
