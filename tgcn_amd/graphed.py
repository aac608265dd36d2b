"""A whole training step as one hipGraph: GraphedTrainStep.  The reference-sized training shapes are bound by the host --
Python and the autograd engine issue a step more slowly than the device runs it -- and a replayed capture issues it in microseconds.
Inference on the streaming layers has the same as nn.GraphedStream."""
import inspect

import torch

from . import _lib, nn as _nn

_OTHER_SHAPES = ("raise", "eager")


def _as_tuple(inputs, who):
    """the tensors of an `inputs` argument: one tensor, or a tuple / list of tensors passed as model(*inputs)"""
    tup = (inputs,) if isinstance(inputs, torch.Tensor) else (tuple(inputs) if isinstance(inputs, (tuple, list)) else None)
    if not tup or not all(isinstance(t, torch.Tensor) for t in tup):
        raise _lib.TgcnError("GraphedTrainStep: %s is a tensor or a non-empty tuple of tensors, got %s" % (who, type(inputs).__name__))
    return tup


def _freeze(v):
    """a hyper-parameter as something a compare is cheap and safe on (lists as tuples: betas)"""
    return tuple(_freeze(x) for x in v) if isinstance(v, (list, tuple)) else v


def _hyper(optimizer):
    """the non-tensor entries of every param group (lr, momentum, weight_decay, betas, eps, flags ...), per group in key order: what a capture
    bakes in.  Tensor entries (a tensor lr) live on the device and are read by the replay."""
    return [[(k, _freeze(v)) for k, v in g.items() if k != "params" and not isinstance(v, torch.Tensor)] for g in optimizer.param_groups]


def _hyper_changed(optimizer, recorded):
    """True when an entry recorded at capture has another value now (host compare, no device work).  Keys added since -- a scheduler's
    initial_lr -- are none of the step's."""
    groups = optimizer.param_groups
    if len(groups) != len(recorded):
        return True
    for g, rec in zip(groups, recorded):
        for k, v in rec:
            if k not in g or _freeze(g[k]) != v:
                return True
    return False


def _same(t, ref):
    return t.shape == ref.shape and t.dtype == ref.dtype and t.device == ref.device


class GraphedTrainStep:
    """One training step -- optimizer.zero_grad(set_to_none=True); loss = loss_fn(model(*inputs), target); loss.backward(); optimizer.step() --
    captured into ONE hipGraph and replayed batch after batch:

        gts = tgcn_amd.GraphedTrainStep(model, optimizer, loss_fn, example_inputs, example_target)
        for x, y in loader:
            loss = gts(x, y)

    inputs is a tensor or a tuple of tensors (model(*inputs): ChebConv models take edge_index there); loss_fn(output, target) returns a 0-dim
    tensor.  gts(inputs, target) copies the batch into static buffers, replays the graph and returns the STATIC 0-dim loss tensor;
    gts.output is the STATIC model output of that step.  The next call overwrites both, and a recapture (below) replaces both tensors by
    new ones: clone() or float() what must be kept, and take gts.output afresh after every call.  An input passed as the very object of
    example_inputs, unmodified since, is not copied again while the static buffer still holds it (an edge_index: its operand is keyed on the
    static copy, which then never changes).  The GRAPH is baked in like the shapes: the layers build their operand from the example's
    edge_index / edge_weight in the warm-up and a replay does not build -- pass the same graph arguments on every call; other VALUES in
    them are not noticed (comparing would synchronise), so another graph needs another GraphedTrainStep.

    Construction is not a training step.  `warmup` >= 1 eager steps run on a side stream (they build the layers' graph operands, their
    transposes and lazily loaded code); then everything they moved is put back in place -- parameters and buffers of the model (BatchNorm
    running statistics and num_batches_tracked included), parameters the optimizer holds besides, the device's RNG state -- and the
    optimizer's state: a state tensor that existed is copied back, one the warm-up made is zeroed, because the captured step updates those
    very tensors.  A zeroed momentum buffer makes the first replayed SGD step buf = mu * 0 + g, torch's first step buf = g bit for bit at
    dampening == 0 only, so momentum with dampening != 0 is refused.  Then one step is captured on static copies of the examples.

    Hyper-parameters: the non-tensor entries of optimizer.param_groups (lr, momentum, weight_decay, betas, eps ...) are Python numbers that
    a capture bakes in.  They are recorded at capture and compared at every call (a host compare); when one differs the step is captured
    again on the same static buffers, parameters and optimizer state, and gts.recaptures counts it.  scheduler.step() once per epoch works
    unchanged; a schedule that moves them on every call recaptures on every call -- keep the learning rate in a tensor then, where the
    optimizer takes one.

    Batches of another shape, dtype or device than the examples: other_shapes="raise" (default) raises TgcnError -- one graph per batch
    shape; other_shapes="eager" runs that batch through the same step eagerly on the same model and optimizer (the short last batch of a
    DataLoader epoch) and returns a fresh loss tensor; gts.output is then that step's output.

    TgcnError before any warm-up step runs: warmup not an integer >= 1; other_shapes not "raise" / "eager"; model or loss_fn not callable,
    model not a torch.nn.Module; model.training False (the capture bakes the mode: a call with model.training changed since raises too); an
    optimizer that is no torch.optim.Optimizer, whose step needs a closure (LBFGS), whose param groups carry capturable=False (the Adam
    family keeps its step counter on the host then: construct it with capturable=True), or with momentum and dampening != 0; example
    tensors that are not on a ROCm device, parameters on another device.  After the first warm-up step: a loss that is not 0-dim.  After the
    warm-up (state restored): a step that trains edge weights (a learnable edge_weight on ChebConv / ChebTimeConv / spmm is re-packed into
    the operand by host-driven passes a replay cannot repeat).
    What a step may contain: the five layer classes in float32 and bfloat16, cheb_relu_pool, cheb_relu_dropout_pool, cheb_series_relu_pool,
    cheb_series_relu_dropout_pool (seed=None: a new mask on every replay; a one-element int64 seed tensor is the caller's to rewrite between
    calls), forward_series with time_chunk= and cheb_series_relu_pool_chunked (the chunk loop is unrolled into the graph; its ring is made
    zero inside the captured region), forward_series(fused=True), torch layers.  A layer that would build a graph operand during a capture
    raises TgcnError rather than synchronise.  Not covered by a test: the large-graph compact forward, which runs its projections on a side
    stream beside the hops -- a captured step that contains it has parallel branches."""

    def __init__(self, model, optimizer, loss_fn, example_inputs, example_target, warmup=3, other_shapes="raise"):
        who = "GraphedTrainStep"
        if not isinstance(warmup, int) or isinstance(warmup, bool) or warmup < 1:
            raise _lib.TgcnError("%s: warmup is an integer >= 1 (the first eager step builds the operands), got %r" % (who, warmup))
        if not (isinstance(other_shapes, str) and other_shapes in _OTHER_SHAPES):
            raise _lib.TgcnError("%s: other_shapes is \"raise\" or \"eager\", got %r" % (who, other_shapes))
        if not callable(model) or not isinstance(model, torch.nn.Module):
            raise _lib.TgcnError("%s: model is a (callable) torch.nn.Module, got %s" % (who, type(model).__name__))
        if not callable(loss_fn):
            raise _lib.TgcnError("%s: loss_fn(output, target) is callable, got %s" % (who, type(loss_fn).__name__))
        if not model.training:
            raise _lib.TgcnError("%s: model.training is False -- a training step is captured in training mode (model.train()); the capture "
                                 "bakes the mode in" % who)
        if not isinstance(optimizer, torch.optim.Optimizer):
            raise _lib.TgcnError("%s: optimizer is a torch.optim.Optimizer, got %s" % (who, type(optimizer).__name__))
        closure = inspect.signature(optimizer.step).parameters.get("closure")
        if isinstance(optimizer, torch.optim.LBFGS) or (closure is not None and closure.default is inspect.Parameter.empty):
            raise _lib.TgcnError("%s: %s.step needs a closure that re-evaluates the model, which one captured step cannot be"
                                 % (who, type(optimizer).__name__))
        for g in optimizer.param_groups:
            if g.get("capturable", None) is False:
                raise _lib.TgcnError("%s: %s keeps its step counter on the host with capturable=False, which a replay cannot move -- "
                                     "construct the optimizer with capturable=True" % (who, type(optimizer).__name__))
            if g.get("momentum", 0) != 0 and g.get("dampening", 0) != 0:
                raise _lib.TgcnError("%s: momentum with dampening != 0 is not supported -- the first replayed step starts from a zeroed "
                                     "momentum buffer, which equals torch's first step at dampening == 0 only" % who)
        inputs, target = _as_tuple(example_inputs, "example_inputs"), example_target
        if not isinstance(target, torch.Tensor):
            raise _lib.TgcnError("%s: example_target is a tensor, got %s" % (who, type(target).__name__))
        _lib.require_device(*inputs, target)
        device = inputs[0].device
        held = list(model.parameters()) + [p for g in optimizer.param_groups for p in g["params"]]
        for t in list(inputs) + [target] + held:
            if t.device != device:
                raise _lib.TgcnError("%s: the example tensors and all parameters are on one device, got %s and %s" % (who, device, t.device))

        self.model, self.optimizer, self.loss_fn, self.other_shapes = model, optimizer, loss_fn, other_shapes
        self.recaptures = 0
        self._device = device
        self._examples = inputs + (target,)
        self._in = tuple(t.detach().clone() for t in self._examples)       # the static batch: inputs..., target
        self._versions = tuple(t._version for t in self._examples)
        self._holds_example = [True] * len(self._in)
        self.graph = self._loss = self._out = self.output = None

        moved, seen = [], set()
        for t in held + list(model.buffers()):
            if id(t) not in seen:
                seen.add(id(t))
                moved.append(t)
        with torch.cuda.device(device):
            before = [t.detach().clone() for t in moved]
            opt_before = {p: {k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in st.items()}
                          for p, st in optimizer.state.items()}
            rng = torch.cuda.get_rng_state(device)
            side = torch.cuda.Stream()
            notes = _nn._warmup_notes = []
            try:
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(warmup):
                        optimizer.zero_grad(set_to_none=True)
                        loss = loss_fn(model(*self._in[:-1]), self._in[-1])
                        if not isinstance(loss, torch.Tensor) or loss.dim() != 0:
                            raise _lib.TgcnError("%s: loss_fn(output, target) returns a 0-dim tensor, got %s" % (
                                who, tuple(loss.shape) if isinstance(loss, torch.Tensor) else type(loss).__name__))
                        loss.backward()
                        optimizer.step()
                    loss = None
            finally:
                _nn._warmup_notes = None
                torch.cuda.current_stream().wait_stream(side)
                self._restore(moved, before, opt_before, rng)
            if notes:
                raise _lib.TgcnError(notes[0])
            self._capture()

    def _restore(self, moved, before, opt_before, rng):
        """put back what the warm-up steps moved, in place: the captured step updates these very tensors"""
        with torch.no_grad():
            for t, t0 in zip(moved, before):
                t.copy_(t0)
            for p, st in self.optimizer.state.items():
                old = opt_before.get(p, {})
                for k, v in st.items():
                    if isinstance(v, torch.Tensor):
                        if isinstance(old.get(k), torch.Tensor):
                            v.copy_(old[k])
                        else:
                            v.zero_()
                    elif k in old:
                        st[k] = old[k]
        self.optimizer.zero_grad(set_to_none=True)
        torch.cuda.set_rng_state(rng, self._device)

    def _step(self, inputs, target):
        self.optimizer.zero_grad(set_to_none=True)
        out = self.model(*inputs)
        loss = self.loss_fn(out, target)
        loss.backward()
        self.optimizer.step()
        return loss.detach(), (out.detach() if isinstance(out, torch.Tensor) else out)

    def _capture(self):
        """one step on the static batch into a new graph; the gradients of the step before are dropped first, so that the backward writes new
        ones inside the graph's own memory"""
        self.graph = self._loss = self._out = self.output = None
        self.optimizer.zero_grad(set_to_none=True)
        hyper = _hyper(self.optimizer)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.device(self._device):
            with torch.cuda.graph(graph):
                loss, out = self._step(self._in[:-1], self._in[-1])
        self.graph, self._loss, self._out, self.output, self._hyper = graph, loss, out, out, hyper

    def __call__(self, inputs, target):
        batch = _as_tuple(inputs, "inputs") + (target,)
        if not self.model.training:
            raise _lib.TgcnError("GraphedTrainStep: model.training is False, the step was captured in training mode -- the capture bakes the "
                                 "mode in (model.train(), or run the evaluation outside this object)")
        if len(batch) != len(self._in) or not isinstance(target, torch.Tensor) or not all(_same(t, s) for t, s in zip(batch, self._in)):
            if self.other_shapes == "eager" and len(batch) == len(self._in) and isinstance(target, torch.Tensor):
                loss, self.output = self._step(batch[:-1], target)
                return loss
            raise _lib.TgcnError("GraphedTrainStep: captured for a batch of %s, got %s -- one graph per batch shape (other_shapes=\"eager\" "
                                 "runs such a batch eagerly)" % (self._describe(self._in), self._describe(batch)))
        if _hyper_changed(self.optimizer, self._hyper):
            self._capture()
            self.recaptures += 1
        for i, (t, s) in enumerate(zip(batch, self._in)):
            example = t is self._examples[i] and t._version == self._versions[i]
            if example and self._holds_example[i]:
                continue        # the example object itself, unmodified, and nothing else copied in since: the static copy holds it already
            s.copy_(t)
            self._holds_example[i] = example
        self.graph.replay()
        self.optimizer._opt_called = True      # what a scheduler's wrapper of optimizer.step notes: the step has run (its warning asks)
        self.output = self._out
        return self._loss

    @staticmethod
    def _describe(batch):
        return ", ".join("%s %s on %s" % (tuple(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t).__name__ for t in batch)
