"""GraphedTrainStep's refusals that need no device, in the order the constructor makes them, and the capture guard of the operand
caches with the capture state monkeypatched.  No GPU."""
import hashlib
import inspect

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib, functional as F, nn as tnn


class _Unreachable(torch.nn.Module):
    """a model whose forward fails the test when a refusal lets a warm-up step through"""

    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(3, 2)

    def forward(self, x):
        raise AssertionError("the model was called: the refusal came too late")


def _loss(out, y):
    raise AssertionError("loss_fn was called: the refusal came too late")


def _args(model=None, opt=None):
    model = _Unreachable() if model is None else model
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.5) if opt is None else opt
    return model, opt, _loss, torch.zeros(4, 3), torch.zeros(4, dtype=torch.long)


def test_exported():
    assert tgcn_amd.GraphedTrainStep is tgcn_amd.graphed.GraphedTrainStep
    assert list(inspect.signature(tgcn_amd.GraphedTrainStep.__init__).parameters) == [
        "self", "model", "optimizer", "loss_fn", "example_inputs", "example_target", "warmup", "other_shapes"]
    sig = inspect.signature(tgcn_amd.GraphedTrainStep.__init__).parameters
    assert sig["warmup"].default == 3 and sig["other_shapes"].default == "raise"


def test_graphed_stream_is_untouched():
    assert str(inspect.signature(tgcn_amd.GraphedStream.__init__)) == "(self, step, example_chunk, warmup=3)"
    assert str(inspect.signature(tgcn_amd.GraphedStream.__call__)) == "(self, chunk)"
    assert hashlib.sha256(tgcn_amd.GraphedStream.__doc__.encode()).hexdigest() == \
        "e94ea77aed9a55df1b018d55e6db1ed8499d2e2f38e8d4e6a408e9ed01e9bc99"


@pytest.mark.parametrize("warmup", [0, -1, 2.0, True, None, "3"])
def test_refuses_warmup(warmup):
    with pytest.raises(_lib.TgcnError, match="warmup is an integer >= 1"):
        tgcn_amd.GraphedTrainStep(*_args(), warmup=warmup)


@pytest.mark.parametrize("other", ["Raise", "skip", None, 0])
def test_refuses_other_shapes(other):
    with pytest.raises(_lib.TgcnError, match="other_shapes is"):
        tgcn_amd.GraphedTrainStep(*_args(), other_shapes=other)


def test_refuses_what_is_not_callable():
    model, opt, _, x, y = _args()
    with pytest.raises(_lib.TgcnError, match="loss_fn.*callable"):
        tgcn_amd.GraphedTrainStep(model, opt, 3.0, x, y)
    with pytest.raises(_lib.TgcnError, match="model is a"):
        tgcn_amd.GraphedTrainStep(object(), opt, _loss, x, y)
    with pytest.raises(_lib.TgcnError, match="model is a"):
        tgcn_amd.GraphedTrainStep(lambda x: x, opt, _loss, x, y)


def test_refuses_eval_mode():
    model = _Unreachable().eval()
    with pytest.raises(_lib.TgcnError, match="model.training is False"):
        tgcn_amd.GraphedTrainStep(*_args(model))


def test_refuses_adam_that_counts_on_the_host():
    model = _Unreachable()
    with pytest.raises(_lib.TgcnError, match="capturable=True"):
        tgcn_amd.GraphedTrainStep(*_args(model, torch.optim.Adam(model.parameters(), lr=1e-3)))
    with pytest.raises(_lib.TgcnError, match="capturable=True"):
        tgcn_amd.GraphedTrainStep(*_args(model, torch.optim.AdamW(model.parameters(), lr=1e-3)))


def test_refuses_a_closure_optimizer():
    model = _Unreachable()
    with pytest.raises(_lib.TgcnError, match="closure"):
        tgcn_amd.GraphedTrainStep(*_args(model, torch.optim.LBFGS(model.parameters())))


def test_refuses_dampening_with_momentum():
    model = _Unreachable()
    with pytest.raises(_lib.TgcnError, match="dampening"):
        tgcn_amd.GraphedTrainStep(*_args(model, torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.5, dampening=0.1)))
    # dampening without momentum is no momentum buffer at all: the device check is reached
    with pytest.raises(_lib.TgcnError, match="no CPU fallback"):
        tgcn_amd.GraphedTrainStep(*_args(model, torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.0, dampening=0.1)))


def test_refuses_what_is_not_an_optimizer():
    model, _, _, x, y = _args()
    with pytest.raises(_lib.TgcnError, match="torch.optim.Optimizer"):
        tgcn_amd.GraphedTrainStep(model, object(), _loss, x, y)


def test_cpu_examples_reach_the_device_check_last():
    """every host check passes: the example tensors' device is what is refused, still before the model runs"""
    with pytest.raises(_lib.TgcnError, match="needs tensors on a ROCm device.*no CPU fallback"):
        tgcn_amd.GraphedTrainStep(*_args())
    model, opt, _, x, y = _args()
    with pytest.raises(_lib.TgcnError, match="no CPU fallback"):
        tgcn_amd.GraphedTrainStep(model, opt, _loss, (x, x), y, other_shapes="eager")
    with pytest.raises(_lib.TgcnError, match="example_inputs is a tensor or a non-empty tuple"):
        tgcn_amd.GraphedTrainStep(model, opt, _loss, (), y)


def test_hyper_parameters_compare_on_the_host():
    from tgcn_amd import graphed
    model = _Unreachable()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
    rec = graphed._hyper(opt)
    assert not graphed._hyper_changed(opt, rec)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.5)      # adds initial_lr: a key the step does not read
    assert not graphed._hyper_changed(opt, rec)
    opt.param_groups[0]["lr"] = 5e-4
    assert graphed._hyper_changed(opt, rec)
    opt.param_groups[0]["lr"] = 1e-3
    opt.param_groups[0]["betas"] = (0.8, 0.999)
    assert graphed._hyper_changed(opt, rec)
    del sched


def test_operand_cache_refuses_a_build_while_capturing(monkeypatch):
    """a cache miss during a capture raises before the build runs; a hit does not ask"""
    cache = tnn._OperandCache()
    built = []
    assert cache.get("a", lambda: built.append(1) or "op") == "op"
    monkeypatch.setattr(F, "stream_is_capturing", lambda: True)
    assert cache.get("a", lambda: built.append(2) or "other") == "op"
    with pytest.raises(_lib.TgcnError, match="built by a warm-up step on the same graph arguments"):
        cache.get("b", lambda: built.append(3) or "op")
    assert built == [1] and cache.peek("b") is None


def test_learnable_edge_weights_are_refused_while_capturing(monkeypatch):
    monkeypatch.setattr(F, "stream_is_capturing", lambda: True)
    w = torch.ones(3, requires_grad=True)
    with pytest.raises(_lib.TgcnError, match="learnable edge weights.*cannot run inside a hipGraph capture"):
        tnn._refresh_values(object(), w, lambda: w)
