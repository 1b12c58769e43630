"""CLI of the layer-wise adaptive optimizers: --optimizer lars / lamb, --trust-coefficient, --adapt-1d."""
import copy

import pytest
import torch

from distributed_pytorch_training_amd.config import parse_args
from distributed_pytorch_training_amd.optim import FusedAdam, FusedLAMB, FusedLARS, FusedSGD, build_optimizer
from distributed_pytorch_training_amd.parallel.flat import FlatArena


def test_new_flags_and_their_defaults():
    a = parse_args([])
    assert a.optimizer == "sgd" and a.trust_coefficient == 0.001 and a.adapt_1d is False
    assert a.betas == (0.9, 0.999) and a.eps == 1e-8 and a.nesterov is False      # existing defaults unchanged
    for name in ("lars", "lamb"):
        assert parse_args(["--optimizer", name]).optimizer == name
    b = parse_args(["--optimizer", "lars", "--trust-coefficient", "0.02", "--adapt-1d"])
    assert b.trust_coefficient == 0.02 and b.adapt_1d is True
    with pytest.raises(SystemExit):
        parse_args(["--optimizer", "lion"])


def _model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(6, 8), torch.nn.Linear(8, 3))


def _one_step(name, argv):
    args = parse_args(["--optimizer", name] + argv)
    m = _model()
    arena = FlatArena(list(m.parameters()))
    opt = build_optimizer(args.optimizer, arena, args)
    torch.manual_seed(1)
    m(torch.randn(4, 6)).square().mean().backward()
    opt.step()
    return opt, arena.param_flat.clone()


@pytest.mark.parametrize("name,cls", [("sgd", FusedSGD), ("adamw", FusedAdam)])
def test_trust_flags_are_ignored_by_sgd_and_adamw(name, cls):
    plain, p0 = _one_step(name, [])
    flagged, p1 = _one_step(name, ["--trust-coefficient", "0.5", "--adapt-1d"])
    assert type(plain) is cls and type(flagged) is cls
    assert torch.equal(p0, p1)
    assert "trust_coefficient" not in flagged.group and not hasattr(flagged, "adapt_1d")


def test_flags_reach_lars_and_lamb():
    lars, _ = _one_step("lars", ["--trust-coefficient", "0.5", "--adapt-1d", "--nesterov"])
    assert type(lars) is FusedLARS and lars.group["trust_coefficient"] == 0.5 and lars.adapt_1d
    assert lars.group["nesterov"] is True
    assert all(r != 1.0 for r in lars.trust_ratios.tolist())
    lamb, _ = _one_step("lamb", ["--betas", "0.8,0.9", "--eps", "1e-6"])
    assert type(lamb) is FusedLAMB and lamb.group["betas"] == (0.8, 0.9) and lamb.group["eps"] == 1e-6
    assert not lamb.adapt_1d
    ones = [r == 1.0 for r, p in zip(lamb.trust_ratios.tolist(), lamb.arena.params) if p.ndim <= 1]
    assert ones and all(ones)
