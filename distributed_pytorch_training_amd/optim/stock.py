"""Per-tensor LARS and LAMB as ``torch.optim.Optimizer`` subclasses, for the stock engine
(``--impl torch``).

They state the same math as the fused arena kernels (csrc/kernels/trust_kernels.hip) in plain
torch, one parameter at a time: two norms and a handful of elementwise launches per tensor.  That
makes them the A/B baseline for the fused steps and the independent implementation the parity
tests compare against.  State keys follow torch.optim.SGD (``momentum_buffer``) and
torch.optim.Adam (``step``, ``exp_avg``, ``exp_avg_sq``).

Parameters with ``ndim <= 1`` (biases, BatchNorm / LayerNorm weights) get trust ratio 1 and no
weight decay unless ``adapt_1d``.
"""
from __future__ import annotations

import torch


def _adapted(p: torch.Tensor, group) -> bool:
    return bool(group["adapt_1d"]) or p.ndim > 1


def _ratio(adapt: bool, wn: torch.Tensor, xn: torch.Tensor, value: torch.Tensor) -> torch.Tensor:
    """``value`` where the parameter is adapted and both norms are positive, else 1 (no host sync)."""
    if not adapt:
        return torch.ones_like(wn)
    return torch.where((wn > 0) & (xn > 0), value, torch.ones_like(wn))


class LARS(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 0.1, momentum: float = 0.9, weight_decay: float = 0.0,
                 nesterov: bool = False, trust_coefficient: float = 0.001, adapt_1d: bool = False) -> None:
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov,
                                      trust_coefficient=trust_coefficient, adapt_1d=adapt_1d))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            mu, eta = group["momentum"], group["trust_coefficient"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                adapt = _adapted(p, group)
                wd = group["weight_decay"] if adapt else 0.0
                wn, gn = p.norm(), g.norm()
                r = _ratio(adapt, wn, gn, eta * wn / (gn + wd * wn))
                d = (g.add(p, alpha=wd) if wd != 0 else g) * r
                st = self.state[p]
                if "momentum_buffer" not in st:
                    buf = st["momentum_buffer"] = d.clone()
                else:
                    buf = st["momentum_buffer"].mul_(mu).add_(d)
                p.add_(d.add(buf, alpha=mu) if group["nesterov"] else buf, alpha=-group["lr"])
        return loss


class LAMB(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, adapt_1d: bool = False) -> None:
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                      adapt_1d=adapt_1d))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                st = self.state[p]
                if not st:
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                m, v = st["exp_avg"], st["exp_avg_sq"]
                m.lerp_(g, 1 - b1)
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                # from the device step count (no host sync), in double: 1 - 0.999f in fp32 is 1.3 % off
                t = st["step"].double()
                bc1, bc2 = (1 - b1 ** t).float(), (1 - b2 ** t).float()
                adapt = _adapted(p, group)
                wd = group["weight_decay"] if adapt else 0.0
                u = (m / bc1) / ((v / bc2).sqrt_().add_(group["eps"]))
                if wd != 0:
                    u.add_(p, alpha=wd)
                wn, un = p.norm(), u.norm()
                r = _ratio(adapt, wn, un, wn / un)
                p.sub_(u * (group["lr"] * r))
        return loss
