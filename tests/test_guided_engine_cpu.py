"""Host side of the guided style layers on the fused engine (planner field guided_engine): the per-region coefficients against fp64 autograd
over a literal restatement of loss.StyleLoss.guided_loss, and the field's default.  No GPU."""
import itertools

import pytest
import torch


class ScaleGradients(torch.autograd.Function):
    """loss.ScaleGradients, restated: identity forwards, g -> g / (|g| + 1e-8) * strength^2 backwards."""

    @staticmethod
    def forward(ctx, input_tensor, strength):
        ctx.strength = strength
        return input_tensor

    @staticmethod
    def backward(ctx, grad_output):
        unit = grad_output / (torch.norm(grad_output, keepdim=True) + 1e-8)
        return unit * ctx.strength * ctx.strength, None


def guided_loss64(grams, targets, strength, vsf, normalize, active, has):
    """guided_loss's loop: t_r = mean((G_r - T_r)^2) enters once with the strength and, for vsf > 0, once more with vsf x strength."""
    acc = (lambda t: ScaleGradients.apply(t, strength)) if normalize else (lambda t: t)
    loss = 0
    for r in range(grams.shape[0]):
        if not (active[r] and has[r]):
            continue
        t = ((grams[r] - targets[r]) ** 2).mean()
        loss = loss + acc(t) * strength
        if vsf > 0:
            loss = loss + vsf * acc(t) * strength
    return loss


@pytest.mark.parametrize("normalize,vsf", list(itertools.product([False, True], [0.0, 100.0])))
def test_coefficients_reproduce_guided_loss(normalize, vsf):
    import engine
    R, C, strength = 3, 7, 0.37
    active, has = [True, False, True], [True, True, False]  # region 1 inactive, region 2 without a target: only region 0 counts
    for active, has in ((active, has), ([True] * R, [True] * R)):
        gen = torch.Generator().manual_seed(5)
        sym = lambda: (lambda m: m + m.transpose(1, 2))(torch.randn(R, C, C, generator=gen, dtype=torch.float64))
        grams, targets = sym().requires_grad_(True), sym()
        loss = guided_loss64(grams, targets, strength, vsf, normalize, active, has)
        ls, gs = engine.guided_coefficients(strength, vsf, normalize, C, active, has)
        assert len(ls) == len(gs) == R
        diff = (grams - targets).detach()
        want_loss = sum(ls[r] * float((diff[r] ** 2).sum()) for r in range(R))
        assert abs(float(loss.detach()) - want_loss) <= 1e-12 * abs(want_loss)
        (dg,) = torch.autograd.grad(loss, grams)
        for r in range(R):
            d = dg[r] + dg[r].t()
            want = gs[r] * diff[r]
            if not (active[r] and has[r]):
                assert ls[r] == 0.0 and gs[r] == 0.0 and not bool(d.any())
                continue
            assert float((d - want).norm()) <= 1e-12 * float(want.norm()), (r, normalize, vsf)


def test_planner_field_defaults_to_the_module_path():
    import optim
    import plan

    assert plan.FIELDS["guided_engine"][0] == "0" and plan.FIELDS["guided_engine"][1] == "host"
    assert not plan.on("guided_engine")

    class Style:
        guide = object()

    class Net:
        style_losses = [Style()]

    net = Net()
    assert optim._engine_of(net) is None
    assert not hasattr(net, "_maua_engine") and not getattr(net, "_maua_engine_refused", False)  # (not remembered)
