"""The oracle pinned to given decisions (oracle/style_oracle.py, `decisions=` of OracleNet._forward / feval / _backward): ReLU masks and
max-pool arg-maxes taken from someone else, every other operation in the oracle's own arithmetic.  The GPU tests pin the fp64 oracle to the
engine's decisions (tests/engine_decisions.py) so that what remains between the two is arithmetic; these tests show, on the CPU, that the
pin changes nothing but the decisions."""
import pytest
import torch

import synth
from conftest import NIN_LAYERS, make_cfg, rel_l2
from engine_decisions import count_flips, oracle_decisions
from oracle import OracleNet, build_spec


def _net(cfg, dtype, S, seed=7):
    sd = synth.nin_state_dict() if cfg.model_file == "nin" else synth.vgg19_state_dict()
    content, style, init = synth.images(S, seed=seed)
    net = OracleNet(build_spec(cfg), sd, dtype)
    net.capture_content(content)
    net.capture_style([style], [1.0])
    return net, init


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model,pooling", [("vgg19", "max"), ("vgg19", "avg"), ("nin", "max"), ("nin", "avg")])
def test_pinned_to_its_own_decisions_is_the_unpinned_oracle(model, pooling, dtype):
    """Pinning the oracle to the decisions it takes itself reproduces its unpinned evaluation bit for bit: losses and gradient."""
    cfg = make_cfg(pooling=pooling, **(NIN_LAYERS if model == "nin" else {}))
    net, init = _net(cfg, dtype, 96 if model == "nin" else 40)
    acts, aux = net._forward(init.to(dtype))
    decisions = oracle_decisions(net.spec, acts, aux)
    assert sum(l.kind == "pool" for l in net.spec) > 0
    assert sum(net.spec[i].kind == "pool" for i in decisions) == (0 if pooling == "avg" else sum(l.kind == "pool" for l in net.spec))
    total, losses, g = net.feval(init)
    ptotal, plosses, pg = net.feval(init, decisions=decisions)
    assert torch.equal(torch.as_tensor(total), torch.as_tensor(ptotal))
    assert losses.keys() == plosses.keys() and all(torch.equal(torch.as_tensor(losses[k]), torch.as_tensor(plosses[k])) for k in losses)
    assert torch.equal(g, pg)
    pacts, paux = net._forward(init.to(dtype), decisions=decisions)
    assert all(torch.equal(a, b) for a, b in zip(acts, pacts))


# VGG-19 at 56 x 56, synth.images seed 10, default flags: fp32 takes one ReLU decision (relu3_4) differently from fp64, which moves the pixel
# gradient by 1.3e-3 rel-L2; pinned to the fp32 decisions the two arithmetics agree to 1.4e-6 (found by a seed search over 32 ... 64 px)
FLIP_S, FLIP_SEED = 56, 10


def test_pinning_removes_the_decision_error_and_nothing_else():
    """Where the fp32 and fp64 oracles take a decision differently, their gradients are a thousand times further apart than their arithmetic
    is; pinned both to the same (fp32) decisions they agree as closely as fp32 arithmetic allows."""
    cfg = make_cfg()
    n64, init = _net(cfg, torch.float64, FLIP_S, FLIP_SEED)
    n32, _ = _net(cfg, torch.float32, FLIP_S, FLIP_SEED)
    a64, x64 = n64._forward(init.double())
    a32, x32 = n32._forward(init.float())
    d32 = oracle_decisions(n32.spec, a32, x32)
    flips = count_flips(n64.spec, d32, a64, x64)
    assert sum(flips.values()) > 0, flips
    _, l64, g64 = n64.feval(init)
    _, l32, g32 = n32.feval(init)
    assert rel_l2(g32, g64) > 1e-4
    _, pl64, pg64 = n64.feval(init, decisions=d32)
    _, pl32, pg32 = n32.feval(init, decisions=d32)
    assert rel_l2(pg32, pg64) <= 1e-5, rel_l2(pg32, pg64)
    assert torch.equal(pg32, g32)    # (fp32 pinned to its own decisions: unchanged)
    for k in pl64:
        assert abs(float(pl32[k]) - float(pl64[k])) <= 1e-5 * abs(float(pl64[k])), k


def test_a_pinned_relu_passes_negative_values_and_masks_the_gradient_by_its_mask():
    """A pinned mask that is set over a negative input passes the negative value (forward) and the gradient (backward); a mask that is
    clear over a positive input passes neither - the pin, not the sign, decides."""
    cfg = make_cfg()
    net, init = _net(cfg, torch.float64, 32)
    acts, aux = net._forward(init.double())
    decisions = oracle_decisions(net.spec, acts, aux)
    r = next(i for i, l in enumerate(net.spec) if l.kind == "relu")
    pre = net._forward(init.double())[0][r - 1]
    neg = (pre < 0).nonzero()[0].tolist()
    pos = (pre > 0).nonzero()[0].tolist()
    decisions[r] = decisions[r].clone()
    decisions[r][tuple(neg)] = True
    decisions[r][tuple(pos)] = False
    pacts, _ = net._forward(init.double(), decisions=decisions)
    assert float(pacts[r][tuple(neg)]) == float(pre[tuple(neg)]) < 0
    assert float(pacts[r][tuple(pos)]) == 0.0
    g_out = torch.zeros_like(acts[r])
    g_out[tuple(neg)], g_out[tuple(pos)] = 1.0, 1.0
    masked = net._backward(init.double(), pacts[:r + 1], [None] * (r + 1), {r: g_out}, decisions=decisions)
    net.spec, spec = net.spec[:r + 1], net.spec
    try:
        want = torch.nn.grad.conv2d_input(init.shape, net.w[0], (g_out * decisions[r]).double(), padding=1)
    finally:
        net.spec = spec
    assert torch.equal(masked, want)


def test_a_pinned_max_pool_gathers_and_scatters_at_the_given_indices():
    """A pinned max pool outputs its input at the given indices, not the window's maximum, and routes the gradient back to them."""
    cfg = make_cfg(style_layers="relu2_1", content_layers="relu2_1")
    net, init = _net(cfg, torch.float64, 32)
    acts, aux = net._forward(init.double())
    decisions = oracle_decisions(net.spec, acts, aux)
    p = next(i for i, l in enumerate(net.spec) if l.kind == "pool")
    idx = decisions[p].clone()
    idx[0, 0, 0, 0] = idx[0, 0, 0, 0] ^ 1     # the other column of the first window
    decisions[p] = idx
    pacts, paux = net._forward(init.double(), decisions=decisions)
    src = acts[p - 1].reshape(*acts[p - 1].shape[:2], -1)
    assert torch.equal(pacts[p], src.gather(2, idx.reshape(*idx.shape[:2], -1)).reshape(idx.shape))
    assert paux[p] is idx
    _, _, g = net.feval(init, decisions=decisions)
    _, _, g0 = net.feval(init)
    assert rel_l2(g, g0) > 0


def test_bad_decisions_raise():
    """Decisions of the wrong shape or dtype, missing for a relu or a max pool, given where there is nothing to decide, or for a window of
    frames, are errors - not silently the oracle's own."""
    cfg = make_cfg()
    net, init = _net(cfg, torch.float64, 32)
    acts, aux = net._forward(init.double())
    good = oracle_decisions(net.spec, acts, aux)
    r = next(i for i, l in enumerate(net.spec) if l.kind == "relu")
    p = next(i for i, l in enumerate(net.spec) if l.kind == "pool")
    for k in (r, p):
        bad = dict(good)
        del bad[k]
        with pytest.raises(ValueError):
            net.feval(init, decisions=bad)
    bad = {**good, r: good[r][:, :, :-1]}
    with pytest.raises(ValueError):
        net.feval(init, decisions=bad)
    bad = {**good, p: good[p][:, :, :, :-1]}
    with pytest.raises(ValueError):
        net.feval(init, decisions=bad)
    bad = {**good, r: good[r].double()}
    with pytest.raises(ValueError):
        net.feval(init, decisions=bad)
    bad = {**good, 0: good[r]}    # (spec entry 0 is the TV module)
    with pytest.raises(ValueError):
        net.feval(init, decisions=bad)
    with pytest.raises(NotImplementedError):
        net.feval(torch.cat([init, init]), decisions=good)
    avg, _ = _net(make_cfg(pooling="avg"), torch.float64, 32)
    with pytest.raises(ValueError):
        avg.feval(init, decisions=good)
