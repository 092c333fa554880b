"""Neural cellular automaton on the MI355X (csrc/nca.hip, nca.py) against the fp64 restatement (tests/nca_restatement.py) and an
fp64 torch-CPU autograd statement of one training step of the reference."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nca_restatement as R
from conftest import REPO

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _params(chn, hidden, seed, w2_scale=0.1, w1_scale=0.2):
    rng = np.random.default_rng(seed)
    k = 4 * chn
    return np.concatenate([rng.normal(0, w1_scale, hidden * k), rng.normal(0, 0.1, hidden),
                           rng.normal(0, w2_scale, chn * hidden)]).astype(np.float32)


def _relu_flips(x, params, chn, hidden):
    """Pixels whose pre-activations lie within fp32 rounding of zero (a ReLU decision fp32 may take differently from fp64)."""
    w1, b1, _ = R.split(params, chn, hidden)
    a = np.einsum("jk,bkhw->bjhw", w1, R.perceive(x)) + b1[None, :, None, None]
    scale = np.einsum("jk,bkhw->bjhw", np.abs(w1), np.abs(R.perceive(x))) + np.abs(b1)[None, :, None, None]
    return (np.abs(a) <= 1e-5 * scale).any(axis=1)


def _rel(a, b):
    return float(np.linalg.norm((np.asarray(a, np.float64) - b).ravel()) / max(np.linalg.norm(np.asarray(b).ravel()), 1e-30))


@pytest.mark.parametrize("chn,hidden", [(12, 96), (16, 128)])
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (4, 3, 5), (1, 128, 128), (4, 127, 200)])
@pytest.mark.parametrize("mode", ["given", "generated", "rate_map"])
def test_step_against_fp64(chn, hidden, n, h, w, mode):
    import hip
    rng = np.random.default_rng(n * 1000 + h + w)
    params = _params(chn, hidden, 1)
    x = rng.normal(0, 0.5, (n, chn, h, w)).astype(np.float32)
    seed, step = 11, 3
    rmap = None
    if mode == "given":
        m = (rng.random((n, 1, h, w)) < 0.5).astype(np.float32)
    elif mode == "generated":
        m = R.mask(seed, step, n, h, w)
    else:
        rmap = rng.random((h, w)).astype(np.float32)
        m = R.mask(seed, step, n, h, w, rate_map=rmap)
    xt, pt = torch.from_numpy(x).to(DEV), torch.from_numpy(params).to(DEV)
    out = hip.nca_step(xt, pt, chn, hidden, mask=torch.from_numpy(m).to(DEV) if mode == "given" else None, seed=seed, step=step,
                       rate_map=None if rmap is None else torch.from_numpy(rmap).to(DEV))
    got = out.cpu().numpy()
    want = R.step(x.astype(np.float64), params, chn, hidden, m)
    assert _rel(got, want) <= 1e-6, _rel(got, want)
    bad = np.abs(got - want) > 1e-5 * (1 + np.abs(want))
    if bad.any():
        flips = _relu_flips(x.astype(np.float64), params, chn, hidden)
        assert not (bad.any(axis=1) & ~flips).any(), "misses not explained by a ReLU decision"


def test_uint8_mask_equals_fp32_mask():
    import hip
    rng = np.random.default_rng(9)
    x = torch.from_numpy(rng.normal(0, 0.5, (2, 12, 9, 11)).astype(np.float32)).to(DEV)
    pt = torch.from_numpy(_params(12, 96, 3)).to(DEV)
    m = torch.from_numpy((rng.random((2, 1, 9, 11)) < 0.5).astype(np.uint8)).to(DEV)
    a = hip.nca_step(x, pt, 12, 96, mask=m)
    b = hip.nca_step(x, pt, 12, 96, mask=m.float())
    assert torch.equal(a, b)


def test_generated_mask_is_the_restated_function_bit_for_bit():
    """W2 = I-like readout of the hidden unit that equals 1: out - x = mask exactly."""
    import hip
    chn, hidden, n, h, w = 12, 96, 3, 67, 130
    k = 4 * chn
    w1, b1, w2 = np.zeros((hidden, k), np.float32), np.zeros(hidden, np.float32), np.zeros((chn, hidden), np.float32)
    b1[0], w2[:, 0] = 1.0, 1.0
    params = torch.from_numpy(np.concatenate([w1.ravel(), b1, w2.ravel()])).to(DEV)
    x = torch.zeros(n, chn, h, w, device=DEV)
    for seed, step, rate in ((0, 0, 0.5), (2 ** 64 - 1, 123456, 0.5), (5, 7, 0.1)):
        got = hip.nca_step(x, params, chn, hidden, rate=rate, seed=seed, step=step)[:, 0].cpu().numpy()
        np.testing.assert_array_equal(got, R.mask(seed, step, n, h, w, rate=rate))


def test_step_4096_squared_on_sampled_tiles():
    import hip
    chn, hidden, s = 12, 96, 4096
    assert hip.nca_supported(1, chn, hidden, s, s)
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(1, chn, s, s, device=DEV, generator=g) * 0.5
    params = _params(chn, hidden, 2)
    out = hip.nca_step(x, torch.from_numpy(params).to(DEV), chn, hidden, seed=9, step=1)
    mask = R.mask(9, 1, 1, s, s)
    for y0, x0 in ((0, 0), (s - 16, s - 16), (2048, 1000), (0, s - 16), (s - 16, 0)):
        ys, xs = (np.arange(y0 - 1, y0 + 17) % s), (np.arange(x0 - 1, x0 + 17) % s)
        patch = x[:, :, torch.as_tensor(ys, device=DEV)][:, :, :, torch.as_tensor(xs, device=DEV)].cpu().double().numpy()
        p = R.perceive(patch)[:, :, 1:-1, 1:-1]
        w1, b1, w2 = R.split(params, chn, hidden)
        a = np.einsum("jk,bkhw->bjhw", w1, p) + b1[None, :, None, None]
        m = mask[:, y0:y0 + 16, x0:x0 + 16]
        want = patch[:, :, 1:-1, 1:-1] + np.einsum("cj,bjhw->bchw", w2, np.maximum(a, 0)) * m[:, None]
        got = out[:, :, y0:y0 + 16, x0:x0 + 16].cpu().numpy()
        assert _rel(got, want) <= 1e-6


def _run_chain(chn, hidden, n, h, w, steps, seed=5, masks=None, params=None):
    import hip
    rng = np.random.default_rng(3)
    params = _params(chn, hidden, 4, w2_scale=0.01, w1_scale=0.03) if params is None else params  # a chain that stays O(10)
    x0 = rng.normal(0, 0.5, (n, chn, h, w)).astype(np.float32)
    gl = rng.normal(size=x0.shape).astype(np.float32)
    pt = torch.from_numpy(params).to(DEV)
    xs = [torch.from_numpy(x0).to(DEV)]
    for k in range(steps):
        xs.append(hip.nca_step(xs[-1], pt, chn, hidden, seed=seed, step=k))
    ws = hip.nca_bwd_workspace(n, chn, hidden, h, w, DEV)
    g = torch.from_numpy(gl).to(DEV)
    for k in reversed(range(steps)):
        g = hip.nca_step_bwd(xs[k], g, pt, chn, hidden, ws, first=(k == steps - 1), seed=seed, step=k, dx=g)
    grad = hip.nca_grad_finish(xs[0].shape, chn, hidden, ws)
    masks = [R.mask(seed, k, n, h, w) for k in range(steps)]
    return params, x0, gl, masks, g.cpu().numpy(), grad.cpu().numpy()


@pytest.mark.parametrize("chn,hidden,n,h,w,steps", [(12, 96, 2, 19, 23, 1), (12, 96, 4, 32, 32, 32), (16, 128, 1, 40, 24, 1),
                                                    (16, 128, 2, 24, 24, 32)])
def test_backward_against_fp64(chn, hidden, n, h, w, steps):
    params, x0, gl, masks, dx0, grad = _run_chain(chn, hidden, n, h, w, steps)
    want_dx, want_dp = R.chain_bwd(x0.astype(np.float64), gl.astype(np.float64), params, chn, hidden, masks)
    assert _rel(dx0, want_dx) <= 1e-5, _rel(dx0, want_dx)
    hk = hidden * 4 * chn
    for sl, name in ((slice(0, hk), "dW1"), (slice(hk, hk + hidden), "db1"), (slice(hk + hidden, None), "dW2")):
        assert _rel(grad[sl], want_dp[sl]) <= 1e-4, (name, _rel(grad[sl], want_dp[sl]))


def test_backward_is_bit_reproducible():
    a = _run_chain(12, 96, 4, 64, 48, 8)
    b = _run_chain(12, 96, 4, 64, 48, 8)
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])


def test_gradient_normalisation():
    import hip
    params, x0, gl, masks, dx0, grad = _run_chain(12, 96, 1, 16, 16, 2)
    # rerun the same chain and finish with normalize = 1 from the same slots
    pt = torch.from_numpy(params).to(DEV)
    xs = [torch.from_numpy(x0).to(DEV)]
    for k in range(2):
        xs.append(hip.nca_step(xs[-1], pt, 12, 96, seed=5, step=k))
    ws = hip.nca_bwd_workspace(1, 12, 96, 16, 16, DEV)
    g = torch.from_numpy(gl).to(DEV)
    for k in reversed(range(2)):
        g = hip.nca_step_bwd(xs[k], g, pt, 12, 96, ws, first=(k == 1), seed=5, step=k, dx=g)
    gn = hip.nca_grad_finish(xs[0].shape, 12, 96, ws, normalize=True).cpu().numpy()
    hk = 96 * 48
    for sl in (slice(0, hk), slice(hk, hk + 96), slice(hk + 96, None)):
        want = grad[sl].astype(np.float64) / (np.linalg.norm(grad[sl].astype(np.float64)) + 1e-8)
        np.testing.assert_allclose(gn[sl], want, rtol=1e-5, atol=1e-7)


# ---- one training step against fp64 torch autograd -------------------------------------------------------------------------------
def _vgg16_file(tmp_path, seed=0):
    import models
    seq = models.build_sequential(models.channel_list["VGG-16"], "max")
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in models.VGG(seq).state_dict().items():
        if k.endswith("weight"):
            fan_in = v.shape[1] * 9
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / fan_in) ** 0.5
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.01
    f = str(tmp_path / "vgg16-397923af.pth")
    torch.save(sd, f)
    return f, sd


def _fp64_reference_step(params, chn, hidden, x0, masks, sd, target):
    """The reference's training step (NCA_train.py:221-230) in fp64 torch on the CPU, masks injected."""
    k = 4 * chn
    p = torch.tensor(params, dtype=torch.float64, requires_grad=True)
    w1 = p[:hidden * k].view(hidden, k, 1, 1)
    b1 = p[hidden * k:hidden * k + hidden]
    w2 = p[hidden * k + hidden:].view(chn, hidden, 1, 1)
    filt = torch.from_numpy(R.FILTERS)[:, None]
    x = torch.from_numpy(x0).double()
    for m in masks:
        b, c, h, w = x.shape
        y = F.conv2d(F.pad(x.reshape(b * c, 1, h, w), [1, 1, 1, 1], "circular"), filt).reshape(b, 4 * c, h, w)
        y = F.conv2d(torch.relu(F.conv2d(y, w1, b1)), w2)
        x = x + y * torch.from_numpy(m).double().reshape(b, 1, h, w)
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float64)[:, None, None]
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float64)[:, None, None]
    f = (x[:, :3] - mean) / std
    loss, conv = 0.0, 0
    layers = []
    import models
    for c in models.channel_list["VGG-16"]:
        layers += ["P"] if c == "P" else ["C", "R"]
    for i, kind in enumerate(layers[:26]):
        if kind == "C":
            f = F.conv2d(f, sd[f"features.{i}.weight"].double(), sd[f"features.{i}.bias"].double(), padding=1)
        elif kind == "R":
            f = torch.relu(f)
        else:
            f = F.max_pool2d(f, 2, 2)
        if i in (1, 6, 11, 18, 25):
            hw = f.shape[-2] * f.shape[-1]
            g = torch.einsum("bchw,bdhw->bcd", f, f) / hw
            loss = loss + (g.mean(0) - target[conv].double()).square().mean()
            conv += 1
    loss.backward()
    gr = p.grad.clone()
    for sl in (slice(0, hidden * k), slice(hidden * k, hidden * k + hidden), slice(hidden * k + hidden, None)):
        gr[sl] = gr[sl] / (gr[sl].norm() + 1e-8)
    return float(loss.detach()), gr.numpy()


def test_one_training_step_against_fp64_autograd(tmp_path):
    import nca
    chn, hidden, n, s, steps = 12, 96, 2, 48, 8
    vgg, sd = _vgg16_file(tmp_path)
    style = nca.StyleModel(vgg, DEV)
    target = nca.target_grams(style, os.path.join(REPO, "tests", "synth_style_256.png"))
    params = _params(chn, hidden, 6, w2_scale=0.02, w1_scale=0.05)
    ca = nca.NCA(torch.from_numpy(params).to(DEV), chn, hidden)
    tr = nca.Trainer(ca, style, target, batch=n, pool=4, size=s, seed=0)
    rng = np.random.default_rng(7)
    x0 = rng.random((n, chn, s, s)).astype(np.float32)
    masks = [(rng.random((n, 1, s, s)) < 0.5).astype(np.float32) for _ in range(steps)]
    loss, _, grad = tr.loss_and_grad(torch.from_numpy(x0).to(DEV), steps, masks=[torch.from_numpy(m).to(DEV) for m in masks])
    want_loss, want_grad = _fp64_reference_step(params, chn, hidden, x0, masks, sd, [t.cpu() for t in target])
    assert abs(float(loss) - want_loss) <= 1e-4 * abs(want_loss), (float(loss), want_loss)
    got = grad.cpu().numpy()
    hk = hidden * 4 * chn
    for sl in (slice(0, hk), slice(hk, hk + hidden), slice(hk + hidden, None)):
        assert _rel(got[sl], want_grad[sl]) <= 2e-3, _rel(got[sl], want_grad[sl])


def test_an_update_goes_downhill(tmp_path):
    """One Adam update on the normalised BPTT gradient lowers the loss of the same batch, masks and step count."""
    import nca
    vgg, _ = _vgg16_file(tmp_path)
    style = nca.StyleModel(vgg, DEV)
    target = nca.target_grams(style, os.path.join(REPO, "tests", "synth_style_256.png"))
    import hip
    ca = nca.NCA(torch.from_numpy(_params(12, 96, 8, w2_scale=0.02, w1_scale=0.05)).to(DEV), 12, 96)
    tr = nca.Trainer(ca, style, target, batch=2, pool=4, size=48, seed=0)
    x0 = torch.rand(2, 12, 48, 48, device=DEV) * 0.5
    l0, _, grad = tr.loss_and_grad(x0, 16, ca_step0=0)
    hip.adam_step(ca.params, grad, tr.m, tr.v, 1, 1e-4)
    l1, _, _ = tr.loss_and_grad(x0, 16, ca_step0=0)
    assert float(l1) < float(l0), (float(l0), float(l1))


def test_training_run_and_render(tmp_path):
    import nca
    vgg, _ = _vgg16_file(tmp_path)
    out = str(tmp_path / "out")
    style = os.path.join(REPO, "tests", "synth_style_256.png")
    args = nca.parse_args(["train", style, out, "--vgg_file", vgg, "--steps", "60", "--size", "64", "--checkpoint_every", "10"])
    _, log = nca.train(args)
    assert len(log) == 60 and np.all(np.isfinite(log))
    # single batches spike (a pool state that has run away), the bulk goes down: the median of the last 20 below the first loss
    assert np.median(log[-20:]) < log[0], log
    for i in range(10, 61, 10):
        assert os.path.exists(os.path.join(out, f"synth_style_256_{i}.pt")) and os.path.exists(os.path.join(out, f"synth_style_256_{i}.png"))
    from PIL import Image
    assert Image.open(os.path.join(out, "synth_style_256_60.png")).size == (4 * 64, 64)
    rate = str(tmp_path / "text.png")
    Image.fromarray(np.uint8(np.pad(np.full((20, 40), 255), 12))).save(rate)
    ck = os.path.join(out, "synth_style_256_60.pt")
    r = nca.parse_args(["render", style, out, "--checkpoint", ck, "--frames", "5", "--size", "48", "--rate_map", rate, "--checkgrid"])
    dirs = nca.render(r)
    assert [os.path.basename(d) for d in dirs] == ["synth_style_256_60", "synth_style_256_checkgrid", "synth_style_256-60-wav"]
    for d in dirs:
        assert len(glob.glob(os.path.join(d, "frame_*.png"))) == 5
    assert Image.open(os.path.join(dirs[0], "frame_00000.png")).size == (96, 96)
    assert Image.open(os.path.join(dirs[1], "frame_00000.png")).size == (2 * (128 * 2 + 2), 2 * 512)  # checkpoints [2:-2] of 6
    first = [np.asarray(Image.open(f)) for f in sorted(glob.glob(os.path.join(dirs[0], "*.png")))]
    nca.render(nca.parse_args(["render", style, out, "--checkpoint", ck, "--frames", "5", "--size", "48"]))
    again = [np.asarray(Image.open(f)) for f in sorted(glob.glob(os.path.join(dirs[0], "*.png")))]
    assert all(np.array_equal(a, b) for a, b in zip(first, again))


class CA(torch.nn.Module):
    """Shaped like the reference's CA (NCA_train.py:165-173), whose whole-module pickles are the reference's checkpoints."""

    def __init__(self):
        super().__init__()
        self.chn = 12
        self.w1 = torch.nn.Conv2d(48, 96, 1)
        self.w2 = torch.nn.Conv2d(96, 12, 1, bias=False)


def test_render_reads_a_reference_pickle(tmp_path):
    import nca
    ca = CA()
    f = str(tmp_path / "style_7500.pt")
    torch.save(ca, f)
    r = nca.parse_args(["render", "x/style.png", str(tmp_path), "--frames", "2", "--size", "32"])
    dirs = nca.render(r)
    assert len(glob.glob(os.path.join(dirs[0], "frame_*.png"))) == 2
