"""Guided (per-region) style loss without a GPU: the fp64 restatement (tests/guided_restatement.py) against the oracle's unguided
evaluation and against its own analytic gradient, mask parsing (load.py), the preset keys (config.get_args), the refusals of the clip
drivers and the binding table."""
import argparse
import json
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import guided_restatement as gr
import synth
from conftest import REPO, make_cfg, rel_l2


@pytest.mark.parametrize("over", [dict(), dict(use_covariance=True), dict(normalize_gradients=False, video_style_factor=0.0),
                                  dict(normalize_weights=True, temporal_weight=0.0)], ids=["default", "covariance", "plain", "normalize_weights"])
def test_one_region_of_ones_is_the_unguided_evaluation(over):
    """R = 1, g = 1: G = Gram / nelement, one term per layer - the oracle's closed-form evaluation, loss for loss, to 1e-12."""
    from oracle.style_oracle import OracleNet, build_spec
    cfg = make_cfg(style_layers="relu1_1,relu2_1,relu3_1", content_layers="relu2_2", **over)
    sd = synth.vgg19_state_dict(dtype=torch.float64)
    content, style, init = (t.double() for t in synth.images(24))
    onet = OracleNet(build_spec(cfg), sd, torch.float64)
    onet.capture_content(content)
    onet.capture_style([style], cfg.style_blend_weights)
    if cfg.normalize_weights:
        onet.normalize_weights()
    total_o, losses_o, grad_o = onet.feval(init)
    ones = (torch.ones(1, 24, 24), [torch.ones(1, 24, 24)])
    for guides in (ones, None):
        net = gr.build(content, [style], cfg, sd, guides)
        total, losses, grad = net.feval(init, None if guides is None else guides[0])
        assert sorted(losses) == sorted(losses_o)
        for i in losses:
            assert abs(float(losses[i]) - float(losses_o[i])) <= 1e-12 * abs(float(losses_o[i])), (i, float(losses[i]), float(losses_o[i]))
        assert abs(float(total) - float(total_o)) <= 1e-12 * abs(float(total_o))
        assert rel_l2(grad, grad_o) <= 1e-12


@pytest.mark.parametrize("cov", [False, True])
def test_analytic_gradient_equals_autograd(cov):
    """dL/dF = sum_r (2 / (C N_r)) g_r^2 D_r (F - mu_r) for symmetric D_r = dL/dG_r: the term through mu_r vanishes."""
    g = torch.Generator().manual_seed(5)
    C, N, R = 7, 45, 3
    f = torch.randn(C, N, generator=g, dtype=torch.float64).requires_grad_(True)
    guides = torch.rand(R, N, generator=g, dtype=torch.float64)
    guides[2, 10:] = 0  # mass < 1 with these values -> inactive
    guides[2, :10] *= 0.1
    target = torch.randn(R, C, C, generator=g, dtype=torch.float64)
    target = target + target.transpose(1, 2)
    G, mass, active = gr.guided_grams(f, guides, cov)
    assert active == [True, True, False] and float(G[2].detach().abs().max()) == 0.0
    loss = sum(((G[r] - target[r]) ** 2).mean() * (r + 1.5) for r in range(R) if active[r])
    loss.backward()
    with torch.no_grad():
        d = torch.stack([2.0 * (r + 1.5) * (G[r] - target[r]) / (C * C) for r in range(R)])
        assert torch.equal(d, d.transpose(1, 2)) or rel_l2(d, d.transpose(1, 2)) <= 1e-15
        want = gr.guided_grad(f.detach(), guides, d, cov)
    assert rel_l2(f.grad, want) <= 1e-12


def test_targets_leave_out_the_styles_in_which_a_region_is_absent():
    """T_r = sum_i b_i G_r(style_i) / sum of b_i over the styles where r is active; a region active nowhere has no target and no term."""
    cfg = make_cfg(style_layers="relu1_1", content_layers="relu1_2", style_blend_weights=[0.25, 0.75])
    sd = synth.vgg19_state_dict(dtype=torch.float64)
    content, s1, s2, init = (t.double() for t in synth.images(16, n=4))
    g1 = torch.zeros(3, 16, 16)
    g1[0, :, :8], g1[1, :, 8:] = 1, 1                # style 1: regions 0 and 1
    g2 = torch.zeros(3, 16, 16)
    g2[0] = 1                                        # style 2: region 0 only
    cg = torch.zeros(3, 16, 16)
    cg[0, :5], cg[1, 5:10], cg[2, 10:] = 1, 1, 1
    net = gr.build(content, [s1, s2], cfg, sd, (cg, [g1, g2]))
    (i,) = [k for k, l in enumerate(net.spec) if l.kind == "style"]
    assert net.style_has[i] == [True, True, False] and net.skipped == [(i, 2)]
    only1 = gr.build(content, [s1], make_cfg(style_layers="relu1_1", content_layers="relu1_2"), sd, (cg, [g1]))
    assert rel_l2(net.style_targets[i][1], only1.style_targets[i][1]) <= 1e-14      # region 1: style 1 alone, weight 0.25 / 0.25
    total, losses, grad = net.feval(init, cg)
    assert torch.isfinite(grad).all() and float(losses[i]) > 0


# -- masks ----------------------------------------------------------------------------------------------------------------------------
def _mask(h, w, colours, layout):
    m = np.zeros((h, w, 3), np.uint8)
    for k, sl in layout:
        m[sl] = colours[k]
    return m


def test_mask_colours_sorted_define_the_regions(tmp_path):
    import load
    colours = [(255, 0, 0), (0, 0, 255), (0, 128, 0)]
    m = _mask(6, 8, colours, [(0, np.s_[:, :]), (1, np.s_[:3, 4:]), (2, np.s_[4:, :2])])
    p = tmp_path / "m.png"
    Image.fromarray(m).save(p)
    read = load.read_mask(str(p))
    assert np.array_equal(read, m)
    order = load.mask_colours(read)
    assert order == [(0, 0, 255), (0, 128, 0), (255, 0, 0)]  # sorted (r, g, b)
    g = load.mask_guides(read, order, (6, 8))
    assert g.shape == (3, 6, 8) and g.dtype == torch.float32
    assert torch.equal(g.sum(0), torch.ones(6, 8))
    assert torch.equal(g[0], torch.from_numpy((m == (0, 0, 255)).all(-1)).float())
    assert g[2, 0, 0] == 1 and g[1, 5, 0] == 1 and g[0, 0, 7] == 1


def test_more_than_eight_colours_is_an_error():
    import load
    m = np.zeros((3, 3, 3), np.uint8)
    m[..., 0] = np.arange(9).reshape(3, 3)
    with pytest.raises(ValueError, match="9 distinct colours"):
        load.mask_colours(m)
    assert len(load.mask_colours(m[:2, :])) == 6


def test_foreign_colour_in_a_style_mask_is_named():
    import load
    content = _mask(4, 4, [(1, 2, 3), (9, 9, 9)], [(0, np.s_[:, :]), (1, np.s_[:2])])
    order = load.mask_colours(content)
    style = content.copy()
    style[3, 3] = (7, 200, 31)
    with pytest.raises(ValueError, match=r"style_masks\[1\].*\(7, 200, 31\)"):
        load.mask_guides(style, order, (4, 4), "style_masks[1]")
    # a style mask may use FEWER colours: the missing region's guide is empty
    g = load.mask_guides(np.full((5, 5, 3), 9, np.uint8), order, (5, 5))
    assert float(g[0].sum()) == 0 and float(g[1].sum()) == 25


def test_masks_are_resized_with_nearest_neighbour():
    import load
    colours = [(0, 0, 0), (255, 255, 255)]
    m = _mask(4, 6, colours, [(0, np.s_[:, :]), (1, np.s_[:, 3:])])
    g = load.mask_guides(m, colours, (8, 3))
    assert torch.equal(g[1], torch.tensor([[0., 0., 1.]] * 8))  # source columns floor(i * 6 / 3) = 0, 2, 4
    big = load.mask_guides(m, colours, (5, 12))
    assert torch.equal(big[1, 0], torch.tensor([0.] * 6 + [1.] * 6))
    assert set(big.unique().tolist()) == {0.0, 1.0}  # one-hot: no blending


# -- preset keys and drivers ----------------------------------------------------------------------------------------------------------
def _preset_args(tmp_path, extra):
    import config
    preset = tmp_path / "preset.json"
    preset.write_text(json.dumps(dict(extra)))
    return config.get_args(["--content", "c.png", "--style", "s.png", "--load_args", str(preset)])


def test_preset_keys_arrive_on_args(tmp_path):
    args = _preset_args(tmp_path, dict(content_mask="cm.png", style_masks=["sm.png"], style_weight=33.0))
    assert args.content_mask == "cm.png" and args.style_masks == ["sm.png"] and args.style_weight == 33.0
    import style
    assert style._mask_keys(args) == ("cm.png", ["sm.png"])
    assert style._mask_keys(_preset_args(tmp_path, dict(style_weight=1.0))) is None
    with pytest.raises(ValueError, match="both preset keys"):
        style._mask_keys(argparse.Namespace(content_mask="cm.png"))


@pytest.mark.parametrize("driver", ["vid_img", "img_vid"])
def test_clip_drivers_refuse_masks(tmp_path, driver):
    import style
    args = _preset_args(tmp_path, dict(content_mask="cm.png", style_masks=["sm.png"]))
    args.transfer_type = driver
    with pytest.raises(NotImplementedError, match="img_img only"):
        getattr(style, driver)(args)


def test_optimize_refuses_guides_for_clips_and_batches():
    import optim
    guides = (torch.ones(1, 8, 8), [torch.ones(1, 8, 8)])
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(NotImplementedError, match="guides"):
        optim.optimize(x[:1], [x[:1]], x, 1, argparse.Namespace(transfer_type="img_img"), guides=guides)
    with pytest.raises(NotImplementedError, match="guides"):
        optim.optimize(x[:1], [x[:1]], x[:1], 1, argparse.Namespace(transfer_type="img_vid"), guides=guides)


def test_style_loss_guide_attribute():
    import loss
    m = loss.StyleLoss(1.0)
    assert m.guide is None and m.guided_target is None
    with pytest.raises(ValueError, match="1 <= R <= 8"):
        m.guide = torch.ones(9, 4, 4)
    with pytest.raises(ValueError):
        m.guide = torch.ones(4, 4)


def test_engine_refuses_a_guided_style_module():
    import engine
    import loss

    class Fake(loss.StyleLoss):
        guide = property(lambda self: object(), lambda self, v: None)

    m = Fake(1.0)
    with pytest.raises(engine.UnsupportedNet, match="guided StyleLoss runs on the module path"):
        engine.StyleEngine(torch.nn.Sequential(m), [m])


def test_signatures_cover_the_guided_entry_points():
    import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "maua_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(maua_[a-z0-9_]+)\s*\(", header)))
    assert sorted(hip.SIGNATURES) == declared
    guided = [n for n in declared if n.startswith("maua_gram_guided_")]
    assert guided == ["maua_gram_guided_bwd", "maua_gram_guided_fwd", "maua_gram_guided_mass", "maua_gram_guided_supported",
                      "maua_gram_guided_workspace_bytes"]
    for name in guided:  # argument counts of the binding = parameter counts of the declaration
        params = re.search(name + r"\s*\(([^()]*)\)\s*;", header).group(1).split(",")
        assert len(hip.SIGNATURES[name][1]) == len(params), name
    assert all(callable(getattr(hip, n)) for n in ("gram_guided_fwd", "gram_guided_bwd", "gram_guided_mass"))
