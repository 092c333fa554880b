"""The plan field of the device-resident temporal path, and the host loop's independence of it (no GPU needed)."""
import json
import os

import numpy as np
import torch

from conftest import REPO, write_video_fixture


def test_plan_field_exists_and_defaults_to_off(monkeypatch):
    import plan
    monkeypatch.delenv("MAUA_PLAN", raising=False)
    assert plan.FIELDS["temporal_device"][0] == "0" and plan.FIELDS["temporal_device"][1] == "host"
    assert not plan.on("temporal_device")
    monkeypatch.setenv("MAUA_PLAN", "temporal_device=1")
    assert plan.on("temporal_device") and plan.in_effect() == {"temporal_device": "1"}
    assert not any("TEMPORAL" in v for v in plan.ENV_VARS)  # set through MAUA_PLAN only


def test_host_loop_does_not_touch_the_device_path(tmp_path, monkeypatch):
    """With the field at 0 style._vid_img_flow runs the host statements: every new wrapper, loader and the device branch itself raise
    when touched.  The optimisation and the network are stand-ins (the loop around them is what is under test)."""
    import config
    import hip
    import load
    import models
    import optim
    import plan
    import style

    def forbidden(*a, **k):
        raise AssertionError("the host loop touched the device-resident temporal path")
    for mod, names in ((hip, ("flow_warp_grid", "grid_sample_border", "mask_u8_resize")),
                       (load, ("flow_warp_grid_device", "reliable_flow_weighting_device")), (style, ("_vid_img_flow_device",))):
        for attr in names:
            assert hasattr(mod, attr)
            monkeypatch.setattr(mod, attr, forbidden)
    monkeypatch.delenv("MAUA_PLAN", raising=False)
    monkeypatch.setitem(plan.OVERRIDES, "temporal_device", "0")

    calls, targets = [], []
    monkeypatch.setattr(models, "load_model", lambda args: (object(), []))
    monkeypatch.setattr(optim, "optimize", lambda content, styles, init, n, a, net=None, losses=None, **k:
                        (calls.append((os.path.basename(a.output), init.clone())), init.clone())[1])
    monkeypatch.setattr(optim, "set_temporal_targets", lambda net, warp, warp_weights=None, args=None: targets.append(warp_weights.shape))

    fdir, outdir = write_video_fixture(str(tmp_path), n_frames=3, S=16)
    scaling = tmp_path / "scaling.json"
    scaling.write_text(json.dumps({"100000": {"gpu": "0", "multidevice": False}}))
    args = config.get_args(["--transfer_type", "vid_img", "--content", fdir, "--style", os.path.join(REPO, "tests", "synth_style_256.png"),
                            "--image_sizes", "16", "--num_iters", "8", "--passes_per_scale", "2", "--init", "prev_warp",
                            "--model_file", "vgg19_none.pth", "--disable_check", "--scaling_args", str(scaling), "--seed", "0",
                            "--no_hist_match", "--output_dir", outdir])
    frames = load.process_content_frames(fdir)
    job = outdir + "/clip_synth_style_256"
    style._vid_img_flow(args, job, frames, load.process_style_images(args), np.array(load.preprocess(frames[0]).size()[-2:]))
    want = ["1_0001.png", "1_0002.png", "1_0000.png", "2_0001.png", "2_0000.png", "2_0002.png"]
    assert [c[0] for c in calls] == want
    assert sorted(os.listdir(os.path.join(job, "16"))) == sorted(want)
    assert targets == [torch.Size([1, 1, 16, 16])] * 3
    assert all(not c[1].is_cuda and torch.isfinite(c[1]).all() for c in calls)
