"""The plan field of the device-resident img_vid path, the host half of the maua_gauss_wrap entry points and the clip's roll rule (no GPU)."""
import math

import pytest
import torch


def test_plan_field_exists_and_defaults_to_off(monkeypatch):
    import plan
    monkeypatch.delenv("MAUA_PLAN", raising=False)
    assert plan.FIELDS["clip_device"][0] == "0" and plan.FIELDS["clip_device"][1] == "host"
    assert not plan.on("clip_device")
    monkeypatch.setenv("MAUA_PLAN", "clip_device=1")
    assert plan.on("clip_device") and plan.in_effect() == {"clip_device": "1"}
    assert not any("CLIP" in v for v in plan.ENV_VARS)  # set through MAUA_PLAN only


@pytest.fixture(scope="module")
def L():
    import build_native
    import hip
    build_native.build()
    return hip.lib()


def test_supported_and_workspace_bytes_on_the_host(L):
    import hip
    assert "maua_gauss_wrap" in hip.SIGNATURES and callable(hip.gauss_wrap)
    assert L.maua_gauss_wrap_supported(48, 3, 2048, 2048, 48.0, 64.0, 64.0) == 1
    tables = sum(-(-min(2 * int(4.0 * s + 0.5) + 1, ext) * 8 // 256) * 256 for s, ext in ((48.0, 48), (64.0, 2048), (64.0, 2048)))
    assert L.maua_gauss_wrap_workspace_bytes(48, 3, 2048, 2048, 48.0, 64.0, 64.0) == tables + 4 * 48 * 3 * 2048 * 2048
    assert L.maua_gauss_wrap_workspace_bytes(9, 3, 33, 65, 0.5, 0.0, 0.0) == 256          # one axis: its table, no second clip
    assert L.maua_gauss_wrap_supported(9, 3, 33, 65, 0.0, 0.0, 0.0) == 1
    assert L.maua_gauss_wrap_workspace_bytes(9, 3, 33, 65, 0.0, 0.0, 0.0) == 0            # no axis: a copy
    limit = 4096                                                                           # MAUA_GAUSS_WRAP_MAX_RADIUS (include/maua_hip.h)
    assert L.maua_gauss_wrap_supported(2, 3, 4, 4, limit / 4.0, 1.0, 1.0) == 1             # radius int(4 sigma + 0.5) = the limit
    bad = [(0, 3, 4, 4, 1.0, 1.0, 1.0), (2, 0, 4, 4, 1.0, 1.0, 1.0), (2, 3, 0, 4, 1.0, 1.0, 1.0), (2, 3, 4, -1, 1.0, 1.0, 1.0),
           (2, 3, 4, 4, -0.5, 1.0, 1.0), (2, 3, 4, 4, 1.0, 1.0, -1e-3), (2, 3, 4, 4, math.nan, 1.0, 1.0), (2, 3, 4, 4, 1.0, math.inf, 1.0),
           (2, 3, 4, 4, 1.0, 1.0, (limit + 1) / 4.0), (2, 3, 4, 4, 1e300, 1.0, 1.0),
           (1 << 16, 3, 1 << 12, 1 << 12, 1.0, 1.0, 1.0), (2147483647, 2147483647, 2147483647, 2147483647, 1.0, 1.0, 1.0)]
    for args in bad:
        assert L.maua_gauss_wrap_supported(*args) == 0, args
        assert L.maua_gauss_wrap_workspace_bytes(*args) == 0, args


def test_header_states_the_radius_limit():
    import os
    import re
    from conftest import REPO
    text = open(os.path.join(REPO, "include", "maua_hip.h")).read()
    assert re.search(r"#define MAUA_GAUSS_WRAP_MAX_RADIUS 4096\b", text)


def test_refusals_touch_no_gpu(L):
    assert L.maua_gauss_wrap(None, None, 2, 3, 4, 4, 1.0, 1.0, 1.0, 0, None, 0, None) == -1
    assert b"null" in L.maua_last_error()
    x, y = 0x1000, 0x2000                                  # never dereferenced: every refusal comes before the first launch
    assert L.maua_gauss_wrap(x, x, 2, 3, 4, 4, 1.0, 1.0, 1.0, 0, None, 0, None) == -1 and b"same buffer" in L.maua_last_error()
    assert L.maua_gauss_wrap(x, y, 2, 3, 4, 4, -1.0, 1.0, 1.0, 0, None, 0, None) == -1 and b"unsupported" in L.maua_last_error()
    assert L.maua_gauss_wrap(x, y, 0, 3, 4, 4, 1.0, 1.0, 1.0, 0, None, 0, None) == -1 and b"unsupported" in L.maua_last_error()
    need = L.maua_gauss_wrap_workspace_bytes(2, 3, 4, 4, 1.0, 1.0, 1.0)
    assert need > 0
    assert L.maua_gauss_wrap(x, y, 2, 3, 4, 4, 1.0, 1.0, 1.0, 0, None, 0, None) == -1 and b"null" in L.maua_last_error()
    assert L.maua_gauss_wrap(x, y, 2, 3, 4, 4, 1.0, 1.0, 1.0, 0, 0x3000, need - 1, None) == -1 and b"too small" in L.maua_last_error()


def test_wrapper_refuses_cpu_tensors_and_wrong_ranks(L):
    import hip
    with pytest.raises(hip.HipError):
        hip.gauss_wrap(torch.zeros(2, 3, 4, 4), (1, 1, 1))
    with pytest.raises(hip.HipError):
        hip.gauss_wrap(torch.zeros(3, 4, 4), (1, 1, 1))


@pytest.mark.parametrize("T", (5, 7, 8, 9))
def test_roll_rule_is_the_reference_concatenation(T):
    """style.clip_roll: np.roll(p, -clip_roll(T), 0) (what hip.gauss_wrap's `roll` means) is the reference's th.cat((p[7:], p[:7]))."""
    import style
    p = torch.arange(T * 3 * 2 * 2, dtype=torch.float32).reshape(T, 3, 2, 2)
    r = style.clip_roll(T)
    assert r == (7 if T > 7 else 0)
    assert torch.equal(torch.roll(p, -r, 0), torch.cat((p[7:], p[:7])))
