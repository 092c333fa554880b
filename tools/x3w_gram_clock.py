"""Where the Gram-carrying backward launches of conv_x3w spend their cycles: K loop / Gram phase / epilogue per wave, from the in-kernel
shader-clock stamps of the diagnostic build (-DXW_STAMP, tools/build_stamp_libs.sh), for the three launches of a 1024 x 1024 iteration and
both settings of `gram_mask_reuse`.
    python tools/x3w_gram_clock.py [SIDE]          (MAUA_HIP_LIB: another stamped build)"""
import ctypes
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "maua-style_amd")]
os.environ.setdefault("MAUA_HIP_LIB", os.path.join(REPO, "tools", "_build", "libmaua_stamp.so"))
import hip  # noqa: E402
import plan  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
L = hip.lib()
L.maua_xw_set_stamp_buffer.argtypes = [ctypes.c_void_p]
L.maua_xw_set_stamp_buffer.restype = None
g = torch.Generator(device="cuda").manual_seed(3)
for name, c, H, unpool in (("conv1_2 bwd + unpool + Gram(relu1_1)", 64, S, True), ("conv2_2 bwd + unpool + Gram(relu2_1)", 128, S // 2, True),
                           ("conv3_2 bwd + Gram(relu3_1)", 256, S // 4, False)):
    w = torch.randn(c, c, 3, 3, device="cuda", generator=g) * (2.0 / (9 * c)) ** 0.5
    f = torch.relu(torch.randn(1, c, H, H, device="cuda", generator=g))
    d = torch.randn(c, c, device="cuda", generator=g) * 1e-3
    d = (d + d.t()).contiguous()
    _, bb, wsc = hip.conv_pack_filters_x3w(w)
    dbank, dinv = hip.conv_x3w_dmat_bank(c, "cuda")
    hip.conv_pack_dmat_x3w(d, dbank, dinv)
    out = torch.empty(1, c, H, H, device="cuda")
    ws = torch.empty(4096, dtype=torch.uint8, device="cuda")  # (too small for slabs: one pass over the chunk list)
    if unpool:
        act = torch.relu(torch.randn(1, c, H, H, device="cuda", generator=g))
        gp = torch.randn(1, c, H // 2, H // 2, device="cuda", generator=g)
        codes = torch.empty(1, c, H // 2, H // 2, dtype=torch.uint8, device="cuda")
        hip.pool2x2_fwd_codes(act, torch.empty(1, c, H // 2, H // 2, device="cuda"), codes)
        fn = lambda: hip.conv3x3_x3w_unpool(gp, codes, True, bb, wsc, c, 1, out=out, out_relu_mask=f, dmat_bank=dbank, dmat_inv_scale=dinv, workspace=ws)
    else:
        gy = torch.randn(1, c, H, H, device="cuda", generator=g) * (torch.rand(1, c, H, H, device="cuda", generator=g) > 0.5)
        fn = lambda: hip.conv3x3_x3w_gram(gy, bb, wsc, f, dbank, dinv, c, 1, out=out, workspace=ws)
    tiles = ((H + 31) // 32) * ((H + 7) // 8)
    gx, ncot = ((tiles + 7) // 8) * 8, (c + 63) // 64
    for reuse in ("1", "0"):
        if L.maua_set_tuning(b"gram_mask_reuse", float(reuse)) != 0:  # (a build from before the constant: one pass)
            if reuse == "0":
                continue
        stamps = torch.zeros(ncot * gx * 4 * 64 * 8, dtype=torch.float32, device="cuda")
        for _ in range(20):  # warm: clocks settle under load
            fn()
        torch.cuda.synchronize()
        L.maua_xw_set_stamp_buffer(stamps.data_ptr())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        L.maua_xw_set_stamp_buffer(None)
        raw = (stamps.view(torch.int32).view(ncot * gx, 4, 64, 8).long() & 0xFFFFFFFF)[:, :, 63]
        raw = raw[raw[:, 0, 1] != 0]
        seg = lambda a, b: ((raw[..., b] - raw[..., a]) & 0xFFFFFFFF).float().mean().item()
        print(f"{name} C = {c} @{H} gram_mask_reuse = {reuse}: stamped launch {e0.elapsed_time(e1) * 1e3:6.1f} us | cycles per wave (mean): "
              f"K loop {seg(1, 5):8.0f}  Gram phase {seg(5, 3):7.0f}  epilogue {seg(3, 6):7.0f}  total {seg(1, 6):8.0f}", flush=True)
    L.maua_set_tuning(b"gram_mask_reuse", 1.0)
