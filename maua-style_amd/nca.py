"""Neural cellular automaton textures on the MI355X: the reference's NCA_train.py (training) and NCA_gen.py (rendering).

    python nca.py train STYLE OUT_DIR [--vgg_file F] [--steps 7500] [--seed S] [--batch 4] [--pool 1024]
    python nca.py render STYLE OUT_DIR [--checkpoint F] [--frames 600] [--size 256] [--rate_map IMG] [--checkgrid]

Every CA step is one launch of csrc/nca.hip (maua_nca_step); training backpropagates through the whole chain with
maua_nca_step_bwd and maua_nca_grad_finish, then steps Adam with maua_adam_step over one flat parameter buffer.  The style
loss runs VGG-16 on the module path (models.Conv2d / ReLU / MaxPool2d, loss._GramFn): HIP kernels forward and backward.
Videos are directories of PNG frames named like the reference's .mp4 files.  DESIGN.md, "Neural cellular automaton".
"""
import argparse
import glob
import os
import pickle
import sys

import numpy as np
import torch
from PIL import Image, ImageFilter

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import hip  # noqa: E402
from utils import name  # noqa: E402

STYLE_LAYERS = [1, 6, 11, 18, 25]  # relu1_1, relu2_1, relu3_1, relu4_1, relu5_1 of VGG-16 `features` (NCA_train.py:125)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
DEFAULT_VGG = "modelzoo/vgg16-397923af.pth"  # torchvision's file name; its `features.*` keys are the ones loaded here
LR, LR_MILESTONES, LR_GAMMA = 1e-3, (2000, 4000), 0.3
SEED_EVERY, STEP_N_RANGE, CHECKPOINT_EVERY = 32, (32, 96), 500
STEPS_PER_ITER = 96  # mask counter stride per training iteration (step_n < 96)


# ---- schedules (NCA_train.py:197-253, NCA_gen.py) -------------------------------------------------------------------------------
def lr_at(i):
    """Adam's learning rate for the i-th update (0-based): MultiStepLR([2000, 4000], 0.3) stepped after every update."""
    return LR * LR_GAMMA ** sum(1 for m in LR_MILESTONES if i >= m)


def evolution_steps(k):
    """CA steps before frame k of the evolution video (NCA_gen.py:17)."""
    return min(2 ** (k // 30), 32)


def rate_map_steps(k):
    """CA steps before frame k of the rate-map video (NCA_gen.py:55)."""
    return min(int(2 ** (k / 30)), 32)


def fade(k):
    """Brightness factor of frame k of the rate-map video (NCA_gen.py:58)."""
    return min(1.0 - (k - 400) / 100, 1.0)


# ---- the model ------------------------------------------------------------------------------------------------------------------
class NCA:
    """Parameters of the reference's CA(chn, hidden_n) as one flat fp32 device buffer [w1 (hidden, 4 chn)][b1][w2 (chn, hidden)]."""

    def __init__(self, params, chn=12, hidden=96):
        self.chn, self.hidden = int(chn), int(hidden)
        n = hip.nca_param_count(self.chn, self.hidden)
        if n == 0 or params.numel() != n:
            raise ValueError(f"NCA: chn/hidden {chn}/{hidden} with {params.numel()} parameters is not a built configuration")
        self.params = params.contiguous()

    @classmethod
    def init(cls, chn=12, hidden=96, seed=0, device="cuda"):
        """torch.nn.Conv2d's default initialisation of w1 (weight and bias uniform in +-1/sqrt(4 chn)), w2 zero (NCA_train.py:168-173)."""
        g = torch.Generator().manual_seed(int(seed))
        bound = 1.0 / (4 * chn) ** 0.5
        w1 = (torch.rand(hidden, 4 * chn, generator=g) * 2 - 1) * bound
        b1 = (torch.rand(hidden, generator=g) * 2 - 1) * bound
        w2 = torch.zeros(chn, hidden)
        return cls(torch.cat([w1.flatten(), b1, w2.flatten()]).to(device), chn, hidden)

    def tensors(self):
        c, h = self.chn, self.hidden
        k = 4 * c
        p = self.params
        return p[:h * k].view(h, k), p[h * k:h * k + h], p[h * k + h:].view(c, h)

    def state_dict(self):
        w1, b1, w2 = (t.detach().cpu().clone() for t in self.tensors())
        return {"w1.weight": w1[:, :, None, None], "w1.bias": b1, "w2.weight": w2[:, :, None, None], "chn": self.chn,
                "hidden": self.hidden}

    @classmethod
    def from_state_dict(cls, sd, device="cuda"):
        w1, b1, w2 = sd["w1.weight"], sd["w1.bias"], sd["w2.weight"]
        hidden, k = w1.shape[:2]
        chn = int(sd.get("chn", k // 4))
        flat = torch.cat([w1.reshape(-1), b1.reshape(-1), w2.reshape(-1)]).float()
        return cls(flat.to(device), chn, int(sd.get("hidden", hidden)))

    def seed(self, n, size=128, device="cuda"):
        return torch.zeros(n, self.chn, size, size, device=device)

    def step(self, x, rate=0.5, rate_map=None, mask=None, seed=0, step=0, out=None):
        return hip.nca_step(x, self.params, self.chn, self.hidden, rate, rate_map, mask, seed, step, out)


# ---- checkpoints ----------------------------------------------------------------------------------------------------------------
class _Stub:
    """Stands in for a pickled torch.nn.Module: BUILD fills __dict__ with its _parameters / _modules / attributes."""

    def __setstate__(self, state):
        self.__dict__.update(state)


class _CAStub(_Stub):
    pass


_TORCH_ALLOWED = {
    ("torch._utils", "_rebuild_tensor_v2"), ("torch._utils", "_rebuild_tensor"), ("torch._utils", "_rebuild_parameter"),
    ("torch._utils", "_rebuild_parameter_with_state"), ("torch.nn.parameter", "Parameter"), ("collections", "OrderedDict"),
    ("builtins", "set"), ("__builtin__", "set"), ("torch", "Size"),
}
_STORAGES = {"FloatStorage", "DoubleStorage", "HalfStorage", "BFloat16Storage", "LongStorage", "IntStorage", "ShortStorage",
             "CharStorage", "ByteStorage", "BoolStorage", "UntypedStorage"}
_MODULE_STUBS = {("torch.nn.modules.conv", "Conv2d")}


class _RestrictedUnpickler(pickle.Unpickler):
    """Reads the reference's whole-module checkpoints (`torch.save(ca, ...)`, NCA_train.py:247): the class `CA` of whatever module
    wrote it becomes a stub, torch's Conv2d a stub, and apart from those only torch's tensor / storage rebuilders are allowed."""

    def find_class(self, module, qualname):
        if qualname == "CA":
            return _CAStub
        if (module, qualname) in _MODULE_STUBS:
            return _Stub
        if (module, qualname) in _TORCH_ALLOWED or (module in ("torch", "torch.storage") and qualname in _STORAGES):
            return super().find_class(module, qualname)
        raise pickle.UnpicklingError(f"checkpoint refers to {module}.{qualname}, which an NCA checkpoint does not contain")


class _restricted_pickle:  # the `pickle_module` torch.load expects
    Unpickler = _RestrictedUnpickler
    load = staticmethod(lambda f, **kw: _RestrictedUnpickler(f, **kw).load())
    __name__ = "nca_restricted_pickle"


def save_checkpoint(ca, path):
    torch.save(ca.state_dict(), path)


def load_checkpoint(path, device="cuda"):
    """A checkpoint of this program (a plain state dict) or the reference's pickled CA module."""
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError:
        sd = None
    if not isinstance(sd, dict):
        obj = torch.load(path, map_location="cpu", weights_only=False, pickle_module=_restricted_pickle)
        if not isinstance(obj, _CAStub):
            raise ValueError(f"{path}: neither an NCA state dict nor a pickled CA module")
        mods = obj.__dict__["_modules"]
        w1, w2 = mods["w1"].__dict__["_parameters"], mods["w2"].__dict__["_parameters"]
        sd = {"w1.weight": w1["weight"].detach(), "w1.bias": w1["bias"].detach(), "w2.weight": w2["weight"].detach(),
              "chn": int(obj.__dict__.get("chn", w2["weight"].shape[0]))}
    return NCA.from_state_dict(sd, device)


# ---- images ---------------------------------------------------------------------------------------------------------------------
def imread_style(path, max_size=128):
    """NCA_train.py:44-52 with max_size 128: thumbnail (Lanczos, PIL's former ANTIALIAS), [0, 1], the first 3 channels.  Greyscale and
    palette images are converted to RGB first (the reference's `[:, :, :3]` fails on them)."""
    img = Image.open(path)
    img.thumbnail((max_size, max_size), Image.LANCZOS)
    if img.mode not in ("RGB", "RGBA"):
        img = img.convert("RGB")
    return np.float32(img)[:, :, :3] / 255.0


def to_rgb_u8(x):
    """(..., >=3, h, w) state -> (h, w, 3) uint8 of the first image: clip to [0, 1], * 255, truncate (NCA_train.py:57-60)."""
    a = x[..., :3, :, :].detach().float().cpu().numpy()
    if a.ndim == 4:
        a = np.concatenate(list(a), axis=2)  # images side by side (np.hstack of the (h, w, 3) images)
    return np.uint8(np.clip(a.transpose(1, 2, 0), 0, 1) * 255)


def zoom(img, scale=2):
    return np.repeat(np.repeat(img, scale, 0), scale, 1)


def load_rate_map(path):
    """NCA_gen.py:45-50 for a user image: greyscale, GaussianBlur(5), p / p.max() * 0.6 + 0.05."""
    im = Image.open(path).convert("L").filter(ImageFilter.GaussianBlur(5))
    p = np.float32(im)
    return p / max(float(p.max()), 1e-12) * 0.6 + 0.05


# ---- the style model ------------------------------------------------------------------------------------------------------------
class StyleModel:
    """VGG-16 `features` up to relu5_1 on the module path, and the batch-mean Gram loss (NCA_train.py:123-143, 235-236)."""

    def __init__(self, vgg_file=DEFAULT_VGG, device="cuda"):
        import models
        if not os.path.exists(vgg_file):
            raise FileNotFoundError(f"model weights not found at {vgg_file}: this build has no network access and never downloads; "
                                    "pass --vgg_file <path to torchvision's vgg16-397923af.pth or another VGG-16 state dict>")
        cnn = models.VGG(models.build_sequential(models.channel_list["VGG-16"], "max"))
        models._load_features(cnn, vgg_file, strict=True)
        self.features = cnn.features[:max(STYLE_LAYERS) + 1].to(device).requires_grad_(False)
        self.mean = torch.tensor(IMAGENET_MEAN, device=device)[:, None, None]
        self.std = torch.tensor(IMAGENET_STD, device=device)[:, None, None]

    def grams(self, imgs):
        """(B, 3, h, w) in [0, 1] -> one (B, C, C) tensor per style layer: einsum(bchw, bdhw -> bcd) / (h w)."""
        from loss import _GramFn
        x = (imgs - self.mean) / self.std
        out = []
        for i, layer in enumerate(self.features):
            x = layer(x)
            if i in STYLE_LAYERS:
                hw = x.shape[-2] * x.shape[-1]
                out.append(torch.stack([_GramFn.apply(x[b:b + 1], False) for b in range(x.shape[0])]) / hw)
        return out

    @staticmethod
    def loss(grams, targets):
        """sum over layers of mean((G.mean(0) - T)^2)."""
        total = 0.0
        for g, t in zip(grams, targets):
            total = total + (g.mean(0) - t).square().mean()
        return total


# ---- training -------------------------------------------------------------------------------------------------------------------
class Trainer:
    def __init__(self, ca, style, target, batch=4, pool=1024, size=128, seed=0):
        self.ca, self.style, self.target = ca, style, target
        dev = ca.params.device
        self.pool = ca.seed(pool, size, dev)
        self.batch, self.size = batch, size
        self.rng = np.random.RandomState(seed)
        self.mask_seed = int(seed)
        self.m = torch.zeros_like(ca.params)
        self.v = torch.zeros_like(ca.params)
        self.i = 0
        self.ws = hip.nca_bwd_workspace(batch, ca.chn, ca.hidden, size, size, dev)
        self.grad = torch.empty_like(ca.params)

    def draw(self):
        """(batch pool indices, step_n) of the next iteration, NCA_train.py:215-223."""
        idx = self.rng.choice(len(self.pool), self.batch, replace=False)
        step_n = self.rng.randint(*STEP_N_RANGE)
        return idx, step_n

    def loss_and_grad(self, x0, step_n, masks=None, ca_step0=0):
        """Forward chain of step_n steps from x0, the style loss of its RGB, and the parameter gradient by BPTT (normalised per
        tensor).  masks: optional list of explicit (B, 1, h, w) masks, one per step.  Returns (loss, x_last, grad)."""
        ca = self.ca
        xs = [x0.contiguous()]
        for k in range(step_n):
            xs.append(ca.step(xs[-1], mask=None if masks is None else masks[k], seed=self.mask_seed, step=ca_step0 + k))
        rgb = xs[-1][:, :3].contiguous().requires_grad_(True)
        loss = self.style.loss(self.style.grams(rgb), self.target)
        (g_rgb,) = torch.autograd.grad(loss, rgb)
        g = torch.zeros_like(xs[-1])
        g[:, :3] = g_rgb
        for k in reversed(range(step_n)):
            hip.nca_step_bwd(xs[k], g, ca.params, ca.chn, ca.hidden, self.ws, first=(k == step_n - 1),
                             mask=None if masks is None else masks[k], seed=self.mask_seed, step=ca_step0 + k, dx=g)
        hip.nca_grad_finish(x0.shape, ca.chn, ca.hidden, self.ws, normalize=True, out=self.grad)
        return loss.detach(), xs[-1], self.grad

    def train_step(self):
        idx, step_n = self.draw()
        it = torch.as_tensor(idx, device=self.pool.device)
        x = self.pool[it]
        if self.i % SEED_EVERY == 0:
            x[:1] = 0.0
        loss, x, grad = self.loss_and_grad(x, step_n, ca_step0=self.i * STEPS_PER_ITER)
        hip.adam_step(self.ca.params, grad, self.m, self.v, self.i + 1, lr_at(self.i))
        self.pool[it] = x
        self.i += 1
        return loss, x


def target_grams(style, style_file, device="cuda"):
    img = torch.from_numpy(imread_style(style_file)).permute(2, 0, 1)[None].contiguous().to(device)
    with torch.no_grad():
        return [g[0] for g in style.grams(img)]


def train(args):
    dev = "cuda"
    os.makedirs(args.out_dir, exist_ok=True)
    style = StyleModel(args.vgg_file, dev)
    target = target_grams(style, args.style, dev)
    ca = NCA.init(args.chn, args.hidden, args.seed, dev)
    tr = Trainer(ca, style, target, args.batch, args.pool, args.size, args.seed)
    stem, log = name(args.style), []
    for i in range(args.steps):
        loss, x = tr.train_step()
        log.append(float(loss))
        if i % 10 == 0 or i + 1 == args.steps:
            print(f"step {i + 1:5d}  loss {log[-1]:.4f}  lr {lr_at(i):.2e}", flush=True)
        if (i + 1) % args.checkpoint_every == 0:
            save_checkpoint(ca, os.path.join(args.out_dir, f"{stem}_{i + 1}.pt"))
            Image.fromarray(to_rgb_u8(x)).save(os.path.join(args.out_dir, f"{stem}_{i + 1}.png"))
    return ca, log


# ---- rendering (NCA_gen.py) -----------------------------------------------------------------------------------------------------
def _save_frame(d, k, img):
    Image.fromarray(np.ascontiguousarray(img)).save(os.path.join(d, f"frame_{k:05d}.png"))


def render_evolution(ca, out, frames, size, seed=0):
    """(a): a zero size^2 seed, frame k after evolution_steps(k) more steps, zoomed 2x."""
    os.makedirs(out, exist_ok=True)
    x, y = ca.seed(1, size, ca.params.device), None
    s = 0
    for k in range(frames):
        for _ in range(evolution_steps(k)):
            y = ca.step(x, seed=seed, step=s, out=y)
            x, y, s = y, x, s + 1
        _save_frame(out, k, zoom(to_rgb_u8(x[0])))


def render_checkgrid(models_, out, frames, rows=512, strip=128, seed=0):
    """(b): the checkpoints side by side as `strip`-wide strips of one rand * 0.1 state; each model steps its own strip + 2 column
    window (wrapping within it) and writes back the interior, 8 rounds per frame, models in order."""
    os.makedirs(out, exist_ok=True)
    chn = models_[0].chn
    dev = models_[0].params.device
    g = torch.Generator().manual_seed(int(seed))
    x = (torch.rand(1, chn, rows, strip * len(models_) + 2, generator=g) * 0.1).to(dev)
    s = 0
    for k in range(frames):
        for _ in range(8):
            for ci, m in enumerate(models_):
                sub = x[:, :, :, ci * strip:ci * strip + strip + 2].contiguous()
                y = m.step(sub, seed=seed, step=s)
                x[:, :, :, ci * strip + 1:ci * strip + strip + 1] = y[:, :, :, 1:-1]
                s += 1
        _save_frame(out, k, zoom(to_rgb_u8(x[0])))


def render_rate_map(ca, out, frames, rate_map, seed=0):
    """(c): a zero state the size of the rate map, the map as per-pixel update rate, frames faded out after 400."""
    os.makedirs(out, exist_ok=True)
    dev = ca.params.device
    p = torch.as_tensor(rate_map, dtype=torch.float32, device=dev).contiguous()
    h, w = p.shape
    x, y, s = torch.zeros(1, ca.chn, h, w, device=dev), None, 0
    for k in range(frames):
        for _ in range(rate_map_steps(k)):
            y = ca.step(x, rate_map=p, seed=seed, step=s, out=y)
            x, y, s = y, x, s + 1
        img = x[0, :3].float().cpu().numpy().transpose(1, 2, 0) * fade(k)
        _save_frame(out, k, zoom(np.uint8(np.clip(img, 0, 1) * 255)))


def render(args):
    stem = name(args.style)
    ckpt = args.checkpoint or os.path.join(args.out_dir, f"{stem}_7500.pt")
    ca = load_checkpoint(ckpt)
    tag = name(ckpt).split("_")[-1]
    written = []
    d = os.path.join(args.out_dir, f"{stem}_{tag}")
    render_evolution(ca, d, args.frames, args.size, args.seed)
    written.append(d)
    if args.checkgrid:
        files = sorted(glob.glob(os.path.join(args.out_dir, f"{stem}*.pt")))[2:-2]
        if not files:
            raise SystemExit(f"--checkgrid: fewer than 5 checkpoints {stem}*.pt in {args.out_dir}")
        d = os.path.join(args.out_dir, f"{stem}_checkgrid")
        render_checkgrid([load_checkpoint(f) for f in files], d, args.frames, seed=args.seed)
        written.append(d)
    if args.rate_map:
        d = os.path.join(args.out_dir, f"{stem}-{tag}-wav")
        render_rate_map(ca, d, args.frames, load_rate_map(args.rate_map), args.seed)
        written.append(d)
    for d in written:
        print(f"wrote {d}/ ({args.frames} frames)")
    return written


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="nca.py", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("train", help="train a CA on a style image (NCA_train.py)")
    t.add_argument("style")
    t.add_argument("out_dir")
    t.add_argument("--vgg_file", default=DEFAULT_VGG)
    t.add_argument("--steps", type=int, default=7500)
    t.add_argument("--seed", type=int, default=0)
    t.add_argument("--batch", type=int, default=4)
    t.add_argument("--pool", type=int, default=1024)
    t.add_argument("--size", type=int, default=128, help="side of the pool's states")
    t.add_argument("--checkpoint_every", type=int, default=CHECKPOINT_EVERY)
    t.add_argument("--chn", type=int, default=12)
    t.add_argument("--hidden", type=int, default=96)
    r = sub.add_parser("render", help="render videos as PNG frame directories (NCA_gen.py)")
    r.add_argument("style")
    r.add_argument("out_dir")
    r.add_argument("--checkpoint", default=None, help="default OUT_DIR/<style name>_7500.pt")
    r.add_argument("--frames", type=int, default=600)
    r.add_argument("--size", type=int, default=256)
    r.add_argument("--rate_map", default=None, help="image whose blurred grey levels become the per-pixel update rate")
    r.add_argument("--checkgrid", action="store_true")
    r.add_argument("--seed", type=int, default=0)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.cmd == "train":
        train(args)
    else:
        render(args)


if __name__ == "__main__":
    main()
