"""A plain torch restatement of the detector (pmce_amd/yolo.py's network) for the tests: the module built from a spec with the
PyTorch-YOLOv3 lineage's names (module_list.{i}.conv_{i}, .batch_norm_{i}), the decoding of a scale, a numpy writer and reader of
darknet ``.weights`` files, and the drawing of weights that keep activations O(1) through 75 layers.  Structure: the published
yolov3.cfg; no tensor was recorded from the yolov3 or multi_person_tracker packages.  Runs on the CPU in fp32 and fp64."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

SEED = 20261019
MINI_WIDTHS, MINI_BLOCKS, MINI_CLASSES, MINI_SIDE = (8, 16, 24, 32, 48, 64), (1, 1, 2, 2, 1), 2, 64


def mini_spec():
    """The same layer kinds as yolov3 at S = 64 (grids 2 / 4 / 8), nc = 2: body convolutions with Cin = 24 and 12 (no multiple of 16),
    both concatenations (24 + 48 and 16 + 32), two residual stages of two blocks."""
    from pmce_amd import yolo as Y
    return Y.darknet53_spec(MINI_WIDTHS, MINI_BLOCKS, MINI_CLASSES, name="mini")


def channels(spec):
    out = []
    for i, l in enumerate(spec["layers"]):
        k = l["kind"]
        if k == "convolutional":
            out.append(l["filters"])
        elif k == "route":
            out.append(sum(out[j] for j in l["layers"]))
        else:
            out.append(out[-1])
    return out


class Darknet(nn.Module):
    def __init__(self, spec):
        super().__init__()
        self.spec = spec
        ch = channels(spec)
        self.module_list = nn.ModuleList()
        for i, l in enumerate(spec["layers"]):
            m = nn.Sequential()
            if l["kind"] == "convolutional":
                k = l["size"]
                m.add_module(f"conv_{i}", nn.Conv2d(ch[i - 1] if i else 3, l["filters"], k, l["stride"], (k - 1) // 2, bias=not l["bn"]))
                if l["bn"]:
                    m.add_module(f"batch_norm_{i}", nn.BatchNorm2d(l["filters"], eps=1e-5))
                if l["leaky"]:
                    m.add_module(f"leaky_{i}", nn.LeakyReLU(0.1))
            self.module_list.append(m)

    def forward(self, x):
        """images [n,3,S,S] -> (the raw detection maps NCHW, in the order of the yolo layers; rows [n, R, 5 + nc])."""
        S = x.shape[-1]
        outs, maps = [], []
        for i, l in enumerate(self.spec["layers"]):
            k = l["kind"]
            if k == "convolutional":
                x = self.module_list[i](x)
            elif k == "shortcut":
                x = outs[l["frm"]] + x            # the activation is inside the convolution's module: the add comes after it
            elif k == "route":
                x = torch.cat([outs[j] for j in l["layers"]], 1)
            elif k == "upsample":
                x = F.interpolate(x, scale_factor=2, mode="nearest")
            elif k == "yolo":
                maps.append(x)
            outs.append(x)
        anchors = [[self.spec["anchors"][a] for a in l["mask"]] for l in self.spec["layers"] if l["kind"] == "yolo"]
        rows = torch.cat([decode_scale(m, a, self.spec["num_classes"], S) for m, a in zip(maps, anchors)], 1)
        return maps, rows


def decode_scale(m, anchors, nc, S):
    """One raw map NCHW [n, 3 (5 + nc), g, g] -> [n, 3 g g, 5 + nc], rows ordered anchor, gy, gx; in the map's dtype."""
    n, _, g, _ = m.shape
    dt = m.dtype
    stride = torch.tensor(S / g, dtype=dt, device=m.device)
    p = m.view(n, 3, 5 + nc, g, g).permute(0, 1, 3, 4, 2)
    gx = torch.arange(g, dtype=dt, device=m.device).view(1, 1, 1, g)
    gy = torch.arange(g, dtype=dt, device=m.device).view(1, 1, g, 1)
    a = torch.tensor(anchors, dtype=dt, device=m.device) / stride
    x = (torch.sigmoid(p[..., 0]) + gx) * stride
    y = (torch.sigmoid(p[..., 1]) + gy) * stride
    w = (torch.exp(p[..., 2]) * a[:, 0].view(1, 3, 1, 1)) * stride
    h = (torch.exp(p[..., 3]) * a[:, 1].view(1, 3, 1, 1)) * stride
    out = torch.cat([torch.stack([x, y, w, h], -1), torch.sigmoid(p[..., 4:])], -1)
    return out.reshape(n, 3 * g * g, 5 + nc)


def draw_state_dict(spec, seed=SEED):
    """Weights that keep activations O(1): uniform with the variance 2 / (1.01 fan_in) that LeakyReLU(0.1) preserves; BatchNorm near the
    identity (gamma in [0.9, 1.1], statistics in [-0.1, 0.1] and [0.9, 1.1]) except before a shortcut, where gamma in [0.2, 0.4] keeps
    the 23 residual sums from doubling the variance each; detection convolutions at half the gain with biases in [-0.1, 0.1]."""
    g = torch.Generator().manual_seed(seed)
    ch = channels(spec)
    L = spec["layers"]
    sd = {}

    def uni(shape, lo, hi):
        return torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo

    for i, l in enumerate(L):
        if l["kind"] != "convolutional":
            continue
        cin, co, k = (ch[i - 1] if i else 3), l["filters"], l["size"]
        fan = cin * k * k
        if l["bn"]:
            b = float(np.sqrt(3.0 * 2.0 / (1.01 * fan)))
            before_shortcut = i + 1 < len(L) and L[i + 1]["kind"] == "shortcut"
            p = f"module_list.{i}.batch_norm_{i}."
            sd[p + "weight"] = uni((co,), 0.2, 0.4) if before_shortcut else uni((co,), 0.9, 1.1)
            sd[p + "bias"] = uni((co,), -0.1, 0.1)
            sd[p + "running_mean"] = uni((co,), -0.1, 0.1)
            sd[p + "running_var"] = uni((co,), 0.9, 1.1)
        else:
            b = 0.5 * float(np.sqrt(3.0 / fan))
            sd[f"module_list.{i}.conv_{i}.bias"] = uni((co,), -0.1, 0.1)
        sd[f"module_list.{i}.conv_{i}.weight"] = uni((co, cin, k, k), -b, b)
    return sd


def make_module(spec, sd, dtype=torch.float32):
    m = Darknet(spec)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return m.to(dtype).eval()


def draw_images(n, S, seed=SEED + 1):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, S, S, generator=g, dtype=torch.float32)


# ----------------------------------------------------------------------------------------------
# darknet .weights files in plain numpy (written here independently of pmce_amd.yolo's reader)
# ----------------------------------------------------------------------------------------------

def conv_layers(spec):
    ch = channels(spec)
    return [(i, l["filters"], ch[i - 1] if i else 3, l["size"], l["bn"]) for i, l in enumerate(spec["layers"]) if l["kind"] == "convolutional"]


def write_darknet(path, sd, spec, major=0, minor=2, revision=5, seen=32013312, extra_floats=0, drop_floats=0):
    parts = []
    for i, co, cin, k, bn in conv_layers(spec):
        if bn:
            p = f"module_list.{i}.batch_norm_{i}."
            parts += [sd[p + "bias"], sd[p + "weight"], sd[p + "running_mean"], sd[p + "running_var"]]
        else:
            parts.append(sd[f"module_list.{i}.conv_{i}.bias"])
        parts.append(sd[f"module_list.{i}.conv_{i}.weight"])
    data = np.concatenate([np.asarray(t, dtype="<f4").reshape(-1) for t in parts])
    if drop_floats:
        data = data[:-drop_floats]
    data = np.concatenate([data, np.zeros(extra_floats, "<f4")])
    with open(path, "wb") as f:
        f.write(np.asarray([major, minor, revision], "<i4").tobytes())
        f.write(np.asarray([seen], "<i8" if major * 10 + minor >= 2 else "<i4").tobytes())
        f.write(data.tobytes())
    return data.size


def read_darknet(path, spec):
    raw = open(path, "rb").read()
    major, minor, _ = np.frombuffer(raw[:12], "<i4")
    data = np.frombuffer(raw[20 if major * 10 + minor >= 2 else 16:], "<f4")
    sd, at = {}, 0
    for i, co, cin, k, bn in conv_layers(spec):
        names = [f"module_list.{i}.batch_norm_{i}." + s for s in ("bias", "weight", "running_mean", "running_var")] if bn \
            else [f"module_list.{i}.conv_{i}.bias"]
        for nm in names:
            sd[nm] = torch.from_numpy(data[at:at + co].copy())
            at += co
        sd[f"module_list.{i}.conv_{i}.weight"] = torch.from_numpy(data[at:at + co * cin * k * k].copy()).view(co, cin, k, k)
        at += co * cin * k * k
    assert at == data.size
    return sd


# ----------------------------------------------------------------------------------------------
# the input transform by torch's own operators
# ----------------------------------------------------------------------------------------------

def letterbox_torch(frame_u8, S, pad_value=0.0, swap_rb=False):
    """uint8 [H,W,3] -> fp32 [3,S,S]: ToTensor's division, F.pad to a square (d // 2 before), F.interpolate(mode="nearest")."""
    x = torch.as_tensor(frame_u8)
    if swap_rb:
        x = x.flip(-1)
    x = x.permute(2, 0, 1).float().div(255)
    H, W = x.shape[1:]
    d = abs(H - W)
    pad = (0, 0, d // 2, d - d // 2) if H <= W else (d // 2, d - d // 2, 0, 0)
    x = F.pad(x, pad, "constant", value=pad_value)
    return F.interpolate(x.unsqueeze(0), size=S, mode="nearest").squeeze(0)
