"""The ENet image encoder on the device (csrc/enet.hip): colour frames to the ``(F, 128, H/8, W/8)``
feature maps that the reference makes with ``scripts/compute_multiview_features.py`` -- ``create_enet`` of ``lib/enet.py``
without its classifier, frozen, in ``eval()``.  Forward only.

* ``ENetEncoder.from_state_dict(sd, device)`` takes the reference's checkpoint as it is (the keys of
  ``create_enet(num_classes).state_dict()``), folds every BatchNorm (eps 0.001, running statistics) and the reference's
  eval-mode dropout factor ``1 - p`` into the convolutions in float64 on the host, composes the asymmetric 1x5 / 5x1 pair into
  its 5x5 equivalent, rounds to float32 once and packs the buffer ``include/spacap_hip.h`` describes;
* ``enc(images)``: normalised f32 ``(B, 3, H, W)`` on the device -> ``(B, (H/8)(W/8), 128)`` pixel-major, the layout
  ``MultiviewProjector.project_features(..., channels_last=True)`` reads with no copy; ``layout="nchw"`` gives the
  reference's ``(B, 128, H/8, W/8)`` as a transposed view;
* ``enc.from_uint8(images_u8, mean, std)``: ``(B, H, W, 3)`` uint8 frames, normalised ``(u8 / 255 - mean) / std`` inside the
  first kernel.

One launch for the initial block and two per bottleneck, no library kernel, no host synchronisation: a call can be captured
in a graph.  CPU tensors raise ``RuntimeError("... CPU not supported")``: there is no host fallback.
"""
import numpy as np
import torch

from ._eval_util import gpu
from ._native import check, lib

EPS = 1e-3
_STAGE = [("reg", 1), ("reg", 2), ("asym", 1), ("reg", 4), ("reg", 1), ("reg", 8), ("asym", 1), ("reg", 16)]
# (kind, C_in, C_out, dilation, drop p) of the 22 bottlenecks; bottleneck i sits at index 4 + i of the reference's Sequential
LAYERS = ([("down", 16, 64, 1, 0.01)] + [("reg", 64, 64, 1, 0.01)] * 4 + [("down", 64, 128, 1, 0.1)]
          + [(k, 128, 128, d, 0.1) for k, d in _STAGE * 2])
KIND = {"reg": 0, "asym": 1, "down": 2}
CLASSIFIER = f"{4 + len(LAYERS)}."


class _Reader:
    """Typed access to a state dict that remembers which keys were read."""

    def __init__(self, sd):
        self.sd, self.used = sd, set()

    def get(self, key, shape):
        if key not in self.sd:
            raise KeyError(f"enet: state dict has no key {key!r}")
        v = self.sd[key]
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if tuple(v.shape) != tuple(shape):
            raise ValueError(f"enet: {key!r} has shape {tuple(v.shape)}, expected {tuple(shape)}")
        self.used.add(key)
        return v.astype(np.float64)

    def bn(self, prefix, c):
        """(scale, mean, beta): y = (x - mean) * scale + beta"""
        g, b, m, v = (self.get(f"{prefix}.{n}", (c,)) for n in ("weight", "bias", "running_mean", "running_var"))
        return g / np.sqrt(v + EPS), m, b


def _fold(w, bias, bn, factor=1.0):
    s, m, beta = bn
    b = np.zeros(w.shape[0]) if bias is None else bias
    return w * (s * factor)[:, None, None, None], ((b - m) * s + beta) * factor


def _rows(w):
    """(O, C, kh, kw) -> (O, kh kw C): tap-major, input-channel-minor"""
    return np.ascontiguousarray(w.transpose(0, 2, 3, 1)).reshape(w.shape[0], -1)


def fold_and_pack(sd):
    """The packed float32 parameter buffer (numpy) of ``sd`` and the set of keys it consumed."""
    r = _Reader(sd)
    s, m, beta = r.bn("2", 16)
    w0 = r.get("0.0.weight", (13, 3, 3, 3)) * s[:13, None, None, None]
    b0 = (r.get("0.0.bias", (13,)) - m[:13]) * s[:13] + beta[:13]
    w = np.zeros((16, 27))
    w[:13] = _rows(w0)
    bias, scale = np.zeros(16), np.ones(16)
    bias[:13], bias[13:] = b0, beta[13:] - m[13:] * s[13:]
    scale[13:] = s[13:]
    parts = [w.reshape(-1), bias, scale, r.get("3.weight", (16,))]
    for i, (kind, cin, cout, _, p) in enumerate(LAYERS):
        mid, pre = cout // 4, f"{4 + i}.0.0"
        w1 = r.get(f"{pre}.0.weight", (mid, cin, 2, 2) if kind == "down" else (mid, cin, 1, 1))
        w1, b1 = _fold(w1, None, r.bn(f"{pre}.1", mid))
        a1 = r.get(f"{pre}.2.weight", (mid,))
        if kind == "asym":   # W[o, i, ky, kx] = sum_m W5x1[o, m, ky] W1x5[m, i, kx]: exact, the 1x5 conv has no bias
            w2 = np.einsum("omy,mix->oiyx", r.get(f"{pre}.4.weight", (mid, mid, 5, 1))[:, :, :, 0],
                           r.get(f"{pre}.3.weight", (mid, mid, 1, 5))[:, :, 0, :])
            b2, k = r.get(f"{pre}.4.bias", (mid,)), 5
        else:
            w2, b2, k = r.get(f"{pre}.3.weight", (mid, mid, 3, 3)), r.get(f"{pre}.3.bias", (mid,)), 4
        w2, b2 = _fold(w2, b2, r.bn(f"{pre}.{k}", mid))
        a2 = r.get(f"{pre}.{k + 1}.weight", (mid,))
        w3, b3 = _fold(r.get(f"{pre}.{k + 2}.weight", (cout, mid, 1, 1)), None, r.bn(f"{pre}.{k + 3}", cout), 1.0 - p)
        a3 = r.get(f"{4 + i}.2.weight", (cout,))
        layer = [_rows(w1).reshape(-1), b1, a1, _rows(w2).reshape(-1), b2, a2, _rows(w3).reshape(-1), b3, a3]
        assert sum(x.size for x in layer) == lib.spacap_enet_bottleneck_param_floats(KIND[kind], cin, cout)
        parts += layer
    packed = np.concatenate(parts).astype(np.float32)
    assert packed.size == lib.spacap_enet_param_floats()
    return packed, r.used


class ENetEncoder:
    SCANNET_MEAN = (0.496342, 0.466664, 0.440796)   # scripts/compute_multiview_features.py: the Normalize of its frames
    SCANNET_STD = (0.277856, 0.28623, 0.291129)

    def __init__(self, params):
        self.params = params                         # the packed float32 buffer on its device

    @classmethod
    def from_state_dict(cls, sd, device):
        """``sd``: the reference's checkpoint (tensors or arrays).  The classifier (``26.0.weight``) and the
        ``num_batches_tracked`` counters are ignored; a missing key raises KeyError, a wrongly shaped one ValueError, both
        naming the key."""
        packed, _ = fold_and_pack(sd)
        return cls(torch.from_numpy(packed).to(device))

    # ---- calls -------------------------------------------------------------------------------------------------------------
    def _encode(self, fn, name, images, B, H, W, extra, layout):
        if layout not in ("pixel", "nchw"):
            raise ValueError(f"enet: layout={layout!r}, expected 'pixel' or 'nchw'")
        dev = images.device
        if self.params.device != dev:
            raise RuntimeError(f"enet: images on {dev}, parameters on {self.params.device}")
        if H % 2 or W % 2 or H < 8 or W < 8:
            raise RuntimeError(f"enet: images of {H} x {W}: H and W must be even and at least 8")
        h, w = H // 8, W // 8
        with torch.cuda.device(dev):
            out = torch.empty(B, h * w, 128, dtype=torch.float32, device=dev)
            if B:
                nb = int(lib.spacap_enet_workspace_bytes(B, H, W))
                ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=dev)
                check(fn(images.data_ptr(), B, H, W, *extra, self.params.data_ptr(), self.params.numel(), ws.data_ptr(), nb,
                         out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), name)
        return out if layout == "pixel" else out.view(B, h, w, 128).permute(0, 3, 1, 2)

    def __call__(self, images, layout="pixel"):
        """``images``: f32 (B, 3, H, W) on the device, normalised as the reference feeds its network (a channels-last tensor
        is read as it is, any other goes through one transposing copy).  Returns (B, (H/8)(W/8), 128) f32, pixel-major;
        ``layout="nchw"``: the same memory as (B, 128, H/8, W/8)."""
        images = gpu("enet", images, "images")
        if images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.float32:
            raise RuntimeError(f"enet: images must be float32 (B, 3, H, W), got {images.dtype} {tuple(images.shape)}")
        B, _, H, W = images.shape
        return self._encode(lib.spacap_enet_encode_f32, "spacap_enet_encode_f32", images.permute(0, 2, 3, 1).contiguous(),
                            B, H, W, (), layout)

    def from_uint8(self, images_u8, mean=SCANNET_MEAN, std=SCANNET_STD, layout="pixel"):
        """``images_u8``: uint8 (B, H, W, 3) on the device, as decoded frames lie in memory; x = (u8 / 255 - mean) / std is
        computed in f32, in that order, inside the initial block's kernel."""
        images_u8 = gpu("enet", images_u8, "images_u8")
        if images_u8.dim() != 4 or images_u8.shape[3] != 3 or images_u8.dtype != torch.uint8:
            raise RuntimeError(f"enet: images_u8 must be uint8 (B, H, W, 3), got {images_u8.dtype} {tuple(images_u8.shape)}")
        B, H, W, _ = images_u8.shape
        extra = tuple(float(v) for v in mean) + tuple(float(v) for v in std)
        if len(extra) != 6:
            raise ValueError("enet: mean and std have three entries each")
        return self._encode(lib.spacap_enet_encode_u8, "spacap_enet_encode_u8", images_u8.contiguous(), B, H, W, extra, layout)

    # ---- single layers (tests, tools) -----------------------------------------------------------------------------------------
    def param_offset(self, i):
        """(offset, floats) of bottleneck ``i`` in the packed buffer; ``i = -1``: the initial block"""
        if i < 0:
            return 0, 480
        off = 480
        for j, (kind, cin, cout, _, _) in enumerate(LAYERS):
            n = int(lib.spacap_enet_bottleneck_param_floats(KIND[kind], cin, cout))
            if j == i:
                return off, n
            off += n
        raise IndexError(i)

    def initial(self, images):
        """f32 (B, 3, H, W) -> the initial block's (B, (H/2)(W/2), 16)"""
        images = gpu("enet", images, "images")
        B, _, H, W = images.shape
        x = images.float().permute(0, 2, 3, 1).contiguous()
        with torch.cuda.device(x.device):
            out = torch.empty(B, (H // 2) * (W // 2), 16, dtype=torch.float32, device=x.device)
            check(lib.spacap_enet_initial_f32(x.data_ptr(), B, H, W, self.params.data_ptr(), out.data_ptr(),
                                              torch.cuda.current_stream(x.device).cuda_stream), "spacap_enet_initial_f32")
        return out

    def bottleneck(self, i, x, h, w):
        """bottleneck ``i`` (its own weights, kind and dilation) on pixel-major x (B, h w, C_in) -> (B, ho wo, C_out)"""
        x = gpu("enet", x, "x")
        kind, cin, cout, dil, _ = LAYERS[i]
        B = x.shape[0]
        if tuple(x.shape) != (B, h * w, cin) or x.dtype != torch.float32:
            raise RuntimeError(f"enet: x must be float32 {(B, h * w, cin)}, got {x.dtype} {tuple(x.shape)}")
        x = x.contiguous()
        ho, wo = (h // 2, w // 2) if kind == "down" else (h, w)
        off, _ = self.param_offset(i)
        with torch.cuda.device(x.device):
            out = torch.empty(B, ho * wo, cout, dtype=torch.float32, device=x.device)
            ws = torch.empty(max(B * ho * wo * (cout // 4), 4), dtype=torch.float32, device=x.device)
            check(lib.spacap_enet_bottleneck_f32(x.data_ptr(), B, h, w, cin, cout, KIND[kind], dil,
                                                 self.params.data_ptr() + 4 * off, ws.data_ptr(), ws.numel() * 4, out.data_ptr(),
                                                 torch.cuda.current_stream(x.device).cuda_stream), "spacap_enet_bottleneck_f32")
        return out
