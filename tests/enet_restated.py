"""numpy restatement of the ENet image encoder (spacap3d_amd/enet.py, csrc/enet.hip; the reference's lib/enet.py: create_enet
without its classifier, in eval()), and the seeded weights and images the fixture and the tests share.

The network as a table -- LAYERS: (kind, C_in, C_out, dilation, drop p) per bottleneck, behind the initial block:
  initial   conv 3 -> 13 (3x3, stride 2, pad 1, bias) next to maxpool 2x2 of the input, 16 channels, BN, PReLU;
  "down"    reduce = 2x2 stride-2 conv; skip = maxpool 2x2 stride 2 of the input, zero channels appended;
  "reg"     reduce = 1x1 conv; middle = 3x3 conv with dilation = padding; skip = the input;
  "asym"    middle = 1x5 conv (pad (0, 2), no bias) then 5x1 conv (pad (2, 0), bias), nothing between them.
  every bottleneck: reduce (no bias) -> BN -> PReLU -> middle (bias) -> BN -> PReLU -> 1x1 expand (no bias) -> BN -> x (1 - p)
  -> + skip -> PReLU.  BN: eps = 0.001, running statistics.  The (1 - p) is the reference's Dropout2d in eval().
Inner width = C_out / 4.

State-dict keys are those of the reference's nn.Sequential: "0.0" the initial conv, "2" its BN, "3" its PReLU, bottleneck i
(0-based) at index 4 + i with its main branch under "<4+i>.0.0.<k>" and its output PReLU at "<4+i>.2", the classifier at "26.0".
``random_state_dict`` draws every tensor from ONE np.random.default_rng(seed) in the order of ``key_table()`` (weight, bias,
running_mean, running_var for a BN; the int64 ``num_batches_tracked`` counters are zeros and draw nothing)."""
import os
import zlib

import numpy as np

EPS = 1e-3
NUM_CLASSES = 41
STAGE2 = [("reg", 1), ("reg", 2), ("asym", 1), ("reg", 4), ("reg", 1), ("reg", 8), ("asym", 1), ("reg", 16)]
LAYERS = ([("down", 16, 64, 1, 0.01)] + [("reg", 64, 64, 1, 0.01)] * 4 + [("down", 64, 128, 1, 0.1)]
          + [(k, 128, 128, d, 0.1) for k, d in STAGE2 * 2])
STAGE_END = {"stage1": 5, "stage2": 14, "stage3": 22}     # bottlenecks done at the end of each stage
CASES = {"a": dict(seed=11, B=2, H=44, W=24), "b": dict(seed=12, B=1, H=144, W=152)}
WEIGHT_SEED = 2024
WEIGHT_CRC = 0xC77DAA0C                                   # of random_state_dict(WEIGHT_SEED), see weights_crc
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enet_ref.npz")


def _bottleneck_modules(kind, cin, cout):
    """[(sub-index, module kind, shape)] of the main branch"""
    m = cout // 4
    first = ("conv", (m, cin, 2, 2), False) if kind == "down" else ("conv", (m, cin, 1, 1), False)
    if kind == "asym":
        mid = [("conv", (m, m, 1, 5), False), ("conv", (m, m, 5, 1), True)]
    else:
        mid = [("conv", (m, m, 3, 3), True)]
    return [first, ("bn", m), ("prelu", m)] + mid + [("bn", m), ("prelu", m), ("conv", (cout, m, 1, 1), False), ("bn", cout)]


def key_table():
    """[(key, what, shape)] in drawing order; what: conv_w (fan-in scaled), conv_b, bn_w, bn_b, bn_mean, bn_var, bn_count, prelu"""
    rows = []

    def conv(prefix, shape, bias):
        rows.append((prefix + ".weight", "conv_w", shape))
        if bias:
            rows.append((prefix + ".bias", "conv_b", (shape[0],)))

    def bn(prefix, c):
        for name, what in (("weight", "bn_w"), ("bias", "bn_b"), ("running_mean", "bn_mean"), ("running_var", "bn_var"),
                           ("num_batches_tracked", "bn_count")):
            rows.append((f"{prefix}.{name}", what, () if what == "bn_count" else (c,)))

    conv("0.0", (13, 3, 3, 3), True)
    bn("2", 16)
    rows.append(("3.weight", "prelu", (16,)))
    for i, (kind, cin, cout, _, _) in enumerate(LAYERS):
        for k, mod in enumerate(_bottleneck_modules(kind, cin, cout)):
            prefix = f"{4 + i}.0.0.{k}"
            if mod[0] == "conv":
                conv(prefix, mod[1], mod[2])
            elif mod[0] == "bn":
                bn(prefix, mod[1])
            else:
                rows.append((prefix + ".weight", "prelu", (mod[1],)))
        rows.append((f"{4 + i}.2.weight", "prelu", (cout,)))
    conv(f"{4 + len(LAYERS)}.0", (NUM_CLASSES, 128, 1, 1), False)
    return rows


def random_state_dict(seed=WEIGHT_SEED):
    """{key: float32 array (int64 for the counters)}: nothing is left at a value that hides a bug"""
    rng = np.random.default_rng(seed)
    sd = {}
    for key, what, shape in key_table():
        if what == "conv_w":
            v = rng.standard_normal(shape) / np.sqrt(shape[1] * shape[2] * shape[3])
        elif what in ("conv_b", "bn_b", "bn_mean"):
            v = 0.2 * rng.standard_normal(shape)
        elif what in ("bn_w", "bn_var"):
            v = rng.uniform(0.5, 1.5, shape)
        elif what == "prelu":
            v = rng.uniform(-0.1, 0.4, shape)
        else:
            sd[key] = np.zeros((), np.int64)
            continue
        sd[key] = v.astype(np.float32)
    return sd


def weights_crc(sd):
    crc = 0
    for key, what, _ in key_table():
        if what != "bn_count":
            crc = zlib.crc32(np.ascontiguousarray(sd[key]).tobytes(), crc)
    return crc


def random_images(seed, B, H, W):
    """(B, 3, H, W) float32, roughly what a normalised photograph looks like: N(0, 1)"""
    return np.random.default_rng(seed).standard_normal((B, 3, H, W)).astype(np.float32)


def case_inputs(name):
    c = CASES[name]
    return random_state_dict(WEIGHT_SEED), random_images(c["seed"], c["B"], c["H"], c["W"])


# ---- layers, in the dtype of x ----------------------------------------------------------------------------------------------
def conv2d(x, w, b=None, stride=1, pad=(0, 0), dil=1):
    """x (B, C, H, W), w (O, C, kh, kw): zero padding, one matrix product per tap"""
    B, C, H, W = x.shape
    O, _, kh, kw = w.shape
    ph, pw = pad
    xp = np.zeros((B, C, H + 2 * ph, W + 2 * pw), x.dtype)
    xp[:, :, ph:ph + H, pw:pw + W] = x
    ho = (H + 2 * ph - dil * (kh - 1) - 1) // stride + 1
    wo = (W + 2 * pw - dil * (kw - 1) - 1) // stride + 1
    out = np.zeros((B, O, ho, wo), x.dtype)
    for ky in range(kh):
        for kx in range(kw):
            patch = xp[:, :, ky * dil:ky * dil + stride * (ho - 1) + 1:stride, kx * dil:kx * dil + stride * (wo - 1) + 1:stride]
            out += np.einsum("oc,bchw->bohw", w[:, :, ky, kx], patch)
    if b is not None:
        out += b[None, :, None, None]
    return out


def maxpool2(x):
    B, C, H, W = x.shape
    h, w = H // 2, W // 2
    return x[:, :, :2 * h, :2 * w].reshape(B, C, h, 2, w, 2).max(axis=(3, 5))


def prelu(x, a):
    return np.where(x > 0, x, a[None, :, None, None] * x)


def _bn(sd, prefix, x, dt):
    g, b, m, v = (sd[f"{prefix}.{n}"].astype(dt) for n in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(v + dt(EPS))
    return (x - m[None, :, None, None]) * s[None, :, None, None] + b[None, :, None, None]


def initial_block(sd, x, dt=np.float64):
    x = x.astype(dt)
    y = np.concatenate([conv2d(x, sd["0.0.weight"].astype(dt), sd["0.0.bias"].astype(dt), 2, (1, 1)), maxpool2(x)], 1)
    return prelu(_bn(sd, "2", y, dt), sd["3.weight"].astype(dt))


def bottleneck(sd, i, x, dt=np.float64, drop=True, parts=False):
    """bottleneck i (0-based, weights at index 4 + i) on x (B, C_in, h, w).  drop=False leaves the reference's (1 - p) out
    (what the network would be without its Dropout2d quirk).  parts=True also returns the main branch alone."""
    kind, cin, cout, dil, p = LAYERS[i]
    g = lambda k, n: sd[f"{4 + i}.0.0.{k}.{n}"].astype(dt)
    x = x.astype(dt)
    y = conv2d(x, g(0, "weight"), None, 2 if kind == "down" else 1)
    y = prelu(_bn(sd, f"{4 + i}.0.0.1", y, dt), g(2, "weight"))
    if kind == "asym":
        y = conv2d(y, g(3, "weight"), None, 1, (0, 2))
        y = conv2d(y, g(4, "weight"), g(4, "bias"), 1, (2, 0))
        k = 5
    else:
        y = conv2d(y, g(3, "weight"), g(3, "bias"), 1, (dil, dil), dil)
        k = 4
    y = prelu(_bn(sd, f"{4 + i}.0.0.{k}", y, dt), g(k + 1, "weight"))
    y = _bn(sd, f"{4 + i}.0.0.{k + 3}", conv2d(y, g(k + 2, "weight")), dt)
    if drop:
        y = y * dt(1 - p)
    if kind == "down":
        skip = np.zeros_like(y)
        skip[:, :cin] = maxpool2(x)
    else:
        skip = x
    out = prelu(y + skip, sd[f"{4 + i}.2.weight"].astype(dt))
    return (out, y) if parts else out


def forward(sd, images, dt=np.float64, checkpoints=False, drop=True):
    """(B, 128, H/8, W/8); checkpoints=True: a dict with "initial", "stage1", "stage2", "stage3" (= the output)"""
    x = initial_block(sd, images, dt)
    cp = {"initial": x}
    ends = {v: k for k, v in STAGE_END.items()}
    for i in range(len(LAYERS)):
        x = bottleneck(sd, i, x, dt, drop)
        if i + 1 in ends:
            cp[ends[i + 1]] = x
    return cp if checkpoints else x


# ---- folding ---------------------------------------------------------------------------------------------------------------------
def _scale_shift(sd, prefix):
    g, b, m, v = (sd[f"{prefix}.{n}"].astype(np.float64) for n in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(v + EPS)
    return s, m, b


def fold_conv(w, bias, sd, bn_prefix, factor=1.0):
    """w' = w s (1 - p), b' = ((b - mean) s + beta)(1 - p) in float64"""
    s, m, beta = _scale_shift(sd, bn_prefix)
    w = w.astype(np.float64)
    b = np.zeros(w.shape[0]) if bias is None else bias.astype(np.float64)
    return w * (s * factor)[:, None, None, None], ((b - m) * s + beta) * factor


def compose_asym(w1x5, w5x1):
    """the 5x5 weights W[o, i, ky, kx] = sum_m W5x1[o, m, ky] W1x5[m, i, kx] (float64)"""
    return np.einsum("omy,mix->oiyx", w5x1[:, :, :, 0].astype(np.float64), w1x5[:, :, 0, :].astype(np.float64))


def fold(sd):
    """float64: {"initial": (w (13,3,3,3), b (13,), pool scale (3,), pool shift (3,), slopes (16,)),
    "layers": [(w1, b1, a1, w2, b2, a2, w3, b3, a3)]}; the asymmetric middle as its 5x5 equivalent"""
    s, m, beta = _scale_shift(sd, "2")
    w0 = sd["0.0.weight"].astype(np.float64) * s[:13, None, None, None]
    b0 = (sd["0.0.bias"].astype(np.float64) - m[:13]) * s[:13] + beta[:13]
    out = {"initial": (w0, b0, s[13:], beta[13:] - m[13:] * s[13:], sd["3.weight"].astype(np.float64)), "layers": []}
    for i, (kind, cin, cout, dil, p) in enumerate(LAYERS):
        g = lambda k, n: sd[f"{4 + i}.0.0.{k}.{n}"]
        w1, b1 = fold_conv(g(0, "weight"), None, sd, f"{4 + i}.0.0.1")
        if kind == "asym":
            w2, b2, k = compose_asym(g(3, "weight"), g(4, "weight")), g(4, "bias"), 5
        else:
            w2, b2, k = g(3, "weight"), g(3, "bias"), 4
        w2, b2 = fold_conv(w2, b2, sd, f"{4 + i}.0.0.{k}")
        w3, b3 = fold_conv(g(k + 2, "weight"), None, sd, f"{4 + i}.0.0.{k + 3}", 1 - p)
        a = lambda key: sd[key].astype(np.float64)
        out["layers"].append((w1, b1, a(f"{4 + i}.0.0.2.weight"), w2, b2, a(f"{4 + i}.0.0.{k + 1}.weight"), w3, b3,
                              a(f"{4 + i}.2.weight")))
    return out


def forward_folded(folded, images, dt=np.float32, checkpoints=False):
    """the network as the kernels see it: folded weights rounded to dt once, y = PReLU(conv(x) + b [+ skip])"""
    c = lambda v: v.astype(dt)
    w0, b0, ps, pt, a0 = folded["initial"]
    x = images.astype(dt)
    x = prelu(np.concatenate([conv2d(x, c(w0), c(b0), 2, (1, 1)),
                              maxpool2(x) * c(ps)[None, :, None, None] + c(pt)[None, :, None, None]], 1), c(a0))
    cp = {"initial": x}
    ends = {v: k for k, v in STAGE_END.items()}
    for i, (kind, cin, cout, dil, p) in enumerate(LAYERS):
        w1, b1, a1, w2, b2, a2, w3, b3, a3 = folded["layers"][i]
        y = prelu(conv2d(x, c(w1), c(b1), 2 if kind == "down" else 1), c(a1))
        d = 1 if kind == "asym" else dil
        pad = 2 if kind == "asym" else dil
        y = prelu(conv2d(y, c(w2), c(b2), 1, (pad, pad), d), c(a2))
        y = conv2d(y, c(w3), c(b3))
        if kind == "down":
            y[:, :cin] += maxpool2(x)
        else:
            y = y + x
        x = prelu(y, c(a3))
        if i + 1 in ends:
            cp[ends[i + 1]] = x
    return cp if checkpoints else x


def load_fixture():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}
