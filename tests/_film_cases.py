"""A plain-torch statement of the FILM frame interpolator and of its four data movements: the on-box reference for shapes no fixture
holds, the baseline arm of tools/film_time.py and - in float64 - the truth the kernel tests compare against.  Everything is functional
over a state dict with the `film_net` key layout, so the same name-keyed synthetic weights serve this file, the fixtures and
cremage_amd.film_hip.

What is independent of the reference and what is not:
  * `warp_truth` and `flow_up2_truth` (float64) are written from the DEFINITION of the operation - source position, clamp, four taps -
    and share nothing with the reference's arithmetic.  They are the truth of the kernel tests.
  * `warp`, `avg_pool2`, `flow_up2_add`, `leaky` and `conv` (fp32) deliberately use the same torch primitives in the same order as the
    reference (`warp`: a normalised grid handed to F.grid_sample), because their ROUNDING is what they are for: they measure how far
    the reference's own fp32 arithmetic is from the truth, which is the yardstick the kernels are held to.
  * `interpolator_forward` is the network's data flow written out functionally from the description below; its building blocks are the
    fp32 functions above, so it reproduces the fixtures to fp32 rounding.

Network, for a configuration cfg (the constructor arguments of Interpolator):
  image pyramid      avg_pool 2 x 2, pyramid_levels levels
  features           a sub-tree of sub_levels (conv3-lrelu, conv3-lrelu, pool) stages with filters << j channels starts at every pyramid
                     level; level i of the cascaded pyramid is cat(stage 0 of tree i, stage 1 of tree i - 1, ...)
  flow               coarse to fine: v = up2(2 v); residual = predictor([feat_a, warp(feat_b, v)]); v += residual.  The finest
                     len(flow_convs) - 1 levels have their own predictor, all coarser ones share the last
  fusion input       per level < fusion_pyramid_levels: warp([image, features] of frame 0, dt * backward flow), the same of frame 1 with
                     (1 - dt) * forward flow, then the two scaled flows
  fusion             coarse to fine: nearest x 2, 2 x 2 conv (pad bottom / right), cat behind the level's input, two conv3-lrelu; 1 x 1 to RGB
"""
import torch
import torch.nn.functional as F

TINY = dict(pyramid_levels=5, fusion_pyramid_levels=4, specialized_levels=2, sub_levels=3, filters=8, flow_convs=(2, 2, 2), flow_filters=(8, 16, 32))
FULL = dict(pyramid_levels=7, fusion_pyramid_levels=5, specialized_levels=3, sub_levels=4, filters=64, flow_convs=(3, 3, 3, 3),
            flow_filters=(32, 64, 128, 256))
FULL_PARAMS = 34436667
SEED = 1234
PREFIX = "film."
DTS = (0.5, 0.25)

# (name, [N, C, H, W], flow amplitude in units of W, per-sample scales or None) - the warp cases of the `film_ops` fixture and of the kernel tests
WARP_CASES = [("warp_c3", (2, 3, 5, 7), 2.0, (0.5, 0.75)), ("warp_c67", (2, 67, 5, 7), 2.0, (0.5, 0.75)), ("warp_c64", (2, 64, 5, 7), 2.0, (0.5, 0.75)),
              ("warp_c3_1x2", (2, 3, 1, 2), 2.0, None),
              ("warp_c67_1x2", (2, 67, 1, 2), 2.0, (0.5, 0.75))]
POOL_CASES = [("pool_c3_6x10", (2, 3, 6, 10)), ("pool_c24_7x9", (2, 24, 7, 9)), ("pool_c3_7x9", (2, 3, 7, 9)), ("pool_c24_6x10", (2, 24, 6, 10))]
UP_CASES = [("up_1x2", (2, 2, 1, 2)), ("up_4x6", (2, 2, 4, 6))]
# (name, Cin, Cout, kernel size, activation) at 8 x 12: every shape class of a FILM conv
CONV_CASES = [("conv_3_8", 3, 8, 3, True), ("conv_128_32", 128, 32, 3, True), ("conv_202_64", 202, 64, 3, True), ("conv_384_64", 384, 64, 3, True),
              ("conv_128_2_k1", 128, 2, 1, False), ("conv_32_2_k1", 32, 2, 1, False), ("conv_128_64_k1", 128, 64, 1, True),
              ("conv_202_32_k2", 202, 32, 2, False), ("conv_128_64_k2", 128, 64, 2, False)]
CONV_HW = (8, 12)


def synth(name, shape, scale=1.0):
    from cremage_amd.synth import synth_input
    return synth_input(name, shape, SEED, scale)


def frames_input(name, shape):
    """frames in [0, 1]"""
    return (synth(name, shape, 0.25) + 0.5).clamp(0.0, 1.0)


def model_inputs(tag, hw):
    """x0, x1, batch_dt of the `film_tiny` / `film_full` fixtures"""
    return frames_input(tag + ".x0", (2, 3) + tuple(hw)), frames_input(tag + ".x1", (2, 3) + tuple(hw)), torch.tensor(DTS, dtype=torch.float32).reshape(2, 1)


def conv_case_inputs(name, cin, cout, k):
    """x, weight, bias of a CONV_CASES entry (weights N(0, 1 / fan_in), as synth_fill_ draws them)"""
    from cremage_amd.synth import synth_tensor
    x = synth(name + ".x", (2, cin) + CONV_HW)
    return x, synth_tensor("film_ops." + name + ".0.weight", (cout, cin, k, k), SEED), synth_tensor("film_ops." + name + ".0.bias", (cout,), SEED)


def warp_case_inputs(name, shape, amp):
    """source, flow: normal flows with a standard deviation of amp * W / 2 (all four borders clamp); every other pixel of the last
    sample's first row flows by whole pixels, every other pixel of the first sample's last row not at all"""
    n, c, h, w = shape
    src = synth(name + ".src", shape)
    flow = synth(name + ".flow", (n, 2, h, w), amp * w / 2.0)
    flow[n - 1, :, 0, ::2] = torch.round(flow[n - 1, :, 0, ::2])
    flow[0, :, h - 1, 1::2] = 0.0
    return src, flow


# ---------------------------------------------------------------------------------------------------------------- the four data movements
def warp(image, flow, scale=None):
    """out[n, :, y, x] = bilinear lookup of image[n] at (x + s flow[n, 0], y + s flow[n, 1]), clamped to the image.  Done the way the
    original does it - normalised grid, F.grid_sample(border, align_corners False) - so that its rounding is the original's."""
    if scale is not None:
        flow = flow * scale.reshape(-1, 1, 1, 1).to(flow.dtype)
    n, _, h, w = flow.shape
    dt, dev = flow.dtype, flow.device
    xs = torch.linspace(-(1 - 1 / w), 1 - 1 / w, w, dtype=dt, device=dev)[None, None, :] + flow[:, 0] / (w * .5)
    ys = torch.linspace(-(1 - 1 / h), 1 - 1 / h, h, dtype=dt, device=dev)[None, :, None] + flow[:, 1] / (h * .5)
    return F.grid_sample(image, torch.stack([xs, ys], dim=3), mode="bilinear", padding_mode="border", align_corners=False)


def warp_truth(image, flow, scale=None):
    """the same lookup from its definition, in float64, without the normalised detour"""
    image, flow = image.double(), flow.double()
    n, c, h, w = image.shape
    s = torch.ones(n, dtype=torch.float64) if scale is None else scale.double().reshape(n)
    xx = torch.arange(w, dtype=torch.float64)[None, None, :] + s[:, None, None] * flow[:, 0]
    yy = torch.arange(h, dtype=torch.float64)[None, :, None] + s[:, None, None] * flow[:, 1]
    xx, yy = xx.clamp(0, w - 1), yy.clamp(0, h - 1)
    x0, y0 = xx.floor(), yy.floor()
    ax, ay = (xx - x0)[:, None], (yy - y0)[:, None]
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
    flat = image.reshape(n, c, h * w)

    def at(yi, xi):
        return torch.gather(flat, 2, (yi * w + xi).reshape(n, 1, h * w).expand(n, c, h * w)).reshape(n, c, h, w)

    return (1 - ay) * ((1 - ax) * at(y0, x0) + ax * at(y0, x1)) + ay * ((1 - ax) * at(y1, x0) + ax * at(y1, x1))


def avg_pool2(x):
    return F.avg_pool2d(x, 2, 2)


def flow_up2_add(v, residual=None):
    up = F.interpolate(2 * v, size=(2 * v.shape[2], 2 * v.shape[3]), mode="bilinear")
    return up if residual is None else residual + up


def flow_up2_truth(v, residual=None):
    """x 2 bilinear, half-pixel centres, from its definition in float64: output o reads o / 2 - 1 / 4 clamped at 0, neighbour clamped at n - 1"""
    v = 2 * v.double()

    def taps(n_in):
        o = torch.arange(2 * n_in, dtype=torch.float64)
        src = ((o + 0.5) / 2 - 0.5).clamp(min=0)
        i0 = src.floor().long()
        return i0, (i0 + 1).clamp(max=n_in - 1), src - i0

    y0, y1, ly = taps(v.shape[2])
    x0, x1, lx = taps(v.shape[3])
    rows = v[:, :, y0] * (1 - ly)[:, None] + v[:, :, y1] * ly[:, None]
    up = rows[:, :, :, x0] * (1 - lx) + rows[:, :, :, x1] * lx
    return up if residual is None else residual.double() + up


def leaky(x, slope=0.2):
    return F.leaky_relu(x, slope)


def conv(x, weight, bias, act=True):
    """kernel 1 / 3: 'same'; kernel 2: zero pad bottom / right"""
    k = weight.shape[2]
    if k % 2 == 0:
        x = F.pad(x, (0, 1, 0, 1))
    y = F.conv2d(x, weight, bias, padding=k // 2 if k % 2 else 0)
    return leaky(y) if act else y


# ---------------------------------------------------------------------------------------------------------------- the network
def _c(sd, key, x, act=True):
    return conv(x, sd[key + ".0.weight"], sd[key + ".0.bias"], act)


def interpolator_forward(sd, cfg, x0, x1, batch_dt):
    """-> the five entries of Interpolator.debug_forward"""
    L, FL, SL = cfg["pyramid_levels"], cfg["fusion_pyramid_levels"], cfg["sub_levels"]
    n_pred = len(cfg["flow_convs"])

    def pyramid(x):
        out = [x]
        for _ in range(L - 1):
            out.append(avg_pool2(out[-1]))
        return out

    def features(images):
        trees = []
        for i, head in enumerate(images):
            stages = []
            for j in range(min(L - i, SL)):
                head = _c(sd, f"extract.extract_sublevels.convs.{j}.1", _c(sd, f"extract.extract_sublevels.convs.{j}.0", head))
                stages.append(head)
                head = avg_pool2(head) if j + 1 < min(L - i, SL) else head
            trees.append(stages)
        return [torch.cat([trees[i - j][j] for j in range(min(i, SL - 1) + 1)], dim=1) for i in range(L)]

    def predictor(level, a, b):
        key = f"predict_flow._predictors.{n_pred - 2 - level}._convs" if level < n_pred - 1 else "predict_flow._predictor._convs"
        n3 = cfg["flow_convs"][min(level, n_pred - 1)]
        net = torch.cat([a, b], dim=1)
        for k in range(n3 + 1):
            net = _c(sd, f"{key}.{k}", net)
        return _c(sd, f"{key}.{n3 + 1}", net, act=False)

    def flow(fa, fb):
        v = predictor(L - 1, fa[-1], fb[-1])
        residuals, flows = [v], [v]
        for i in range(L - 2, -1, -1):
            v = flow_up2_add(v)
            r = predictor(i, fa[i], warp(fb[i], v))
            v = r + v
            residuals.insert(0, r)
            flows.insert(0, v)
        return residuals, flows[:FL]

    im0, im1 = pyramid(x0), pyramid(x1)
    f0, f1 = features(im0), features(im1)
    fres, fflow = flow(f0, f1)
    bres, bflow = flow(f1, f0)
    dt = batch_dt.reshape(-1, 1, 1, 1)
    aligned = []
    for i in range(FL):
        bw, fw = bflow[i] * dt, fflow[i] * (1 - dt)
        aligned.append(torch.cat([warp(torch.cat([im0[i], f0[i]], 1), bw), warp(torch.cat([im1[i], f1[i]], 1), fw), bw, fw], dim=1))
    net = aligned[-1]
    for k in range(FL - 1):
        i = FL - 2 - k
        net = F.interpolate(net, size=aligned[i].shape[2:], mode="nearest")
        net = torch.cat([aligned[i], _c(sd, f"fuse.convs.{k}.0", net, act=False)], dim=1)
        net = _c(sd, f"fuse.convs.{k}.2", _c(sd, f"fuse.convs.{k}.1", net))
    image = F.conv2d(net, sd["fuse.output_conv.weight"], sd["fuse.output_conv.bias"])
    return {"image": [image], "forward_residual_flow_pyramid": fres, "backward_residual_flow_pyramid": bres, "forward_flow_pyramid": fflow,
            "backward_flow_pyramid": bflow}


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))
