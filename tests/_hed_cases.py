"""Case tables of ControlNet's HED annotator (modules/annotator/hed/__init__.py: DoubleConvBlock, ControlNetHED_Apache2) and a plain-torch
functional restatement of it over a state dict: in float64 the truth the tests compare against, in float32 on the device the PyTorch
arm of tools/hed_time.py.  The same name-keyed synthetic weights serve this file, the fixtures (tools/gen_golden_hed.py) and
cremage_amd.annotator_hip.

Network: VGG-16 trunk, five blocks of 2, 2, 3, 3, 3 3 x 3 convs (3 -> 64 -> 128 -> 256 -> 512 -> 512) with ReLU, a 2 x 2 max pool in front
of blocks 2 .. 5, and per block a 1 x 1 projection of its ReLU'd output to one channel.  The input has `norm` subtracted.

The "composed arm" (`composed_arm`) does what ops.relu_pool_proj does with nothing but what existed before it: ops.leaky_split(slope=0)
for the ReLU and its planes, F.max_pool2d + ops.split_bf16 for the pooled planes, a torch 1 x 1 conv for the projection.  Same operand
format (hi / lo planes) into the same convs, so its error against a fixture is the yardstick of the new kernel.

Projection scaling.  With the plain name-keyed fill the mean logit of the five projections reaches 35 and about 80 % of the edge map sits
at 254 / 255: byte comparisons would see two values.  `fill_` therefore multiplies the five projection weights and biases by 1 / 16 after
the fill: the logits then lie in [-0.5, 2.4] and the map spans about 110 distinct levels (measured on the CPU, 256 x 320 input)."""
import hashlib

import torch
import torch.nn.functional as F

SEED = 1234
PREFIX = "hed."
FULL_PARAMS = 14716168
FULL_KEYS = 37
PROJ_SCALE = 1.0 / 16.0
LAYERS = (2, 2, 3, 3, 3)

# ---- block fixtures: name -> ((input_channel, output_channel, layer_number), input [N, C, H, W], down_sampling) ------------------------------
BLOCK_CASES = {
    "block_3_64": ((3, 64, 2), (2, 3, 9, 12), False),
    "block_64_128_pool": ((64, 128, 2), (2, 64, 10, 14), True),
    "block_256_512_pool": ((256, 512, 3), (1, 256, 6, 9), True),
}
# full network: name -> (H, W), batch 1
FULL_CASES = {"full_64x96": (64, 96), "full_256x320": (256, 320)}

# ---- kernel cases -----------------------------------------------------------------------------------------------------------------------------
RPP_CHANNELS = (8, 64, 72, 512)  # 1 lane, 8 lanes (butterfly), 9 lanes (the LDS order), 64 lanes (one wave per window)
RPP_SIZES = ((1, 1), (2, 2), (5, 7), (16, 16), (33, 18))  # (1, 1): no pool
RPP_BATCH = 2


def halving_chain(h, w, n):
    """the sizes of n side maps of an (h, w) image: floor-halved from one to the next, as the max pools do"""
    out = []
    for _ in range(n):
        out.append((h, w))
        h, w = max(h // 2, 1), max(w // 2, 1)
    return out


# name -> (target (H, W), side map sizes, batch, seed)
FUSE_CASES = {
    "fuse_37x50": ((37, 50), halving_chain(37, 50, 5), 1, SEED),
    "fuse_64x128_n2": ((64, 128), halving_chain(64, 128, 5), 2, SEED),
    "fuse_16x16_to_1x1": ((16, 16), halving_chain(16, 16, 5), 1, SEED),
    "fuse_three_maps": ((37, 50), halving_chain(37, 50, 5)[1:4], 2, SEED),
    "fuse_single_map": ((37, 50), [(9, 12)], 1, SEED),
}
MARGIN = 1e-6  # no float64 e * 255 of any byte-compared case may lie this close to an integer (tests/test_annot_cpu.py)


def synth(name, shape, scale=1.0):
    from cremage_amd.synth import synth_input
    return synth_input(name, shape, SEED, scale)


def image_input(name, shape):
    """an image as the detector sees it: float32 with integer values 0 .. 255"""
    return (synth(name, shape) * 64 + 128).clamp(0, 255).round()


def block_input(name):
    (cin, _, _), shape, _ = BLOCK_CASES[name]
    return image_input(name + ".x", shape) if cin == 3 else synth(name + ".x", shape)


def full_input(name):
    h, w = FULL_CASES[name]
    return image_input(name + ".x", (1, 3, h, w))


def fuse_maps(name):
    """the side maps of a FUSE_CASES entry, float32 [N, h, w] each"""
    (_, sizes, n, seed) = FUSE_CASES[name]
    from cremage_amd.synth import synth_input
    return [(synth_input(f"{name}.map{i}", (n, h, w), seed) * 4).clamp(-12, 12) for i, (h, w) in enumerate(sizes)]


@torch.no_grad()
def fill_(module, prefix=PREFIX):
    """name-keyed synthetic weights, then every `projection` scaled by PROJ_SCALE (see the module docstring).  Works on the reference's
    classes and on cremage_amd.annotator_hip's: both a whole network and a single DoubleConvBlock."""
    from cremage_amd.synth import synth_fill_
    synth_fill_(module, SEED, prefix=prefix)
    for name, p in module.named_parameters():
        if name.split(".")[-2:-1] == ["projection"]:
            p.mul_(PROJ_SCALE)
    return module


def key_digest(state_dict):
    items = sorted(f"{k}:{tuple(v.shape)}" for k, v in state_dict.items())
    return hashlib.sha1("\n".join(items).encode()).hexdigest(), len(items)


def rel_l2(a, b):
    b = b.double()
    return float((a.detach().double().cpu() - b.cpu()).norm() / b.norm().clamp_min(1e-30))


def to_double(sd):
    return {k: v.double() for k, v in sd.items()}


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def double_conv_block(x, sd, p, layers, down_sampling=False):
    """DoubleConvBlock over the keys p + 'convs.J.weight' ...: returns (h, projection)"""
    h = x
    if down_sampling:
        h = F.max_pool2d(h, kernel_size=(2, 2), stride=(2, 2))
    for j in range(layers):
        h = F.relu(F.conv2d(h, sd[p + f"convs.{j}.weight"], sd[p + f"convs.{j}.bias"], padding=1))
    return h, F.conv2d(h, sd[p + "projection.weight"], sd[p + "projection.bias"])


def hed_forward(x, sd, p=""):
    """ControlNetHED_Apache2.forward: the five projections"""
    h = x - sd[p + "norm"]
    out = []
    for k, layers in enumerate(LAYERS):
        h, proj = double_conv_block(h, sd, p + f"block{k + 1}.", layers, down_sampling=k > 0)
        out.append(proj)
    return tuple(out)


# ---- the composed arm (device; what existed before ops.relu_pool_proj) ---------------------------------------------------------------------------
def composed_relu_pool_proj(x, *, planes=None, pool=None, proj=None):
    from cremage_amd import ops
    pl = pooled = y = None
    r = None
    if planes:
        r, pl, _ = ops.leaky_split(x, 0.0, planes=True)
    else:
        r = F.relu(x)
    if pool:
        pooled = ops.split_bf16(F.max_pool2d(r, 2, 2))
    if proj is not None:
        w, b = proj
        y = F.conv2d(r, w.reshape(1, -1, 1, 1), b)
    return pl, pooled, y


class composed_arm:
    """Context manager: inside it cremage_amd.annotator_hip runs everything between its convs in the composed form above."""

    def __enter__(self):
        from cremage_amd import ops
        self._saved = ops.relu_pool_proj
        ops.relu_pool_proj = composed_relu_pool_proj
        return self

    def __exit__(self, *exc):
        from cremage_amd import ops
        ops.relu_pool_proj = self._saved
        return False


# ---- running cremage_amd.annotator_hip on a fixture (device) ---------------------------------------------------------------------------------
def build_block(name, device):
    from cremage_amd import annotator_hip
    args, _, _ = BLOCK_CASES[name]
    torch.manual_seed(0)
    m = annotator_hip.DoubleConvBlock(*args)
    fill_(m, prefix=PREFIX + name + ".")
    return m.to(device).eval()


def build_full(device):
    from cremage_amd import annotator_hip
    torch.manual_seed(0)
    m = annotator_hip.ControlNetHED_Apache2()
    fill_(m)
    return m.to(device).eval()
