"""Case tables of the face unblur / colorize network (modules/unblur_face: UnblurCremageModelV6) and a plain-torch functional
restatement of it over a state dict: the on-box reference for shapes no fixture holds, the baseline arm of tools/unblur_time.py and -
in float64 - the truth the kernel tests compare against.  The same name-keyed synthetic weights serve this file, the fixtures
(tools/gen_golden_unblur.py) and cremage_amd.unblur_hip.

Network (cremage_model_v6.py):
  down   7 x ResnetBlock(stride 2): 3 -> 16 -> 32 -> 64 -> 128 -> 256 -> 512 -> 1024, six post-norm single blocks each, one multi-head
         self-attention behind the blocks of levels 3 .. 6 whose output REPLACES x; then ConvAct(1024 -> 2048, kernel 2, no padding) on 2 x 2
  mid    ConvAct 1x1 2048 -> 4096, self-attention over the single token, ConvAct 1x1 4096 -> 2048
  up     ConvTransposeAct(2048 -> 1024) on the 1 x 1 image (no concat), seven ResnetTransposeBlock's on cat([x, tap]) - the first single
         block of each has ConvTranspose2d(4, 2, 1) as conv1 and as conv_skip - then Conv2d(64 -> 3, 3 x 3) (no concat)
  single block   y = SiLU(GN2(conv2(SiLU(GN1(conv1(x))))) + skip(x)), groups = min(32, C), 28 at C = 112 in the transposed blocks

The "composed arm" (`composed_*`, device functions) does the two new operations with nothing but kernels that existed before them:
the transposed conv as ONE 3 x 3 conv with 4 Cout output channels whose weight holds each parity's 2 x 2 taps embedded in a zero 3 x 3
kernel, followed by a pixel shuffle; the block tail as ops.group_norm + a torch add + F.silu + ops.split_bf16.  Same operand format
(hi / lo bf16 planes), so its error against the float64 truth is the yardstick of the new kernels."""
import hashlib

import torch
import torch.nn.functional as F

SEED = 1234
PREFIX = "unblur."
FULL_PARAMS = 620145507
FULL_KEYS = 573
TAPS = 8  # the eight `h` taps of the down path

# ---- kernel cases ---------------------------------------------------------------------------------------------------------------------
# (name, Cin, Cout, (H, W) of the source grid, bias and SiLU): scaled-down stand-ins for the model's eight transposed-conv shapes
CONVT_CASES = [("ct_64_64_1x1", 64, 64, (1, 1), False), ("ct_128_64_2x2", 128, 64, (2, 2), False), ("ct_192_96_4x4", 192, 96, (4, 4), False),
               ("ct_224_112_8x8", 224, 112, (8, 8), False), ("ct_224_112_5x7", 224, 112, (5, 7), False), ("ct_128_64_16x16", 128, 64, (16, 16), False),
               ("ct_64_64_16x8", 64, 64, (16, 8), False), ("ct_128_64_1x1_bias_silu", 128, 64, (1, 1), True),
               ("ct_64_64_24x24", 64, 64, (24, 24), False)]  # more than 512 source pixels: the one-stage kernel of the large grids
# the model's own eight shapes (tools/unblur_time.py)
CONVT_MODEL_SHAPES = [(2048, 1024, 1), (2048, 1024, 2), (1536, 768, 4), (1024, 512, 8), (640, 320, 16), (384, 192, 32), (224, 112, 64), (128, 64, 128)]
GN_CASES = [(16, 16), (64, 32), (112, 28), (192, 32), (320, 32), (768, 32)]
GN_HW = [(2, 2), (5, 7), (16, 16)]
# (tokens, d_head) of every attention of the model, heads = 8
ATTN_CASES = [(256, 16), (64, 32), (16, 64), (4, 128), (1, 512), (16, 128), (64, 96), (256, 64), (1024, 40)]

# ---- block fixtures: name -> (class, constructor args, input [B, C, H, W] or [B, T, C]) ----------------------------------------------------
BLOCK_CASES = {
    "rsb_3_16_s2": ("ResnetSingleBlock", (3, 16, 2), (2, 3, 6, 10)),
    "rsb_64_128_s2": ("ResnetSingleBlock", (64, 128, 2), (2, 64, 7, 9)),
    "rsb_64_64": ("ResnetSingleBlock", (64, 64, 1), (2, 64, 5, 7)),
    "rstb_224_112": ("ResnetSingleTransposeBlock", (224, 112, 2), (2, 224, 4, 6)),
    "rstb_64_64": ("ResnetSingleTransposeBlock", (64, 64, 1), (2, 64, 5, 7)),
    "rb_64_128": ("ResnetBlock", (64, 128, 2, 2, 8), (2, 64, 8, 12)),
    "rtb_640_320": ("ResnetTransposeBlock", (640, 320, 2, 2, 8), (2, 640, 2, 3)),
    "convact_64_128_k2": ("ConvAct", (64, 128, 2), (2, 64, 2, 2)),
    "convact_64_128_k1": ("ConvAct", (64, 128, 1), (2, 64, 1, 1)),
    "convtact_128_64": ("ConvTransposeAct", (128, 64, 4, 2, 1), (2, 128, 1, 1)),
    "mha_512_8_t1": ("MultiHeadSelfAttention", (512, 8), (2, 1, 512)),
    "mha_512_8_t4": ("MultiHeadSelfAttention", (512, 8), (2, 4, 512)),
}
FULL_HW = (256, 256)
SAMPLE = 16384  # values kept of each tensor of the full-model fixture
_P = 1000003


def synth(name, shape, scale=1.0):
    from cremage_amd.synth import synth_input
    return synth_input(name, shape, SEED, scale)


def block_input(name):
    return synth(name + ".x", BLOCK_CASES[name][2])


def full_input(batch=2):
    """faces in [0, 1] as infer_processed_face hands them over (face_unblur.py:252: / 255)"""
    return (synth("unblur_full.x", (batch, 3) + FULL_HW, 0.25) + 0.5).clamp(0.0, 1.0)


def sample_index(numel, n=SAMPLE):
    """the positions of a flattened tensor a full-model fixture keeps: n of them, a fixed stride apart modulo the size"""
    if numel <= n:
        return torch.arange(numel)
    return (torch.arange(n, dtype=torch.int64) * _P) % numel


def sampled(t, n=SAMPLE):
    return t.detach().reshape(-1)[sample_index(t.numel(), n).to(t.device)]


def key_digest(state_dict):
    items = sorted(f"{k}:{tuple(v.shape)}" for k, v in state_dict.items())
    return hashlib.sha1("\n".join(items).encode()).hexdigest(), len(items)


def rel_l2(a, b):
    b = b.double()
    return float((a.detach().double().cpu() - b.cpu()).norm() / b.norm().clamp_min(1e-30))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def conv_transpose_parity(x, w, bias=None):
    """ConvTranspose2d(kernel 4, stride 2, padding 1) by the parity formula: for output parity (a, b)
    y[2i+a][2j+b] = sum_{u,v in {0,1}} w[:, :, 3-a-2u, 3-b-2v]^T x[i+a-1+u][j+b-1+v], x outside the image = 0.  x [N, Cin, H, W], w [Cin, Cout, 4, 4]."""
    n, cin, h, wd = x.shape
    cout = w.shape[1]
    xp = F.pad(x, (1, 1, 1, 1))
    y = x.new_zeros((n, cout, 2 * h, 2 * wd))
    for a in range(2):
        for b in range(2):
            acc = x.new_zeros((n, cout, h, wd))
            for u in range(2):
                for v in range(2):
                    src = xp[:, :, a + u:a + u + h, b + v:b + v + wd]  # x[i + a - 1 + u][j + b - 1 + v] in padded coordinates
                    acc = acc + torch.einsum("nchw,cd->ndhw", src, w[:, :, 3 - a - 2 * u, 3 - b - 2 * v])
            y[:, :, a::2, b::2] = acc
    return y if bias is None else y + bias.reshape(1, -1, 1, 1)


def groups_of(c, transposed=False):
    return 28 if (transposed and c == 112) else min(32, c)


def single_block(x, sd, p, stride=1, transposed=False):
    """ResnetSingleBlock (transposed=False) / ResnetSingleTransposeBlock over the keys p + 'conv1.weight' ..."""
    w1 = sd[p + "conv1.weight"]
    up = transposed and w1.shape[2] == 4
    skip = x
    if p + "conv_skip.weight" in sd:
        ws = sd[p + "conv_skip.weight"]
        skip = F.conv_transpose2d(x, ws, stride=2, padding=1) if up else F.conv2d(x, ws, stride=stride)
    h = F.conv_transpose2d(x, w1, stride=2, padding=1) if up else F.conv2d(x, w1, stride=1 if transposed else stride, padding=1)
    c = h.shape[1]
    g = groups_of(c, transposed)
    h = F.silu(F.group_norm(h, g, sd[p + "gn1.weight"], sd[p + "gn1.bias"], 1e-5))
    h = F.conv2d(h, sd[p + "conv2.weight"], padding=1)
    h = F.group_norm(h, g, sd[p + "gn2.weight"], sd[p + "gn2.bias"], 1e-5)
    return F.silu(h + skip)


def mha(x, sd, p, heads):
    """MultiHeadSelfAttention on [B, T, C] tokens: softmax(q k^T d^-1/2) v per head, then `out`"""
    b, t, c = x.shape
    d = c // heads
    q = F.linear(x, sd[p + "queries.weight"]).reshape(b, t, heads, d).transpose(1, 2)
    k = F.linear(x, sd[p + "keys.weight"]).reshape(b, t, heads, d).transpose(1, 2)
    v = F.linear(x, sd[p + "values.weight"]).reshape(b, t, heads, d).transpose(1, 2)
    a = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1)
    o = (a @ v).transpose(1, 2).reshape(b, t, c)
    return F.linear(o, sd[p + "out.weight"], sd[p + "out.bias"])


def _attend_image(x, sd, p, heads):
    b, c, h, w = x.shape
    t = mha(x.reshape(b, c, h * w).transpose(1, 2), sd, p, heads)
    return t.transpose(1, 2).reshape(b, c, h, w)


def resnet_block(x, sd, p, stride, transposed=False, heads=8):
    """ResnetBlock / ResnetTransposeBlock: the single blocks p + 'blocks.N.' that the state dict holds, then p + 'attentions.0.' if it is there"""
    i = 0
    while p + f"blocks.{i}.conv1.weight" in sd:
        x = single_block(x, sd, p + f"blocks.{i}.", stride if i == 0 else 1, transposed)
        i += 1
    if p + "attentions.0.out.weight" in sd:
        x = _attend_image(x, sd, p + "attentions.0.", heads)
    return x


def conv_act(x, sd, p, transposed=False):
    w, b = sd[p + "conv.weight"], sd[p + "conv.bias"]
    return F.silu(F.conv_transpose2d(x, w, b, stride=2, padding=1) if transposed else F.conv2d(x, w, b))


def model_forward(x, sd, p=""):
    """UnblurCremageModelV6.forward.  Returns (output, the eight h taps, the mid output)."""
    taps = []
    for i in range(7):
        x = resnet_block(x, sd, p + f"down_blocks.{i}.", 2)
        taps.append(x)
    x = conv_act(x, sd, p + "down_blocks.7.")
    taps.append(x)
    x = conv_act(x, sd, p + "mid_blocks.0.")
    x = _attend_image(x, sd, p + "mid_blocks.1.", 8)
    x = conv_act(x, sd, p + "mid_blocks.2.")
    mid = x
    x = conv_act(x, sd, p + "up_blocks.0.", transposed=True)
    for i in range(1, 8):
        x = torch.cat([x, taps[7 - i]], dim=1)
        x = resnet_block(x, sd, p + f"up_blocks.{i}.", 2, transposed=True)
    return F.conv2d(x, sd[p + "up_blocks.8.weight"], sd[p + "up_blocks.8.bias"], padding=1), taps, mid


def block_forward(name, x, sd):
    """the restatement of a BLOCK_CASES entry over the state dict of the reference class"""
    cls, args, _ = BLOCK_CASES[name]
    if cls == "ResnetSingleBlock":
        return single_block(x, sd, "", args[2])
    if cls == "ResnetSingleTransposeBlock":
        return single_block(x, sd, "", args[2], transposed=True)
    if cls == "ResnetBlock":
        return resnet_block(x, sd, "", args[2], heads=args[4])
    if cls == "ResnetTransposeBlock":
        return resnet_block(x, sd, "", args[2], transposed=True, heads=args[4])
    if cls == "ConvAct":
        return conv_act(x, sd, "")
    if cls == "ConvTransposeAct":
        return conv_act(x, sd, "", transposed=True)
    if cls == "MultiHeadSelfAttention":
        return mha(x, sd, "", args[1])
    raise KeyError(cls)


def to_double(sd):
    return {k: v.double() for k, v in sd.items()}


# ---- the composed arm (device; kernels that existed before conv_transpose2d / group_norm_add_act) -------------------------------------------
def composed_convt_weight(w, bias=None):
    """[Cin, Cout, 4, 4] -> the 3 x 3 conv weight [4 Cout, Cin, 3, 3] (and bias [4 Cout]) whose output channel (2a + b) Cout + co at source
    pixel (i, j) is output (2i + a, 2j + b): tap (u, v) of parity (a, b) sits at kernel position (a + u, b + v), the other five are zero."""
    cin, cout = w.shape[:2]
    w3 = w.new_zeros((4 * cout, cin, 3, 3))
    for a in range(2):
        for b in range(2):
            for u in range(2):
                for v in range(2):
                    w3[(2 * a + b) * cout:(2 * a + b + 1) * cout, :, a + u, b + v] = w[:, :, 3 - a - 2 * u, 3 - b - 2 * v].t()
    return w3.contiguous(), (None if bias is None else bias.repeat(4).contiguous())


def composed_conv_transpose(x, w3, b3, silu=False):
    """x fp32 channels-last on the device, (w3, b3) from composed_convt_weight: split_bf16 -> ops.conv2d on planes -> pixel shuffle (-> F.silu)"""
    from cremage_amd import ops
    hi, lo = ops.split_bf16(x)
    y = ops.conv2d(hi, w3, b3, padding=1, x_lo=lo)
    n, c4, h, wd = y.shape
    cout = c4 // 4
    y = y.reshape(n, 2, 2, cout, h, wd).permute(0, 3, 4, 1, 5, 2).reshape(n, cout, 2 * h, 2 * wd)
    return F.silu(y) if silu else y


def composed_gn_add_act(x, weight, bias, groups, eps, skip=None, silu=True):
    """ops.group_norm + torch add + F.silu + ops.split_bf16: four passes over the tensor.  Returns (y, (hi, lo))."""
    from cremage_amd import ops
    y = ops.group_norm(x, weight, bias, groups, eps)
    if skip is not None:
        y = y + skip
    if silu:
        y = F.silu(y)
    return y, ops.split_bf16(y)


class composed_arm:
    """Context manager: inside it cremage_amd.unblur_hip runs its two new operations in the composed form above - the network made of
    nothing but the kernels that existed before them.  Same planes in, same destinations out."""

    def __enter__(self):
        from cremage_amd import ops
        self._saved = (ops.conv_transpose2d, ops.group_norm_add_act)
        w3s = {}

        def conv_transpose2d(x_hi, x_lo, weight, bias=None, silu=False):
            key = (id(weight), weight._version, None if bias is None else id(bias))
            if key not in w3s:
                w3s[key] = (weight,) + composed_convt_weight(weight.detach(), None if bias is None else bias.detach())
            _, w3, b3 = w3s[key]
            y = ops.conv2d(x_hi, w3, b3, padding=1, x_lo=x_lo)
            n, c4, h, wd = y.shape
            cout = c4 // 4
            y = y.reshape(n, 2, 2, cout, h, wd).permute(0, 3, 4, 1, 5, 2).reshape(n, cout, 2 * h, 2 * wd).contiguous(memory_format=torch.channels_last)
            return F.silu(y) if silu else y

        def group_norm_add_act(x, weight, bias, groups, eps, skip=None, silu=True, out=None, planes=None, fp32=True):
            y, (hi, lo) = composed_gn_add_act(x, weight, bias, groups, eps, skip, silu)
            if out is not None:
                out.copy_(y)
                y = out
            if planes is None or planes is False:
                return (y if fp32 else None), None
            if planes is not True:
                planes[0].copy_(hi)
                planes[1].copy_(lo)
                hi, lo = planes
            return (y if fp32 else None), (hi, lo)

        ops.conv_transpose2d, ops.group_norm_add_act = conv_transpose2d, group_norm_add_act
        return self

    def __exit__(self, *exc):
        from cremage_amd import ops
        ops.conv_transpose2d, ops.group_norm_add_act = self._saved
        return False


# ---- running cremage_amd.unblur_hip on a fixture (device) ----------------------------------------------------------------------------------
def build_block(name, device):
    """the cremage_amd.unblur_hip class of a BLOCK_CASES entry with the fixture's name-keyed weights, on the device"""
    from cremage_amd import unblur_hip
    from cremage_amd.synth import synth_fill_
    cls, args, _ = BLOCK_CASES[name]
    torch.manual_seed(0)
    m = getattr(unblur_hip, cls)(*args)
    synth_fill_(m, SEED, prefix=PREFIX + name + ".")
    return m.to(device).eval()


def run_block(m, x):
    """x on the device; [B, T, C] tokens go to forward(q, k, v)"""
    with torch.no_grad():
        return m(x, x, x) if x.dim() == 3 else m(x.contiguous(memory_format=torch.channels_last))


def full_tensors(out):
    """debug_forward's dict -> the fixture's names"""
    d = {"out": out["out"][0], "mid": out["mid"][0]}
    for i, t in enumerate(out["h"]):
        d[f"h.{i}"] = t
    return d
