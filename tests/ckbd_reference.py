"""Plain-torch restatement of the checkerboard context model (He et al., CVPR 2021), the specification the
HIP path is tested against.  Runs on the CPU, in whatever dtype its inputs have (fp64 for the parity tests).

  * mask: the taps of the 5x5 context conv at odd (i + j) -- 12 taps, the centre is 0;
  * anchors: the positions with odd (h + w), floor(H W / 2) of them;
  * coder's order of an image: the anchors in raster order, then the non-anchors in raster order, all M channels
    of a position adjacent (brute-force enumeration here; `slot_closed_form` is the formula the kernels use);
  * entropy parameters: ctx = conv(y_hat, weight * mask) + bias, set to 0 at the anchors, then the 1x1 stack on
    cat(params, ctx);
  * two-pass encode: pass A codes the anchors from a zero context, pass B the others from the anchors' y_hat.
"""
import torch
import torch.nn.functional as F


def checkerboard_mask(kh=5, kw=5):
    i = torch.arange(kh).view(kh, 1)
    j = torch.arange(kw).view(1, kw)
    return (i + j) % 2 == 1


def anchor_map(H, W):
    h = torch.arange(H).view(H, 1)
    w = torch.arange(W).view(1, W)
    return (h + w) % 2 == 1


def slot_order(H, W):
    """[(h, w)] in the coder's order, by enumeration."""
    pos = [(h, w) for h in range(H) for w in range(W)]
    return [p for p in pos if (p[0] + p[1]) % 2 == 1] + [p for p in pos if (p[0] + p[1]) % 2 == 0]


def slot_closed_form(h, w, H, W):
    """Slot of (h, w) within its group (anchors or non-anchors)."""
    if W % 2 == 0:
        return h * (W // 2) + (w >> 1)
    return (h * W + w) >> 1


def to_coder_order(t):
    """[B, M, H, W] -> [B, H W M] in the coder's order."""
    B, M, H, W = t.shape
    order = slot_order(H, W)
    hs = torch.tensor([p[0] for p in order], dtype=torch.long)
    ws = torch.tensor([p[1] for p in order], dtype=torch.long)
    return t[:, :, hs, ws].permute(0, 2, 1).reshape(B, H * W * M)


def zero_anchors(t):
    keep = ~anchor_map(t.shape[-2], t.shape[-1])
    return t * keep.to(t.dtype).to(t.device)


def model_weights(net, dtype=torch.float64):
    """(cp_weight, cp_bias, [(w, b)] of the 1x1 stack, slope) of a context model, on the CPU."""
    cp, ep = net.context_prediction, net.entropy_parameters
    layers = [(ep[i].weight.detach().to("cpu", dtype), ep[i].bias.detach().to("cpu", dtype)) for i in (0, 2, 4)]
    return cp.weight.detach().to("cpu", dtype), cp.bias.detach().to("cpu", dtype), layers, ep[1].negative_slope


def entropy_params(y_hat, params, cp_weight, cp_bias, layers, slope=0.01):
    """(scales, means) of the training / estimation forward, given y_hat."""
    kh, kw = cp_weight.shape[-2:]
    w = cp_weight * checkerboard_mask(kh, kw).to(cp_weight.dtype)
    ctx = zero_anchors(F.conv2d(y_hat, w, cp_bias, padding=(kh // 2, kw // 2)))
    h = torch.cat((params, ctx), 1)
    for i, (lw, lb) in enumerate(layers):
        h = F.conv2d(h, lw, lb)
        if i + 1 < len(layers):
            h = F.leaky_relu(h, slope)
    return h.chunk(2, 1)


def build_indexes(scales, scale_table, scale_bound):
    s = torch.clamp_min(scales, scale_bound)
    idx = torch.full(s.shape, len(scale_table) - 1, dtype=torch.int32)
    for t in scale_table[:-1]:
        idx -= (s <= t).int()
    return idx


def two_pass_encode(y, params, cp_weight, cp_bias, layers, slope, scale_table, scale_bound):
    """-> {"symbols", "indexes" ([B, H W M], the coder's order), "y_hat", "scales", "means" ([B, M, H, W])}."""
    B, M, H, W = y.shape
    anchor = anchor_map(H, W)
    y_hat = torch.zeros_like(y)
    scales = torch.zeros_like(y)
    means = torch.zeros_like(y)
    symbols = torch.zeros(y.shape, dtype=torch.int32)
    for sel in (anchor, ~anchor):
        s, m = entropy_params(y_hat, params, cp_weight, cp_bias, layers, slope)
        q = torch.round(y - m)
        y_hat = torch.where(sel, q + m, y_hat)
        symbols = torch.where(sel, q.int(), symbols)
        scales = torch.where(sel, s, scales)
        means = torch.where(sel, m, means)
    indexes = build_indexes(scales, scale_table.to(scales.dtype), scale_bound)
    return {"symbols": to_coder_order(symbols), "indexes": to_coder_order(indexes), "y_hat": y_hat, "scales": scales,
            "means": means}


def make_oracle_checkerboard(ref):
    """Turn the CPU oracle's JointAutoregressiveHierarchicalPriors into the checkerboard model: the mask, and the
    context features zeroed at the anchors (a forward hook on its context conv)."""
    cp = ref.context_prediction
    kh, kw = cp.mask.shape[-2:]
    cp.mask.copy_(checkerboard_mask(kh, kw).to(cp.mask.dtype).expand_as(cp.mask))
    cp.register_forward_hook(lambda mod, inp, out: zero_anchors(out))
    return mask_weight_grad(ref)


def mask_weight_grad(ref):
    """The masked taps take no gradient (a tensor hook: a deepcopy of the model needs it set again)."""
    cp = ref.context_prediction
    cp.weight.register_hook(lambda g: g * cp.mask.to(g.dtype))
    return ref
