"""Plain-torch restatement of the operations of csrc/swin.hip, written from their definitions: LayerNorm, exact
GELU, shifted-window cross attention over 4 x 4 windows with 32-wide heads, and the channel aligner's pooled sum
and affine.  Every function computes in the dtype of its operands (fp32 or fp64), so the same code gives the
reference (fp64) and the error model of a correct fp32 implementation.

Tokens are rows: token l = r * Wr + c of image b is row b * Hr * Wr + l.
"""
import math

import torch

WS, HD = 4, 32
WN = WS * WS


# ---- LayerNorm ------------------------------------------------------------------------------------------------------
def layernorm_fwd(x, w, b, eps):
    """x [n][C] -> y, mean [n], rstd [n] (biased variance, as nn.LayerNorm)."""
    mean = x.mean(dim=1)
    d = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((d * d).mean(dim=1) + eps)
    return d * rstd[:, None] * w + b, mean, rstd


def layernorm_bwd(x, dy, w, mean, rstd):
    """The gradient of layernorm_fwd's y for the given (saved) mean and rstd -> dx, dw, db."""
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * w
    dx = rstd[:, None] * (g - g.mean(dim=1, keepdim=True) - xh * (g * xh).mean(dim=1, keepdim=True))
    return dx, (dy * xh).sum(dim=0), dy.sum(dim=0)


# ---- GELU -----------------------------------------------------------------------------------------------------------
def gelu_fwd(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_bwd(x, g):
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return g * (cdf + x * pdf)


# ---- window attention -----------------------------------------------------------------------------------------------
def rel_index():
    """[16][16] int32: row of the (2 * 4 - 1)^2 bias table for query token i and key token j of a window."""
    idx = torch.empty(WN, WN, dtype=torch.int32)
    for i in range(WN):
        for j in range(WN):
            dy, dx = i // WS - j // WS, i % WS - j % WS
            idx[i, j] = (dy + WS - 1) * (2 * WS - 1) + (dx + WS - 1)
    return idx


def _windows(t, B, Hr, Wr, shift):
    """rows [B*Hr*Wr][F] -> [B * nW][16][F] after the cyclic shift by -shift."""
    F = t.shape[1]
    t = torch.roll(t.reshape(B, Hr, Wr, F), shifts=(-shift, -shift), dims=(1, 2))
    t = t.reshape(B, Hr // WS, WS, Wr // WS, WS, F).permute(0, 1, 3, 2, 4, 5)
    return t.reshape(-1, WN, F)


def _unwindows(t, B, Hr, Wr, shift):
    F = t.shape[2]
    t = t.reshape(B, Hr // WS, Wr // WS, WS, WS, F).permute(0, 1, 3, 2, 4, 5).reshape(B, Hr, Wr, F)
    return torch.roll(t, shifts=(shift, shift), dims=(1, 2)).reshape(B * Hr * Wr, F)


def window_attn(q, kv, table, index, mask, B, Hr, Wr, heads, shift, scale):
    """q [B*L][heads*32], kv [B*L][2*heads*32] (k then v), table [49][heads], index [16][16], mask [nW][16][16]
    or None -> out [B*L][heads*32]."""
    C = heads * HD
    nW = (Hr // WS) * (Wr // WS)
    qw = _windows(q, B, Hr, Wr, shift).reshape(B * nW, WN, heads, HD).transpose(1, 2)
    kw = _windows(kv[:, :C], B, Hr, Wr, shift).reshape(B * nW, WN, heads, HD).transpose(1, 2)
    vw = _windows(kv[:, C:], B, Hr, Wr, shift).reshape(B * nW, WN, heads, HD).transpose(1, 2)
    s = (qw * scale) @ kw.transpose(-1, -2)                          # [B*nW][heads][16][16]
    s = s + table[index.long().reshape(-1)].reshape(WN, WN, heads).permute(2, 0, 1)
    if mask is not None:
        s = (s.reshape(B, nW, heads, WN, WN) + mask[None, :, None]).reshape(B * nW, heads, WN, WN)
    p = torch.softmax(s, dim=-1)
    o = (p @ vw).transpose(1, 2).reshape(B * nW, WN, C)
    return _unwindows(o, B, Hr, Wr, shift)


def window_attn_grads(q, kv, table, index, mask, B, Hr, Wr, heads, shift, scale, dout):
    """-> out, dq, dkv, dtable: the backward is autograd of window_attn."""
    q, kv, table = (t.detach().clone().requires_grad_() for t in (q, kv, table))
    out = window_attn(q, kv, table, index, mask, B, Hr, Wr, heads, shift, scale)
    dq, dkv, dtable = torch.autograd.grad(out, (q, kv, table), dout)
    return out.detach(), dq, dkv, dtable


# ---- channel aligner ------------------------------------------------------------------------------------------------
def channel_mean(x, x2, scale):
    """x, x2 [B][HW][C] -> scale * sum_p x (* x2)  [B][C]."""
    return scale * (x if x2 is None else x * x2).sum(dim=1)


def channel_affine(x, gamma, beta, beta_scale, HW):
    """x [B][HW][C] (unused and possibly None when gamma is None), gamma / beta [B][C], either None, not both
    -> gamma * x + beta_scale * beta  [B][HW][C]."""
    if gamma is None:
        return (beta * beta_scale)[:, None, :].expand(beta.shape[0], HW, beta.shape[1]).clone()
    y = gamma[:, None, :] * x
    return y if beta is None else y + (beta * beta_scale)[:, None, :]
