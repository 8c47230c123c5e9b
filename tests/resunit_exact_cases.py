"""Case table and CPU reference of the exact integer-lattice tests of the fused ResidualUnit kernels
(csrc/resunit.hip: cai_resunit, cai_resunit_wgrad, cai_resunit_wgrad_batch).  No GPU in here: the coverage and
sensitivity proof (test_resunit_exact_cases.py) runs on the reference alone, test_resunit_exact_gpu.py compares the
kernels with it bit for bit.

The reference restates compressai/layers/layers.py:211-226 in torch on the CPU.  Every operand is a small integer,
so every stage is an exact integer before its one round-to-nearest-even to bf16, and the next stage takes the
rounded value, as the kernel does (it keeps h1 / h2 as bf16 in LDS):

  forward    h1 = bf16(relu(conv1x1(x, wa) + ba)),  h2 = bf16(relu(conv3x3(h1, wb, pad 1) + bb)),
             y  = bf16(relu(conv1x1(h2, wc) + bc + x))
  backward   gc = gy (y > 0),  gb = bf16((gc Wc^T) (h2 > 0)),  ga = bf16(conv3x3^T(gb, wb) (h1 > 0)),
             dx = bf16((ga Wa^T + gc [+ res2]) [(xmask > 0)]);  y, h1, h2, xmask are masks only: independent
             draws with zeros, negative zeros and negative values at a chosen density of positives
  weight gradients   dWa = sum_p ga x,  dWb[ty][tx] = sum_p gb h1[p + (ty - 1, tx - 1)],  dWc = sum_p gc h2 and the
             column sums of ga, gb, gc; six independent operands from {+-1, +-2, +-3}, fp32 results

Dense +-1 operands cannot keep all three chained bf16 stages at or below 256, where bf16 holds every integer, so
every cai_resunit case declares one focus stage (A: h1 / gb, B: h2 / ga, C: y / dx): at most 1 % of that stage's
exact values may exceed 256.  The other stages are still compared bit for bit with the rounding of the exact
integer, they are only less sensitive in the low bits.  Bias shifts (forward) and mask densities (backward) bring the
focus stage under the cap; SHARES records the share above 256 of every stage as measured on the reference.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

from test_conv_exact_gpu import _gen, lattice

EXACT = 1 << 24
CAP = 0.01                # largest share of a focus stage's exact values above 256
FWD, BWD = 0, 1
RW_BATCH_MAX = 24         # csrc/resunit.hip: jobs per batched launch and width

Unit = namedtuple("Unit", "id n B H W direction focus opts")
Wg = namedtuple("Wg", "id n B H W acc pitch")


def mask_draw(shape, density, gen):
    """A ReLU-mask operand: positive (1 or 2) with probability `density`, else one of 0, -0, -1, -2."""
    pos = torch.rand(shape, generator=gen) < density
    p = torch.randint(1, 3, shape, generator=gen).float()
    k = torch.randint(0, 4, shape, generator=gen)
    neg = torch.tensor([0.0, -0.0, -1.0, -2.0])[k]
    return torch.where(pos, p, neg)


# ---- cai_resunit -----------------------------------------------------------------------------------------------------
# forward bias shifts (ba, bb) and backward mask densities (y, h2, h1) per (width, focus)
SHIFTS = {(192, "A"): (0, 0), (192, "B"): (-20, 0), (192, "C"): (-24, -100),
          (128, "A"): (0, 0), (128, "B"): (-16, 0), (128, "C"): (-20, -60)}
DENS = {(192, "A"): (0.5, 0.5, 0.5), (192, "B"): (0.125, 0.06, 0.5), (192, "C"): (0.125, 0.06, 0.05),
        (128, "A"): (0.5, 0.5, 0.5), (128, "B"): (0.125, 0.06, 0.5), (128, "C"): (0.25, 0.1, 0.05)}
XMASK_DENSITY = 0.5

# (B, H, W), forward focus, backward focus, backward options (gy_masked, res2, xmask), pitch
_SHAPES = [
    ((1, 8, 8), "A", "A", (0, 0, 1), False),       # one full tile; last unit of a chain
    ((1, 3, 5), "A", "B", (1, 0, 1), False),       # smaller than a tile: halo outside on all sides; middle unit
    ((1, 1, 1), "B", "C", (1, 1, 0), False),       # first unit of AttentionBlock's branch a
    ((1, 1, 19), "B", "A", (1, 0, 0), False),      # a single row, three tiles; first unit of branch b
    ((2, 9, 17), "C", "C", (0, 1, 0), False),      # ragged both ways, batch 2
    ((2, 13, 21), "C", "B", (0, 0, 0), False),
    ((3, 16, 24), "B", "C", (1, 1, 1), False),     # whole tiles only
    ((2, 9, 12), "A", "B", (0, 1, 1), True),       # every row pitch above N
]
# the four option sets compressai._ops issues (_chain_forward / _chain_backward)
ISSUED = {(0, 0, 1), (1, 0, 1), (1, 1, 0), (1, 0, 0)}

UNITS = []
for _n in (192, 128):
    for (_B, _H, _W), _ff, _fb, _o, _pitch in _SHAPES:
        _tag = f"{_n}-{_B}x{_H}x{_W}" + ("-pitch" if _pitch else "")
        UNITS.append(Unit("fwd" + _tag, _n, _B, _H, _W, FWD, _ff, dict(pitch=_pitch)))
        UNITS.append(Unit("bwd" + _tag, _n, _B, _H, _W, BWD, _fb,
                          dict(gy_masked=_o[0], res2=_o[1], xmask=_o[2], pitch=_pitch)))


def unit_lds(u):
    """Row pitches of a case: (x_ld, out_ld, y_ld, res2_ld, xmask_ld); different multiples of 8 / 4 above N."""
    n = u.n
    if not u.opts["pitch"]:
        return n, n, n, n, n
    return n + 8, n + 4, n + 16, n + 12, n + 20


def draw_unit(u):
    """The operands of a cai_resunit case, NCHW fp32 on the CPU."""
    n, nh = u.n, u.n // 2
    gen = _gen(u.id)
    shp = lambda c: (u.B, c, u.H, u.W)    # noqa: E731
    t = dict(wa=lattice((nh, n, 1, 1), 1, gen), wb=lattice((nh, nh, 3, 3), 1, gen), wc=lattice((n, nh, 1, 1), 1, gen))
    if u.direction == FWD:
        sa, sb = SHIFTS[(n, u.focus)]
        t.update(x=lattice(shp(n), 1, gen), ba=lattice((nh,), 3, gen) + sa, bb=lattice((nh,), 3, gen) + sb,
                 bc=lattice((n,), 3, gen))
    else:
        dy, d2, d1 = DENS[(n, u.focus)]
        t.update(gy=lattice(shp(n), 1, gen), y=mask_draw(shp(n), dy, gen), h2=mask_draw(shp(nh), d2, gen),
                 h1=mask_draw(shp(nh), d1, gen))
        t["res2"] = lattice(shp(n), 1, gen) if u.opts["res2"] else None
        t["xmask"] = mask_draw(shp(n), XMASK_DENSITY, gen) if u.opts["xmask"] else None
    return t


def bf(t):
    """One round-to-nearest-even to bf16, back in t's type."""
    return t.to(torch.bfloat16).to(t.dtype)


TAP = (2, 1)              # the tap the `tap_row` mutant zeroes in the bottom row of every 8 x 8 tile


def _one_tap(wb):
    w = torch.zeros_like(wb)
    w[:, :, TAP[0], TAP[1]] = wb[:, :, TAP[0], TAP[1]]
    return w


def _tile_bottom(v):
    rows = (torch.arange(v.shape[2]) % 8 == 7).to(v.dtype).view(1, 1, -1, 1)
    return v * rows


def ref_forward(t, d=torch.float32, mutant=None):
    """-> (exact, stored, l1): per stage the exact integers before rounding, the bf16-rounded values the kernel
    stores (h1, h2, y) and the L1 bound sum |w| |operand| + |addends| of every element.
    Mutants: "halo_bias" the out-of-image halo of h1 holds relu(ba) instead of 0; "tap_row" one tap of wb
    contributes nothing to the bottom row of every tile."""
    x, wa, wb, wc, ba, bb, bc = (t[k].to(d) for k in ("x", "wa", "wb", "wc", "ba", "bb", "bc"))
    e1 = torch.relu(F.conv2d(x, wa, ba))
    h1 = bf(e1)
    if mutant == "halo_bias":
        B, nh, H, W = h1.shape
        hp = bf(torch.relu(ba)).view(1, -1, 1, 1).expand(B, nh, H + 2, W + 2).clone()
        hp[:, :, 1:-1, 1:-1] = h1
        c2 = F.conv2d(hp, wb)
    else:
        c2 = F.conv2d(h1, wb, padding=1)
    if mutant == "tap_row":
        c2 = c2 - _tile_bottom(F.conv2d(h1, _one_tap(wb), padding=1))
    e2 = torch.relu(c2 + bb.view(1, -1, 1, 1))
    h2 = bf(e2)
    e3 = torch.relu(F.conv2d(h2, wc, bc) + x)
    y = bf(e3)
    l1 = (F.conv2d(x.abs(), wa.abs(), ba.abs()), F.conv2d(h1.abs(), wb.abs(), bb.abs(), padding=1),
          F.conv2d(h2.abs(), wc.abs(), bc.abs()) + x.abs())
    return (e1, e2, e3), (h1, h2, y), l1


def ref_backward(t, d=torch.float32, mutant=None):
    """-> (exact, stored, l1) of (gb, ga, dx), and gc.  Mutants: "tap_row"; "res2_tail" res2 is dropped for the last
    16 channels; "h1_ge" the h1 mask is taken as >= 0."""
    gy, ym, h1m, h2m, wa, wb, wc = (t[k].to(d) for k in ("gy", "y", "h1", "h2", "wa", "wb", "wc"))
    gc = gy * (ym > 0)                                     # in {-1, 0, 1}: bf16 holds it
    wct, wat = wc.transpose(0, 1), wa.transpose(0, 1)
    eb = F.conv2d(gc, wct) * (h2m > 0)
    gb = bf(eb)
    c = F.conv_transpose2d(gb, wb, padding=1)
    if mutant == "tap_row":
        c = c - _tile_bottom(F.conv_transpose2d(gb, _one_tap(wb), padding=1))
    ea = c * ((h1m >= 0) if mutant == "h1_ge" else (h1m > 0))
    ga = bf(ea)
    ex = F.conv2d(ga, wat) + gc
    lx = F.conv2d(ga.abs(), wat.abs()) + gc.abs()
    if t["res2"] is not None:
        r = t["res2"].to(d).clone()
        if mutant == "res2_tail":
            r[:, -16:] = 0
        ex = ex + r
        lx = lx + t["res2"].to(d).abs()
    if t["xmask"] is not None:
        ex = ex * (t["xmask"].to(d) > 0)
    dx = bf(ex)
    l1 = (F.conv2d(gc.abs(), wct.abs()), F.conv_transpose2d(gb.abs(), wb.abs(), padding=1), lx)
    return (eb, ea, ex), (gb, ga, dx), l1, gc


def ref_unit(u, t, d=torch.float32, mutant=None):
    """-> (exact, stored, l1[, gc]) of a case in either direction."""
    return ref_forward(t, d, mutant) if u.direction == FWD else ref_backward(t, d, mutant)


def shares(exact):
    """Share of each stage's exact values above 256."""
    return tuple((e.abs() > 256).double().mean().item() for e in exact)


def check_unit_lattice(u, ref):
    """The two conditions of a cai_resunit case, on the reference alone: every partial sum of every stage is an
    exact fp32 integer, and the focus stage stays where bf16 holds every integer."""
    exact, stored, l1 = ref[:3]
    for k, b in enumerate(l1):
        assert b.max().item() < EXACT, (u.id, "ABC"[k], b.max().item())
    for e in exact:
        assert torch.equal(e, e.round()), u.id
    sh = shares(exact)
    k = "ABC".index(u.focus)
    assert sh[k] <= CAP, f"{u.id}: {sh[k]:.4f} of the exact stage {u.focus} values exceed 256"
    assert sh[0] <= CAP, f"{u.id}: stage A exceeds 256 ({sh[0]:.4f})"
    return sh


# percent of the exact values above 256 per stage (A, B, C), measured on the reference (test_resunit_exact_cases.py
# asserts the record)
SHARES = {
    "fwd192-1x8x8": (0.0, 17.53, 45.42),
    "bwd192-1x8x8": (0.0, 8.81, 42.46),
    "fwd192-1x3x5": (0.0, 10.35, 45.59),
    "bwd192-1x3x5": (0.0, 0.0, 10.52),
    "fwd192-1x1x1": (0.0, 0.0, 3.12),
    "bwd192-1x1x1": (0.0, 0.0, 0.0),
    "fwd192-1x1x19": (0.0, 0.0, 12.09),
    "bwd192-1x1x19": (0.0, 1.37, 74.59),
    "fwd192-2x9x17": (0.0, 0.0, 0.01),
    "bwd192-2x9x17": (0.0, 0.0, 0.15),
    "fwd192-2x13x21": (0.0, 0.0, 0.05),
    "bwd192-2x13x21": (0.0, 0.0, 26.91),
    "fwd192-3x16x24": (0.0, 0.01, 30.8),
    "bwd192-3x16x24": (0.0, 0.0, 0.16),
    "fwd192-2x9x12-pitch": (0.0, 16.26, 47.07),
    "bwd192-2x9x12-pitch": (0.0, 0.0, 13.11),
    "fwd128-1x8x8": (0.0, 5.81, 41.36),
    "bwd128-1x8x8": (0.0, 2.37, 35.99),
    "fwd128-1x3x5": (0.0, 7.6, 41.72),
    "bwd128-1x3x5": (0.0, 0.0, 0.47),
    "fwd128-1x1x1": (0.0, 0.0, 3.12),
    "bwd128-1x1x1": (0.0, 0.0, 0.0),
    "fwd128-1x1x19": (0.0, 0.0, 2.88),
    "bwd128-1x1x19": (0.0, 0.16, 52.3),
    "fwd128-2x9x17": (0.0, 0.0, 0.0),
    "bwd128-2x9x17": (0.0, 0.0, 0.31),
    "fwd128-2x13x21": (0.0, 0.0, 0.0),
    "bwd128-2x13x21": (0.0, 0.0, 4.39),
    "fwd128-3x16x24": (0.0, 0.0, 15.04),
    "bwd128-3x16x24": (0.0, 0.0, 0.21),
    "fwd128-2x9x12-pitch": (0.0, 7.32, 41.78),
    "bwd128-2x9x12-pitch": (0.0, 0.0, 2.79),
}


# ---- cai_resunit_wgrad -----------------------------------------------------------------------------------------------
def rw_splits(P):
    """(S, chunk) of csrc/resunit.hip rw_splits / rw_ws: S pixel splits of `chunk` pixels, a multiple of 64."""
    s0 = min(32, max(1, P // 256))
    chunk = ((P + s0 - 1) // s0 + 63) // 64 * 64
    return (P + chunk - 1) // chunk, chunk


def rw_workspace_bytes(n, P):
    """The workspace layout of rw_ws: three slab sets and three bias partials, each rounded up to 256 bytes."""
    nh, (S, _) = n // 2, rw_splits(P)
    up = lambda v: (v + 255) // 256 * 256    # noqa: E731
    return (up(S * nh * n * 4) + up(S * nh * 9 * nh * 4) + up(S * n * nh * 4)
            + up(S * nh * 4) + up(S * nh * 4) + up(S * n * 4))


# (B, H, W), x_ld / gc_ld above N
_WG_SHAPES = [
    ((1, 5, 7), False),        # P = 35: one partial step
    ((1, 13, 13), False),      # P = 169: S = 1, rows no multiple of anything
    ((2, 9, 16), True),        # P = 288
    ((2, 13, 21), False),      # P = 546: S = 2, chunk 320, ragged last split, the plane boundary 273 inside a step
    ((1, 20, 55), True),       # P = 1100: S = 4, last split 140
    ((4, 24, 24), False),      # P = 2304: S = 9
    ((2, 64, 64), False),      # P = 8192: S = 32
    ((2, 37, 1), False),       # W = 1: both column taps are outside everywhere
    ((3, 1, 50), False),       # H = 1
]
WGRADS = []
for _k, _n in enumerate((192, 128)):
    for _i, ((_B, _H, _W), _pitch) in enumerate(_WG_SHAPES):
        _acc = (_i + _k) % 2
        WGRADS.append(Wg(f"wg{_n}-{_B}x{_H}x{_W}" + ("-acc" if _acc else "") + ("-pitch" if _pitch else ""),
                         _n, _B, _H, _W, _acc, _pitch))

# cai_resunit_wgrad_batch: 28 units of N = 192 (one launch flushes at RW_BATCH_MAX = 24), 7 of N = 128 in between
_BATCH_SHAPES = [(1, 5, 7), (1, 13, 13), (2, 9, 16), (2, 13, 21), (1, 7, 30)]
BATCH = []
for _i in range(35):
    _n = 128 if _i % 5 == 2 else 192
    _B, _H, _W = (4, 24, 24) if _i == 11 else _BATCH_SHAPES[_i % len(_BATCH_SHAPES) if _n == 192 else _i % 3]
    BATCH.append(Wg(f"batch{_i}-{_n}-{_B}x{_H}x{_W}", _n, _B, _H, _W, _i % 2, False))


def wg_shapes(n):
    nh = n // 2
    return (nh, n, 1, 1), (nh,), (nh, nh, 3, 3), (nh,), (n, nh, 1, 1), (n,)


def draw_wgrad(c):
    """Six independent operands (x, h1, h2, ga, gb, gc) from {+-1, +-2, +-3}, and the accumulate prefill
    (dwa, dba, dwb, dbb, dwc, dbc) from the same lattice."""
    n, nh = c.n, c.n // 2
    gen = _gen(c.id)
    ops = [lattice((c.B, ch, c.H, c.W), 3, gen) for ch in (n, nh, nh, nh, nh, n)]
    init = [lattice(s, 3, gen) for s in wg_shapes(n)] if c.acc else None
    return ops, init


def ref_wgrad(c, ops, init, d=torch.float32, mutant=None):
    """(dwa, dba, dwb, dbb, dwc, dbc) by the formulas of cai_resunit_wgrad_args (include/cai.h) on pixel-major
    [P][C] matrices.  Mutants: "last_pixel" the last pixel of the last split is lost; "col_wrap" dWb's column shift
    ignores the row end, so j + dx wraps into the neighbouring row (or image)."""
    n, nh, H, W = c.n, c.n // 2, c.H, c.W
    P = c.B * H * W
    assert P * 9 + 3 < EXACT
    x, h1, h2, ga, gb, gc = (v.to(d).permute(0, 2, 3, 1).reshape(P, -1) for v in ops)
    if mutant == "last_pixel":
        ga, gb, gc = (torch.cat([g[:-1], torch.zeros_like(g[-1:])]) for g in (ga, gb, gc))
    m = torch.arange(P)
    r = m % (H * W)
    i, j = r // W, r % W
    dwb = torch.zeros(nh, nh, 3, 3, dtype=d)
    for ty in range(3):
        for tx in range(3):
            dy, dx = ty - 1, tx - 1
            src = m + dy * W + dx
            ok = (i + dy >= 0) & (i + dy < H)
            if mutant == "col_wrap":
                ok &= (src >= 0) & (src < P)
            else:
                ok &= (j + dx >= 0) & (j + dx < W)
            xs = torch.zeros_like(h1)
            xs[ok] = h1[src[ok]]
            dwb[:, :, ty, tx] = gb.t() @ xs
    out = [(ga.t() @ x).reshape(nh, n, 1, 1), ga.sum(0), dwb, gb.sum(0), (gc.t() @ h2).reshape(n, nh, 1, 1), gc.sum(0)]
    if init is not None:
        out = [o + v.to(d) for o, v in zip(out, init)]
    return out
