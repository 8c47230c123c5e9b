"""Case table of the exact integer-lattice conv tests (test_conv_exact_gpu.py) and the host-side geometry
helpers its coverage proof (test_conv_exact_cases.py) needs.  No GPU and no torch in here.

A run is one call of the C ABI: a module geometry, a direction (0 forward, 1 input gradient, 2 weight gradient),
the kernel cai_conv_kernel_name must report for it, whether cai_conv_split_factor must be above 1, and the
epilogue / layout options of the call.

Options (all optional):
  dtype   "bf16" (default) or "f32": the operand type
  forward:  y = "f32" (pixel-major fp32, default), "bf16" (pixel-major bf16) or "nchw" (fp32 NCHW, scalar stores);
            act = 0 / 1 (ReLU) / 2 (LeakyReLU 0.25); res (cai_conv_fwd_res); abs (in_abs); bias (default True)
  dgrad:    mask = 0 / 1 (POS) / 2 (LEAKY 0.25) / 3 (SIGN); res = 0 / 1 (dgrad_res) / 2 (dgrad_res2)
  wgrad:    abs / sq (input transforms); acc (accumulate = 1 into lattice-filled dw / db); bias (db, default True)
  pitch   row pitches above the channel count on every operand, and a non-dense ysb / ysy on a forward output
"""
from collections import namedtuple

Run = namedtuple("Run", "id geom direction kernel split opts")

FWD, DGRAD, WGRAD = 0, 1, 2
RELU, LEAKY = 1, 2
POS, MLEAKY, SIGN = 1, 2, 3
SLOPE = 0.25


def geom12(kind, B, cin, cout, H, W, k, s, pad=None, op=None):
    """The 12 fields of cai_conv_geom for nn.Conv2d ("conv") / nn.ConvTranspose2d ("deconv") with the module
    input H x W; pad defaults to k // 2 and output_padding to s - 1 (transposed only)."""
    pad = k // 2 if pad is None else pad
    if kind == "conv":
        return (B, cin, H, W, cout, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1, k, s, pad, 0, 0)
    op = s - 1 if op is None else op
    return (B, cin, H, W, cout, (H - 1) * s - 2 * pad + k + op, (W - 1) * s - 2 * pad + k + op, k, s, pad, op, 1)


def gemm_view(g, direction):
    """(phase, kin_c, kout_c, out_h, out_w, OHg, OWg) of the implicit GEMM of a forward / input-gradient call:
    the kernel's input / output channels, its output plane and the (largest) per-phase output grid."""
    B, cin, ih, iw, cout, oh, ow, k, s, pad, op, tr = g
    phase = bool(tr) != bool(direction)
    if direction == 0:
        kin, kout, H, W = cin, cout, oh, ow
    else:
        kin, kout, H, W = cout, cin, ih, iw
    st = s if phase else 1
    return phase, kin, kout, H, W, (H + st - 1) // st, (W + st - 1) // st


def wgrad_view(g):
    """(Ng, Cq, Hg, Wg, M): gradient-side channels, gathered-side channels, the G plane and its pixel count."""
    B, cin, ih, iw, cout, oh, ow, k, s, pad, op, tr = g
    if tr:
        return cin, cout, ih, iw, B * ih * iw
    return cout, cin, oh, ow, B * oh * ow


RUNS = []


def _add(name, g, direction, kernel, split, **opts):
    tag = "fwd dgrad wgrad".split()[direction]
    RUNS.append(Run(f"{name}-{tag}", geom12(*g), direction, kernel, split, opts))


def fwd(name, g, kernel, split, **o):
    _add(name, g, FWD, kernel, split, **o)


def dgr(name, g, kernel, split, **o):
    _add(name, g, DGRAD, kernel, split, **o)


def wgr(name, g, kernel, split, **o):
    _add(name, g, WGRAD, kernel, split, **o)


GB = "conv_gemm_kernel<bf16,%s>"
GF = "conv_gemm_kernel<float,%s>"
GL = "conv_glds_kernel<%s>"
SM = "conv_small_kernel<%s>"

# ---- conv_gemm_kernel<bf16>: input widths that are no multiple of 32 (3 padded to 8, 24, 40, 168) or |x| ----------
g = ("deconv", 2, 40, 3, 9, 7, 5, 2)          # x_hat-like ConvTranspose2d: 3 output channels, fp32 NCHW output
fwd("gemm16-d40-3", g, GB % "256x16", False, y="nchw")
dgr("gemm16-d40-3", g, GB % "128x64", False, mask=POS)
wgr("gemm16-d40-3", g, "wgrad_glds_kernel<256>", False)
g = ("deconv", 2, 168, 3, 9, 7, 5, 2)
fwd("gemm16-d168-3", g, GB % "256x16", True, y="nchw", act=RELU)
dgr("gemm16-d168-3", g, GB % "64x192", False, pitch=True)
wgr("gemm16-d168-3", g, "wgrad_glds_kernel<256>", False, acc=True)
g = ("conv", 3, 40, 40, 9, 7, 5, 2)
fwd("gemm64-c40-40", g, GB % "128x64", True, act=LEAKY)
dgr("gemm64-c40-40", g, GB % "128x64", False, mask=SIGN)
wgr("gemm64-c40-40", g, "wgrad_glds_kernel<256>", False, pitch=True)
g = ("conv", 2, 24, 160, 18, 14, 5, 2)
fwd("gemm192-c24-160", g, GB % "64x192", True, y="bf16", act=RELU)
dgr("gemm192-c24-160", g, SM % "16x32", False, mask=POS, res=1)
g = ("conv", 2, 3, 160, 18, 14, 5, 2)
fwd("gemm192-c3-160", g, GB % "64x192", False, pitch=True)
g = ("conv", 2, 24, 104, 18, 14, 5, 2)
fwd("gemm128-c24-104", g, GB % "128x128", True, y="bf16", act=RELU, res=True)
dgr("gemm128-c24-104", g, GB % "128x64", True, mask=MLEAKY)
g = ("conv", 3, 3, 96, 18, 14, 5, 2)           # 3 input channels (padded to 8)
fwd("gemm128-c3-96", g, GB % "128x128", False, y="bf16", act=LEAKY)
dgr("gemm128-c3-96", g, SM % "16x32", False)
wgr("gemm128-c3-96", g, "wgrad_glds_kernel<256>", False)
g = ("conv", 2, 3, 40, 66, 70, 3, 2)
fwd("gemm64-c3-40", g, GB % "128x64", False, y="bf16")
dgr("gemm64-c3-40", g, GB % "256x16", False, mask=MLEAKY)          # 3 channels: no residual form
wgr("gemm64-c3-40", g, "wgrad_glds_kernel<128>", True)
g = ("conv", 2, 64, 96, 50, 70, 1, 1)          # |x| on load keeps a 64-channel input off the LDS-DMA kernel
fwd("gemm128-abs", g, GB % "128x128", False, abs=True, act=RELU)

# ---- fp32 operands: conv_gemm_kernel<float>, wgrad_kernel<float> (column-sum bias gradient) ------------------------
g = ("conv", 2, 24, 100, 18, 14, 5, 2)
fwd("f32-c24-100", g, GF % "128x128", True, dtype="f32", act=LEAKY)
dgr("f32-c24-100", g, GF % "128x64", True, dtype="f32", mask=POS)
wgr("f32-c24-100", g, "wgrad_kernel<float>", True, dtype="f32")
g = ("deconv", 2, 20, 160, 5, 7, 3, 2)
fwd("f32-d20-160", g, GF % "64x192", False, dtype="f32", pitch=True)
dgr("f32-d20-160", g, GF % "128x64", True, dtype="f32")
wgr("f32-d20-160", g, "wgrad_kernel<float>", True, dtype="f32", acc=True)
g = ("conv", 2, 12, 3, 9, 7, 3, 1)
fwd("f32-c12-3", g, GF % "256x16", False, dtype="f32", y="nchw")

# ---- conv_glds_kernel: the six tilings (128x128 is built but no geometry selects it) --------------------------------
g = ("conv", 2, 64, 96, 50, 70, 1, 1)
fwd("glds256x128-c64-96", g, GL % "256x128", False, act=RELU)
dgr("glds256x128-c64-96", g, SM % "32x64", False, mask=SIGN, res=1)
wgr("glds256x128-c64-96", g, "wgrad_glds_kernel<128>", True)
g = ("conv", 2, 64, 104, 50, 70, 3, 1)
fwd("glds256x128-c64-104", g, GL % "256x128", True, y="bf16", act=LEAKY, res=True)
wgr("glds256x128-c64-104", g, "wgrad_glds_kernel<256>", True, acc=True)
g = ("conv", 2, 96, 160, 50, 70, 1, 1)         # 32-mod-64 input width: the last K-tile is half empty
fwd("glds128x192-c96-160", g, GL % "128x192", False, y="bf16", res=True, act=RELU)
dgr("glds128x192-c96-160", g, GL % "256x128", False, mask=MLEAKY, res=2)
wgr("glds128x192-c96-160", g, "wgrad_glds_kernel<128>", True, pitch=True)
g = ("conv", 2, 160, 160, 50, 70, 3, 1)        # 160: K-tiles straddle two taps
fwd("glds128x192-c160-160", g, GL % "128x192", True, pitch=True)
dgr("glds128x192-c160-160", g, GL % "128x192", True, mask=MLEAKY, res=2, pitch=True)
g = ("conv", 2, 64, 40, 70, 90, 1, 1)
fwd("glds256x64-c64-40", g, GL % "256x64", False, y="bf16", act=RELU)
g = ("conv", 2, 256, 40, 20, 36, 3, 1)
fwd("glds256x64-c256-40", g, GL % "256x64", True, act=RELU)
g = ("conv", 2, 64, 96, 70, 90, 1, 1)
fwd("glds64x128-c64-96", g, GL % "64x128", False, y="bf16", act=LEAKY)
g = ("conv", 2, 512, 96, 70, 90, 1, 1)
fwd("glds64x128-c512-96", g, GL % "64x128", True, y="bf16")
dgr("glds64x128-c512-96", g, GL % "64x128", False, mask=SIGN, res=1)
g = ("conv", 2, 64, 160, 70, 90, 1, 1)
fwd("glds64x192-c64-160", g, GL % "64x192", False)
dgr("glds64x192-c64-160", g, GL % "256x64", False, res=1, mask=POS)
g = ("conv", 2, 512, 160, 70, 90, 1, 1)
fwd("glds64x192-c512-160", g, GL % "64x192", True, y="bf16", act=RELU, res=True)
g = ("deconv", 3, 96, 160, 20, 36, 3, 2)       # the s^2-phase direction on the LDS-DMA kernel, 32-mod-64 width
fwd("glds-phase-d96-160", g, GL % "64x192", False, y="bf16")
dgr("glds-phase-d96-160", g, "conv_halo_kernel<3>", True, mask=POS)     # 5 chunks, 5 splits

# ---- conv_small_kernel: latent-size problems -------------------------------------------------------------------------
g = ("conv", 3, 64, 40, 9, 7, 5, 2)
fwd("small16-c64-40", g, SM % "16x32", False, act=LEAKY)
wgr("small16-c64-40", g, "wgrad_glds_kernel<256>", False, abs=True)
g = ("deconv", 3, 160, 80, 17, 15, 3, 2)       # phase mode
fwd("small32-d160-80", g, SM % "32x32", False, y="bf16", act=RELU, res=True)
dgr("small32-d160-80", g, GB % "64x192", True, mask=MLEAKY, res=1)
g = ("conv", 3, 96, 96, 20, 36, 3, 1)
fwd("small64-c96-96", g, SM % "32x64", False, abs=True)
dgr("small64-c96-96", g, SM % "32x64", False, mask=SIGN, res=2)
wgr("small64-c96-96", g, "wgrad_glds_kernel<256>", True, sq=True)

# ---- halo-staged stride-2 gather kernels (Conv2d forward, ConvTranspose2d input gradient) ----------------------------
g = ("conv", 2, 32, 40, 18, 66, 5, 2)          # 9 x 33 outputs: ragged 8 x 32 tiles, one 32-channel chunk: no split
fwd("halo5-c32-40", g, "conv_halo_kernel<5>", False, y="bf16", act=RELU)
g = ("conv", 2, 96, 40, 18, 66, 5, 2)
fwd("halo5-c96-40", g, "conv_halo_kernel<5>", True, act=LEAKY)
g = ("conv", 4, 160, 96, 56, 272, 3, 2)        # 5 chunks over 3 splits (2, 2, 1)
fwd("halo3-c160-96", g, "conv_halo_kernel<3>", True, y="bf16", act=RELU, res=True)
g = ("conv", 2, 32, 40, 18, 66, 3, 2)
fwd("halo3-c32-40", g, "conv_halo_kernel<3>", False, pitch=True)
g = ("deconv", 2, 40, 32, 9, 33, 5, 2)
dgr("halo5-d40-32", g, "conv_halo_kernel<5>", False, mask=POS, res=1)
g = ("deconv", 2, 96, 64, 9, 33, 3, 2)
dgr("halo3-d96-64", g, "conv_halo_kernel<3>", True, mask=MLEAKY, res=2, pitch=True)

# ---- halo-staged s^2-phase kernels (ConvTranspose2d k5 s2 forward, Conv2d k5 s2 input gradient) -----------------------
g = ("deconv", 2, 64, 40, 9, 33, 5, 2)
fwd("phase-d64-40", g, "conv_halo_phase_kernel", False, y="bf16", act=LEAKY)
g = ("deconv", 2, 128, 40, 9, 33, 5, 2)
fwd("phase-d128-40", g, "conv_halo_phase_kernel", True, act=RELU, pitch=True)
g = ("deconv", 2, 192, 40, 9, 33, 5, 2)       # 192 input channels: three 64-channel chunks, three splits
fwd("phase-d192-40", g, "conv_halo_phase_kernel", True, y="bf16", act=LEAKY, res=True)
g = ("conv", 2, 40, 64, 18, 66, 5, 2)
dgr("phase-c40-64", g, "conv_halo_phase_kernel", False, mask=SIGN, res=1)
g = ("conv", 2, 96, 128, 18, 66, 5, 2)
dgr("phase-c96-128", g, "conv_halo_phase_kernel", True, mask=POS, res=2)
g = ("deconv", 16, 64, 320, 9, 33, 5, 2)       # 192-channel tiles: >= 512 blocks, register-direct stores only
fwd("phase192-d64-320", g, "conv_halo_phase_kernel<192>", False, y="bf16", act=RELU, res=True)
g = ("conv", 16, 320, 64, 18, 66, 5, 2)
dgr("phase192-c320-64", g, "conv_halo_phase_kernel<192>", False, mask=MLEAKY, res=1)
g = ("deconv", 64, 128, 40, 9, 33, 5, 2)       # the four-phase kernel: 256 tiles of 8 x 32
fwd("quad-d128-40", g, "conv_halo_quad_kernel", False, y="bf16", act=LEAKY, pitch=True)
g = ("conv", 64, 40, 128, 18, 66, 5, 2)
dgr("quad-c40-128", g, "conv_halo_quad_kernel", False)
g = ("deconv", 16, 128, 128, 64, 64, 5, 2)     # the training shape (C2 g_s[4]): 64^2 -> 128^2 at B = 16
fwd("quad-full", g, "conv_halo_quad_kernel", False, y="bf16", act=RELU)

# ---- halo-staged stride-1 k3 kernels, 13 images of 33 x 33 (130 ragged tiles) --------------------------------------
g = ("conv", 13, 64, 64, 33, 33, 3, 1)
fwd("s1-64-c64-64", g, "conv_halo_s1_kernel<64>", False, y="bf16", act=RELU, res=True)
dgr("s1-64-c64-64", g, "conv_halo_s1_kernel<64>", False, mask=POS, res=1)
wgr("s1-64-c64-64", g, "wgrad_glds_kernel<256>", True)
g = ("conv", 13, 64, 128, 33, 33, 3, 1)
dgr("s1-64-c64-128", g, "conv_halo_s1_kernel<64>", True, mask=SIGN, res=1)
g = ("conv", 13, 64, 96, 33, 33, 3, 1)
fwd("s1-128-c64-96", g, "conv_halo_s1_kernel<128>", False, act=LEAKY)
g = ("conv", 13, 128, 96, 33, 33, 3, 1)
fwd("s1-128-c128-96", g, "conv_halo_s1_kernel<128>", True, y="bf16", act=RELU, res=True)
dgr("s1-128-c128-96", g, GL % "64x128", True, mask=MLEAKY, res=2)
g = ("conv", 13, 192, 96, 33, 33, 3, 1)       # 192 input channels: 3 chunks over 2 splits (2, 1)
fwd("s1-128-c192-96", g, "conv_halo_s1_kernel<128>", True, act=LEAKY)
g = ("conv", 13, 96, 128, 33, 33, 3, 1)
dgr("s1-128-c96-128", g, "conv_halo_s1_kernel<128>", True, mask=POS, res=1, pitch=True)
g = ("conv", 13, 64, 160, 33, 33, 3, 1)
fwd("s1-192-c64-160", g, "conv_halo_s1_kernel<192>", False, y="bf16", act=LEAKY, res=True)
g = ("conv", 13, 160, 64, 33, 33, 3, 1)
dgr("s1-192-c160-64", g, "conv_halo_s1_kernel<192>", False, mask=SIGN, res=2)
g = ("conv", 13, 128, 320, 33, 33, 3, 1)
fwd("s1-192-c128-320", g, "conv_halo_s1_kernel<192>", False, y="bf16", pitch=True)
g = ("conv", 13, 128, 160, 33, 33, 3, 1)
fwd("s1-192-c128-160", g, "conv_halo_s1_kernel<192>", True, act=RELU)
g = ("conv", 7, 192, 768, 33, 33, 3, 1)        # the longest input-gradient reduction of the table: K = 6912
dgr("s1-192-c192-768", g, "conv_halo_s1_kernel<192>", True, mask=POS)

# ---- weight gradients ---------------------------------------------------------------------------------------------
g = ("conv", 3, 160, 96, 9, 7, 3, 1)
wgr("wsmall-c160-96", g, "wgrad_small_kernel", False)
g = ("conv", 4, 96, 160, 16, 16, 1, 1)
wgr("wsmall-c96-160", g, "wgrad_small_kernel", False, abs=True, acc=True)
g = ("deconv", 3, 96, 160, 9, 7, 3, 2)
wgr("wsmall-d96-160", g, "wgrad_small_kernel", False, pitch=True)
g = ("conv", 2, 3, 40, 18, 14, 3, 2)
wgr("wglds128-c3-40", g, "wgrad_glds_kernel<128>", False, acc=True)
g = ("conv", 2, 64, 40, 50, 70, 1, 1)
wgr("wglds128-c64-40", g, "wgrad_glds_kernel<128>", True, sq=True, acc=True)
g = ("deconv", 2, 40, 24, 25, 35, 5, 2)
wgr("wglds256-d40-24", g, "wgrad_glds_kernel<256>", True, acc=True)
for k in (3, 5):
    # G width 64 (one row per strip), 32 (two rows), 16 (four rows); 3 / 22 strips: one split / five uneven ones
    for r, (Wo, h1, h2) in {1: (64, 3, 11), 2: (32, 6, 22), 4: (16, 8, 44)}.items():
        nm = "wgrad_halo_kernel<%d%s>" % (k, "" if r == 1 else ",r%d" % r)
        wgr("whalo%dr%d-one" % (k, r), ("conv", 2, 64, 40, 2 * h1, 2 * Wo, k, 2), nm, False, pitch=(r == 2))
        wgr("whalo%dr%d-split" % (k, r), ("conv", 2, 64, 40, 2 * h2, 2 * Wo, k, 2), nm, True, acc=(r == 4))
wgr("whalo5-full", ("conv", 8, 128, 128, 128, 128, 5, 2), "wgrad_halo_kernel<5>", True)     # C2 g_a[2] at B = 8: 32768 pixels
wgr("wglds256-c64-64", ("conv", 4, 64, 64, 160, 150, 5, 2), "wgrad_glds_kernel<256>", True)  # several chunks per split
wgr("whalo5-d192-64", ("deconv", 2, 192, 64, 11, 64, 5, 2), "wgrad_halo_kernel<5>", True)      # 64-row tiles
wgr("whalo3r2-d96-128", ("deconv", 2, 96, 128, 22, 32, 3, 2), "wgrad_halo_kernel<3,r2>", True, acc=True)
wgr("whalo3s1-one", ("conv", 2, 64, 40, 3, 64, 3, 1), "wgrad_halo_kernel<3,s1>", False)
wgr("whalo3s1-split", ("conv", 2, 64, 40, 11, 64, 3, 1), "wgrad_halo_kernel<3,s1>", True, acc=True)
wgr("whalo3s1-c128-192", ("conv", 2, 128, 192, 11, 64, 3, 1), "wgrad_halo_kernel<3,s1>", True)   # 192-row tiles
wgr("whalo3s1-c64-64", ("conv", 2, 64, 64, 11, 128, 3, 1), "wgrad_halo_kernel<3,s1>", True, pitch=True)   # 64-row

# ---- names the dispatcher can report but no geometry reaches (the coverage proof scans for them) --------------------
UNREACHED = {
    "conv_glds_kernel<128x128>": "pick_cfg_glds never returns CFG_G4",
    "wgrad_kernel<bf16>": "every bf16 weight gradient takes an LDS-DMA kernel (make_wgrad_plan is called with glds)",
}
# kernels whose split factor is fixed by construction: no case on the other side
NEVER_SPLIT = {"conv_small_kernel<16x32>", "conv_small_kernel<32x32>", "conv_small_kernel<32x64>",
               "conv_halo_quad_kernel", "conv_halo_phase_kernel<192>", "wgrad_small_kernel"}
ALWAYS_SPLIT = {"wgrad_kernel<float>"}       # 8 pixel groups (one per XCD) at least

# ---- csrc/edge.hip and csrc/deconv_small.hip (their own entry points; no dispatch) -----------------------------------
EDGE_CONV = [   # B, C, N, H, W, k   (image H x W, feature grid H/2 x W/2)
    (2, 3, 128, 64, 64, 5),
    (2, 3, 192, 48, 80, 5),
    (2, 1, 128, 32, 34, 3),
    (3, 2, 192, 20, 132, 1),
    (6, 3, 192, 200, 330, 5),    # several tiles per persistent block, ragged column blocks
    (8, 3, 128, 256, 256, 5),    # 131072 gradient pixels: more tiles than resident blocks
]
EDGE_DECONV = [  # B, N, C, H, W, k  (feature grid H x W, image 2H x 2W)
    (2, 128, 3, 32, 32, 5),
    (2, 192, 3, 20, 33, 5),
    (2, 128, 1, 17, 70, 3),
    (4, 128, 3, 128, 128, 5),    # more input-gradient tiles than resident blocks
]
DECONV_SMALL = [  # B, N, C, H, W, k, s
    (2, 128, 3, 16, 16, 5, 2),
    (2, 192, 3, 33, 20, 5, 2),   # odd sizes
    (2, 64, 1, 12, 12, 3, 1),
]
