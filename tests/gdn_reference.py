"""Case tables and plain-torch restatements for the per-element tests of csrc/gdn.hip, csrc/gdn_lane.hip and the
gdn1 kernels of csrc/elementwise.hip (test_gdn_elem_gpu.py); test_gdn_reference_cpu.py proves this file on the CPU.
No GPU in here.

The reference is written from the header of gdn.hip, in fp64, on the operands exactly as the kernel holds them
(bf16 and fp32 values widen to fp64 without rounding):
    norm[p,i] = beta_i + sum_j gamma[i,j] x[p,j]^2
    GDN : y = x norm^-1/2,  u = -1/2 g x norm^-3/2      IGDN: y = x norm^1/2,  u = 1/2 g x norm^-1/2
    dx[p,j] = g norm^-+1/2 + 2 x[p,j] sum_i gamma[i,j] u[p,i]
    dgamma[i,j] = sum_p u[p,i] x[p,j]^2      dbeta[i] = sum_p u[p,i]
    d = 2 max(raw, bound) dparam,  draw = (raw >= bound or d < 0) ? d : 0        (LowerBound)
with the fp32 bounds the kernels receive, sqrtf(beta_min + ped) and sqrtf(ped), ped = reparam_offset^2 in fp32.

Every reference function also returns, per element, the sum of the absolute values of the terms of that element's
fp64 evaluation (s_*): the scale a rounding error of that element is measured against.
"""
import zlib
from collections import namedtuple

import torch

BETA_MIN, OFF = 1e-6, 2.0 ** -18
_f = lambda v: torch.tensor(v, dtype=torch.float32)
PED = (_f(OFF) * _f(OFF)).item()                          # exact: 2^-36
BBOUND = torch.sqrt(_f(BETA_MIN) + _f(PED)).item()        # fp32 arithmetic, as gdn.hip's host code
GBOUND = torch.sqrt(_f(0.0) + _f(PED)).item()             # 2^-18
EXACT = 1 << 24
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}

C_OF = {"bf16": (32, 64, 96, 128, 160, 192, 224, 256), "f32": (32, 64, 96, 128, 160, 192)}     # GDN_DISPATCH
GBM = 64                                                  # pixels per tile (gdn_fwd_kernel, gdn_bwd_*_kernel)
LANE_MIN_NPIX = 32768
SMALL_NPIX = (1, 63, 64, 65, 130)
# pitch above C of (x, dy, dx, y): one set per entry of SMALL_NPIX in turn, and of every table row by its index
PADS = (dict(x=0, dy=8, dx=24, y=24), dict(x=8, dy=24, dx=0, y=0), dict(x=24, dy=0, dx=8, y=8))


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def rnd(t, dt):
    """fp32 CPU values as the operand type holds them."""
    return t.to(TORCH_DT[dt]).float()


# ---- the launch arithmetic of gdn.hip / gdn_lane.hip, restated ---------------------------------------------------------
def fwd_kernel(dt, npix, C, lane_on=True):
    lane = dt == "bf16" and lane_on and C in (64, 128, 192) and npix >= LANE_MIN_NPIX
    return f"{'gdn_fwd_lane_kernel' if lane else 'gdn_fwd_kernel'}<{C}>"


def bwd_kernel(dt, npix, C, lane_on=True):
    if not (dt == "bf16" and C in (64, 128, 160, 192)):
        return f"gdn_bwd_kernel+param_grad<{C}>"
    if lane_on and C in (64, 128) and npix >= LANE_MIN_NPIX:
        return f"gdn_bwd_lane_kernel<{C}>"
    return f"{'gdn_bwd_wide_kernel' if C >= 160 else 'gdn_bwd_fused_kernel'}<{C}>"


def fwd_tile_launch(dt, npix, C):
    """gdn_fwd_kernel: (grid, PAIR, tiles of block 0, tiles of the last block)."""
    ntiles = (npix + GBM - 1) // GBM
    grid = min(ntiles, 256 * (2 if dt == "bf16" and C <= 192 else 1))
    pair = C <= 128 if dt == "bf16" else C <= 96
    per = lambda b: (ntiles - b + grid - 1) // grid
    return grid, pair, per(0), per(grid - 1)


def bwd_blocks(dt, npix, C, lane_on=True):
    """Blocks (= partials of the reduce job) of the fused, wide and lane backward; 0 on the two-pass path."""
    k = bwd_kernel(dt, npix, C, lane_on)
    if k.startswith("gdn_bwd_kernel"):
        return 0
    if k.startswith("gdn_bwd_lane"):
        return max(1, min(256, ((npix + 63) // 64 + 1) // 2))
    return min(256, (npix + GBM - 1) // GBM)


# ---- case tables ------------------------------------------------------------------------------------------------------
# forward above one tile per block: (id, dtype, C, npix, lane knob, pitch set)
FW = namedtuple("FW", "id dt C npix lane pads")
FWD_MULTI = [
    FW("f32_c32_pair_odd", "f32", 32, 64 * 513 + 5, True, 0),          # grid 256: blocks of 3 (pair + odd tail) and 2
    FW("f32_c64_pair_odd", "f32", 64, 64 * 513 + 5, True, 1),
    FW("f32_c128_single", "f32", 128, 64 * 513 + 5, True, 2),          # one register set
    FW("bf16_c64_pair_odd", "bf16", 64, 64 * 1025 + 5, False, 1),      # grid 512, CAI_GDN_LANE=0
    FW("bf16_c160_single", "bf16", 160, 64 * 1025 + 5, True, 2),       # (no lane kernel at C = 160)
    FW("bf16_c224_occ1", "bf16", 224, 64 * 257 + 5, True, 0),          # grid 256: blocks of 2 and 1
]
FWD_LANE = [FW(f"lane_c{C}_n{n}", "bf16", C, n, True, p)
            for C in (64, 128, 192) for n, p in ((32768, 0), (32768 + 37, 1))]
FWD_LANE.append(FW("lane_c192_n65549_ld32", "bf16", 192, 65549, True, None))        # ld = C + 32 on both sides
FWD_LANE_LD32 = dict(x=32, y=32)

# backward: (id, dtype, C, npix, pitch set)
BW = namedtuple("BW", "id dt C npix pads")
BWD_TWO_PASS = [("bf16", 32), ("bf16", 96)] + [("f32", C) for C in C_OF["f32"]]
BWD_TWO_PASS_BIG = [BW("bf16_c32_n16451", "bf16", 32, 64 * 257 + 3, 1), BW("f32_c32_n16451", "f32", 32, 64 * 257 + 3, 2)]
BWD_FUSED_C = (64, 128, 160, 192)
BWD_FUSED_BIG = [BW(f"bf16_c{C}_n16451", "bf16", C, 64 * 257 + 3, i % 3) for i, C in enumerate(BWD_FUSED_C)]
BWD_LANE = [BW(f"lane_c{C}_n{n}", "bf16", C, n, p)
            for C in (64, 128) for n, p in ((32768, 0), (32768 + 64 * 3 + 5, 1))]

GDN1 = namedtuple("GDN1", "id C npix x n g dx dn y")       # pitches above C
GDN1_CASES = [GDN1("c12", 12, 131, 0, 4, 1, 3, 2, 5), GDN1("c16", 16, 130, 8, 0, 16, 24, 8, 0),
              GDN1("c40", 40, 67, 3, 1, 0, 2, 5, 7)]
REPARAM_C = (32, 192, 256)


# ---- the reference ----------------------------------------------------------------------------------------------------
def reference(x, g, gamma, beta, inverse):
    """fp64 -> dict of y, u, dx, dgamma, dbeta, norm and their scales s_*; g None: forward only."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    q = x * x
    norm = beta + q @ gamma.t()
    f = norm.sqrt() if inverse else norm.rsqrt()
    y = x * f
    out = dict(norm=norm, y=y, s_y=y.abs())
    if g is None:
        return out
    g = g.double()
    u = 0.5 * g * x / norm.sqrt() if inverse else -0.5 * g * x * norm.rsqrt() ** 3
    t1, au = g * f, u.abs()
    out.update(u=u, s_u=au, dx=t1 + 2 * x * (u @ gamma), s_dx=t1.abs() + 2 * x.abs() * (au @ gamma.abs()),
               dgamma=u.t() @ q, s_dgamma=au.t() @ q, dbeta=u.sum(0), s_dbeta=au.sum(0))
    return out


def model(x, g, gamma, beta, inverse, dt, two_pass):
    """A correct implementation at the kernels' declared precision, on the CPU: fp32 arithmetic and accumulation;
    for bf16 the roundings the kernel comments name: x^2 as the MFMA operand, u as the LDS tile, t1 as the dx tile
    it feeds, and the outputs.  dbeta sums the fp32 u in the fused, wide and lane kernels and the stored u on the
    two-pass path (two_pass)."""
    rd = (lambda t: t.bfloat16().float()) if dt == "bf16" else (lambda t: t)
    x, gamma, beta = x.float(), gamma.float(), beta.float()
    q = rd(x * x)
    norm = q @ gamma.t() + beta
    rs = torch.rsqrt(norm)
    f = norm * rs if inverse else rs
    out = dict(y=rd(x * f))
    if g is None:
        return out
    g = g.float()
    u = 0.5 * g * x * rs if inverse else -0.5 * g * x * rs * rs * rs
    ub, t1 = rd(u), rd(g * f)
    out.update(u=ub, dx=rd(t1 + 2.0 * x * (ub @ gamma)), dgamma=ub.t() @ q, dbeta=(ub if two_pass else u).sum(0))
    return out


def reparam(raw, bound, ped=PED):
    """max(raw, bound)^2 - ped in fp64 on the fp32 operands."""
    lb = torch.clamp(raw.double(), min=bound)
    return lb * lb - ped


def gate(raw, bound, dparam):
    """LowerBound / NonNegativeParametrizer backward in the dtype of dparam (fp32: the kernels' own one rounding of
    (2 lb) * dparam, 2 lb being exact)."""
    raw = raw.to(dparam.dtype)
    d = (2.0 * torch.clamp(raw, min=bound)) * dparam
    return torch.where((raw >= bound) | (d < 0), d, torch.zeros_like(d))


def elem_error(got, ref, s):
    """max over elements of |got - ref| / s; an element of scale 0 must be met exactly (inf otherwise)."""
    d = (got.double() - ref).abs()
    nz = s > 0
    if bool((d[~nz] != 0).any()) or bool(torch.isnan(d).any()):
        return float("inf")
    return (d[nz] / s[nz]).max().item() if bool(nz.any()) else 0.0


# ---- gdn1: out = x / norm (inverse: x * norm) and its backward, one product each ---------------------------------------------
def gdn1(x, n, g, inverse):
    """In the dtype of the operands -> y, dx, dnorm."""
    if inverse:
        return x * n, g * n, g * x
    r = 1.0 / n
    return x * r, g * r, -g * x * r * r


# ---- bf16 rounding of an fp64 value, with its neighbours ----------------------------------------------------------------
def bf16_neighbours(ref):
    """fp64 -> (rne, lo, hi, near): the round-to-nearest-even bf16 value of each element (no intermediate fp32), the
    two bf16 values around it (towards and away from zero, signed), and whether it lies within 2^-20 relative of
    their midpoint (such an element may take either).  Zeros give 0, 0, 0, False."""
    a = ref.abs()
    _, e = torch.frexp(a)                                  # a = m 2^e, m in [0.5, 1): 8 significant bits -> ulp 2^(e-8)
    ulp = torch.ldexp(torch.ones_like(a), e - 8)
    k = torch.floor(a / ulp)
    lo, mid = k * ulp, (k + 0.5) * ulp
    hi = lo + ulp
    up = (a > mid) | ((a == mid) & (k % 2 == 1))
    sg = torch.sign(ref)
    zero = a == 0
    z = lambda t: torch.where(zero, torch.zeros_like(t), t)
    near = (a - mid).abs() <= a * 2.0 ** -20
    return z(sg * torch.where(up, hi, lo)), z(sg * lo), z(sg * hi), near & ~zero


# ---- operands ---------------------------------------------------------------------------------------------------------
def tol_operands(name, npix, C, dt):
    """x, dy ~ N(0, 1) in the operand type, gamma = 0.1 I + 0.02 U in the operand type, beta = 1 + 0.1 U (fp32)."""
    g = gen("tol-" + name)
    x, dy = rnd(torch.randn(npix, C, generator=g), dt), rnd(torch.randn(npix, C, generator=g), dt)
    gamma = rnd(0.1 * torch.eye(C) + 0.02 * torch.rand(C, C, generator=g), dt)
    return x, dy, gamma, 1.0 + 0.1 * torch.rand(C, generator=g)


def a1_operands(name, npix, C):
    """x in {0, +-1, +-2}, gamma in {0, 1, 2, 3} / 64, beta in {1, 1.5, 2}: every norm is a multiple of 1 / 64."""
    g = gen("a1-" + name)
    x = torch.randint(-2, 3, (npix, C), generator=g).float()
    gamma = torch.randint(0, 4, (C, C), generator=g).float() / 64
    beta = 1.0 + 0.5 * torch.randint(0, 3, (C,), generator=g).float()
    return x, gamma, beta


def a1_norm_units(x, gamma, beta):
    """The largest sum of |terms| of a norm, in units of 1 / 64 (all terms are non-negative: it is the norm)."""
    return (64 * (beta.double() + (x.double() ** 2) @ gamma.double().t())).max().item()


def a2_operands(name, npix, C):
    """g, x on {0, +-1, +-2, +-3}; with gamma_op = 0, beta = 1 the norm is 1 and u = -+ g x / 2 exactly."""
    g = gen("a2-" + name)
    return (torch.randint(-3, 4, (npix, C), generator=g).float(), torch.randint(-3, 4, (npix, C), generator=g).float())


def a2_prefill(name, C):
    g = gen("a2p-" + name)
    return torch.randint(-5, 6, (C,), generator=g).float(), torch.randint(-5, 6, (C, C), generator=g).float()


def signed_operands(name, npix, C, sign):
    """Non-zero lattice x and g with sign(g x) = sign everywhere."""
    g = gen("sg-" + name)
    x = torch.randint(1, 4, (npix, C), generator=g).float() * (torch.randint(0, 2, (npix, C), generator=g) * 2 - 1)
    return x, sign * torch.sign(x) * torch.randint(1, 4, (npix, C), generator=g).float()


def gate_raws(shape, bound):
    """fp32 raws cycling through: below the bound, one ulp below, at it, one ulp above, above, 0, negative."""
    b = _f(bound)
    vals = torch.stack([b * 0.5, torch.nextafter(b, _f(0.0)), b, torch.nextafter(b, _f(2.0)), b * 2 + 0.25, _f(0.0),
                        -b, _f(-1.0), _f(0.5)])
    n = 1
    for s in shape:
        n *= s
    return vals[(torch.arange(n) * 5 + torch.arange(n) // 9) % len(vals)].reshape(shape)


def sparse_rows(npix, dt, C, lane_on=True):
    """The pixels of a sparse dy: pixel 0, the last valid one (at npix % 64 == 1 the one valid row of a ragged last
    tile), the last row of a full tile and the first row of block 0's second tile (64-pixel tiles or steps; 32-pixel
    tiles in the wide kernel)."""
    rows = {0, npix - 1}
    if npix > GBM:
        rows.add(GBM - 1)
    nb = bwd_blocks(dt, npix, C, lane_on)
    tile = 32 if bwd_kernel(dt, npix, C, lane_on).startswith("gdn_bwd_wide") else GBM
    if nb and nb * tile < npix:
        rows.add(nb * tile)
    return sorted(rows)


# ---- reference mutants of the forward (the faults a whole-tensor norm at bf16 cannot see) ------------------------------
def wave_cols(C, dt):
    """Channels per wave of gdn_fwd_kernel (GdnGeo::NW)."""
    return C // (4 if C % 64 == 0 else 2 if C % 32 == 0 else 1)


MUTANTS = ("drop_kblock", "swap_kblocks", "gamma_t", "skip_beta_tile", "ragged_row")


def mutant_applies(kind, npix, C):
    if kind == "swap_kblocks":
        return C >= 64
    if kind == "ragged_row":
        return npix % GBM != 0 and npix >= 2
    return True


def forward_mutant(kind, x, gamma, beta, inverse, dt):
    """fp64 y of a forward with one fault."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    npix, C = x.shape
    q = x * x
    norm = beta + q @ gamma.t()
    if kind == "drop_kblock":                  # one 32-channel K block lost for one wave's column slice
        kb, cols = C // 32 - 1, slice(0, wave_cols(C, dt))
        norm[:, cols] -= q[:, 32 * kb:32 * kb + 32] @ gamma[cols, 32 * kb:32 * kb + 32].t()
    elif kind == "swap_kblocks":               # x^2 K blocks 0 and 1 meet each other's gamma columns
        qs = q.clone()
        qs[:, 0:32], qs[:, 32:64] = q[:, 32:64], q[:, 0:32]
        norm = beta + qs @ gamma.t()
    elif kind == "gamma_t":
        norm = beta + q @ gamma
    elif kind == "skip_beta_tile":             # the last 16-channel tile without beta
        norm[:, C - 16:] -= beta[C - 16:]
    elif kind == "ragged_row":                 # the ragged tile's last row takes the norm of the row its clamp re-reads
        norm[npix - 1] = norm[npix - 2]
    else:
        raise ValueError(kind)
    return x * (norm.sqrt() if inverse else norm.rsqrt())
