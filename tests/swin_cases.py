"""Case table of the per-op tests of csrc/swin.hip (test_swin_ops_gpu.py) and the host-side restatement of its
launch arithmetic that the coverage proof (test_swin_reference_cpu.py) compares with the built library.  No GPU
and no torch in here.

Every shape is the smallest that reaches its branch; the grid-stride rows (more than 16384 * 256 work items)
are the only ones above a few MB (8 to 70 MB).
"""
from collections import namedtuple

# ---- LayerNorm: (ntok, C) -------------------------------------------------------------------------------------------
# backward launch: nblk = min(1024, ceil(ntok / 64)) blocks of per = ceil(ntok / nblk) tokens, one wave per token;
# C <= 128 runs the register kernel, above it the general one; the parameter reduce unrolls eight rows of a row
# group (32 groups) once a group has eight, i.e. from nblk >= 225 on for group 0 and for every group from 257 on
LN = namedtuple("LN", "id ntok C")
LN_CASES = [
    LN("n5_c1", 5, 1),                # one block, ntok % 4 != 0, C = 1 (63 idle lanes)
    LN("n5_c63", 5, 63),
    LN("n70_c65", 70, 65),            # the second channel of a lane in the register kernel, one lane only
    LN("n130_c96", 130, 96),          # the model's C; 3 blocks of 44 tokens, the last ragged (42)
    LN("n130_c128", 130, 128),        # last C of the register kernel
    LN("n130_c129", 130, 129),        # first C of the general kernel
    LN("n7_c1024", 7, 1024),          # 32 KB of dynamic LDS
    LN("n19203_c24", 19203, 24),      # nblk = 301: the eight-wide unrolled reduce and its remainder loop
    LN("n66001_c8", 66001, 8),        # nblk = 1024, per = 65, 8 trailing empty blocks
]
LN_GENERAL_AT_96 = "n130_c96"         # the row the CAI_LN_BWD_REG=0 child process runs


def ln_launch(ntok, C):
    """(nblk, per, blocks that hold a token, tokens of the last such block)."""
    nblk = max(1, min(1024, (ntok + 63) // 64))
    per = (ntok + nblk - 1) // nblk
    used = (ntok + per - 1) // per
    return nblk, per, used, ntok - (used - 1) * per


# ---- GELU / channel affine dispatch: (rows, C, pitch above C, base offset in elements) ---------------------------------
# bf16 takes the 8-channel vector kernel when C % 8 == 0, every ld % 8 == 0 and every base is 16-byte aligned
EW = namedtuple("EW", "id rows C pad off")
EW_CASES = [
    EW("vec", 37, 16, 0, 0),
    EW("vec_pitched", 37, 16, 8, 0),
    EW("c_mod8", 37, 12, 0, 0),
    EW("ld_mod8", 37, 16, 4, 0),
    EW("base_unaligned", 37, 16, 8, 4),
]
GRID_CAP = 16384 * 256                # grid256(): work items of one pass of the grid-stride loops
# (rows, C) above one pass: fp32 / bf16 scalar by elements, bf16 vector by 8-element groups
EW_STRIDE = {"f32": (65600, 64), "bf16": (524800, 64), "bf16-scalar": (65600, 68)}


def ew_vec(case, dtype):
    """True when a bf16 call of this row takes the vector kernel (fp32 never does)."""
    ld = case.C + case.pad
    es = 2
    return dtype == "bf16" and case.C % 8 == 0 and ld % 8 == 0 and (case.off * es) % 16 == 0


# ---- channel mean: (B, HW, C, dtypes) ---------------------------------------------------------------------------------
# stage 1: chunk = max(256, ceil(HW / max(1, 1024 // B))) pixels per block, ngrp = ceil(C / VEC) 16-byte groups
# (VEC 4 fp32 / 8 bf16), rows = 256 // ngrp pixel rows in flight; stage 2: one wave per (b, c) over the chunks
CM = namedtuple("CM", "id B HW C dtypes")
CM_CASES = [
    CM("b1_hw100_c6", 1, 100, 6, ("f32", "bf16")),          # nchunk 1; C % VEC != 0 in both types
    CM("b3_hw300_c96", 3, 300, 96, ("f32", "bf16")),        # nchunk 2; ngrp 24 / 12: idle threads
    CM("b1_hw16384_c20", 1, 16384, 20, ("f32", "bf16")),    # nchunk 64
    CM("b1_hw16385_c96", 1, 16385, 96, ("f32", "bf16")),    # nchunk 65: stage 2's lane loop wraps
    CM("b2_hw300_c1024", 2, 300, 1024, ("f32", "bf16")),    # fp32 ngrp 256: one row in flight
    CM("b1_hw300_c2048", 1, 300, 2048, ("bf16",)),          # bf16 ngrp 256
]


def cm_launch(B, HW, C, dtype):
    """(nchunk, ngrp, rows)."""
    target = max(1, 1024 // B)
    chunk = max(256, (HW + target - 1) // target)
    vec = 8 if dtype == "bf16" else 4
    ngrp = (C + vec - 1) // vec
    return (HW + chunk - 1) // chunk, ngrp, 256 // ngrp


# ---- channel affine: the EW rows with rows = B * HW -------------------------------------------------------------------
AFFINE_B = (1, 3)
AFFINE_HW = 37
AFFINE_BETA_SCALE = (1.0, 0.5, 0.0)

# ---- window attention: (B, Hr, Wr, heads, shift) ----------------------------------------------------------------------
# one wave per (window, head) item, four per block; the bias gradient goes block partials -> 64 splits of
# ceil(nblk / 64) blocks -> totals -> table rows
AT = namedtuple("AT", "id B Hr Wr heads shift")
AT_CASES = [
    AT("b1_4x12_h3_s1", 1, 4, 12, 3, 1),       # 9 items (% 4 = 1); Hr < Wr, a single window along H
    AT("b1_12x4_h5_s3", 1, 12, 4, 5, 3),       # 15 items (% 4 = 3); Hr > Wr
    AT("b3_8x12_h1_s2", 3, 8, 12, 1, 2),       # 18 items (% 4 = 2)
    AT("b2_12x8_h8_s0", 2, 12, 8, 8, 0),       # 96 items (% 4 = 0), 24 blocks; the 2048-float accumulator
    AT("b3_16x20_h5_s1", 3, 16, 20, 5, 1),     # 300 items, 75 blocks: two-block splits, a one-block split, empty ones
]
# live-score (tolerance) rows: the model's mask at shift 2, none at shift 0
AT_TOL = [
    AT("b1_4x12_h3_s2", 1, 4, 12, 3, 2),
    AT("b1_12x4_h5_s0", 1, 12, 4, 5, 0),
    AT("b3_8x12_h1_s2", 3, 8, 12, 1, 2),
    AT("b2_12x8_h8_s0", 2, 12, 8, 8, 0),
    AT("b3_16x20_h5_s2", 3, 16, 20, 5, 2),
]
AT_TOL_BIG_TABLE = "b3_8x12_h1_s2"             # also run with table entries of +-8
ATTN_SPLITS = 64


def at_launch(c):
    """(items, nblk)."""
    items = c.B * (c.Hr // 4) * (c.Wr // 4) * c.heads
    return items, (items + 3) // 4
