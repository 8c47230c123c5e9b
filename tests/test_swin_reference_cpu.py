"""On the CPU: (1) the plain restatement of the Swin / channel-aligner ops (swin_reference.py) equals the project's
oracle in fp64, so the GPU tests' reference is not wrong in the kernels' way; (2) the case table (swin_cases.py)
reaches every launch branch of csrc/swin.hip, with the launch arithmetic read back from the built library's
workspace functions; (3) every exact case's precondition holds on the reference alone.  No kernel is launched.
"""
import ctypes
import os

import pytest
import torch

import swin_cases as T
import swin_inputs as I
import swin_reference as R

EXACT = 1 << 24


# ---- (1) restatement == oracle, fp64 --------------------------------------------------------------------------------
@pytest.mark.parametrize("Hr,Wr", [(8, 12), (12, 8)])
@pytest.mark.parametrize("shift", [0, 2])
def test_window_attention_equals_oracle(Hr, Wr, shift):
    import cai_oracle_master as OM

    B, heads = 2, 3
    C = heads * R.HD
    g = torch.Generator().manual_seed(7 + shift)
    blk = OM.SwinTransformerBlock(C, (Hr, Wr), heads, window_size=4, shift_size=shift).double()
    att = blk.attn
    att.qkv1, att.qkv2, att.proj = torch.nn.Identity(), torch.nn.Identity(), torch.nn.Identity()
    with torch.no_grad():
        att.relative_position_bias_table.copy_(torch.randn(49, heads, generator=g, dtype=torch.float64))
    assert torch.equal(att.relative_position_index.int(), R.rel_index())
    q = torch.randn(B, Hr * Wr, C, generator=g, dtype=torch.float64, requires_grad=True)
    kv = torch.randn(B, Hr * Wr, 2 * C, generator=g, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(B * Hr * Wr, C, generator=g, dtype=torch.float64)

    # SwinTransformerBlock.forward's shift / partition / reverse path around its attention core
    xq, xg = q.view(B, Hr, Wr, C), kv.view(B, Hr, Wr, 2 * C)
    if shift:
        xq = torch.roll(xq, shifts=(-shift, -shift), dims=(1, 2))
        xg = torch.roll(xg, shifts=(-shift, -shift), dims=(1, 2))
    aw = att(OM.window_partition(xq, 4).view(-1, 16, C), OM.window_partition(xg, 4).view(-1, 16, 2 * C),
             mask=blk.attn_mask).view(-1, 4, 4, C)
    o = OM.window_reverse(aw, 4, Hr, Wr)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    o = o.reshape(B * Hr * Wr, C)
    want = (o.detach(),) + torch.autograd.grad(o, (q, kv, att.relative_position_bias_table), dout)

    got = R.window_attn_grads(q.detach().reshape(-1, C), kv.detach().reshape(-1, 2 * C),
                              att.relative_position_bias_table.detach(), R.rel_index(), blk.attn_mask, B, Hr, Wr,
                              heads, shift, att.scale, dout)
    for name, a, b in zip(("out", "dq", "dkv", "dtable"), got, want):
        assert (a - b.reshape(a.shape)).abs().max().item() <= 1e-12, name


def test_layernorm_gelu_equal_torch_modules():
    g = torch.Generator().manual_seed(3)
    n, C = 37, 96
    x = (torch.randn(n, C, generator=g, dtype=torch.float64) * 2 + 1).requires_grad_()
    dy = torch.randn(n, C, generator=g, dtype=torch.float64)
    ln = torch.nn.LayerNorm(C).double()
    with torch.no_grad():
        ln.weight.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
        ln.bias.copy_(torch.randn(C, generator=g, dtype=torch.float64))
    y = ln(x)
    dx, dw, db = torch.autograd.grad(y, (x, ln.weight, ln.bias), dy)
    y_r, mean, rstd = R.layernorm_fwd(x.detach(), ln.weight.detach(), ln.bias.detach(), ln.eps)
    got = (y_r,) + R.layernorm_bwd(x.detach(), dy, ln.weight.detach(), mean, rstd)
    for name, a, b in zip(("y", "dx", "dw", "db"), got, (y.detach(), dx, dw, db)):
        assert (a - b).abs().max().item() <= 1e-12, name

    x = (torch.rand(4096, generator=g, dtype=torch.float64) * 16 - 8).requires_grad_()
    gy = torch.randn(4096, generator=g, dtype=torch.float64)
    y = torch.nn.GELU()(x)
    dx, = torch.autograd.grad(y, x, gy)
    assert (R.gelu_fwd(x.detach()) - y.detach()).abs().max().item() <= 1e-12
    assert (R.gelu_bwd(x.detach(), gy) - dx).abs().max().item() <= 1e-12


def test_channel_ops_equal_definition():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 30, 7, generator=g, dtype=torch.float64)
    x2 = torch.randn(2, 30, 7, generator=g, dtype=torch.float64)
    ga, be = torch.randn(2, 7, generator=g, dtype=torch.float64), torch.randn(2, 7, generator=g, dtype=torch.float64)
    pooled = torch.nn.AdaptiveAvgPool2d(1)(x.transpose(1, 2).reshape(2, 7, 5, 6)).reshape(2, 7)
    assert (R.channel_mean(x, None, 1 / 30) - pooled).abs().max().item() <= 1e-12
    assert (R.channel_mean(x, x2, 1.0) - torch.einsum("bpc,bpc->bc", x, x2)).abs().max().item() <= 1e-12
    want = torch.stack([x[b] * ga[b] + 0.5 * be[b] for b in range(2)])
    assert (R.channel_affine(x, ga, be, 0.5, 30) - want).abs().max().item() <= 1e-12
    assert torch.equal(R.channel_affine(None, None, be, 2.0, 30), (2.0 * be)[:, None, :].expand(2, 30, 7))
    assert torch.equal(R.channel_affine(x, ga, None, 0.0, 30), x * ga[:, None, :])


# ---- (2) the table reaches every branch -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from compressai import _native

    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libcai.so not built")
    _native.lib.load()
    return _native


def test_layernorm_rows_reach_every_launch_shape(native):
    lib = native.lib.load()
    shapes = {}
    for c in T.LN_CASES:
        nblk, per, used, last = T.ln_launch(c.ntok, c.C)
        assert lib.cai_layernorm_bwd_workspace_bytes(c.ntok, c.C) // (2 * c.C * 4) == nblk, c.id
        shapes[c.id] = (nblk, per, used, last)
        print(f"layernorm {c.id}: nblk {nblk} per {per} used {used} last {last}")
    v = list(shapes.values())
    assert any(nblk == 1 for nblk, *_ in v)
    assert any(1 < nblk and last != per for nblk, per, used, last in v), "a ragged last block"
    assert any(257 <= nblk < 1024 for nblk, *_ in v), "the eight-wide unrolled reduce"
    assert any(nblk == 1024 and per > 64 and used < nblk for nblk, per, used, last in v), "the capped grid"
    Cs = {c.C for c in T.LN_CASES}
    assert {1, 63, 65, 128, 129, 1024} <= Cs
    assert any(c.ntok % 4 for c in T.LN_CASES)
    assert next(c for c in T.LN_CASES if c.id == T.LN_GENERAL_AT_96).C == 96


def test_channel_mean_rows_reach_every_launch_shape(native):
    lib = native.lib.load()
    seen = {"f32": set(), "bf16": set()}
    for c in T.CM_CASES:
        for dt in c.dtypes:
            nchunk, ngrp, rows = T.cm_launch(c.B, c.HW, c.C, dt)
            assert lib.cai_channel_mean_workspace_bytes(c.B, c.HW, c.C) // (c.B * c.C * 4) == nchunk, c.id
            vec = 8 if dt == "bf16" else 4
            seen[dt].add((nchunk, c.C % vec != 0, 256 % ngrp != 0, rows, c.B > 1))
            print(f"channel_mean {c.id} {dt}: nchunk {nchunk} ngrp {ngrp} rows {rows}")
    for dt, s in seen.items():
        assert {1, 2, 64, 65} <= {n for n, *_ in s}, dt
        assert any(rag for _, rag, *_ in s), f"{dt}: C % VEC != 0"
        assert any(idle for _, _, idle, *_ in s), f"{dt}: idle threads"
        assert any(rows == 1 for *_, rows, _ in s), f"{dt}: ngrp = 256"
        assert any(b for *_, b in s), f"{dt}: B > 1"


def test_attention_rows_reach_every_launch_shape(native):
    lib = native.lib.load()
    for cases in (T.AT_CASES, T.AT_TOL):
        for c in cases:
            items, nblk = T.at_launch(c)
            P = native.WindowAttn(16, c.heads * 32, 16, 2 * c.heads * 32, 16, 16, None, c.B, c.Hr, c.Wr, c.heads, 32, 4,
                                  c.shift, 0.25)
            ws = lib.cai_window_attn_bwd_workspace_bytes(ctypes.byref(P))
            assert ws // (c.heads * 256 * 4) - 65 == nblk, c.id
            print(f"attention {c.id}: items {items} nblk {nblk}")
    ex = T.AT_CASES
    assert {T.at_launch(c)[0] % 4 for c in ex} == {0, 1, 2, 3}
    assert any(T.at_launch(c)[1] < T.ATTN_SPLITS for c in ex)
    assert any(T.at_launch(c)[1] > T.ATTN_SPLITS and T.at_launch(c)[1] % T.ATTN_SPLITS for c in ex)
    assert {c.heads for c in ex} == {1, 3, 5, 8} == {c.heads for c in T.AT_TOL}
    assert {c.shift for c in ex} == {0, 1, 2, 3}
    assert any(c.Hr < c.Wr for c in ex) and any(c.Hr > c.Wr for c in ex) and any(4 in (c.Hr, c.Wr) for c in ex)
    assert {c.shift for c in T.AT_TOL} == {0, 2}
    assert {T.at_launch(c)[0] % 4 for c in T.AT_TOL} == {0, 1, 2, 3}


def test_elementwise_rows_reach_every_dispatch():
    """GELU and the channel affine: the bf16 vector kernel and each of its three ways out, and a second pass of
    the grid-stride loop for the scalar (by elements) and the vector (by 8-element groups) kernels."""
    vec = [c for c in T.EW_CASES if T.ew_vec(c, "bf16")]
    assert any(c.pad == 0 for c in vec) and any(c.pad for c in vec)
    out = [c for c in T.EW_CASES if not T.ew_vec(c, "bf16")]
    assert any(c.C % 8 for c in out)
    assert any(c.C % 8 == 0 and (c.C + c.pad) % 8 and c.off == 0 for c in out)
    assert any(c.C % 8 == 0 and (c.C + c.pad) % 8 == 0 and (c.off * 2) % 16 for c in out)
    assert not any(T.ew_vec(c, "f32") for c in T.EW_CASES)
    rows, C = T.EW_STRIDE["f32"]
    assert rows * C > T.GRID_CAP
    rows, C = T.EW_STRIDE["bf16"]
    assert C % 8 == 0 and rows * C // 8 > T.GRID_CAP
    rows, C = T.EW_STRIDE["bf16-scalar"]
    assert C % 8 and rows * C > T.GRID_CAP
    assert set(T.AFFINE_B) == {1, 3} and set(T.AFFINE_BETA_SCALE) == {1.0, 0.5, 0.0}


# ---- (3) preconditions of the exact cases ---------------------------------------------------------------------------
def _bf16_exact(t):
    return torch.equal(t.float().bfloat16().double(), t.double())


def test_group_masks_use_every_group_size():
    for c in T.AT_CASES:
        nW = (c.Hr // 4) * (c.Wr // 4)
        mask, sizes = I.group_mask(nW, c.id)
        assert {s for parts in sizes for s in parts} >= ({16, 8, 4, 2, 1} if nW >= 2 else {16})
        assert all(sum(p) == 16 for p in sizes)
        assert torch.equal(mask, mask.transpose(1, 2)) and (mask.diagonal(dim1=1, dim2=2) == 0).all()
        if nW > 1:
            assert not torch.equal(mask[0], mask[1])          # per window: w versus wglob shows
    assert torch.exp(torch.tensor(I.MASKED)).item() == 0.0 and torch.exp(torch.tensor(I.MASKED).double()).item() == 0.0


def _ds(case, d):
    """dS [B*nW][heads][16][16] of an exact case, written out: P = 1 / n inside a group, dP = dO V^T."""
    C = case.heads * 32
    win = lambda t: R._windows(t.double(), case.B, case.Hr, case.Wr, case.shift).reshape(
        -1, 16, case.heads, 32).transpose(1, 2)
    dp = win(d["dout"]) @ win(d["kv"][:, C:]).transpose(-1, -2)
    nW = (case.Hr // 4) * (case.Wr // 4)
    m = torch.zeros(nW, 16, 16, dtype=torch.float64) if d["mask"] is None else d["mask"].double()
    p = torch.softmax(m, dim=-1).repeat(case.B, 1, 1)[:, None]
    return p * (dp - (p * dp).sum(-1, keepdim=True))


@pytest.mark.parametrize("case", T.AT_CASES, ids=[c.id for c in T.AT_CASES])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_attention_exact_preconditions(case, dtype):
    """The fp32 restatement is bit-equal to the fp64 one; sum |terms| of every reduction, in units of its lattice
    step, stays below 2^24, so any order and grouping of the fp32 sums gives the same bits.  bf16: out and dv
    (k / n, |k| <= n <= 16) are representable; dq and dk are fp32-exact values with up to 18 significant bits (a
    multiple of 1 / 1024 below 256) that the kernel and the reference each round once to bf16."""
    for zero in ("q", "k"):
        for masked in (False, True):
            d = I.attn_exact(case, dtype, zero, masked)
            r32, r64 = I.attn_exact_ref(case, d, torch.float32), I.attn_exact_ref(case, d, torch.float64)
            for name, a, b in zip(("out", "dq", "dkv", "dtable"), r32, r64):
                assert torch.equal(a.double(), b), (name, zero, masked)
            out, dq, dkv, dtable = r64
            C = case.heads * 32
            # q = 0: dk = sum dS q = 0 and dq = sum dS k is live; k = 0: the other way round
            assert torch.equal(dkv[:, :C] if zero == "q" else dq, torch.zeros_like(dq))
            assert (dq if zero == "q" else dkv[:, :C]).abs().max() > 0
            # steps: out, dv 1/16; dS 1/256; dq, dk = 0.25 * sum dS * lattice: 1/1024
            vmax = 3 if dtype == "f32" else 1
            assert 16 * vmax * 16 < EXACT                                        # P.V and P^T.dO, 16 terms
            ds_max = 2 * 32 * vmax * vmax                                        # |dP - sum P dP|
            ds = _ds(case, d)
            assert ds.abs().max() <= ds_max and torch.equal((ds * 256).round(), ds * 256)
            # dq / dk: 16 terms dS * lattice in steps of 1 / 256 (times scale = 1 / 4 at the end or in q)
            assert max(ds.abs().sum(-1).max().item(), ds.abs().sum(-2).max().item()) * vmax * 1024 < EXACT
            for t in (out, dq, dkv):
                assert torch.equal((t * 1024).round(), t * 1024)
            # dtable[r][h] sums dS (steps of 1 / 256) over (i, j) with rel_index == r and every window of head h,
            # plus the integer prefill: bound it by the sum of |dS| of this case's own values
            assert torch.equal((dtable * 256).round(), dtable * 256)
            idx = R.rel_index().long().reshape(-1)
            per_ij = ds.sum(0).reshape(case.heads, 256).t()
            assert torch.equal(torch.zeros(49, case.heads, dtype=torch.float64).index_add_(0, idx, per_ij), dtable)
            tot = torch.zeros(49, case.heads, dtype=torch.float64).index_add_(
                0, idx, ds.abs().sum(0).reshape(case.heads, 256).t())
            assert (tot.max().item() + 3) * 256 < EXACT, "sum of |dS| of a bias-table entry"
            if dtype == "bf16":
                assert _bf16_exact(out) and _bf16_exact(dkv[:, C:])


@pytest.mark.parametrize("case", T.LN_CASES, ids=[c.id for c in T.LN_CASES])
def test_layernorm_db_precondition(case):
    d = I.ln_db(case, "f32")
    assert case.ntok * 3 + 3 < EXACT
    assert torch.equal(d["dy"].sum(0).double(), d["dy"].double().sum(0))
    assert _bf16_exact(d["dy"])


@pytest.mark.parametrize("case", T.CM_CASES, ids=[c.id for c in T.CM_CASES])
def test_channel_mean_precondition(case):
    d = I.channel_mean(case, "f32")
    assert case.HW * 9 < EXACT
    for x2 in (None, d["x2"]):
        s32 = R.channel_mean(d["x"], x2, 1.0)
        assert torch.equal(s32.double(), R.channel_mean(d["x"].double(), None if x2 is None else x2.double(), 1.0))
    assert _bf16_exact(d["x"]) and _bf16_exact(d["x2"])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_channel_affine_precondition(dtype):
    for B in T.AFFINE_B:
        d = I.channel_affine(B, T.AFFINE_HW, 16, dtype, "vec")
        for bs in T.AFFINE_BETA_SCALE:
            for ga, be in ((d["gamma"], d["beta"]), (None, d["beta"]), (d["gamma"], None)):
                y32 = R.channel_affine(d["x"], ga, be, bs, T.AFFINE_HW)
                y64 = R.channel_affine(d["x"].double(), None if ga is None else ga.double(),
                                       None if be is None else be.double(), bs, T.AFFINE_HW)
                assert torch.equal(y32.double(), y64)
                assert dtype == "f32" or _bf16_exact(y64)
