"""On the CPU: (1) the fp64 restatement of GDN / IGDN (gdn_reference.py) equals the oracle's GDN module under
autograd, parameter gradients through the parametrizer included, so the GPU tests' reference is not wrong in the
kernels' way; (2) the case tables reach every kernel and launch shape they name, with the kernel names read back
from the built library; (3) the preconditions of the exact cases hold on the reference alone: the norm lattice,
sum |terms| below 2^24 units, the share of near-ties; (4) each reference mutant changes at least 16 stored bf16
values of every case it applies to.  No kernel is launched.
"""
import os

import pytest
import torch

import gdn_reference as R

SMALL_CASES = [(dt, C, n) for dt in ("f32", "bf16") for C in R.C_OF[dt] for n in R.SMALL_NPIX]
BIG_FWD = R.FWD_MULTI + R.FWD_LANE


# ---- (1) restatement == oracle, fp64 --------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("C", [32, 96])
def test_reference_equals_oracle(C, inverse):
    import cai_oracle as O

    g = torch.Generator().manual_seed(11 + C + inverse)
    m = O.GDN(C, inverse=inverse).double()
    bb, gb = m.beta_reparam.lower_bound.bound.item(), m.gamma_reparam.lower_bound.bound.item()
    ped = m.gamma_reparam.pedestal.item()
    assert gb == R.GBOUND and ped == R.PED and abs(bb - R.BBOUND) <= 2.0 ** -33     # one fp32 ulp of 1e-3
    with torch.no_grad():
        # raws on both sides of the bounds, so the gate decides: a fifth of gamma's and a quarter of beta's below
        graw = torch.sqrt(0.1 * torch.eye(C) + 0.02 * torch.rand(C, C, generator=g) + ped).double()
        graw[torch.rand(C, C, generator=g) < 0.2] = -0.5 * gb
        braw = torch.sqrt(1.0 + 0.1 * torch.rand(C, generator=g)).double()
        braw[torch.rand(C, generator=g) < 0.25] = 0.5 * bb
        m.gamma.copy_(graw)
        m.beta.copy_(braw)
    B, H, W = 2, 5, 7
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    y = m(x)
    dx, dbraw, dgraw = torch.autograd.grad(y, (x, m.beta, m.gamma), dy)
    rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, C)
    gamma, beta = R.reparam(graw, gb, ped), R.reparam(braw, bb, ped)
    ref = R.reference(rows(x), rows(dy), gamma, beta, inverse)
    got = dict(y=ref["y"], dx=ref["dx"], dbeta_raw=R.gate(braw, bb, ref["dbeta"]), dgamma_raw=R.gate(graw, gb, ref["dgamma"]))
    want = dict(y=rows(y), dx=rows(dx), dbeta_raw=dbraw, dgamma_raw=dgraw)
    for k in got:
        assert (got[k] - want[k]).abs().max().item() <= 1e-12, k
    assert bool((got["dgamma_raw"] == 0).any()) and bool((got["dbeta_raw"] == 0).any()), "the gate closed nowhere"
    # the scales are sums of the absolute values of the same terms
    assert bool((ref["s_dx"] >= ref["dx"].abs() - 1e-12).all()) and bool((ref["s_dgamma"] >= ref["dgamma"].abs() - 1e-12).all())
    assert bool((ref["s_dbeta"] >= ref["dbeta"].abs() - 1e-12).all())


def test_gdn1_equals_autograd():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(40, 12, generator=g, dtype=torch.float64, requires_grad=True)
    n = (1.0 + torch.rand(40, 12, generator=g, dtype=torch.float64)).requires_grad_()
    gy = torch.randn(40, 12, generator=g, dtype=torch.float64)
    for inverse in (False, True):
        y = x * n if inverse else x / n
        dx, dn = torch.autograd.grad(y, (x, n), gy)
        got = R.gdn1(x.detach(), n.detach(), gy, inverse)
        for a, b in zip(got, (y.detach(), dx, dn)):
            assert (a - b).abs().max().item() <= 1e-12


def test_bf16_neighbours_round_like_torch():
    g = torch.Generator().manual_seed(9)
    v = torch.randn(20000, generator=g, dtype=torch.float64) * torch.exp(4 * torch.randn(20000, generator=g, dtype=torch.float64))
    v = torch.cat([v, torch.tensor([0.0, 1.0, -1.0, 1.00390625, 1.01171875, 0.998046875, 255.5, 3.0 * 2.0 ** -130])])
    rne, lo, hi, near = R.bf16_neighbours(v)
    assert torch.equal(rne, v.float().bfloat16().double())         # (random fp64 values are not fp32 ties)
    assert bool((lo.abs() <= v.abs()).all()) and bool((v.abs() <= hi.abs()).all())
    assert near[-5].item() and near[-4].item() and not near[-8].item()       # the two ties; 0 is not
    assert rne[-5].item() == 1.0 and rne[-4].item() == 1.015625    # ties go to even
    assert near.float().mean().item() < 1e-3


# ---- (2) the tables reach every kernel and launch shape ------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from compressai import _native

    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libcai.so not built")
    _native.lib.load()
    return _native


def _lane_env(on):
    os.environ["CAI_GDN_LANE"] = "1" if on else "0"


def test_kernel_names_match_the_library(native):
    lib = native.lib.load()
    code = {"f32": native.F32, "bf16": native.BF16}
    old = os.environ.get("CAI_GDN_LANE")
    try:
        for lane in (True, False):
            _lane_env(lane)
            for dt in ("f32", "bf16"):
                for C in R.C_OF[dt]:
                    for n in R.SMALL_NPIX + (64 * 257 + 3, 32768, 32768 + 197, 65549, 65605):
                        assert lib.cai_gdn_kernel_name(code[dt], n, C, C + 8, C + 24, 0).decode() == R.fwd_kernel(dt, n, C, lane)
                        assert lib.cai_gdn_kernel_name(code[dt], n, C, C + 8, C + 24, 1).decode() == R.bwd_kernel(dt, n, C, lane)
                        nb = R.bwd_blocks(dt, n, C, lane)
                        if nb:
                            assert lib.cai_gdn_backward_workspace_bytes(n, C, code[dt]) >= nb * (C * C + C) * 4
    finally:
        if old is None:
            del os.environ["CAI_GDN_LANE"]
        else:
            os.environ["CAI_GDN_LANE"] = old


def test_tables_reach_every_launch_shape():
    seen = {}
    for c in R.FWD_MULTI:
        assert R.fwd_kernel(c.dt, c.npix, c.C, c.lane) == f"gdn_fwd_kernel<{c.C}>", c.id
        grid, pair, first, last = R.fwd_tile_launch(c.dt, c.npix, c.C)
        seen[c.id] = (c.dt, pair, first, last)
        assert first > last >= 1 and c.npix % R.GBM, c.id                   # both tile counts, a ragged last tile
    v = set(seen.values())
    assert ("f32", True, 3, 2) in v and ("bf16", True, 3, 2) in v, "PAIR: one pair and the odd tail, and one pair"
    assert ("f32", False, 3, 2) in v and ("bf16", False, 3, 2) in v, "the single-set loop"
    assert seen["bf16_c224_occ1"] == ("bf16", False, 2, 1)
    assert {c.C for c in R.FWD_MULTI if c.dt == "f32" and seen[c.id][1]} == {32, 64}
    for dt in ("f32", "bf16"):
        for C in R.C_OF[dt]:
            for n in R.SMALL_NPIX:
                assert R.fwd_tile_launch(dt, n, C)[2:] == (1, 1)
    for c in R.FWD_LANE:
        assert R.fwd_kernel(c.dt, c.npix, c.C) == f"gdn_fwd_lane_kernel<{c.C}>", c.id
    assert {c.C for c in R.FWD_LANE} == {64, 128, 192} and any(c.npix % 16 for c in R.FWD_LANE)
    for dt, C in R.BWD_TWO_PASS:
        assert R.bwd_kernel(dt, 130, C) == f"gdn_bwd_kernel+param_grad<{C}>"
    assert {C for dt, C in R.BWD_TWO_PASS if dt == "f32"} == set(R.C_OF["f32"])
    for c in R.BWD_FUSED_BIG:
        name = "gdn_bwd_wide_kernel" if c.C >= 160 else "gdn_bwd_fused_kernel"
        assert R.bwd_kernel(c.dt, c.npix, c.C) == f"{name}<{c.C}>" and R.bwd_blocks(c.dt, c.npix, c.C) == 256
        assert (c.npix + 63) // 64 == 258 and c.npix < R.LANE_MIN_NPIX      # blocks 0 and 1 on two tiles
        assert len(R.sparse_rows(c.npix, c.dt, c.C)) == 4
    for c in R.BWD_LANE:
        assert R.bwd_kernel(c.dt, c.npix, c.C) == f"gdn_bwd_lane_kernel<{c.C}>" and R.bwd_blocks(c.dt, c.npix, c.C) == 256
    steps = sorted({(c.npix + 63) // 64 for c in R.BWD_LANE})
    assert steps == [512, 516] and any(c.npix % 64 for c in R.BWD_LANE)       # 2 steps each; 3 in blocks 0-3, ragged end
    assert {p for d in R.PADS for p in d.values()} == {0, 8, 24}
    assert all(len({d["x"], d["dy"], d["dx"]}) == 3 and d["x"] != d["y"] for d in R.PADS)


def test_gate_raws_cover_both_sides():
    for bound in (R.GBOUND, R.BBOUND):
        r = R.gate_raws((64, 64), bound)
        b = torch.tensor(bound)
        for want in (torch.nextafter(b, torch.tensor(0.0)), b, torch.nextafter(b, torch.tensor(2.0)), torch.tensor(0.0)):
            assert bool((r == want).any())
        assert bool((r < 0).any()) and bool((r > 2 * b).any()) and bool(((r > 0) & (r < 0.75 * b)).any())
        assert len({tuple(row.tolist()) for row in r[:9]}) == 9            # rows differ: a transposed index shows


# ---- (3) preconditions of the exact cases ---------------------------------------------------------------------------
def _a1_check(name, dt, C, npix):
    x, gamma, beta = R.a1_operands(name, npix, C)
    assert R.a1_norm_units(x, gamma, beta) < R.EXACT
    for t in (x, x * x, gamma, beta):
        assert torch.equal(t.bfloat16().float(), t)
    ref = {inv: R.reference(x, None, gamma, beta, inv) for inv in (False, True)}
    n64 = ref[False]["norm"]
    assert torch.equal((n64 * 64).round(), n64 * 64)
    # fp32 in any order: the restatement's fp32 matmul gives the fp64 norm
    assert torch.equal(((x * x) @ gamma.t() + beta).double(), n64)
    shares = []
    for inv in (False, True):
        near = R.bf16_neighbours(ref[inv]["y"])[3]
        shares.append(near.float().mean().item())
        assert shares[-1] <= 0.01, (name, inv, shares[-1])
    return x, gamma, beta, ref, max(shares)


@pytest.mark.parametrize("dt,C", [(dt, C) for dt in ("f32", "bf16") for C in R.C_OF[dt]])
def test_a1_lattice_small(dt, C):
    """Every norm a multiple of 1 / 64 below 2^24 units, near-ties within 1 %; each mutant changes >= 16 stored bf16
    values of every case from 63 pixels up (a 1-pixel case holds C values in all: there the fp32 run decides)."""
    for npix in R.SMALL_NPIX:
        name = f"{dt}-c{C}-n{npix}"
        x, gamma, beta, ref, share = _a1_check(name, dt, C, npix)
        if npix < 63:
            continue
        for inv in (False, True):
            good = R.bf16_neighbours(ref[inv]["y"])[0]
            for kind in R.MUTANTS:
                if R.mutant_applies(kind, npix, C):
                    bad = R.bf16_neighbours(R.forward_mutant(kind, x, gamma, beta, inv, dt))[0]
                    changed = int(((bad != good) | torch.isnan(bad)).sum())
                    assert changed >= 16, (name, inv, kind, changed)


@pytest.mark.parametrize("case", BIG_FWD, ids=[c.id for c in BIG_FWD])
def test_a1_lattice_big(case):
    x, gamma, beta, ref, share = _a1_check(case.id, case.dt, case.C, case.npix)
    print(f"{case.id}: near-tie share {share:.5f}")
    good = R.bf16_neighbours(ref[False]["y"])[0]
    for kind in R.MUTANTS:
        if R.mutant_applies(kind, case.npix, case.C):
            bad = R.bf16_neighbours(R.forward_mutant(kind, x, gamma, beta, False, case.dt))[0]
            assert int(((bad != good) | torch.isnan(bad)).sum()) >= 16, (case.id, kind)


A2_SHAPES = sorted({(C, n) for C in (32, 256) for n in R.SMALL_NPIX} | {(c.C, c.npix) for c in R.BWD_FUSED_BIG + R.BWD_LANE})


@pytest.mark.parametrize("C,npix", A2_SHAPES)
def test_a2_reductions_are_exact(C, npix):
    """norm = 1: u = -+ g x / 2, dx = g, and dgamma / dbeta are sums of half-integers whose sum of |terms| (plus the
    integer prefill) stays below 2^24 half-units: any fp32 order and grouping gives the same bits."""
    x, g = R.a2_operands(f"c{C}-n{npix}", npix, C)
    gamma, beta = torch.zeros(C, C), torch.ones(C)
    for inv in (False, True):
        ref = R.reference(x, g, gamma, beta, inv)
        assert torch.equal(ref["u"], (0.5 if inv else -0.5) * g.double() * x.double())
        assert torch.equal(ref["dx"], g.double()) and torch.equal(ref["y"], x.double())
        for t in (ref["u"], x * x, g, x):
            assert torch.equal(t.float().bfloat16().double(), t.double())
        for k in ("dgamma", "dbeta"):
            assert torch.equal((2 * ref[k]).round(), 2 * ref[k])
            assert 2 * (ref["s_" + k].max().item() + 5) < R.EXACT
        m = R.model(x, g, gamma, beta, inv, "bf16", False)
        assert torch.equal(m["dgamma"].double(), ref["dgamma"]) and torch.equal(m["dbeta"].double(), ref["dbeta"])
    db0, dg0 = R.a2_prefill(f"c{C}", C)
    assert torch.equal(db0.round(), db0) and db0.abs().max() <= 5 and dg0.abs().max() <= 5
    # raw = 0.5 >= both bounds: d_raw = (2 * 0.5) * d_param exactly
    assert 0.5 >= R.BBOUND and 0.5 >= R.GBOUND
    d = ref["dgamma"].float()
    assert torch.equal(R.gate(torch.full((C, C), 0.5), R.GBOUND, d), d)


def test_signed_operands_make_sign_definite_gradients():
    for sign in (1, -1):
        x, g = R.signed_operands("t", 65, 32, sign)
        assert bool((torch.sign(g * x) == sign).all())
        for inv in (False, True):
            ref = R.reference(x, g, torch.zeros(32, 32), torch.ones(32), inv)
            want = sign if inv else -sign
            assert bool((torch.sign(ref["dgamma"]) == want).all()) and bool((torch.sign(ref["dbeta"]) == want).all())
