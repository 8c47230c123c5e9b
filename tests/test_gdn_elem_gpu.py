"""Every kernel of csrc/gdn.hip and csrc/gdn_lane.hip, and the gdn1 kernels of csrc/elementwise.hip, called through
the C ABI and compared per element with the fp64 restatement of gdn_reference.py, run on the CPU on the operands
exactly as the kernel holds them.  The kernels take beta and gamma_op = [gamma | gamma^T] as buffers, so every case
chooses them freely.  test_gdn_reference_cpu.py proves the restatement against the oracle and the preconditions of
the exact cases.  Every call first asserts, with cai_gdn_kernel_name, that it reaches the kernel the case declares.

Exact cases
  A1  forward on a lattice where every norm is a multiple of 1 / 64 far below 2^24 units: any fp32 summation order
      gives the same norm, what remains is rsqrtf (within 2 ulp), nv * rs for the inverse and the final product.
      fp32: |y - ref| <= 2^-21 |ref| per element (a reasoned bar, not a measured one); bf16: y == RNE_bf16(ref) by
      bits, either neighbour where ref lies within 2^-20 relative of a tie; x == 0 gives +-0 by bits.
  A2  gamma_op = 0, beta = 1 (norm == 1), g and x on {0, +-1, +-2, +-3}, raws 0.5: dx == g and the raw gradients
      are sums of half-integers, bit-equal over every backward kernel and block count, immediate and deferred,
      overwriting and accumulating onto an integer prefill.  Needs rsqrtf(1) == sqrtf(1) == 1: the forward on the
      same operands shows it (y == x by bits).
  A3  dy zero except at chosen pixels: dx rows of the other pixels are +-0 by bits; dgamma / dbeta under bar C.
  A4  cai_gdn_reparam around the bound and the LowerBound gate with sign-definite gradients.
Tolerance cases (C): x, dy ~ N(0, 1), gamma = 0.1 I + 0.02 U, beta = 1 + 0.1 U.  Per element e = |kernel - ref64| / s
with s the element's own sum of |terms| (gdn_reference.reference); the case's error is the maximum, and
e_kernel <= 4 * e_ref where e_ref is the same measure of gdn_reference.model (a correct CPU implementation at the
kernel's declared precision), never taken from the kernel.  Every tensor prints a "BAR ..." line.

Outputs live in sentinel-guarded, NaN-prefilled buffers (Out of test_conv_exact_gpu.py); the pitch columns of the
inputs and four rows behind the last pixel hold NaN; workspaces hold NaN bit patterns.
"""
import contextlib
import ctypes
import os

import pytest
import torch

import gdn_reference as R
from test_conv_exact_gpu import Env, Out, assert_bits

pytestmark = pytest.mark.gpu

MARGIN = 4.0
NAN = float("nan")
TORCH_DT = R.TORCH_DT


@pytest.fixture(scope="module")
def env(cuda):
    return Env(cuda)


def code(env, dt):
    return env.native.BF16 if dt == "bf16" else env.native.F32


@contextlib.contextmanager
def lane_knob(on):
    """CAI_GDN_LANE is read at every call."""
    old = os.environ.get("CAI_GDN_LANE")
    os.environ["CAI_GDN_LANE"] = "1" if on else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["CAI_GDN_LANE"]
        else:
            os.environ["CAI_GDN_LANE"] = old


class In:
    """[n][C] fp32 CPU values as device rows at pitch ld; the pitch columns and four rows behind the last hold NaN."""

    def __init__(self, t, ld, dt, dev):
        n, C = t.shape
        assert ld >= C
        buf = torch.full((n + 4, ld), NAN)
        buf[:n, :C] = t
        self.buf = buf.to(TORCH_DT[dt]).to(dev)
        self.ld = ld
        self.ptr = ctypes.c_void_p(self.buf.data_ptr())


def rows_out(n, C, ld, dt, dev, prefill=None):
    return Out((n, C), (ld, 1), TORCH_DT[dt], dev, prefill)


def f32_out(shape, dev, prefill=None):
    strides = (shape[1], 1) if len(shape) == 2 else (1,)
    return Out(shape, strides, torch.float32, dev, prefill)


class Params:
    """beta and gamma_op as the kernels take them, and the raws the gate reads (0.5: above both bounds, and
    d_raw = (2 * 0.5) * d_param exactly)."""

    def __init__(self, env, dt, gamma, beta, braw=None, graw=None):
        C = beta.numel()
        self.gamma, self.beta_cpu = gamma, beta
        self.gop = torch.cat([gamma.reshape(-1), gamma.t().reshape(-1)]).to(TORCH_DT[dt]).to(env.dev)
        self.beta = beta.float().to(env.dev)
        self.braw_cpu = torch.full((C,), 0.5) if braw is None else braw
        self.graw_cpu = torch.full((C, C), 0.5) if graw is None else graw
        self.braw, self.graw = self.braw_cpu.to(env.dev), self.graw_cpu.contiguous().to(env.dev)


def run_fwd(env, dt, x, P, inverse, pads, kernel, lane=True):
    dev, lib = env.dev, env.lib
    npix, C = x.shape
    xd = In(x, C + pads["x"], dt, dev)
    y_ld = C + pads["y"]
    y = rows_out(npix, C, y_ld, dt, dev)
    with lane_knob(lane):
        name = lib.cai_gdn_kernel_name(code(env, dt), npix, C, xd.ld, y_ld, 0).decode()
        assert name == kernel, (name, kernel)
        lib.cai_gdn_fwd(code(env, dt), xd.ptr, xd.ld, npix, C, env.p(P.gop), env.p(P.beta), int(inverse), y.ptr, y_ld,
                        env.stream())
    torch.cuda.synchronize()
    return y.take(f"gdn_fwd {kernel} npix {npix} {dt}").cpu()


def run_backward(env, dt, x, dy, P, inverse, pads, kernel, accumulate=0, prefill=None, deferred=False, lane=True):
    """cai_gdn_backward, or cai_gdn_backward_deferred followed by cai_reduce_jobs -> dx, dbeta_raw, dgamma_raw."""
    dev, lib, native = env.dev, env.lib, env.native
    npix, C = x.shape
    xd, gd = In(x, C + pads["x"], dt, dev), In(dy, C + pads["dy"], dt, dev)
    dx_ld = C + pads["dx"]
    dx = rows_out(npix, C, dx_ld, dt, dev)
    dbr = f32_out((C,), dev, prefill[0] if accumulate else None)
    dgr = f32_out((C, C), dev, prefill[1] if accumulate else None)
    with lane_knob(lane):
        name = lib.cai_gdn_kernel_name(code(env, dt), npix, C, max(xd.ld, gd.ld), dx_ld, 1).decode()
        assert name == kernel, (name, kernel)
        ws, wsb = env.ws(lib.cai_gdn_backward_workspace_bytes(npix, C, code(env, dt)))
        args = (code(env, dt), xd.ptr, xd.ld, gd.ptr, gd.ld, npix, C, env.p(P.gop), env.p(P.beta), int(inverse), dx.ptr,
                dx_ld, env.p(P.braw), env.p(P.graw), R.BETA_MIN, R.OFF, dbr.ptr, dgr.ptr, accumulate, env.p(ws), wsb,
                env.stream())
        if deferred:
            job = native.ReduceJob()
            lib.cai_gdn_backward_deferred(*args, ctypes.byref(job))
            fused = not kernel.startswith("gdn_bwd_kernel")
            assert (job.kind == 2 and job.nblocks > 0) if fused else job.kind == 0      # CAI_JOB_GDN / none left to run
            lib.cai_reduce_jobs((native.ReduceJob * 1)(job), 1, env.stream())
        else:
            lib.cai_gdn_backward(*args)
    torch.cuda.synchronize()
    what = f"gdn_backward {kernel} npix {npix} {dt}"
    return dx.take(what).cpu(), dbr.take(what).cpu(), dgr.take(what).cpu()


def run_two_kernels(env, dt, x, dy, P, inverse, pads):
    """cai_gdn_bwd then cai_gdn_param_grad, each on its own -> dx, u, dbeta_raw, dgamma_raw."""
    dev, lib = env.dev, env.lib
    npix, C = x.shape
    xd, gd = In(x, C + pads["x"], dt, dev), In(dy, C + pads["dy"], dt, dev)
    dx_ld = C + pads["dx"]
    dx, u = rows_out(npix, C, dx_ld, dt, dev), rows_out(npix, C, C, dt, dev)
    name = lib.cai_gdn_kernel_name(code(env, dt), npix, C, max(xd.ld, gd.ld), dx_ld, 1).decode()
    assert name == f"gdn_bwd_kernel+param_grad<{C}>", name       # the pair cai_gdn_backward runs for these arguments
    lib.cai_gdn_bwd(code(env, dt), xd.ptr, xd.ld, gd.ptr, gd.ld, npix, C, env.p(P.gop), env.p(P.beta), int(inverse),
                    dx.ptr, dx_ld, u.ptr, env.stream())
    dbr, dgr = f32_out((C,), dev), f32_out((C, C), dev)
    ws, wsb = env.ws(lib.cai_gdn_param_grad_workspace_bytes(npix, C, code(env, dt)))
    lib.cai_gdn_param_grad(code(env, dt), xd.ptr, xd.ld, u.ptr, npix, C, env.p(P.braw), env.p(P.graw), R.BETA_MIN, R.OFF,
                           dbr.ptr, dgr.ptr, 0, env.p(ws), wsb, env.stream())
    torch.cuda.synchronize()
    what = f"gdn_bwd + gdn_param_grad npix {npix} C {C} {dt}"
    return dx.take(what).cpu(), u.take(what).cpu(), dbr.take(what).cpu(), dgr.take(what).cpu()


def bar(kernel, case, tensor, got, ref, s, mod):
    e, e_ref = R.elem_error(got, ref, s), R.elem_error(mod, ref, s)
    print(f"\nBAR {kernel} {case} {tensor} e_kernel {e:.3e} e_ref {e_ref:.3e} ratio {e / e_ref if e_ref else 0.0:.2f}")
    assert e <= MARGIN * e_ref, (kernel, case, tensor, e, e_ref)


def signless_zero(t):
    bits = t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    return bool(((bits & (0x7FFF if t.dtype == torch.bfloat16 else 0x7FFFFFFF)) == 0).all())


# ---- forward ----------------------------------------------------------------------------------------------------------
def check_a1(what, dt, y, x, ref):
    yd = y.double()
    if dt == "f32":
        bad = ~((yd - ref).abs() <= 2.0 ** -21 * ref.abs())
    else:
        rne, lo, hi, near = R.bf16_neighbours(ref)
        bad = ~((yd == rne) | (near & ((yd == lo) | (yd == hi))))
    n = int(bad.sum())
    if n:
        i = tuple(bad.nonzero()[0].tolist())
        pytest.fail(f"{what}: {n} of {bad.numel()} elements off the lattice bar; first {i}: got {yd[i].item()!r} "
                    f"want {ref[i].item()!r}")
    assert signless_zero(y[x == 0]), f"{what}: x == 0 did not give +-0"


def forward_case(env, name, dt, C, npix, pads, kernel, lane=True):
    for inverse in (False, True):
        tag = f"{name}-{'igdn' if inverse else 'gdn'}"
        x, gamma, beta = R.a1_operands(name, npix, C)
        y = run_fwd(env, dt, x, Params(env, dt, gamma, beta), inverse, pads, kernel, lane)
        check_a1(f"A1 {tag}", dt, y, x, R.reference(x, None, gamma, beta, inverse)["y"])
        x, _, gamma, beta = R.tol_operands(name, npix, C, dt)
        y = run_fwd(env, dt, x, Params(env, dt, gamma, beta), inverse, pads, kernel, lane)
        ref = R.reference(x, None, gamma, beta, inverse)
        bar(kernel, tag, "y", y, ref["y"], ref["s_y"], R.model(x, None, gamma, beta, inverse, dt, False)["y"])


ALL_C = [(dt, C) for dt in ("f32", "bf16") for C in R.C_OF[dt]]


@pytest.mark.parametrize("dt,C", ALL_C, ids=[f"{d}-c{c}" for d, c in ALL_C])
def test_forward_one_tile(env, dt, C):
    """Every instantiation of gdn_fwd_kernel at 1, 63, 64, 65 and 130 pixels, x and y at different pitches."""
    for i, npix in enumerate(R.SMALL_NPIX):
        forward_case(env, f"{dt}-c{C}-n{npix}", dt, C, npix, R.PADS[i % 3], f"gdn_fwd_kernel<{C}>")


@pytest.mark.parametrize("case", R.FWD_MULTI, ids=[c.id for c in R.FWD_MULTI])
def test_forward_tile_kernel_above_one_tile(env, case):
    """Blocks of two and three tiles: the PAIR loop with its odd tail and the single-register-set loop, fp32 and bf16
    (the latter with CAI_GDN_LANE=0 where the lane kernel would take the call)."""
    forward_case(env, case.id, case.dt, case.C, case.npix, R.PADS[case.pads], f"gdn_fwd_kernel<{case.C}>", case.lane)


@pytest.mark.parametrize("case", R.FWD_LANE, ids=[c.id for c in R.FWD_LANE])
def test_forward_lane(env, case):
    pads = R.FWD_LANE_LD32 if case.pads is None else R.PADS[case.pads]
    forward_case(env, case.id, case.dt, case.C, case.npix, pads, f"gdn_fwd_lane_kernel<{case.C}>")


# ---- backward ---------------------------------------------------------------------------------------------------------
def a2_case(env, name, dt, C, npix, pads, kernel, fwd_too):
    """norm == 1: dx == g, the raw gradients bit-equal, immediate / deferred x overwrite / accumulate."""
    x, g = R.a2_operands(f"c{C}-n{npix}", npix, C)
    P = Params(env, dt, torch.zeros(C, C), torch.ones(C))
    pre = R.a2_prefill(f"c{C}", C)
    tdt = TORCH_DT[dt]
    for inverse in (False, True):
        tag = f"A2 {name} {'igdn' if inverse else 'gdn'}"
        if fwd_too:          # rsqrtf(1) == 1 and sqrtf(1) == 1 on this device: y == x by bits
            y = run_fwd(env, dt, x, P, inverse, pads, R.fwd_kernel(dt, npix, C))
            assert_bits(y, x.to(tdt), f"{tag}: forward with norm == 1")
        ref = R.reference(x, g, P.gamma, P.beta_cpu, inverse)
        for deferred in (False, True):
            for acc in (0, 1):
                dx, dbr, dgr = run_backward(env, dt, x, g, P, inverse, pads, kernel, acc, pre, deferred)
                what = f"{tag} deferred {deferred} accumulate {acc}"
                assert_bits(dx, g.to(tdt), f"{what}: dx")
                assert_bits(dbr, ref["dbeta"].float() + (pre[0] if acc else 0), f"{what}: dbeta_raw")
                assert_bits(dgr, ref["dgamma"].float() + (pre[1] if acc else 0), f"{what}: dgamma_raw")


def tol_case(env, name, dt, C, npix, pads, kernel, two_pass):
    """Random operands under bar C, and the same with a sparse dy (A3)."""
    tdt = TORCH_DT[dt]
    for inverse in (False, True):
        tag = f"{name}-{'igdn' if inverse else 'gdn'}"
        x, dy, gamma, beta = R.tol_operands(name, npix, C, dt)
        P = Params(env, dt, gamma, beta)
        rows = R.sparse_rows(npix, dt, C)
        sp = torch.zeros_like(dy)
        sp[rows] = dy[rows]
        for kind, g in (("", dy), ("-sparse", sp)):
            ref = R.reference(x, g, gamma, beta, inverse)
            mod = R.model(x, g, gamma, beta, inverse, dt, two_pass)
            dx, dbr, dgr = run_backward(env, dt, x, g, P, inverse, pads, kernel)
            bar(kernel, tag + kind, "dx", dx, ref["dx"], ref["s_dx"], mod["dx"])
            bar(kernel, tag + kind, "dgamma", dgr, ref["dgamma"], ref["s_dgamma"], mod["dgamma"])
            bar(kernel, tag + kind, "dbeta", dbr, ref["dbeta"], ref["s_dbeta"], mod["dbeta"])
            if kind:
                quiet = torch.ones(npix, dtype=torch.bool)
                quiet[rows] = False
                assert signless_zero(dx[quiet]), f"{tag}: dx of a pixel with dy == 0 is not +-0"
        if two_pass:
            ref = R.reference(x, dy, gamma, beta, inverse)
            mod = R.model(x, dy, gamma, beta, inverse, dt, True)
            dx, u, dbr, dgr = run_two_kernels(env, dt, x, dy, P, inverse, pads)
            bar("gdn_bwd_kernel", tag, "dx", dx, ref["dx"], ref["s_dx"], mod["dx"])
            bar("gdn_bwd_kernel", tag, "u", u, ref["u"], ref["s_u"], mod["u"].to(tdt))
            bar("gdn_param_grad", tag, "dgamma", dgr, ref["dgamma"], ref["s_dgamma"], mod["dgamma"])
            bar("gdn_param_grad", tag, "dbeta", dbr, ref["dbeta"], ref["s_dbeta"], mod["dbeta"])


@pytest.mark.parametrize("dt,C", R.BWD_TWO_PASS, ids=[f"{d}-c{c}" for d, c in R.BWD_TWO_PASS])
def test_backward_two_pass(env, dt, C):
    """gdn_bwd_kernel + cai_gdn_param_grad (cai_conv_wgrad's split-K GEMM and gdn_reparam_bwd_kernel): through
    cai_gdn_backward and each entry point on its own, u compared as well."""
    kernel = f"gdn_bwd_kernel+param_grad<{C}>"
    for i, npix in enumerate(R.SMALL_NPIX):
        name = f"{dt}-c{C}-n{npix}"
        a2_case(env, name, dt, C, npix, R.PADS[i % 3], kernel, fwd_too=i == 4)
        tol_case(env, name, dt, C, npix, R.PADS[i % 3], kernel, True)


@pytest.mark.parametrize("case", R.BWD_TWO_PASS_BIG, ids=[c.id for c in R.BWD_TWO_PASS_BIG])
def test_backward_two_pass_258_tiles(env, case):
    kernel = f"gdn_bwd_kernel+param_grad<{case.C}>"
    a2_case(env, case.id, case.dt, case.C, case.npix, R.PADS[case.pads], kernel, False)
    tol_case(env, case.id, case.dt, case.C, case.npix, R.PADS[case.pads], kernel, True)


def _fused_name(C):
    return f"{'gdn_bwd_wide_kernel' if C >= 160 else 'gdn_bwd_fused_kernel'}<{C}>"


@pytest.mark.parametrize("C", R.BWD_FUSED_C)
def test_backward_fused_and_wide_small(env, C):
    """One to three blocks of one tile each (the wide kernel: 32-pixel tiles, up to two per block)."""
    for i, npix in enumerate(R.SMALL_NPIX):
        name = f"bf16-c{C}-n{npix}"
        a2_case(env, name, "bf16", C, npix, R.PADS[i % 3], _fused_name(C), fwd_too=i == 4)
        tol_case(env, name, "bf16", C, npix, R.PADS[i % 3], _fused_name(C), False)


@pytest.mark.parametrize("case", R.BWD_FUSED_BIG, ids=[c.id for c in R.BWD_FUSED_BIG])
def test_backward_fused_and_wide_256_blocks(env, case):
    """258 tiles on 256 blocks, below the lane threshold: blocks 0 and 1 take a second tile, the last one is ragged;
    the reduce job sums 256 partials."""
    a2_case(env, case.id, case.dt, case.C, case.npix, R.PADS[case.pads], _fused_name(case.C), False)
    tol_case(env, case.id, case.dt, case.C, case.npix, R.PADS[case.pads], _fused_name(case.C), False)


@pytest.mark.parametrize("case", R.BWD_LANE, ids=[c.id for c in R.BWD_LANE])
def test_backward_lane(env, case):
    """256 blocks of two 64-pixel steps, and 516 steps: three in blocks 0-3 and a ragged end."""
    kernel = f"gdn_bwd_lane_kernel<{case.C}>"
    a2_case(env, case.id, case.dt, case.C, case.npix, R.PADS[case.pads], kernel, False)
    tol_case(env, case.id, case.dt, case.C, case.npix, R.PADS[case.pads], kernel, False)


# ---- A4: the reparametrisation and its gate ---------------------------------------------------------------------------------
def _f32_ulp(v):
    _, e = torch.frexp(v.abs())
    return torch.ldexp(torch.ones_like(v), e - 24)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C", R.REPARAM_C)
def test_reparam_around_the_bound(env, C, dt):
    """max(raw, bound)^2 - ped with raws below, one ulp below, at, one ulp above and above the bound, 0 and negative.
    The kernel's lb * lb - ped may or may not be contracted to an FMA: the unfused form rounds lb^2 (half an ulp of
    lb^2) and then the difference (at most half an ulp of lb^2 again), so the fp32 result lies within one fp32 ulp
    of lb^2 of the fp64 value; the bf16 result is the rounding of some fp32 value in that interval (rounding is
    monotone).  The transposed half is bit-equal to the transpose of the first."""
    dev, lib = env.dev, env.lib
    graw, braw = R.gate_raws((C, C), R.GBOUND), R.gate_raws((C,), R.BBOUND)
    gd, bd = graw.to(dev), braw.to(dev)
    beta = f32_out((C,), dev)
    gop = Out((2 * C * C,), (1,), TORCH_DT[dt], dev)
    lib.cai_gdn_reparam(env.p(bd), env.p(gd), C, R.BETA_MIN, R.OFF, code(env, dt), beta.ptr, gop.ptr, env.stream())
    torch.cuda.synchronize()
    beta, gop = beta.take("reparam beta").cpu(), gop.take("reparam gamma_op").cpu()
    gam, gam_t = gop[:C * C].view(C, C), gop[C * C:].view(C, C)
    assert_bits(gam_t, gam.t().contiguous(), "gamma^T half")
    for name, got, raw, bound, out_dt in (("beta", beta, braw, R.BBOUND, "f32"), ("gamma", gam, graw, R.GBOUND, dt)):
        ref = R.reparam(raw, bound)
        ulp = _f32_ulp(torch.clamp(raw.double(), min=bound) ** 2)
        if out_dt == "f32":
            assert bool(((got.double() - ref).abs() <= ulp).all()), name
        else:
            lo, hi = R.bf16_neighbours(ref - ulp)[0], R.bf16_neighbours(ref + ulp)[0]
            assert bool(((lo <= got.double()) & (got.double() <= hi)).all()), name
        closed = raw <= bound
        want0 = bound * bound - R.PED            # every raw at or below the bound gives the bound's own value
        assert bool(((got.double()[closed] - want0).abs() <= ulp[closed]).all()) and closed.any() and (~closed).any()


GATE_PATHS = [("bf16", 64, "gdn_bwd_fused_kernel<64>"), ("bf16", 160, "gdn_bwd_wide_kernel<160>"),
              ("bf16", 32, "gdn_bwd_kernel+param_grad<32>"), ("f32", 32, "gdn_bwd_kernel+param_grad<32>")]


@pytest.mark.parametrize("dt,C,kernel", GATE_PATHS, ids=[f"{d}-c{c}" for d, c, _ in GATE_PATHS])
def test_lowerbound_gate(env, dt, C, kernel):
    """d_raw = (raw >= bound or d < 0) ? d : 0 through the reduce job (fused, wide) and gdn_reparam_bwd_kernel, with
    gradients of one sign so that no decision hangs on rounding: where d < 0 everything passes; where d > 0 a raw
    below the bound stores exactly +0 (accumulate: leaves the prefill's bits), a raw at or above it passes.
    norm == 1 operands: d_param is exact and d = (2 lb) * d_param is one fp32 rounding on both sides."""
    npix = 130
    braw, graw = R.gate_raws((C,), R.BBOUND), R.gate_raws((C, C), R.GBOUND)
    P = Params(env, dt, torch.zeros(C, C), torch.ones(C), braw, graw)
    pre = R.a2_prefill(f"gate-c{C}", C)
    for inverse in (False, True):
        for sign in (1, -1):
            x, g = R.signed_operands(f"{dt}-c{C}-{inverse}", npix, C, sign)
            ref = R.reference(x, g, P.gamma, P.beta_cpu, inverse)
            positive = (sign > 0) == inverse                     # GDN: g x > 0 gives u < 0
            for acc in (0, 1):
                dx, dbr, dgr = run_backward(env, dt, x, g, P, inverse, R.PADS[0], kernel, acc, pre)
                for name, got, raw, bound, dpar, p0 in (("dbeta_raw", dbr, braw, R.BBOUND, ref["dbeta"], pre[0]),
                                                        ("dgamma_raw", dgr, graw, R.GBOUND, ref["dgamma"], pre[1])):
                    what = f"gate {kernel} {dt} inverse {inverse} sign {sign} accumulate {acc}: {name}"
                    assert bool(((dpar > 0) == positive).all()) and bool((dpar != 0).all())
                    want = R.gate(raw, bound, dpar.float())
                    closed = (raw < bound) & positive
                    assert bool((want[closed] == 0).all()) and bool((want[~closed] != 0).all())
                    assert bool(closed.any()) == positive
                    if not acc:
                        assert_bits(got, want, what)
                        assert bool((got[closed].view(torch.int32) == 0).all()), f"{what}: a closed gate is not +0"
                        continue
                    assert_bits(got[closed], p0[closed], f"{what}: closed gates left the prefill")
                    # open gates: prefill + d, the product rounded first or not (an FMA)
                    two = p0 + want
                    one = (p0.double() + 2.0 * torch.clamp(raw.double(), min=bound) * dpar).float()
                    ok = (got == two) | (got == one)
                    assert bool(ok[~closed].all()), what


# ---- gdn1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.GDN1_CASES, ids=[c.id for c in R.GDN1_CASES])
def test_gdn1_out(env, case, dt):
    """out = x / norm (inverse: x * norm) and its backward: one product each, so s = |ref|; every operand at its
    own pitch."""
    dev, lib = env.dev, env.lib
    n, C = case.npix, case.C
    g_ = R.gen(f"gdn1-{case.id}-{dt}")
    x, gy = R.rnd(torch.randn(n, C, generator=g_), dt), R.rnd(torch.randn(n, C, generator=g_), dt)
    nrm = R.rnd(0.5 + 2.0 * torch.rand(n, C, generator=g_), dt)
    tdt = TORCH_DT[dt]
    for inverse in (False, True):
        xd, nd, gd = In(x, C + case.x, dt, dev), In(nrm, C + case.n, dt, dev), In(gy, C + case.g, dt, dev)
        y, dx, dn = (rows_out(n, C, C + p, dt, dev) for p in (case.y, case.dx, case.dn))
        lib.cai_gdn1_out(code(env, dt), xd.ptr, xd.ld, nd.ptr, nd.ld, y.ptr, C + case.y, n, C, int(inverse), env.stream())
        lib.cai_gdn1_out_bwd(code(env, dt), xd.ptr, xd.ld, nd.ptr, nd.ld, gd.ptr, gd.ld, dx.ptr, C + case.dx, dn.ptr,
                             C + case.dn, n, C, int(inverse), env.stream())
        torch.cuda.synchronize()
        ref = R.gdn1(x.double(), nrm.double(), gy.double(), inverse)
        mod = R.gdn1(x, nrm, gy, inverse)
        tag = f"{case.id}-{dt}-{'igdn' if inverse else 'gdn'}"
        for name, o, r, m in zip(("y", "dx", "dnorm"), (y, dx, dn), ref, mod):
            bar("gdn1_out_kernel" if name == "y" else "gdn1_out_bwd_kernel", tag, name, o.take(tag).cpu(), r, r.abs(),
                m.to(tdt))
