"""Exact integer-lattice tests of the fused ResidualUnit kernels (csrc/resunit.hip): cai_resunit in both directions
and both widths, cai_resunit_wgrad (immediate and deferred) and cai_resunit_wgrad_batch, through the C ABI.  No
tolerance anywhere in this file: every stored value is compared bit for bit with the CPU reference of
resunit_exact_cases.py (the lattice argument and the focus-stage rule are stated there; the two conditions, 2^24
and the 1 % cap, are asserted on the reference before the kernel's output is looked at).

Guards, as in test_conv_exact_gpu.py: every output lies inside a larger buffer, its elements pre-filled with NaN (or
the lattice, for accumulate), 4096 sentinel elements before and after and sentinel pitch columns that must survive;
input pitch columns hold junk; workspaces are filled with 0xFF; with gy_masked the gc buffer holds the sentinel and
must stay untouched; zero signs are normalised on both sides.
"""
import ctypes
import math

import pytest
import torch

import conv_exact_cases as CT
import resunit_exact_cases as T
from test_conv_exact_gpu import FP64_MACS, SENT, Env, Out, assert_bits, pm_in, round_up

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def env(cuda):
    return Env(cuda)


def _pm_out(B, C, H, W, ld, dev, prefill=None):
    """A pixel-major bf16 output [B*H*W][ld], logical NCHW, inside its guards."""
    return Out((B, C, H, W), (H * W * ld, 1, W * ld, ld), BF, dev, prefill)


def _packed(env, geom, direction, w):
    """The packed MFMA operand of a layer and its row length, as compressai._ops._packed_kp."""
    g = env.native.ConvGeom(*geom)
    wp = env.pack(g, env.native.BF16, direction, w)
    kout = g.out_c if direction == 0 else g.in_c
    return wp, wp.numel() // (2 * round_up(kout, 16))


def _unit_macs(u):
    nh = u.n // 2
    return u.B * u.H * u.W * (2 * u.n * nh + 9 * nh * nh)


def _reference(case, fn, macs):
    """fn(dtype) -> list of tensors: fp32, and for a small case asserted equal to fp64."""
    ref = fn(torch.float32)
    if macs <= FP64_MACS:
        for a, b in zip(ref, fn(torch.float64)):
            assert torch.equal(a.double(), b), f"{case.id}: the fp32 reference is not exact on the lattice"
    return ref


@pytest.mark.parametrize("u", T.UNITS, ids=[u.id for u in T.UNITS])
def test_resunit_exact(env, u):
    dev, n, nh, B, H, W = env.dev, u.n, u.n // 2, u.B, u.H, u.W
    t = T.draw_unit(u)
    full = T.ref_unit(u, t)
    T.check_unit_lattice(u, full)
    want = _reference(u, lambda d: list(T.ref_unit(u, t, d)[1]), _unit_macs(u))
    x_ld, out_ld, y_ld, r_ld, m_ld = T.unit_lds(u)
    ga = CT.geom12("conv", B, n, nh, H, W, 1, 1)
    gb = CT.geom12("conv", B, nh, nh, H, W, 3, 1)
    gc = CT.geom12("conv", B, nh, n, H, W, 1, 1)
    A = env.native.ResunitArgs(batch=B, h=H, w=W, n=n, x_ld=x_ld, out_ld=out_ld)
    out = _pm_out(B, n, H, W, out_ld, dev)
    A.out = out.ptr.value
    keep = []
    if u.direction == T.FWD:
        packs = [_packed(env, ga, 0, t["wa"]), _packed(env, gb, 0, t["wb"]), _packed(env, gc, 0, t["wc"])]
        xd = pm_in(t["x"], x_ld, BF, dev)
        bias = [t[k].to(dev).contiguous() for k in ("ba", "bb", "bc")]
        o1, o2 = _pm_out(B, nh, H, W, nh, dev), _pm_out(B, nh, H, W, nh, dev)
        A.x, A.h1, A.h2 = xd.data_ptr(), o1.ptr.value, o2.ptr.value
        A.ba, A.bb, A.bc = (b.data_ptr() for b in bias)
        outs = [(o1, "h1"), (o2, "h2"), (out, "y")]
    else:
        packs = [_packed(env, gc, 1, t["wc"]), _packed(env, gb, 1, t["wb"]), _packed(env, ga, 1, t["wa"])]
        masked = u.opts["gy_masked"]
        gyd = pm_in(full[3] if masked else t["gy"], x_ld, BF, dev)       # a masked gy is gc itself
        yd = pm_in(t["y"], y_ld, BF, dev)
        h1d, h2d = pm_in(t["h1"], nh, BF, dev), pm_in(t["h2"], nh, BF, dev)
        og = _pm_out(B, n, H, W, n, dev, torch.full((B, n, H, W), SENT) if masked else None)
        o1, o2 = _pm_out(B, nh, H, W, nh, dev), _pm_out(B, nh, H, W, nh, dev)
        A.x, A.y, A.y_ld, A.h1, A.h2 = gyd.data_ptr(), yd.data_ptr(), y_ld, h1d.data_ptr(), h2d.data_ptr()
        A.gc, A.gb, A.ga, A.gy_masked = og.ptr.value, o1.ptr.value, o2.ptr.value, int(masked)
        if t["res2"] is not None:
            rd = pm_in(t["res2"], r_ld, BF, dev)
            A.res2, A.res2_ld = rd.data_ptr(), r_ld
            keep.append(rd)
        if t["xmask"] is not None:
            md = pm_in(t["xmask"], m_ld, BF, dev)
            A.xmask, A.xmask_ld = md.data_ptr(), m_ld
            keep.append(md)
        keep += [yd, h1d, h2d]
        gc_want = torch.full((B, n, H, W), SENT) if masked else full[3]
        outs = [(og, "gc"), (o1, "gb"), (o2, "ga"), (out, "dx")]
        want = [gc_want] + want
    (wa, A.kpa), (wb, A.kpb), (wc, A.kpc) = packs
    A.wa, A.wb, A.wc = wa.data_ptr(), wb.data_ptr(), wc.data_ptr()
    env.lib.cai_resunit(ctypes.byref(A), u.direction, env.stream())
    torch.cuda.synchronize()
    for (o, name), w in zip(outs, want):
        assert_bits(o.take(f"{u.id} {name}"), w.to(BF), f"{u.id} {name}")


def _wg_call(env, c, ops, init):
    """The argument block of one cai_resunit_wgrad call: operands on the device, the six outputs inside guards."""
    dev, n, nh = env.dev, c.n, c.n // 2
    x_ld, gc_ld = (n + 8, n + 16) if c.pitch else (n, n)
    lds = (x_ld, nh, nh, nh, nh, gc_ld)
    dops = [pm_in(v, ld, BF, dev) for v, ld in zip(ops, lds)]
    outs = []
    for k, s in enumerate(T.wg_shapes(n)):
        strides = tuple(math.prod(s[i + 1:]) for i in range(len(s)))
        outs.append(Out(s, strides, torch.float32, dev, init[k] if c.acc else None))
    A = env.native.ResunitWgradArgs(batch=c.B, h=c.H, w=c.W, n=n, x_ld=x_ld, gc_ld=gc_ld, accumulate=c.acc)
    A.x, A.h1, A.h2, A.ga, A.gb, A.gc = (v.data_ptr() for v in dops)
    A.dwa, A.dba, A.dwb, A.dbb, A.dwc, A.dbc = (o.ptr.value for o in outs)
    return A, dops, outs


def _wg_want(c, ops, init):
    nh = c.n // 2
    macs = c.B * c.H * c.W * (2 * c.n * nh + 9 * nh * nh)
    return _reference(c, lambda d: T.ref_wgrad(c, ops, init, d), macs)


def _wg_check(c, outs, want, how):
    for o, w, name in zip(outs, want, ("dwa", "dba", "dwb", "dbb", "dwc", "dbc")):
        assert_bits(o.take(f"{c.id} {name}"), w, f"{c.id} {name} ({how})")


@pytest.mark.parametrize("c", T.WGRADS, ids=[c.id for c in T.WGRADS])
def test_resunit_wgrad_exact(env, c):
    """One call run now (jobs = NULL) and one deferred: three jobs returned, then cai_reduce_jobs.  Both exact."""
    ops, init = T.draw_wgrad(c)
    want = _wg_want(c, ops, init)
    for deferred in (False, True):
        A, dops, outs = _wg_call(env, c, ops, init)
        nbytes = env.lib.cai_resunit_wgrad_workspace_bytes(ctypes.byref(A))
        assert nbytes == T.rw_workspace_bytes(c.n, c.B * c.H * c.W)
        ws, _ = env.ws(nbytes)
        if deferred:
            jobs = (env.native.ReduceJob * 3)()
            env.lib.cai_resunit_wgrad(ctypes.byref(A), env.p(ws), nbytes, env.stream(), jobs)
            assert [j.kind for j in jobs] == [env.native.JOB_WGRAD] * 3
            env.lib.cai_reduce_jobs(jobs, 3, env.stream())
        else:
            env.lib.cai_resunit_wgrad(ctypes.byref(A), env.p(ws), nbytes, env.stream(), None)
        torch.cuda.synchronize()
        _wg_check(c, outs, want, "deferred" if deferred else "immediate")


def test_resunit_wgrad_batch_exact(env):
    """35 units in one cai_resunit_wgrad_batch call: 28 of N = 192 (the launch of that width flushes at
    RW_BATCH_MAX = 24) with 7 of N = 128 in between, every unit with its own data and every gradient exact
    against torch; n = 0 returns OK and writes nothing."""
    units = T.BATCH
    assert sum(1 for c in units if c.n == 192) > T.RW_BATCH_MAX + 1 and sum(1 for c in units if c.n == 128) > 1
    env.lib.cai_resunit_wgrad_batch(None, None, None, 0, env.stream(), None)
    arr = (env.native.ResunitWgradArgs * len(units))()
    wss = (ctypes.c_void_p * len(units))()
    nbs = (ctypes.c_size_t * len(units))()
    keep, wants = [], []
    for i, c in enumerate(units):
        ops, init = T.draw_wgrad(c)
        wants.append(_wg_want(c, ops, init))
        A, dops, outs = _wg_call(env, c, ops, init)
        arr[i] = A
        nbs[i] = env.lib.cai_resunit_wgrad_workspace_bytes(ctypes.byref(A))
        ws, _ = env.ws(nbs[i])
        wss[i] = ws.data_ptr()
        keep.append((dops, outs, ws))
    jobs = (env.native.ReduceJob * (3 * len(units)))()
    env.lib.cai_resunit_wgrad_batch(arr, wss, nbs, 0, env.stream(), jobs)       # n = 0 with live arguments
    torch.cuda.synchronize()
    for c, (dops, outs, ws) in zip(units, keep):
        assert bool((ws == 0xFF).all()), f"{c.id}: n = 0 wrote a workspace"
        for o in outs:
            assert torch.equal(o.buf.view(torch.int32), o.snap.view(torch.int32)), f"{c.id}: n = 0 wrote a gradient"
    env.lib.cai_resunit_wgrad_batch(arr, wss, nbs, len(units), env.stream(), jobs)
    env.lib.cai_reduce_jobs(jobs, len(jobs), env.stream())
    torch.cuda.synchronize()
    for c, (dops, outs, ws), want in zip(units, keep, wants):
        _wg_check(c, outs, want, "batch")
