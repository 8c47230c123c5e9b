"""Exact integer-lattice tests of every conv, input-gradient and weight-gradient kernel (conv.hip, conv_quad.hip,
edge.hip, deconv_small.hip): no tolerance anywhere in this file.

Every operand is drawn from a small set of non-zero integers.  Each bf16 product is then exact in fp32 and every
partial sum is an integer below 2^24, so the result has the same bit pattern in any accumulation order, tiling or
split: a correct kernel is bit-exact against torch, a kernel that drops, doubles or misplaces one product is not.

  fp32 outputs (forward with fp32 y, every weight / bias gradient): operands from {+-1, +-2, +-3};
  bf16 outputs (every dx, forward with bf16 y): operands from {-1, +1}, so the sums stay where bf16 holds every
    integer (|v| <= 256) and one lost product is visible; the expected bits are ref.bfloat16(), the one
    round-to-nearest-even the kernels' (bf16)v performs.  At most 1 % of a case's elements may exceed 256.

Each case asserts terms * vmax^2 + addends < 2^24 on the host, and the small ones that the fp32 CPU reference
equals the fp64 one.  Outputs live inside larger buffers: the output elements are pre-filled with NaN (an
unwritten element fails), everything around them (guard rows, pitch padding, row gaps) with a sentinel that must
survive.  Zero signs are normalised on both sides (v + 0): a masked element may be -0 or +0.

The case table and the proof that it reaches every kernel are conv_exact_cases.py / test_conv_exact_cases.py.
"""
import ctypes
import zlib

import pytest
import torch
import torch.nn.functional as F

import conv_exact_cases as T

pytestmark = pytest.mark.gpu

EXACT = 1 << 24
SENT = 12345.0            # bf16- and fp32-exact, outside every case's range of results
JUNK = 5.0                # pitch columns of the inputs: finite, off the lattice
FP64_MACS = 3e8           # cases up to this many multiply-adds also check the fp32 reference against fp64
SLOPE = T.SLOPE


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def lattice(shape, vmax, gen):
    """Uniform over the non-zero integers of [-vmax, vmax], fp32 on the CPU."""
    mag = torch.randint(1, vmax + 1, shape, generator=gen)
    sgn = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (mag * sgn).float()


def _bits(t):
    t = t + 0          # -0 -> +0
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def assert_bits(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    n = int(bad.sum())
    if n:
        idx = bad.nonzero()[:8]
        rows = [tuple(i.tolist()) + (float(got[tuple(i)]), float(want[tuple(i)])) for i in idx]
        pytest.fail(f"{what}: {n} of {bad.numel()} elements differ; first (index..., got, want): {rows}")


def round_up(v, m):
    return (v + m - 1) // m * m


def pm_in(t, ld, dtype, dev):
    """NCHW fp32 (CPU) -> pixel-major [B*H*W][ld] on the device: channels C.. of the 8-channel group zero (the
    padding cai_pack_nchw writes), the pitch columns past it junk."""
    B, C, H, W = t.shape
    n = B * H * W
    buf = torch.full((n + 16, ld), JUNK)          # 16 junk rows behind the last pixel
    buf[:, :min(ld, round_up(C, 8))] = 0
    buf[:n, :C] = t.permute(0, 2, 3, 1).reshape(-1, C)
    return buf.to(dtype).to(dev).contiguous()[:n]


class Out:
    """An output of logical `shape` at element `strides` inside a sentinel-filled buffer."""

    def __init__(self, shape, strides, dtype, dev, prefill=None):
        span = 1 + sum((n - 1) * s for n, s in zip(shape, strides))
        self.guard = 4096
        self.buf = torch.full((self.guard + round_up(span, 64) + self.guard,), SENT, dtype=dtype, device=dev)
        self.shape, self.strides = tuple(shape), tuple(strides)
        v = self.view(self.buf)
        if prefill is None:
            v.fill_(float("nan"))
        else:
            v.copy_(prefill.to(dev))
        self.snap = self.buf.clone()

    def view(self, buf):
        return buf.as_strided(self.shape, self.strides, self.guard)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.guard * self.buf.element_size())

    def take(self, what):
        """The output values; asserts that nothing outside them was written."""
        got = self.view(self.buf).clone()
        self.view(self.buf).zero_()
        self.view(self.snap).zero_()
        assert torch.equal(_bits(self.buf), _bits(self.snap)), f"{what}: wrote outside its output elements"
        return got


def pm_out(B, C, H, W, ld, dtype, dev, gap=False, prefill=None):
    """Pixel-major output, logical NCHW; gap: one pixel between rows and two rows between images."""
    ysy = (W + (1 if gap else 0)) * ld
    ysb = H * ysy + (2 * ysy if gap else 0)
    return Out((B, C, H, W), (ysb, 1, ysy, ld), dtype, dev, prefill), (ysb, 1, ysy, ld)


def _conv(g, x, w, b):
    B, cin, ih, iw, cout, oh, ow, k, s, p, op, tr = g
    if tr:
        return F.conv_transpose2d(x, w, b, stride=s, padding=p, output_padding=op)
    return F.conv2d(x, w, b, stride=s, padding=p)


def _wshape(g):
    B, cin, ih, iw, cout, oh, ow, k, s, p, op, tr = g
    return (cin, cout, k, k) if tr else (cout, cin, k, k)


def _macs(g):
    B, cin, ih, iw, cout, oh, ow, k, s, p, op, tr = g
    return B * (ih * iw if tr else oh * ow) * cin * cout * k * k


def _both(fn, g):
    """fn(dtype) -> reference tensors; computed in fp32 and, for a small case, checked against fp64."""
    ref = fn(torch.float32)
    if _macs(g) <= FP64_MACS:
        for a, b in zip(ref, fn(torch.float64)):
            assert torch.equal(a.double(), b), "the fp32 reference is not exact on the lattice"
    return ref


def _cap(exact, what):
    """bf16 outputs: at most 1 % of the exact values may lie where bf16 no longer holds every integer."""
    frac = (exact.abs() > 256).float().mean().item()
    assert frac <= 0.01, f"{what}: {frac:.4f} of the reference exceeds 256"


def _act(y, act):
    if act == T.RELU:
        return torch.relu(y)
    if act == T.LEAKY:
        return torch.where(y > 0, y, y * SLOPE)
    return y


def _mask(aux, mode, dt):
    if mode == T.POS:
        return (aux > 0).to(dt)
    if mode == T.MLEAKY:
        return torch.where(aux > 0, 1.0, SLOPE).to(dt)
    if mode == T.SIGN:
        return torch.sign(aux).to(dt)
    return torch.ones_like(aux, dtype=dt)


class Env:
    def __init__(self, dev):
        from compressai import _native as native
        from compressai._ops import _p, _stream

        self.dev, self.native, self.lib, self.p, self.stream = dev, native, native.lib, _p, _stream

    def ws(self, nbytes):
        """A workspace of arbitrary content (NaN bit patterns): the kernels must not rely on zeros."""
        if not nbytes:
            return None, 0
        return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=self.dev), nbytes

    def pack(self, g, dt, direction, w):
        n = self.lib.cai_conv_packed_weight_bytes(ctypes.byref(g), dt, direction)
        wp = torch.empty(n, dtype=torch.uint8, device=self.dev)
        wd = w.to(self.dev).contiguous()      # (named: alive until the launch is queued on this stream)
        self.lib.cai_conv_pack_weight(ctypes.byref(g), dt, direction, self.p(wd), None,
                                      self.p(wp), self.stream())
        return wp


@pytest.fixture(scope="module")
def env(cuda):
    return Env(cuda)


def _check_dispatch(env, run, g, dt):
    tf = 1 if (run.opts.get("abs") or run.opts.get("sq")) else 0
    name = env.lib.cai_conv_kernel_name(ctypes.byref(g), dt, run.direction, tf).decode()
    if name != run.kernel:       # an A/B knob of this process moved the case: still exact, on another kernel
        print(f"{run.id}: runs on {name}, written for {run.kernel}")


def run_forward(env, run):
    o, dev = run.opts, env.dev
    B, cin, ih, iw, cout, oh, ow, k, s, p, op, tr = run.geom
    f32ops = o.get("dtype") == "f32"
    ydt = torch.float32 if (f32ops or o.get("y", "f32") != "bf16") else torch.bfloat16
    tdt, dt = (torch.float32, env.native.F32) if f32ops else (torch.bfloat16, env.native.BF16)
    vmax = 1 if ydt == torch.bfloat16 else 3
    gen = _gen(run.id)
    x = lattice((B, cin, ih, iw), vmax, gen)
    w = lattice(_wshape(run.geom), vmax, gen)
    bias = lattice((cout,), vmax, gen) if o.get("bias", True) else None
    res = lattice((B, cout, oh, ow), vmax, gen) if o.get("res") else None
    assert k * k * cin * vmax * vmax + (vmax if bias is not None else 0) + (vmax if res is not None else 0) < EXACT

    def ref(d):
        y = _conv(run.geom, x.to(d).abs() if o.get("abs") else x.to(d), w.to(d), None if bias is None else bias.to(d))
        if res is not None:
            y = y + res.to(d)
        return (_act(y, o.get("act", 0)),)

    want, = _both(ref, run.geom)
    if ydt == torch.bfloat16:
        _cap(want, run.id)
    want = want.to(ydt)

    g = env.native.ConvGeom(*run.geom)
    _check_dispatch(env, run, g, dt)
    pitch = 8 if o.get("pitch") else 0
    x_ld = round_up(cin, 8) + pitch
    xd = pm_in(x, x_ld, tdt, dev)
    wp = env.pack(g, dt, 0, w)
    bd = None if bias is None else bias.to(dev)
    if o.get("y") == "nchw":
        strides = (cout * oh * ow + (16 if pitch else 0), oh * ow, ow, 1)
        out = Out((B, cout, oh, ow), strides, ydt, dev)
    else:
        out, strides = pm_out(B, cout, oh, ow, round_up(cout, 8) + pitch, ydt, dev, gap=bool(pitch))
    ws, wsb = env.ws(env.lib.cai_conv_workspace_bytes(ctypes.byref(g), dt, 0))
    ydc = env.native.BF16 if ydt == torch.bfloat16 else env.native.F32
    common = (ctypes.c_void_p(out.ptr.value), ydc, *strides, env.p(ws), wsb, env.stream())
    if res is not None:
        r_ld = round_up(cout, 8) + pitch
        rd = pm_in(res, r_ld, torch.bfloat16, dev)
        env.lib.cai_conv_fwd_res(ctypes.byref(g), dt, env.p(xd), x_ld, int(bool(o.get("abs"))), env.p(wp), env.p(bd),
                                 o.get("act", 0), SLOPE, env.p(rd), r_ld, *common)
    else:
        env.lib.cai_conv_fwd(ctypes.byref(g), dt, env.p(xd), x_ld, int(bool(o.get("abs"))), env.p(wp), env.p(bd),
                             o.get("act", 0), SLOPE, *common)
    torch.cuda.synchronize()
    assert_bits(out.take(run.id), want, run.id)


def run_dgrad(env, run):
    o, dev = run.opts, env.dev
    B, cin, ih, iw, cout, oh, ow, k, s, p, op, tr = run.geom
    f32ops = o.get("dtype") == "f32"
    tdt, dt = (torch.float32, env.native.F32) if f32ops else (torch.bfloat16, env.native.BF16)
    vmax = 3 if f32ops else 1
    gen = _gen(run.id)
    dy = lattice((B, cout, oh, ow), vmax, gen)
    w = lattice(_wshape(run.geom), vmax, gen)
    nres = o.get("res", 0)
    rs = [lattice((B, cin, ih, iw), vmax, gen) for _ in range(nres)]
    mode = o.get("mask", 0)
    aux = torch.randint(-2, 3, (B, cin, ih, iw), generator=gen).float() if mode else None   # zeros included
    assert k * k * cout * vmax * vmax + nres * vmax < EXACT

    def ref(d):
        x0 = torch.zeros(B, cin, ih, iw, dtype=d, requires_grad=True)
        dx, = torch.autograd.grad(_conv(run.geom, x0, w.to(d), None), x0, dy.to(d))
        for r in rs:
            dx = dx + r.to(d)
        return (dx * _mask(aux, mode, d) if mode else dx,)

    want, = _both(ref, run.geom)
    if not f32ops:
        _cap(want, run.id)
    want = want.to(tdt)

    g = env.native.ConvGeom(*run.geom)
    _check_dispatch(env, run, g, dt)
    pitch = 8 if o.get("pitch") else 0
    dy_ld = round_up(cout, 8) + pitch
    dx_ld = round_up(cin, 8) + pitch
    dyd = pm_in(dy, dy_ld, tdt, dev)
    wp = env.pack(g, dt, 1, w)
    out, _ = pm_out(B, cin, ih, iw, dx_ld, tdt, dev)
    ws, wsb = env.ws(env.lib.cai_conv_workspace_bytes(ctypes.byref(g), dt, 1))
    a_ld = round_up(cin, 8) + pitch
    ad = pm_in(aux, a_ld, tdt, dev) if mode else None
    rd = [pm_in(r, a_ld, torch.bfloat16, dev) for r in rs]
    tail = (ctypes.c_void_p(out.ptr.value), dx_ld, mode, SLOPE, env.p(ad), a_ld if mode else 0, env.p(ws), wsb,
            env.stream())
    head = (ctypes.byref(g), dt, env.p(dyd), dy_ld, env.p(wp))
    if nres == 2:
        env.lib.cai_conv_dgrad_res2(*head, env.p(rd[0]), a_ld, env.p(rd[1]), a_ld, *tail)
    elif nres == 1:
        env.lib.cai_conv_dgrad_res(*head, env.p(rd[0]), a_ld, *tail)
    else:
        env.lib.cai_conv_dgrad(*head, *tail)
    torch.cuda.synchronize()
    assert_bits(out.take(run.id), want, run.id)


def run_wgrad(env, run):
    o, dev = run.opts, env.dev
    B, cin, ih, iw, cout, oh, ow, k, s, p, op, tr = run.geom
    f32ops = o.get("dtype") == "f32"
    tdt, dt = (torch.float32, env.native.F32) if f32ops else (torch.bfloat16, env.native.BF16)
    gen = _gen(run.id)
    x = lattice((B, cin, ih, iw), 3, gen)
    dy = lattice((B, cout, oh, ow), 3, gen)
    acc = bool(o.get("acc"))
    dw0 = lattice(_wshape(run.geom), 3, gen) if acc else None
    db0 = lattice((cout,), 3, gen) if acc else None
    xmax = 9 if o.get("sq") else 3
    assert max(B * ih * iw, B * oh * ow) * xmax * 3 + 3 < EXACT

    def ref(d):
        xt = x.to(d)
        xt = xt.abs() if o.get("abs") else (xt * xt if o.get("sq") else xt)
        w0 = torch.zeros(_wshape(run.geom), dtype=d, requires_grad=True)
        b0 = torch.zeros(cout, dtype=d, requires_grad=True)
        dw, db = torch.autograd.grad(_conv(run.geom, xt, w0, b0), (w0, b0), dy.to(d))
        return (dw + dw0.to(d), db + db0.to(d)) if acc else (dw, db)

    want_w, want_b = _both(ref, run.geom)

    g = env.native.ConvGeom(*run.geom)
    _check_dispatch(env, run, g, dt)
    pitch = 8 if o.get("pitch") else 0
    x_ld = round_up(cin, 8) + pitch
    dy_ld = round_up(cout, 8) + pitch
    xd = pm_in(x, x_ld, tdt, dev)
    dyd = pm_in(dy, dy_ld, tdt, dev)
    ws_ = want_w.shape
    dw = Out(ws_, (ws_[1] * k * k, k * k, k, 1), torch.float32, dev, dw0)
    db = Out((cout,), (1,), torch.float32, dev, db0) if o.get("bias", True) else None
    ws, wsb = env.ws(env.lib.cai_conv_wgrad_workspace_bytes(ctypes.byref(g), dt))
    env.lib.cai_conv_wgrad(ctypes.byref(g), dt, env.p(xd), x_ld, int(bool(o.get("abs"))), int(bool(o.get("sq"))),
                           env.p(dyd), dy_ld, ctypes.c_void_p(dw.ptr.value),
                           None if db is None else ctypes.c_void_p(db.ptr.value), int(acc), env.p(ws), wsb,
                           env.stream())
    torch.cuda.synchronize()
    assert_bits(dw.take(run.id), want_w, run.id + " dw")
    if db is not None:
        assert_bits(db.take(run.id), want_b, run.id + " db")


@pytest.mark.parametrize("run", T.RUNS, ids=[r.id for r in T.RUNS])
def test_conv_exact(env, run):
    (run_forward, run_dgrad, run_wgrad)[run.direction](env, run)


# ---- csrc/edge.hip --------------------------------------------------------------------------------------------------
def _edge_frag(env, g, direction, w):
    n = env.lib.cai_edge_frag_bytes(ctypes.byref(g), env.native.BF16, direction)
    assert n > 0
    frag = torch.empty(n, dtype=torch.uint8, device=env.dev)
    wd = w.to(env.dev).contiguous()
    env.lib.cai_edge_pack_weights(ctypes.byref(g), env.native.BF16, direction, env.p(wd),
                                  env.p(frag), env.stream())
    return frag


def _nchw_out(shape, dev, prefill=None):
    B, C, H, W = shape
    return Out(shape, (C * H * W, H * W, W, 1), torch.float32, dev, prefill)


@pytest.mark.parametrize("case", T.EDGE_CONV, ids=[f"conv{c[1]}-{c[2]}k{c[5]}_{c[3]}x{c[4]}" for c in T.EDGE_CONV])
def test_edge_conv_exact(env, case):
    """Conv2d(C <= 3, N, k, 2, k/2) on edge_s2d_kernel (bf16 y: the {-1, +1} lattice, |y| <= 76) and its weight /
    bias gradient on the edge weight-gradient kernels (fp32: {+-1, +-2, +-3}), overwritten and accumulated."""
    B, C, N, H, W, k = case
    dev = env.dev
    geom = T.geom12("conv", B, C, N, H, W, k, 2)
    g = env.native.ConvGeom(*geom)
    assert env.lib.cai_edge_supported(ctypes.byref(g), env.native.BF16) == 1
    Hs, Ws = H // 2, W // 2
    gen = _gen(f"edge-conv-{case}")
    x1, w1, b1 = lattice((B, C, H, W), 1, gen), lattice((N, C, k, k), 1, gen), lattice((N,), 1, gen)
    assert k * k * C + 1 <= 256
    want, = _both(lambda d: (_conv(geom, x1.to(d), w1.to(d), b1.to(d)),), geom)
    y_ld = N + 8
    out, _ = pm_out(B, N, Hs, Ws, y_ld, torch.bfloat16, dev)
    x1d, b1d, frag = x1.to(dev), b1.to(dev), _edge_frag(env, g, 0, w1)
    env.lib.cai_edge_conv_fwd(ctypes.byref(g), env.p(x1d), env.p(frag), env.p(b1d),
                              ctypes.c_void_p(out.ptr.value), y_ld, env.stream())
    torch.cuda.synchronize()
    assert_bits(out.take("edge conv y"), want.bfloat16(), "edge conv y")

    x, dy = lattice((B, C, H, W), 3, gen), lattice((B, N, Hs, Ws), 3, gen)
    dw0, db0 = lattice((N, C, k, k), 3, gen), lattice((N,), 3, gen)
    assert B * Hs * Ws * 9 + 3 < EXACT

    def ref(d):
        w0 = torch.zeros(N, C, k, k, dtype=d, requires_grad=True)
        b0 = torch.zeros(N, dtype=d, requires_grad=True)
        return torch.autograd.grad(_conv(geom, x.to(d), w0, b0), (w0, b0), dy.to(d))

    want_w, want_b = _both(ref, geom)
    xd, dyd = x.to(dev), pm_in(dy, y_ld, torch.bfloat16, dev)
    for acc in (0, 1):
        dw = Out((N, C, k, k), (C * k * k, k * k, k, 1), torch.float32, dev, dw0 if acc else None)
        db = Out((N,), (1,), torch.float32, dev, db0 if acc else None)
        ws, wsb = env.ws(env.lib.cai_edge_workspace_bytes(ctypes.byref(g), env.native.BF16))
        env.lib.cai_edge_wgrad(ctypes.byref(g), env.p(xd), env.p(dyd), y_ld, ctypes.c_void_p(dw.ptr.value),
                               ctypes.c_void_p(db.ptr.value), acc, env.p(ws), wsb, env.stream())
        torch.cuda.synchronize()
        assert_bits(dw.take("edge conv dw"), want_w + dw0 if acc else want_w, f"edge conv dw (accumulate {acc})")
        assert_bits(db.take("edge conv db"), want_b + db0 if acc else want_b, f"edge conv db (accumulate {acc})")


@pytest.mark.parametrize("case", T.EDGE_DECONV,
                         ids=[f"deconv{c[1]}-{c[2]}k{c[5]}_{c[3]}x{c[4]}" for c in T.EDGE_DECONV])
def test_edge_deconv_exact(env, case):
    """ConvTranspose2d(N, C <= 3, k, 2, k/2, 1): forward on edge_d2s_kernel (fp32 image), input gradient on
    edge_s2d_kernel (bf16 dx: {-1, +1}, at most 9 C taps), weight / bias gradient (fp32)."""
    B, N, C, H, W, k = case
    dev = env.dev
    geom = T.geom12("deconv", B, N, C, H, W, k, 2)
    g = env.native.ConvGeom(*geom)
    assert env.lib.cai_edge_supported(ctypes.byref(g), env.native.BF16) == 1
    gen = _gen(f"edge-deconv-{case}")
    x, w, b = lattice((B, N, H, W), 3, gen), lattice((N, C, k, k), 3, gen), lattice((C,), 3, gen)
    dy = lattice((B, C, 2 * H, 2 * W), 3, gen)
    dw0, db0 = lattice((N, C, k, k), 3, gen), lattice((C,), 3, gen)
    assert max(9 * N * 9 + 3, 4 * B * H * W * 9 + 3) < EXACT

    def ref(d):
        w0 = w.to(d).requires_grad_()
        b0 = b.to(d).requires_grad_()
        y = _conv(geom, x.to(d), w0, b0)
        return (y.detach(),) + torch.autograd.grad(y, (w0, b0), dy.to(d))

    want_y, want_w, want_b = _both(ref, geom)
    x_ld = N + 8
    xd = pm_in(x, x_ld, torch.bfloat16, dev)
    out = _nchw_out((B, C, 2 * H, 2 * W), dev)
    bd, frag = b.to(dev), _edge_frag(env, g, 0, w)
    env.lib.cai_edge_deconv_fwd(ctypes.byref(g), env.p(xd), x_ld, env.p(frag), env.p(bd),
                                ctypes.c_void_p(out.ptr.value), env.stream())
    torch.cuda.synchronize()
    assert_bits(out.take("edge deconv y"), want_y, "edge deconv y")

    dyd = dy.to(dev)
    for acc in (0, 1):
        dw = Out((N, C, k, k), (C * k * k, k * k, k, 1), torch.float32, dev, dw0 if acc else None)
        db = Out((C,), (1,), torch.float32, dev, db0 if acc else None)
        ws, wsb = env.ws(env.lib.cai_edge_workspace_bytes(ctypes.byref(g), env.native.BF16))
        env.lib.cai_edge_wgrad(ctypes.byref(g), env.p(dyd), env.p(xd), x_ld, ctypes.c_void_p(dw.ptr.value),
                               ctypes.c_void_p(db.ptr.value), acc, env.p(ws), wsb, env.stream())
        torch.cuda.synchronize()
        assert_bits(dw.take("edge deconv dw"), want_w + dw0 if acc else want_w, f"edge deconv dw (accumulate {acc})")
        assert_bits(db.take("edge deconv db"), want_b + db0 if acc else want_b, f"edge deconv db (accumulate {acc})")

    w1, dy1 = lattice((N, C, k, k), 1, gen), lattice((B, C, 2 * H, 2 * W), 1, gen)
    assert k * k * C <= 256

    def ref_dx(d):
        x0 = torch.zeros(B, N, H, W, dtype=d, requires_grad=True)
        return torch.autograd.grad(_conv(geom, x0, w1.to(d), None), x0, dy1.to(d))

    want_dx, = _both(ref_dx, geom)
    dx, _ = pm_out(B, N, H, W, x_ld, torch.bfloat16, dev)
    dy1d, frag1 = dy1.to(dev), _edge_frag(env, g, 1, w1)
    env.lib.cai_edge_deconv_dgrad(ctypes.byref(g), env.p(dy1d), env.p(frag1),
                                  ctypes.c_void_p(dx.ptr.value), x_ld, env.stream())
    torch.cuda.synchronize()
    assert_bits(dx.take("edge deconv dx"), want_dx.bfloat16(), "edge deconv dx")


# ---- csrc/deconv_small.hip ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.DECONV_SMALL, ids=[f"{c[1]}-{c[2]}k{c[5]}s{c[6]}_{c[3]}x{c[4]}" for c in T.DECONV_SMALL])
def test_deconv_small_exact(env, case):
    """ConvTranspose2d with <= 16 output channels as per-input-pixel GEMM + col2im.  The forward keeps the GEMM's
    result P = x W' (one sum over the N input channels per tap) in bf16 by design, so its operands come from
    {-1, +1}: |P| <= N <= 256 is then held exactly and the fp32 col2im sum (+ bias from {+-1, +-2, +-3}) stays
    exact.  Backward: dx (bf16, k*k*C <= 75 terms) from {-1, +1}; dw / db (fp32) from {+-1, +-2, +-3}."""
    B, N, C, H, W, k, s = case
    dev = env.dev
    geom = T.geom12("deconv", B, N, C, H, W, k, s)
    g = env.native.ConvGeom(*geom)
    OH, OW = geom[5], geom[6]
    wsb = env.lib.cai_deconv_small_workspace_bytes(ctypes.byref(g), env.native.BF16)
    assert wsb > 0
    gen = _gen(f"deconv-small-{case}")
    x1, w1, b3 = lattice((B, N, H, W), 1, gen), lattice((N, C, k, k), 1, gen), lattice((C,), 3, gen)
    assert N <= 256 and k * k * N + 3 < EXACT
    want_y, = _both(lambda d: (_conv(geom, x1.to(d), w1.to(d), b3.to(d)),), geom)
    x_ld = N + 8
    xd = pm_in(x1, x_ld, torch.bfloat16, dev)
    out = _nchw_out((B, C, OH, OW), dev)
    ws, _ = env.ws(wsb)
    w1d, b3d = w1.to(dev), b3.to(dev)
    env.lib.cai_deconv_small_fwd(ctypes.byref(g), env.native.BF16, env.p(xd), x_ld, env.p(w1d), env.p(b3d),
                                 ctypes.c_void_p(out.ptr.value), env.p(ws), wsb, env.stream())
    torch.cuda.synchronize()
    assert_bits(out.take("deconv_small y"), want_y, "deconv_small y")

    # backward with w from {-1, +1}: dx (bf16) stays within k*k*C*3 = 225 for either dy lattice
    x3, dy3 = lattice((B, N, H, W), 3, gen), lattice((B, C, OH, OW), 3, gen)
    dy1 = lattice((B, C, OH, OW), 1, gen)
    dw0, db0 = lattice((N, C, k, k), 3, gen), lattice((C,), 3, gen)
    assert k * k * C <= 256 and B * OH * OW * 9 + 3 < EXACT

    def ref(xv, dyv, wv):
        def fn(d):
            x0 = xv.to(d).requires_grad_()
            w0 = wv.to(d).requires_grad_()
            b0 = torch.zeros(C, dtype=d, requires_grad=True)
            return torch.autograd.grad(_conv(geom, x0, w0, b0), (x0, w0, b0), dyv.to(d))
        return _both(fn, geom)

    for xv, dyv, acc, what in ((x1, dy1, 0, "{-1,+1}"), (x3, dy3, 1, "{+-1..3}")):
        want_dx, want_w, want_b = ref(xv, dyv, w1)
        xd = pm_in(xv, x_ld, torch.bfloat16, dev)
        dx, _ = pm_out(B, N, H, W, x_ld, torch.bfloat16, dev)
        dw = Out((N, C, k, k), (C * k * k, k * k, k, 1), torch.float32, dev, dw0 if acc else None)
        db = Out((C,), (1,), torch.float32, dev, db0 if acc else None)
        ws, _ = env.ws(wsb)
        dyd = dyv.to(dev)
        env.lib.cai_deconv_small_bwd(ctypes.byref(g), env.native.BF16, env.p(xd), x_ld, env.p(w1d),
                                     env.p(dyd), ctypes.c_void_p(dx.ptr.value), x_ld,
                                     ctypes.c_void_p(dw.ptr.value), ctypes.c_void_p(db.ptr.value), acc, env.p(ws), wsb,
                                     env.stream())
        torch.cuda.synchronize()
        assert_bits(dx.take("deconv_small dx"), want_dx.bfloat16(), f"deconv_small dx {what}")   # |dx| <= 225
        assert_bits(dw.take("deconv_small dw"), want_w + dw0 if acc else want_w, f"deconv_small dw {what}")
        assert_bits(db.take("deconv_small db"), want_b + db0 if acc else want_b, f"deconv_small db {what}")
