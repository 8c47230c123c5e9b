"""Every kernel of csrc/swin.hip, called through the C ABI, against the plain restatement (swin_reference.py) run on
the CPU: LayerNorm forward / backward, exact GELU, shifted-window cross attention, the channel aligner's pooled sum
and affine.  The case table is swin_cases.py; test_swin_reference_cpu.py proves that it reaches every launch branch,
that the restatement equals the oracle, and that the exact cases' preconditions hold.

Exact cases (no tolerance): operands on an integer lattice chosen so that every sum is exact in fp32 in any order
or grouping, so a kernel that drops, doubles or misplaces one term differs in its bits.
  attention   bias table 0, q = 0 or k = 0, so every score is 0 and P = 1 / n inside a mask group of n = 16, 8, 4,
              2 or 1 tokens (mask -1000 across groups: expf gives exactly 0); out, dq, dk, dv and the bias-table
              gradient (block partials -> 64 splits -> totals -> rel_index gather -> accumulate) are bit-equal
  LayerNorm   db = sum dy with dy on the lattice, whatever x is
  mean        fp32(integer sum) * fp32(scale), one multiply
  affine      gamma * x + beta_scale * beta on the lattice
bf16 results are the one round-to-nearest-even of the exact value on both sides; zero signs are normalised.

Tolerance cases: e_kernel <= 4 * e_ref per tensor, the bar of test_ssf_ops_gpu.py: e_ref is the fp32 CPU
restatement's own max error against the fp64 one on the same operands, computed in the test; for bf16 both round
their result once to bf16 from the same bf16 operands.  Every tensor prints "BAR <case> <tensor> e_kernel e_ref".

Outputs live in sentinel-guarded, NaN-prefilled buffers (Out of test_conv_exact_gpu.py); the pitch columns of the
inputs and the rows around them hold NaN.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import swin_cases as T
import swin_inputs as I
import swin_reference as R
from test_conv_exact_gpu import Env, Out, assert_bits

pytestmark = pytest.mark.gpu

MARGIN = 4.0
NAN = float("nan")
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
EPS = torch.tensor(1e-5, dtype=torch.float32).item()       # the fp32 value the kernel receives


@pytest.fixture(scope="module")
def env(cuda):
    return Env(cuda)


def code(env, dt):
    return env.native.BF16 if dt == "bf16" else env.native.F32


def rnd(t, dt):
    """fp32 CPU values as the operand type holds them."""
    return t.to(TORCH_DT[dt]).float()


class In:
    """[n][C] fp32 CPU values as device rows at pitch ld, `off` elements into the buffer; the pitch columns, the
    leading elements and four rows behind the last hold NaN."""

    def __init__(self, t, ld, dt, dev, off=0):
        n, C = t.shape
        assert ld >= C
        buf = torch.full((off + (n + 4) * ld,), NAN)
        buf[off:off + n * ld].view(n, ld)[:, :C] = t
        self.buf = buf.to(TORCH_DT[dt]).to(dev)
        self.ld = ld
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + off * self.buf.element_size())


class OutAt(Out):
    """Out whose first element sits `off` elements past the (16-byte aligned) start of the guarded span."""

    def __init__(self, shape, strides, dtype, dev, prefill=None, off=0):
        self.off = off
        super().__init__(shape, strides, dtype, dev, prefill)

    def view(self, buf):
        return buf.as_strided(self.shape, self.strides, self.guard + self.off)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + (self.guard + self.off) * self.buf.element_size())


def rows_out(n, C, ld, dt, dev, prefill=None, off=0):
    return OutAt((n, C), (ld, 1), TORCH_DT[dt] if isinstance(dt, str) else dt, dev, prefill, off)


def vec_out(n, dev, prefill=None):
    return Out((n,), (1,), torch.float32, dev, prefill)


def check(name, tensor, got, ref32, ref64):
    e = (got.double().cpu() - ref64).abs().max().item()
    e_ref = (ref32.double() - ref64).abs().max().item()
    print(f"\nBAR {name} {tensor} e_kernel {e:.3e} e_ref {e_ref:.3e} ratio {e / e_ref if e_ref else 0.0:.2f} "
          f"(|ref| max {ref64.abs().max().item():.3g})")
    assert e <= MARGIN * e_ref, (name, tensor, e, e_ref)


# ---- window attention -----------------------------------------------------------------------------------------------
PADS_DENSE = dict(q=0, kv=0, out=0, dout=0, dq=0, dkv=0)
PADS_PITCH = dict(q=3, kv=5, out=1, dout=7, dq=9, dkv=11)


def run_attn(env, case, dt, q, kv, dout, table, mask, scale, pads, accumulate=0, table0=None):
    """Forward and backward of one call; operands fp32 CPU.  -> out, dq, dkv, dtable (device)."""
    dev, lib = env.dev, env.lib
    n, C = case.B * case.Hr * case.Wr, case.heads * R.HD
    qd = In(q, C + pads["q"], dt, dev)
    kvd = In(kv, 2 * C + pads["kv"], dt, dev)
    dod = In(dout, C + pads["dout"], dt, dev)
    tab, idx = table.to(dev).contiguous(), R.rel_index().to(dev)
    md = None if mask is None else mask.to(dev).contiguous()
    P = env.native.WindowAttn(qd.ptr, qd.ld, kvd.ptr, kvd.ld, env.p(tab), env.p(idx), env.p(md), case.B, case.Hr, case.Wr,
                              case.heads, R.HD, R.WS, case.shift, scale)
    out = rows_out(n, C, C + pads["out"], dt, dev)
    lib.cai_window_attn_fwd(code(env, dt), ctypes.byref(P), out.ptr, C + pads["out"], env.stream())
    dq = rows_out(n, C, C + pads["dq"], dt, dev)
    dkv = rows_out(n, 2 * C, 2 * C + pads["dkv"], dt, dev)
    dtab = Out((49, case.heads), (case.heads, 1), torch.float32, dev, table0 if accumulate else None)
    ws, wsb = env.ws(lib.cai_window_attn_bwd_workspace_bytes(ctypes.byref(P)))
    lib.cai_window_attn_bwd(code(env, dt), ctypes.byref(P), dod.ptr, dod.ld, dq.ptr, C + pads["dq"], dkv.ptr,
                            2 * C + pads["dkv"], dtab.ptr, accumulate, env.p(ws), wsb, env.stream())
    torch.cuda.synchronize()
    what = f"attention {case.id} {dt}"
    return out.take(what), dq.take(what), dkv.take(what), dtab.take(what)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", T.AT_CASES, ids=[c.id for c in T.AT_CASES])
def test_attention_exact(env, case, dt):
    """Addressing (shift, windows, heads, pitches, the tail block) and the bias-gradient tree, bit for bit: with and
    without a per-window group mask, dense and pitched, overwriting and accumulating into an integer-filled table."""
    for zero in ("q", "k"):
        for masked, pads, acc in ((False, PADS_DENSE, 0), (True, PADS_PITCH, 1), (True, PADS_DENSE, 0),
                                  (False, PADS_PITCH, 1)):
            d = I.attn_exact(case, dt, zero, masked)
            out, dq, dkv, dtable = I.attn_exact_ref(case, d, torch.float32)
            if acc:
                dtable = dtable + d["table0"]
            got = run_attn(env, case, dt, d["q"], d["kv"], d["dout"], d["table"], d["mask"], I.ATTN_SCALE, pads, acc,
                           d["table0"])
            what = f"{case.id} {dt} zero {zero} mask {masked} pitched {pads is PADS_PITCH} accumulate {acc}"
            tdt = TORCH_DT[dt]
            for name, g, w in zip(("out", "dq", "dkv"), got, (out, dq, dkv)):
                assert_bits(g, w.to(tdt), f"{what}: {name}")
            assert_bits(got[3], dtable, f"{what}: dtable")


def _tol_attn(env, case, dt, table_pm8, pads):
    from compressai.models.master import _shifted_window_mask

    name = f"attn-tol-{case.id}-{dt}-{int(table_pm8)}"
    g = I.gen(name)
    n, C = case.B * case.Hr * case.Wr, case.heads * R.HD
    scale = R.HD ** -0.5
    # score = scale * q.k over 32 dims has deviation sigma^2: 7.5 puts the largest of a few thousand near 30
    sigma = 7.5 ** 0.5
    q, k = rnd(torch.randn(n, C, generator=g) * sigma, dt), rnd(torch.randn(n, C, generator=g) * sigma, dt)
    v, dout = rnd(torch.randn(n, C, generator=g), dt), rnd(torch.randn(n, C, generator=g), dt)
    kv = torch.cat([k, v], dim=1)
    if table_pm8:
        table = (torch.randint(0, 2, (49, case.heads), generator=g) * 16 - 8).float()
    else:
        table = torch.randn(49, case.heads, generator=g) * 0.5
    mask = _shifted_window_mask(case.Hr, case.Wr, R.WS, case.shift).float() if case.shift else None
    ref = {}
    for d in (torch.float32, torch.float64):
        ref[d] = R.window_attn_grads(q.to(d), kv.to(d), table.to(d), R.rel_index(), None if mask is None else mask.to(d),
                                     case.B, case.Hr, case.Wr, case.heads, case.shift, scale, dout.to(d))
    smax = (scale * (q.double().reshape(n, case.heads, R.HD) ** 2).sum(-1).sqrt().max()
            * (k.double().reshape(n, case.heads, R.HD) ** 2).sum(-1).sqrt().max()).item()
    print(f"\n{name}: |q||k| scale bound {smax:.1f}")
    got = run_attn(env, case, dt, q, kv, dout, table, mask, scale, pads)
    tdt = TORCH_DT[dt]
    split = lambda t: (t[0], t[1], t[2][:, :C], t[2][:, C:], t[3])
    for tensor, gt, r32, r64 in zip(("out", "dq", "dk", "dv", "dtable"), split(got), split(ref[torch.float32]),
                                    split(ref[torch.float64])):
        check(name, tensor, gt, r32 if tensor == "dtable" else r32.to(tdt), r64)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", T.AT_TOL, ids=[c.id for c in T.AT_TOL])
def test_attention_live_scores(env, case, dt):
    """|score| up to about 30, bias table N(0, 0.5), the model's -100 mask at shift 2 and none at shift 0."""
    _tol_attn(env, case, dt, False, PADS_PITCH if T.AT_TOL.index(case) % 2 else PADS_DENSE)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_attention_live_scores_table_pm8(env, dt):
    case = next(c for c in T.AT_TOL if c.id == T.AT_TOL_BIG_TABLE)
    _tol_attn(env, case, dt, True, PADS_PITCH)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------
def run_ln_bwd(env, case, dt, x, dy, w, mean, rstd, pad, acc=0, dw0=None, db0=None, want_dw=True, want_db=True):
    dev, lib = env.dev, env.lib
    n, C = case.ntok, case.C
    xd, gd = In(x, C + pad, dt, dev), In(dy, C + 2 * pad, dt, dev)
    wd, md, rd = w.to(dev), mean.to(dev), rstd.to(dev)
    dx = rows_out(n, C, C + 3 * pad, dt, dev)
    dw = vec_out(C, dev, dw0 if acc else None)
    db = vec_out(C, dev, db0 if acc else None)
    ws, wsb = env.ws(lib.cai_layernorm_bwd_workspace_bytes(n, C))
    lib.cai_layernorm_bwd(code(env, dt), xd.ptr, xd.ld, gd.ptr, gd.ld, n, C, env.p(wd), env.p(md), env.p(rd), dx.ptr,
                          C + 3 * pad, dw.ptr if want_dw else None, db.ptr if want_db else None, acc, env.p(ws), wsb,
                          env.stream())
    torch.cuda.synchronize()
    what = f"layernorm_bwd {case.id} {dt}"
    return dx.take(what), dw.take(what), db.take(what)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", T.LN_CASES, ids=[c.id for c in T.LN_CASES])
def test_layernorm_db_exact(env, case, dt):
    """db = sum dy over every block count of the table, overwritten and accumulated; a NULL dw or db leaves the
    other output's bits unchanged, and its unused (NaN-prefilled, sentinel-guarded) buffer untouched."""
    d = I.ln_db(case, dt)
    x = rnd(d["x"], dt)
    _, mean, rstd = R.layernorm_fwd(x.double(), d["w"].double(), torch.zeros(case.C, dtype=torch.float64), EPS)
    mean, rstd = mean.float(), rstd.float()
    want_db = d["dy"].sum(0)
    args = (env, case, dt, x, d["dy"], d["w"], mean, rstd)
    dx, dw, db = run_ln_bwd(*args, pad=0)
    assert_bits(db, want_db, f"{case.id} {dt}: db")
    assert not torch.isnan(dw).any() and not torch.isnan(dx.float()).any()
    dx1, dw1, db1 = run_ln_bwd(*args, pad=8, acc=1, dw0=d["dw0"], db0=d["db0"])
    assert_bits(db1, want_db + d["db0"], f"{case.id} {dt}: db accumulated")
    assert_bits(dw1, dw.cpu() + d["dw0"], f"{case.id} {dt}: dw accumulated")      # one fp32 add of the same sum
    assert_bits(dx1, dx, f"{case.id} {dt}: dx pitched")
    dx2, dw2, db2 = run_ln_bwd(*args, pad=0, want_dw=False)
    assert_bits(db2, db, f"{case.id} {dt}: db with dw NULL")
    assert torch.isnan(dw2).all(), "the unused dw buffer was written"
    dx3, dw3, db3 = run_ln_bwd(*args, pad=0, want_db=False)
    assert_bits(dw3, dw, f"{case.id} {dt}: dw with db NULL")
    assert torch.isnan(db3).all(), "the unused db buffer was written"
    assert_bits(dx2, dx, f"{case.id} {dt}: dx with dw NULL")
    assert_bits(dx3, dx, f"{case.id} {dt}: dx with db NULL")


LN_TOL = [(c, 0.0) for c in T.LN_CASES] + [(next(c for c in T.LN_CASES if c.id == T.LN_GENERAL_AT_96), 100.0)]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case,offset", LN_TOL, ids=[c.id + ("_mean100" if o else "") for c, o in LN_TOL])
def test_layernorm_tolerance(env, case, offset, dt):
    """y, mean, rstd, dx and dw against fp64, dense and pitched; weight in [0.5, 1.5]; one row has a token mean of
    about 100 times its spread.  The backward takes the reference's mean / rstd (rounded to fp32) on every side."""
    dev, lib = env.dev, env.lib
    n, C = case.ntok, case.C
    name = f"ln-{case.id}-{dt}" + ("-mean100" if offset else "")
    g = I.gen(name)
    x = rnd(torch.randn(n, C, generator=g) * (1.0 if offset else 2.0) + (offset if offset else 0.5), dt)
    dy = rnd(torch.randn(n, C, generator=g), dt)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    f64 = R.layernorm_fwd(x.double(), w.double(), b.double(), EPS)
    f32 = R.layernorm_fwd(x, w, b, EPS)
    mean, rstd = f64[1].float(), f64[2].float()
    b64 = R.layernorm_bwd(x.double(), dy.double(), w.double(), mean.double(), rstd.double())
    b32 = R.layernorm_bwd(x, dy, w, mean, rstd)
    tdt = TORCH_DT[dt]
    for pad in (0, 8):
        tag = f"{name}-{'pitched' if pad else 'dense'}"
        xd = In(x, C + pad, dt, dev)
        y = rows_out(n, C, C + 2 * pad, dt, dev)
        mo, ro = vec_out(n, dev), vec_out(n, dev)
        wd, bd = w.to(dev), b.to(dev)
        lib.cai_layernorm_fwd(code(env, dt), xd.ptr, xd.ld, n, C, env.p(wd), env.p(bd), EPS, y.ptr, C + 2 * pad, mo.ptr,
                              ro.ptr, env.stream())
        torch.cuda.synchronize()
        check(tag, "y", y.take(tag), f32[0].to(tdt), f64[0])
        check(tag, "mean", mo.take(tag), f32[1], f64[1])
        check(tag, "rstd", ro.take(tag), f32[2], f64[2])
        dx, dw, db = run_ln_bwd(env, case, dt, x, dy, w, mean, rstd, pad)
        check(tag, "dx", dx, b32[0].to(tdt), b64[0])
        check(tag, "dw", dw, b32[1], b64[1])


def test_layernorm_general_kernel_at_96(cuda):
    """CAI_LN_BWD_REG=0 (read once per process) sends C <= 128 to the general backward kernel: the C = 96 rows of the
    tolerance test, with the same bars, in a fresh child process."""
    envp = dict(os.environ, CAI_LN_BWD_REG="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-p", "no:cacheprovider",
                        "-k", f"test_layernorm_tolerance and {T.LN_GENERAL_AT_96}"], env=envp, capture_output=True,
                       text=True, timeout=300, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(r.stdout[-6000:].replace("BAR ln-", "BAR general-ln-"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "4 passed" in r.stdout, r.stdout[-3000:]


# ---- GELU -----------------------------------------------------------------------------------------------------------
GELU_BANDS = ((-8.0, -3.0), (-3.0, 3.0), (3.0, 8.0))
GELU_VARIANTS = [("f32", T.EW_CASES[0])] + [("bf16", c) for c in T.EW_CASES]


def run_gelu(env, dt, x, g, C, pad, off):
    dev, lib = env.dev, env.lib
    n = x.shape[0]
    ld = C + pad
    xd, gd = In(x, ld, dt, dev, off), In(g, ld, dt, dev, off)
    y, dx = rows_out(n, C, ld, dt, dev, off=off), rows_out(n, C, ld, dt, dev, off=off)
    lib.cai_gelu_fwd(code(env, dt), xd.ptr, ld, y.ptr, ld, n, C, env.stream())
    lib.cai_gelu_bwd(code(env, dt), xd.ptr, ld, gd.ptr, ld, dx.ptr, ld, n, C, env.stream())
    torch.cuda.synchronize()
    return y.take("gelu y"), dx.take("gelu dx")


@pytest.mark.parametrize("dt,case", GELU_VARIANTS, ids=[f"{d}-{c.id}" for d, c in GELU_VARIANTS])
def test_gelu_per_band(env, dt, case):
    """Forward and backward over [-8, -3], [-3, 3] and [3, 8] separately, so that the negative tail (|y| ~ 1e-6 at
    x = -5) is measured against its own e_ref: fp32, the bf16 vector kernel and its three scalar fallbacks."""
    n = 8 * case.rows
    tdt = TORCH_DT[dt]
    for lo, hi in GELU_BANDS:
        name = f"gelu-{dt}-{case.id}[{lo:g},{hi:g}]"
        g = I.gen(name)
        x = rnd(torch.rand(n, case.C, generator=g) * (hi - lo) + lo, dt)
        gy = rnd(torch.randn(n, case.C, generator=g), dt)
        y, dx = run_gelu(env, dt, x, gy, case.C, case.pad, case.off)
        check(name, "y", y, R.gelu_fwd(x).to(tdt), R.gelu_fwd(x.double()))
        check(name, "dx", dx, R.gelu_bwd(x, gy).to(tdt), R.gelu_bwd(x.double(), gy.double()))


@pytest.mark.parametrize("row", list(T.EW_STRIDE))
def test_gelu_grid_stride(env, row):
    """More than 16384 * 256 work items: the second pass of the grid-stride loop (scalar fp32, vector bf16, and
    scalar bf16 at C % 8 != 0)."""
    n, C = T.EW_STRIDE[row]
    dt = row.split("-")[0]
    name = f"gelu-stride-{row}"
    g = I.gen(name)
    x = rnd(torch.rand(n, C, generator=g) * 16 - 8, dt)
    gy = rnd(torch.randn(n, C, generator=g), dt)
    y, dx = run_gelu(env, dt, x, gy, C, 0, 0)
    tdt = TORCH_DT[dt]
    check(name, "y", y, R.gelu_fwd(x).to(tdt), R.gelu_fwd(x.double()))
    check(name, "dx", dx, R.gelu_bwd(x, gy).to(tdt), R.gelu_bwd(x.double(), gy.double()))


# ---- channel mean ---------------------------------------------------------------------------------------------------
CM_RUNS = [(c, dt) for c in T.CM_CASES for dt in c.dtypes]


@pytest.mark.parametrize("case,dt", CM_RUNS, ids=[f"{c.id}-{d}" for c, d in CM_RUNS])
def test_channel_mean_exact(env, case, dt):
    """sum_p x and sum_p x * x2 (different pitches) of lattice values, scale 1 and 1 / HW: the integer sum times
    the scale, one fp32 multiply."""
    dev, lib = env.dev, env.lib
    B, HW, C = case.B, case.HW, case.C
    d = I.channel_mean(case, dt)
    vec = 8 if dt == "bf16" else 4
    ld = (C + vec - 1) // vec * vec
    xd = In(d["x"].reshape(B * HW, C), ld + vec, dt, dev)
    x2d = In(d["x2"].reshape(B * HW, C), ld + 3 * vec, dt, dev)
    for use2 in (False, True):
        s = R.channel_mean(d["x"], d["x2"] if use2 else None, 1.0)
        for scale in (1.0, 1.0 / HW):
            out = Out((B, C), (C, 1), torch.float32, dev)
            ws, wsb = env.ws(lib.cai_channel_mean_workspace_bytes(B, HW, C))
            lib.cai_channel_mean(code(env, dt), xd.ptr, xd.ld, x2d.ptr if use2 else None, x2d.ld if use2 else 0, B, HW, C,
                                 out.ptr, scale, env.p(ws), wsb, env.stream())
            torch.cuda.synchronize()
            what = f"channel_mean {case.id} {dt} x2 {use2} scale {scale:g}"
            assert_bits(out.take(what), s * torch.tensor(scale, dtype=torch.float32), what)


# ---- channel affine -------------------------------------------------------------------------------------------------
def run_affine(env, dt, d, B, HW, C, pad, off, beta_scale, use_gamma, use_beta, what):
    dev, lib = env.dev, env.lib
    ld = C + pad
    xd = In(d["x"].reshape(B * HW, C), ld, dt, dev, off) if use_gamma else None
    ga, be = d["gamma"].to(dev), d["beta"].to(dev)
    y = rows_out(B * HW, C, ld, dt, dev, off=off)
    lib.cai_channel_affine(code(env, dt), xd.ptr if use_gamma else None, ld if use_gamma else 0,
                           env.p(ga) if use_gamma else None, env.p(be) if use_beta else None, beta_scale, y.ptr, ld, B,
                           HW, C, env.stream())
    torch.cuda.synchronize()
    want = R.channel_affine(d["x"], d["gamma"] if use_gamma else None, d["beta"] if use_beta else None, beta_scale, HW)
    assert_bits(y.take(what), want.reshape(B * HW, C).to(TORCH_DT[dt]), what)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", T.EW_CASES, ids=[c.id for c in T.EW_CASES])
def test_channel_affine_exact(env, case, dt):
    """y = gamma * x + beta_scale * beta on the lattice: both NULL forms, B 1 and 3 (the per-image gamma / beta row),
    beta_scale 1, 0.5 and 0, the bf16 vector kernel and each scalar fallback."""
    for B in T.AFFINE_B:
        d = I.channel_affine(B, T.AFFINE_HW, case.C, dt, case.id)
        for bs in T.AFFINE_BETA_SCALE:
            for use_gamma, use_beta in ((True, True), (False, True), (True, False)):
                run_affine(env, dt, d, B, T.AFFINE_HW, case.C, case.pad, case.off, bs, use_gamma, use_beta,
                           f"affine {case.id} {dt} B {B} beta_scale {bs} gamma {use_gamma} beta {use_beta}")


@pytest.mark.parametrize("row", list(T.EW_STRIDE))
def test_channel_affine_grid_stride(env, row):
    n, C = T.EW_STRIDE[row]
    dt = row.split("-")[0]
    B, HW = 2, n // 2
    d = I.channel_affine(B, HW, C, dt, "stride")
    run_affine(env, dt, d, B, HW, C, 0, 0, 0.5, True, True, f"affine grid-stride {row}")
