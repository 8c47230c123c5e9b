"""The rate path per element, in the log domain, against an fp64 oracle.

The rate term is sum(-log2(likelihood)); a tail symbol costs 10-30 bits, so a likelihood error that a max-norm
comparison cannot see (1e-4 absolute at a likelihood of 1e-5) is bits on that symbol.  Every case here runs

  * the kernel (through the product modules),
  * the fp64 oracle (``copy.deepcopy(oracle).double()`` on ``x.double()`` and the same noise): the reference,
  * the fp32 CPU oracle on the same inputs: the reference's own error ``e_ref``,

on deterministic ladders that reach the tails (GaussianConditional: 0 ... 6.5 sigma; EntropyBottleneck:
|x - median| up to R = 200, likelihoods down to the 1e-9 bound), and prints ``RATEPATH <case> e_k=... e_ref=...``
before it asserts.

Metrics: ``bits_err`` = max |log2(lik) - log2(lik64)| over elements whose fp64 clamped likelihood is above 4e-9;
``elem_rel`` = max |g - g64| / max(|g64|, 1e-3 max|g64|); parameter gradients in per-tensor max norm.

Bars (BARS below): twice the ``e_k`` measured on one MI355X, rounded up to one significant digit (the table is in
DESIGN.md section 3, the run in profiles/rate_path_bars.log).  Ceilings, which no bar may exceed: likelihoods 1e-3
bits per element (the project's 1e-4 relative bpp promise at the symbol level); gradients max(10 e_ref, 2e-3).
A gradient stored in bf16 gets one bf16 rounding, 2^-8, on top of the bar of its fp32 sibling case.  The RD sums
use max(1e-5, 4 x the error of torch's own fp32 CPU sum of the same data).

LowerBound masks (likelihood clamp, gradient masks): elements whose fp64 raw likelihood is within 0.1 % of the bound
are left out, and so are scale gradients whose raw scale is within 0.1 % of 0.11; each set is asserted to hold at
most 1 % of the elements.
"""
import copy
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import cai_oracle as O

pytestmark = pytest.mark.gpu

LIK_BOUND32 = torch.tensor(1e-9, dtype=torch.float32)      # what the kernels and the oracle's buffer hold
LIK_BOUND = float(LIK_BOUND32.double())
SCALE_BOUND = float(torch.tensor(0.11, dtype=torch.float32).double())
KEEP = 4e-9
BAND = 1e-3
BAND_CAP = 0.01
LIK_CEIL = 1e-3            # bits per element
GRAD_FLOOR = 2e-3          # the project's gradient bar
BF16_ROUND = 2.0 ** -8
FP32_ROUND = 2.0 ** -24

# case -> bar: 2 x the e_k measured on an MI355X (profiles/rate_path_bars.log), rounded up to one digit
BARS = {
    "gc_fwd[eval-fp32]": 2e-05,
    "gc_fwd[eval-sm_bf16]": 2e-05,
    "gc_fwd[eval-bf16]": 2e-05,
    "gc_fwd[eval_means-fp32]": 2e-05,
    "gc_fwd[eval_means-sm_bf16]": 2e-05,
    "gc_fwd[eval_means-bf16]": 2e-05,
    "gc_fwd[train-fp32]": 2e-05,
    "gc_fwd[train-sm_bf16]": 2e-05,
    "gc_fwd[train-bf16]": 2e-05,
    "gc_bwd_rate[train-fp32].dx": 9e-06,
    "gc_bwd_rate[train-fp32].ds": 3e-05,
    "gc_bwd_rate[train-fp32].dm": 9e-06,
    "gc_bwd_rate[train-sm_bf16].dx": 2e-05,
    "gc_bwd_mixed[train-fp32].dx": 8e-06,
    "gc_bwd_mixed[train-fp32].ds": 0.0001,
    "gc_bwd_mixed[train-fp32].dm": 8e-06,
    "gc_bwd_relu[train-fp32].dx": 2e-05,
    "gc_bwd_relu[train-fp32].ds": 3e-05,
    "gc_bwd_relu[train-fp32].dm": 2e-05,
    "gc_bwd_paired[train-fp32].dx": 9e-06,
    "gc_bwd_paired[train-fp32].ds": 3e-05,
    "gc_bwd_paired[train-fp32].dm": 9e-06,
    "eb_fwd[small-eval]": 0.0001,
    "eb_fwd[small-train]": 0.0002,
    "eb_fwd[split-eval]": 0.0002,
    "eb_fwd[split-train]": 0.0002,
    "eb_fwd[small-train-bf16]": 0.0001,
    "eb_bwd_rate[small-eval].dx": 0.0,
    "eb_bwd_rate[small-eval].params": 4e-05,
    "eb_bwd_rate[small-train].dx": 0.002,
    "eb_bwd_rate[small-train].params": 5e-05,
    "eb_bwd_rate[split-eval].dx": 0.0,
    "eb_bwd_rate[split-eval].params": 2e-05,
    "eb_bwd_rate[split-train].dx": 0.002,
    "eb_bwd_rate[split-train].params": 9e-06,
    "eb_bwd_rate[small-train-bf16].params": 5e-05,
}


# ------------------------------------------------------------------------------------------------ metrics

def _cpu64(t):
    return t.detach().double().cpu()


def bits_err(lik, lik64):
    """max |log2 lik - log2 lik64| over the elements whose fp64 (clamped) likelihood is above 4e-9"""
    keep = lik64 > KEEP
    assert keep.any()
    return (torch.log2(_cpu64(lik)) - torch.log2(lik64)).abs()[keep].max().item()


def elem_rel(g, g64, keep=None):
    """max |g - g64| / max(|g64|, 1e-3 max|g64|); an all-zero reference asks for exact zeros"""
    g, g64 = _cpu64(g), _cpu64(g64)
    top = g64.abs().max().item()
    if top == 0.0:
        return 0.0 if g.abs().max().item() == 0.0 else math.inf
    e = (g - g64).abs() / g64.abs().clamp_min(1e-3 * top)
    if keep is not None:
        e = e[keep]
    return e.max().item()


def max_rel(g, g64):
    g, g64 = _cpu64(g), _cpu64(g64)
    top = g64.abs().max().item()
    return (g - g64).abs().max().item() / (top if top > 0 else 1.0)


def _report(case, e_k, e_ref):
    print(f"\nRATEPATH {case} e_k={e_k:.3e} e_ref={e_ref:.3e}")


def _check(case, e_k, e_ref, ceiling, extra=0.0, bar_case=None):
    """print, then assert e_k against the recorded bar (+ extra: a derivable rounding on top) and the bar
    against its ceiling"""
    _report(case, e_k, e_ref)
    bar = BARS[bar_case or case]
    assert bar <= ceiling, (case, bar, ceiling)
    assert e_k <= bar + extra, (case, e_k, bar + extra, e_ref)


def _grad_ceiling(e_ref):
    return max(10.0 * e_ref, GRAD_FLOOR)


def _bf16r(t):
    return t.bfloat16().float()


def _noise_feed(tensors):
    q = list(tensors)
    return lambda x: q.pop(0)


def _lik_masks(raw64):
    """(band, clamped): within 0.1 % of the likelihood bound / below it"""
    band = (raw64 / LIK_BOUND - 1.0).abs() < BAND
    assert band.double().mean().item() <= BAND_CAP
    return band, (raw64 < LIK_BOUND) & ~band


def _scale_band(s):
    band = (s.double() / SCALE_BOUND - 1.0).abs() < BAND
    assert band.double().mean().item() <= BAND_CAP
    return band


# ------------------------------------------------------------------------------------------------ GaussianConditional

GC_SHAPE = (2, 24, 7, 5)        # C = 24: no multiple of 32; 1680 elements
GC_DTYPES = {"fp32": (torch.float32, torch.float32), "sm_bf16": (torch.float32, torch.bfloat16),
             "bf16": (torch.bfloat16, torch.bfloat16)}
GC_MODES = {"eval": (False, False), "eval_means": (False, True), "train": (True, True)}


@functools.lru_cache(maxsize=None)
def _gc_inputs(shape, dt, with_means, relu=False, seed=11):
    """The ladder: scales = rand * 3 with one channel at 0.01 (relu: relu(pre), ~20 % of pre non-positive, exact
    zeros among them), means = randn, x = means +- k max(scales, 0.11), k a shuffled linspace(0, 6.5).  bf16
    operands are rounded here, so the oracles see exactly the kernel's values."""
    xdt, smdt = GC_DTYPES[dt]
    g = torch.Generator().manual_seed(seed)
    n = math.prod(shape)
    s = torch.rand(shape, generator=g) * 3
    if relu:
        s = s - 0.6
        s[:, 1] = 0.0
    s[:, 3] = 0.01
    m = torch.randn(shape, generator=g)
    if smdt == torch.bfloat16:
        s, m = _bf16r(s), _bf16r(m)
    k = torch.linspace(0, 6.5, n)[torch.randperm(n, generator=g)].reshape(shape)
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    x = (m if with_means else 0) + sign * k * torch.relu(s).clamp_min(0.11)
    if xdt == torch.bfloat16:
        x = _bf16r(x)
    noise = torch.empty(shape).uniform_(-0.5, 0.5, generator=g)
    return SimpleNamespace(x=x, s=s, m=m if with_means else None, noise=noise, relu=relu, xdt=xdt, smdt=smdt)


def _gc_oracle(inp, training, dtype):
    """the CPU oracle in `dtype`; leaves and outputs keep their graph (callers use autograd.grad, which leaves
    them unchanged)"""
    mod = O.GaussianConditional(None).train(training)
    if dtype == torch.float64:
        mod = copy.deepcopy(mod).double()
    x = inp.x.clone().to(dtype).requires_grad_()
    s_leaf = inp.s.clone().to(dtype).requires_grad_()
    s = torch.relu(s_leaf) if inp.relu else s_leaf
    m = inp.m.clone().to(dtype).requires_grad_() if inp.m is not None else None
    with O.NoiseFeed([inp.noise.to(dtype)] if training else []):
        q, lik = mod(x, s, m)
    with torch.no_grad():
        raw = mod._likelihood(q, s, m)
    leaves = [x, s_leaf] + ([m] if m is not None else [])
    return SimpleNamespace(q=q.detach(), lik=lik, raw=raw, leaves=leaves, s=s.detach())


@functools.lru_cache(maxsize=None)
def _gc_refs(shape, dt, mode, relu=False):
    training, with_means = GC_MODES[mode]
    inp = _gc_inputs(shape, dt, with_means, relu)
    return inp, _gc_oracle(inp, training, torch.float64), _gc_oracle(inp, training, torch.float32)


def _grads(o, upstream=None):
    """d sum(-log2 lik) (the rate) or d sum(lik * upstream) with respect to the oracle's leaves"""
    loss = (-torch.log2(o.lik)).sum() if upstream is None else (o.lik * upstream.to(o.lik.dtype)).sum()
    return [g.detach() for g in torch.autograd.grad(loss, o.leaves, retain_graph=True)]


def _gc_device(cuda, inp, training):
    from compressai.entropy_models import GaussianConditional, set_noise_source

    mod = GaussianConditional(None).to(cuda).train(training)
    xd = inp.x.to(cuda, inp.xdt).requires_grad_()
    sd = (torch.relu(inp.s) if inp.relu else inp.s).to(cuda, inp.smdt).requires_grad_()
    md = inp.m.to(cuda, inp.smdt).requires_grad_() if inp.m is not None else None
    set_noise_source(_noise_feed([inp.noise]))
    try:
        q, lik = mod(xd, sd, md, scales_relu=inp.relu)
    finally:
        set_noise_source(None)
    return SimpleNamespace(q=q, lik=lik, leaves=[xd, sd] + ([md] if md is not None else []))


def _rate_backward(lik):
    (-torch.log2(lik)).sum().backward()


@pytest.mark.parametrize("dt", list(GC_DTYPES))
@pytest.mark.parametrize("mode", list(GC_MODES))
def test_gc_forward(cuda, mode, dt):
    training = GC_MODES[mode][0]
    inp, r64, r32 = _gc_refs(GC_SHAPE, dt, mode)
    d = _gc_device(cuda, inp, training)
    lik64 = r64.lik.detach()
    band, clamped = _lik_masks(r64.raw)
    assert d.lik.dtype == torch.float32
    _check(f"gc_fwd[{mode}-{dt}]", bits_err(d.lik, lik64), bits_err(r32.lik, lik64), LIK_CEIL)
    assert clamped.any()                                   # the ladder reaches the bound
    assert torch.equal(d.lik.detach().cpu()[clamped], LIK_BOUND32.expand(int(clamped.sum())))
    q = d.q.detach().cpu()
    assert q.dtype == inp.xdt
    if training:        # x + noise: one rounding of the operand dtype
        u = BF16_ROUND if inp.xdt == torch.bfloat16 else FP32_ROUND
        assert ((q.double() - r64.q).abs() <= u * r64.q.abs()).all()
    else:               # round-to-index: bit-exact
        assert torch.equal(r32.q, r64.q.float())           # the same index in fp32 and fp64: no rounding tie
        assert torch.equal(q, r32.q.to(inp.xdt))


def _gc_grad_checks(case, d, r64, r32, inp, g64, g32, bar_case=None):
    band, _ = _lik_masks(r64.raw)
    sband = _scale_band(r64.s)
    names = ["dx", "ds"] + (["dm"] if inp.m is not None else [])
    for i, (name, leaf) in enumerate(zip(names, d.leaves)):
        keep = ~band & ~sband if name == "ds" else ~band
        assert leaf.grad.dtype == leaf.dtype
        e_ref = elem_rel(g32[i], g64[i], keep)
        bf16_store = leaf.dtype == torch.bfloat16
        extra = BF16_ROUND if bf16_store else 0.0
        # a bf16 store: the fp32 sibling's bar plus one bf16 rounding
        bc = f"{bar_case or case}.{name}"
        if bf16_store:
            bc = bc.replace("-sm_bf16", "-fp32").replace("-bf16", "-fp32")
        _check(f"{case}.{name}", elem_rel(leaf.grad, g64[i], keep), e_ref, _grad_ceiling(e_ref), extra, bc)


@pytest.mark.parametrize("dt", list(GC_DTYPES))
def test_gc_backward_rate(cuda, dt):
    """gc_bwd_kernel under the rate upstream -1 / (lik ln 2), formed with torch ops on the op's output"""
    inp, r64, r32 = _gc_refs(GC_SHAPE, dt, "train")
    d = _gc_device(cuda, inp, True)
    _rate_backward(d.lik)
    _gc_grad_checks(f"gc_bwd_rate[train-{dt}]", d, r64, r32, inp, _grads(r64), _grads(r32))


def test_gc_backward_mixed_sign(cuda):
    """gl = randn: both branches of the two LowerBound rules (x >= bound or g < 0)"""
    inp, r64, r32 = _gc_refs(GC_SHAPE, "fp32", "train")
    gl = torch.randn(GC_SHAPE, generator=torch.Generator().manual_seed(12))
    _, clamped = _lik_masks(r64.raw)
    assert (clamped & (gl > 0)).any() and (clamped & (gl < 0)).any()
    d = _gc_device(cuda, inp, True)
    d.lik.backward(gl.to(cuda))
    _gc_grad_checks("gc_bwd_mixed[train-fp32]", d, r64, r32, inp, _grads(r64, gl), _grads(r32, gl))


def test_gc_backward_scales_relu(cuda):
    """scales = relu(pre): the op returns d pre (its ds, already masked by the ReLU's backward)"""
    inp, r64, r32 = _gc_refs(GC_SHAPE, "fp32", "train", True)
    nonpos = (inp.s <= 0).float().mean().item()
    assert 0.1 < nonpos < 0.35 and (inp.s == 0).any() and (inp.s < 0).any()
    d = _gc_device(cuda, inp, True)
    _rate_backward(d.lik)
    assert (d.leaves[1].grad.cpu()[inp.s <= 0] == 0).all()
    _gc_grad_checks("gc_bwd_relu[train-fp32]", d, r64, r32, inp, _grads(r64), _grads(r32))


PAIRED = {"fp32": ((2, 24, 7, 5), torch.float32), "bf16": ((1, 192, 4, 4), torch.bfloat16)}


@pytest.mark.parametrize("dt", list(PAIRED))
def test_gc_backward_paired(cuda, dt):
    """scales, means = the halves of one pixel-major [B, 2C, H, W] tensor (MeanScaleHyperprior.forward): the op
    writes both gradients into one [pixels][2C] buffer, which the chunk op's backward hands back whole"""
    from compressai._ops import ChunkFn
    from compressai.entropy_models import GaussianConditional, set_noise_source

    shape, tdt = PAIRED[dt]
    B, C, H, W = shape
    inp, r64, r32 = _gc_refs(shape, dt, "train")
    params = torch.cat([inp.s, inp.m], 1)
    pd = params.to(cuda, tdt).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_()
    xd = inp.x.to(cuda, tdt).requires_grad_()
    mod = GaussianConditional(None).to(cuda).train(True)
    set_noise_source(_noise_feed([inp.noise]))
    try:
        sd, md = ChunkFn.apply(pd)
        q, lik = mod(xd, sd, md)
    finally:
        set_noise_source(None)
    assert lik.grad_fn.paired is True
    _rate_backward(lik)
    assert pd.grad.shape == pd.shape and pd.grad.dtype == tdt
    d = SimpleNamespace(leaves=[xd, SimpleNamespace(grad=pd.grad[:, :C], dtype=tdt),
                                SimpleNamespace(grad=pd.grad[:, C:], dtype=tdt)])
    _gc_grad_checks(f"gc_bwd_paired[train-{dt}]", d, r64, r32, inp, _grads(r64), _grads(r32),
                    bar_case="gc_bwd_paired[train-fp32]")


# ------------------------------------------------------------------------------------------------ EntropyBottleneck

EB_C = 40                  # two 32-channel table blocks, the second partial
EB_R = 200.0               # picked once on the CPU: see _eb_inputs
EB_SHAPES = {"small": (3, EB_C, 6, 5),       # one backward block per channel
             "split": (2, EB_C, 24, 24)}     # 1152 pixels per channel: the split backward, ticket hand-off
EB_CASES = [("small", False, False), ("small", True, False), ("split", False, False), ("split", True, False),
            ("small", True, True)]
EB_IDS = [f"{s}-{'train' if t else 'eval'}{'-bf16' if b else ''}" for s, t, b in EB_CASES]
EB_PARAMS = ([f"_matrix{i}" for i in range(5)] + [f"_bias{i}" for i in range(5)]
             + [f"_factor{i}" for i in range(4)] + ["quantiles"])


@functools.lru_cache(maxsize=None)
def _eb_inputs(shape_key, bf16):
    """x = shuffled linspace(-R, R) over the pixels + rand, broadcast over the channels; the module gets the
    0.1 randn parameter perturbation of test_kernels_gpu.py::test_entropy_bottleneck.  R = 200 puts the fp64 raw
    likelihood below the 1e-9 bound for a share of the elements that the tests assert to lie in [2 %, 15 %]."""
    shape = EB_SHAPES[shape_key]
    B, C, H, W = shape
    g = torch.Generator().manual_seed(1)
    ref = O.EntropyBottleneck(C)
    with torch.no_grad():
        for p in ref.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    npix = B * H * W
    base = torch.linspace(-EB_R, EB_R, npix)[torch.randperm(npix, generator=g)].reshape(B, 1, H, W)
    x = base + torch.rand(shape, generator=g)
    # eval mode rounds x - median: an element within 1e-3 of a half-integer there could round to another index in
    # fp32 than in fp64 (the subtraction's rounding), so it is moved 0.01 away; ties themselves are the quantize
    # tests' business, bit-exactly
    d = x.double() - ref.quantiles.detach().double()[:, 0, 1].reshape(1, C, 1, 1)
    x = torch.where(((d - torch.floor(d)) - 0.5).abs() < 1e-3, x + 0.01, x)
    if bf16:
        x = _bf16r(x)
    noise = torch.empty(shape).uniform_(-0.5, 0.5, generator=g)
    return SimpleNamespace(ref=ref, x=x, noise=noise, xdt=torch.bfloat16 if bf16 else torch.float32)


def _eb_oracle(inp, training, dtype):
    mod = copy.deepcopy(inp.ref).train(training)
    if dtype == torch.float64:
        mod = mod.double()
    x = inp.x.clone().to(dtype).requires_grad_()
    with O.NoiseFeed([inp.noise.to(dtype)] if training else []):
        q, lik = mod(x)
    with torch.no_grad():
        C = x.shape[1]
        raw = mod._likelihood(q.transpose(0, 1).reshape(C, 1, -1))
        raw = raw.reshape(C, x.shape[0], *x.shape[2:]).transpose(0, 1)
    return SimpleNamespace(mod=mod, x=x, q=q.detach(), lik=lik, raw=raw)


@functools.lru_cache(maxsize=None)
def _eb_refs(shape_key, training, bf16):
    inp = _eb_inputs(shape_key, bf16)
    out = []
    for dtype in (torch.float64, torch.float32):
        o = _eb_oracle(inp, training, dtype)
        (-torch.log2(o.lik)).sum().backward()
        o.lik = o.lik.detach()
        out.append(o)
    share = (out[0].raw < LIK_BOUND).double().mean().item()
    assert 0.02 <= share <= 0.15, share          # the ladder still reaches the bound
    return inp, out[0], out[1]


def _eb_device(cuda, inp, training):
    from compressai.entropy_models import EntropyBottleneck, set_noise_source

    mod = EntropyBottleneck(EB_C)
    mod.load_state_dict(inp.ref.state_dict())
    mod = mod.to(cuda).train(training)

    def run():
        mod.zero_grad()
        xd = inp.x.to(cuda, inp.xdt).requires_grad_()
        set_noise_source(_noise_feed([inp.noise]))
        try:
            q, lik = mod(xd)
        finally:
            set_noise_source(None)
        return xd, q, lik

    return mod, run


@pytest.mark.parametrize("shape_key,training,bf16", EB_CASES, ids=EB_IDS)
def test_eb_forward(cuda, shape_key, training, bf16):
    inp, r64, r32 = _eb_refs(shape_key, training, bf16)
    _, run = _eb_device(cuda, inp, training)
    _, q, lik = run()
    band, clamped = _lik_masks(r64.raw)
    case = f"eb_fwd[{EB_IDS[EB_CASES.index((shape_key, training, bf16))]}]"
    _check(case, bits_err(lik, r64.lik), bits_err(r32.lik, r64.lik), LIK_CEIL)
    assert clamped.any()
    assert torch.equal(lik.detach().cpu()[clamped], LIK_BOUND32.expand(int(clamped.sum())))
    q = q.detach().cpu()
    if training:
        u = BF16_ROUND if bf16 else FP32_ROUND
        assert ((q.double() - r64.q).abs() <= u * r64.q.abs()).all()
    else:
        assert torch.equal(r32.q, r64.q.float())
        assert torch.equal(q, r32.q.to(inp.xdt))


@pytest.mark.parametrize("shape_key,training,bf16", EB_CASES, ids=EB_IDS)
def test_eb_backward_rate(cuda, shape_key, training, bf16):
    inp, r64, r32 = _eb_refs(shape_key, training, bf16)
    mod, run = _eb_device(cuda, inp, training)
    xd, _, lik = run()
    _rate_backward(lik)
    band, _ = _lik_masks(r64.raw)
    case = f"eb_bwd_rate[{EB_IDS[EB_CASES.index((shape_key, training, bf16))]}]"
    assert xd.grad.dtype == inp.xdt
    e_ref = elem_rel(r32.x.grad, r64.x.grad, ~band)
    _check(f"{case}.dx", elem_rel(xd.grad, r64.x.grad, ~band), e_ref, _grad_ceiling(e_ref),
           BF16_ROUND if bf16 else 0.0, f"{case.replace('-bf16', '')}.dx")
    # the 14 parameter gradients, and quantiles where the oracle gives one, in one per-tensor max-norm figure
    e_k = e_ref = 0.0
    for n in EB_PARAMS:
        g, g64, g32 = getattr(mod, n).grad, getattr(r64.mod, n).grad, getattr(r32.mod, n).grad
        if g64 is None:
            assert g is None or g.abs().max().item() == 0, n
            continue
        assert g is not None and torch.isfinite(g).all(), n
        e_k, e_ref = max(e_k, max_rel(g, g64)), max(e_ref, max_rel(g32, g64))
    _check(f"{case}.params", e_k, e_ref, _grad_ceiling(e_ref))
    # determinism (the split backward's hand-off): the same bits on a second pass
    first = [getattr(mod, n).grad.clone() for n in EB_PARAMS if getattr(mod, n).grad is not None] + [xd.grad.clone()]
    xd2, _, lik2 = run()
    _rate_backward(lik2)
    second = [getattr(mod, n).grad for n in EB_PARAMS if getattr(mod, n).grad is not None] + [xd2.grad]
    assert len(first) == len(second) and all(torch.equal(a, b) for a, b in zip(first, second))


# ------------------------------------------------------------------------------------------------ RD loss

RD_Q = 3
RD_XSHAPE = (3, 4, 257, 129)
RD_BIG = (2, 26, 160, 256)           # 2 129 920 elements, n % 4 == 0: rd_sum's 4x-unrolled body runs
RD_TAIL = 1_000_003                  # n % 4 == 3
RD_UNALIGNED = 200_003
RD_SETS = {1: ("big",), 2: ("tail", "five"), 3: ("big", "unaligned", "five"),
           4: ("big", "tail", "five", "unaligned")}


def _loguniform(shape, g):
    return torch.pow(10.0, -9.0 * torch.rand(shape, generator=g)).clamp_(1e-9, 1.0)


@functools.lru_cache(maxsize=None)
def _rd_data():
    g = torch.Generator().manual_seed(7)
    return SimpleNamespace(x=torch.rand(RD_XSHAPE, generator=g), xh=torch.rand(RD_XSHAPE, generator=g),
                           big=_loguniform(RD_BIG, g), tail=_loguniform((1, RD_TAIL, 1, 1), g),
                           five=_loguniform((1, 5, 1, 1), g), unaligned=_loguniform((1, RD_UNALIGNED, 1, 1), g),
                           strided=_loguniform((2, 24, 9, 7), g))


def _rd_ref(xh, x, liks):
    """fp64 {loss, mse, bpp}, gradients, and the relative error of torch's own fp32 CPU sums of the same data"""
    from compressai.losses import LMBDA

    N, _, H, W = x.shape
    npix = N * H * W
    sums = [torch.log(l.double()).sum().item() for l in liks]
    coef = 1.0 / (-math.log(2) * npix)
    bpp = sum(sums) * coef
    diff = xh.double() - x.double()
    mse = (diff * diff).mean().item()
    lmbda = float(LMBDA[RD_Q])
    s32 = sum(torch.log(l).sum().item() for l in liks)
    e_sum = abs(s32 - sum(sums)) / abs(sum(sums))
    d32 = xh - x
    e_sq = abs((d32 * d32).sum().item() - (diff * diff).sum().item()) / (diff * diff).sum().item()
    return SimpleNamespace(loss=lmbda * mse + bpp, mse=mse, bpp=bpp, coef=coef, e_sum=max(e_sum, e_sq),
                           dxh=lmbda * 2.0 * diff / diff.numel(), dliks=[coef / l.double() for l in liks])


def _pixel_major(t, cuda):
    """the layout of the product's own likelihood outputs: [B, C, H, W] over a [B, H, W, C] buffer"""
    return t.to(cuda).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _rd_device_liks(names, cuda):
    D = _rd_data()
    out = []
    for n in names:
        t = getattr(D, n)
        if n == "unaligned":     # storage one float past a 16-byte boundary: rd_sum's scalar path
            buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=cuda)
            v = buf[1:1 + t.numel()].reshape(t.shape)
            v.copy_(t)
            assert v.data_ptr() % 16 == 4
        elif n == "strided":     # ld = 40 > C = 24: a channel slice of a pixel-major buffer
            B, C, H, W = t.shape
            buf = torch.ones((B, H, W, 40), dtype=torch.float32, device=cuda)
            v = buf.permute(0, 3, 1, 2)[:, :C]
            v.copy_(t)
        else:
            v = _pixel_major(t, cuda)
        out.append(v.requires_grad_())
    return out


def _rd_check(case, cd, ref, xhd, liks_d, liks):
    bar = max(1e-5, 4.0 * ref.e_sum)
    print(f"\nRATEPATH {case} torch_fp32_sum_err={ref.e_sum:.3e} bar={bar:.3e}")
    for k, want in (("loss", ref.loss), ("mse_loss", ref.mse), ("bpp_loss", ref.bpp)):
        got = cd[k].item()
        print(f"RATEPATH {case}.{k} e_k={abs(got - want) / max(1.0, abs(want)):.3e}")
        assert abs(got - want) <= bar * max(1.0, abs(want)), (k, got, want)
    for ld, l, want in zip(liks_d, liks, ref.dliks):      # coef / lik: one fp32 divide and one multiply
        assert ld.grad.shape == l.shape
        assert ((_cpu64(ld.grad) - want).abs() <= 1e-6 * want.abs()).all()
    assert elem_rel(xhd.grad, ref.dxh) <= 1e-6


@pytest.mark.parametrize("nlik", [1, 2, 3, 4])
def test_rd_loss_fused(cuda, nlik):
    from compressai.losses import RateDistortionLoss

    D = _rd_data()
    names = RD_SETS[nlik]
    liks = [getattr(D, n) for n in names]
    ref = _rd_ref(D.xh, D.x, liks)
    liks_d = _rd_device_liks(names, cuda)
    xhd = D.xh.to(cuda).requires_grad_()
    cd = RateDistortionLoss(RD_Q)({"x_hat": xhd, "likelihoods": dict(zip(names, liks_d))}, D.x.to(cuda))
    if "unaligned" in names:     # the buffer the kernel read (saved for backward) is the unaligned view itself
        saved = cd["loss"].grad_fn.saved_tensors[2 + names.index("unaligned")]
        assert saved.data_ptr() == liks_d[names.index("unaligned")].data_ptr() and saved.data_ptr() % 16 == 4
    cd["loss"].backward()
    _rd_check(f"rd_fused[{nlik}]", cd, ref, xhd, liks_d, liks)


def test_rd_loss_fifth_likelihood_raises(cuda):
    from compressai._ops import RdLossFn

    D = _rd_data()
    five = [D.five.to(cuda) for _ in range(5)]
    with pytest.raises(ValueError):
        RdLossFn.apply(D.five.to(cuda), D.five.to(cuda), 1.0, 5, *five)


def test_rd_loss_unfused(cuda):
    """RdLossFnUnfused (cai_sum_log / cai_log_bwd, with a row pitch ld > C) against the same reference and
    bars, and against the fused loss"""
    from compressai._ops import RdLossFn, RdLossFnUnfused
    from compressai.losses import LMBDA

    D = _rd_data()
    names = ("big", "strided", "five")
    liks = [getattr(D, n) for n in names]
    ref = _rd_ref(D.xh, D.x, liks)
    N, _, H, W = D.x.shape
    out = {}
    for key, fn in (("unfused", RdLossFnUnfused), ("fused", RdLossFn)):
        liks_d = _rd_device_liks(names, cuda)
        xhd = D.xh.to(cuda).requires_grad_()
        loss, mse, bpp = fn.apply(xhd, D.x.to(cuda), float(LMBDA[RD_Q]), N * H * W, *liks_d)
        loss.backward()
        cd = {"loss": loss, "mse_loss": mse, "bpp_loss": bpp}
        _rd_check(f"rd_{key}[big,strided,five]", cd, ref, xhd, liks_d, liks)
        out[key] = cd
    bar = max(1e-5, 4.0 * ref.e_sum)
    for k in ("loss", "mse_loss", "bpp_loss"):
        a, b = out["unfused"][k].item(), out["fused"][k].item()
        assert abs(a - b) <= bar * max(1.0, abs(b)), (k, a, b)


# ------------------------------------------------------------------------------------------------ quantize

def test_quantize_bf16_half_to_even(cuda):
    """bf16 x and bf16 means whose difference is exactly +-0.5, +-1.5, +-2.5"""
    from compressai.entropy_models import EntropyModel

    diffs = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, -2.5])
    want = torch.tensor([0, 2, 2, 0, -2, -2], dtype=torch.int32)
    mvals = torch.tensor([0.0, 0.25, -3.0, 8.0])
    means = mvals.reshape(1, 4, 1, 1).expand(1, 4, 1, 6).contiguous()
    x = means + diffs.reshape(1, 1, 1, 6)
    xb, mb = x.bfloat16(), means.bfloat16()
    assert torch.equal(xb.float(), x) and torch.equal(mb.float(), means)       # exact in bf16
    assert torch.equal(xb.float() - mb.float(), diffs.reshape(1, 1, 1, 6).expand(1, 4, 1, 6))
    em = EntropyModel()
    r = torch.round(xb.float() - mb.float())
    assert torch.equal(r.int(), want.reshape(1, 1, 1, 6).expand(1, 4, 1, 6))
    sym = em.quantize(xb.to(cuda), "symbols", mb.to(cuda)).cpu()
    assert sym.dtype == torch.int32 and torch.equal(sym, r.int())
    deq = em.quantize(xb.to(cuda), "dequantize", mb.to(cuda)).cpu()
    assert deq.dtype == torch.bfloat16 and torch.equal(deq, (r + mb.float()).bfloat16())


def test_quantize_fp32_where_rint_is_identity(cuda):
    """|x - mean| at 2^23 +- 0.5 and 2^24: the symbols are exact in int32"""
    from compressai.entropy_models import EntropyModel

    a, b = 2.0 ** 23, 2.0 ** 24
    xs = [a - 0.5, a + 1.0, a, a + 2.0, b, b + 2.0, b - 1.0, b + 4.0]
    ms = [0.0, 0.5, 0.5, 1.5, 0.0, 0.0, 0.5, 2.0]
    x = torch.tensor(xs + [-v for v in xs], dtype=torch.float32).reshape(1, 2, 2, 4)
    m = torch.tensor(ms + [-v for v in ms], dtype=torch.float32).reshape(1, 2, 2, 4)
    assert torch.equal(x.double(), torch.tensor(xs + [-v for v in xs], dtype=torch.float64).reshape(1, 2, 2, 4))
    r = torch.round(x - m)
    assert r.abs().min() >= a - 1 and r.abs().max() <= b + 4
    em = EntropyModel()
    sym = em.quantize(x.to(cuda), "symbols", m.to(cuda)).cpu()
    assert torch.equal(sym, r.int()) and torch.equal(sym.double(), r.double())
    assert torch.equal(em.quantize(x.to(cuda), "symbols").cpu(), torch.round(x).int())
    assert torch.equal(em.quantize(x.to(cuda), "dequantize", m.to(cuda)).cpu(), r + m)
