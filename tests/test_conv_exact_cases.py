"""Coverage proof of the exact-lattice conv table (conv_exact_cases.py), on the CPU: no kernel is launched.

The names and split factors come from the built library (cai_conv_kernel_name / cai_conv_split_factor), so a
dispatch change that moves a case off its kernel fails here, before test_conv_exact_gpu.py silently stops
testing that kernel.  Run with -s to see the case -> kernel -> split-factor table (DESIGN.md section 3 quotes it).
"""
import ctypes
import os
import re

import pytest

import conv_exact_cases as T

# A/B knobs that switch kernels off (the names matching the pattern are then not expected), and knobs that move
# thresholds or split factors (with one set, only the names are scanned, not the table)
OFF_KNOBS = {
    "CAI_HALO_OFF": r"halo", "CAI_HALO_PH_OFF": r"conv_halo_(phase|quad)", "CAI_QUAD_OFF": r"quad",
    "CAI_HALO_S1_OFF": r"conv_halo_s1", "CAI_SMALL_CONV_OFF": r"conv_small", "CAI_GLDS32_OFF": r".",
    "CAI_HALO_WGRAD_OFF": r"wgrad_halo", "CAI_HALO_WGRAD_S1_OFF": r"wgrad_halo_kernel<3,s1>",
    "CAI_HALO_WGRAD_ROWS_OFF": r"wgrad_halo_kernel<\d,r", "CAI_SMALL_WGRAD_OFF": r"wgrad_small",
}
ZERO_OFF_KNOBS = {"CAI_GLDS_M64": r"conv_glds_kernel<64x", "CAI_HALO_S1_BN64": r"conv_halo_s1_kernel<64>"}
TUNING_KNOBS = ["CAI_SMALL_CONV_KMAX", "CAI_SMALL_CONV_MMAX", "CAI_SMALL_CONV_KMAX512", "CAI_HALO_MIN_TILES",
                "CAI_HALO_S1_SPLIT_CIN", "CAI_KSPLIT_MAX", "CAI_WG_BLOCKS", "CAI_WG_MIN_STRIPS", "CAI_WG_BLOCKS_R192",
                "CAI_HALO_WGRAD_K3_ROWS64", "CAI_HALO_WGRAD_ROWS128", "CAI_HALO_WGRAD_ROWS192",
                "CAI_SMALL_WGRAD_MMAX", "CAI_SMALL_WGRAD_W64", "CAI_SMALL_WGRAD_WMAX"]


def _switched_off():
    pats = [p for k, p in OFF_KNOBS.items() if os.environ.get(k, "0") not in ("", "0")]
    pats += [p for k, p in ZERO_OFF_KNOBS.items() if os.environ.get(k, "") == "0"]
    return [re.compile(p) for p in pats]


def _off(name, pats):
    return any(p.search(name) for p in pats)


@pytest.fixture(scope="module")
def native():
    from compressai import _native

    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libcai.so not built")
    _native.lib.load()
    return _native


def _name_split(native, run):
    lib = native.lib.load()
    g = native.ConvGeom(*run.geom)
    dt = native.F32 if run.opts.get("dtype") == "f32" else native.BF16
    tf = 1 if (run.opts.get("abs") or run.opts.get("sq")) else 0     # weight gradient: any input transform
    return (lib.cai_conv_kernel_name(ctypes.byref(g), dt, run.direction, tf).decode(),
            lib.cai_conv_split_factor(ctypes.byref(g), dt, run.direction, tf))


def runs_named_kernel(run):
    """The name is computed for a bf16 pixel-major output without mask or residual; a call outside that form
    leaves the register-direct kernels (run_conv falls back).  True when this run's call keeps the named kernel."""
    o = run.opts
    if run.direction == T.WGRAD:
        return True
    bf16_pm = run.direction == T.DGRAD or o.get("y", "f32") == "bf16"
    if run.kernel == "conv_halo_quad_kernel":
        return bf16_pm and not o.get("mask") and not o.get("res")
    if run.kernel in ("conv_halo_phase_kernel<192>", "conv_halo_s1_kernel<192>") and not run.split:
        return bf16_pm
    return True


FD_NAMES = (["conv_halo_kernel<3>", "conv_halo_kernel<5>", "conv_halo_phase_kernel", "conv_halo_phase_kernel<192>",
             "conv_halo_quad_kernel", "conv_halo_s1_kernel<64>", "conv_halo_s1_kernel<128>",
             "conv_halo_s1_kernel<192>"]
            + [T.SM % t for t in ("16x32", "32x32", "32x64")]
            + [T.GL % t for t in ("256x128", "128x192", "256x64", "128x128", "64x128", "64x192")]
            + [T.GB % t for t in ("256x16", "128x64", "64x192", "128x128")])
WG_NAMES = ["wgrad_small_kernel", "wgrad_kernel<bf16>", "wgrad_kernel<float>", "wgrad_glds_kernel<128>",
            "wgrad_glds_kernel<256>", "wgrad_halo_kernel<3>", "wgrad_halo_kernel<3,r2>", "wgrad_halo_kernel<3,r4>",
            "wgrad_halo_kernel<5>", "wgrad_halo_kernel<5,r2>", "wgrad_halo_kernel<5,r4>", "wgrad_halo_kernel<3,s1>"]


def _ragged(run):
    """Output height, width and channel count are no multiples of the kernel's tile, at a batch above 1."""
    B = run.geom[0]
    k = run.kernel
    if run.direction != T.WGRAD:
        phase, kin, kout, H, W, OHg, OWg = T.gemm_view(run.geom, run.direction)
        m = re.search(r"(\d+)x(\d+)>", k)
        if m:                                    # GEMM tiles: BM rows of the flattened pixels x BN channels
            return B > 1 and (B * OHg * OWg) % int(m.group(1)) != 0 and kout % int(m.group(2)) != 0
        bn = 192 if "<192>" in k else 128         # halo tiles: 8 x 32 pixels x BN channels
        chan = kout % bn != 0 or k == "conv_halo_s1_kernel<64>"     # <64> takes exactly 64 channels
        return B > 1 and OHg % 8 != 0 and OWg % 32 != 0 and chan
    Ng, Cq, Hg, Wg, M = T.wgrad_view(run.geom)
    kk = run.geom[7] ** 2
    vec = 4 if run.opts.get("dtype") == "f32" else 8
    ncols = kk * ((Cq + vec - 1) // vec * vec)
    if k.startswith("wgrad_halo"):               # whole 64-pixel strips and 64-channel chunks by construction
        return B > 1 and Ng % 64 != 0
    if k == "wgrad_small_kernel":                # 64 x 64 tiles, 32-pixel steps
        return B > 1 and Ng % 64 != 0 and Cq % 64 != 0 and M % 32 != 0
    ct = 256 if k == "wgrad_glds_kernel<256>" else 128
    return B > 1 and Ng % 128 != 0 and ncols % ct != 0 and M % 64 != 0


def test_table_names_and_splits(native):
    """Every run of the table lands on the kernel and on the side of the split it was written for."""
    pats = _switched_off()
    tuned = [k for k in TUNING_KNOBS if os.environ.get(k, "")]
    if tuned:
        pytest.skip(f"dispatch thresholds moved by {tuned}")
    assert len({r.id for r in T.RUNS}) == len(T.RUNS)
    print()
    print(f"{'run':30s} {'geometry (B, Cin, H, W, Cout, OH, OW, k, s, p, op, T)':58s} {'kernel':34s} split options")
    for r in T.RUNS:
        name, split = _name_split(native, r)
        opts = " ".join(f"{k}={v}" for k, v in r.opts.items())
        print(f"{r.id:30s} {str(r.geom):58s} {name:34s} {split:5d} {opts}")
        if _off(r.kernel, pats):
            continue
        assert name == r.kernel, (r.id, name, r.kernel)
        if r.kernel not in T.NEVER_SPLIT:        # (wgrad_small_kernel reports the unused pixel-split plan)
            assert (split > 1) == r.split, (r.id, split)
        assert runs_named_kernel(r), r.id
        assert r.kernel not in T.UNREACHED


def test_table_covers_every_kernel(native):
    pats = _switched_off()
    fd = {(r.kernel, r.split) for r in T.RUNS if r.direction != T.WGRAD}
    wg = {(r.kernel, r.split) for r in T.RUNS if r.direction == T.WGRAD}
    for names, have in ((FD_NAMES, fd), (WG_NAMES, wg)):
        for n in names:
            if n in T.UNREACHED or _off(n, pats):
                continue
            sides = {s for k, s in have if k == n}
            want = {False} if n in T.NEVER_SPLIT else ({True} if n in T.ALWAYS_SPLIT else {False, True})
            assert want <= sides, (n, sides)
    floats = {r.kernel for r in T.RUNS if r.kernel.startswith("conv_gemm_kernel<float")}
    assert len(floats) >= 2
    assert set(T.UNREACHED) <= set(FD_NAMES + WG_NAMES)
    # ragged tiles at a batch above 1, on every tiled kernel
    for n in FD_NAMES + WG_NAMES + sorted(floats):
        if n in T.UNREACHED or _off(n, pats):
            continue
        assert any(_ragged(r) for r in T.RUNS if r.kernel == n), n
    # input widths: 3 (padded to 8), 32-mod-64 (96, 160), 192; both phase-direction forms
    kin = {T.gemm_view(r.geom, r.direction)[1] for r in T.RUNS if r.direction != T.WGRAD}
    assert {3, 96, 160, 192} <= kin
    phase = {(r.geom[11], r.direction) for r in T.RUNS
             if r.direction != T.WGRAD and T.gemm_view(r.geom, r.direction)[0]}
    assert {(1, T.FWD), (0, T.DGRAD)} <= phase
    # a split that does not divide the chunk count: 5 chunks of 32 channels over 3 splits
    uneven = [r for r in T.RUNS if r.id == "halo3-c160-96-fwd"][0]
    assert _name_split(native, uneven)[1] == 3 or _off(uneven.kernel, pats) or os.environ.get("CAI_KSPLIT_MAX")


def test_table_covers_every_epilogue():
    """Bias, ReLU, LeakyReLU, the forward residual, the three masks with one and two residual gradients, |x| and
    x^2 inputs and accumulate each appear on the LDS epilogue (GEMM / LDS-DMA kernels, no split), on the halo
    kernels' register-direct epilogue (bf16 output, no split) and behind the split-K reduce."""
    def impl(r):
        if r.split:
            return "reduce"
        if "halo" in r.kernel:
            bf16 = r.direction == T.DGRAD or r.opts.get("y") == "bf16"
            return "direct" if bf16 else "halo-lds"
        return "lds"

    fd = [r for r in T.RUNS if r.direction != T.WGRAD and r.opts.get("dtype") != "f32"]
    for im in ("lds", "direct", "reduce"):
        rs = [r for r in fd if impl(r) == im]
        f = [r.opts for r in rs if r.direction == T.FWD]
        d = [r.opts for r in rs if r.direction == T.DGRAD]
        assert any(o.get("act") == T.RELU for o in f), im
        assert any(o.get("act") == T.LEAKY for o in f), im
        assert any(o.get("res") for o in f), im
        assert any(o.get("bias", True) for o in f), im
        for mask in (T.POS, T.MLEAKY, T.SIGN):
            assert any(o.get("mask") == mask and o.get("res") for o in d), (im, mask)
        assert {1, 2} <= {o.get("res") for o in d}, im
    assert any(impl(r) == "halo-lds" for r in fd)
    assert any(r.opts.get("abs") for r in fd if r.direction == T.FWD)
    wg = [r.opts for r in T.RUNS if r.direction == T.WGRAD]
    assert any(o.get("abs") for o in wg) and any(o.get("sq") for o in wg) and any(o.get("acc") for o in wg)
    for d in (T.FWD, T.DGRAD, T.WGRAD):
        assert any(r.opts.get("pitch") for r in T.RUNS if r.direction == d)


def test_no_other_kernel_is_reachable(native):
    """A scan of the geometry space returns no name outside the lists above, and none of the names recorded as
    unreachable: a dispatch change that brings a new kernel (or one of those) into play must extend the table."""
    lib = native.lib.load()
    pats = _switched_off()
    seen = set()
    for kind in ("conv", "deconv"):
        for k, s in ((1, 1), (3, 1), (3, 2), (5, 2), (5, 1), (2, 2)):
            for B in (1, 4, 16):
                for cin in (3, 32, 40, 64, 96, 128, 192, 512):
                    for cout in (3, 16, 40, 64, 96, 128, 192, 320, 768):
                        for H, W in ((4, 4), (9, 7), (16, 16), (20, 36), (32, 32), (64, 64), (64, 128), (130, 150)):
                            pad = 0 if k == 2 else None
                            g = native.ConvGeom(*T.geom12(kind, B, cin, cout, H, W, k, s, pad))
                            for d in (0, 1, 2):
                                for dt in (native.BF16, native.F32):
                                    for ia in (0, 1):
                                        seen.add(lib.cai_conv_kernel_name(ctypes.byref(g), dt, d, ia).decode())
    seen.discard("")
    floats = {T.GF % t for t in ("256x16", "128x64", "64x192", "128x128")}
    assert seen <= set(FD_NAMES) | set(WG_NAMES) | floats, seen - set(FD_NAMES) - set(WG_NAMES) - floats
    if not pats:
        assert not (seen & set(T.UNREACHED)), seen & set(T.UNREACHED)
