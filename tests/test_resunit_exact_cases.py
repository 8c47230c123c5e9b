"""Coverage and sensitivity proof of the exact-lattice ResidualUnit table (resunit_exact_cases.py), on the CPU: no
kernel is launched.  The lattice conditions (every L1 bound below 2^24, the focus stage's 1 % cap) hold for every
case on the reference alone; rw_splits and the workspace layout restated in Python equal the built library's; and
six reference mutants -- the defects a fused tile / ring / pixel-split kernel can have -- each change a stored bit, so
the data can see them.  Run with -s to see the case table (DESIGN.md section 3 quotes it).
"""
import ctypes
import os

import pytest
import torch

import resunit_exact_cases as T


@pytest.fixture(scope="module")
def native():
    from compressai import _native

    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libcai.so not built")
    _native.lib.load()
    return _native


@pytest.fixture(scope="module")
def unit_refs():
    """Operands and fp32 reference of every cai_resunit case, computed once."""
    out = {}
    for u in T.UNITS:
        t = T.draw_unit(u)
        out[u.id] = (t, T.ref_unit(u, t))
    return out


def test_unit_lattice_conditions(unit_refs):
    """Exactness (L1 bound per stage and element below 2^24, fp32 == fp64) and the focus cap for every case; the
    recorded shares are the measured ones."""
    assert len({u.id for u in T.UNITS}) == len(T.UNITS)
    print()
    print(f"{'case':22s} {'B, H, W, N':16s} {'options':36s} focus  % above 256 (A, B, C)")
    for u in T.UNITS:
        t, ref = unit_refs[u.id]
        sh = T.check_unit_lattice(u, ref)
        for a, b in zip(ref[1], T.ref_unit(u, t, torch.float64)[1]):
            assert torch.equal(a.double(), b), u.id
        pct = tuple(round(100 * s, 2) for s in sh)
        opts = " ".join(f"{k}={v}" for k, v in u.opts.items() if v)
        if u.direction == T.FWD:
            opts += " shifts=%s" % (T.SHIFTS[(u.n, u.focus)],)
        else:
            opts += " dens=%s" % (T.DENS[(u.n, u.focus)],)
        print(f"{u.id:22s} {str((u.B, u.H, u.W, u.n)):16s} {opts:36s} {u.focus:5s}  {pct}")
        assert T.SHARES[u.id] == pct, (u.id, pct)
    # the operands the issue of this table names: +-1 activations and weights, masks with zeros of both signs
    for u in T.UNITS:
        t, _ = unit_refs[u.id]
        for k in ("x", "gy", "res2", "wa", "wb", "wc"):
            if t.get(k) is not None:
                assert bool((t[k].abs() == 1).all()), (u.id, k)
        if u.direction == T.BWD and u.B * u.H * u.W >= 15:
            for k in ("y", "h1", "h2", "xmask"):
                if t[k] is not None:
                    z = t[k] == 0
                    assert bool((z & torch.signbit(t[k])).any()) and bool((z & ~torch.signbit(t[k])).any()), (u.id, k)
                    assert bool((t[k] < 0).any()) and bool((t[k] > 0).any()), (u.id, k)


def test_unit_coverage():
    """Every instantiation resunit_kernel<128 | 192, fwd | bwd> has the listed shapes, a case per focus stage, a
    case with every row pitch above N, and the backward option grid with the four sets compressai._ops issues."""
    shapes = {(1, 8, 8), (1, 3, 5), (1, 1, 1), (1, 1, 19), (2, 9, 17), (2, 13, 21), (3, 16, 24)}
    for n in (128, 192):
        for d in (T.FWD, T.BWD):
            us = [u for u in T.UNITS if u.n == n and u.direction == d]
            assert shapes <= {(u.B, u.H, u.W) for u in us}, (n, d)
            assert {u.focus for u in us} == {"A", "B", "C"}, (n, d)
            pitched = [u for u in us if u.opts["pitch"]]
            assert pitched, (n, d)
            for u in pitched:
                lds = T.unit_lds(u)
                assert all(v > n for v in lds) and len(set(lds)) == 5
                assert lds[0] % 8 == 0 and lds[2] % 8 == 0 and all(v % 4 == 0 for v in lds)
                if d == T.BWD:     # every pitch is read: y (gy not masked), res2 and xmask given
                    assert (u.opts["gy_masked"], u.opts["res2"], u.opts["xmask"]) == (0, 1, 1)
            # ragged tiles at a batch above 1, and an image smaller than a tile
            assert any(u.B > 1 and u.H % 8 and u.W % 8 for u in us)
            assert any(u.H < 8 and u.W < 8 and u.H > 1 for u in us)
        grid = {(u.opts["gy_masked"], u.opts["res2"], u.opts["xmask"])
                for u in T.UNITS if u.n == n and u.direction == T.BWD}
        assert T.ISSUED <= grid and len(grid) == 8, (n, grid)


def test_wgrad_workspace_restatement(native):
    """rw_splits and the workspace layout restated in Python equal cai_resunit_wgrad_workspace_bytes for every
    case; the listed split cases exist for both widths."""
    lib = native.lib.load()
    print()
    print(f"{'case':28s} {'B, H, W, N':18s} {'P':>5s} {'S':>3s} {'chunk':>5s} last")
    for c in T.WGRADS + T.BATCH:
        P = c.B * c.H * c.W
        S, chunk = T.rw_splits(P)
        A = native.ResunitWgradArgs(batch=c.B, h=c.H, w=c.W, n=c.n)
        if not os.environ.get("CAI_RW_SPLITS"):
            assert lib.cai_resunit_wgrad_workspace_bytes(ctypes.byref(A)) == T.rw_workspace_bytes(c.n, P), c.id
        assert chunk % 64 == 0 and (S - 1) * chunk < P <= S * chunk
        print(f"{c.id:28s} {str((c.B, c.H, c.W, c.n)):18s} {P:5d} {S:3d} {chunk:5d} {P - (S - 1) * chunk:4d}")
    assert len({c.id for c in T.WGRADS + T.BATCH}) == len(T.WGRADS) + len(T.BATCH)
    for n in (128, 192):
        cs = [c for c in T.WGRADS if c.n == n]
        geo = {c.B * c.H * c.W: T.rw_splits(c.B * c.H * c.W) for c in cs}
        assert {35, 169, 288, 546, 1100, 2304, 8192} <= set(geo), n
        assert geo[35][0] == 1 and geo[169][0] == 1 and geo[288][0] == 1
        assert geo[546] == (2, 320) and 546 % 320 % 64 != 0           # S > 1, ragged last split
        assert 273 // 64 == 272 // 64                                    # the plane boundary lies inside a step
        assert geo[2304][0] == 9 and geo[8192][0] == 32
        assert {c.acc for c in cs} == {0, 1}
        assert any(c.W == 1 for c in cs) and any(c.H == 1 for c in cs)
        assert sum(1 for c in cs if c.pitch) >= 2
    n192 = [c for c in T.BATCH if c.n == 192]
    n128 = [c for c in T.BATCH if c.n == 128]
    assert len(n192) >= 26 and len(n192) > T.RW_BATCH_MAX and len(n128) >= 3
    first = [i for i, c in enumerate(T.BATCH) if c.n == 128]
    assert first[0] < T.RW_BATCH_MAX < first[-1]                         # N = 128 units on both sides of the flush
    assert all(35 <= c.B * c.H * c.W <= 546 or c.B * c.H * c.W == 2304 for c in T.BATCH)
    assert sum(1 for c in T.BATCH if c.B * c.H * c.W == 2304) == 1


def test_wgrad_reference_is_torchs():
    """The pixel-major restatement of the three weight gradients equals torch's own, in fp32 and fp64."""
    c = [c for c in T.WGRADS if (c.B, c.H, c.W) == (2, 13, 21)][0]
    ops, init = T.draw_wgrad(c)
    nh = c.n // 2
    for d in (torch.float32, torch.float64):
        x, h1, h2, ga, gb, gc = (v.to(d) for v in ops)
        got = T.ref_wgrad(c, ops, None, d)
        want = [torch.einsum("bchw,bkhw->kc", x, ga).reshape(nh, c.n, 1, 1), ga.sum((0, 2, 3)),
                torch.nn.grad.conv2d_weight(h1, (nh, nh, 3, 3), gb, padding=1), gb.sum((0, 2, 3)),
                torch.einsum("bchw,bkhw->kc", h2, gc).reshape(c.n, nh, 1, 1), gc.sum((0, 2, 3))]
        for a, b in zip(got, want):
            assert torch.equal(a, b)


def _differs(a, b):
    return any(not torch.equal(x.to(torch.bfloat16) + 0, y.to(torch.bfloat16) + 0) for x, y in zip(a, b))


UNIT_MUTANTS = {"halo_bias": (T.FWD,), "tap_row": (T.FWD, T.BWD), "res2_tail": (T.BWD,), "h1_ge": (T.BWD,)}


@pytest.mark.parametrize("mutant", sorted(UNIT_MUTANTS))
def test_unit_reference_mutants_are_seen(unit_refs, mutant):
    """Each defect, applied to the torch restatement, changes a stored bit in a case of every instantiation it
    can affect: the table's data can see it."""
    for n in (128, 192):
        for d in UNIT_MUTANTS[mutant]:
            seen = []
            for u in T.UNITS:
                if u.n == n and u.direction == d:
                    t, ref = unit_refs[u.id]
                    if _differs(T.ref_unit(u, t, mutant=mutant)[1], ref[1]):
                        seen.append(u.id)
            print(mutant, n, "fwd" if d == T.FWD else "bwd", seen)
            assert seen, (mutant, n, d)


@pytest.mark.parametrize("mutant", ["last_pixel", "col_wrap"])
def test_wgrad_reference_mutants_are_seen(mutant):
    for n in (128, 192):
        seen = []
        for c in T.WGRADS:
            if c.n == n and c.B * c.H * c.W <= 2304:
                ops, init = T.draw_wgrad(c)
                a, b = T.ref_wgrad(c, ops, init), T.ref_wgrad(c, ops, init, mutant=mutant)
                if any(not torch.equal(x, y) for x, y in zip(a, b)):
                    seen.append(c.id)
        print(mutant, n, seen)
        assert seen, (mutant, n)
        if mutant == "last_pixel":      # every case sees it: each gradient element sums every pixel
            assert len(seen) == sum(1 for c in T.WGRADS if c.n == n and c.B * c.H * c.W <= 2304)
