"""Inputs of the exact (integer-lattice) cases of test_swin_ops_gpu.py, as fp32 CPU tensors, shared with the proof of
their preconditions in test_swin_reference_cpu.py.  Seeded by the case's name: both files see the same values."""
import random
import zlib

import torch

import swin_reference as R

MASKED = -1000.0          # expf(MASKED) is exactly 0 in fp32 and fp64
ATTN_SCALE = 0.25
# group sizes of the first windows' partitions (every size occurs whatever the window count), then random ones
_PRESET = ([16], [8, 4, 2, 1, 1], [4, 4, 4, 2, 2], [8, 8], [2] * 8, [1] * 16, [8, 2, 2, 2, 1, 1])


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def lattice(shape, vmax, g):
    """Uniform over the non-zero integers of [-vmax, vmax]."""
    mag = torch.randint(1, vmax + 1, shape, generator=g)
    sgn = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sgn).float()


def group_mask(nW, name):
    """[nW][16][16]: every window gets its own partition of its 16 tokens into groups of 16, 8, 4, 2 or 1 tokens;
    0 inside a group, MASKED across groups.  Also returns the group sizes per window."""
    rnd = random.Random(zlib.crc32(name.encode()))
    mask = torch.full((nW, R.WN, R.WN), MASKED)
    sizes = []
    for w in range(nW):
        if w < len(_PRESET):
            parts = list(_PRESET[w])
        else:
            parts, left = [], R.WN
            while left:
                p = rnd.choice([s for s in (16, 8, 4, 2, 1) if s <= left])
                parts.append(p)
                left -= p
        toks = list(range(R.WN))
        rnd.shuffle(toks)
        at = 0
        for p in parts:
            grp = torch.tensor(toks[at:at + p])
            mask[w, grp[:, None], grp[None, :]] = 0.0
            at += p
        sizes.append(parts)
    return mask, sizes


def attn_exact(case, dtype, zero, masked):
    """All scores 0 (zero = "q" or "k" is all zeros, the other on the lattice, bias table 0), so P is 1 / n inside
    a group of n tokens.  -> dict of q, kv, dout, table, table0 (the accumulate prefill), mask (or None)."""
    name = f"attn-{case.id}-{dtype}-{zero}-{int(masked)}"
    g = gen(name)
    n, C = case.B * case.Hr * case.Wr, case.heads * R.HD
    vmax = 3 if dtype == "f32" else 1
    q = torch.zeros(n, C) if zero == "q" else lattice((n, C), vmax, g)
    k = torch.zeros(n, C) if zero == "k" else lattice((n, C), vmax, g)
    v, dout = lattice((n, C), vmax, g), lattice((n, C), vmax, g)
    nW = (case.Hr // R.WS) * (case.Wr // R.WS)
    return dict(q=q, kv=torch.cat([k, v], dim=1), dout=dout, table=torch.zeros(49, case.heads),
                table0=lattice((49, case.heads), 3, g), mask=group_mask(nW, name)[0] if masked else None)


def attn_exact_ref(case, d, dt):
    """out, dq, dkv, dtable of the restatement in dtype dt."""
    m = None if d["mask"] is None else d["mask"].to(dt)
    return R.window_attn_grads(d["q"].to(dt), d["kv"].to(dt), d["table"].to(dt), R.rel_index(), m, case.B, case.Hr,
                               case.Wr, case.heads, case.shift, ATTN_SCALE, d["dout"].to(dt))


def ln_db(case, dtype):
    """x off the lattice, dy on it: db = sum dy is exact whatever x is."""
    g = gen(f"lndb-{case.id}-{dtype}")
    x = torch.randn(case.ntok, case.C, generator=g)
    return dict(x=x, dy=lattice((case.ntok, case.C), 3, g), w=torch.rand(case.C, generator=g) + 0.5,
                dw0=lattice((case.C,), 3, g), db0=lattice((case.C,), 3, g))


def channel_mean(case, dtype):
    g = gen(f"cmean-{case.id}-{dtype}")
    shape = (case.B, case.HW, case.C)
    return dict(x=lattice(shape, 3, g), x2=lattice(shape, 3, g))


def channel_affine(B, HW, C, dtype, name):
    g = gen(f"affine-{name}-{B}-{dtype}")
    vmax = 3
    return dict(x=lattice((B, HW, C), 1 if dtype == "bf16" else vmax, g), gamma=lattice((B, C), vmax, g),
                beta=lattice((B, C), vmax, g))
