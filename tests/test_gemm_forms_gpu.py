"""Every GEMM kernel family of csrc/lrl_gemm.hip at the operand forms the PPO update runs them in (through
lrl_gemm_f32_ex): grouped products whose group offsets are column offsets inside a shared row pitch, column-slice
outputs, unaligned bases, gathered rows, split-k partials in the update's [split][group][M][N] layout.

Each case lives in an arena: every operand and the output sit in buffers with 128 rows and 128 columns of owned slack
on every side.  The output arena, the workspace tail and the db buffer hold a sentinel bit pattern; the operand slack
(rows outside the matrix, the pitch gap, the unselected rows of a gathered source) holds poison.  A case asserts
  value         per element against a float64 product of the same fp32 inputs: |C - ref| / (sum_k |a b| + |bias|) <= 1e-6
                (store / bias / partial; the bias gradient relative to sum |dY|); for the ELU, ELU', tanh, tanh'
                epilogues the native error against float64 is at most twice that of the torch fp32 form;
  footprint     every int32 outside the groups x M x N product (and past the workspace's used part) is still the sentinel;
  independence  the run with NaN poison and the run with 1e30 poison give the same bits, all finite;
  path          the family / tile the dispatcher reports is the one the case is meant for.
Run with -s for the measured errors."""
import ctypes as C
import math
import struct
from types import SimpleNamespace as NS

import pytest
import torch

from lrl import _abi

pytestmark = pytest.mark.gpu
dev = "cuda:0"
NT, NN, TN = 0, 2, 3
SLACK = 128
SENT = 0x7FA5A5A5                                       # a NaN with a payload no kernel produces
NAN_BITS = 0x7FC00000
BIG_BITS = struct.unpack("<i", struct.pack("<f", 1e30))[0]
FAM = {v: k for k, v in _abi.GEMM_FAMILIES.items()}
RECORDED = {}  # family name -> set of (bm, bn, interior) the passing cases reported
WORST = {}     # family name -> worst measured (kind, figure)


# ---- the case table -------------------------------------------------------------------------------------------------
def case(layout, M, N, K, epi=None, form="a", gather=False, mask=0, planes=False, expect=None, twin=None, **ov):
    """form a: contiguous, one group; b: the update's grouped form (2 groups, column offsets inside one row pitch);
    c: column-slice output (C at +42 floats in a pitch of 64); d / d1: unaligned B (base +42 floats, ldb 60: 8-byte
    aligned; base +43, ldb 61: 4-byte); bp: form b with 8 floats of poison at the end of every pitch and 4 between
    the groups.  twin: a mask under which the same product must run on gemm_x6_kernel and give
    the same bits (planes dropped).  ov: pitch overrides (lda / ldb)."""
    epi = (4 if layout == TN else 0) if epi is None else epi
    c = NS(layout=layout, M=M, N=N, K=K, epi=epi, form=form, gather=gather, mask=mask, planes=planes, expect=expect,
           twin=twin, ov=ov, groups=2 if form in ("b", "bp") else 1)
    c.id = "%s-%dx%dx%d-e%d-%s%s-m%d%s%s" % ({NT: "nt", NN: "nn", TN: "tn"}[layout], M, N, K, epi, form,
                                              "g" if gather else "", mask, "p" if planes else "",
                                              "".join("-%s%d" % kv for kv in sorted(ov.items())))
    return c


CASES = []


def add(*a, **k):
    CASES.append(case(*a, **k))


NT_EPIS, NN_EPIS = (0, 1, 2, 5), (0, 3, 6)
for L, epis in ((NT, NT_EPIS), (NN, NN_EPIS)):
    # -- x6, 64 x 64 tile: interior, ragged in m / n / k, the lower eligibility edge
    for e in epis:
        add(L, 128, 128, 64, e, expect=("x6", 64, 64, True))
        add(L, 129, 70, 40, e, "b", expect=("x6", 64, 64, False))
    add(L, 128, 128, 64, epis[-1], "b", expect=("x6", 64, 64, True))
    add(L, 128, 128, 64, epis[1], "a", True, expect=("x6", 64, 64, True))
    add(L, 129, 70, 40, epis[2], "a", True, expect=("x6", 64, 64, False))
    add(L, 64, 16, 32, epis[1], expect=("x6", 64, 64, False))
    add(L, 128, 18, 64, epis[1], "c", expect=("x6", 64, 64, False))
    # -- x6, 128-row / 128-wide tiles (the workgroup counts the dispatcher asks for), and x6d on the same tiles.  No
    # NT / NN shape reaches 64 x 128: 1,024 64 x 128 workgroups are always at least 512 128 x 128 ones
    add(L, 8192, 512, 32, epis[2], "b", expect=("x6", 128, 128, True))
    add(L, 8192, 256, 32, epis[1], "b", expect=("x6", 128, 64, True))
    add(L, 8192, 512, 32, epis[1], "b", mask=8, expect=("x6d", 128, 128), twin=4)
    add(L, 8192, 256, 32, epis[2], "b", True, mask=8, expect=("x6d", 128, 64), twin=4)
    # -- x6d, 64 x 64: every epilogue, grouped, gathered; bit-identical to x6
    for e in epis:
        add(L, 128, 128, 64, e, "b", mask=8, expect=("x6d", 64, 64), twin=4)
    add(L, 128, 128, 64, epis[1], "a", True, mask=8, expect=("x6d", 64, 64), twin=4)
    # -- x6p (pre-split B planes): every epilogue, grouped, gathered; bit-identical to x6
    for e in epis:
        add(L, 64, 128, 32, e, "b", planes=True, expect=("x6p", 64, 128), twin=0)
    add(L, 192, 256, 48, epis[1], "a", True, planes=True, expect=("x6p", 64, 128), twin=0)
    add(L, 192, 256, 48, epis[2], "b", True, planes=True, expect=("x6p", 64, 128), twin=0)
    # -- glds (k not a multiple of 32) / glds32: every epilogue, grouped, gathered
    for e in epis:
        add(L, 128, 128, 48, e, "b", mask=16, expect=("glds", 64, 64))
        add(L, 128, 128, 64, e, "b", mask=16, expect=("glds32", 64, 64))
    add(L, 128, 128, 48, epis[1], "a", True, mask=16, expect=("glds", 64, 64))
    add(L, 128, 128, 64, epis[2], "a", True, mask=16, expect=("glds32", 64, 64))
    # -- register-staged, what the other fp32 families refuse: ragged, grouped, gathered, column slice
    for e in epis:
        add(L, 129, 70, 40, e, "b", mask=16, expect=("staged", 64, 64))
    add(L, 129, 70, 40, epis[1], "a", True, mask=16, expect=("staged", 64, 64))
    add(L, 128, 18, 64, epis[1], "c", mask=16, expect=("staged", 128, 32))
    add(L, 40, 128, 64, epis[1], expect=("staged", 64, 64))      # short m (default switches: x6 wants m >= 64)
    add(L, 20, 100, 64, epis[2], "b", expect=("staged", 32, 128))
# x6 128 x 128, ragged in m, n and k
add(NT, 8129, 500, 40, 2, "b", expect=("x6", 128, 128, False))
# x6p's 128-row tile (768 128 x 128 tiles)
add(NT, 8192, 768, 32, 1, "b", planes=True, expect=("x6p", 128, 128), twin=0)
# -- unaligned B (forms d / d1): x6 stages it with dword loads; x6d and glds need float4 operands and must refuse
add(NT, 128, 64, 40, 1, "d", expect=("x6", 64, 64, False))
add(NT, 128, 64, 40, 2, "d1", expect=("x6", 64, 64, False))
add(NN, 128, 18, 64, 0, "d", expect=("x6", 64, 64, False))
add(NT, 128, 64, 48, 1, "d", mask=8, expect=("x6", 64, 64, False))
add(NT, 128, 64, 48, 1, "d", mask=16, expect=("staged", 64, 64))
add(NT, 128, 64, 40, 5, "d1", mask=16, expect=("staged", 64, 64))
add(NN, 128, 18, 64, 3, "d", mask=16, expect=("staged", 128, 32))
add(NT, 128, 18, 64, 2, "c", mask=8, expect=("x6", 64, 64, False))   # (x6d wants whole 64-wide n tiles)
add(TN, 128, 60, 2048, form="d", expect=("x6", 128, 64, False))       # (x6t and glds_tn want a float4 B)
add(TN, 128, 60, 2048, form="d", gather=True, mask=16, expect=("staged", 128, 64))
# -- the grouped form with poison between the groups and at the end of every pitch
add(NT, 129, 70, 40, 2, "bp", expect=("x6", 64, 64, False))
add(NN, 129, 70, 40, 3, "bp", True, expect=("x6", 64, 64, False))
add(NN, 128, 128, 64, 6, "bp", mask=8, expect=("x6d", 64, 64), twin=4)
add(NT, 64, 128, 32, 5, "bp", planes=True, expect=("x6p", 64, 128), twin=0)
add(NT, 128, 128, 48, 2, "bp", True, mask=16, expect=("glds", 64, 64))
add(NN, 128, 128, 64, 3, "bp", mask=16, expect=("glds32", 64, 64))
add(NT, 256, 24, 512, 5, "bp", True, expect=("thin16", 16, 32))
add(NT, 256, 24, 512, 2, "bp", mask=32, expect=("thin32", 32, 32))
add(NN, 129, 70, 40, 6, "bp", mask=16, expect=("staged", 64, 64))
add(NT, 200, 3, 128, 1, "bp", expect=("staged", 128, 32))
add(TN, 128, 128, 6000, form="bp", expect=("x6t", 128, 128), twin=2)
add(TN, 100, 70, 5000, form="bp", gather=True, expect=("x6", 128, 128, False))
add(TN, 256, 128, 6000, form="bp", mask=16, expect=("glds_tn", 128, 128))
add(TN, 100, 12, 2000, form="bp", mask=16, expect=("staged", 128, 32))
# -- thin16 (default) and thin32 (bit 5)
for m, fam in ((0, ("thin16", 16, 32)), (32, ("thin32", 32, 32))):
    for e in NT_EPIS:
        add(NT, 256, 24, 512, e, "b", mask=m, expect=fam)
    add(NT, 300, 18, 1024, 1, "a", True, mask=m, expect=fam)
    add(NT, 257, 32, 512, 2, mask=m, expect=fam)
    add(NT, 300, 18, 512, 1, "c", mask=m, expect=fam)
    add(NN, 300, 18, 1024, 0, "d", mask=m, expect=fam)      # the latent gradient
    add(NN, 256, 24, 512, 0, "b", True, mask=m, expect=fam)
# -- register-staged, default switches: the narrow heads, short k (lda = 18: 8-byte rows), NN with n = 7
for n in (12, 3, 1):
    add(NT, 200, n, 128, 1, expect=("staged", 128, 32))
add(NT, 200, 3, 128, 5, "b", expect=("staged", 128, 32))
add(NT, 777, 256, 18, 2, "a", True, expect=("staged", 64, 64))
add(NT, 777, 256, 18, 1, "b", expect=("staged", 64, 64))
add(NN, 300, 7, 64, 3, expect=("staged", 128, 32))
add(NN, 300, 7, 64, 6, "b", expect=("staged", 128, 32))
# -- weight gradients.  x6: the four tiles at one split, the update's split count with a short last split, ragged, gather
add(TN, 64, 64, 96, expect=("x6", 64, 64, True))
add(TN, 64, 128, 96, form="b", expect=("x6", 64, 128, True))
add(TN, 64, 128, 96, gather=True, expect=("x6", 64, 128, True))
add(TN, 128, 64, 96, mask=2, expect=("x6", 128, 64, True))
add(TN, 128, 128, 96, form="b", mask=2, expect=("x6", 128, 128, True))
add(TN, 128, 256, 6000, form="b", mask=2, expect=("x6", 128, 128, True))
add(TN, 100, 70, 5000, expect=("x6", 128, 128, False))
add(TN, 100, 70, 5000, form="b", gather=True, expect=("x6", 128, 128, False))
add(TN, 18, 128, 4097, expect=("x6", 64, 128, False))
# x6t, each bit-identical to x6
add(TN, 128, 60, 2048, ldb=64, expect=("x6t", 128, 64), twin=2)
add(TN, 128, 60, 2048, gather=True, ldb=64, expect=("x6t", 128, 64), twin=2)
add(TN, 256, 200, 2048, ldb=256, expect=("x6t", 128, 128), twin=2)
add(TN, 256, 200, 2048, gather=True, ldb=256, expect=("x6t", 128, 128), twin=2)
add(TN, 128, 128, 6000, form="b", expect=("x6t", 128, 128), twin=2)
# glds_tn
add(TN, 128, 60, 2048, mask=16, ldb=64, expect=("glds_tn", 128, 64))
add(TN, 128, 60, 2048, gather=True, mask=16, ldb=64, expect=("glds_tn", 128, 64))
add(TN, 128, 200, 2048, mask=16, ldb=256, expect=("glds_tn", 128, 128))
add(TN, 256, 128, 6000, form="b", mask=16, expect=("glds_tn", 128, 128))
add(TN, 256, 128, 6000, form="b", gather=True, mask=16, expect=("glds_tn", 128, 128))
# register-staged: the six tiles
add(TN, 12, 128, 96, expect=("staged", 32, 128))
add(TN, 100, 12, 2000, form="b", expect=("staged", 128, 32))
add(TN, 18, 128, 4097, mask=16, expect=("staged", 32, 128))
add(TN, 100, 70, 5000, form="b", mask=16, expect=("staged", 128, 128))
add(TN, 100, 70, 5000, gather=True, mask=16, expect=("staged", 128, 128))
add(TN, 100, 60, 2000, mask=16, expect=("staged", 128, 64))
add(TN, 60, 100, 2000, form="b", gather=True, mask=16, expect=("staged", 64, 128))
add(TN, 60, 60, 2000, mask=16, expect=("staged", 64, 64))

# one store-epilogue case per family for the power-of-two scaling test
SCALE_CASES = [case(NT, 129, 70, 40, 0, "b", expect=("x6", 64, 64, False)),
               case(TN, 100, 70, 5000, expect=("x6", 128, 128, False)),
               case(NN, 128, 128, 64, 0, "b", mask=8, expect=("x6d", 64, 64)),
               case(NT, 64, 128, 32, 0, "b", planes=True, expect=("x6p", 64, 128)),
               case(TN, 128, 60, 2048, ldb=64, expect=("x6t", 128, 64)),
               case(NT, 128, 128, 48, 0, "b", mask=16, expect=("glds", 64, 64)),
               case(NN, 128, 128, 64, 0, "b", mask=16, expect=("glds32", 64, 64)),
               case(TN, 128, 60, 2048, mask=16, ldb=64, expect=("glds_tn", 128, 64)),
               case(NT, 256, 24, 512, 0, "b", expect=("thin16", 16, 32)),
               case(NT, 256, 24, 512, 0, "b", mask=32, expect=("thin32", 32, 32)),
               case(NT, 129, 70, 40, 0, "b", mask=16, expect=("staged", 64, 64)),
               case(TN, 100, 70, 5000, mask=16, expect=("staged", 128, 128))]


# ---- arenas ---------------------------------------------------------------------------------------------------------
class Buf:
    """`groups` matrices [rows][cols] (row pitch ld, gs floats between groups) at `shift` floats past a 256-byte aligned
    address, inside a flat int32 buffer with SLACK rows and SLACK columns before and after, all filled with `fill`."""

    def __init__(self, groups, rows, cols, ld, gs, shift, fill, dtype=torch.float32):
        assert cols <= ld or rows == 1
        span = (groups - 1) * gs + (rows - 1) * ld + cols
        pre = -(-(SLACK * ld + SLACK) // 64) * 64
        self.flat = torch.full((pre + shift + span + SLACK * ld + SLACK,), fill, dtype=torch.int32, device=dev)
        self.geo = ((groups, rows, cols), (gs, ld, 1), pre + shift)
        self.view = torch.as_strided(self.flat.view(dtype), *self.geo)
        self.ptr = C.c_void_p(self.flat.data_ptr() + 4 * (pre + shift))

    def untouched_outside(self, fill):
        keep = torch.ones(self.flat.numel(), dtype=torch.bool, device=dev)
        torch.as_strided(keep, *self.geo).fill_(False)
        return bool((self.flat[keep] == fill).all())


def _pick_splits(M, N, K, groups):
    """gemm_pick_splits, restated: the workspace is sized from it, and the library's own count must agree."""
    bm, bn = (128 if M > 64 else 64 if M > 32 else 32), (128 if N > 64 else 64 if N > 32 else 32)
    if bm == 32 and bn < 128:
        bn = 128
    if bn == 32 and bm < 128:
        bm = 128
    tiles, out, s = groups * -(-M // bm) * -(-N // bn), groups * M * N, 1
    while tiles * s < 512 and s < 256 and K // (2 * s) >= 128 and out * s * 2 <= (12 << 20):
        s *= 2
    return s


def _geometry(c):
    """Pitches, group strides and base shifts of the case's form."""
    M, N, K, g = c.M, c.N, c.K, c.groups
    f = NS(shA=0, shB=0, shC=0, ga=0, gb=0, gc=0, gbias=0, gaux=0, ld_aux=N)
    if c.layout == TN:
        f.lda, f.ldb, f.ldc = M, N, N
        if c.form == "b":
            f.lda, f.ga, f.ldb, f.gb = 2 * M, M, 2 * N, N
        elif c.form == "bp":
            f.lda, f.ga, f.ldb, f.gb = 2 * M + 12, M + 4, 2 * N + 12, N + 4
        elif c.form == "d":
            f.ldb, f.shB = 60, 42
        f.gc = M * N
    else:
        f.lda, f.ldb, f.ldc = K, (K if c.layout == NT else N), N
        if c.form == "b":
            f.lda, f.ga, f.gb, f.ldc, f.gc, f.gbias, f.ld_aux, f.gaux = 2 * K, K, N * K, 2 * N, N, N, 2 * N, N
        elif c.form == "bp":
            f.lda, f.ga, f.gb, f.gbias = 2 * K + 12, K + 4, N * K + 64, N + 4
            f.ldc, f.gc, f.ld_aux, f.gaux = 2 * N + 12, N + 4, 2 * N + 12, N + 4
        elif c.form == "c":
            f.ldc, f.shC = 64, 42
        elif c.form == "d":
            f.ldb, f.shB = 60, 42
        elif c.form == "d1":
            f.ldb, f.shB = 61, 43
    for k, v in c.ov.items():
        setattr(f, k, v)
    return f


_DATA = {}


def _data(c, pow2=False):
    """The case's fp32 inputs and its references, computed once (float64 product, sum_k |a b|, the torch fp32 form)."""
    key = (c.id, pow2)
    if key in _DATA:
        return _DATA[key]
    _DATA.clear()
    M, N, K, g, L, e = c.M, c.N, c.K, c.groups, c.layout, c.epi
    gen = torch.Generator(device=dev).manual_seed(sum(map(ord, c.id)))

    def rnd(*shape):
        if pow2:  # magnitudes in [2^-6, 1]: every scaled operand, split part and product stays normal
            sign = torch.where(torch.rand(*shape, device=dev, generator=gen) < 0.5, -1.0, 1.0)
            return sign * torch.exp2(-6.0 * torch.rand(*shape, device=dev, generator=gen))
        return torch.randn(*shape, device=dev, generator=gen)

    d = NS(bias=None, aux=None, rows=None, t32=None)
    if L == TN:
        d.A, d.B = rnd(g, K, M), rnd(g, K, N) * (1.0 if pow2 else 0.1)
        a64, b64 = d.A.double(), d.B.double()
        d.ref, d.mag = a64.transpose(1, 2) @ b64, a64.abs().transpose(1, 2) @ b64.abs()
        d.db_ref, d.db_mag = a64.sum(1), a64.abs().sum(1)
        d.src = K + 11 if c.gather else K
    else:
        d.A = rnd(g, M, K)
        d.B = (rnd(g, N, K) if L == NT else rnd(g, K, N)) * (1.0 if pow2 else 1.0 / math.sqrt(K))
        op = (lambda b: b.transpose(1, 2)) if L == NT else (lambda b: b)
        acc, acc32 = d.A.double() @ op(d.B.double()), d.A @ op(d.B)
        d.mag = d.A.double().abs() @ op(d.B.double().abs())
        if e in (1, 2, 5):
            d.bias = rnd(g, 1, N)
            acc, acc32, d.mag = acc + d.bias.double(), acc32 + d.bias, d.mag + d.bias.double().abs()
        if e in (3, 6):
            pre = rnd(g, M, N)
            d.aux = torch.nn.functional.elu(pre) if e == 3 else torch.tanh(pre)
        x, x64 = d.aux, (d.aux.double() if d.aux is not None else None)
        d.ref, d.t32 = {0: lambda: (acc, None), 1: lambda: (acc, None),
                        2: lambda: (torch.nn.functional.elu(acc), torch.nn.functional.elu(acc32)),
                        5: lambda: (torch.tanh(acc), torch.tanh(acc32)),
                        3: lambda: (acc * torch.where(x64 > 0, torch.ones_like(x64), x64 + 1),
                                    acc32 * torch.where(x > 0, torch.ones_like(x), x + 1)),
                        6: lambda: (acc * (1 - x64 * x64), acc32 * (1 - x * x))}[e]()
        d.src = M + 37 if c.gather else M
    if c.gather:
        cnt = K if L == TN else M
        perm = torch.randperm(d.src, device=dev, generator=gen)
        d.rows = perm[:cnt].contiguous()
        # the list's own slack names a row of the source that no product row selects (it holds poison)
        d.rowlist = torch.cat([d.rows, perm[cnt:cnt + 1].expand(SLACK)]).contiguous()
    _DATA[key] = d
    return d


def _run(c, fill, mask=None, planes=None, scale=(1.0, 1.0), pow2=False):
    """One launch of the case in a fresh arena whose operand slack holds `fill`.  Asserts the footprint; returns the
    product (a copy), db, the path report and the split count."""
    d, f = _data(c, pow2), _geometry(c)
    M, N, K, g, L, e = c.M, c.N, c.K, c.groups, c.layout, c.epi
    mask = c.mask if mask is None else mask
    planes = c.planes if planes is None else planes
    sel = d.rows if c.gather else slice(0, K if L == TN else M)
    bias = aux = ws = db = None
    need = 0
    if L == TN:
        A = Buf(g, K, M, f.lda, f.ga, f.shA, fill)
        A.view.copy_(d.A * scale[0])
        B = Buf(g, d.src, N, f.ldb, f.gb, f.shB, fill)
        B.view[:, sel] = d.B * scale[1]
        out = Buf(g, M, N, N, M * N, 0, SENT)
        db = Buf(g, 1, M, M, M, 0, SENT)
        splits = _pick_splits(M, N, K, g)
        need = splits * g * (M * N + M)
    else:
        A = Buf(g, d.src, K, f.lda, f.ga, f.shA, fill)
        A.view[:, sel] = d.A * scale[0]
        B = Buf(g, N if L == NT else K, K if L == NT else N, f.ldb, f.gb, f.shB, fill)
        B.view.copy_(d.B * scale[1])
        out = Buf(g, M, N, f.ldc, f.gc, f.shC, SENT)
        if d.bias is not None:
            bias = Buf(g, 1, N, N, f.gbias, 0, fill)
            bias.view.copy_(d.bias * (scale[0] * scale[1]))
        if d.aux is not None:
            aux = Buf(g, M, N, f.ld_aux, f.gaux, 0, fill)
            aux.view.copy_(d.aux)
        if planes:
            need = -(-3 * g * N * (-(-K // 16) * 16) // 2)
    if need:
        ws = torch.full((need + SLACK * SLACK,), SENT, dtype=torch.int32, device=dev)
    path, splits_out = C.c_int32(-1), C.c_int32(-1)
    desc = _abi.LrlGemmDesc(layout=L, epi=e, M=M, N=N, K=K, groups=g, planes=int(planes), splits=0,
                            A=A.ptr, B=B.ptr, C=out.ptr, bias=(db or bias).ptr if (db or bias) else None,
                            aux=aux.ptr if aux else None, rows=d.rowlist.data_ptr() if c.gather else None,
                            workspace=ws.data_ptr() if need else None, lda=f.lda, ldb=f.ldb, ldc=f.ldc,
                            ld_aux=f.ld_aux, ga=f.ga, gb=f.gb, gc=f.gc, gbias=f.gbias, gaux=f.gaux,
                            workspace_floats=need, path_out=C.pointer(path), splits_out=C.pointer(splits_out))
    lib = _abi.lib()
    prev = lib.lrl_debug_gemm_paths(C.c_int32(mask))
    try:
        _abi.check(lib.lrl_gemm_f32_ex(C.byref(desc), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
    finally:
        lib.lrl_debug_gemm_paths(C.c_int32(prev))
    assert out.untouched_outside(SENT), "a store outside the groups x M x N product"
    if need:
        assert bool((ws[need:] == SENT).all()), "a store past the workspace's used part"
    if L == TN:
        assert splits_out.value == splits
        assert db.untouched_outside(SENT), "a store outside db"
    p = path.value
    return NS(out=out.view.clone(), db=db.view.clone() if db else None, splits=splits_out.value,
              path=(_abi.GEMM_FAMILIES.get(p & 0xff, "?"), (p >> 8) & 0xff, (p >> 16) & 0xff, bool(p >> 24)))


def _check_path(c, r, expect=None):
    expect = expect or c.expect
    assert r.path[:len(expect)] == tuple(expect), f"{c.id}: ran on {r.path}, meant for {expect}"


def _worst(fam, kind, v):
    if v > WORST.get((fam, kind), 0.0):
        WORST[(fam, kind)] = v


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_family_at_the_updates_operand_forms(c):
    d = _data(c)
    r = _run(c, NAN_BITS)
    _check_path(c, r)
    fam = r.path[0]
    # value
    assert torch.isfinite(r.out).all()
    if d.t32 is None:
        rel = ((r.out.double() - d.ref).abs() / d.mag).max().item()
        print(f"{c.id}: {r.path} splits {r.splits} rel {rel:.3e}")
        _worst(fam, "rel", rel)
        assert rel <= 1e-6, rel
    else:
        e_nat, e_t32 = (r.out.double() - d.ref).abs().max().item(), (d.t32.double() - d.ref).abs().max().item()
        print(f"{c.id}: {r.path} native {e_nat:.3e} torch-fp32 {e_t32:.3e} ratio {e_nat / e_t32:.2f}")
        _worst(fam, "ratio", e_nat / e_t32)
        assert e_nat <= 2.0 * e_t32
    if c.layout == TN:
        assert torch.isfinite(r.db).all()
        rel = ((r.db[:, 0].double() - d.db_ref).abs() / d.db_mag).max().item()
        _worst(fam, "db rel", rel)
        assert rel <= 1e-6, rel
    # independence from padding (and run-to-run determinism)
    r2 = _run(c, BIG_BITS)
    assert r2.path == r.path
    assert torch.equal(r.out.view(torch.int32), r2.out.view(torch.int32)), "the result depends on operand padding"
    if c.layout == TN:
        assert torch.equal(r.db.view(torch.int32), r2.db.view(torch.int32)), "db depends on operand padding"
    # the same bits as gemm_x6_kernel
    if c.twin is not None:
        rx = _run(c, NAN_BITS, mask=c.twin, planes=False)
        _check_path(c, rx, ("x6",))
        assert torch.equal(r.out.view(torch.int32), rx.out.view(torch.int32)), (r.out - rx.out).abs().max().item()
        if c.layout == TN:
            assert torch.equal(r.db.view(torch.int32), rx.db.view(torch.int32))
    RECORDED.setdefault(fam, set()).add(r.path[1:])


@pytest.mark.parametrize("c", SCALE_CASES, ids=[c.id for c in SCALE_CASES])
def test_power_of_two_scaling_commutes(c):
    """Operands scaled by 2^30 and by 2^-30 (all values stay normal): the rescaled result has the bits of the unscaled
    one.  The fp32 MFMA and the exact three-way bf16 split commute with a power-of-two scale; an absolute threshold
    anywhere in a kernel does not."""
    base = _run(c, NAN_BITS, pow2=True)
    _check_path(c, base)
    for s in (2.0 ** 30, 2.0 ** -30):
        r = _run(c, NAN_BITS, scale=(s, s), pow2=True)
        assert r.path == base.path
        assert torch.equal((r.out / (s * s)).view(torch.int32), base.out.view(torch.int32)), s
        if c.layout == TN:
            assert torch.equal((r.db / s).view(torch.int32), base.db.view(torch.int32)), s


@pytest.mark.parametrize("fam", sorted(FAM))
def test_every_family_is_reached(fam):
    """Each family id appears in a passing case's path report (a dispatch change that empties a family's cases fails
    here even if every remaining case passes).  Run on its own, the family's first case is launched here."""
    mine = [c for c in CASES if c.expect[0] == fam]
    assert mine, f"no case is meant for {fam}"
    if fam not in RECORDED:
        r = _run(mine[0], NAN_BITS)
        _check_path(mine[0], r)
        RECORDED.setdefault(fam, set()).add(r.path[1:])
    tiles = sorted(RECORDED[fam])
    print(f"{fam}: tiles {tiles}; worst " +
          ", ".join(f"{k[1]} {v:.3e}" for k, v in sorted(WORST.items()) if k[0] == fam))
    assert tiles


# a shape and switch setting that would reach each family: (family, M, N, K, mask, planes)
UNOFFERED_ROUTES = [("x6", 128, 128, 64, 0, False), ("x6d", 128, 128, 64, 8, False),
                    ("glds32", 128, 128, 64, 16, False), ("glds", 128, 128, 48, 16, False),
                    ("staged", 129, 70, 40, 16, False), ("thin16", 256, 24, 512, 0, False),
                    ("thin32", 256, 24, 512, 32, False), ("x6p", 64, 128, 32, 0, True)]
UNOFFERED_PAIRS = [(NT, 3), (NN, 1), (NN, 2)]


@pytest.mark.parametrize("layout,epi", UNOFFERED_PAIRS, ids=["nt-e3", "nn-e1", "nn-e2"])
@pytest.mark.parametrize("route", UNOFFERED_ROUTES, ids=[r[0] for r in UNOFFERED_ROUTES])
def test_an_unoffered_pair_is_refused_in_front_of_every_family(route, layout, epi):
    """A (layout, epilogue) pair outside the library's table is an error whatever family the shape and the switches
    would pick, and nothing is written.  Bias and aux are real buffers of full extent: a dispatch mistake shows as a
    return code of 0 or a touched output, never as a read through a null pointer."""
    _, M, N, K, mask, planes = route
    A = Buf(1, M, K, K, 0, 0, NAN_BITS)
    B = Buf(1, N, K, K, 0, 0, NAN_BITS) if layout == NT else Buf(1, K, N, N, 0, 0, NAN_BITS)
    bias, aux = Buf(1, 1, N, N, 0, 0, NAN_BITS), Buf(1, M, N, N, 0, 0, NAN_BITS)
    for b in (A, B, bias, aux):
        b.view.fill_(0.25)
    out = Buf(1, M, N, N, 0, 0, SENT)
    need = -(-3 * N * (-(-K // 16) * 16) // 2) if planes else 0
    ws = torch.full((need + SLACK,), SENT, dtype=torch.int32, device=dev)
    desc = _abi.LrlGemmDesc(layout=layout, epi=epi, M=M, N=N, K=K, groups=1, planes=int(planes), splits=0,
                            A=A.ptr, B=B.ptr, C=out.ptr, bias=bias.ptr, aux=aux.ptr,
                            workspace=ws.data_ptr() if planes else None, workspace_floats=need,
                            lda=K, ldb=K if layout == NT else N, ldc=N, ld_aux=N)
    lib = _abi.lib()
    before = lib.lrl_debug_gemm_paths(C.c_int32(mask))
    try:
        rc = lib.lrl_gemm_f32_ex(C.byref(desc), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    finally:
        assert lib.lrl_debug_gemm_paths(C.c_int32(before)) == mask
    assert rc != 0
    assert bool((out.flat == SENT).all()), "a refused product wrote to its output"
    assert bool((ws[need:] == SENT).all())
    assert lib.lrl_debug_gemm_paths(C.c_int32(before)) == before   # the switches are as the test found them


def test_an_empty_split_is_refused():
    """A split count that leaves a split without rows is an error (production never produces one), and nothing is
    written."""
    A, B = Buf(1, 96, 64, 64, 0, 0, NAN_BITS), Buf(1, 96, 64, 64, 0, 0, NAN_BITS)
    out = Buf(1, 64, 64, 64, 0, 0, SENT)
    ws = torch.full((8 * (64 * 64 + 64),), SENT, dtype=torch.int32, device=dev)
    desc = _abi.LrlGemmDesc(layout=TN, epi=4, M=64, N=64, K=96, groups=1, splits=8, A=A.ptr, B=B.ptr, C=out.ptr,
                            workspace=ws.data_ptr(), workspace_floats=ws.numel(), lda=64, ldb=64, ldc=64)
    assert _abi.lib().lrl_gemm_f32_ex(C.byref(desc), None) != 0   # 8 splits of 16 rows: the last two are empty
    torch.cuda.synchronize()
    assert bool((out.flat == SENT).all())
    assert bool((ws == SENT).all())
