"""Weight-gradient kernels (conv_wgrad.hip, conv_wgrad_taps.hip) element by element against fp64: every tile of the general
kernel, the normalise-on-load template, the tap-sharing kernel and the ordered slab reduce.

References are tests.util.wgrad_fp64 on the CPU from the rounded operands; tests.util.assert_elementwise holds EVERY element of
dW to the worst-case bound of an fp32 sum of k = M + splits + 2 terms (M = N*OH*OW products, `splits` partial sums), so one wrong
tap, pixel or channel fails.  Every case first asserts the variant fn_conv2d_variant names for it: a heuristic change cannot drop
the coverage silently.

All cases keep M <= tests.util.WGRAD_MAX_M = 2048: a dropped pixel term is about absref / M and the bound about M 2^-24 absref,
so the check sees a single missing term only while M^2 << 2^24 (tests/test_conv_refs_host.py plants such errors into every case
below and shows them rejected)."""
import ctypes as C
import functools

import pytest
import torch

from facenet_amd import _lib
from tests.util import (ACC_STAT_BITS, WGRAD_MAX_M, assert_elementwise, conv_desc, lp_dtype, ptr, stream, to_acc, wgrad_fp64, wgrad_k,
                        wgrad_operands, wgrad_pixels)

pytestmark = pytest.mark.gpu

DTYPES = [_lib.FN_BF16, _lib.FN_F16]
TAPS = 5064090
NORM_FLAG = _lib.VARIANT_FLAG

# Every FN_WGRAD_TILES instantiation is reachable (final_wgrad_tile); maps under 32 pixels keep k x k layers off the tap-sharing
# kernel.  Where the first layer has M <= 64 (one 64-pixel stage: a forced split is clamped to one piece) a second one with more
# images can be split.                                   N, H, W, Cin, Cout, kh, kw, stride, ph, pw
TILE_CASES = {
    32064: [(2, 17, 17, 256, 32, 1, 1, 1, 0, 0)],                                          # M = 578
    64064: [(2, 5, 5, 80, 80, 3, 3, 1, 1, 1), (4, 5, 5, 80, 80, 3, 3, 1, 1, 1)],            # K = 720: ragged column tile, ragged cout tile
    64128: [(2, 5, 5, 312, 192, 3, 3, 1, 1, 1), (3, 5, 5, 312, 192, 3, 3, 1, 1, 1)],        # K = 2808, 66 tiles
    128064: [(2, 5, 5, 232, 256, 3, 3, 1, 1, 1), (3, 5, 5, 232, 256, 3, 3, 1, 1, 1)],       # K = 2088, 66 tiles
    128128: [(5, 3, 3, 1792, 640, 1, 1, 1, 0, 0), (9, 3, 3, 1792, 640, 1, 1, 1, 0, 0)],     # 70 tiles, M = 45 < one stage / M = 81
    32128: [(2, 5, 5, 1184, 32, 7, 1, 1, 3, 0), (3, 5, 5, 1184, 32, 7, 1, 1, 3, 0)],        # K = 8288
}
TILE_PARAMS = [(t, g) for t, geos in TILE_CASES.items() for g in geos]

# ordered slab reduce: forced splits (chunks are whole 64-pixel stages); all three layers are one 64x64 group
REDUCE_CASES = [((3, 15, 15, 64, 64, 1, 1, 1, 0, 0), 11),       # M = 675: 11 slabs, the last one short; one unrolled pass + a two-slab tail
                ((2, 9, 9, 1088, 64, 1, 1, 1, 0, 0), 3),        # tail loop only; 69632 floats: a second, ragged trip of the 16384 x 4 grid
                ((17, 8, 8, 64, 64, 1, 1, 1, 0, 0), 17)]        # M = 1088: two unrolled passes, no tail

# normalise-on-load (NORM = true): (case, tile); 'same' padding must stay zero, not relu(shift)
NORM_CASES = [((2, 17, 17, 32, 32, 3, 3, 1, 1, 1), 32064), ((3, 8, 8, 128, 128, 1, 7, 1, 0, 3), 64064), ((2, 15, 15, 32, 64, 3, 3, 1, 0, 0), 64064),
              ((3, 9, 9, 64, 80, 1, 1, 1, 0, 0), 64064), ((2, 17, 17, 192, 256, 3, 3, 2, 0, 0), 64064), ((2, 5, 5, 312, 192, 3, 3, 1, 1, 1), 64128),
              ((2, 5, 5, 232, 256, 3, 3, 1, 1, 1), 128064)]

# tap-sharing kernel: test_gpu_conv.TAPS_CASES with the 37x37 map shrunk to 31x31 (M <= 2048, tiles still cross the image boundary)
TAPS_GEOS = [
    (2, 19, 19, 32, 64, 3, 3, 1, 0, 0),        # 2b-like, 'valid'
    (2, 17, 17, 32, 32, 3, 3, 1, 1, 1),        # block35 3x3 'same', 32 couts
    (2, 31, 31, 80, 192, 3, 3, 1, 0, 0),       # 4a: Cin = 80 -> the third 32-channel slice is half empty
    (2, 35, 35, 192, 256, 3, 3, 2, 0, 0),      # 4b-like stride 2 (35 -> 17)
    (2, 17, 17, 256, 384, 3, 3, 2, 0, 0),      # reduction_a stride 2 on an odd map (17 -> 8)
    (3, 8, 8, 128, 128, 1, 7, 1, 0, 3),        # block17 1x7
    (3, 8, 8, 128, 128, 7, 1, 1, 3, 0),        # block17 7x1
    (1, 45, 39, 32, 40, 3, 3, 1, 1, 1),        # N = 1, ragged tiles, Cout = 40 (one partly empty cout tile)
    (1, 4, 8, 64, 64, 3, 3, 1, 1, 1),          # OH * OW exactly 32: the smallest map the kernel takes
    (2, 9, 9, 40, 72, 3, 3, 1, 1, 1),          # second 32-channel slice a quarter full, second 64-cout tile an eighth full
    (2, 18, 18, 64, 64, 3, 3, 2, 0, 0),        # stride 2 on an even map (18 -> 8): the last row and column feed no output
    (2, 9, 5, 64, 64, 1, 7, 1, 0, 3),          # 1x7 on a map narrower than the kernel
    (2, 5, 9, 64, 64, 7, 1, 1, 3, 0),          # 7x1 on a map lower than the kernel
]
NOT_TAPS_GEO = (1, 3, 9, 64, 64, 3, 3, 1, 1, 1)     # 27 output pixels: stays on the general kernel

# the layer shapes of Inception-ResNet-v2 under the library's own variant: (case, fn_conv2d_variant(d, 2))
V2_CASES = [
    ((2, 17, 17, 48, 64, 5, 5, 1, 2, 2), 64064),        # Mixed_5a 5x5: 25 taps, not a layer of the tap-sharing kernel
    ((2, 17, 17, 32, 48, 3, 3, 1, 1, 1), TAPS),         # block35 0b (Cout = 48: a cout tile three quarters full)
    ((2, 17, 17, 48, 64, 3, 3, 1, 1, 1), TAPS),         # block35 0c (Cin = 48: the second 32-channel slice half empty)
    ((2, 17, 17, 128, 320, 1, 1, 1, 0, 0), 64064),      # block35 up
    ((2, 17, 17, 320, 32, 1, 1, 1, 0, 0), 32064),       # block35 in
    ((2, 17, 17, 320, 384, 3, 3, 2, 0, 0), TAPS),       # Mixed_6a stride 2
    ((3, 8, 8, 1088, 192, 1, 1, 1, 0, 0), 64064),       # block17 in
    ((3, 8, 8, 128, 160, 1, 7, 1, 0, 3), TAPS),         # block17 1x7 (Cout = 160)
    ((3, 8, 8, 160, 192, 7, 1, 1, 3, 0), TAPS),         # block17 7x1 (Cin = 160)
    ((3, 8, 8, 384, 1088, 1, 1, 1, 0, 0), 64064),       # block17 up
    ((3, 8, 8, 256, 288, 3, 3, 2, 0, 0), 64128),        # Mixed_7a stride 2 (27 output pixels: the general kernel)
    ((3, 8, 8, 288, 320, 3, 3, 2, 0, 0), 64064),
    ((5, 3, 3, 2080, 192, 1, 1, 1, 0, 0), 64064),       # block8 in: K = 2080 = 32.5 column tiles of 64
    ((5, 3, 3, 192, 224, 1, 3, 1, 0, 1), 64064),        # block8 1x3 (Cout = 224)
    ((5, 3, 3, 224, 256, 3, 1, 1, 1, 0), 64064),        # block8 3x1 (Cin = 224)
    ((5, 3, 3, 448, 2080, 1, 1, 1, 0, 0), 64064),       # block8 up: 32.5 cout tiles
    ((5, 3, 3, 2080, 1536, 1, 1, 1, 0, 0), 128064),     # Conv2d_7b
    ((7, 1, 1, 1536, 128, 1, 1, 1, 0, 0), 64064),       # Bottleneck
    ((1, 35, 35, 32, 48, 3, 3, 1, 1, 1), TAPS),         # block35 0b at 299 pixels: M = 1225, the one case here above M = 578 (the
    #                                                     layer is listed for the forward's halo kernel; its dW is held too, M <= WGRAD_MAX_M)
]

ALL_WGRAD_CASES = ([g for _, g in TILE_PARAMS] + [g for g, _ in REDUCE_CASES] + [g for g, _ in NORM_CASES] + TAPS_GEOS + [NOT_TAPS_GEO]
                   + [g for g, _ in V2_CASES])
assert all(wgrad_pixels(g) <= WGRAD_MAX_M for g in ALL_WGRAD_CASES)


class WgradOut(C.Structure):
    """First member of every per-layer record fn_conv2d_wgrad_group_build writes (csrc/wgrad_taps.h): where the layer's result
    goes.  ws == NULL: stored straight into dw; otherwise split z stores slab z of ws and the reduce adds the slabs in order."""
    _fields_ = [("dw", C.c_void_p), ("ws", C.c_void_p), ("Cout", C.c_int32), ("KTOT", C.c_int32), ("splits", C.c_int32), ("store", C.c_int32)]


@functools.lru_cache(maxsize=4)
def _reference(case, dt, seed):
    """(x, dy) on the CPU and the fp64 (dW, |.| sums) of a case: computed once, shared, never modified."""
    x, dy = wgrad_operands(case, dt, seed)
    ref, aref = wgrad_fp64(x, dy, *case[5:10])
    return x, dy, ref, aref


def _place(t, sliced):
    """The operand on the device: contiguous, or channels [8, 8 + C) of a buffer whose neighbour channels hold NaN (an element
    of dW depends only on its own input and output channel: a 16-byte over-read of a neighbour cannot legitimately reach it)."""
    if not sliced:
        return t.cuda(), 0
    b = torch.full(t.shape[:-1] + (t.shape[-1] + 16,), float("nan"), dtype=t.dtype)
    b[..., 8:8 + t.shape[-1]] = t
    return b.cuda(), 8


def _desc(case, dt, xb, x0, dyb, y0, dw, splits=0):
    d = conv_desc(*case[:10], dt, ld_x=xb.shape[-1], ld_y=dyb.shape[-1])
    d.x, d.y, d.dw, d.splits = ptr(xb, x0), ptr(dyb, y0), ptr(dw), splits
    return d


def _cdiv(a, b):
    return -(-a // b)


def _pieces(M, splits):
    """Pieces the general kernel splits M pixels into when `splits` are asked for (plan_wgrad: chunks of whole 64-pixel stages)."""
    chunk = _cdiv(_cdiv(M, splits), 64) * 64
    return _cdiv(M, chunk)


class _Group:
    """One grouped weight-gradient launch (+ the ordered reduce) over descriptors of one variant: the sizing call (ws == NULL)
    and the planning call must agree; the workspace is NaN with a bit-patterned guard behind its last float."""
    GUARD = 64

    def __init__(self, lib, descs, variant, dt):
        self.lib, self.n, self.variant, self.dt = lib, len(descs), variant, dt
        nb = lib.fn_conv2d_wgrad_arg_bytes()
        arr = (_lib.ConvDesc * self.n)(*descs)
        sized = C.c_int64(-1)
        total0 = lib.fn_conv2d_wgrad_group_build(arr, self.n, variant, (C.c_uint8 * (nb * self.n))(), (C.c_int32 * (self.n + 1))(), None, C.byref(sized))
        _lib.check(min(total0, 0), "wgrad_group_build (sizing)")
        self.ws_elems = sized.value
        self.ws = torch.full((self.ws_elems + self.GUARD,), float("nan"), device="cuda")
        self.guard = (torch.arange(self.GUARD, dtype=torch.int32, device="cuda") * 40503 + 0x3A5C3A5C)
        self.ws[self.ws_elems:] = self.guard.view(torch.float32)
        host_args, host_prefix, planned = (C.c_uint8 * (nb * self.n))(), (C.c_int32 * (self.n + 1))(), C.c_int64(-1)
        self.total = lib.fn_conv2d_wgrad_group_build(arr, self.n, variant, host_args, host_prefix, ptr(self.ws), C.byref(planned))
        assert (self.total, planned.value) == (total0, sized.value), "sizing and planning calls disagree"
        self.prefix = list(host_prefix)
        assert self.prefix[0] == 0 and self.prefix[-1] == self.total and all(b > a for a, b in zip(self.prefix, self.prefix[1:]))
        self.out = [WgradOut.from_buffer_copy(bytes(host_args)[i * nb:i * nb + C.sizeof(WgradOut)]) for i in range(self.n)]
        self.dev_args = torch.frombuffer(bytearray(host_args), dtype=torch.uint8).cuda()
        self.dev_prefix = torch.tensor(self.prefix, dtype=torch.int32, device="cuda")

    def slabs(self, i):
        """Number of slabs of layer i (0: not split, stored straight into dw)."""
        return self.out[i].splits if self.out[i].ws else 0

    def slab(self, i, z):
        o = self.out[i]
        n = o.Cout * o.KTOT
        off = (o.ws - self.ws.data_ptr()) // 4 + z * n
        assert 0 <= off and off + n <= self.ws_elems
        return self.ws[off:off + n]

    def run(self):
        self.ws[:self.ws_elems] = float("nan")
        _lib.check(self.lib.fn_conv2d_wgrad_grouped(ptr(self.dev_args), ptr(self.dev_prefix), self.n, self.total, self.variant, self.dt, stream()))
        _lib.check(self.lib.fn_conv2d_wgrad_reduce(ptr(self.dev_args), self.n, stream()))
        torch.cuda.synchronize()
        assert torch.equal(self.ws[self.ws_elems:].view(torch.int32), self.guard), "workspace floats beyond ws_elems changed"


def _run_grouped_twice(lib, d, variant, dt, dw, ref, aref, M, what, want_slabs=None):
    """One layer through the grouped path into a NaN-filled dW, twice: within the bound, the same bits both times."""
    grp = _Group(lib, [d], variant, dt)
    if want_slabs is not None:
        assert grp.slabs(0) == want_slabs and grp.ws_elems == want_slabs * dw.numel(), (what, grp.slabs(0), grp.ws_elems)
    runs = []
    for _ in range(2):
        dw.fill_(float("nan"))
        grp.run()
        runs.append(dw.clone())
    assert_elementwise(runs[0], ref, aref, wgrad_k(M, grp.slabs(0)), dt, what, out_f32=True)
    assert torch.equal(runs[0], runs[1]), what + ": two grouped launches differ"
    return grp


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("tile,case", TILE_PARAMS)
def test_wgrad_every_tile_against_fp64(lib, tile, case, dt):
    """conv_wgrad_kernel / conv_wgrad_grouped_kernel, all six FN_WGRAD_TILES instantiations (each named by fn_conv2d_variant):
    the single launch (atomics into a zeroed dW) with the library's and a forced split, the grouped launch unsplit (direct
    stores into a NaN-filled dW) and split (NaN-filled slabs + the ordered reduce), each grouped launch twice with the same
    bits; then all of it again with x and dy as channel slices between NaN channels."""
    N, H, W, Cin, Cout, kh, kw, s, ph, pw = case
    M = wgrad_pixels(case)
    x, dy, ref, aref = _reference(case, dt, 700)
    for sliced in (False, True):
        (xb, x0), (dyb, y0) = _place(x, sliced), _place(dy, sliced)
        dw = torch.zeros(Cout, kh, kw, Cin, dtype=torch.float32, device="cuda")
        what = f"{tile} {case} {'sliced' if sliced else 'contiguous'}"
        d = _desc(case, dt, xb, x0, dyb, y0, dw)
        assert lib.fn_conv2d_variant(C.byref(d), 2) == tile
        for splits in (0, 3):
            d.splits = splits
            dw.zero_()
            _lib.check(lib.fn_conv2d_wgrad(C.byref(d), stream()))
            torch.cuda.synchronize()
            pieces = _pieces(M, splits) if splits else _cdiv(M, 64)          # the library's own choice: at most one piece per stage
            assert_elementwise(dw, ref, aref, wgrad_k(M, pieces), dt, f"{what}, single launch, splits {splits}", out_f32=True)
        d.splits = 1
        _run_grouped_twice(lib, d, tile, dt, dw, ref, aref, M, what + ", grouped, unsplit", want_slabs=0)
        d.splits = 3
        pieces = _pieces(M, 3)                                                # M <= 64: one stage, the request is clamped to one piece
        _run_grouped_twice(lib, d, tile, dt, dw, ref, aref, M, what + ", grouped, splits 3", want_slabs=pieces if pieces > 1 else 0)
    assert any(_pieces(wgrad_pixels(g), 3) > 1 for g in TILE_CASES[tile])     # every tile has a layer that really splits


@pytest.mark.parametrize("dt", DTYPES)
def test_wgrad_slab_reduce_adds_the_slabs_in_order(lib, dt):
    """wgrad_reduce_kernel (eight slab reads in flight + a tail loop, a grid-stride loop over the layer): three layers of one
    64x64 group with forced splits 11, 3 and 17.  dW is within the fp64 bound AND is the fp32 sum of the slabs in slab order bit
    for bit (the slabs are read back from the workspace and added with torch); floats beyond ws_elems keep their bits."""
    descs, keep = [], []
    for i, (case, splits) in enumerate(REDUCE_CASES):
        N, H, W, Cin, Cout, kh, kw, s, ph, pw = case
        x, dy = wgrad_operands(case, dt, 710 + 10 * i)
        ref, aref = wgrad_fp64(x, dy, kh, kw, s, ph, pw)
        xb, dyb = x.cuda(), dy.cuda()
        dw = torch.full((Cout, kh, kw, Cin), float("nan"), dtype=torch.float32, device="cuda")
        d = _desc(case, dt, xb, 0, dyb, 0, dw, splits)
        assert lib.fn_conv2d_variant(C.byref(d), 2) == 64064
        descs.append(d)
        keep.append((xb, dyb, dw, ref, aref))
    grp = _Group(lib, descs, 64064, dt)
    assert [grp.slabs(i) for i in range(3)] == [11, 3, 17] == [_pieces(wgrad_pixels(c), sp) for c, sp in REDUCE_CASES]
    assert grp.ws_elems == sum(sp * k[2].numel() for (_, sp), k in zip(REDUCE_CASES, keep))
    first = None
    for _ in range(2):
        for k in keep:
            k[2].fill_(float("nan"))
        grp.run()
        got = [k[2].clone() for k in keep]
        assert first is None or all(torch.equal(a, b) for a, b in zip(first, got))
        first = got
    for i, ((case, splits), (xb, dyb, dw, ref, aref)) in enumerate(zip(REDUCE_CASES, keep)):
        assert_elementwise(dw, ref, aref, wgrad_k(wgrad_pixels(case), splits), dt, f"reduce layer {i}", out_f32=True)
        total = grp.slab(i, 0).clone()
        for z in range(1, splits):
            total += grp.slab(i, z)
        assert not bool(torch.isnan(total).any()), f"reduce layer {i}: a slab element was not written"
        assert torch.equal(total.view(torch.int32), dw.view(-1).view(torch.int32)), f"reduce layer {i}: dW is not the ordered sum of its slabs"


def _bn_operand(lib, case, dt, seed):
    """The raw tensor (channels [8, 8 + Cin) of a wider buffer), its replicated statistics at channel offset 16 of a wider
    channel space, beta, and z = what fn_bn_relu_train_fwd writes from them (the tensor tests/test_gpu_elementwise_edges.py
    holds element-wise)."""
    N, H, W, Cin = case[:4]
    M_in = N * H * W
    ld = Cin + 16
    g = torch.Generator().manual_seed(seed)
    raw = (torch.randn((N, H, W, ld), generator=g) * 1.5).to(lp_dtype(dt)).cuda()
    raw[..., :8] = raw[..., 8 + Cin:] = float("nan")
    rawf = raw[..., 8:8 + Cin].float().reshape(M_in, Cin)
    reps, CBs = 4, Cin + 24
    stats = torch.zeros(reps, 2 * CBs, dtype=torch.int64, device="cuda")
    part = torch.arange(M_in, device="cuda") % reps
    for r in range(reps):
        stats[r, 16:16 + Cin] = to_acc(rawf[part == r].sum(0), ACC_STAT_BITS)
        stats[r, CBs + 16:CBs + 16 + Cin] = to_acc((rawf[part == r] ** 2).sum(0), ACC_STAT_BITS)
    beta = (torch.randn(CBs, generator=g) * 0.3).cuda()
    z = torch.full_like(raw, float("nan"))                 # the materialised operand sits between NaN channels
    sc, sh = torch.zeros(CBs, device="cuda"), torch.zeros(CBs, device="cuda")
    _lib.check(lib.fn_bn_relu_train_fwd(ptr(raw, 8), ld, ptr(z, 8), ld, M_in, Cin, ptr(stats, 16), CBs, reps, 2 * CBs, ptr(beta, 16),
                                        ptr(sc, 16), ptr(sh, 16), None, None, 0.99, 1e-3, 1, dt, stream()))
    torch.cuda.synchronize()

    def set_norm(d):
        d.x, d.nrm_stats, d.nrm_beta = ptr(raw, 8), ptr(stats, 16), ptr(beta, 16)
        d.nrm_sq_off, d.nrm_replicas, d.nrm_rep_stride, d.nrm_count, d.nrm_eps = CBs, reps, 2 * CBs, M_in, 1e-3
    return raw, z, set_norm, (stats, beta, sc, sh)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case,tile", NORM_CASES)
def test_wgrad_normalise_on_load_against_fp64(lib, case, tile, dt):
    """The NORM = true template, single launch and grouped (variant + 1000000): dW from the RAW tensor + statistics (a slice at
    a non-zero statistics offset) against wgrad_fp64 of the tensor fn_bn_relu_train_fwd writes from the same statistics -- zero
    padding stays zero, it does not become relu(shift) -- and, at splits = 1, bit-equal to the launch on the materialised tensor."""
    N, H, W, Cin, Cout, kh, kw, s, ph, pw = case
    M = wgrad_pixels(case)
    raw, z, set_norm, keep = _bn_operand(lib, case, dt, 730)
    dyb, y0 = _place(wgrad_operands(case, dt, 740)[1], True)
    zs = z[..., 8:8 + Cin]
    assert not bool(torch.isnan(zs).any()) and float(zs.float().max()) > 0 and bool((zs == 0).any())
    ref, aref = wgrad_fp64(zs, dyb[..., 8:8 + Cout], kh, kw, s, ph, pw)
    dw = torch.zeros(Cout, kh, kw, Cin, dtype=torch.float32, device="cuda")
    d = _desc(case, dt, z, 8, dyb, y0, dw, 1)
    _lib.check(lib.fn_conv2d_wgrad(C.byref(d), stream()))              # the materialised operand, general kernel, one piece
    torch.cuda.synchronize()
    plain = dw.clone()
    assert_elementwise(plain, ref, aref, wgrad_k(M, 1), dt, f"{case} materialised", out_f32=True)
    set_norm(d)
    assert lib.fn_conv2d_variant(C.byref(d), 2) == tile                # callers add the flag of a normalise-on-load group themselves
    for splits in (1, 3, 0):
        d.splits = splits
        dw.zero_()
        _lib.check(lib.fn_conv2d_wgrad(C.byref(d), stream()))
        torch.cuda.synchronize()
        pieces = _pieces(M, splits) if splits else _cdiv(M, 64)
        assert_elementwise(dw, ref, aref, wgrad_k(M, pieces), dt, f"{case} nrm single, splits {splits}", out_f32=True)
        if splits == 1:
            assert torch.equal(dw, plain), f"{case}: normalise-on-load differs from the materialised operand"
    d.splits = 1
    _run_grouped_twice(lib, d, tile + NORM_FLAG, dt, dw, ref, aref, M, f"{case} nrm grouped, unsplit", want_slabs=0)
    assert torch.equal(dw, plain), f"{case}: grouped normalise-on-load differs from the materialised operand"
    d.splits = 3
    pieces = _pieces(M, 3)
    _run_grouped_twice(lib, d, tile + NORM_FLAG, dt, dw, ref, aref, M, f"{case} nrm grouped, splits 3", want_slabs=pieces if pieces > 1 else 0)
    with pytest.raises(ValueError):                                    # a normalise-on-load member needs the flagged group
        _Group(lib, [d], tile, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", TAPS_GEOS)
def test_wgrad_tap_sharing_kernel_against_fp64(lib, case, dt):
    """conv_wgrad_taps_kernel (variant 5064090) element by element: unsplit (direct stores into a NaN-filled dW), the library's
    own split, a forced split that does not divide the pixel-tile count and one larger than the tile count (clamped to one tile
    per slab; sizing and planning calls agree), contiguous operands and channel slices between NaN channels; every launch twice
    with the same bits."""
    N, H, W, Cin, Cout, kh, kw, s, ph, pw = case
    M = wgrad_pixels(case)
    x, dy, ref, aref = _reference(case, dt, 750)
    for sliced in (False, True):
        (xb, x0), (dyb, y0) = _place(x, sliced), _place(dy, sliced)
        dw = torch.full((Cout, kh, kw, Cin), float("nan"), dtype=torch.float32, device="cuda")
        what = f"taps {case} {'sliced' if sliced else 'contiguous'}"
        d = _desc(case, dt, xb, x0, dyb, y0, dw, 1)
        assert lib.fn_conv2d_variant(C.byref(d), 2) == TAPS
        _run_grouped_twice(lib, d, TAPS, dt, dw, ref, aref, M, what + ", unsplit", want_slabs=0)
        if not sliced:
            d.splits = 0
            _run_grouped_twice(lib, d, TAPS, dt, dw, ref, aref, M, what + ", library split")
            continue
        d.splits = 1 << 20                                             # more pieces than pixel tiles: one tile per slab
        ntiles = _run_grouped_twice(lib, d, TAPS, dt, dw, ref, aref, M, what + ", splits > tiles").slabs(0) or 1     # 1: a single tile, never split
        assert ntiles <= M and (ntiles > 1 or N * d.OH * d.OW <= 64), ntiles
        odd = [sp for sp in range(2, ntiles) if ntiles % sp]           # a split that does not divide the tile count: a short last slab
        if odd:
            d.splits = odd[0]
            _run_grouped_twice(lib, d, TAPS, dt, dw, ref, aref, M, what + f", splits {odd[0]} of {ntiles} tiles",
                               want_slabs=_cdiv(ntiles, _cdiv(ntiles, odd[0])))
    # the general kernel's single launch of the same descriptor is held to the same reference
    d.splits = 0
    dw.zero_()
    _lib.check(lib.fn_conv2d_wgrad(C.byref(d), stream()))
    torch.cuda.synchronize()
    assert_elementwise(dw, ref, aref, wgrad_k(M, _cdiv(M, 64)), dt, f"taps {case}, single launch", out_f32=True)


@pytest.mark.parametrize("dt", DTYPES)
def test_wgrad_map_below_32_pixels_stays_on_the_general_kernel(lib, dt):
    """A 3x9 map (27 output pixels) next to the 4x8 one above: not a layer for the tap-sharing kernel, and right on the kernel
    that takes it."""
    case = NOT_TAPS_GEO
    N, H, W, Cin, Cout, kh, kw, s, ph, pw = case
    x, dy, ref, aref = _reference(case, dt, 760)
    dw = torch.zeros(Cout, kh, kw, Cin, dtype=torch.float32, device="cuda")
    xb, dyb = x.cuda(), dy.cuda()
    d = _desc(case, dt, xb, 0, dyb, 0, dw, 1)
    variant = lib.fn_conv2d_variant(C.byref(d), 2)
    assert variant == 64064 and not _lib.variant_is_taps(variant)
    with pytest.raises(ValueError):
        _Group(lib, [d], TAPS, dt)
    _run_grouped_twice(lib, d, variant, dt, dw, ref, aref, wgrad_pixels(case), f"{case} grouped", want_slabs=0)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case,variant", V2_CASES)
def test_wgrad_v2_layer_shapes_against_fp64(lib, case, variant, dt):
    """Every layer shape of Inception-ResNet-v2 on the kernel the library itself chooses for it (asserted): the single launch
    with the library's split, then the grouped launch of that variant unsplit (direct stores into a NaN-filled dW) and with the
    library's split, twice with the same bits; x and dy are channel slices between NaN channels."""
    N, H, W, Cin, Cout, kh, kw, s, ph, pw = case
    M = wgrad_pixels(case)
    x, dy, ref, aref = _reference(case, dt, 770)
    (xb, x0), (dyb, y0) = _place(x, True), _place(dy, True)
    dw = torch.zeros(Cout, kh, kw, Cin, dtype=torch.float32, device="cuda")
    d = _desc(case, dt, xb, x0, dyb, y0, dw)
    assert lib.fn_conv2d_variant(C.byref(d), 2) == variant
    _lib.check(lib.fn_conv2d_wgrad(C.byref(d), stream()))
    torch.cuda.synchronize()
    assert_elementwise(dw, ref, aref, wgrad_k(M, _cdiv(M, 64)), dt, f"v2 {case}, single launch", out_f32=True)
    d.splits = 1
    _run_grouped_twice(lib, d, variant, dt, dw, ref, aref, M, f"v2 {case}, grouped, unsplit", want_slabs=0)
    d.splits = 0
    _run_grouped_twice(lib, d, variant, dt, dw, ref, aref, M, f"v2 {case}, grouped, library split")
