"""fp64 oracle of the fused inference blocks (csrc/block_fused.hip) and the inputs that make a comparison with it sharp.

The two blocks, restated from the header comments of block_fused.hip (every convolution is stride 1, zero padded to the same
size; weights are the inference packs of the C ABI, [Cout][taps][Cin], taps row major):

    Block17 (8 x 8 x 896):   t0  = 1x1(x)            t1a = 1x1(x)       t1b = 1x7(t1a)      t1c = 7x1(t1b)
                             out = act(x + scale * (1x1(t0 | t1c) + bias))
    Block35 (17 x 17 x 256): t0  = 1x1(x)            t1a = 1x1(x)       t1b = 3x3(t1a)
                             t2a = 1x1(x)            t2b = 3x3(t2a)     t2c = 3x3(t2b)
                             out = act(x + scale * (1x1(t0 | t1b | t2c) + bias))

Every tower activation is round_lp(relu(sum + bias)); the output is round_lp(act(x + scale * (sum + bias))), act = ReLU or nothing.

A worst-case error bound carried through four dense GEMM stages is far too loose to see an indexing fault (`dense_case`), so
the oracle builds two kinds of input for which the expectation is sharp:

* `exact_case`: ternary inputs and weights, small integer biases, a power-of-two scale.  Every partial sum is an integer that
  fp32 holds exactly in ANY summation order, every tower activation is representable in the storage type, and the fp32 value
  before the one final rounding is exact: the kernel must return the bits of the fp64 chain.  `check_exact` verifies that
  premise and `check_not_vacuous` that the case exercises every tap and every 32-channel k tile; both raise.
* `isolation_case`: every stage but one is an exact selection (one-hot weights, centre tap, zero bias), the remaining stage
  is dense and random.  `interval_forward` derives, with no tuned number, the interval the stored result must lie in:
  the fp32 value of the dense stage lies in s +- gamma_K A (s the fp64 sum, A the sum of the absolute terms, K the GEMM depth
  plus the epilogue operations), rounding and ReLU are monotone, so the stored activation lies in
  [rd(relu(s - E)), rd(relu(s + E))]; selections carry the interval exactly, the final x + scale * (...) widens it by the
  gamma of its few fp32 operations, and the last rounding is monotone again.
"""
import math
from typing import NamedTuple

import numpy as np
import torch

from tests.util import gamma

F16, BF16 = torch.float16, torch.bfloat16
# integers of magnitude <= 2^(p) are exact in a type with p + 1 significand bits; the premise keeps them strictly below
EXACT_LIMIT = {F16: 2 ** 11, BF16: 2 ** 8}


class Layer(NamedTuple):
    name: str
    src: str          # "x", a tower layer, or "mixed" (the concat)
    kh: int
    kw: int
    cin: int
    cout: int

    @property
    def taps(self):
        return self.kh * self.kw

    @property
    def depth(self):
        return self.taps * self.cin

    @property
    def pack_shape(self):
        return (self.cout, self.cin) if self.taps == 1 else (self.cout, self.taps, self.cin)


class Block(NamedTuple):
    name: str
    H: int
    W: int
    C: int
    towers: tuple     # in execution order
    concat: tuple     # names of the layers whose outputs form `mixed`, in channel order
    up: Layer
    scale: float      # the production scale

    @property
    def layers(self):
        return self.towers + (self.up,)

    def layer(self, name):
        return next(L for L in self.layers if L.name == name)


BLOCK17 = Block("block17", 8, 8, 896,
                (Layer("t0", "x", 1, 1, 896, 128), Layer("t1a", "x", 1, 1, 896, 128),
                 Layer("t1b", "t1a", 1, 7, 128, 128), Layer("t1c", "t1b", 7, 1, 128, 128)),
                ("t0", "t1c"), Layer("up", "mixed", 1, 1, 256, 896), 0.10)
BLOCK35 = Block("block35", 17, 17, 256,
                (Layer("t0", "x", 1, 1, 256, 32), Layer("t1a", "x", 1, 1, 256, 32), Layer("t2a", "x", 1, 1, 256, 32),
                 Layer("t1b", "t1a", 3, 3, 32, 32), Layer("t2b", "t2a", 3, 3, 32, 32), Layer("t2c", "t2b", 3, 3, 32, 32)),
                ("t0", "t1b", "t2c"), Layer("up", "mixed", 1, 1, 96, 256), 0.17)
BLOCKS = {"block17": BLOCK17, "block35": BLOCK35}


class Case(NamedTuple):
    block: Block
    dt: torch.dtype
    x: torch.Tensor       # [N, H, W, C] storage type
    w: dict               # layer name -> pack, storage type
    b: dict               # layer name -> fp32 bias
    scale: float
    relu: int
    what: str


def f32_scale(scale):
    """The C ABI takes `scale` as a float: the value the kernel multiplies with."""
    return float(torch.tensor(scale, dtype=torch.float32))


def round_lp(v, dt):
    """fp64 -> storage type the way a kernel gets there: its value is an fp32 number, rounded once to nearest even.  For the
    exact cases the fp64 value IS an fp32 number (`check_exact`); for interval end points rounding through fp32 is what keeps
    the containment argument valid (an fp32 value v >= lo has v = rd32(v) >= rd32(lo))."""
    return v.to(torch.float32).to(dt)


def conv64(x, w, L):
    """Zero-padded stride-1 cross-correlation in the dtype of x, NHWC, w = [Cout][kh * kw][Cin]: one matrix product per tap
    on a shifted view of the padded image."""
    N, H, W, _ = x.shape
    w3 = w.reshape(L.cout, L.taps, L.cin)
    ph, pw = L.kh // 2, L.kw // 2
    xp = x.new_zeros(N, H + 2 * ph, W + 2 * pw, L.cin)
    xp[:, ph:ph + H, pw:pw + W] = x
    out = x.new_zeros(N, H, W, L.cout)
    for ky in range(L.kh):
        for kx in range(L.kw):
            out += xp[:, ky:ky + H, kx:kx + W] @ w3[:, ky * L.kw + kx].T
    return out


class Forward(NamedTuple):
    out: torch.Tensor     # storage type
    acts: dict            # "x" and every tower layer: the stored activations, as fp64
    pre: dict             # every layer: sum + bias before the activation, fp64
    absum: dict           # every layer: sum |terms| + |bias|, fp64 (bounds every partial sum in any order)
    final: torch.Tensor   # x + scale * (sum + bias) before the activation and the rounding, fp64


def forward(case):
    """The fp64 chain, rounded to the storage type where the kernel stores."""
    blk, dt = case.block, case.dt
    acts, pre, absum = {"x": case.x.double()}, {}, {}

    def src_of(L):
        return torch.cat([acts[n] for n in blk.concat], -1) if L.src == "mixed" else acts[L.src]

    for L in blk.layers:
        src, w, b = src_of(L), case.w[L.name].double(), case.b[L.name].double()
        pre[L.name] = conv64(src, w, L) + b
        absum[L.name] = conv64(src.abs(), w.abs(), L) + b.abs()
        if L is not blk.up:
            acts[L.name] = round_lp(torch.relu(pre[L.name]), dt).double()
    final = acts["x"] + f32_scale(case.scale) * pre["up"]
    v = torch.relu(final) if case.relu else final
    return Forward(round_lp(v, dt), acts, pre, absum, final)


# ---- exact cases ------------------------------------------------------------------------------------------------------------
# Weight densities (probability of a non-zero ternary weight) at an input density of 1/2, chosen so that every pre-activation
# stays below EXACT_LIMIT with room to spare while about half of every tower intermediate is non-zero.  Largest |sum + bias|
# on the CPU over EXACT_RUNS: 1047 (Block17 f16), 200 (Block17 bf16), 1048 (Block35 f16), 215 (Block35 bf16); least non-zero
# fraction of a tower intermediate 0.40 (tests/test_fused_block_oracle_host.py prints both for every run).
EXACT_DENSITY = {
    ("block17", F16): {"x": 1 / 2, "t0": 1 / 16, "t1a": 1 / 16, "t1b": 1 / 32, "t1c": 1 / 32, "up": 1 / 16},
    ("block17", BF16): {"x": 1 / 2, "t0": 1 / 16, "t1a": 1 / 16, "t1b": 1 / 64, "t1c": 1 / 128, "up": 1 / 256},
    ("block35", F16): {"x": 1 / 2, "t0": 1 / 8, "t1a": 1 / 8, "t2a": 1 / 8, "t1b": 1 / 8, "t2b": 1 / 8, "t2c": 1 / 8, "up": 1 / 4},
    ("block35", BF16): {"x": 1 / 2, "t0": 1 / 8, "t1a": 1 / 8, "t2a": 1 / 8, "t1b": 1 / 16, "t2b": 1 / 16, "t2c": 1 / 32, "up": 1 / 32},
}

# (seed, N, scale, relu, warm): what the GPU test runs for every block and type.  257 images are more than the 256 CUs, the
# batches of 64 run once plainly and once through the _warm entry point; scales: 0, 1, the production values rounded to a
# power of two (0.125 for both blocks) and negative powers of two.
EXACT_RUNS = (
    (0, 2, 0.125, 1, False),
    (1, 1, 1.0, 0, False),
    (2, 9, -0.25, 0, False),
    (3, 2, 0.0, 1, False),
    (4, 9, 0.125, 0, False),
    (5, 64, 1.0, 1, False),
    (6, 64, 0.125, 0, True),
    (7, 257, -0.5, 1, False),
)


def _ternary(shape, density, g):
    mask = torch.rand(shape, generator=g) < density
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mask * sign).to(torch.float32)


def exact_case(blk, dt, seed, N, scale, relu):
    """Ternary x and weights, biases in {-1, 0, 1}, a power-of-two (or zero) scale; every image has its own content.  Raises if
    the exactness premise fails or the case is vacuous.  Returns (case, Forward)."""
    if scale != 0.0 and math.frexp(abs(scale))[0] != 0.5:
        raise ValueError(f"scale {scale} is no power of two")
    g = torch.Generator().manual_seed(1000 + seed)
    dens = EXACT_DENSITY[(blk.name, dt)]
    w = {L.name: _ternary(L.pack_shape, dens[L.name], g).to(dt) for L in blk.layers}
    b = {L.name: torch.randint(-1, 2, (L.cout,), generator=g).to(torch.float32) for L in blk.layers}
    x = _ternary((N, blk.H, blk.W, blk.C), dens["x"], g).to(dt)
    case = Case(blk, dt, x, w, b, scale, relu, f"{blk.name} {dt} exact seed {seed} N {N} scale {scale} relu {relu}")
    fwd = forward(case)
    check_exact(case, fwd)
    check_not_vacuous(case, fwd)
    return case, fwd


def check_exact(case, fwd):
    """The premise of bit equality: integer operands, every |sum + bias| below EXACT_LIMIT (tower activations representable),
    every sum of absolute terms below 2^24 (partial sums exact in fp32 in any order), final value an fp32 number."""
    lim = EXACT_LIMIT[case.dt]
    for name, t in list(case.w.items()) + list(case.b.items()) + [("x", case.x)]:
        t = t.double()
        if not bool(((t == t.round()) & (t.abs() <= 1)).all()):
            raise ValueError(f"{case.what}: {name} is not ternary")
    for L in case.block.layers:
        m, a = float(fwd.pre[L.name].abs().max()), float(fwd.absum[L.name].max())
        if not m < lim:
            raise ValueError(f"{case.what}: |sum + bias| of {L.name} reaches {m:g}, not below {lim}")
        if not a < 2 ** 24:
            raise ValueError(f"{case.what}: sum of |terms| of {L.name} reaches {a:g}")
    if not torch.equal(fwd.final.to(torch.float32).double(), fwd.final):
        raise ValueError(f"{case.what}: the value before the final rounding is not exact in fp32")
    for n in (L.name for L in case.block.towers):       # representable: storing changed nothing
        if not torch.equal(fwd.acts[n], torch.relu(fwd.pre[n])):
            raise ValueError(f"{case.what}: {n} is not representable in {case.dt}")


def check_not_vacuous(case, fwd):
    """At least a quarter of every tower intermediate is non-zero, every tap of every layer has a non-zero weight in every
    32-channel k tile (so a dropped tile or a wrong tap moves a whole integer somewhere), no two images are alike in x or in
    the expected output (a wrong image index cannot hide), and without the ReLU some output is negative."""
    for L in case.block.towers:
        frac = float((fwd.acts[L.name] != 0).double().mean())
        if frac < 0.25:
            raise ValueError(f"{case.what}: only {frac:.1%} of {L.name} is non-zero")
    for L in case.block.layers:
        w = case.w[L.name].float().reshape(L.cout, L.taps, L.cin // 32, 32)
        if not bool((w != 0).any(3).any(0).all()):
            raise ValueError(f"{case.what}: a (tap, k tile) of {L.name} has no non-zero weight")
    for name, t in (("x", case.x), ("the expected output", fwd.out)):
        if len({t[n].contiguous().view(torch.int16).numpy().tobytes() for n in range(t.shape[0])}) != t.shape[0]:
            raise ValueError(f"{case.what}: two images of {name} are alike")
    if not case.relu and not bool((fwd.out.float() < 0).any()):
        raise ValueError(f"{case.what}: no negative output survives without the ReLU")


# ---- stage isolation --------------------------------------------------------------------------------------------------------
def _one_hot_pack(L, g):
    """Exact selection: output channel o reads input channel sel[o] at the centre tap with weight 1.  Where the layer is
    wider than its input (the up-projection) every input channel is read at least once."""
    reps = -(-L.cout // L.cin)
    sel = torch.cat([torch.randperm(L.cin, generator=g) for _ in range(reps)])[:L.cout]
    if L.cout >= L.cin:
        assert len(set(sel.tolist())) == L.cin
    w = torch.zeros(L.cout, L.taps, L.cin)
    w[torch.arange(L.cout), L.taps // 2, sel] = 1.0
    return w.reshape(L.pack_shape)


def isolation_case(blk, dt, stage, seed, N, relu, scale=None):
    """`stage` gets dense random weights (std 1 / sqrt(depth): activations keep the magnitude of the input) and a bias, every
    other layer is a one-hot selection with zero bias; x is non-negative (it passes ReLUs unchanged), own content per image."""
    g = torch.Generator().manual_seed(2000 + seed)
    w, b = {}, {}
    for L in blk.layers:
        if L.name == stage:
            w[L.name] = (torch.randn(L.pack_shape, generator=g) * L.depth ** -0.5).to(dt)
            b[L.name] = torch.randn(L.cout, generator=g) * 0.1
        else:
            w[L.name] = _one_hot_pack(L, g).to(dt)
            b[L.name] = torch.zeros(L.cout)
    x = (torch.randn(N, blk.H, blk.W, blk.C, generator=g).abs() * 0.5).to(dt)
    scale = blk.scale if scale is None else scale
    return Case(blk, dt, x, w, b, scale, relu, f"{blk.name} {dt} isolated {stage} seed {seed} N {N} relu {relu}")


def dense_case(blk, dt, seed, N, relu):
    """Dense random data in every stage at once, checked against the worst-case interval carried through all four stages
    (`interval_forward` with every layer dense: gamma_K sum |terms| per stage plus the storage rounding of each stage).

    What it is worth: it catches gross faults, NaN and the overflow of an intermediate, and is relied on for nothing finer.
    Measured on the CPU for Block17 with the bound in its |err| <= bound form: a clean fp32 emulation reaches at most 2 % of
    the bound in f16 and 4 % in bf16; a dropped 32-channel k tile, two swapped 1x7 taps and a missing ReLU reach only 8-36 %
    (f16) and 5-11 % (bf16) of it, and a wrong weight row for one channel does not move the worst ratio at all.  Carried as an
    interval through the actual roundings, as here, it is narrower (median width 23 storage steps for Block17 f16, 3 for bf16,
    below 1 for Block35) but still blind where it matters: the Block17 interval contains every element of an emulation
    with a dropped k tile of the 1x7 layer, and of one with a zeroed 1x7 weight.  The exact and the isolation cases find those."""
    g = torch.Generator().manual_seed(3000 + seed)
    w = {L.name: (torch.randn(L.pack_shape, generator=g) * L.depth ** -0.5).to(dt) for L in blk.layers}
    b = {L.name: torch.randn(L.cout, generator=g) * 0.1 for L in blk.layers}
    x = (torch.randn(N, blk.H, blk.W, blk.C, generator=g) * 0.5).to(dt)
    return Case(blk, dt, x, w, b, blk.scale, relu, f"{blk.name} {dt} dense seed {seed} N {N} relu {relu}")


def _require_selection(case, L):
    w, b = case.w[L.name].double().reshape(L.cout, -1), case.b[L.name]
    if not (bool(((w == 0) | (w == 1)).all()) and bool(((w != 0).sum(1) == 1).all()) and bool((b == 0).all())):
        raise ValueError(f"{case.what}: {L.name} is treated as an exact selection but is none")


def interval_forward(case, dense):
    """(lo, hi) in the storage type: the interval every stored output element of a correct fp32-accumulating kernel lies in.
    `dense`: the layers whose fp32 sum carries a rounding error (gamma_K sum |terms|); every other layer must be a one-hot
    selection, whose sum has one non-zero term and is exact in any order.  Returns also the intervals of the intermediates."""
    blk, dt = case.block, case.dt
    lo, hi = {"x": case.x.double()}, {"x": case.x.double()}

    def src_of(d, L):
        return torch.cat([d[n] for n in blk.concat], -1) if L.src == "mixed" else d[L.src]

    for L in blk.layers:
        w, b = case.w[L.name].double(), case.b[L.name].double()
        wp, wn = w.clamp_min(0), w.clamp_max(0)
        slo_in, shi_in = src_of(lo, L), src_of(hi, L)
        s_lo = conv64(slo_in, wp, L) + conv64(shi_in, wn, L) + b
        s_hi = conv64(shi_in, wp, L) + conv64(slo_in, wn, L) + b
        A = conv64(torch.maximum(slo_in.abs(), shi_in.abs()), w.abs(), L) + b.abs()
        if L.name in dense:
            depth = L.depth
        else:
            _require_selection(case, L)
            depth = 0
        if L is not blk.up:
            # fp32: `depth` accumulations and the bias add
            E = gamma(depth + 1) * A if depth else 0.0
            lo[L.name] = round_lp(torch.relu(s_lo - E), dt).double()
            hi[L.name] = round_lp(torch.relu(s_hi + E), dt).double()
        else:
            # fp32: `depth` accumulations, the bias add, the multiplication with scale, the residual add
            sc, x = f32_scale(case.scale), lo["x"]
            E = gamma(depth + 3) * (x.abs() + abs(sc) * A)
            v_lo = x + torch.minimum(sc * s_lo, sc * s_hi) - E
            v_hi = x + torch.maximum(sc * s_lo, sc * s_hi) + E
            if case.relu:
                v_lo, v_hi = torch.relu(v_lo), torch.relu(v_hi)
            return round_lp(v_lo, dt), round_lp(v_hi, dt), lo, hi


# ---- comparisons ------------------------------------------------------------------------------------------------------------
def _where(bad, shape):
    i = int(bad.reshape(-1).to(torch.uint8).argmax())
    n, y, x, c = (int(v) for v in np.unravel_index(i, tuple(shape)))
    return f"first at image {n}, pixel ({y}, {x}), channel {c}"


def assert_bits(got, expect, what=""):
    """Bit equality of two storage-type tensors [N, H, W, C]; names the first failing image, pixel and channel."""
    got, expect = got.cpu().contiguous(), expect.cpu().contiguous()
    assert got.shape == expect.shape and got.dtype == expect.dtype, (what, got.shape, expect.shape, got.dtype, expect.dtype)
    bad = got.view(torch.int16) != expect.view(torch.int16)
    if bool(bad.any()):
        i = _where(bad, got.shape)
        k = int(bad.reshape(-1).to(torch.uint8).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits; {i}: got "
                             f"{float(got.reshape(-1)[k]):.8g}, expected {float(expect.reshape(-1)[k]):.8g}")


def assert_in_interval(got, lo, hi, what=""):
    """lo <= got <= hi at every element (NaN fails); names the first failing image, pixel and channel."""
    got, lo, hi = got.cpu().double(), lo.cpu().double(), hi.cpu().double()
    assert got.shape == lo.shape == hi.shape, (what, got.shape, lo.shape, hi.shape)
    bad = ~((got >= lo) & (got <= hi))
    if bool(bad.any()):
        i = _where(bad, got.shape)
        k = int(bad.reshape(-1).to(torch.uint8).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the interval; {i}: got "
                             f"{float(got.reshape(-1)[k]):.8g}, interval [{float(lo.reshape(-1)[k]):.8g}, {float(hi.reshape(-1)[k]):.8g}]")
