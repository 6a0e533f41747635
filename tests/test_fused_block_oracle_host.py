"""The instruments of tests/test_gpu_fused_blocks.py, proven on the CPU before they are pointed at a kernel.

An fp32 torch emulation of each fused block stands in for the kernel.  It sums in another order than the oracle (k tiles of
32 channels outermost and reversed, taps reversed), stores the tower activations in the storage type, and can carry one
planted fault.  The clean emulation must pass every exact case bit for bit, every isolation interval and the dense bound;
every planted fault must be reported by the exact cases and by the isolation case of the stage it sits in."""
import pytest
import torch

from tests import fused_block_oracle as fo
from tests.fused_block_oracle import BF16, BLOCK17, BLOCK35, F16
from tests.util import conv_fp64

BLOCKS = (BLOCK17, BLOCK35)
DTS = (F16, BF16)
IDS = {F16: "f16", BF16: "bf16"}


# ---- the stand-in for the kernel --------------------------------------------------------------------------------------------
def _conv32(x, w, L, fault):
    """fp32 zero-padded convolution, k tiles outermost.  fault: None or (kind, ...) applying to THIS layer."""
    N, H, W, _ = x.shape
    w3 = w.reshape(L.cout, L.taps, L.cin).clone()
    ph, pw = L.kh // 2, L.kw // 2
    xp = x.new_zeros(N, H + 2 * ph, W + 2 * pw, L.cin)
    xp[:, ph:ph + H, pw:pw + W] = x
    kind = fault[0] if fault else None
    if kind == "halo":                      # one border column (row for the 7x1) replicates its neighbour instead of being zero
        if pw:
            xp[:, :, pw - 1] = xp[:, :, pw]
        else:
            xp[:, ph - 1] = xp[:, ph]
    elif kind == "leak":                    # Block35: pixel rows 289..303 of the padded M extent land in the bottom halo row
        assert L.taps == 9 and H == 17
        xp[:, H + 1, 1:16] = 1.0
    elif kind == "swap_taps":
        t0, t1 = fault[1]
        w3[:, [t0, t1]] = w3[:, [t1, t0]]
    elif kind == "zero_weight":             # the first non-zero weight at the centre tap (every case reads that tap)
        c = L.taps // 2
        o, i = (w3[:, c] != 0).nonzero()[0].tolist()
        w3[o, c, i] = 0.0
    out = x.new_zeros(N, H, W, L.cout)
    for kt in reversed(range(L.cin // 32)):
        ks = slice(kt * 32, kt * 32 + 32)
        for t in reversed(range(L.taps)):
            if kind == "drop_ktile" and (t, kt) == (L.taps // 2, fault[1]):
                continue
            ky, kx = divmod(t, L.kw)
            out += xp[:, ky:ky + H, kx:kx + W, ks] @ w3[:, t, ks].T
    return out


def emulate(case, fault=None):
    """fault = (kind, layer, ...).  Kinds: drop_ktile (layer, k tile at the centre tap), swap_taps (layer, (t0, t1)), halo, leak,
    no_relu, bias_shift, zero_weight (layer), concat_swap ("up")."""
    blk, dt = case.block, case.dt
    acts = {"x": case.x.float()}
    for L in blk.layers:
        f = fault[:1] + fault[2:] if fault and fault[1] == L.name else None
        kind = f[0] if f else None
        if L.src == "mixed":
            names = list(blk.concat)
            if kind == "concat_swap":
                names[0], names[-1] = names[-1], names[0]
            src = torch.cat([acts[n] for n in names], -1)
        else:
            src = acts[L.src]
        s = _conv32(src, case.w[L.name].float(), L, f)
        b = case.b[L.name].float()
        if kind == "bias_shift":
            b = torch.roll(b, -1)
        if L is not blk.up:
            v = s + b
            acts[L.name] = (v if kind == "no_relu" else torch.relu(v)).to(dt).float()
        else:
            v = acts["x"] + torch.tensor(case.scale, dtype=torch.float32) * (s + b)
            return (torch.relu(v) if case.relu else v).to(dt)


# ---- the clean emulation passes everything ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=IDS.get)
@pytest.mark.parametrize("blk", BLOCKS, ids=lambda b: b.name)
def test_clean_emulation_passes_every_exact_case(blk, dt):
    """Also: the exactness premise and the non-vacuity checks hold for every seed the GPU test uses (exact_case raises
    otherwise), with the margins printed."""
    for seed, N, scale, relu, _ in fo.EXACT_RUNS:
        case, fwd = fo.exact_case(blk, dt, seed, N, scale, relu)
        peak = max(float(v.abs().max()) for v in fwd.pre.values())
        fill = min(float((fwd.acts[L.name] != 0).double().mean()) for L in blk.towers)
        print(f"{case.what}: largest |sum + bias| {peak:g} of {fo.EXACT_LIMIT[dt]}, least non-zero fraction of a tower {fill:.2f}")
        fo.assert_bits(emulate(case), fwd.out, case.what)


@pytest.mark.parametrize("relu", (0, 1))
@pytest.mark.parametrize("dt", DTS, ids=IDS.get)
@pytest.mark.parametrize("blk", BLOCKS, ids=lambda b: b.name)
def test_clean_emulation_stays_inside_every_isolation_interval(blk, dt, relu):
    for i, L in enumerate(blk.layers):
        case = fo.isolation_case(blk, dt, L.name, i, 2, relu)
        lo, hi, _, _ = fo.interval_forward(case, {L.name})
        fo.assert_in_interval(emulate(case), lo, hi, case.what)
        # the oracle's own value lies inside its interval
        ref = fo.forward(case).out
        fo.assert_in_interval(ref, lo, hi, case.what + " (fp64 chain)")


@pytest.mark.parametrize("dt", DTS, ids=IDS.get)
@pytest.mark.parametrize("blk", BLOCKS, ids=lambda b: b.name)
def test_clean_emulation_stays_inside_the_dense_bound(blk, dt):
    case = fo.dense_case(blk, dt, 0, 2, 1)
    lo, hi, _, _ = fo.interval_forward(case, {L.name for L in blk.layers})
    fo.assert_in_interval(emulate(case), lo, hi, case.what)


def test_an_interval_needs_exact_selections_around_the_dense_stage():
    case = fo.dense_case(BLOCK35, F16, 0, 1, 1)
    with pytest.raises(ValueError, match="exact selection"):
        fo.interval_forward(case, {"t0"})


def test_exact_case_rejects_inputs_that_break_the_premise(monkeypatch):
    dense = dict(fo.EXACT_DENSITY[("block35", BF16)], t2c=1 / 2, up=1 / 2)
    monkeypatch.setitem(fo.EXACT_DENSITY, ("block35", BF16), dense)
    with pytest.raises(ValueError, match="not below 256"):
        fo.exact_case(BLOCK35, BF16, 0, 1, 0.125, 1)
    monkeypatch.setitem(fo.EXACT_DENSITY, ("block35", BF16), dict(dense, t2c=1 / 32, up=1 / 32, t1b=1 / 4096))
    with pytest.raises(ValueError, match="non-zero"):
        fo.exact_case(BLOCK35, BF16, 0, 1, 0.125, 1)
    with pytest.raises(ValueError, match="power of two"):
        fo.exact_case(BLOCK35, BF16, 0, 1, 0.17, 1)


# ---- every planted fault is found -------------------------------------------------------------------------------------------
def _faults(blk):
    """(fault, the stage it sits in)."""
    out = []
    for L in blk.layers:                                    # a dropped 32-channel k tile in each stage
        out.append((("drop_ktile", L.name, L.cin // 32 - 1), L.name))
    conv = "t1b"                                            # 1x7 (Block17) / first 3x3 (Block35)
    out.append((("swap_taps", conv, (1, 5)), conv))
    out.append((("halo", conv), conv))
    last = blk.concat[-1]                                   # 7x1 (Block17) / last 3x3 (Block35)
    out.append((("swap_taps", last, (0, blk.layer(last).taps - 1)), last))
    out.append((("halo", last), last))
    out.append((("no_relu", "t0"), "t0"))
    out.append((("no_relu", last), last))
    for name in ("t0", conv, "up"):
        out.append((("bias_shift", name), name))
        out.append((("zero_weight", name), name))
    out.append((("concat_swap", "up"), "up"))
    if blk is BLOCK35:
        for name in ("t1b", "t2b", "t2c"):
            out.append((("leak", name), name))
    return out


FAULTS = [(blk, f, stage) for blk in BLOCKS for f, stage in _faults(blk)]
FAULT_IDS = [f"{blk.name}-{'-'.join(str(v) for v in f)}".replace(" ", "") for blk, f, _ in FAULTS]


@pytest.mark.parametrize("dt", DTS, ids=IDS.get)
@pytest.mark.parametrize("blk,fault,stage", FAULTS, ids=FAULT_IDS)
def test_planted_fault_is_found_by_the_exact_cases(blk, fault, stage, dt):
    """One small exact case per `relu` is enough for every fault; the GPU test runs all of EXACT_RUNS."""
    for seed, N, scale, relu, _ in fo.EXACT_RUNS[:2]:
        case, fwd = fo.exact_case(blk, dt, seed, N, scale, relu)
        with pytest.raises(AssertionError, match="differ in their bits"):
            fo.assert_bits(emulate(case, fault), fwd.out, case.what)


@pytest.mark.parametrize("dt", DTS, ids=IDS.get)
@pytest.mark.parametrize("blk,fault,stage", FAULTS, ids=FAULT_IDS)
def test_planted_fault_is_found_by_the_isolation_case_of_its_stage(blk, fault, stage, dt):
    i = [L.name for L in blk.layers].index(stage)
    for relu in (0, 1):
        case = fo.isolation_case(blk, dt, stage, i, 2, relu)
        lo, hi, _, _ = fo.interval_forward(case, {stage})
        with pytest.raises(AssertionError, match="outside the interval"):
            fo.assert_in_interval(emulate(case, fault), lo, hi, case.what)


# ---- the oracle agrees with the project's fp64 convolution reference ------------------------------------------------------------
def _conv_fp64_layer(case, L, src):
    w = case.w[L.name].double().reshape(L.cout, L.kh, L.kw, L.cin)
    s, a = conv_fp64(src, w, 1, L.kh // 2, L.kw // 2)
    return s + case.b[L.name].double(), a + case.b[L.name].double().abs()


@pytest.mark.parametrize("dt", DTS, ids=IDS.get)
@pytest.mark.parametrize("blk", BLOCKS, ids=lambda b: b.name)
def test_oracle_agrees_with_conv_fp64_composed_layer_by_layer(blk, dt):
    """tests/util.py: conv_fp64 (torch conv2d on OHWI weights, its own padding) composed into the whole block.  On an exact case
    every sum is an integer whatever the order, so the two chains must agree exactly: intermediates, sums of absolute terms,
    the stored output."""
    case, fwd = fo.exact_case(blk, dt, 0, 2, 0.125, 0)
    acts = {"x": case.x.double()}
    for L in blk.layers:
        src = torch.cat([acts[n] for n in blk.concat], -1) if L.src == "mixed" else acts[L.src]
        s, a = _conv_fp64_layer(case, L, src)
        assert torch.equal(s, fwd.pre[L.name]) and torch.equal(a, fwd.absum[L.name]), L.name
        if L is not blk.up:
            acts[L.name] = torch.relu(s).to(torch.float32).to(dt).double()
            assert torch.equal(acts[L.name], fwd.acts[L.name]), L.name
    out = (case.x.double() + fo.f32_scale(case.scale) * s).to(torch.float32).to(dt)
    fo.assert_bits(out, fwd.out, case.what)


@pytest.mark.parametrize("dt", DTS, ids=IDS.get)
@pytest.mark.parametrize("blk", BLOCKS, ids=lambda b: b.name)
def test_oracle_layers_agree_with_conv_fp64_on_dense_data(blk, dt):
    """Each layer on the oracle's own stored input, dense random data: equal up to the fp64 summation order."""
    case = fo.dense_case(blk, dt, 1, 2, 0)
    fwd = fo.forward(case)
    for L in blk.layers:
        src = torch.cat([fwd.acts[n] for n in blk.concat], -1) if L.src == "mixed" else fwd.acts[L.src]
        s, a = _conv_fp64_layer(case, L, src)
        assert float(((s - fwd.pre[L.name]).abs() / a).max()) <= L.depth * 2.0 ** -52, L.name
        assert float(((a - fwd.absum[L.name]).abs() / a).max()) <= L.depth * 2.0 ** -52, L.name
