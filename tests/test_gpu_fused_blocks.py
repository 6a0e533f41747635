"""The fused inference blocks (csrc/block_fused.hip: fn_block17_infer, fn_block35_infer and their _warm forms) on their own,
through the C ABI, against the fp64 oracle of tests/fused_block_oracle.py.

No tolerance here is a tuned number.  The exact cases (ternary data, power-of-two scale) expect the bits of the fp64 chain;
the stage-isolation cases expect the interval derived in the oracle (one dense stage, gamma_K sum |terms|, carried exactly
through selections and monotone roundings); the one dense case per block and type expects the same interval carried through
all stages, which only finds gross faults.  tests/test_fused_block_oracle_host.py shows on the CPU that a clean fp32
implementation passes all three and that a dropped k tile, swapped taps, a non-zero halo, a missing ReLU, a shifted bias, a
swapped concat, one zeroed weight and a leaking padded row each fail the first two.

Every launch writes into a buffer of N + 1 images pre-filled with a bit pattern: image N must keep its bits, and x must be
unchanged."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from facenet_amd import _lib
from tests import fused_block_oracle as fo
from tests.fused_block_oracle import BF16, BLOCK17, BLOCK35, F16
from tests.util import bitpattern, ptr, same_bits, stream

pytestmark = pytest.mark.gpu

BLOCKS = (BLOCK17, BLOCK35)
DTS = (F16, BF16)
DT_ID = {F16: "f16", BF16: "bf16"}
CODE = {F16: _lib.FN_F16, BF16: _lib.FN_BF16}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_GUARD = "FN_FUSED_BLOCK_TEST_CHILD"


def _arr(ptrs):
    return (C.c_void_p * 3)(*ptrs)


class Device:
    """The operands of a case on the GPU, and the argument lists of the two entry points."""

    def __init__(self, case):
        self.case, self.blk = case, case.block
        self.w = {k: v.cuda() for k, v in case.w.items()}
        self.b = {k: v.float().cuda() for k, v in case.b.items()}
        self.x = case.x.cuda()

    def call(self, lib, x, y, N, warm=None, scale=None, relu=None, code=None, w=None, b=None):
        """rc of one launch.  warm: None (plain entry point) or (pointer, bytes) (the _warm entry point).  w / b: pointer
        overrides by layer name (0 = null)."""
        wp = {k: ptr(v) for k, v in self.w.items()}
        bp = {k: ptr(v) for k, v in self.b.items()}
        wp.update(w or {})
        bp.update(b or {})
        scale = self.case.scale if scale is None else scale
        relu = self.case.relu if relu is None else relu
        code = CODE[self.case.dt] if code is None else code
        tail = (scale, relu) + (tuple(warm) if warm is not None else ()) + (code, stream())
        if self.blk is BLOCK17:
            names = ("t0", "t1a", "t1b", "t1c", "up")
            fn = lib.fn_block17_infer if warm is None else lib.fn_block17_infer_warm
            return fn(x, y, N, *[wp[n] for n in names], *[bp[n] for n in names], *tail)
        n1, n3 = ("t0", "t1a", "t2a"), ("t1b", "t2b", "t2c")
        self.keep = (_arr([wp[n] for n in n1]), _arr([wp[n] for n in n3]), _arr([bp[n] for n in n1]), _arr([bp[n] for n in n3]))
        fn = lib.fn_block35_infer if warm is None else lib.fn_block35_infer_warm
        return fn(x, y, N, self.keep[0], self.keep[1], wp["up"], self.keep[2], self.keep[3], bp["up"], *tail)

    def run(self, lib, warm=None):
        """One launch over all images of the case into an (N + 1)-image buffer; checks the guard image and x; returns y[:N]."""
        N, dt = self.x.shape[0], CODE[self.case.dt]
        x0 = self.x.clone()
        y = bitpattern((N + 1,) + tuple(self.x.shape[1:]), dt)
        y0 = y.clone()
        _lib.check(self.call(lib, ptr(self.x), ptr(y), N, warm), self.case.what)
        torch.cuda.synchronize()
        assert same_bits(y[N], y0[N]), f"{self.case.what}: the launch wrote past image {N - 1}"
        assert same_bits(self.x, x0), f"{self.case.what}: the launch changed x"
        return y[:N].cpu()


# ---- exact cases: bit equality ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", fo.EXACT_RUNS, ids=lambda r: f"seed{r[0]}-N{r[1]}-scale{r[2]}-relu{r[3]}" + ("-warm" if r[4] else ""))
@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("blk", BLOCKS, ids=lambda b: b.name)
def test_exact_cases_match_the_fp64_chain_bit_for_bit(lib, blk, dt, run):
    """Ternary x and weights, integer biases, scale 0 / 1 / 0.125 / negative powers of two, relu 0 and 1, N = 1, 2, 9, 64 (once
    with warm-ahead workgroups appended) and 257 (more images than CUs), every image with its own content: every fp32 partial
    sum is an exact integer in any order, so the kernel owes the bits of the fp64 chain.  A failure names image, pixel, channel."""
    seed, N, scale, relu, warm = run
    case, fwd = fo.exact_case(blk, dt, seed, N, scale, relu)
    dev = Device(case)
    junk = torch.randn(70001, device="cuda").to(dt)                      # 140 002 bytes: ragged against every chunking
    got = dev.run(lib, (ptr(junk), 140000 // 16 * 16) if warm else None)
    fo.assert_bits(got, fwd.out, case.what)


# ---- stage isolation: the derived interval ----------------------------------------------------------------------------------
STAGES = [(blk, L.name) for blk in BLOCKS for L in blk.layers]


@pytest.mark.parametrize("relu", (0, 1))
@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("blk,stage", STAGES, ids=[f"{b.name}-{s}" for b, s in STAGES])
def test_isolated_stage_stays_inside_the_derived_interval(lib, blk, stage, dt, relu):
    """One dense random stage (weights, bias) between exact selections, production scale (0.10 / 0.17), three images: every
    output element lies in the interval tests/fused_block_oracle.py: interval_forward derives for that stage."""
    i = [L.name for L in blk.layers].index(stage)
    case = fo.isolation_case(blk, dt, stage, i, 3, relu)
    lo, hi, _, _ = fo.interval_forward(case, {stage})
    fo.assert_in_interval(Device(case).run(lib), lo, hi, case.what)


# ---- dense data in every stage: gross faults only ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("blk", BLOCKS, ids=lambda b: b.name)
def test_dense_case_stays_inside_the_propagated_bound(lib, blk, dt):
    """Dense random data in all stages at the production scale against the worst-case interval carried through every stage.
    Worth: gross faults, NaN, an overflowing intermediate -- nothing finer (see fused_block_oracle.dense_case for the CPU
    measurements: a clean emulation at 2-4 % of the bound, planted indexing faults at 5-36 %)."""
    case = fo.dense_case(blk, dt, 0, 2, 1)
    lo, hi, _, _ = fo.interval_forward(case, {L.name for L in blk.layers})
    got = Device(case).run(lib)
    assert bool(torch.isfinite(got.float()).all())
    fo.assert_in_interval(got, lo, hi, case.what)


# ---- warm-ahead entry point of Block35 --------------------------------------------------------------------------------------
def test_block35_warm_ahead_entry_point(lib):
    """fn_block35_infer_warm: the warm-ahead workgroups change no bit of the output for a ragged range, a 16-byte range and the
    block's own w_up pack; a range without a size, a size without a range, a misaligned range and a negative size are FN_EINVAL
    with nothing launched (as test_block17_warm_ahead_entry_point has it for Block17)."""
    case = fo.dense_case(BLOCK35, F16, 2, 5, 1)
    dev = Device(case)
    junk = torch.randn(70001, device="cuda").to(F16)
    ref = dev.run(lib)
    assert float(ref.float().abs().max()) > 0
    w_up = dev.w["up"]
    for warm in ((None, 0), (ptr(junk), 140000 // 16 * 16), (ptr(junk), 16), (ptr(w_up), w_up.numel() * 2)):
        fo.assert_bits(dev.run(lib, warm), ref, f"block35 warm range {warm[1]} bytes")
    for warm in ((ptr(junk), 0), (None, 64), (ptr(junk) + 2, 64), (ptr(junk), -16)):
        y = bitpattern(tuple(dev.x.shape), CODE[F16])
        y0 = y.clone()
        with pytest.raises(ValueError):
            _lib.check(dev.call(lib, ptr(dev.x), ptr(y), 5, warm))
        torch.cuda.synchronize()
        assert same_bits(y, y0)                                          # nothing was launched
        assert b"warm" in lib.fn_last_error()


# ---- bad arguments ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blk", BLOCKS, ids=lambda b: b.name)
def test_bad_arguments_are_refused_before_anything_is_launched(lib, blk):
    """x == y, a null pack, a null bias, a null entry inside a Block35 pointer array, N = 0, a negative N and an unknown dtype:
    ValueError (FN_EINVAL), y untouched, fn_last_error says what."""
    case = fo.dense_case(blk, F16, 3, 2, 1)
    dev = Device(case)
    y = bitpattern(tuple(dev.x.shape), CODE[F16])
    y0, x0 = y.clone(), dev.x.clone()
    X, Y = ptr(dev.x), ptr(y)
    bad = [("x == y", b"bad arguments", lambda: dev.call(lib, X, X, 2)),
           ("null x", b"bad arguments", lambda: dev.call(lib, None, Y, 2)),
           ("null y", b"bad arguments", lambda: dev.call(lib, X, None, 2)),
           ("null w_up", b"bad arguments", lambda: dev.call(lib, X, Y, 2, w={"up": None})),
           ("null b_up", b"bad arguments", lambda: dev.call(lib, X, Y, 2, b={"up": None})),
           ("N = 0", b"bad arguments", lambda: dev.call(lib, X, Y, 0)),
           ("N < 0", b"bad arguments", lambda: dev.call(lib, X, Y, -1)),
           ("dtype", b"dtype", lambda: dev.call(lib, X, Y, 2, code=7))]
    inner = b"bad arguments" if blk is BLOCK17 else b"null layer"        # Block35 takes these through pointer arrays
    for name in ("t0", "t1b", blk.concat[-1]):
        bad.append((f"null w {name}", inner, lambda name=name: dev.call(lib, X, Y, 2, w={name: None})))
        bad.append((f"null b {name}", inner, lambda name=name: dev.call(lib, X, Y, 2, b={name: None})))
    for what, msg, launch in bad:
        with pytest.raises(ValueError):
            _lib.check(launch(), what)
        assert msg in lib.fn_last_error(), (what, lib.fn_last_error())
        torch.cuda.synchronize()
        assert same_bits(y, y0) and same_bits(dev.x, x0), what
    _lib.check(dev.call(lib, X, Y, 2), "the same arguments, all valid")   # ... and the good call still works
    torch.cuda.synchronize()
    assert not same_bits(y, y0)


# ---- the register-ring form of Block17 stages 2-4 ---------------------------------------------------------------------------
CHILD_SELECTION = "block17 and (test_exact_cases or test_isolated_stage)"
CHILD_SELECTED = len(DTS) * len(fo.EXACT_RUNS) + len(BLOCK17.layers) * len(DTS) * 2      # 16 exact + 20 isolation tests
CHILD_SELECTION_SECONDS = 2.7           # measured: the same 36 tests in the parent process (sum of pytest --durations, MI355X host)
CHILD_TIMEOUT = max(60.0, 10 * CHILD_SELECTION_SECONDS)


@pytest.mark.skipif(os.environ.get(CHILD_GUARD) == "1", reason="this IS the child run")
def test_block17_register_ring_path_in_a_child_process():
    """FN_B17_DMA=0 selects the register-ring weight stream for Block17 stages 2-4.  The switch is read once
    into a static, so the Block17 exact and isolation tests of this file run again in ONE fresh child interpreter with the
    variable set: return code 0 and all 36 selected tests passed.  One run, no retry.

    Time limit: the same selection takes 2.7 s in the parent process (measured on an MI355X host, most of it the fp64
    reference on the CPU; the whole child, interpreter start and library load included, took 8.7 s).  Ten times the 2.7 s
    is below a minute, so the limit is the minute that covers imports and the library load."""
    env = dict(os.environ, FN_B17_DMA="0")
    env[CHILD_GUARD] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-k", CHILD_SELECTION,
                        "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, f"the FN_B17_DMA=0 run ended with {r.returncode}:\n{r.stdout[-4000:]}"
    assert f"{CHILD_SELECTED} passed" in r.stdout, r.stdout[-4000:]
