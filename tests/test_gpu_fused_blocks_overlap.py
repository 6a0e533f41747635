"""The fused inference blocks (csrc/block_fused.hip) keep loads in flight across stage boundaries and reuse LDS regions as soon
as their last reader is done: bias, residual and weight-slab requests are made a stage (or a pass) ahead of their use.  The faults
such overlap can introduce are races and stale reads, which one launch of one exact case may miss, and prefetches that reach
past the image they belong to.  Two checks, through the C ABI, with the oracle of tests/fused_block_oracle.py:

* repeat-launch determinism: eight launches of one dense production-scale case into fresh bit-patterned buffers give the
  same bits eight times, and the first lies inside the interval the oracle carries through all stages (the bound of
  test_gpu_fused_blocks.py: test_dense_case_stays_inside_the_propagated_bound, derived, not tuned);
* neighbour independence: an exact case whose x and y sit inside larger allocations filled with NaN bit patterns still equals
  the fp64 chain bit for bit, and the surrounding bytes keep their bits.  Nothing is provoked: a descriptor-bounded load past
  the image returns zeros, a prefetch that read a neighbouring row instead would carry a NaN into the result."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from facenet_amd import _lib
from tests import fused_block_oracle as fo
from tests.test_gpu_fused_blocks import CHILD_GUARD, CODE, DT_ID, DTS, ROOT, BLOCKS, Device
from tests.util import bitpattern, ptr, same_bits

pytestmark = pytest.mark.gpu

LAUNCHES = 8
# (N, warm): three images; 64 with warm-ahead workgroups appended; 257 = more images than CUs, a second round of workgroups
SHAPES = ((3, False), (64, True), (257, False))


@functools.lru_cache(maxsize=None)
def _dense(blk_name, dt, N, relu):
    """The dense case and its propagated interval, computed once per (block, type, N, relu) and left unchanged."""
    blk = fo.BLOCKS[blk_name]
    case = fo.dense_case(blk, dt, 10 + N, N, relu)
    lo, hi, _, _ = fo.interval_forward(case, {L.name for L in blk.layers})
    return case, lo, hi


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"N{s[0]}" + ("-warm" if s[1] else ""))
@pytest.mark.parametrize("relu", (0, 1))
@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("blk", BLOCKS, ids=lambda b: b.name)
def test_repeat_launches_give_the_same_bits(lib, blk, dt, relu, shape):
    """Eight launches of a dense random case at production scale, each into a fresh bit-patterned (N + 1)-image buffer: all
    eight outputs are bit-equal to the first, the first lies inside the propagated interval, image N keeps its pattern and x
    its bits (Device.run checks both on every launch)."""
    N, warm = shape
    case, lo, hi = _dense(blk.name, dt, N, relu)
    dev = Device(case)
    junk = torch.randn(70001, device="cuda").to(dt)
    first = None
    for k in range(LAUNCHES):
        got = dev.run(lib, (ptr(junk), 140000 // 16 * 16) if warm else None)
        if first is None:
            first = got
            assert bool(torch.isfinite(first.float()).all())
            fo.assert_in_interval(first, lo, hi, case.what)
        else:
            fo.assert_bits(got, first, f"{case.what}: launch {k} against launch 0")


NAN_BITS = -1          # 0xFFFF: a NaN in f16 and in bf16
NEIGHBOUR_RUNS = ((0, 2, 0.125, 1), (2, 9, -0.25, 0), (5, 64, 1.0, 1))          # (seed, N, scale, relu) of fo.EXACT_RUNS


@pytest.mark.parametrize("run", NEIGHBOUR_RUNS, ids=lambda r: f"seed{r[0]}-N{r[1]}-scale{r[2]}-relu{r[3]}")
@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("blk", BLOCKS, ids=lambda b: b.name)
def test_result_does_not_depend_on_what_lies_next_to_the_images(lib, blk, dt, run):
    """x is images 1 .. N of an (N + 2)-image allocation whose first and last image are NaN bit patterns, y likewise (its
    interior a finite bit pattern): the result equals the fp64 chain bit for bit, and both allocations keep every bit outside
    y's interior."""
    seed, N, scale, relu = run
    case, fwd = fo.exact_case(blk, dt, seed, N, scale, relu)
    dev = Device(case)
    shape = tuple(case.x.shape[1:])
    X = torch.full((N + 2,) + shape, NAN_BITS, dtype=torch.int16, device="cuda").view(dt)
    Y = torch.full((N + 2,) + shape, NAN_BITS, dtype=torch.int16, device="cuda").view(dt)
    X[1:N + 1] = dev.x
    Y[1:N + 1] = bitpattern((N,) + shape, CODE[dt])
    assert bool(torch.isnan(X[0].float()).all()) and bool(torch.isnan(Y[N + 1].float()).all())
    X0, Y0 = X.clone(), Y.clone()
    _lib.check(dev.call(lib, ptr(X[1:]), ptr(Y[1:]), N), case.what)
    torch.cuda.synchronize()
    assert same_bits(X, X0), f"{case.what}: the launch changed x or its surroundings"
    assert same_bits(Y[0], Y0[0]) and same_bits(Y[N + 1], Y0[N + 1]), f"{case.what}: the launch wrote outside its N images"
    fo.assert_bits(Y[1:N + 1].cpu(), fwd.out, case.what)


# ---- the register-ring form of Block17 stages 2-4 ---------------------------------------------------------------------------
CHILD_SELECTION = "block17 and test_repeat_launches"
CHILD_SELECTED = len(DTS) * 2 * len(SHAPES)              # 12 tests
CHILD_TIMEOUT = 120.0      # the same twelve tests take a few seconds in this process; the limit covers imports and the library load


@pytest.mark.skipif(os.environ.get(CHILD_GUARD) == "1", reason="this IS the child run")
def test_block17_register_ring_path_repeats_in_a_child_process():
    """FN_B17_DMA=0 is read once into a static, so the Block17 determinism tests run again in ONE fresh child interpreter with
    the variable set (as test_gpu_fused_blocks.py does for its exact and isolation tests): return code 0, all twelve passed."""
    env = dict(os.environ, FN_B17_DMA="0")
    env[CHILD_GUARD] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-k", CHILD_SELECTION,
                        "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, f"the FN_B17_DMA=0 run ended with {r.returncode}:\n{r.stdout[-4000:]}"
    assert f"{CHILD_SELECTED} passed" in r.stdout, r.stdout[-4000:]
