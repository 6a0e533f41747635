"""The developer-only phase-clock switch of csrc/block_fused.hip (-DFN_FUSED_PHASES=1, tools/dev_fused_blocks.py) on the host:
the translation unit compiles for gfx950 with and without it, and the default object carries nothing of it -- neither the
debug entry point fn_debug_fused_phases nor the device array fn_fused_phase it reads.

The two compilations run side by side (a few seconds each); no GPU is needed, hipcc cross-compiles."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "facenet_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-unused-variable"]     # csrc/Makefile
NAMES = (b"fn_debug_fused_phases", b"fn_fused_phase")


def test_phase_switch_compiles_and_is_absent_from_the_default_object(tmp_path):
    objs = {"default": (tmp_path / "default.o", []), "phases": (tmp_path / "phases.o", ["-DFN_FUSED_PHASES=1"])}
    procs = {k: subprocess.Popen([HIPCC, *FLAGS, *extra, "-c", "block_fused.hip", "-o", str(out)], cwd=CSRC,
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for k, (out, extra) in objs.items()}
    for k, p in procs.items():
        log = p.communicate(timeout=600)[0]
        assert p.returncode == 0, f"{k} build of block_fused.hip failed:\n{log[-4000:]}"
    default, phases = (objs[k][0].read_bytes() for k in ("default", "phases"))
    for name in NAMES:
        assert name in phases, f"the phase build lacks {name.decode()}"
        assert name not in default, f"the default object mentions {name.decode()}: the switch does not compile out"
    # the four public entry points are in both
    for name in (b"fn_block17_infer", b"fn_block17_infer_warm", b"fn_block35_infer", b"fn_block35_infer_warm"):
        assert name in default and name in phases, name
