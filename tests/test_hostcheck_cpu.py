"""CPU: tools/hostcheck/step_outputs_check.hip -- the arena and mirror arithmetic and the pure host checks of csrc/rec_state.h (mode
exclusions, slot lists, fans, prompt-store ranges) -- built as a stand-alone program with the address and undefined-behaviour sanitizers
on its host code, by the command of its header comment, and run: exit status 0 and the `ok` line. Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join("tools", "hostcheck", "step_outputs_check.hip")
FLAGS = "--offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Xarch_host -fsanitize=address,undefined"


def test_hostcheck_program_is_clean_under_the_host_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with open(os.path.join(ROOT, SRC)) as f:
        head = " ".join(line.strip("/ \\\n") for line in f.read().split("#include")[0].splitlines())
    assert f"hipcc {FLAGS} {SRC}" in head                                       # the command below is the one the program documents
    exe = str(tmp_path / "step_outputs_check")
    subprocess.run([hipcc, *FLAGS.split(), SRC, "-o", exe], cwd=ROOT, check=True, timeout=600)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "step_outputs_check: ok" in run.stdout.splitlines()
