"""csrc/hificar_host_util.h on its own (no GPU, no library): tests/host_util_main.cpp — its own ``main``, the header and a stub for ``fail`` —
built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer, and run.  The program checks Carver (a null and a real
base give the same total; granule-aligned, increasing, non-overlapping pointers; zero-byte and skipped takes; the offset form), WeightIntake
(both refusals leave the staged set alone; a second set replaces; first_missing in map order; expected survives clear_staged), TapTable
(set, forget one, forget all; a capacity one float short is refused, the exact capacity passes) and check_workspace."""

import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_util_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (CXX, c++, g++, clang++)"
    exe = tmp_path / "host_util_main"
    build = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(REPO, "articulatory_amd", "csrc"), os.path.join(REPO, "tests", "host_util_main.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "host_util: ok" and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
