"""csrc/gemm_plan.h stands alone: tests/gemm_plan_sweep.cpp (its own main, that header and nothing else) builds with the host compiler under
AddressSanitizer + UBSan, walks the threshold grid of tests/support_gemm_grid.py without a report, and answers every query -- route or refusal,
workspace size -- exactly as the built library does through its C ABI.  No device, and no sanitizer inside this process."""
import os
import shutil
import subprocess

import pytest

from facialmmt_amd import _lib
from tests import support_gemm_cases as GC
from tests import support_gemm_grid as GG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _host_compilers():
    """every host C++ compiler found: $CXX, g++, clang++ (ROCm's, where it is not on the path)"""
    found = {}
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cxx) if cxx else None
        if path:
            found.setdefault(os.path.realpath(path), path)
    assert found, "no host C++ compiler (g++ / clang++) to build tests/gemm_plan_sweep.cpp with"
    return list(found.values())


@pytest.fixture(scope="module")
def grid():
    return GG.grid()


@pytest.fixture(scope="module", params=_host_compilers(), ids=os.path.basename)
def sweep(request, tmp_path_factory, grid):
    """the sanitized program, built with one of the host compilers, run over the grid: (exit code, stderr, answers)"""
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_sweep")
    subprocess.run([request.param, "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + SANITIZE + [os.path.join(ROOT, "tests", "gemm_plan_sweep.cpp"), "-o", exe],
                   check=True)
    text = "".join(" ".join(map(str, q)) + "\n" for q in grid)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    return run.returncode, run.stderr, [tuple(map(int, line.split())) for line in run.stdout.splitlines()]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from facialmmt_amd.build import build
        build(verbose=False)
    return GG.load(_lib.LIB_PATH)


def test_grid_sits_on_the_thresholds(grid):
    ms = {q[2] for q in grid}
    for v in (128, 256, 768, 2048, 4096, 8192, 16384, 65536, 262144):
        assert {v - 1, v, v + 1} <= ms, v
    assert {8256, 262208, 501760, 1 << 20} <= ms
    assert {q[0] for q in grid} == {0, 1, 2, 3, 4, 5} and {q[1] for q in grid} == {0, 1}
    assert {q[15] for q in grid if q[0] == 0} >= {0, 1, 2, 3, 4} and {q[16] for q in grid} >= {0, 1, 31, 32, 49}
    assert any(q[2] * q[5] == 1 << 31 for q in grid) and any(q[2] * q[5] == (1 << 31) - 8 * q[2] for q in grid)


def test_planner_runs_clean_under_sanitizers(sweep, grid):
    code, err, answers = sweep
    assert code == 0 and err == "", err[-2000:]
    assert len(answers) == len(grid)


def test_planner_answers_what_the_library_answers(sweep, grid, lib):
    _, _, answers = sweep
    assert len(answers) == len(grid)
    wrong = [(q, got, GG.ask(lib, q)) for q, got in zip(grid, answers) if got != GG.ask(lib, q)]
    assert wrong == [], (len(wrong), wrong[:5])
    # the grid reaches every route of enum fmmt_route, and refusals
    assert {a[0] for a in answers if a[0] > 0} == set(GC.route_enum().values()) and any(a[0] < 0 for a in answers)
