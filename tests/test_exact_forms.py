"""The short forms of the correctly rounded division and square root (rt_exact.hpp: the quotient triple with one
Markstein correction, the root chosen among its seed's neighbours, normalize under one guard, the branch-free
reciprocal), compiled with g++ -ffp-contract=off and run on the CPU against `/` and sqrtf bit for bit
(tests/c/exact_forms_test.cpp): 10^8 random operands per operation inside the guard ranges and across both of their
edges, mantissas biased towards all-zeros and all-ones, and structured operands -- those mantissas +-1, numerators +-0,
denormals, infinities, NaNs, denominators at the guards' ends and of either sign; the root with its seed moved by -1,
0 and +1 ulp. No GPU: tests/test_gpu_exact_forms.py checks the device forms (v_rcp_f32, v_sqrt_f32) exhaustively."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exact_forms(tmp_path):
    exe = tmp_path / "exact_forms_test"
    src = os.path.join(ROOT, "tests", "c", "exact_forms_test.cpp")
    inc = os.path.join(ROOT, "parallel-ray-tracer_amd", "csrc", "hip")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-pthread",
                    "-I", inc, "-o", str(exe), src], check=True)
    r = subprocess.run([str(exe), "100"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches: div3 0 root 0 normalize 0 rcp_small 0" in r.stdout, r.stdout
    assert "all checks passed" in r.stdout
