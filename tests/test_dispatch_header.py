"""gigl_amd/csrc/dispatch.h (run-time value -> compile-time tag, what every launch site picks its kernel instantiation
with) checked on the CPU: tests/c/dispatch_check.cpp includes only that header, is compiled with g++ -std=c++17 and
asserts that each listed value reaches its own tag, an unlisted one the last tag, f runs once and its result returns."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatch_header_on_the_cpu(tmp_path):
    exe = str(tmp_path / "dispatch_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "gigl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "dispatch_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "dispatch OK" in out.stdout
