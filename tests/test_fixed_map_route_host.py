"""The route of a fixed-map update (openekfmonoslam_amd/csrc/update_route.h, UpdateRouteIn::fixed_map), CPU
only: tests/cpp/fixed_map_route_check.cpp holds the expected routes at 2048 and 2080 padded rows for the fp64 and the two exact
configurations (no digit planes, no GEMM on them), the refusals (sharded, fp32 rows of B), and that the input's default leaves a
sample of the existing table's routes identical.  It runs under AddressSanitizer and UBSan in a process of its own, built as
tests/test_update_route_host.py builds its program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixed_map_route_against_the_table(tmp_path):
    exe = str(tmp_path / "fixed_map_route_check")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-g", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "fixed_map_route_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fixed_map_route_check: ok" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
