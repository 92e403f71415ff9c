"""The route of an EKF update (openekfmonoslam_amd/csrc/update_route.h: choose_update_route, choose_pair_step, persist_layout), CPU
only: tests/cpp/update_route_check.cpp holds the expected routes, written out by hand, at both sides of every boundary; it runs under
AddressSanitizer and UBSan in a process of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_update_route_against_the_table(tmp_path):
    exe = str(tmp_path / "update_route_check")
    # no HIP: the header is plain C++.  The sanitizer runtimes are linked into the program, so it runs the same whatever else the
    # environment loads into a process.
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-g", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "update_route_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "update_route_check: ok" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
