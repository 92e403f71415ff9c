"""The digit word of the exact downdate as a double (openekfmonoslam_amd/csrc/digit_planes.h: px_word_value, what k_dx_planes converts
every element of B with), CPU only: tests/cpp/digit_word_check.cpp compares it bit for bit with the 64-bit integer path for every top
byte crossed with corner and seeded random low words, and the round trip through px_digit_word; it runs under UBSan in a process of
its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_digit_word_value_against_the_integer_path(tmp_path):
    exe = str(tmp_path / "digit_word_check")
    # no HIP: without hipcc the header is plain C++.  The sanitizer runtime is linked into the program.
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-static-libubsan",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "digit_word_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "digit_word_check: ok" in r.stdout
    assert "runtime error" not in r.stderr, r.stderr
