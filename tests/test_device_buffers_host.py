"""The owner of an engine's device allocations (openekfmonoslam_amd/csrc/device_buffers.h), CPU only: tests/cpp/
device_buffers_check.cpp drives it with a counting allocator that fails the k-th allocation, under AddressSanitizer (whose
leak check must stay silent) and UBSan, in a process of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_buffers_against_a_counting_allocator(tmp_path):
    exe = str(tmp_path / "device_buffers_check")
    # no HIP is linked: the header needs hipError_t alone.  The sanitizer runtimes are linked into the program, so it runs
    # the same whatever else the environment loads into a process.
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-g", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "device_buffers_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device_buffers_check: ok" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
