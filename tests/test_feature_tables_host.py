"""The list of per-feature tables, the compaction plan and the row gather (openekfmonoslam_amd/csrc/feature_tables.h), CPU only:
tests/cpp/feature_tables_check.cpp checks the plan against a row-ownership reference over every type mix and drop subset up to 7
features (and a seeded map of 200), the gather against a copy-out reference in buffers of exactly N rows, and the list against the
blob layout of map_blob.h, under AddressSanitizer and UBSan, in a process of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_feature_tables_plan_gather_and_list(tmp_path):
    exe = str(tmp_path / "feature_tables_check")
    # no HIP is needed or linked.  The sanitizer runtimes are linked into the program, so it runs the same whatever else the
    # environment loads into a process.
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-g", "-o", exe, os.path.join(ROOT, "tests", "cpp", "feature_tables_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "feature_tables_check: ok" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
