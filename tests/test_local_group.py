"""The in-process data-parallel group (neus2_amd/csrc/localgroup.h): tests/host/groups_main.cpp, which includes that header
alone and drives a group from one thread per rank, compiled once with the thread sanitizer and once with the address and
undefined-behaviour sanitizers and run as a child process. The program checks: worlds 1, 2 and 3 over 50 collectives
back to back (f32 sums of 1, 3 and 1000 elements, a u32 sum, an f32 max) bitwise against the sequential rank-order loop;
and a rank that misses a collective: the caller's barrier times out, its arrival is withdrawn and every later collective
fails at once on every rank. No GPU and no library: no HIP call."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [["-fsanitize=thread"], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["thread", "address-undefined"])
def test_group_program(tmp_path, sanitize):
    exe = tmp_path / "groups"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", *sanitize,
                    "-I", os.path.join(ROOT, "neus2_amd", "csrc"), os.path.join(ROOT, "tests", "host", "groups_main.cpp"),
                    "-o", str(exe)], check=True)
    # nothing of the caller's environment: no preload
    r = subprocess.run([str(exe)], env={"PATH": os.environ.get("PATH", "")}, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"exit status {r.returncode}\n{r.stdout}{r.stderr}"
    assert r.stdout.strip() == "ok", r.stdout + r.stderr
