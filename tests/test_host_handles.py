"""The owning handle of the host units (neus2_amd/csrc/handle.h): tests/host/handles_main.cpp, which includes that header
alone and instantiates it with a counting destroyer, compiled with the address and undefined-behaviour sanitizers and run
as a child process. The program checks: an empty handle, an adopted value, move construction, move assignment onto a
live handle, self-move, reset twice, release, a value-initialised [2][11] array, a vector grown past its capacity, and,
by static_assert, that the handle does not copy and moves without throwing. No GPU and no library: no HIP call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_handle_program(tmp_path):
    exe = tmp_path / "handles"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "neus2_amd", "csrc"), os.path.join(ROOT, "tests", "host", "handles_main.cpp"),
                    "-o", str(exe)], check=True)
    # nothing of the caller's environment: no preload
    r = subprocess.run([str(exe)], env={"PATH": os.environ.get("PATH", "")}, capture_output=True, text=True)
    assert r.returncode == 0, f"exit status {r.returncode}\n{r.stdout}{r.stderr}"
    assert r.stdout.strip() == "ok", r.stdout + r.stderr
