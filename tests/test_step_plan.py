"""The shape of a training step (neus2_amd/csrc/step_plan.h): tests/host/step_plan_main.cpp, which includes that header
alone, compiled with the address and undefined-behaviour sanitizers and run as a child process. The program checks
plan_step field by field against the rules as the training step spelled them out before they moved into the header
(the two cuts, the occupancy and readback cadence, the progressive rule, the lookahead's conditions and its plan for the
next step, risky, split, scan_group, xo, a_over, canon_opt), the invariants the comments promise (no cut on a step the
host reads back; the march cut's distance from call ends, readbacks and occupancy updates; a lookahead's plan for the next
step equal to the plan that step would make for itself), and the chunk-end rule with ChunkSchedule::set's validation.

The sweep is the full product of steps 0..527, 0..3 steps left, the 9 mode / keep-ratio pairs, 1 / 2 / 3 / 14 chunk ends,
prog_cut, march_cut, ray_sort, fixed_rays, dyn, profiling, balanced, force_full, 4 / 8 lanes and two cone angles, and
the same over three schedules whose cut ends differ from their ends (the auto rule's with two and three rounds; cut ends
beside no ends, below the bound of the cut's round count). The six
inputs that only the lookahead's conjunction reads are crossed with it at steps 0..40 and 250..290 only, and the inputs of
the remaining fields at steps 254..274; those two passes keep 8 of the schedules (the program's header says which and
why): the whole product there is 2 G points, minutes under the sanitizers. Built with -O2 for the same reason.
No GPU and no library: no HIP call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_plan_program(tmp_path):
    exe = tmp_path / "step_plan"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "neus2_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "step_plan_main.cpp"), "-o", str(exe)], check=True)
    # nothing of the caller's environment: no preload
    r = subprocess.run([str(exe)], env={"PATH": os.environ.get("PATH", "")}, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"exit status {r.returncode}\n{r.stdout}{r.stderr}"
    assert r.stdout.strip() == "ok", r.stdout + r.stderr
