"""CPU suite: the rules of a frame's end (sac-cot_amd/csrc/sc_frame_check.hpp) — the verdict on a frame that has run and its
priority, what each verdict does, the estimate's hold-off and the covers of the shape's history — under the sanitizers, in a
program of their own.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_frame_rules_under_the_sanitizers(tmp_path):
    """Every way finalize_wait is left and the order between them, the packed word of a host-free frame's counts at its edges,
    every row of the verdict table with its text, the hold-offs of nine failures and their count-down, and the covers through two
    roll-overs of the window: tests/native/frame_check_main.cpp, a program of its own built with -fsanitize=address,undefined and
    run on the CPU.  Its expected values are written out by hand."""
    exe = str(tmp_path / "frame_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "frame_check_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "all passed" in out.stdout and "runtime error" not in out.stderr
