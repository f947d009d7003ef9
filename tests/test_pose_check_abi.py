"""CPU suite: the rules of the caller's pose records that every pose entry shares (sac-cot_amd/csrc/sc_pose_check.hpp) and the
parameter rules of sc_polish_poses and sc_pose_info_frame, under the sanitizers, in a program of their own.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_checks_under_the_sanitizers(tmp_path):
    """Every refusal rule of the two entries with its full message and in its order, the bytes read of the pose array, and the
    three messages of the guides' stride rule: tests/native/pose_check_main.cpp, a program of its own built with
    -fsanitize=address,undefined and run on the CPU."""
    exe = str(tmp_path / "pose_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "pose_check_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "all passed" in out.stdout and "runtime error" not in out.stderr
