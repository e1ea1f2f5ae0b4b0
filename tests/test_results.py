"""The result format on the host (jda_amd/csrc/results.h, with post.cpp and plan.cpp), both dialects, on seeded random
inputs: the gid decoder against a brute-force enumeration and locate(), rows written directly against rows packed from
emit()'s results, emit() with NMS off."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gid_decoder_rows_and_emit_agree(tmp_path):
    exe = str(tmp_path / "results_check")
    csrc = os.path.join(ROOT, "jda_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I" + csrc,
                           os.path.join(ROOT, "tests", "cpp", "results_check.cpp"), os.path.join(csrc, "post.cpp"),
                           os.path.join(csrc, "plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stdout + out.stderr
