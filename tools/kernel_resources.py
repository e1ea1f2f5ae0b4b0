"""kernel_resources(kernel_file, kernel_name): the compile-time resource figures of one kernel of jda_amd/csrc -- VGPRs, AGPRs,
SGPRs, scratch, LDS per block, waves per SIMD -- from the library's own flags and -Rpass-analysis=kernel-resource-usage.  No
GPU needed.  The `--resources FILE` option of pack_bench.py, turn_bench.py and chips_bench.py writes them next to the timings."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_resources(kernel_file, kernel_name):
    from jda_amd import build as lib_build
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([lib_build.hipcc()] + lib_build.CFLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(lib_build.CSRC, kernel_file),
                            "-o", os.path.join(d, kernel_name + ".o")], capture_output=True, text=True, check=True)
    got = {}
    for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                     ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)")):
        got[key] = int(re.search(pat, r.stderr).group(1))
    assert kernel_name in r.stderr and got["scratch_bytes_per_lane"] == 0, r.stderr
    return got
