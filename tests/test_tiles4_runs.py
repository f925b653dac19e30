"""mn_tile_runs.h -- where the run of a pixel starts, from the 64-bit link mask of its tile row: the arithmetic of the
rows of mn_cc_tiles4 (one start from the mask per lane, the other three from the lane's link nibble).

tests/tools/tile_runs_check.cpp includes the header, has its own main and is compiled by g++ alone with the address
and undefined-behaviour sanitizers; it holds every column and every lane position to a loop that walks left pixel by
pixel, on the all-zero and all-one masks, every single-bit mask and its complement and 16384 random masks of four
densities.  It runs as a child process: nothing is loaded into this one.  CPU only.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_starts_against_a_naive_loop(tmp_path):
    exe = str(tmp_path / "tile_runs_check")
    src = os.path.join(ROOT, "tests", "tools", "tile_runs_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover", src, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip() == "tile runs ok: %d masks" % (3 + 2 * 64 + 4 * 4096), res.stdout + res.stderr
