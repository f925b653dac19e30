"""mn_memory.h -- the registry that owns a context's memory, and the carver that lays arrays out in one block -- on
the HOST, with allocators that know every live pointer and fail on demand (tests/tools/memory_check.cpp, a program of
its own).  The program runs the library's lifetimes (base, record and first-use groups; the record lists swapped for
larger ones; a carved workspace grown twice; batch arrays grown; everything freed) once clean and once for every k with
the k-th allocation failing, and after each failure holds the registry to: counted bytes = live counted buffers, every
field of a freed group null, a group whole or absent, the capacities describing what is there, every buffer released
exactly once and nothing live at the end.  Its carver case: three arrays whose sizes are no multiples of the alignment.

CPU only.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "memory_check.cpp")


def test_registry_and_carver_hold_their_invariants_under_every_single_failure(tmp_path):
    exe = str(tmp_path / "memory_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.startswith("ok: clean run of 19 allocations, 19 runs with one failing"), res.stdout + res.stderr
