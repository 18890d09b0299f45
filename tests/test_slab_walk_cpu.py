"""The slab walk of the cache row movers (kivi_amd/csrc/kivi_slab.h) on the host, under AddressSanitizer and UBSan.

tests/slab_walk_main.cpp is a stand-alone program: it includes the header the kernels include, prepares slab lists over host buffers
with kivi_prepare_slabs and walks the grid of the two-sided copy kernel (every chunk, row, thread and unit in flight) with
KIVI_SLAB_OF_CHUNK / kivi_slab_offsets, one memcpy per unit.  It compares with a nested-loop copy of the same slabs and counts the
writes of every destination byte: 16-byte and 4-byte units; a flat slab, a 3-level slab with other strides per side, exactly one full
chunk, a full chunk plus one unit, a single unit, empty slabs between live ones; two caller sides (admit) and the dense buffer side
in both directions (snapshot).  The program runs as a child process of its own; nothing is loaded into this interpreter.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slab_walk_matches_a_nested_loop_copy_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "slab_walk")
    # the sanitizer runtimes are linked into the program (clang's default), so it does not depend on the order libraries load in
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static, "-o", exe, os.path.join(ROOT, "tests", "slab_walk_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "slab walk ok" and run.stderr == "", run.stdout + run.stderr
